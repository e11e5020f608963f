"""GPU tests of the line scans at the launch shapes the rest of the suite does not reach on purpose: two tiles per workgroup (the
slot index and thread 0's tile-by-tile walk of lines_scan_body.hpp's sum pass, `lt.at` carried from a workgroup's first tile into its
second in line_tile_done), the borders between lines_chunk_kernel's chunks of 256 parts, and runs of more than one chunk per thread
of lines_combine_kernel (more than 1,024 chunks: records above 2^33).  One searcher of the inverted library and one haystack serve
all twelve (how, inverted) combinations.

The haystacks are one filler byte with scenes planted at the borders (tests/_lines_sparse.py); the reference is worked out from the
scene list alone, which tests/test_lines_sparse_cpu.py holds against the dense rules - except at 8 MiB, where the dense rules
themselves are the reference.  Every comparison is of integers and exact; every output array is a window of a larger one whose
sentinels on both sides must survive."""
import numpy as np
import pytest

from _lines_sparse import (BORDER_KINDS, FILLER, HOWS as HOW_NAMES, KINDS, NL, Grid, background_scenes, border_scenes, checked, sparse_lines,
                           two_tile_scenes, write_scenes)
from test_gpu_bounded import SENT, TILE, Window
from test_gpu_inverted import HOWS, inverted_lib, make, ref_inverted
from test_gpu_matches import kernel_of, n_tiles, tiles_per_workgroup

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NEEDLE = b"qzjx"                                            # verified in registers
LONG = b"quite a long needle, 33 bytes: qz"                 # verified in memory
MODE2 = ((b"xyz" * 20)[:50], (1, 35, 35))                   # tests/test_gpu_matches.py's test_two_tile_workgroups_mode2: 34 apart, d = 2
COMBOS = [(how, inverted) for how in HOW_NAMES for inverted in (False, True)]
CHUNK = 256                                                 # parts per chunk of lines_chunk_kernel
THREADS = 1024                                              # threads of lines_combine_kernel


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with inverted_lib(m):
        pass
    return m


# ---- the launch shape, restated from the library --------------------------------------------------------------------------------
class Shape:
    """what plan_lines (ss_lines.hip) makes of a view of n_bytes at a 16-byte-aligned address: tiles, tiles per workgroup, parts
    (the workgroups and the two edge parts), chunks of parts; `grid` has the borders in haystack offsets"""
    def __init__(self, cus, fa, mode, n, n_bytes):
        self.cus, self.mode, self.mis = cus, mode, fa % 16
        self.ntiles = n_tiles(self.mis, n_bytes, n)
        self.tpw = tiles_per_workgroup(self.ntiles, self.cus, self.mode)
        self.blocks = -(-self.ntiles // self.tpw)
        self.parts = self.blocks + 2
        self.chunks = -(-self.parts // CHUNK)
        self.grid = Grid(n_bytes, TILE, self.tpw, self.ntiles, fa - self.mis)

    def chunk_border(self, c):
        """the first byte of the workgroup that is the first part of chunk c + 1 (workgroup w is part w + 1)"""
        return self.grid.start(CHUNK * (c + 1) - 1)

    def __repr__(self):
        return "ntiles %d, %d per workgroup, parts %d, chunks %d (mode %d, %d CUs)" % (self.ntiles, self.tpw, self.parts, self.chunks,
                                                                                      self.mode, self.cus)


def facts(ss, s):
    """(compute units, index of the first filter byte, MODE, needle length) of searcher s on this device"""
    return ss.device_info()["compute_units"], s.device_triple()[0], kernel_of(s)[1], len(s.needle)


def length_for(ntiles, mis, n):
    """a view whose last candidate is 7 short of the end of tile ntiles - 1"""
    return ntiles * TILE - mis + n - 1 - 7


def filled(n_bytes):
    hay = torch.full((n_bytes,), FILLER, dtype=torch.uint8, device="cuda")
    assert hay.data_ptr() % 16 == 0
    return hay


def plant(hay, scenes, erase=False):
    """the scenes into the device haystack in one scatter; erase: the filler back over them"""
    idx = np.concatenate([np.arange(o, o + len(b), dtype=np.int64) for o, b in scenes])
    val = np.frombuffer(b"".join(b for _, b in scenes), dtype=np.uint8).copy()
    if erase:
        val[:] = FILLER
    hay[torch.from_numpy(idx).cuda()] = torch.from_numpy(val).cuda()


def need(n_bytes):
    free, _ = torch.cuda.mem_get_info()
    if free < n_bytes + (1 << 30):
        pytest.skip("a haystack of %d MiB needs that much device memory and 1 GiB, %d MiB are free" % (n_bytes >> 20, free >> 20))


# ---- calls against a reference --------------------------------------------------------------------------------------------------
def blame(grid, notes, got, ref, ends):
    """where a record array first differs from the reference, as the workgroup that closes that record and what was planted around it"""
    k = min(got.size, ref.size)
    d = np.flatnonzero(got[:k] != ref[:k])
    j = int(d[0]) if d.size else k
    w = int(grid.workgroup_of(min(int(ends[j]), grid.length - 1))) if j < ends.size else grid.nwg - 1
    return "record %d (want %s, got %s), closed in workgroup %d: %s" % (j, ref[j:j + 2], got[j:j + 2], w,
                                                                        {v: notes[v] for v in range(w - 2, w + 2) if v in notes})


def find_into(s, hay, inverted, kw, cap, skip=None):
    """find_lines(_inverted)_into three windows of `cap` (one left out: skip); returns (total, windows)"""
    ws = [Window(cap) for _ in range(3)]
    args = [None if (k == skip or cap == 0) else ws[k].view for k in range(3)]
    fn = s.find_lines_inverted_into if inverted else s.find_lines_into
    return fn(hay, args[0], args[1], args[2], cap, **kw), ws


def check_combo(s, hay, how, inverted, want, grid, notes, what):
    """the count and the records at exact capacity against `want`"""
    kw = HOWS[how]
    what = (what, how, "inverted" if inverted else "plain")
    total = want[0].size
    got = (s.count_lines_inverted if inverted else s.count_lines)(hay, **kw)
    assert got == total, (what, got, total)
    n, ws = find_into(s, hay, inverted, kw, total)
    assert n == total, (what, n, total)
    for k, (w, ref) in enumerate(zip(ws, want)):
        h = w.buf.cpu().numpy()
        assert (h[:8] == SENT).all() and (h[8 + total:] == SENT).all(), (what, k, "sentinels")
        assert (h[8:8 + total] == ref).all(), (what, ("begin", "end", "number")[k], blame(grid, notes, h[8:8 + total], ref, want[1]))


def check_cut(s, hay, how, inverted, want, cap, what, skip=None):
    """a window of `cap` records: the first cap of them, the total, both sentinels; a left-out array stays untouched"""
    total = want[0].size
    n, ws = find_into(s, hay, inverted, HOWS[how], cap, skip)
    assert n == total, (what, how, inverted, cap, n, total)
    for k in range(3):
        ws[k].check(want[k][:0 if (k == skip or cap == 0) else min(cap, total)], (what, how, inverted, cap, skip, k))


def check_async(s, hay, refs, how, what):
    """count_lines_async and count_lines_inverted_async once, on a side stream"""
    side = torch.cuda.Stream()
    out = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s.count_lines_async(hay, out[1:2], **HOWS[how])
        s.count_lines_inverted_async(hay, out[2:3], **HOWS[how])
    side.synchronize()
    assert out.cpu().tolist() == [SENT, refs[how, False][0].size, refs[how, True][0].size, SENT], (what, how)


# ---- B1, B2: two tiles per workgroup ---------------------------------------------------------------------------------------------
def two_tile_length(cus, fa, mode, n):
    """the smallest odd number of tiles that gives a workgroup two, and two tiles more"""
    return length_for(2 * cus * (256 if mode == 0 else 128) + 3, fa % 16, n)


def both_tiles(grid, want):
    """(the workgroups that close records of `want` in both of their tiles, every record's tile)"""
    tile = grid.tile_of(want[1])
    return np.intersect1d(tile[tile % 2 == 0] // 2, tile[tile % 2 == 1] // 2), tile


def two_tile_plan(cus, fa, mode, needle, rng, what):
    """(shape, scenes, notes, references, cuts) of one two-tile haystack; everything that can be said without the GPU is asserted here"""
    n = len(needle)
    n_bytes = two_tile_length(cus, fa, mode, n)
    sh = Shape(cus, fa, mode, n, n_bytes)
    print("%s: %r" % (what, sh))
    assert sh.ntiles == 2 * cus * (256 if mode == 0 else 128) + 3 and sh.ntiles % 2 == 1 and sh.tpw == 2, sh
    assert tiles_per_workgroup(sh.ntiles - 4, cus, mode) == 1 and sh.ntiles - 2 * (sh.blocks - 1) == 1, sh    # the last workgroup has one tile
    grid, nwg = sh.grid, sh.blocks
    w0 = nwg // 3
    long_line = (w0, w0 + 44, w0 + 20)                      # one line through 45 workgroups
    special = {0, 1, nwg - 2, nwg - 1}
    if n_bytes > (1 << 32) + 4 * TILE:
        special |= {((1 << 32) // TILE) // 2 - 1, ((1 << 32) // TILE) // 2}
    free = np.array([w for w in range(2, nwg - 2) if not w0 - 1 <= w <= w0 + 44], dtype=np.int64)
    wgs = sorted(set(rng.choice(free, size=216, replace=False).tolist()) | special)
    notes = {}
    scenes = two_tile_scenes(grid, needle, wgs, long_line, notes)
    print("%s: %d workgroups chosen of %d, %d scenes, uses of the kinds %s" % (what, len(wgs), nwg, len(scenes), sorted(notes["uses"].items())))
    refs = {(how, inv): sparse_lines(scenes, n_bytes, needle, 10, how, inv) for how, inv in COMBOS}
    # the conditions that keep the test honest
    assert sorted(notes["uses"]) == list(range(len(KINDS))) and min(notes["uses"].values()) >= 20, notes["uses"]
    assert both_tiles(grid, refs["", False])[0].size >= 150
    b, e, _ = refs["", False]
    spans = grid.workgroup_of(e - 1) - grid.workgroup_of(b)
    assert spans.max() >= 40 and int((spans >= 40).sum()) == 1 and e[np.argmax(spans)] == grid.start(long_line[1]) + n + n + 3 + 2
    assert grid.tile_of(grid.border(2 * long_line[2] + 1) + TILE // 2) % 2 == 1
    counts = [refs[how, False][0].size for how in HOW_NAMES]
    assert len(set(counts)) >= 4, counts
    for how in HOW_NAMES:
        lines = refs[how, False][0].size + refs[how, True][0].size
        assert 0 < refs[how, True][0].size < lines and lines == refs["", False][0].size + refs["", True][0].size, (how, lines)
    # capacity cuts in three workgroups that close selected lines in both tiles: a rank inside the second tile, the workgroup's
    # last record, one more, one fewer
    cuts = []
    for how, inv in (("", False), ("w", False), ("", True)):
        both, tile = both_tiles(grid, refs[how, inv])
        wg = tile // 2
        both = np.array([w for w in both.tolist() if int(((wg == w) & (tile % 2 == 1)).sum()) >= 2 and w != nwg - 1])
        assert both.size >= 3, (how, inv, both.size)
        for w in (int(both[0]), int(both[both.size // 2]), int(both[-1])):
            first_second = int(np.flatnonzero((wg == w) & (tile % 2 == 1))[0])
            last = int(np.flatnonzero(wg == w)[-1])
            assert first_second + 1 <= last
            cuts += [(how, inv, cap, w) for cap in (first_second + 1, last + 1, last + 2, last)]
    return sh, scenes, notes, refs, cuts


def two_tile(ss, s, mode, hay, rng, what):
    cus, fa, m, n = facts(ss, s)
    assert m == mode
    sh, scenes, notes, refs, cuts = two_tile_plan(cus, fa, mode, s.needle, rng, what)
    view = hay[:sh.grid.length]
    plant(view, scenes)
    for how, inv in COMBOS:
        check_combo(s, view, how, inv, refs[how, inv], sh.grid, notes, what)
    check_async(s, view, refs, "wi", what)
    for how, inv, cap, w in cuts:
        check_cut(s, view, how, inv, refs[how, inv], cap, "%s, workgroup %d: %s" % (what, w, notes.get(w)))
    plant(view, scenes, erase=True)


def test_two_tiles_per_workgroup_mode0(ss):
    """2 GiB and 48 KiB on 256 CUs: 131,075 tiles, 65,538 workgroups, the last of one tile; a needle verified in registers and one
    verified in memory, each with its own scenes in the same allocation"""
    short, long_ = make(ss, NEEDLE), make(ss, LONG, triple=(0, 5, 5))
    assert len(NEEDLE) == 4 and len(LONG) >= 33
    top = max(two_tile_length(*facts(ss, t)) for t in (short, long_))
    need(top)
    hay = filled(top)
    rng = np.random.default_rng(201)
    for s, what in ((short, "mode 0, 4 bytes"), (long_, "mode 0, 33 bytes")):
        assert kernel_of(s)[1] == 0
        two_tile(ss, s, 0, hay, rng, what)
    del hay
    torch.cuda.empty_cache()


def test_two_tiles_per_workgroup_mode2(ss):
    """1 GiB and 48 KiB on 256 CUs, a filter pair 34 bytes apart"""
    needle, triple = MODE2
    s = make(ss, needle, triple=triple)
    assert kernel_of(s)[1] == 2
    top = two_tile_length(*facts(ss, s))
    need(top)
    hay = filled(top)
    two_tile(ss, s, 2, hay, np.random.default_rng(202), "mode 2, 50 bytes")
    del hay
    torch.cuda.empty_cache()


# ---- B3: chunk borders at one tile per workgroup, against the dense rules -----------------------------------------------------------
def chunk_border_plan(cus, fa, mode, needle):
    """the shape and [(name, host array, dense references)] of the 8 MiB haystacks.  The dense rules that ignore case cost four times
    the others on 8 MiB (they fold the whole array), so they run on the first rotation and on the first haystack without a
    delimiter in chunk 1; the other six haystacks take the six case-sensitive combinations (the chunk and combine kernels are the
    same launches for both, only the scan in front of them differs)."""
    n = len(needle)
    n_bytes = length_for(514, fa % 16, n)
    sh = Shape(cus, fa, mode, n, n_bytes)
    print("chunk borders: %r" % sh)
    assert (sh.ntiles, sh.tpw, sh.blocks, sh.parts, sh.chunks) == (514, 1, 514, 516, 3) and n_tiles(sh.mis, n_bytes - TILE, n) == 513, sh
    grid = sh.grid
    X = [sh.chunk_border(0), sh.chunk_border(1)]
    assert [int(grid.workgroup_of(x)) for x in X] == [255, 511] and [int(grid.workgroup_of(x - 1)) for x in X] == [254, 510]
    quiet = [w for w in range(3, 514, 23) if min(abs(w - 254.5), abs(w - 510.5)) > 3]
    variants = [("kinds %d and %d" % (r, (r + 3) % 6), border_scenes(r, X[0], needle) + border_scenes((r + 3) % 6, X[1], needle), quiet)
                for r in range(len(BORDER_KINDS))]
    outside = [w for w in quiet if not 250 <= w <= 512]
    variants.append(("chunk 1 without a delimiter, a match pending from chunk 0",
                     [(grid.start(252) + 100, NL + needle), (grid.start(511) + 50, NL)], outside))
    variants.append(("chunk 1 without a delimiter, its match inside",
                     [(grid.start(252) + 100, NL), (grid.start(400) + 7000, needle), (grid.start(512) + 50, NL)], outside))
    out, nscenes = [], 0
    for k, (name, scenes, bg) in enumerate(variants):
        scenes = checked(scenes + background_scenes(grid, needle, bg) + [(0, needle + b" "), (n_bytes - n - 1, NL + needle)], n_bytes)
        nscenes += len(scenes)
        host = write_scenes(np.full(n_bytes, FILLER, dtype=np.uint8), scenes)
        refs = {}
        for how in HOW_NAMES if k in (0, 6) else ("", "w", "x"):     # the dense rules: tests/test_gpu_inverted.py's, on the array
            refs[how, True], refs[how, False], every = ref_inverted(host, needle, 10, how)
        if "without" in name:
            assert not (host[X[0]:X[1]] == 10).any()
            b, e, _ = refs["", False]
            assert ((b < X[0]) & (e >= X[1])).sum() == 1
        else:
            for x in X:                                     # a line closes within 2 n + 6 bytes on either side of each border
                e = every[1]
                assert ((e >= x - 2 * n - 6) & (e < x)).any() and ((e >= x) & (e <= x + 2 * n + 6)).any(), name
        assert 0 < refs["", False][0].size and 0 < refs["", True][0].size
        out.append((name, host, refs))
    print("chunk borders: 514 workgroups, %d haystacks, %d scenes" % (len(variants), nscenes))
    return sh, X, out


def test_chunk_borders_at_one_tile_per_workgroup(ss):
    """8 MiB and two tiles: 514 workgroups, 516 parts, three chunks.  Every kind of BORDER_KINDS at the part borders 255|256 and
    511|512 (one kind per border and haystack, rotating), and two haystacks whose chunk 1 holds no delimiter at all: a match
    pending from chunk 0, and a match inside chunk 1 only, the closing delimiter in chunk 2.  All twelve combinations on two of the
    eight haystacks, the six case-sensitive ones on the other six (chunk_border_plan says why)."""
    s = make(ss, NEEDLE)
    sh, X, variants = chunk_border_plan(*facts(ss, s)[:3], NEEDLE)
    for name, host, refs in variants:
        hay = torch.from_numpy(host).cuda()
        assert hay.data_ptr() % 16 == 0
        assert len(refs) in (6, 12)
        for how, inv in sorted(refs):
            check_combo(s, hay, how, inv, refs[how, inv], sh.grid, {}, name)
        check_async(s, hay, refs, "", name)
        # cuts at the ranks of the records that close just in front of, on and just behind each border; each array left out in turn
        for inv in (False, True):
            want = refs["", inv]
            for x in X:
                k = int(np.searchsorted(want[1], x, side="left"))
                for cap in sorted({max(k - 1, 0), k, k + 1, k + 2}):
                    check_cut(s, hay, "", inv, want, cap, name)
                for skip in (0, 1, 2):
                    check_cut(s, hay, "", inv, want, k + 1, name, skip)


# ---- B4: more than 1,024 chunks ----------------------------------------------------------------------------------------------------
MANY = (("", False), ("w", False), ("i", False), ("", True))


def many_chunks_length(cus, fa, n):
    for tpw in (2, 1):
        ntiles = (THREADS * CHUNK - 2) * tpw + 1            # blocks + 2 == 1024 * 256 + 1 parts
        if tiles_per_workgroup(ntiles, cus, 0) == tpw:
            break
    assert tiles_per_workgroup(ntiles, cus, 0) == tpw and -(-(-(-ntiles // tpw) + 2) // CHUNK) == THREADS + 1
    ntiles = max(ntiles, (1 << 33) // TILE + 5)             # ... and past 2^33
    if tpw == 2 and ntiles % 2 == 0:
        ntiles += 1
    return length_for(ntiles, fa % 16, n)


def many_chunks_plan(cus, fa, needle):
    """the shape, the scenes that stay, and per rotation (the scenes at the chunk borders, all scenes' references)"""
    n = len(needle)
    n_bytes = many_chunks_length(cus, fa, n)
    sh = Shape(cus, fa, 0, n, n_bytes)
    print("more than 1,024 chunks: %r" % sh)
    per = -(-sh.chunks // THREADS)
    assert sh.chunks > THREADS and per >= 2 and n_bytes > (1 << 33) + 2 * TILE, sh
    grid, nwg = sh.grid, sh.blocks
    ts = (0, 1, 255, 511, (sh.chunks - 1) // per)
    inside = sorted({t * per for t in ts if t * per + 1 < sh.chunks})
    between = sorted({(t + 1) * per - 1 for t in ts if (t + 1) * per < sh.chunks})
    assert len(inside) >= 4 and len(between) >= 4 and not set(inside) & set(between), (inside, between)
    borders = sorted(inside + between)
    # a delimiter-free stretch over the whole run of thread 300, a match pending across it
    tf = 300
    assert tf not in ts and (tf + 2) * per < sh.chunks
    wa, wb = CHUNK * tf * per - 4, CHUNK * (tf + 1) * per + 1
    stretch = [(grid.start(wa) + TILE // 3, NL + needle), (grid.start(wb) + TILE // 3, NL)]
    near = np.array([CHUNK * (c + 1) - 1 for c in borders] + [int(grid.workgroup_of(1 << 33))])
    quiet = [w for w in range(5, nwg - 5, 1009) if np.abs(near - w).min() > 2 and not wa - 1 <= w <= wb + 1]
    fixed = checked(stretch + background_scenes(grid, needle, quiet) + border_scenes(2, 1 << 33, needle) +
                    [((1 << 33) + TILE + 100, NL + b"kk" + NL), (n_bytes - n - 1, NL + needle)], n_bytes)
    notes = {CHUNK * (c + 1) - 1: "the first workgroup of chunk %d (a border %s a run)" % (c + 1, "inside" if c in inside else "between")
             for c in borders}
    rotations, nscenes = [], 0
    for rot in (0, 1):
        moving = []
        for j, c in enumerate(borders):
            moving += border_scenes((j + rot) % len(BORDER_KINDS), sh.chunk_border(c), needle)
        scenes = checked(fixed + moving, n_bytes)
        nscenes += len(scenes)
        refs = {(how, inv): sparse_lines(scenes, n_bytes, needle, 10, how, inv) for how in ("", "w", "i") for inv in (False, True)}
        for key in MANY:                                    # records above 2^33, and (matching) one across it
            b, e, _ = refs[key]
            assert (b > (1 << 33)).any() and ((b < (1 << 33)) & (e > (1 << 33))).any() == (not key[1]), key
        b, e, _ = refs["", False]
        assert ((b < grid.start(CHUNK * tf * per - 1)) & (e >= grid.start(CHUNK * (tf + 1) * per - 1))).sum() == 1
        assert refs["", False][1][-1] == n_bytes            # the unterminated last line matches
        rotations.append((moving, refs))
    kinds = {side: sorted({(borders.index(c) + rot) % len(BORDER_KINDS) for c in cs for rot in (0, 1)}) for side, cs in
             (("inside", inside), ("between", between))}
    assert all(len(v) == len(BORDER_KINDS) for v in kinds.values()) or per != 2, kinds
    print("more than 1,024 chunks: %d workgroups, %d chunks per thread, borders behind chunks %s, 2 rotations, %d scenes" % (nwg, per, borders, nscenes))
    return sh, fixed, notes, rotations


def test_more_than_1024_chunks(ss):
    """The smallest view with more than 1,024 chunks of parts - 262,143 workgroups, 8 GiB less 48 KiB at two tiles each - made a few
    tiles longer so that it reaches past 2^33 (still 1,025 chunks): lines_combine_kernel's threads walk runs of two chunks.
    BORDER_KINDS at the chunk borders inside a run (2t | 2t + 1) and between runs (2t + 1 | 2t + 2) for t = 0, 1, 255, 511 and the
    last thread, in two rotations, so that both sorts of border see every kind."""
    s = make(ss, NEEDLE)
    cus, fa, mode, n = facts(ss, s)
    assert mode == 0
    need(many_chunks_length(cus, fa, n))
    sh, fixed, notes, rotations = many_chunks_plan(cus, fa, NEEDLE)
    hay = filled(sh.grid.length)
    plant(hay, fixed)
    for rot, (moving, refs) in enumerate(rotations):
        plant(hay, moving)
        for how, inv in MANY:
            check_combo(s, hay, how, inv, refs[how, inv], sh.grid, notes, "rotation %d" % rot)
            check_cut(s, hay, how, inv, refs[how, inv], refs[how, inv][0].size // 2, "rotation %d, the middle" % rot)
        check_async(s, hay, refs, "", "rotation %d" % rot)
        plant(hay, moving, erase=True)
    del hay
    torch.cuda.empty_cache()
