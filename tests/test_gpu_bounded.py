"""GPU tests of the whole-word / whole-line calls (include/sliceslice_hip_bounded.h, libsliceslice_hip_bounded.so):
ss_count_bounded_device / _async, ss_find_all_bounded_device, ss_count_lines_bounded_device / _async and
ss_find_lines_bounded_device against the rule restated on numpy arrays - the occurrences of tests/test_gpu_matches.py (through
``bytes.lower()`` where case is ignored), kept where both neighbour bytes are absent, no word bytes or (line forms) the delimiter -
and against tests/golden/bounded_kat.json.  Every comparison is of integers and exact; every output array is a window of a larger
one whose sentinels on both sides must survive."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_gpu_matches import _loaded, kernel_of, n_tiles, ref_offsets, tiles_per_workgroup

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MiB = 1 << 20
TILE = 16384                    # bytes per tile: 4 waves x 4 pieces of 1 KiB
SENT = -0x5A5A5A5A5A5A5A5B
GUARD = 8
_LOWER = np.frombuffer(bytes(range(256)).lower(), dtype=np.uint8)
_WORD = np.zeros(256, dtype=bool)
_WORD[list(b"0123456789_") + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B))] = True
# neighbour bytes: word bytes of every kind, the usual delimiter, and the non-word bytes that sit next to the word ranges or look
# like letters in their low seven bits
NEIGHBOURS = [ord("k"), ord("K"), ord(" "), 10, ord("_"), ord("7"), 0x80, 0xC1, 0xE1, ord("@"), ord("["), ord("`"), ord("{"), ord("/"),
              ord(":"), 0xFF, 0x00]
# needle lengths for every verify path (tests/test_gpu_nocase.py): the one-byte test (1), the in-register exact compare (2..16,
# with flags handed over from the next lane), the LDS compare (17..2048), the global continuation (> 2048)
LENGTHS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 18, 31, 33, 64, 100, 1000, 2047, 2048, 2049, 2500, 3000]


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with bounded_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "bounded_kat.json")))


@pytest.fixture(scope="module")
def manual():
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    return data, torch.from_numpy(data.copy()).cuda()


def bounded_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the bounded entry points, else `ss.bounded_build()`."""
    return _loaded() if getattr(ss.lib(), "has_bounded", False) else ss.bounded_build()


def make(ss, needle, position=None, triple=None):
    """a searcher of the bounded library for `needle` as it is (the tests' needles hold no upper-case byte, so ignore_case works)"""
    with bounded_lib(ss):
        s = ss.DynamicHipSearcher(needle, position)
        if triple is not None:
            s.set_filter(*triple)
        return s


def dev_of(host):
    host = np.asarray(host, dtype=np.uint8)
    return torch.from_numpy(host.copy()).cuda() if host.size else torch.empty(0, dtype=torch.uint8, device="cuda")


# ---- the rule on numpy arrays ---------------------------------------------------------------------------------------------------
def ref_kept(h, needle, nocase, line, delim):
    """offsets of the occurrences of `needle` in h (ignoring case: both through bytes.lower()) both of whose neighbours are absent,
    equal to `delim` (None: the occurrence forms, which have none) or - unless `line` - no word bytes; neighbours are read RAW"""
    h = np.asarray(h, dtype=np.uint8)
    nd = bytes(needle).lower() if nocase else bytes(needle)
    offs = ref_offsets(_LOWER[h] if nocase else h, nd)
    if len(nd) == 0 or offs.size == 0:
        return offs[:0]
    keep = np.ones(offs.size, dtype=bool)
    for at in (offs - 1, offs + len(nd)):
        absent = (at < 0) | (at >= h.size)
        b = h[np.clip(at, 0, h.size - 1)]
        ok = np.zeros(offs.size, dtype=bool) if line else ~_WORD[b]
        if delim is not None:
            ok |= b == delim
        keep &= absent | ok
    return offs[keep]


def ref_lines(h, needle, delim, line, nocase):
    """(begin, end, number) of the lines of h - cut at `delim` on the bytes as they are - that hold a kept occurrence"""
    h = np.asarray(h, dtype=np.uint8)
    nd = bytes(needle).lower() if nocase else bytes(needle)
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, h.size, dtype=np.int64)))
    if begins[-1] == h.size:
        begins, ends = begins[:-1], ends[:-1]
    if delim in nd:
        k = np.zeros(0, dtype=np.int64)
    else:
        offs = ref_kept(h, nd, nocase, line, delim)
        # an occurrence must not run over a delimiter (ignoring case, a delimiter 'A' folds onto a needle byte 'a')
        first = np.searchsorted(dpos, offs, side="left")
        inside = np.searchsorted(dpos, offs + len(nd) - 1, side="right") == first
        k = np.unique(first[inside]).astype(np.int64)
    return begins[k], ends[k], k + 1


class Window:
    """`cap` int64 slots inside a larger device array filled with a sentinel"""
    def __init__(self, cap):
        self.cap = cap
        self.buf = torch.full((cap + 2 * GUARD,), SENT, dtype=torch.int64, device="cuda")
        self.view = self.buf[GUARD:GUARD + cap]

    def check(self, want, what):
        """the first len(want) slots hold `want`, every other slot of the larger array the sentinel"""
        h = self.buf.cpu().numpy()
        k = len(want)
        assert (h[:GUARD] == SENT).all() and (h[GUARD + k:] == SENT).all(), what
        assert (h[GUARD:GUARD + k] == np.asarray(want, dtype=np.int64)).all(), (what, h[GUARD:GUARD + min(k, 6)], want[:6])


def check_offsets(s, dev, host, needle, nocase, what):
    """count, count_async and find_all_into (exact capacity) with whole_word against the rule; returns the offsets"""
    want = ref_kept(host, needle, nocase, False, None)
    got = s.count(dev, ignore_case=nocase, whole_word=True)
    assert got == want.size, (what, needle[:24], nocase, got, want.size)
    w = Window(want.size)
    assert s.find_all_into(dev, w.view, ignore_case=nocase, whole_word=True) == want.size, (what, nocase)
    w.check(want, (what, needle[:24], nocase))
    return want


def check_lines(s, dev, host, needle, delim, nocase, what, modes=(False, True)):
    """count_lines and find_lines_into (exact capacity) with whole_word and with whole_line against the rule"""
    sizes = []
    for line in modes:
        kw = dict(ignore_case=nocase, whole_word=not line, whole_line=line)
        wb, we, wn = ref_lines(host, needle, delim, line, nocase)
        got = s.count_lines(dev, delim, **kw)
        assert got == wb.size, (what, needle[:24], delim, kw, got, wb.size)
        ws = [Window(wb.size) for _ in range(3)]
        assert s.find_lines_into(dev, ws[0].view, ws[1].view, ws[2].view, wb.size, delim, **kw) == wb.size, (what, delim, kw)
        for w, want in zip(ws, (wb, we, wn)):
            w.check(want, (what, needle[:24], delim, kw))
        sizes.append(wb.size)
    return sizes


def check(s, dev, host, needle, delims=(10,), what="", cases=(False, True)):
    out = None
    for nocase in cases:
        want = check_offsets(s, dev, host, needle, nocase, what)
        out = want if out is None else out
        for delim in delims:
            check_lines(s, dev, host, needle, delim, nocase, what)
    return out


def mixed_case(rng, needle):
    """a copy of the needle with every letter in a random case"""
    nb = np.frombuffer(bytes(needle), dtype=np.uint8).copy()
    letters = (nb >= 0x61) & (nb <= 0x7A)
    nb[letters & (rng.random(nb.size) < 0.5)] ^= 0x20
    return nb


def needle_of(rng, n):
    """n bytes over lower-case letters, digits and punctuation: no upper case, none of NEIGHBOURS' letters, no usual delimiter"""
    alphabet = np.frombuffer(b"azmazmetnor0189-.+", dtype=np.uint8)
    nb = rng.choice(alphabet, size=n)
    nb[0] = ord("a")
    nb[-1] = ord("z") if n > 1 else nb[-1]
    return nb.tobytes()


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def test_only_the_bounded_library_has_the_entry_points(ss):
    with ss.nocase_build() as L:
        assert not L.has_bounded
    with ss.bounded_build() as L:
        assert L.has_bounded and L.has_nocase and L.has_lines and L.has_matches and not L.has_matches_batched
    with ss.nocase_build():
        t = ss.DynamicHipSearcher(b"abc")
    d = dev_of(np.frombuffer(b"abc abc", dtype=np.uint8))
    for call in (lambda: t.count(d, whole_word=True), lambda: t.count_lines(d, whole_line=True),
                 lambda: t.find_all(d, ignore_case=True, whole_word=True)):
        with pytest.raises(ss.SlicesliceError, match="bounded_build"):
            call()
    # with both keywords off a searcher of the bounded library takes the plain and the folding calls
    s = make(ss, b"abc")
    assert (s.count(d), s.count(d, ignore_case=True), s.count(d, whole_word=True), s.count_lines(d), s.count_lines(d, whole_line=True)) == \
        (2, 2, 2, 1, 0)


def test_the_small_case_table(ss, kat):
    for c in kat["cases"]:
        hay, needle = bytes.fromhex(c["haystack"]), bytes.fromhex(c["needle"])
        nocase, line = c["how"].endswith("i"), c["how"].startswith("x")
        s = make(ss, needle)
        h = np.frombuffer(hay, dtype=np.uint8)
        d = dev_of(h)
        if not line:
            assert s.count(d, ignore_case=nocase, whole_word=True) == len(c["offsets"]), c["what"]
            assert s.find_all(d, ignore_case=nocase, whole_word=True).cpu().tolist() == c["offsets"], c["what"]
            assert ref_kept(h, needle, nocase, False, None).tolist() == c["offsets"], c["what"]
        kw = dict(ignore_case=nocase, whole_word=not line, whole_line=line)
        assert s.count_lines(d, c["delimiter"], **kw) == len(c["records"]), c["what"]
        b, e, n = (t.cpu().tolist() for t in s.find_lines(d, bytes([c["delimiter"]]), **kw))
        assert [list(r) for r in zip(b, e, n)] == c["records"], (c["what"], b, e, n)
        # ... and the restatement of this file agrees with the fixture
        assert [list(r) for r in zip(*(a.tolist() for a in ref_lines(h, needle, c["delimiter"], line, nocase)))] == c["records"], c["what"]


def test_every_golden_word_of_the_manual(ss, kat, manual):
    data, d = manual
    keys = ("word_count", "word_lines", "line_lines")
    rows = [(w.encode("latin-1"), {k: kat[k][j] for k in kat if k.startswith(keys)}) for j, w in enumerate(kat["words"])]
    rows += [(w.encode(), t) for w, t in kat["table"].items()]
    assert len(rows) >= 300
    bad = []
    for j, (w, want) in enumerate(rows):
        for nocase, tag in ((False, ""), (True, "_nocase")):
            nd = w.lower() if nocase else w
            s = make(ss, nd)
            got = (s.count(d, ignore_case=nocase, whole_word=True), s.count_lines(d, ignore_case=nocase, whole_word=True),
                   s.count_lines(d, ignore_case=nocase, whole_line=True))
            if got != tuple(want[k + tag] for k in keys):
                bad.append((w, nocase, got, want))
            if j % 16 == 0 or j >= len(kat["words"]):           # offsets and records: every sixteenth word and the table's
                check_offsets(s, d, data, nd, nocase, "manual")
                check_lines(s, d, data, nd, 10, nocase, "manual")
    assert not bad, bad[:10]
    t = kat["table"]["the"]
    s = make(ss, b"the")
    assert (s.count(d), s.count(d, whole_word=True), s.count_lines(d, whole_word=True)) == (t["count"], t["word_count"], t["word_lines"])


UNITS = (16, 1024, 4096, TILE)     # a lane's chunk, a piece, a wave's four pieces, a tile


def borders(length):
    """(border, unit): ends of a lane's 16-byte chunk, of a 1 KiB piece, of a wave's 4 KiB and of a 16 KiB tile below `length`,
    each labelled with the largest unit it is a border of"""
    out = {16 * k for k in (3, 10, 67, 131)} | {1024 * k for k in (1, 3, 5, 17, 33)} | {4096 * k for k in (1, 3, 6, 9)} | {TILE * k for k in (1, 2)}
    return [(b, max(u for u in UNITS if b % u == 0)) for b in sorted(out) if b < length]


# which byte sits on the border: the left neighbour on the last byte in front of it / on the first byte behind it, the right
# neighbour likewise - as the offset of p from the border (the needle's length is subtracted for the right neighbour)
KINDS = (("p - 1 last before", lambda n: 0), ("p - 1 first behind", lambda n: 1), ("p + n last before", lambda n: -1 - n),
         ("p + n first behind", lambda n: -n))


def test_neighbours_on_every_border(ss):
    rng = np.random.default_rng(71)
    G = 64
    kept_sum = every_sum = 0
    fill = np.frombuffer(b"#\n \x00%\xe1k7_", dtype=np.uint8)
    for n in LENGTHS:
        needle = needle_of(rng, n) if n > 1 else b"a"
        s = make(ss, needle)
        for L, mis in ((3 * TILE, 0), (5 * 1024, 0), (3 * TILE, 9)):
            # ONE kind per haystack, so that every border that has room takes a copy of that kind (planted together, a copy at
            # p = border leaves no room for the other three).  Borders are taken from the 16-byte-aligned start of the buffer,
            # which is what the kernels' chunks, pieces and tiles are aligned to; the view starts `mis` bytes behind it.
            for kind, shift in KINDS:
                host = rng.choice(fill, size=L + 2 * G + 16)
                v0 = G + mis
                at, stop, ends, units, j = v0 + 1, v0 + L, 0, set(), int(rng.integers(len(NEIGHBOURS)))
                # p == 0 and p + n == len, with word bytes just outside the view: both ends are absent neighbours
                if 4 * n + 64 < L:
                    host[v0:v0 + n] = mixed_case(rng, needle)
                    host[v0 + n] = ord(" ")
                    host[v0 + L - n:v0 + L] = np.frombuffer(needle, dtype=np.uint8)
                    host[v0 + L - n - 1] = 10
                    at, stop, ends = v0 + n + 2, v0 + L - n - 1, 2
                for border, unit in borders(L):
                    p = G + border + shift(n)
                    if p < at or p + n + 1 > stop:
                        continue
                    host[p:p + n] = mixed_case(rng, needle) if j % 2 else np.frombuffer(needle, dtype=np.uint8)
                    # the two neighbours run through NEIGHBOURS at different paces, so every pair of classes occurs
                    host[p - 1] = NEIGHBOURS[j % len(NEIGHBOURS)]
                    host[p + n] = NEIGHBOURS[(3 * j + 5) % len(NEIGHBOURS)]
                    at, j = p + n + 2, j + 1
                    units.add(unit)
                host[v0 - 1], host[v0 + L] = ord("w"), ord("W")
                what = "n %d len %d mis %d, %s" % (n, L, mis, kind)
                assert units, what                              # every kind lands at least once in every haystack ...
                if n <= 100 and L == 3 * TILE:
                    assert units == set(UNITS), (what, units)   # ... and on a border of every unit where the needle leaves room
                dev = dev_of(host)
                assert dev.data_ptr() % 16 == 0
                view, hview = dev[v0:v0 + L], host[v0:v0 + L]
                want = check(s, view, hview, needle, (10, ord("k")), what)
                every = ref_offsets(_LOWER[hview], needle).size
                assert every >= len(units) + ends, (what, units, every)
                kept_sum, every_sum = kept_sum + want.size, every_sum + every
    assert 0 < kept_sum < every_sum, (kept_sum, every_sum)      # the neighbours decided: some copies are words, some are not


def test_filter_shapes_all_nine_kernels_in_both_units(ss):
    rng = np.random.default_rng(72)
    L = 3 * TILE + 321
    base = needle_of(rng, 1400)
    rows = [("one byte", b"a", {}), ("mode0 q0", base[:40], dict(triple=(0, 2, 2))), ("mode0 q1", base[:40], dict(triple=(0, 5, 5))),
            ("mode0 q2", base[:40], dict(triple=(0, 9, 9))), ("mode0 q3", base[:40], dict(triple=(0, 13, 13))),
            ("mode0 q3 first at 2", base[:40], dict(triple=(2, 3, 15))),
            ("with_position 20", base[:48], dict(position=20)), ("with_position 47", base[:48], dict(position=47)),
            ("mode2 q0", base[:48], dict(triple=(0, 16, 16))), ("mode2 q1", base[:48], dict(triple=(3, 23, 23))),
            ("mode2 q2", base[:60], dict(triple=(0, 40, 40))), ("mode2 q3", base[:48], dict(triple=(5, 33, 33))),
            ("pair alone d=3", base[:70], dict(triple=(1, 61, 61))), ("far_off", base, dict(triple=(0, 1300, 1300)))]
    # (the library adds a third byte of its own to a plain pair, which can move the window: further MODE 0 pairs stand by, and a
    # candidate runs when it is one of the rows above or brings a kernel that has not run yet)
    named = len(rows)
    rows += [("mode0 pair %d" % fb, base[:40], dict(triple=(0, fb, fb))) for fb in (1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15)]
    rows += [("mode0 triple %d %d" % (fb, fc), base[:40], dict(triple=(0, fb, fc))) for fb, fc in ((1, 2), (4, 5), (8, 9), (12, 13))]
    kernels = set()
    for k, (name, nd, kw) in enumerate(rows):
        s = make(ss, nd, **kw)
        if k >= named and kernel_of(s) in kernels:
            continue
        kernels.add(kernel_of(s))
        nl = len(nd)
        host = rng.choice(np.frombuffer(b"azmAZM \n_", dtype=np.uint8), size=L + 64)
        at, j = 100, 0
        while at + nl + 64 < L:
            host[at:at + nl] = mixed_case(rng, nd) if j % 2 else np.frombuffer(nd, dtype=np.uint8)
            host[at - 1] = NEIGHBOURS[j % len(NEIGHBOURS)]
            host[at + nl] = NEIGHBOURS[(3 * j + 5) % len(NEIGHBOURS)]
            at, j = at + nl + int(rng.integers(20, 3000)), j + 1
        dev = dev_of(host)
        before = s.tuning_state(dev[:L])
        for mis in (0, 11):                                  # (both units: `check` runs the case-sensitive and the folding kernels)
            want = check(s, dev[mis:mis + L], host[mis:mis + L], nd, (10,), "%s mis %d" % (name, mis))
            assert want.size >= 1, (name, want.size)
        assert s.tuning_state(dev[:L]) == before, name       # the kernel choice is the searcher's own, untouched by the calls
    want = {(q, m, False) for q in range(4) for m in (0, 2)} | {(0, 0, True)}
    assert kernels == want, sorted(want - kernels)


def test_views_misaligned_at_both_ends(ss):
    rng = np.random.default_rng(73)
    G = 64
    pool = np.frombuffer(b"aAbB \n_", dtype=np.uint8)
    searchers = [(nd, make(ss, nd)) for nd in (b"ab", b"abab", b"a")]
    for mis in range(1, 16):
        for L in (1, 2, 5, 16, 17, 33, 1025, TILE + 1, 2 * TILE + 16 - mis):
            host = rng.choice(pool, size=L + 2 * G, p=[0.2, 0.15, 0.2, 0.15, 0.15, 0.1, 0.05])
            v0 = G + mis
            if L >= 4:
                host[v0:v0 + 2] = host[v0 + L - 2:v0 + L] = np.frombuffer(b"ab", dtype=np.uint8)       # p == 0 and p + n == len
            if mis % 2:
                # needle copies immediately outside and straddling both ends: neither occurrences nor neighbours
                host[v0 - 5:v0] = np.frombuffer(b"\nabab", dtype=np.uint8)
                host[v0 + L:v0 + L + 5] = np.frombuffer(b"abab\n", dtype=np.uint8)
            else:
                host[v0 - 3:v0] = np.frombuffer(b"xyz", dtype=np.uint8)                                # word bytes: absent all the same
                host[v0 + L:v0 + L + 3] = np.frombuffer(b"XYZ", dtype=np.uint8)
            dev = dev_of(host)
            for nd, s in searchers:
                check(s, dev[v0:v0 + L], host[v0:v0 + L], nd, (10, ord("b")) if mis % 4 == 1 else (10,), "mis %d len %d" % (mis, L))
    # a haystack that is exactly the needle; len == n + 1 with the extra byte on either side, a word byte and none
    for nd, s in searchers:
        n = len(nd)
        for extra in (b"", b"c", b" ", b"\n", b"_"):
            for hay in ({nd} if not extra else {nd + extra, extra + nd}):
                host = np.frombuffer(b"ab" + hay + b"ab", dtype=np.uint8)
                want = check(s, dev_of(host)[2:2 + len(hay)], host[2:2 + len(hay)], nd, (10,), repr(hay))
                if n > 1:
                    assert want.size == (0 if extra in (b"c", b"_") else 1), hay


def test_lines_delimiters_that_are_word_bytes_and_capacity_cuts(ss):
    rng = np.random.default_rng(74)
    L = 3 * TILE + 99
    host = rng.choice(np.frombuffer(b"aAbBx _0\n\x00", dtype=np.uint8), size=L, p=[0.2, 0.08, 0.2, 0.08, 0.14, 0.12, 0.06, 0.06, 0.03, 0.03])
    # a line whose only kept occurrence comes behind others that are not; a line matched only across a tile border; empty lines;
    # no trailing delimiter; a last line equal to the needle
    late = np.frombuffer(b"\nxbxb bxbx _bxb bxb0 bxb\n\n\nbxb\n", dtype=np.uint8)
    host[100:100 + late.size] = late
    host[TILE - 3:TILE + 4] = np.frombuffer(b"\n bxb \n", dtype=np.uint8)
    host[2 * TILE - 2:2 * TILE + 3] = np.frombuffer(b"\nbxb\n", dtype=np.uint8)
    host[L - 4:] = np.frombuffer(b"\nbxb", dtype=np.uint8)
    dev = dev_of(host)
    for nd in (b"bxb", b"b", b"xb", b"bx bx", b"b" * 17):
        s = make(ss, nd)
        for delim in (ord("a"), ord("A"), ord("_"), ord("0"), 0x00, 10):
            for nocase in (False, True):
                sizes = check_lines(s, dev, host, nd, delim, nocase, "lines")
                if delim in nd:
                    assert sizes == [0, 0]
        # the line structure is the models' own: whole_line keeps a subset of whole_word's lines when the delimiter is no word byte
        a, b = s.count_lines(dev, whole_word=True), s.count_lines(dev, whole_line=True)
        assert s.count_lines(dev) >= a >= b
    s = make(ss, b"bxb")
    for view, what in ((dev, "open last line"), (dev[:L - 4 + 1], "closed before the last line")):
        hv = host[:view.numel()]
        for delim in (10, ord("x") ^ 0x20):
            check_lines(s, view, hv, b"bxb", delim, False, what)
    for tail in (b"\nbxb", b"\nbxb\n"):                     # whole_line with the needle as the whole last line, with and without its delimiter
        hv = np.concatenate((host[:5000], np.frombuffer(tail, dtype=np.uint8)))
        wb, we, wn = ref_lines(hv, b"bxb", 10, True, False)
        assert wb.size >= 1 and we[-1] == 5000 + 4
        check_lines(s, dev_of(hv), hv, b"bxb", 10, False, repr(tail))
    # capacity cuts at 0, 1, total - 1, total, total + 1, each array left out in turn
    for kw in (dict(whole_word=True), dict(whole_line=True), dict(whole_word=True, ignore_case=True)):
        ref = ref_lines(host, b"bxb", 10, kw.get("whole_line", False), kw.get("ignore_case", False))
        total = ref[0].size
        assert total >= 3
        for cap in (0, 1, total - 1, total, total + 1):
            for skip in (None, 0, 1, 2):
                ws = [Window(cap) for _ in range(3)]
                args = [None if (k == skip or cap == 0) else ws[k].view for k in range(3)]
                assert s.find_lines_into(dev, args[0], args[1], args[2], cap, **kw) == total, (kw, cap, skip)
                for k in range(3):
                    ws[k].check(ref[k][:0 if (k == skip or cap == 0) else min(cap, total)], (kw, cap, skip, k))
    offs = ref_kept(host, b"bxb", False, False, None)
    for cap in (0, 1, offs.size - 1, offs.size, offs.size + 1):
        w = Window(cap)
        assert s.find_all_into(dev, w.view, whole_word=True) == offs.size >= 3
        w.check(offs[:cap], ("find_all", cap))


def test_relations_on_random_two_letter_text(ss):
    rng = np.random.default_rng(75)
    L = 3 * TILE + 5
    host = rng.choice(np.frombuffer(b"ab \n", dtype=np.uint8), size=L, p=[0.4, 0.4, 0.15, 0.05])
    dev = dev_of(host)
    for nd in (b"a", b"ab", b"aba", b"abab", b"b" * 5):
        s = make(ss, nd)
        before = s.tuning_state(dev)
        every = s.find_all(dev).cpu().numpy()
        kept = s.find_all(dev, whole_word=True).cpu().numpy()
        assert s.count(dev, whole_word=True) == kept.size <= s.count(dev) == every.size
        n = len(nd)
        left = np.where(every > 0, host[np.maximum(every - 1, 0)], ord(" "))
        right = np.where(every + n < L, host[np.minimum(every + n, L - 1)], ord(" "))
        assert (kept == every[~_WORD[left] & ~_WORD[right]]).all() and kept.size > 0
        x, w, a = s.count_lines(dev, whole_line=True), s.count_lines(dev, whole_word=True), s.count_lines(dev)
        assert x <= w <= a and w > 0
        out = torch.full((3,), SENT, dtype=torch.int64, device="cuda")
        s.count_async(dev, out[1:2], whole_word=True)
        torch.cuda.synchronize()
        assert out.cpu().tolist() == [SENT, kept.size, SENT]
        s.count_lines_async(dev, out[1:2], whole_line=True)
        torch.cuda.synchronize()
        assert out.cpu().tolist() == [SENT, x, SENT]
        assert s.tuning_state(dev) == before, nd


def test_every_refusal_writes_nothing(ss):
    text = np.frombuffer(b"abc abc\nabc", dtype=np.uint8)
    d = dev_of(text)
    s, empty, upper = make(ss, b"abc"), make(ss, b""), make(ss, b"Abc")
    W, X, I = ss.searcher.SS_BOUND_WORD, ss.searcher.SS_BOUND_LINE, ss.searcher.SS_BOUND_NOCASE
    with bounded_lib(ss):
        L = ss.lib()
    out = Window(4)
    st = torch.cuda.current_stream().cuda_stream

    def forms(h, how, c):
        """the six entry points with `how`, by name; host results go to `c`, device results into the window"""
        p, n, o = d.data_ptr(), d.numel(), out.view.data_ptr()
        return {"count": lambda: L.ss_count_bounded_device(h, p, n, how, st, ctypes.byref(c)),
                "count_async": lambda: L.ss_count_bounded_device_async(h, p, n, how, st, o),
                "find_all": lambda: L.ss_find_all_bounded_device(h, p, n, how, st, o, 4, ctypes.byref(c)),
                "count_lines": lambda: L.ss_count_lines_bounded_device(h, p, n, 10, how, st, ctypes.byref(c)),
                "count_lines_async": lambda: L.ss_count_lines_bounded_device_async(h, p, n, 10, how, st, o),
                "find_lines": lambda: L.ss_find_lines_bounded_device(h, p, n, 10, how, st, o, None, None, 4, ctypes.byref(c))}

    def refused(h, how, only=None, match=()):
        c = ctypes.c_uint64(0xA5A5)
        for name, call in forms(h, how, c).items():
            if only is not None and name not in only:
                continue
            rc = call()
            msg = L.ss_last_error().decode()
            assert rc == ss.SS_ERR_ARGUMENT and c.value == 0xA5A5, (name, how, rc, c.value)
            for m in match:
                assert m in msg, (name, how, msg)
            assert name.split("_")[0] in msg and "bounded" in msg, (name, msg)
        torch.cuda.synchronize()
        out.check([], ("refusal", how))

    occurrence = ("count", "count_async", "find_all")
    refused(s._h, 0, match=("neither",))
    refused(s._h, 0, only=occurrence, match=("ss_count_device",))
    refused(s._h, 0, only=("count_lines", "find_lines"), match=("ss_count_lines_device",))
    refused(s._h, I, only=occurrence, match=("ss_count_nocase_device",))
    refused(s._h, I, only=("count_lines",), match=("ss_count_lines_nocase_device",))
    refused(s._h, W | X, match=("both",))
    refused(s._h, W | X | I, match=("both",))
    refused(s._h, X, only=occurrence, match=("SS_BOUND_LINE", "lines"))
    refused(s._h, X | I, only=occurrence, match=("SS_BOUND_LINE",))
    for how in (8, W | 8, X | 0x100, 0x80000000 | W):
        refused(s._h, how, match=("bits",))
    refused(empty._h, W, match=("empty needle",))
    refused(empty._h, X, only=("count_lines", "count_lines_async", "find_lines"), match=("empty needle",))
    refused(upper._h, W | I, match=("ss_searcher_new_nocase",))
    refused(upper._h, X | I, only=("count_lines", "find_lines"), match=("ss_searcher_new_nocase",))
    # ... and the Python keywords raise what the library says
    with pytest.raises(ss.SlicesliceError, match="both") as e:
        s.count_lines(d, whole_word=True, whole_line=True)
    assert e.value.code == ss.SS_ERR_ARGUMENT
    with pytest.raises(ss.SlicesliceError, match="empty needle"):
        empty.count(d, whole_word=True)
    with pytest.raises(ss.SlicesliceError, match="ss_searcher_new_nocase"):
        upper.find_all(d, ignore_case=True, whole_word=True)
    # the same searchers are taken where the rule allows them
    assert upper.count(d, whole_word=True) == 0 and s.count(d, whole_word=True) == 3 and s.count_lines(d, whole_line=True) == 1
    # n > len gives 0; the models' own refusals stay theirs
    assert make(ss, b"abc abc\nabcd").count(d, whole_word=True) == 0 == make(ss, b"abc abc\nabcd").count_lines(d, whole_line=True)
    with pytest.raises(ss.SlicesliceError, match="delimiter"):
        s.count_lines(d, 256, whole_word=True)


def test_a_160_mib_haystack_of_40_chunks_at_one_tile_per_workgroup(ss):
    n_bytes = 160 * MiB                                     # (one tile per workgroup; the size of tests/test_gpu_nocase.py's test of this name)
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x0B0D)
    hay.masked_fill_(hay == ord("Q"), ord("r"))
    hay.masked_fill_(hay == ord("q"), ord("r"))
    rng = np.random.default_rng(76)
    needle = b"quite a long needle, 33 bytes: qz"
    s, s2 = make(ss, needle), make(ss, b"qz")
    # the shape this size really has (the launch rules as tests/test_gpu_matches.py restates them): 10,240 tiles, ONE per workgroup
    # - two begin at 2 * CUs * 256 tiles, 2 GiB on 256 CUs - and 10,242 parts, so lines_chunk_kernel has 40 full chunks and the
    # combine walks them.  Two-tile grids, chunk borders on purpose and runs of chunks: tests/test_gpu_lines_grids.py.
    cus = ss.device_info()["compute_units"]
    ntiles = n_tiles(s.device_triple()[0] % 16, n_bytes, len(needle))
    assert tiles_per_workgroup(ntiles, cus, 0) == 1 and ntiles + 2 > 256 and (ntiles + 2) // 256 == 40
    n = len(needle)
    spots = sorted({TILE - 5, 2 * TILE - 1, 64 * MiB - 16, 64 * MiB + 1, n_bytes - n - 1} |
                   {int(x) for x in rng.integers(1, n_bytes - 100, size=300)})
    for k, p in enumerate(spots):
        # dense runs of copies: blank between them (kept), glued together or to a word byte (not kept)
        copy = np.concatenate((np.frombuffer(b"w" if k % 3 == 0 else b" ", dtype=np.uint8), mixed_case(rng, needle) if k % 2 else
                               np.frombuffer(needle, dtype=np.uint8), np.frombuffer(b"_" if k % 5 == 0 else b"\n", dtype=np.uint8)))
        hay[p - 1:p + n + 1] = torch.from_numpy(copy).cuda()
    hay[:n] = torch.from_numpy(np.frombuffer(needle, dtype=np.uint8).copy()).cuda()         # p == 0
    hay[n] = ord(".")
    host = hay.cpu().numpy()
    before = s.tuning_state(hay)
    for sr, nd in ((s, needle), (s2, b"qz")):
        want = check_offsets(sr, hay, host, nd, False, "large")
        assert 50 < want.size < ref_offsets(host, nd).size
        check_lines(sr, hay, host, nd, 10, False, "large")
    folded = check_offsets(s, hay, host, needle, True, "large")         # (the folding unit: the long needle)
    assert want.size < folded.size or folded.size > 100
    check_lines(s, hay, host, needle, 10, True, "large", modes=(False,))
    assert s.tuning_state(hay) == before
    # the async forms on a side stream; the lines form refuses a capturing stream, naming itself
    side = torch.cuda.Stream()
    out = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s.count_async(hay, out[1:2], ignore_case=True, whole_word=True)
        s.count_lines_async(hay, out[2:3], whole_word=True)
    side.synchronize()
    assert out.cpu().tolist() == [SENT, folded.size, ref_lines(host, needle, 10, False, False)[0].size, SENT]
    del hay
    torch.cuda.empty_cache()


def test_offsets_above_2_32(ss):
    """dense kept and not-kept copies around 2^32 and at the end of a haystack that cannot match elsewhere (the way
    tools/fuzz_matches.py does its large mode): the reference is built from host copies of the planted regions and of the
    delimiters' positions alone"""
    n_bytes = (1 << 32) + 64 * MiB
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x0B32)
    step = 1 << 30
    for lo in range(0, n_bytes, step):                      # (in slices: the masks are temporaries of the slice's size)
        part = hay[lo:lo + step]
        part.masked_fill_(part == ord("q"), ord("r"))
    needle = b"qz-needle"
    n = len(needle)
    seps = [b" ", b"_", b"", b"\n", b"\n", b"k", b".", b"7", b" "]       # (two of nine copies are words, one of them a whole line)
    run = b"".join(seps[k % len(seps)] + needle for k in range(60)) + b"\n"
    starts = [(1 << 32) - 2000, (1 << 32) - len(run) // 2, (1 << 32) + 1000, (1 << 32) + 3 * TILE - 100, n_bytes - len(run) - 40]
    assert len(run) + 16 < 1000 - len(run) // 2             # (the regions and the windows around them do not overlap)
    tail = b" " + needle                                    # ... and p + n == len
    kept, whole = [], []
    for p0, text in [(p, run) for p in starts] + [(n_bytes - len(tail), tail)]:
        hay[p0:p0 + len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    for p0, text in [(p, run) for p in starts] + [(n_bytes - len(tail), tail)]:
        lo, hi = p0 - 8, min(p0 + len(text) + 8, n_bytes)   # (the margins hold no 'q': no occurrence touches a window's edge but the view's end)
        window = hay[lo:hi].cpu().numpy()
        kept.append(ref_kept(window, needle, False, False, None) + lo)
        whole.append(ref_kept(window, needle, False, True, 10) + lo)
    kept, whole = np.concatenate(kept), np.concatenate(whole)
    assert (np.diff(kept) > 0).all() and (np.diff(whole) > 0).all()
    assert kept.size > 50 and whole.size >= 5 and kept.min() < (1 << 32) < kept.max() and kept[-1] == n_bytes - n
    dpos = np.concatenate([(torch.nonzero(hay[lo:lo + step] == 10).flatten() + lo).cpu().numpy() for lo in range(0, n_bytes, step)])

    def lines_of(offs):
        k = np.unique(np.searchsorted(dpos, offs, side="left"))
        begins = np.where(k > 0, dpos[np.maximum(k - 1, 0)] + 1, 0)
        ends = np.where(k < dpos.size, dpos[np.minimum(k, dpos.size - 1)], n_bytes)
        return begins, ends, k + 1

    s = make(ss, needle)
    assert s.count(hay, whole_word=True) == kept.size < s.count(hay)
    w = Window(kept.size)
    assert s.find_all_into(hay, w.view, whole_word=True) == kept.size
    w.check(kept, "above 2^32")
    for offs, kw in ((kept, dict(whole_word=True)), (whole, dict(whole_line=True))):
        want = lines_of(offs)
        assert s.count_lines(hay, **kw) == want[0].size, kw
        ws = [Window(want[0].size) for _ in range(3)]
        assert s.find_lines_into(hay, ws[0].view, ws[1].view, ws[2].view, want[0].size, **kw) == want[0].size, kw
        for win, ref in zip(ws, want):
            win.check(ref, ("above 2^32", kw))
    del hay, part
    torch.cuda.empty_cache()


def test_the_async_count_replays_from_a_graph(ss):
    """a single-branch graph: one captured ss_count_bounded_device_async, replayed twice"""
    rng = np.random.default_rng(77)
    host = rng.choice(np.frombuffer(b"ab \n", dtype=np.uint8), size=3 * TILE + 7)
    dev = dev_of(host)
    s = make(ss, b"ab")
    want = ref_kept(host, b"ab", False, False, None).size
    cap = torch.zeros(1, dtype=torch.int64, device="cuda")
    lines = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
    s.count_async(dev, cap, whole_word=True)               # (first use outside the capture: the needle's device copy exists)
    torch.cuda.synchronize()
    assert cap.item() == want > 0
    g = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.graph(g):
        s.count_async(dev, cap, whole_word=True)
        try:
            s.count_lines_async(dev, lines, whole_word=True)
        except ss.SlicesliceError as err:
            refused = err
    assert refused is not None and refused.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(refused) and "bounded" in str(refused), refused
    for _ in range(2):
        cap.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert cap.item() == want
    assert lines.item() == SENT
