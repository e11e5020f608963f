"""GPU tests of the calls that ignore ASCII case (include/sliceslice_hip_nocase.h, libsliceslice_hip_nocase.so): ss_count_nocase_device /
_async, ss_find_all_nocase_device, ss_count_lines_nocase_device / _async and ss_find_lines_nocase_device against the rule restated
in Python - ``bytes.lower()`` on the haystack and on the needle, then the overlapping-occurrence and matching-lines restatements
of tests/test_gpu_matches.py and tests/test_gpu_lines.py, the line cut made on the UNFOLDED bytes - and against
tests/golden/nocase_kat.json.  Every comparison is of integers and exact."""
import hashlib
import json
import os
import struct

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
_LOWER = np.frombuffer(bytes(range(256)).lower(), dtype=np.uint8)
# what differs from a letter without being its other case: the neighbours of the two ranges, and bit 7 over a letter pattern
SPOILERS = {ord("a"): (ord("`"), ord("@"), 0xC1, 0xE1), ord("z"): (ord("{"), ord("["), 0xDA, 0xFA), ord("m"): (0xCD, 0xED, ord("-"), ord("M") ^ 0x40)}


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with nocase_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "nocase_kat.json")))


@pytest.fixture(scope="module")
def manual():
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    return data, torch.from_numpy(data.copy()).cuda()


def nocase_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the nocase entry points (another build of
    libsliceslice_hip_nocase.so), else `ss.nocase_build()`."""
    return _loaded() if getattr(ss.lib(), "has_nocase", False) else ss.nocase_build()


def make(ss, needle, position=None, triple=None, raw=False):
    """new_nocase(needle); or - position / triple / raw - the ordinary constructors on a needle that holds no upper-case byte"""
    with nocase_lib(ss):
        if position is None and triple is None and not raw:
            return ss.DynamicHipSearcher.new_nocase(needle)
        s = ss.DynamicHipSearcher(needle, position)
        if triple is not None:
            s.set_filter(*triple)
        return s


def lower(h):
    return _LOWER[np.asarray(h, dtype=np.uint8)]


def ref_all(h, needle):
    return ref_offsets(lower(h), bytes(needle).lower())


def ref_lines(h, needle, delim):
    """(begin, end, number) of the lines of h - cut at `delim` on the bytes as they are - that hold the needle ignoring case; a
    searcher's needle is the folded one, and one that holds the delimiter matches no line."""
    h = np.asarray(h, dtype=np.uint8)
    needle = bytes(needle).lower()
    L = h.size
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, L, dtype=np.int64)))
    if begins[-1] == L:
        begins, ends = begins[:-1], ends[:-1]
    if len(needle) == 0:
        k = np.arange(begins.size, dtype=np.int64)
    elif delim in needle:
        k = np.zeros(0, dtype=np.int64)
    else:
        offs = ref_offsets(lower(h), needle)
        # an occurrence must not run over a delimiter (a delimiter that is an upper-case letter folds onto a needle byte)
        first = np.searchsorted(dpos, offs, side="left")
        inside = np.searchsorted(dpos, offs + len(needle) - 1, side="right") == first
        k = np.unique(first[inside]).astype(np.int64)
    return begins[k], ends[k], k + 1


def dev_of(host):
    host = np.asarray(host, dtype=np.uint8)
    return torch.from_numpy(host.copy()).cuda() if host.size else torch.empty(0, dtype=torch.uint8, device="cuda")


def check(s, hay_dev, hay_host, needle, delims=(10,), what=""):
    """count, find_all, count_lines and find_lines ignoring case against the rule; returns the offsets"""
    want = ref_all(hay_host, needle)
    got = s.count(hay_dev, ignore_case=True)
    assert got == want.size, (what, needle[:32], got, want.size)
    offs = s.find_all(hay_dev, ignore_case=True).cpu().numpy()
    assert offs.size == want.size and (offs == want).all(), (what, needle[:32], offs[:8], want[:8])
    for delim in delims:
        wb, we, wn = ref_lines(hay_host, needle, delim)
        got = s.count_lines(hay_dev, delim, ignore_case=True)
        assert got == wb.size, (what, needle[:32], delim, got, wb.size)
        b, e, n = (t.cpu().numpy() for t in s.find_lines(hay_dev, delim, ignore_case=True))
        assert b.size == wb.size and (b == wb).all() and (e == we).all() and (n == wn).all(), \
            (what, needle[:32], delim, b[:6], e[:6], n[:6], wb[:6], we[:6], wn[:6])
    return want


def mixed_case(rng, needle):
    """a copy of the needle with every letter in a random case"""
    nb = np.frombuffer(bytes(needle), dtype=np.uint8).copy()
    letters = (nb >= 0x61) & (nb <= 0x7A)
    nb[letters & (rng.random(nb.size) < 0.5)] ^= 0x20
    return nb


def spoiled(rng, needle, at=None):
    """a copy in mixed case in which ONE byte (a letter of the needle) is replaced by a byte that is not its other case"""
    nb = mixed_case(rng, needle)
    low = np.frombuffer(bytes(needle), dtype=np.uint8)
    spots = [k for k in range(nb.size) if int(low[k]) in SPOILERS] if at is None else [at]
    k = spots[int(rng.integers(len(spots)))]
    choices = SPOILERS[int(low[k])]
    nb[k] = choices[int(rng.integers(len(choices)))]
    return nb


def test_only_the_nocase_library_has_the_entry_points(ss):
    with ss.lines_build() as L:
        assert not L.has_nocase
    with ss.nocase_build() as L:
        assert L.has_nocase and L.has_lines and L.has_matches and not L.has_matches_batched
    s = make(ss, b"MiXed Case 42")
    assert s.needle == b"mixed case 42" == ss.fold_ascii(b"MiXed Case 42")
    with ss.lines_build():
        t = ss.DynamicHipSearcher(b"abc")
    d = dev_of(np.frombuffer(b"abc", dtype=np.uint8))
    with pytest.raises(ss.SlicesliceError, match="nocase_build"):
        t.count(d, ignore_case=True)


def test_the_small_case_table(ss, kat):
    for c in kat["cases"]:
        hay, needle = bytes.fromhex(c["haystack"]), bytes.fromhex(c["needle"])
        s = make(ss, needle)
        d = dev_of(np.frombuffer(hay, dtype=np.uint8))
        assert s.count(d, ignore_case=True) == len(c["offsets"]), c["what"]
        assert s.find_all(d, ignore_case=True).cpu().tolist() == c["offsets"], c["what"]
        assert s.count_lines(d, c["delimiter"], ignore_case=True) == len(c["records"]), c["what"]
        b, e, n = (t.cpu().tolist() for t in s.find_lines(d, bytes([c["delimiter"]]), ignore_case=True))
        assert [list(r) for r in zip(b, e, n)] == c["records"], (c["what"], b, e, n)
        # ... and the restatement of this file agrees with the fixture
        h = np.frombuffer(hay, dtype=np.uint8)
        assert ref_all(h, needle).tolist() == c["offsets"], c["what"]
        assert [list(r) for r in zip(*(a.tolist() for a in ref_lines(h, needle, c["delimiter"])))] == c["records"], c["what"]


def test_every_word_of_the_manual(ss, kat, manual):
    data, d = manual
    words = open(os.path.join(GOLDEN, "data", "words.txt"), "rb").read().split()
    assert len(words) == kat["words"] == 4585
    searchers = [make(ss, w) for w in words]
    got = [s.count(d, ignore_case=True) for s in searchers]
    bad = [(w, g, k) for w, g, k in zip(words, got, kat["count"]) if g != k]
    assert not bad, bad[:10]
    got = [s.count_lines(d, ignore_case=True) for s in searchers]
    bad = [(w, g, k) for w, g, k in zip(words, got, kat["count_lines"]) if g != k]
    assert not bad, bad[:10]
    assert sum(got) == kat["total_lines"]
    for w, t in kat["table"].items():
        s = make(ss, w.encode())
        assert (s.count(d), s.count(d, ignore_case=True)) == (t["count"], t["count_nocase"]), w
        assert (s.count_lines(d), s.count_lines(d, ignore_case=True)) == (t["lines"], t["lines_nocase"]), w


def test_records_of_chosen_words_with_capacity_cuts_and_sentinels(ss, kat, manual):
    data, d = manual
    assert len(kat["records"]) >= 50
    for j, (w, want) in enumerate(kat["records"].items()):
        needle = w.encode("latin-1")
        s = make(ss, needle)
        offs = s.find_all(d, ignore_case=True).cpu().tolist()
        assert len(offs) == want["count"], w
        assert hashlib.sha256(b"".join(struct.pack("<Q", o) for o in offs)).hexdigest() == want["offsets_sha256"], w
        b, e, n = (t.cpu().tolist() for t in s.find_lines(d, ignore_case=True))
        assert len(b) == want["lines"], w
        assert hashlib.sha256(b"".join(struct.pack("<3Q", *r) for r in zip(b, e, n))).hexdigest() == want["records_sha256"], w
        if j % 4:
            continue
        # capacity cuts: windows of larger buffers whose sentinels on both sides must survive
        for total, cap in ((want["count"], c) for c in (1, max(want["count"] - 1, 0), want["count"] + 3)):
            buf = torch.full((cap + 16,), SENT, dtype=torch.int64, device="cuda")
            assert s.find_all_into(d, buf[8:8 + cap], ignore_case=True) == total, (w, cap)
            h = buf.cpu().numpy()
            k = min(cap, total)
            assert (h[:8] == SENT).all() and (h[8 + k:] == SENT).all() and h[8:8 + k].tolist() == offs[:k], (w, cap)
        for total, cap in ((want["lines"], c) for c in (0, 1, max(want["lines"] - 1, 0), want["lines"] + 3)):
            for skip in (None, 1):
                bufs = [torch.full((cap + 16,), SENT, dtype=torch.int64, device="cuda") for _ in range(3)]
                args = [None if (k == skip or cap == 0) else bufs[k][8:8 + cap] for k in range(3)]
                assert s.find_lines_into(d, args[0], args[1], args[2], cap, ignore_case=True) == total, (w, cap)
                k = min(cap, total)
                for i, ref in enumerate((b, e, n)):
                    h = bufs[i].cpu().numpy()
                    assert (h[:8] == SENT).all() and (h[8 + k:] == SENT).all(), (w, cap, skip, i)
                    if i == skip or cap == 0:
                        assert (h == SENT).all(), (w, cap, skip, i)
                    else:
                        assert h[8:8 + k].tolist() == ref[:k], (w, cap, skip, i)
    s = make(ss, b"Intel")
    assert s.find_all(d, capacity=1, ignore_case=True).cpu().tolist() == ref_all(data, b"intel")[:1].tolist()   # "is it there, where first"


# needle lengths for every verify path: the one-byte test (1), the in-register exact compare (2..16), the LDS compare (17..2048),
# the global continuation (> 2048)
LENGTHS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 18, 31, 33, 64, 100, 1000, 2047, 2048, 2049, 2500, 3000]


def needle_of(rng, n):
    """n bytes: letters a, z, m (which have spoilers) among other lower-case letters, digits and punctuation - no upper case"""
    alphabet = np.frombuffer(b"azmazmazmetnor 0189_-.{`@[", dtype=np.uint8)
    nb = rng.choice(alphabet, size=n)
    nb[0] = ord("a")
    nb[-1] = ord("z") if n > 1 else nb[-1]
    return nb.tobytes()


def test_needle_lengths_and_verify_paths_with_spoiled_copies_across_borders(ss):
    rng = np.random.default_rng(59)
    L = 4 * TILE + 777
    G = 4096
    for n in LENGTHS:
        needle = needle_of(rng, n)
        if n == 1:
            cases = [(b"a", make(ss, b"A")), (b"{", make(ss, b"{")), (b"7", make(ss, b"7"))]       # a letter, two non-letters
        else:
            cases = [(needle, make(ss, mixed_case(rng, needle).tobytes()))]
        for nd, s in cases:
            assert s.needle == nd
            nl = len(nd)
            for mis in (0, 7, 15):
                host = rng.choice(np.frombuffer(b"qQ#\n\x00\xff \xe1[@", dtype=np.uint8), size=L + 2 * G)
                v0 = G + mis
                # copies differing only in case - and spoiled ones next to them - across the borders of a 16-byte chunk, a 1 KiB piece and
                # a 16 KiB tile (border taken relative to the view, the kernels' pieces relative to the aligned base: both kinds occur)
                planted = 0
                at = v0 + 40
                for border in (1024 + 16, 2048, 3 * 1024, TILE, TILE + 4096, 2 * TILE, 3 * TILE):
                    for delta in (-(nl // 2), -1, 0, -nl + 1):
                        p = max(v0 + border + delta, at)
                        if p + 2 * nl + 8 > v0 + L:
                            continue
                        host[p:p + nl] = mixed_case(rng, nd)
                        planted += 1
                        if any(b in SPOILERS for b in nd):
                            host[p + nl + 3:p + 2 * nl + 3] = spoiled(rng, nd)
                        at = p + 2 * nl + 8
                # (views: spoiled copies and true copies just outside both ends must not count; copies straddling the ends neither)
                if nl > 1:
                    host[v0 - nl:v0] = mixed_case(rng, nd)
                    host[v0 + L:v0 + L + nl] = mixed_case(rng, nd)
                    host[v0 - nl - 20:v0 - 20] = spoiled(rng, nd) if any(b in SPOILERS for b in nd) else mixed_case(rng, nd)
                else:
                    host[v0 - 1] = nd[0] ^ (0x20 if nd.isalpha() else 0)
                    host[v0 + L] = nd[0]
                dev = dev_of(host)
                assert dev.data_ptr() % 16 == 0
                want = check(s, dev[v0:v0 + L], host[v0:v0 + L], nd, (10, 0, 255), "n %d mis %d" % (nl, mis))
                assert want.size >= planted > 0, (nl, mis, want.size, planted)
                # the case-sensitive calls of the same (folded) searcher: the rule on the folded needle WITHOUT the haystack fold
                view = host[v0:v0 + L]
                assert s.count(dev[v0:v0 + L]) == ref_offsets(view, nd).size <= want.size


def test_every_spoiler_byte_for_every_verify_path(ss):
    """haystacks in which the ONLY difference between a match and a non-match is '@' '[' '`' '{' or a byte with bit 7 set over a
    letter pattern, at every index of the needle that holds such a letter"""
    rng = np.random.default_rng(60)
    for n in (1, 2, 7, 16, 17, 40, 2049, 2300):
        needle = (b"az" * (n // 2 + 1))[:n]
        s = make(ss, needle.upper())
        assert s.needle == needle
        step = n + 5
        idx = sorted(set(range(min(n, 24))) | {n - 1, n // 2} | ({2047, 2048, n - 2} if n > 2048 else set()))
        variants = []
        for k in idx:
            for sp in SPOILERS[needle[k]]:
                v = mixed_case(rng, needle)
                v[k] = sp
                variants.append(v)
            v = np.frombuffer(needle, dtype=np.uint8).copy()
            v[k] ^= 0x20                                        # the other case: a match
            variants.append(v)
        host = np.full(64 + step * len(variants) + 64, ord("#"), dtype=np.uint8)
        for j, v in enumerate(variants):
            host[64 + j * step:64 + j * step + n] = v
        dev = dev_of(host)
        want = check(s, dev, host, needle, (10, ord("#")), "spoilers n %d" % n)
        assert want.size == len(idx), (n, want.size, len(idx))


def test_filter_shapes_mode2_and_the_far_byte(ss):
    rng = np.random.default_rng(61)
    L = 6 * TILE + 321
    # MODE 2 via with_position on a folded needle; set_filter3 pairs: every MODE 2 window, and one far enough apart (>= 16 * 63)
    # that the device filters near the first byte and tests the far byte in memory first (far_off)
    base = needle_of(rng, 1400)
    rows = [("with_position 20", base[:48], dict(position=20)), ("with_position 47", base[:48], dict(position=47)),
            ("mode2 q0", base[:48], dict(triple=(0, 16, 16))), ("mode2 q1", base[:48], dict(triple=(3, 23, 23))),
            ("mode2 q2", base[:60], dict(triple=(0, 40, 40))), ("mode2 q3", base[:48], dict(triple=(5, 33, 33))),
            ("mode0 q3 first at 2", base[:40], dict(triple=(2, 3, 15))), ("pair alone d=3", base[:70], dict(triple=(1, 61, 61))),
            ("far_off", base, dict(triple=(0, 1300, 1300))), ("far_off from 5", base, dict(triple=(5, 1399, 1399)))]
    kernels = set()
    for name, nd, kw in rows:
        s = make(ss, nd, **kw)
        kernels.add(kernel_of(s))
        nl = len(nd)
        host = rng.choice(np.frombuffer(b"azmAZM \n", dtype=np.uint8), size=L + 64)
        at = 100
        while at + 2 * nl + 64 < L:
            host[at:at + nl] = mixed_case(rng, nd)
            sp = spoiled(rng, nd, at=kw["triple"][1] if "triple" in kw and nd[kw["triple"][1]] in SPOILERS else None)
            host[at + nl + 9:at + 2 * nl + 9] = sp
            at += 2 * nl + int(rng.integers(20, 3000))
        for mis in (0, 11):
            dev = dev_of(host)
            want = check(s, dev[mis:mis + L], host[mis:mis + L], nd, (10,), "%s mis %d" % (name, mis))
            assert want.size >= 3, (name, want.size)
    assert {m for _, m, _ in kernels} == {0, 2}, kernels


def test_views_with_spoiled_copies_just_outside_both_ends(ss):
    rng = np.random.default_rng(62)
    G = 64
    pool = np.frombuffer(b"aAbB\n", dtype=np.uint8)
    searchers = [(nd, make(ss, nd.upper())) for nd in (b"ab", b"abab", b"a", b"")]
    for mis in range(16):
        for L in (0, 1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 16):
            host = rng.choice(pool, size=L + 2 * G, p=[0.225, 0.225, 0.225, 0.225, 0.1])
            v0 = G + mis
            host[v0 - 5:v0] = np.frombuffer(b"\nAbaB", dtype=np.uint8)          # copies immediately outside, straddling both ends
            host[v0 + L:v0 + L + 5] = np.frombuffer(b"aBAb\n", dtype=np.uint8)
            if mis % 2:
                host[v0 - 1] = ord("@")                                         # spoiled: '@b' is not 'ab'
                host[v0 + L] = 0xE1
            dev = dev_of(host)
            for nd, s in searchers:
                check(s, dev[v0:v0 + L], host[v0:v0 + L], nd, (10, ord("A")) if mis % 4 == 0 else (10,), "mis %d len %d" % (mis, L))


def test_delimiters_that_are_letters(ss):
    rng = np.random.default_rng(63)
    L = 3 * TILE + 99
    host = rng.choice(np.frombuffer(b"aAbBxX\n\x00\xff", dtype=np.uint8), size=L)
    dev = dev_of(host)
    for nd in (b"a", b"ab", b"xb", b"bxa", b"xxbb" * 5, b"b" * 17):
        s = make(ss, nd.upper())
        # delimiter 'A' cuts at 'A' only: needle bytes 'a' still match inside the lines; a needle that holds the delimiter matches none
        for delim in (ord("A"), ord("a"), ord("X"), 0, 255, 10):
            wb, we, wn = ref_lines(host, nd, delim)
            assert s.count_lines(dev, delim, ignore_case=True) == wb.size, (nd, delim)
            b, e, n = (t.cpu().numpy() for t in s.find_lines(dev, delim, ignore_case=True))
            assert (b == wb).all() and (e == we).all() and (n == wn).all(), (nd, delim)
            if delim in nd:
                assert wb.size == 0
            elif delim in nd.upper() and len(nd) <= 2:
                assert wb.size > 0, (nd, delim)             # only the delimiter's other case: can match, and does here
    # the line structure is the unfolded one: as many lines as the case-sensitive empty needle counts
    e = make(ss, b"")
    for delim in (ord("A"), ord("a")):
        assert e.count_lines(dev, delim, ignore_case=True) == e.count_lines(dev, delim) == ref_lines(host, b"", delim)[0].size


def test_a_160_mib_haystack_of_40_chunks_at_one_tile_per_workgroup(ss):
    n_bytes = 160 * MiB                                     # (one tile per workgroup; tests/test_gpu_bounded.py and test_gpu_inverted.py use the same size)
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x0CA5E)
    hay.masked_fill_(hay == ord("Q"), ord("r"))
    hay.masked_fill_(hay == ord("q"), ord("r"))
    rng = np.random.default_rng(64)
    needle = b"quite a long needle, 33 bytes: qz"
    s, s2 = make(ss, needle.upper()), make(ss, b"qz")
    # the shape this size really has (the launch rules as tests/test_gpu_matches.py restates them): 10,240 tiles, ONE per workgroup
    # - two begin at 2 * CUs * 256 tiles, 2 GiB on 256 CUs - and 10,242 parts, so lines_chunk_kernel has 40 full chunks and the
    # combine walks them.  Two-tile grids, chunk borders on purpose and runs of chunks: tests/test_gpu_lines_grids.py.
    cus = ss.device_info()["compute_units"]
    ntiles = n_tiles(s.device_triple()[0] % 16, n_bytes, len(needle))
    assert tiles_per_workgroup(ntiles, cus, 0) == 1 and ntiles + 2 > 256 and (ntiles + 2) // 256 == 40
    spots = sorted({0, 1, TILE - 5, 2 * TILE - 1, 64 * MiB - 16, 64 * MiB + 1, n_bytes - len(needle)} |
                   {int(x) for x in rng.integers(0, n_bytes - 100, size=300)})
    regions = []
    for k, p in enumerate(spots):
        v = spoiled(rng, needle, at=len(needle) - 1) if k % 3 == 2 else mixed_case(rng, needle)
        hay[p:p + len(needle)] = torch.from_numpy(v).cuda()
        regions.append(p)
    host = hay.cpu().numpy()
    before = s.tuning_state(hay)
    for sr, nd in ((s, needle), (s2, b"qz")):
        want = ref_all(host, nd)
        assert sr.count(hay, ignore_case=True) == want.size > 150
        assert (sr.find_all(hay, ignore_case=True).cpu().numpy() == want).all()
        wb, we, wn = ref_lines(host, nd, 10)
        assert sr.count_lines(hay, ignore_case=True) == wb.size
        b, e, n = (t.cpu().numpy() for t in sr.find_lines(hay, ignore_case=True))
        assert (b == wb).all() and (e == we).all() and (n == wn).all()
    # the calls neither start nor feed the census
    assert s.tuning_state(hay) == before
    # async forms on a side stream; the count form is capturable, the lines form refuses a capturing stream
    side = torch.cuda.Stream()
    out = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s.count_async(hay, out[1:2], ignore_case=True)
        s.count_lines_async(hay, out[2:3], ignore_case=True)
    side.synchronize()
    assert out.cpu().tolist() == [SENT, ref_all(host, needle).size, ref_lines(host, needle, 10)[0].size, SENT]
    g = torch.cuda.CUDAGraph()
    refused = None
    cap = torch.zeros(1, dtype=torch.int64, device="cuda")
    with torch.cuda.graph(g):
        s.count_async(hay, cap, ignore_case=True)
        try:
            s.count_lines_async(hay, out[2:3], ignore_case=True)
        except ss.SlicesliceError as err:
            refused = err
    assert refused is not None and refused.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(refused) and "nocase" in str(refused), refused
    cap.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert cap.item() == ref_all(host, needle).size
    assert s.tuning_state(hay) == before
    del hay
    torch.cuda.empty_cache()


def test_a_needle_with_an_upper_case_byte_is_refused(ss):
    text = np.frombuffer(b"abc ABC Abc abC Zz", dtype=np.uint8)
    d = dev_of(text)
    out = torch.zeros(4, dtype=torch.int64, device="cuda")
    for needle in (b"Abc", b"abC", b"Z", b"a" * 2100 + b"Q"):
        s = make(ss, needle, raw=True)
        calls = [lambda: s.count(d, ignore_case=True), lambda: s.count_async(d, out[0:1], ignore_case=True),
                 lambda: s.find_all(d, ignore_case=True), lambda: s.find_all_into(d, out, ignore_case=True),
                 lambda: s.count_lines(d, ignore_case=True), lambda: s.count_lines_async(d, out[0:1], ignore_case=True),
                 lambda: s.find_lines(d, ignore_case=True), lambda: s.find_lines_into(d, out, None, None, 4, ignore_case=True)]
        for call in calls:
            with pytest.raises(ss.SlicesliceError, match="ss_searcher_new_nocase") as info:
                call()
            assert info.value.code == ss.SS_ERR_ARGUMENT
        assert s.count(d) == ref_offsets(text, needle).size == (1 if len(needle) < 2100 else 0)     # the case-sensitive calls take it as ever
    # any constructor will do when the needle holds no upper-case byte: '@', '[', digits and bytes >= 0x80 are none
    for needle in (b"abc", b"@[`{", b"\xc1\xda"):
        assert make(ss, needle, raw=True).count(d, ignore_case=True) == ref_all(text, needle).size


def test_a_folded_searcher_used_case_sensitively(ss, manual):
    data, d = manual
    for w in (b"Descriptor", b"THE", b"Intel", b"GDT", b"A"):
        s = make(ss, w)
        nd = w.lower()
        assert s.needle == nd
        assert s.count(d) == ref_offsets(data, nd).size
        assert (s.find_all(d).cpu().numpy() == ref_offsets(data, nd)).all()
        from test_gpu_lines import ref_lines as ref_lines_sensitive
        wb, we, wn = ref_lines_sensitive(data, nd, 10)
        assert s.count_lines(d) == wb.size
        assert (s.find_lines(d)[0].cpu().numpy() == wb).all()
        assert s.search_in(d) == (ref_offsets(data, nd).size > 0)
        first = s.find(d)
        assert first == (int(ref_offsets(data, nd)[0]) if ref_offsets(data, nd).size else None)
        assert s.count(d, ignore_case=True) == ref_all(data, nd).size >= s.count(d)
