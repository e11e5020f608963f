"""GPU tests of every-occurrence search (include/sliceslice_hip_matches.h, libsliceslice_hip_matches.so): ss_count_device / _async
and ss_find_all_device against a naive overlapping candidate-and-verify restatement in numpy.  Offsets are compared, not just
counts."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = os.path.join(ROOT, "tests", "golden", "data")
MiB = 1 << 20


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with m.matches_build():
        pass
    return m


def ref_offsets(h, n):
    """Every i with h[i:i+len(n)] == n (overlapping), ascending."""
    h = np.asarray(h, dtype=np.uint8)
    n = np.frombuffer(bytes(n), dtype=np.uint8)
    L, m = h.size, n.size
    if m == 0:
        return np.arange(L + 1, dtype=np.int64)
    if m > L:
        return np.zeros(0, dtype=np.int64)
    cand = np.flatnonzero(h[:L - m + 1] == n[0])
    for k in range(1, m):
        if cand.size == 0:
            break
        cand = cand[h[cand + k] == n[k]]
    return cand.astype(np.int64)


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def matches_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the matches entry points (another build of
    libsliceslice_hip_matches.so), else `ss.matches_build()`."""
    return _loaded() if getattr(ss.lib(), "has_matches", False) else ss.matches_build()


def make(ss, needle, position=None, triple=None, memchr=False):
    with matches_lib(ss):
        if memchr:
            return ss.MemchrHipSearcher(needle[0])
        s = ss.DynamicHipSearcher(needle, position)
        if triple is not None:
            s.set_filter(*triple)
        return s


def check(s, hay_dev, hay_host, needle, what=""):
    want = ref_offsets(hay_host, needle)
    assert s.count(hay_dev) == want.size, (what, needle[:32], s.count(hay_dev), want.size)
    got = s.find_all(hay_dev).cpu().numpy()
    assert got.size == want.size and (got == want).all(), (what, needle[:32], got[:8], want[:8])


def test_the_product_library_has_no_matches_entry_points(ss):
    s = ss.DynamicHipSearcher.new(b"abc")          # outside matches_build(): the drop-in library
    with pytest.raises(ss.SlicesliceError, match="matches_build"):
        s.count(torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ss.SlicesliceError, match="matches_build"):
        s.find_all(torch.zeros(16, dtype=torch.uint8, device="cuda"))


def test_edge_cases(ss):
    dev = torch.zeros(0, dtype=torch.uint8, device="cuda")
    for needle, hay in [(b"", b""), (b"", b"abc"), (b"abcd", b"abc"), (b"abc", b"abc"), (b"abc", b"xabc"), (b"a", b""),
                        (b"aa", b"a" * 1000), (b"abab", b"ab" * 3000), (b"aaa", b"a" * 70000), (b"a", b"a" * 5000)]:
        h = np.frombuffer(hay, dtype=np.uint8).copy()
        d = torch.from_numpy(h).cuda() if h.size else dev
        check(make(ss, needle), d, h, needle, "edge")
    # host bytes are uploaded
    s = make(ss, b"aa")
    assert s.count(b"aaaa") == 3 and s.find_all(b"aaaa").cpu().tolist() == [0, 1, 2]
    assert make(ss, b"").count(b"abc") == 4 and make(ss, b"").find_all(b"abc").cpu().tolist() == [0, 1, 2, 3]


def test_one_byte_needles_both_searchers(ss):
    rng = np.random.default_rng(1)
    h = rng.integers(0, 8, size=3 * MiB + 77, dtype=np.uint8)
    d = torch.from_numpy(h).cuda()
    for b in (0, 3, 7, 200):
        check(make(ss, bytes([b])), d, h, bytes([b]), "dynamic")
        check(make(ss, bytes([b]), memchr=True), d, h, bytes([b]), "memchr")


def test_needle_lengths_and_misalignment(ss):
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, size=2 * MiB + 4096, dtype=np.uint8)
    big = torch.from_numpy(base).cuda()
    for k, n in enumerate((2, 3, 5, 8, 15, 16, 17, 31, 64, 100, 257, 1000, 2048, 3000)):
        mis = k % 16
        L = 2 * MiB - 999
        h = base[mis:mis + L].copy()
        needle = bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
        for p in rng.integers(0, L - n, size=9):
            h[p:p + n] = np.frombuffer(needle, dtype=np.uint8)
        h[L - n:] = np.frombuffer(needle, dtype=np.uint8)          # flush against len
        h[:n] = np.frombuffer(needle, dtype=np.uint8)
        big[mis:mis + L] = torch.from_numpy(h).cuda()
        check(make(ss, needle), big[mis:mis + L], h, needle, "n=%d mis=%d" % (n, mis))


def test_text_like_needles_that_overlap_themselves_at_every_border(ss):
    # dense matches: every piece (1 KiB), wave (4 KiB), tile / workgroup (16 KiB) border is crossed by some match
    for pat, needle in [(b"ab", b"abab"), (b"abc", b"abcabcab"), (b"xyz" * 5 + b"q", b"xyz" * 5 + b"qxyz"), (b"a", b"a" * 20)]:
        for mis in (0, 5, 13):
            h = np.frombuffer((pat * (MiB // len(pat) + 64))[mis:mis + MiB + 333], dtype=np.uint8).copy()
            check(make(ss, needle), torch.from_numpy(h).cuda(), h, needle, "dense %r" % pat)


@pytest.mark.parametrize("kind", ["exact16", "memory40", "with_position", "pair_d40", "far_pair"])
def test_needles_planted_around_borders(ss, kind):
    rng = np.random.default_rng(3)
    n = {"exact16": 13, "memory40": 40, "with_position": 24, "pair_d40": 64, "far_pair": 2000}[kind]
    needle = bytes(rng.integers(1, 256, size=n, dtype=np.uint8))
    s = make(ss, needle, position=17 if kind == "with_position" else None,
             triple={"pair_d40": (3, 43, 43), "far_pair": (0, 1500, 1500)}.get(kind))
    L = 4 * MiB + 123
    base = rng.integers(0, 256, size=L, dtype=np.uint8)
    borders = [1024 * 7, 4096 * 5, 16384 * 3, 16384 * 17 + 1024, 32768 * 9, 16384 * 101 + 4096 * 3]
    for delta in range(-n - 2, 3, 1 if n <= 64 else max(3, n // 40)):
        h = base.copy()
        for b in borders:
            h[b + delta:b + delta + n] = np.frombuffer(needle, dtype=np.uint8)
        h[L - n:] = np.frombuffer(needle, dtype=np.uint8)
        check(s, torch.from_numpy(h).cuda(), h, needle, "%s delta %d" % (kind, delta))


def test_filter_choices(ss):
    rng = np.random.default_rng(4)
    text = np.frombuffer(open(os.path.join(GD, "i386.txt"), "rb").read(), dtype=np.uint8)
    d = torch.from_numpy(text.copy()).cuda()
    for needle in (b"instruction", b"the", b"Intel Architecture", b"operand size attribute"):
        n = len(needle)
        for pos in (0, n // 2, n - 1):
            check(make(ss, needle, position=pos), d, text, needle, "with_position %d" % pos)
        for tri in ((0, 1, 2), (0, n - 1, n - 1), (1, min(n - 1, 15), 2)):
            check(make(ss, needle, triple=tri), d, text, needle, "triple %r" % (tri,))
    # d > 0 pairs (MODE 2) and a far caller byte on random bytes with plants
    h = rng.integers(0, 4, size=MiB + 5, dtype=np.uint8)
    long_needle = bytes(rng.integers(0, 4, size=1200, dtype=np.uint8))
    for p in (0, 999, 4000, 65536 - 7, MiB + 5 - 1200):
        h[p:p + 1200] = np.frombuffer(long_needle, dtype=np.uint8)
    dh = torch.from_numpy(h).cuda()
    for tri in ((0, 20, 20), (5, 700, 700), (0, 1199, 1199), (3, 10, 7)):
        check(make(ss, long_needle, triple=tri), dh, h, long_needle, "long triple %r" % (tri,))
    for tri in ((0, 17, 17), (1, 63, 63)):
        check(make(ss, long_needle[:64], triple=tri), dh, h, long_needle[:64], "pair %r" % (tri,))


def test_capacity_contract(ss):
    rng = np.random.default_rng(5)
    h = rng.integers(0, 3, size=MiB, dtype=np.uint8)
    d = torch.from_numpy(h).cuda()
    needle = b"\x01\x02\x00"
    s = make(ss, needle)
    want = ref_offsets(h, needle)
    total = want.size
    assert total > 1000
    for cap in (0, 1, total - 1, total, total + 1, 17):
        buf = torch.full((cap + 8,), -7, dtype=torch.int64, device="cuda")
        got = s.find_all_into(d, buf[:cap])
        assert got == total
        b = buf.cpu().numpy()
        k = min(cap, total)
        assert (b[:k] == want[:k]).all() and (b[k:] == -7).all(), cap
    assert s.find_all(d, capacity=5).cpu().tolist() == want[:5].tolist()


def test_words_of_the_manual(ss):
    text = np.frombuffer(open(os.path.join(GD, "i386.txt"), "rb").read(), dtype=np.uint8)
    d = torch.from_numpy(text.copy()).cuda()
    words = [w for w in open(os.path.join(GD, "words.txt"), "rb").read().split(b"\n") if w]
    assert len(words) == 4585
    with ss.matches_build():
        for k, w in enumerate(words):
            s = ss.DynamicHipSearcher.new(w)
            want = ref_offsets(text, w)
            assert s.count(d) == want.size, w
            if k % 37 == 0:
                assert (s.find_all(d).cpu().numpy() == want).all(), w


def test_one_gib_random_with_plants(ss):
    n_bytes = 1 << 30
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x5EED0042)
    rng = np.random.default_rng(6)
    needle = bytes(rng.integers(0, 256, size=12, dtype=np.uint8))
    nt = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
    plants = np.unique(np.concatenate([rng.integers(0, n_bytes - 12, size=300), [0, n_bytes - 12, 16384 * 1000 - 5]]))
    plants = plants[np.concatenate([[True], np.diff(plants) >= 12])]
    for p in plants:
        hay[int(p):int(p) + 12] = nt
    s = make(ss, needle)
    assert s.count(hay) == plants.size
    assert (s.find_all(hay).cpu().numpy() == plants).all()
    one = make(ss, needle[:1])                        # a one-byte needle on random bytes: ~4 M matches
    got = one.find_all(hay)
    assert got.numel() == one.count(hay) == int((hay == needle[0]).sum().item())
    assert bool((got[1:] > got[:-1]).all()) and bool((hay[got] == needle[0]).all())
    del hay, got
    torch.cuda.empty_cache()


def test_four_and_a_half_gib_matches_above_four_gib(ss):
    n_bytes = (9 << 30) // 2
    hay = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
    needle = b"needle in a haystack"
    nt = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
    plants = [5, (1 << 32) - 7, (1 << 32) + 16384 - 3, (1 << 32) + 12345678, n_bytes - len(needle)]
    for p in plants:
        hay[p:p + len(needle)] = nt
    s = make(ss, needle)
    assert s.count(hay) == len(plants)
    assert s.find_all(hay).cpu().tolist() == plants
    del hay
    torch.cuda.empty_cache()


def test_quarter_gib_of_one_byte(ss):
    n_bytes = 256 * MiB
    hay = torch.full((n_bytes,), ord("a"), dtype=torch.uint8, device="cuda")
    assert make(ss, b"a").count(hay) == n_bytes
    assert make(ss, b"aa").count(hay) == n_bytes - 1
    assert make(ss, b"a" * 16).count(hay) == n_bytes - 15
    got = make(ss, b"aa").find_all(hay, capacity=100000)
    assert (got.cpu().numpy() == np.arange(100000)).all()
    del hay
    torch.cuda.empty_cache()


def test_two_threads_two_streams(ss):
    rng = np.random.default_rng(7)
    hs = [rng.integers(0, 4, size=3 * MiB + k, dtype=np.uint8) for k in (0, 9)]
    needles = [b"\x01\x02\x03", b"\x00\x00"]
    wants = [ref_offsets(h, n) for h, n in zip(hs, needles)]
    errors = []

    def work(k):
        try:
            st = torch.cuda.Stream()
            s = make(ss, needles[k])
            with torch.cuda.stream(st):
                d = torch.from_numpy(hs[k]).cuda()
                for _ in range(40):
                    assert s.count(d) == wants[k].size
                    got = s.find_all(d).cpu().numpy()
                    assert (got == wants[k]).all()
        except Exception as e:                      # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_count_async_in_a_graph(ss):
    needle = b"graph needle"
    nt = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
    hay = torch.zeros(8 * MiB, dtype=torch.uint8, device="cuda")
    d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    s = make(ss, needle)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s.count_async(hay, d_count)                 # warm-up: the needle's device copy
    torch.cuda.synchronize()
    assert d_count.item() == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.count_async(hay, d_count)
    for k in range(1, 4):
        hay[1000 * k * k:1000 * k * k + len(needle)] = nt
        g.replay()
        torch.cuda.synchronize()
        assert d_count.item() == k


def test_repeatable_and_the_search_side_is_unchanged(ss):
    n_bytes = 256 * MiB
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x5EED0099)
    needle = b"repeatable needle"
    nt = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
    for p in (77, 12345678, n_bytes - len(needle)):
        hay[p:p + len(needle)] = nt
    s = make(ss, needle)
    ref_search, ref_find = s.search_in(hay), s.find(hay)
    s.search_in(hay)
    torch.cuda.synchronize()
    before = s.tuning_state(hay)
    first = s.find_all(hay).cpu().tolist()
    assert first == [77, 12345678, n_bytes - len(needle)]
    for _ in range(5):
        assert s.count(hay) == 3
        assert s.find_all(hay).cpu().tolist() == first
        assert s.search_in(hay) == ref_search and s.find(hay) == ref_find
    torch.cuda.synchronize()
    s2 = make(ss, b"never seen before")
    before2 = s2.tuning_state(hay)
    for _ in range(4):
        s2.count(hay)
        s2.find_all(hay)
    assert s2.tuning_state(hay) == before2              # the calls neither start nor feed the census
    assert before["autotune"] == s.tuning_state(hay)["autotune"]
    del hay
    torch.cuda.empty_cache()


# ---- edges, large grids, every kernel -------------------------------------------------------------------------------------------
# The geometry the tests aim at, restated from the library: a tile is 16 KiB of candidate offsets in aligned coordinates (offset +
# mis, mis = (address of the first filter byte) % 16); plan_all (ss_matches.hip) gives a workgroup one tile, or two contiguous tiles
# once there are at least 2 * CUs * 256 tiles (MODE 0) or 2 * CUs * 128 (MODE 2); prefix_kernel (scan_inst_all.hip) gives each of its
# 1,024 threads a run of ceil(workgroups / 1024) workgroup counts.
TILE = 16384
SENT = -0x5A5A5A5A5A5A5A5B


def kernel_of(s):
    """(Q, MODE, one-byte) of the all-matches kernel that runs searcher `s`: fill_problem's rule (ss_scan.hip) on the bytes the
    device tests.  MODE is 0 or 2 (a pair 16 or more apart runs the MODE 2 kernel, with or without a third byte of its own)."""
    n = len(s.needle)
    if n == 1:
        return 0, 0, True
    fa, fb, fc = s.device_triple()
    position = fb - fa
    d = position // 16
    three = fa < fc < n and fc - fa <= 15 and fc != fb
    position3 = fc - fa if three else position % 16
    if three and d == 0 and position3 // 4 > position // 4:
        position, position3 = position3, position
    return (position % 16) // 4, 0 if d == 0 else 2, False


def n_tiles(mis, length, n):
    return (((mis + length - n + 1 + 15) // 16 + 63) // 64 + 15) // 16


def tiles_per_workgroup(ntiles, cus, mode):
    return max(1, min(2, ntiles // (cus * (256 if mode == 0 else 128))))


def ref_regions(hay, regions, needle):
    """Reference offsets of a haystack on which only `regions` ((start, length)) can match: host copies widened by len(needle)."""
    n, L = len(needle), hay.numel()
    parts = [np.zeros(0, dtype=np.int64)]
    for p, ln in regions:
        a, b = max(0, p - n), min(L, p + ln + n)
        parts.append(ref_offsets(hay[a:b].cpu().numpy(), needle) + a)
    return np.unique(np.concatenate(parts))


def check_cut(s, hay, want, cap, what):
    """find_all_into a window of `cap` offsets inside a larger buffer: the first cap offsets, the total, both sentinels."""
    buf = torch.full((cap + 16,), SENT, dtype=torch.int64, device="cuda")
    assert s.find_all_into(hay, buf[8:8 + cap]) == want.size, (what, cap)
    b = buf.cpu().numpy()
    k = min(cap, want.size)
    assert (b[8:8 + k] == want[:k]).all(), (what, cap, b[8:8 + min(k, 8)], want[:min(k, 8)])
    assert (b[:8] == SENT).all() and (b[8 + k:] == SENT).all(), (what, cap)


def edge_lengths(n):
    return n, n + 1, 16 * 1024 - 1, 16 * 1024 + 1, 1008 * 16 + 3, 70000


def edge_searchers(ss, needle, k):
    """new, the first filter byte at k (1..15) and, for needles of 17 bytes or more, a pair 16 or more apart"""
    n = len(needle)
    out = [("new", make(ss, needle))]
    if n >= 3:
        a = min(k, n - 2)
        out.append(("first at %d" % a, make(ss, needle, triple=(a, n - 1 if n - 1 - a <= 15 else a + 15, a + 1))))
    elif n == 2:
        out.append(("with_position 1", make(ss, needle, position=1)))
    if n >= 17:
        a = k % max(1, min(16, n - 16))
        b = min(n - 1, a + 1007)                      # at most 62 chunks apart: the cross-lane kernels, no far byte
        out.append(("pair d=%d" % ((b - a) // 16), make(ss, needle, triple=(a, b, b))))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 13, 16, 17, 33, 40, 64, 1200])
def test_nothing_outside_the_view_is_read_or_counted(ss, n):
    """The analogue of test_no_read_or_match_beyond_len for count and find-all: copies of the needle entirely in front of the view,
    straddling its start by 1 .. n-1 bytes, straddling its end, and entirely after it.  Only copies wholly inside may count."""
    rng = np.random.default_rng(100 + n)
    needle = bytes(rng.integers(1, 256, size=n, dtype=np.uint8))
    arr = np.frombuffer(needle, dtype=np.uint8)
    G = 2048
    for mis in range(16):
        searchers = edge_searchers(ss, needle, 1 + mis % 15)
        # straddles of j bytes: 1, n-1 and, over the 16 misalignments, every j (n <= 129) or 8 of each residue mod 16 (n = 1200)
        spread = [j for j in range(1, n) if j % 16 == mis]
        spread = spread[::max(1, -(-len(spread) // 8))]
        for L in edge_lengths(n)[mis % 3::3]:
            base = rng.integers(0, 256, size=L + 2 * G, dtype=np.uint8)
            v0 = G + mis
            if L >= 3 * n:
                base[v0 + L // 2:v0 + L // 2 + n] = arr                  # one copy inside, away from the edges
            js = sorted({1, n - 1} | set(spread)) if n > 1 else []
            for front, back in [("whole", "whole")] + [(j, j) for j in js] + [(j, "whole") for j in js[:1]] + [("whole", j) for j in js[-1:]]:
                h = base.copy()
                if front == "whole":
                    h[v0 - n:v0] = arr
                else:
                    h[v0 - (n - front):v0 - (n - front) + n] = arr      # `front` bytes inside the view
                if back == "whole":
                    h[v0 + L:v0 + L + n] = arr
                else:
                    h[v0 + L - back:v0 + L - back + n] = arr            # `back` bytes inside the view
                dev = torch.from_numpy(h).cuda()
                for what, s in searchers:
                    check(s, dev[v0:v0 + L], h[v0:v0 + L], needle, "%s mis %d len %d front %s back %s" % (what, mis, L, front, back))


def test_search_side_ignores_copies_straddling_the_start(ss):
    """The product library (search_in / find) on the same start-straddling copies: a needle that begins in front of the pointer
    and ends inside the view is not in the view."""
    rng = np.random.default_rng(110)
    for n in (2, 3, 13, 16, 17, 40, 64, 1200):
        needle = bytes(rng.integers(1, 256, size=n, dtype=np.uint8))
        arr = np.frombuffer(needle, dtype=np.uint8)
        s = ss.DynamicHipSearcher.new(needle)
        s1 = ss.DynamicHipSearcher.new(needle)
        s1.set_filter(min(5, n - 2), n - 1)
        for mis in range(16):
            L = (70000, 16 * 1024 + 1, 2 * n)[mis % 3]
            for j in sorted({1, n // 2, n - 1}):
                h = np.zeros(L + 4096, dtype=np.uint8)
                v0 = 2048 + mis
                h[v0 - (n - j):v0 + j] = arr
                dev = torch.from_numpy(h).cuda()
                view = dev[v0:v0 + L]
                for t in (s, s1):
                    assert t.search_in(view) is False and t.find(view) is None, (n, mis, L, j)
                h[v0 + L - n:v0 + L] = arr                                # and one wholly inside, flush against the end
                dev = torch.from_numpy(h).cuda()
                for t in (s, s1):
                    assert t.find(dev[v0:v0 + L]) == L - n, (n, mis, L, j)


def _two_tile(ss, s, mode, n_bytes, unit, rng):
    """One haystack of n_bytes zeros (the needle holds no zero byte) with dense runs of `unit` in both tiles of many two-tile
    workgroups, across their inner tile borders, around 2^32 and in the last workgroup; count, find_all and capacity cuts."""
    needle = s.needle
    n = len(needle)
    cus = ss.device_info()["compute_units"]
    mis = s.device_triple()[0] % 16                     # a fresh allocation is aligned far beyond 16 bytes
    ntiles = n_tiles(mis, n_bytes, n)
    assert kernel_of(s)[1] == mode and tiles_per_workgroup(ntiles, cus, mode) == 2 and ntiles % 2 == 1, (ntiles, cus)
    nwg = (ntiles + 1) // 2
    hay = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
    wgs = sorted(set(rng.choice(nwg - 1, size=min(nwg - 1, 240), replace=False).tolist()) | {0, 1, nwg - 2, nwg - 1} |
                 ({((1 << 32) // TILE) // 2, ((1 << 32) // TILE) // 2 - 1} if n_bytes > (1 << 32) + 4 * TILE else set()))
    regions = []
    for w in wgs:
        t0 = 2 * w * TILE - mis
        spots = [t0 + 1000 + int(rng.integers(0, 5000)), t0 + TILE - 300]           # tile 2w, and across the border to tile 2w+1
        if w != nwg - 1:
            spots.append(t0 + TILE + 2000 + int(rng.integers(0, 5000)))             # tile 2w+1
        else:
            spots.append(n_bytes - 700)                                               # the last workgroup's single tile, flush with the end
        for p in spots:
            p = max(0, min(p, n_bytes - 700))
            regions.append((p, 700))
    if n_bytes > (1 << 32) + 4 * TILE:
        regions.append(((1 << 32) - 350, 700))                                        # across 2^32
    regions = sorted(set(regions))
    body = torch.from_numpy(np.frombuffer((unit * (700 // len(unit) + 1))[:700], dtype=np.uint8).copy()).cuda()
    for p, ln in regions:
        hay[p:p + ln] = body
    want = ref_regions(hay, regions, needle)
    wg_of = ((want + mis) // TILE) // 2
    tile_of = (want + mis) // TILE
    both = np.intersect1d(wg_of[tile_of % 2 == 0], wg_of[tile_of % 2 == 1])
    assert both.size > 200 and wg_of[-1] == nwg - 1, (both.size, wg_of[-1], nwg)
    assert s.count(hay) == want.size
    got = s.find_all(hay).cpu().numpy()
    assert got.size == want.size and (got == want).all(), (got.size, want.size)
    for w in (int(both[0]), int(both[both.size // 2]), int(both[-1]) if both[-1] != nwg - 1 else int(both[-2])):
        first_second = int(np.flatnonzero((wg_of == w) & (tile_of % 2 == 1))[0])
        last = int(np.flatnonzero(wg_of == w)[-1])
        for cap in (first_second + 3, last + 1, last + 2, last):                       # inside a second tile, at a workgroup's last
            check_cut(s, hay, want, cap, "wg %d" % w)                                  # match, at the next one's first
    check_cut(s, hay, want, want.size - 1, "last")
    del hay
    torch.cuda.empty_cache()


def test_two_tile_workgroups_mode0_across_four_gib(ss):
    free, _ = torch.cuda.mem_get_info()
    if free < (5 << 30):
        pytest.skip("needs about 4.2 GiB of free device memory")
    cus = ss.device_info()["compute_units"]
    rng = np.random.default_rng(120)
    s = make(ss, b"abab")                               # exact in-register verification
    s40 = make(ss, b"ab" * 20)                          # verification in memory
    for t in (s, s40):
        assert kernel_of(t)[1] == 0
    mis = s.device_triple()[0] % 16
    n_bytes = (1 << 32) + 5 * TILE + 123
    if n_tiles(mis, n_bytes, 4) % 2 == 0:
        n_bytes += TILE
    assert tiles_per_workgroup(n_tiles(mis, n_bytes, 4), cus, 0) == 2
    _two_tile(ss, s, 0, n_bytes, b"ab", rng)
    mis = s40.device_triple()[0] % 16
    if n_tiles(mis, n_bytes, 40) % 2 == 0:
        n_bytes += TILE
    _two_tile(ss, s40, 0, n_bytes, b"ab", rng)


def test_two_tile_workgroups_mode2(ss):
    cus = ss.device_info()["compute_units"]
    rng = np.random.default_rng(121)
    needle = (b"xyz" * 20)[:50]
    s = make(ss, needle, triple=(1, 35, 35))                      # 34 apart: d = 2
    assert kernel_of(s)[1] == 2
    mis = s.device_triple()[0] % 16
    n_bytes = 2 * cus * 128 * TILE + 3 * TILE + 77
    if n_tiles(mis, n_bytes, len(needle)) % 2 == 0:
        n_bytes += TILE
    _two_tile(ss, s, 2, n_bytes, b"xyz", rng)


@pytest.mark.parametrize("grid", [1023, 1024, 1025, 2047, 2049, 65537])
def test_prefix_run_boundaries(ss, grid):
    """Grids of one tile per workgroup around multiples of the prefix kernel's 1,024 threads; matches only in the workgroups at
    the ends of the threads' runs (0, per-1, per, ...) and in the last one; offsets and capacity cuts at each of them."""
    cus = ss.device_info()["compute_units"]
    grid = min(grid, 2 * cus * 256 - 1)                           # one tile per workgroup
    needle = b"q\x01needle\x02"
    n = len(needle)
    s = make(ss, needle)
    assert kernel_of(s)[1] == 0
    mis = s.device_triple()[0] % 16
    n_bytes = grid * TILE - mis + n - 1 - 7
    assert n_tiles(mis, n_bytes, n) == grid and tiles_per_workgroup(grid, cus, 0) == 1
    per = -(-grid // 1024)
    wgs = sorted({w for w in (0, per - 1, per, 2 * per - 1, 2 * per, 511 * per, 512 * per, 1023, 1024, grid - 1) if 0 <= w < grid})
    hay = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
    nt = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
    plants = []
    for w in wgs:
        t0 = w * TILE - mis
        for p in (t0 + 16, t0 + 7001, t0 + TILE - 1):                   # the tile's first, a middle and its last candidate
            plants.append(max(0, min(p, n_bytes - n)))
    plants = np.unique(np.array(plants + [n_bytes - n], dtype=np.int64))
    for p in plants:
        hay[int(p):int(p) + n] = nt
    want = ref_regions(hay, [(int(p), n) for p in plants], needle)
    assert want.size == plants.size and (want == plants).all()
    wg_of = (want + mis) // TILE
    assert set(wg_of.tolist()) == set(wgs), (sorted(set(wg_of.tolist())), wgs)
    assert s.count(hay) == want.size
    got = s.find_all(hay).cpu().numpy()
    assert got.size == want.size and (got == want).all(), (grid, got, want)
    for w in wgs:
        first = int(np.flatnonzero(wg_of == w)[0])
        for cap in (first, first + 1, first + 2):
            check_cut(s, hay, want, cap, "grid %d wg %d" % (grid, w))
    del hay
    torch.cuda.empty_cache()


# (name, needle, triple or ("position", p) or None): together they reach each of the nine all-matches kernels (Q x MODE 0, Q x MODE 2,
# one-byte); the triples are ones the device runs as given (device_triple() == the triple, or its first two bytes for a plain pair)
KERNEL_ROWS = [
    ("one byte", b"x", None),
    ("mode0 q0", (b"xyzw" * 4)[:14], (0, 1, 2)),
    ("mode0 q1 first at 3", (b"xyzw" * 4)[:14], (3, 8, 5)),
    ("mode0 q2 first at 1", (b"xyz" * 5)[:14], (1, 10, 3)),
    ("mode0 q3 swapped", (b"xyz" * 20)[:40], (2, 3, 15)),
    ("mode0 q3 with_position", (b"xyzw" * 10)[:40], ("position", 13)),
    ("mode2 q0", (b"xyz" * 20)[:48], (0, 16, 16)),
    ("mode2 q1", (b"xyzw" * 20)[:48], (3, 23, 23)),
    ("mode2 q2", (b"xyz" * 20)[:60], (0, 40, 40)),
    ("mode2 q3", (b"xyzw" * 20)[:48], (5, 33, 33)),
    ("pair alone d=3", (b"xyz" * 30)[:70], (1, 61, 61)),
]


def _kernel_row(ss, needle, spec):
    if spec is None:
        return make(ss, needle)
    if spec[0] == "position":
        return make(ss, needle, position=spec[1])
    s = make(ss, needle, triple=spec)
    dt = s.device_triple()
    assert dt[:2] == spec[:2] and (spec[2] == spec[1] or dt[2] == spec[2]), (spec, dt)
    return s


def test_every_kernel_instantiation(ss):
    rng = np.random.default_rng(130)
    rows = [(name, needle, _kernel_row(ss, needle, spec)) for name, needle, spec in KERNEL_ROWS]
    kernels = {kernel_of(s) for _, _, s in rows}
    assert kernels == {(q, m, False) for q in range(4) for m in (0, 2)} | {(0, 0, True)}, kernels
    L = 4 * TILE + 777
    G = 256
    for name, needle, s in rows:
        n = len(needle)
        unit = needle[:4] if needle[:4] == needle[4:8] else needle[:3]
        dense = np.frombuffer((unit * ((L + 2 * G) // len(unit) + 1))[:L + 2 * G], dtype=np.uint8).copy()
        rnd = rng.integers(0, 256, size=L + 2 * G, dtype=np.uint8)
        rnd[rnd == needle[0]] = needle[0] ^ 0x40                        # random bytes with plants only
        borders = [1024 * 5, 4096 * 3, TILE, 2 * TILE + 1024, 3 * TILE]
        deltas = [-n + 1, -n // 2, -1, 0, 1, -16, 15, -n - 1]
        for mis in range(16):
            d = dense.copy()
            dev = torch.from_numpy(d).cuda()
            check(s, dev[G + mis:G + mis + L], d[G + mis:G + mis + L], needle, "%s dense mis %d" % (name, mis))
            h = rnd.copy()
            delta = deltas[mis % len(deltas)]
            for b in borders:
                h[G + mis + b + delta:G + mis + b + delta + n] = np.frombuffer(needle, dtype=np.uint8)
            h[G + mis + L - n:G + mis + L] = np.frombuffer(needle, dtype=np.uint8)
            dev = torch.from_numpy(h).cuda()
            check(s, dev[G + mis:G + mis + L], h[G + mis:G + mis + L], needle, "%s plants mis %d delta %d" % (name, mis, delta))


def _nonlatin(n_bytes, seed):
    """UTF-8-like text in a non-Latin script (the generator of tools/fuzz_gpu.py nonlatin)."""
    nrng = np.random.default_rng(seed)
    pairs = n_bytes // 2
    lead = nrng.choice(np.array([0xD0, 0xD1], dtype=np.uint8), size=pairs, p=[0.6, 0.4])
    trail = (0x80 + np.minimum(nrng.geometric(0.08, size=pairs) - 1, 63)).astype(np.uint8)
    host = np.empty(n_bytes, dtype=np.uint8)
    host[0::2], host[1::2] = lead, trail
    blanks = nrng.integers(0, pairs, size=pairs // 7)
    host[2 * blanks] = 0x20
    host[2 * blanks + 1] = 0x20
    return host


def _find_every(hb, needle):
    """Every (overlapping) offset through bytes.find: the reference where a numpy candidate list would not fit in memory."""
    out, i = [], hb.find(needle)
    while i >= 0:
        out.append(i)
        i = hb.find(needle, i + 1)
    return np.array(out, dtype=np.int64)


def test_count_and_find_all_after_the_library_moved_the_bytes(ss):
    """On 512 MiB of non-Latin text the census moves a `new` searcher's filter bytes (tuning_state: in_force != own).  count and
    find_all run the static bytes and must not care; search_in / find answers and the tuning state must not care about them."""
    n_bytes = 512 * MiB
    host = _nonlatin(n_bytes, 140)
    rng = np.random.default_rng(141)
    needles = []
    for k in range(8):
        n = (8, 12, 16, 17, 24, 32, 12, 16)[k]
        at = int(rng.integers(0, n_bytes - n))
        nd = bytearray(host[at:at + n].tobytes())
        if k >= 6:
            nd[n // 2] = 0xFF                                        # absent
        needles.append(bytes(nd))
    host[n_bytes - 16:] = np.frombuffer(needles[2], dtype=np.uint8)  # planted flush against the end
    hb = host.tobytes()
    hay = torch.from_numpy(host).cuda()
    moved = 0
    for nd in needles:
        want = _find_every(hb, nd)
        s = make(ss, nd)
        for _ in range(16):
            s.search_in(hay)
            torch.cuda.synchronize()
            st = s.tuning_state(hay)
            if st["in_force"] != st["own"] and st["settled"]:
                break
        moved += st["in_force"] != st["own"]
        si, fd = s.search_in(hay), s.find(hay)
        assert si == (want.size > 0) and fd == (int(want[0]) if want.size else None), nd
        torch.cuda.synchronize()
        before = s.tuning_state(hay)
        for _ in range(2):
            assert s.count(hay) == want.size, nd
            got = s.find_all(hay).cpu().numpy()
            assert got.size == want.size and (got == want).all(), nd
        torch.cuda.synchronize()
        assert s.tuning_state(hay) == before, nd
        assert s.search_in(hay) == si and s.find(hay) == fd, nd
    assert moved >= 3, moved                # otherwise the test proves nothing
    del hay
    torch.cuda.empty_cache()


def test_count_and_find_all_campaign(ss):
    """tools/fuzz_matches.py for a few seconds in both modes: small haystacks, and a big one on which MODE 0 and MODE 2 workgroups
    scan two tiles (its size from the device's compute units)."""
    import json
    import subprocess
    import sys
    cus = ss.device_info()["compute_units"]
    gib = (2 * cus * 256 + 3) * TILE / (1 << 30)
    for extra, least in (([], 1000), (["%.9f" % gib], 400)):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_matches.py"), "8", "4243"] + extra,
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        d = json.loads(out.stdout.strip().splitlines()[-1])
        assert d["fuzz_matches"] == "ok" and d["calls"] >= least, d
