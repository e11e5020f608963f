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


def make(ss, needle, position=None, triple=None, memchr=False):
    with ss.matches_build():
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
