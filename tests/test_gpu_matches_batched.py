"""GPU tests of the batched every-occurrence calls (include/sliceslice_hip_matches_batched.h, libsliceslice_hip_matches_batched.so):
ss_count_batched and ss_find_all_batched against the host bytes - `bytes.find` stepping by one, or a numpy candidate-and-verify
restatement (a private copy).  Counts, row begins and every offset are compared.

Wall time on an MI355X, per test: DESIGN.md 5.7."""
import ctypes
import os
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
TILE = 16384
SENTINEL = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with batched_lib(m):
        pass
    return m


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def batched_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the batched entry points (another build of
    libsliceslice_hip_matches_batched.so), else `ss.matches_batched_build()`."""
    return _loaded() if getattr(ss.lib(), "has_matches_batched", False) else ss.matches_batched_build()


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


def find_stepping(h, n):
    """bytes.find stepping by one: the overlapping offsets of n in h."""
    out, i = [], h.find(n)
    while i >= 0:
        out.append(i)
        i = h.find(n, i + 1)
    return np.array(out, dtype=np.int64)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dtype is None else torch.tensor(a, dtype=dtype, device="cuda")


class Batch:
    """A batch on the device: one haystack blob, one needle blob, explicit (begin, end) ranges."""

    def __init__(self, hay_dev, hay_ranges, needles):
        self.hay = hay_dev
        self.count = len(needles)
        blob, self.nd_ranges = bytearray(b"\x00\x00\x00"), []           # (needles at odd addresses)
        for nd in needles:
            self.nd_ranges.append((len(blob), len(blob) + len(nd)))
            blob += nd + b"\xA5"
        self.nd = dev(np.frombuffer(bytes(blob), dtype=np.uint8).copy())
        self.hb, self.he = dev([r[0] for r in hay_ranges], torch.int64), dev([r[1] for r in hay_ranges], torch.int64)
        self.nb, self.ne = dev([r[0] for r in self.nd_ranges], torch.int64), dev([r[1] for r in self.nd_ranges], torch.int64)

    def kw(self):
        return dict(hay_ranges=(self.hb, self.he), needle_ranges=(self.nb, self.ne))

    def args(self):
        return (self.hay, None, self.nd, None)


def check_batch(ss, b, want, what=""):
    """count_batched and find_all_batched of batch `b` against `want` (one offsets array per problem)."""
    want_counts = np.array([w.size for w in want], dtype=np.int64)
    want_rows = np.concatenate([[0], np.cumsum(want_counts)]).astype(np.int64)
    with batched_lib(ss):
        got = ss.count_batched(*b.args(), **b.kw()).cpu().numpy()
        counts, rows, offs = ss.find_all_batched(*b.args(), **b.kw())
    bad = np.flatnonzero(got != want_counts)
    assert bad.size == 0, (what, "count_batched", int(bad[0]), int(got[bad[0]]), int(want_counts[bad[0]]))
    assert np.array_equal(counts.cpu().numpy(), want_counts), (what, "find_all_batched counts")
    assert np.array_equal(rows.cpu().numpy(), want_rows), (what, "row_begin")
    offs = offs.cpu().numpy()
    assert offs.size == want_rows[-1], (what, offs.size, int(want_rows[-1]))
    for i, w in enumerate(want):
        g = offs[want_rows[i]:want_rows[i + 1]]
        assert np.array_equal(g, w), (what, "offsets of problem", i, g[:8], w[:8])
    return got, rows, offs


@pytest.fixture(scope="module")
def table(ss, corpus):
    """The i386 table: 4,585 words x i386.txt, aliased ranges; the host's offsets by bytes.find stepping by one."""
    text, words = corpus["i386"], corpus["words"]
    assert len(words) == 4585
    want = [find_stepping(text, w) for w in words]
    b = Batch(dev(np.frombuffer(text, dtype=np.uint8).copy()), [(0, len(text))] * len(words), words)
    return b, want, text, words


def test_the_i386_table(ss, table):
    """1. Counts, row_begin and every offset of the 4,585-word table; the host restatement pinned by three figures."""
    b, want, text, words = table
    counts = np.array([w.size for w in want])
    assert int(counts.sum()) == 716940 and int(counts.max()) == 59485 and int(counts.min()) > 0
    check_batch(ss, b, want, "i386")


def test_capacity_cuts_on_the_table(ss, table):
    """2. Capacities 0, 1, inside a row, at a row border, total - 1, total, total + 7: sentinels on both sides of the caller's
    window survive; total, rows and counts are the same at every capacity."""
    b, want, text, words = table
    want_counts = np.array([w.size for w in want], dtype=np.int64)
    want_rows = np.concatenate([[0], np.cumsum(want_counts)]).astype(np.int64)
    want_all = np.concatenate(want)
    total = int(want_rows[-1])
    inside = int(want_rows[1000] + want_counts[1000] // 2 + 1)
    assert want_rows[1000] < inside < want_rows[1001] or want_counts[1000] < 2
    with batched_lib(ss):
        L = ss.lib()
        for cap in (0, 1, inside, int(want_rows[2000]), total - 1, total, total + 7):
            buf = torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device="cuda")
            counts = torch.full((b.count,), -1, dtype=torch.int64, device="cuda")
            rows = torch.full((b.count + 1,), -1, dtype=torch.int64, device="cuda")
            tot = ctypes.c_uint64(0)
            rc = L.ss_find_all_batched(b.hay.data_ptr(), b.hb.data_ptr(), b.he.data_ptr(), b.nd.data_ptr(), b.nb.data_ptr(), b.ne.data_ptr(),
                                       b.count, None, counts.data_ptr(), rows.data_ptr(), buf.data_ptr() + 64 if cap else None, cap,
                                       ctypes.byref(tot))
            torch.cuda.synchronize()
            assert rc == 0 and tot.value == total, (cap, rc, tot.value)
            assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(counts.cpu().numpy(), want_counts), cap
            h = buf.cpu().numpy()
            k = min(cap, total)
            assert (h[:8] == SENTINEL).all() and (h[8 + k:] == SENTINEL).all(), cap
            assert np.array_equal(h[8:8 + k], want_all[:k]), cap
        # counts may be NULL; count == 0 is a valid call
        rows = torch.full((b.count + 1,), -1, dtype=torch.int64, device="cuda")
        tot = ctypes.c_uint64(7)
        assert L.ss_find_all_batched(b.hay.data_ptr(), b.hb.data_ptr(), b.he.data_ptr(), b.nd.data_ptr(), b.nb.data_ptr(), b.ne.data_ptr(),
                                     b.count, None, None, rows.data_ptr(), None, 0, ctypes.byref(tot)) == 0
        assert tot.value == total and np.array_equal(rows.cpu().numpy(), want_rows)
        assert L.ss_find_all_batched(b.hay.data_ptr(), b.hb.data_ptr(), b.he.data_ptr(), b.nd.data_ptr(), b.nb.data_ptr(), b.ne.data_ptr(),
                                     0, None, None, rows.data_ptr(), None, 0, ctypes.byref(tot)) == 0
        assert tot.value == 0 and int(rows[0]) == 0
        assert L.ss_count_batched(b.hay.data_ptr(), b.hb.data_ptr(), b.he.data_ptr(), b.nd.data_ptr(), b.nb.data_ptr(), b.ne.data_ptr(),
                                  0, None, None) == 0
        # argument checks follow ss_search_batched
        assert L.ss_count_batched(b.hay.data_ptr(), None, b.he.data_ptr(), b.nd.data_ptr(), b.nb.data_ptr(), b.ne.data_ptr(),
                                  b.count, None, counts.data_ptr()) == ss.SS_ERR_ARGUMENT
        assert L.ss_find_all_batched(b.hay.data_ptr(), b.hb.data_ptr(), b.he.data_ptr(), b.nd.data_ptr(), b.nb.data_ptr(), b.ne.data_ptr(),
                                     b.count, None, None, rows.data_ptr(), None, 5, ctypes.byref(tot)) == ss.SS_ERR_ARGUMENT
        assert b"capacity" in L.ss_last_error()


def test_relations_to_the_other_calls(ss, table):
    """3. counts > 0 == search_batched's flag; first offset of a non-empty row == find_batched; a sample == count() / find_all()."""
    b, want, text, words = table
    absent = [b"no such phrase", b"zzzzzzzzzz", b"Zq"]
    b2 = Batch(b.hay, [(0, len(text))] * (len(words) + len(absent)), list(words) + absent)
    with batched_lib(ss):
        counts, rows, offs = ss.find_all_batched(*b2.args(), **b2.kw())
        flags = ss.search_batched(*b2.args(), **b2.kw())
        first = ss.find_batched(*b2.args(), **b2.kw())
        counts, rows, offs, flags, first = (t.cpu().numpy() for t in (counts, rows, offs, flags, first))
        assert np.array_equal(counts > 0, flags != 0) and (counts[-len(absent):] == 0).all()
        nz = np.flatnonzero(counts > 0)
        assert np.array_equal(offs[rows[nz]], first[nz]) and (first[counts == 0] == -1).all()
        for i in list(range(0, len(words), 97)) + [int(np.argmax(counts))]:
            s = ss.DynamicHipSearcher(words[i])
            assert s.count(b.hay) == counts[i]
            assert np.array_equal(s.find_all(b.hay).cpu().numpy(), offs[rows[i]:rows[i + 1]]), words[i]


def test_ragged_batches(ss):
    """4. Seeded ragged batches: haystacks from empty to several MiB inside one blob at odd begins, needles of 0 .. 2,000 bytes,
    n > len, one-byte needles, self-overlapping needles ('aa' in an 8 MiB run of 'a': len - 1), explicit ranges and CSR."""
    rng = np.random.default_rng(20260501)
    lens = [0, 1, 2, 15, 16, 17, 63, 1000, 4096, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 100000, MiB + 3, 3 * MiB + 17, 5 * MiB]
    blob = rng.choice(np.frombuffer(b"abcdefgh \n", dtype=np.uint8), sum(lens) + 64 * len(lens) + 8 * MiB + 256)
    ranges, needles, at = [], [], 3
    for k, L in enumerate(lens):
        ranges.append((at, at + L))
        hay = blob[at:at + L]
        if k % 6 == 0:
            nd = b""
        elif k % 6 == 1 or L == 0:
            nd = bytes(rng.integers(0, 256, L + 1 + k % 3, dtype=np.uint8)) if L < 3000 else b"a"
        elif k % 6 == 2:
            nd = bytes(hay[L // 2:L // 2 + 1])                          # one byte
        else:
            n = min(L, [2, 3, 16, 17, 40, 700, 2000][k % 7])
            nd = bytes(hay[L - n:])                                     # flush against the end
        needles.append(nd)
        at += L + 1 + (k * 7) % 40
    # an 8 MiB run of 'a' at an odd begin: 'aa' (len - 1), 'a' (len), 17 x 'a', and a needle longer than the run
    run0 = at + 5
    blob[run0 - 1], blob[run0:run0 + 8 * MiB], blob[run0 + 8 * MiB] = ord("b"), ord("a"), ord("b")
    for nd in (b"aa", b"a", b"a" * 17, b"a" * 2000):
        ranges.append((run0, run0 + 8 * MiB))
        needles.append(nd)
    # (the run's offsets follow from its being a run: 0 .. len - n; the restatement takes 40 s for the 2,000-byte needle)
    assert blob[run0:run0 + 8 * MiB].tobytes() == b"a" * (8 * MiB)
    want = [ref_offsets(blob[b:e], nd) for (b, e), nd in zip(ranges[:-4], needles[:-4])] + \
        [np.arange(8 * MiB - len(nd) + 1, dtype=np.int64) for nd in needles[-4:]]
    assert want[-4].size == 8 * MiB - 1 and want[-3].size == 8 * MiB and want[-1].size == 8 * MiB - 1999
    d_blob = dev(blob)
    check_batch(ss, Batch(d_blob, ranges, needles), want, "ragged, explicit ranges")
    # the run among 25,000 tiny problems: one workgroup per problem, so the run's workgroup counts 8 Mi matches alone
    tiny = [(3 + 40 * k, 3 + 40 * k + 32) for k in range(25000)]
    tn = [bytes(blob[b + 7:b + 9]) for b, e in tiny]
    want_t = [ref_offsets(blob[b:e], nd) for (b, e), nd in zip(tiny, tn)]
    check_batch(ss, Batch(d_blob, tiny[:12000] + [(run0, run0 + 8 * MiB)] + tiny[12000:], tn[:12000] + [b"aa"] + tn[12000:]),
                want_t[:12000] + [want[-4]] + want_t[12000:], "run among 25,000")
    # CSR: contiguous haystacks and needles
    cuts = np.concatenate([[0], np.cumsum(rng.integers(0, 3000, 500))]).astype(np.int64)
    nds = [bytes(blob[cuts[k] + 5:cuts[k] + 5 + (k % 4)]) if cuts[k + 1] - cuts[k] > 12 else b"ab" for k in range(500)]
    ncuts = np.concatenate([[0], np.cumsum([len(x) for x in nds])]).astype(np.int64)
    want_c = [ref_offsets(blob[cuts[k]:cuts[k + 1]], nds[k]) for k in range(500)]
    with batched_lib(ss):
        d_n = dev(np.frombuffer(b"".join(nds) + b"\x00", dtype=np.uint8).copy())
        got = ss.count_batched(d_blob, dev(cuts), d_n, dev(ncuts)).cpu().numpy()
        counts, rows, offs = ss.find_all_batched(d_blob, dev(cuts), d_n, dev(ncuts))
    assert np.array_equal(got, [w.size for w in want_c]) and np.array_equal(counts.cpu().numpy(), got)
    assert np.array_equal(offs.cpu().numpy(), np.concatenate(want_c))
    assert np.array_equal(rows.cpu().numpy(), np.concatenate([[0], np.cumsum(got)]))


def test_borders(ss):
    """5. Needle copies straddling hay_begin and hay_end of adjacent problems are counted by neither; matches flush against both
    ends are; matches across the slice and tile borders of a problem scanned by several workgroups are counted once each."""
    rng = np.random.default_rng(5)
    for nd in (b"needle", b"xy", b"q", b"abcdefghijklmnopqrstuvwxyz0123456789" * 3, b"ww"):
        n, L = len(nd), 40 * TILE + 123
        blob = rng.integers(ord("A"), ord("P"), 5 * L + 8192, dtype=np.uint8)      # (none of the needles' bytes)
        src = np.frombuffer(nd, dtype=np.uint8)
        a0 = 1000 + 13
        # A and B adjacent (A's end is B's begin), C and D apart
        ranges = [(a0, a0 + L), (a0 + L, a0 + 2 * L), (a0 + 2 * L + 777, a0 + 3 * L + 777), (a0 + 3 * L + 2001, a0 + 4 * L + 2001)]
        for b, e in ranges:
            for t in range(1, 40):                                                 # across every tile border, at several phases
                o = b + t * TILE - (t * 5) % (n + 16)
                blob[o:o + n] = src
            if n == 2 and nd[0] == nd[1]:
                blob[b + 7 * TILE - 300:b + 7 * TILE + 300] = nd[0]                # a self-overlapping run across a border
        (ab, ae), (bb, be), (cb, ce), (db, de) = ranges
        blob[ab:ab + n] = src                                                      # flush against A's begin, B's end, both ends of D
        blob[be - n:be] = src
        blob[db:db + n] = src
        blob[de - n:de] = src
        if n > 1:
            k = n // 2
            for at in (ae - k, cb - k, ce - k):                                    # cut by A's end = B's begin, C's begin, C's end
                blob[at:at + n] = src
        want = [ref_offsets(blob[b:e], nd) for b, e in ranges]
        assert all(w.size >= 38 for w in want)
        assert want[0][0] == 0 and want[1][-1] == L - n and want[3][0] == 0 and want[3][-1] == L - n
        if n > 1 and nd[0] != nd[1]:
            assert want[0][-1] < L - n and want[1][0] > 0 and want[2][0] > 0 and want[2][-1] < L - n
        check_batch(ss, Batch(dev(blob), ranges, [nd] * 4), want, "borders %r" % nd[:8])


def _scrubbed(ss, nbytes, seed, x, lo=0):
    """Random bytes on the device with the byte value x replaced from offset lo on."""
    hay = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, seed)
    step = 1 << 30
    for o in range(lo, nbytes, step):
        v = hay[o:o + step]
        v.masked_fill_(v == x, (x + 1) & 0xFF)
    return hay


def _plant_runs(hay, begin, length, x, n, rng, nruns=300):
    """Runs of x inside hay[begin : begin + length) - flush against both ends, at tile borders, at random places; returns the
    offsets (relative to begin) at which x * n matches: a run of R >= n bytes holds R - n + 1.  x occurs nowhere else in the range."""
    runs = [(0, n + 3)]
    for t in sorted(set(int(t) for t in rng.integers(1, length // TILE, nruns))):
        s, R = t * TILE - int(rng.integers(0, 48)), int(rng.integers(1, 64))
        if s > runs[-1][0] + runs[-1][1] and s + R < length - 200:                 # (a byte that is not x between two runs)
            runs.append((s, R))
    runs.append((length - n - 2, n + 2))
    want = []
    for s, R in runs:
        hay[begin + s:begin + s + R] = x
        if R >= n:
            want.append(np.arange(s, s + R - n + 1, dtype=np.int64))
    return np.concatenate(want)


def test_above_4gib_long_problems_and_one_long_among_many(ss):
    """6. A blob above 4 GiB whose problems begin above 2^32: four long problems (256 MiB each, thousands of slices apiece), and in
    another call one of them among 30,000 short ones - ONE workgroup scans all of it, correct, and the wall time says what it costs.
    Surplus slices contribute nothing; offsets are 64-bit and problem-relative."""
    X = 0xE7
    rng = np.random.default_rng(6)
    first = (1 << 32) + 12345
    L = 256 * MiB
    nbytes = first + 4 * (L + 4096) + 30000 * 64 + 4096
    hay = _scrubbed(ss, nbytes, 0x600D, X, lo=1 << 32)
    ranges, needles, want = [], [], []
    for k, n in enumerate((2, 1, 17, 5)):
        b = first + k * (L + 4096) + k
        ranges.append((b, b + L))
        needles.append(bytes([X]) * n)
        want.append(_plant_runs(hay, b, L, X, n, rng))
    t0 = time.time()
    check_batch(ss, Batch(hay, ranges, needles), want, "four long problems above 2^32")
    t_long = time.time() - t0
    # one long problem among 30,000 short ones (64 bytes each, behind the long ones): one workgroup per problem
    short0 = first + 4 * (L + 4096) + 64
    shorts = [(short0 + 64 * k, short0 + 64 * k + 61) for k in range(30000)]
    sw = [np.zeros(0, dtype=np.int64)] * 30000
    for k in range(0, 30000, 1000):
        hay[shorts[k][0] + 20:shorts[k][0] + 23] = X
        sw[k] = np.array([20, 21], dtype=np.int64)
    t0 = time.time()
    check_batch(ss, Batch(hay, shorts[:777] + [ranges[0]] + shorts[777:], [bytes([X]) * 2] * 30001), sw[:777] + [want[0]] + sw[777:],
                "one long problem among 30,000")
    t_one = time.time() - t0
    print("four long problems: %.3f s; one long among 30,000 (count + 2 x find_all passes, uploads included): %.3f s" % (t_long, t_one))


def test_two_threads_two_streams(ss, table):
    """7. Two threads on two streams calling concurrently get their own answers (call-owned scratch)."""
    b, want, text, words = table
    half = len(words) // 2
    parts = [Batch(b.hay, [(0, len(text))] * half, words[:half]), Batch(b.hay, [(0, len(text))] * (len(words) - half), words[half:])]
    wants = [want[:half], want[half:]]
    errors = []

    def work(k):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(6):
                    got = ss.count_batched(*parts[k].args(), **parts[k].kw())
                    counts, rows, offs = ss.find_all_batched(*parts[k].args(), **parts[k].kw())
                    st.synchronize()
                    wc = np.array([w.size for w in wants[k]], dtype=np.int64)
                    assert np.array_equal(got.cpu().numpy(), wc) and np.array_equal(counts.cpu().numpy(), wc)
                    assert np.array_equal(offs.cpu().numpy(), np.concatenate(wants[k]))
        except Exception as e:          # noqa: BLE001
            errors.append((k, repr(e)))

    with batched_lib(ss):
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors


def test_single_and_batched_calls_on_different_streams_share_no_scratch(ss, table):
    """The single calls and the batched ones take their scratch from one free list.  ss_count_batched hands its buffer back without
    a wait, so a count() / find_all() on ANOTHER stream - a side stream is not ordered behind the default one - must not get it while
    the batched scan may still be reading its descriptors there: count_batched on the default stream from one thread, alternating
    with a searcher's count() and find_all() on a side stream from a second thread; every answer is checked."""
    b, want, text, words = table
    wc = np.array([w.size for w in want], dtype=np.int64)
    errors, stop = [], threading.Event()
    with batched_lib(ss):
        word = words[int(np.argmax(wc))]
        s = ss.DynamicHipSearcher(word)
        want_one = want[int(np.argmax(wc))]

        def singles():
            try:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    while not stop.is_set():
                        assert s.count(b.hay) == want_one.size
                        assert np.array_equal(s.find_all(b.hay).cpu().numpy(), want_one)
            except Exception as e:          # noqa: BLE001
                errors.append(("single", repr(e)))

        t = threading.Thread(target=singles)
        t.start()
        try:
            for _ in range(300):
                got = ss.count_batched(*b.args(), **b.kw())             # the default stream; no wait in between
                got2 = ss.count_batched(*b.args(), **b.kw())
                assert np.array_equal(got.cpu().numpy(), wc) and np.array_equal(got2.cpu().numpy(), wc)
        finally:
            stop.set()
            t.join()
    assert not errors, errors


def test_a_capturing_stream_is_refused(ss, table):
    """Both calls answer SS_ERR_ARGUMENT on a capturing stream, as ss_search_batched does, and launch nothing into the capture."""
    b = table[0]
    with batched_lib(ss):
        L = ss.lib()
        counts = torch.zeros(b.count, dtype=torch.int64, device="cuda")
        rows = torch.zeros(b.count + 1, dtype=torch.int64, device="cuda")
        tot = ctypes.c_uint64(0)
        ranges = (b.hay.data_ptr(), b.hb.data_ptr(), b.he.data_ptr(), b.nd.data_ptr(), b.nb.data_ptr(), b.ne.data_ptr(), b.count)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            counts.zero_()                                               # (something to capture: the refused calls add nothing)
            st = torch.cuda.current_stream().cuda_stream
            rc1 = L.ss_count_batched(*ranges, st, counts.data_ptr())
            msg = L.ss_last_error()
            rc2 = L.ss_find_all_batched(*ranges, st, counts.data_ptr(), rows.data_ptr(), None, 0, ctypes.byref(tot))
        assert rc1 == ss.SS_ERR_ARGUMENT and rc2 == ss.SS_ERR_ARGUMENT and b"hipGraph" in msg, (rc1, rc2, msg)
        # and the calls work as before afterwards
        assert L.ss_count_batched(*ranges, None, counts.data_ptr()) == 0
        torch.cuda.synchronize()
        assert int(counts.sum()) == 716940


def test_grep_hip_counts_several_patterns_in_one_call(ss, corpus, tmp_path):
    """tools/grep_hip.py --count with -e repeated and -f FILE: one count per pattern and line, in the order given."""
    import subprocess
    import sys
    text = corpus["i386"]
    pats = [b"the", b"Intel", b"no such phrase", b"register", b"aa"]
    f = tmp_path / "patterns.txt"
    f.write_bytes(b"\n".join(pats[3:]) + b"\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py"), "--count", "-e", "the", "-e", "Intel", "-e", "no such phrase",
                          "-f", str(f), os.path.join(ROOT, "tests", "golden", "data", "i386.txt")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert [int(l) for l in out.stdout.split()] == [find_stepping(text, p).size for p in pats]


def test_python_refuses_outside_the_build(ss, table):
    b = table[0]
    with pytest.raises(ss.SlicesliceError, match="matches_batched_build"):
        ss.count_batched(*b.args(), **b.kw())
    with pytest.raises(ss.SlicesliceError, match="matches_batched_build"):
        ss.find_all_batched(*b.args(), **b.kw())


def test_campaign(ss):
    """8. tools/fuzz_matches_batched.py for a bounded time."""
    import json
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_matches_batched.py"), "12", "4244"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["fuzz_matches_batched"] == "ok" and d["rounds"] >= 10 and d["csr"] >= 1, d
