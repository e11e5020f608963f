"""GPU tests of the matching-lines calls (include/sliceslice_hip_lines.h, libsliceslice_hip_lines.so): ss_count_lines_device / _async
and ss_find_lines_device against tests/golden/lines_kat.json and against the rule restated in Python - cut the view at every
delimiter byte, drop a trailing empty piece, a line matches when the needle occurs inside it.  Records are compared bit-exact."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from test_gpu_matches import KERNEL_ROWS, _kernel_row, kernel_of, ref_offsets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MiB = 1 << 20
TILE = 16384                    # bytes per tile: 4 waves x 4 pieces of 1 KiB
SENT = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with m.lines_build():
        pass
    return m


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "lines_kat.json")))


def make(ss, needle, position=None, triple=None, memchr=False):
    with ss.lines_build():
        if memchr:
            return ss.MemchrHipSearcher(needle[0])
        s = ss.DynamicHipSearcher(needle, position)
        if triple is not None:
            s.set_filter(*triple)
        return s


def ref_lines(h, needle, delim):
    """(begin, end, number) int64 arrays of the matching lines of h: the rule, on numpy arrays."""
    h = np.asarray(h, dtype=np.uint8)
    L = h.size
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, L, dtype=np.int64)))
    if begins[-1] == L:
        begins, ends = begins[:-1], ends[:-1]
    if len(needle) == 0:
        k = np.arange(begins.size, dtype=np.int64)
    elif delim in bytes(needle):
        k = np.zeros(0, dtype=np.int64)
    else:
        k = np.unique(np.searchsorted(dpos, ref_offsets(h, needle), side="left")).astype(np.int64)
    return begins[k], ends[k], k + 1


def dev_of(host):
    host = np.asarray(host, dtype=np.uint8)
    return torch.from_numpy(host.copy()).cuda() if host.size else torch.empty(0, dtype=torch.uint8, device="cuda")


def check(s, hay_dev, hay_host, needle, delim=10, what=""):
    wb, we, wn = ref_lines(hay_host, needle, delim)
    got = s.count_lines(hay_dev, delim)
    assert got == wb.size, (what, needle[:32], delim, got, wb.size)
    b, e, n = (t.cpu().numpy() for t in s.find_lines(hay_dev, delim))
    assert b.size == wb.size and (b == wb).all() and (e == we).all() and (n == wn).all(), \
        (what, needle[:32], delim, b[:6], e[:6], n[:6], wb[:6], we[:6], wn[:6])
    return wb, we, wn


def test_only_the_lines_library_has_the_entry_points(ss):
    assert not getattr(ss.lib(), "has_lines", False)
    with ss.matches_build() as L:
        assert not L.has_lines
    with ss.lines_build() as L:
        assert L.has_lines and L.has_matches and not L.has_matches_batched


def test_the_small_case_table(ss, kat):
    for c in kat["cases"]:
        hay, needle = bytes.fromhex(c["haystack"]), bytes.fromhex(c["needle"])
        s = make(ss, needle)
        d = dev_of(np.frombuffer(hay, dtype=np.uint8))
        want = c["records"]
        assert s.count_lines(d, c["delimiter"]) == len(want), c["what"]
        b, e, n = (t.cpu().tolist() for t in s.find_lines(d, bytes([c["delimiter"]])))
        assert [list(r) for r in zip(b, e, n)] == want, (c["what"], b, e, n)
    with ss.lines_build():
        s = ss.DynamicHipSearcher(b"a")
        d = dev_of(np.frombuffer(b"a\nb", dtype=np.uint8))
        for bad in (-1, 256, 1000):
            with pytest.raises(ss.SlicesliceError):
                s.count_lines(d, bad)
        assert ss.MemchrHipSearcher(ord("a")).count_lines(d) == 1


def test_every_word_of_the_manual(ss, kat):
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    words = open(os.path.join(GOLDEN, "data", "words.txt"), "rb").read().split()
    d = dev_of(data)
    assert make(ss, b"").count_lines(d) == kat["i386_lines"]
    got = [make(ss, w).count_lines(d) for w in words]
    bad = [(w, g, k) for w, g, k in zip(words, got, kat["count_lines"]) if g != k]
    assert not bad, bad[:10]
    assert sum(got) == kat["total"] == 410509
    for w, want in kat["records"].items():
        needle = w.encode("latin-1")
        s = make(ss, needle)
        b, e, n = (t.cpu().tolist() for t in s.find_lines(d))
        assert len(b) == want["lines"], w
        assert hashlib.sha256(b"".join(struct.pack("<3Q", *r) for r in zip(b, e, n))).hexdigest() == want["sha256"], w
        # relations to the other calls of the same searcher
        total = s.count(d)
        assert len(b) <= total and (len(b) > 0) == s.search_in(d), w
        if b:
            assert b[0] <= s.find(d) < e[0], w
            assert all(n[k] < n[k + 1] and e[k] < b[k + 1] for k in range(len(b) - 1)), w


def test_misalignments_and_lengths_with_copies_outside_both_ends(ss):
    rng = np.random.default_rng(20)
    needle = b"ab"
    s3, s1, s0 = make(ss, b"abab"), make(ss, b"a"), make(ss, b"")
    G = 64
    for mis in range(16):
        for L in (0, 1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 16):
            host = rng.choice(np.frombuffer(b"ab\n", dtype=np.uint8), size=L + 2 * G, p=[0.45, 0.45, 0.1])
            v0 = G + mis
            # delimiters and needle copies immediately outside both ends; copies straddling both ends
            host[v0 - 5:v0] = np.frombuffer(b"\nabab", dtype=np.uint8)
            host[v0 + L:v0 + L + 5] = np.frombuffer(b"abab\n", dtype=np.uint8)
            if mis % 2:
                host[v0 - 1] = 10
                host[v0 + L] = 10
            dev = dev_of(host)
            assert dev.data_ptr() % 16 == 0
            for s, nd in ((make(ss, needle), needle), (s3, b"abab"), (s1, b"a"), (s0, b"")):
                check(s, dev[v0:v0 + L], host[v0:v0 + L], nd, 10, "mis %d len %d" % (mis, L))


def test_matches_of_one_line_across_every_border_count_once(ss):
    needle = b"needle"
    s = make(ss, needle)
    L = 3 * 2 * TILE + 500
    nb = np.frombuffer(needle, dtype=np.uint8)
    for border in (16, 1024, 4096, TILE, 2 * TILE):
        for mis in (0, 5):
            host = np.full(L + 32, ord("."), dtype=np.uint8)
            v = host[mis:mis + L]
            # one line around the border with matches on both sides of it and one straddling it; quiet lines around
            v[border - 700 if border > 800 else 1] = 10
            for p in (border - 40, border - 3, border + 9, border + 300):
                if p >= 0:
                    v[p:p + 6] = nb
            v[border + 900] = 10
            v[border + 950:border + 956] = nb               # a last line without delimiter
            dev = dev_of(host)
            wb, _, _ = check(s, dev[mis:mis + L], v, needle, 10, "border %d mis %d" % (border, mis))
            assert wb.size == 2


def test_a_line_over_many_workgroups(ss):
    needle = b"the needle"
    s = make(ss, needle)
    nb = np.frombuffer(needle, dtype=np.uint8)
    L = 40 * TILE + 123                                     # one tile per workgroup at this size: 41 workgroups
    for where in ("first", "middle", "none", "both"):
        host = np.full(L, ord("x"), dtype=np.uint8)
        host[100] = 10
        host[2 * TILE + 17] = 10                            # the long line opens in workgroup 2 ...
        host[30 * TILE + 5000] = 10                         # ... and closes in workgroup 30; nothing in between
        host[35 * TILE] = 10
        if where in ("first", "both"):
            host[2 * TILE + 300:2 * TILE + 310] = nb
        if where in ("middle", "both"):
            host[17 * TILE - 4:17 * TILE + 6] = nb          # across a workgroup border in the middle of the line
        host[36 * TILE:36 * TILE + 10] = nb                 # the unterminated last line matches too
        wb, we, wn = check(s, dev_of(host), host, needle, 10, where)
        if where == "none":
            assert wb.tolist() == [35 * TILE + 1] and wn.tolist() == [5]
        else:
            assert wb.tolist() == [2 * TILE + 18, 35 * TILE + 1] and we.tolist() == [30 * TILE + 5000, L] and wn.tolist() == [3, 5]
    # no delimiter at all: one line, the whole view
    host = np.full(L, ord("x"), dtype=np.uint8)
    host[20 * TILE:20 * TILE + 10] = nb
    wb, we, wn = check(s, dev_of(host), host, needle, 10, "no delimiter")
    assert (wb.tolist(), we.tolist(), wn.tolist()) == ([0], [L], [1])


def test_every_kernel_and_the_filter_bytes_do_not_matter(ss):
    with ss.lines_build():
        rows = [(name, needle, _kernel_row(ss, needle, spec)) for name, needle, spec in KERNEL_ROWS]
    assert all(getattr(s._L if hasattr(s, "_L") else s._inner._L, "has_lines", False) for _, _, s in rows)
    kernels = {kernel_of(s) for _, _, s in rows}
    assert kernels == {(q, m, False) for q in range(4) for m in (0, 2)} | {(0, 0, True)}, kernels
    L = 4 * TILE + 777
    G = 256
    answers = {}
    for name, needle, s in rows:
        n = len(needle)
        unit = needle[:4] if needle[:4] == needle[4:8] else needle[:3]
        for delim in (10, 0, 255, ord("w")):
            for mis in (0, 3, 9, 15):
                if delim == ord("w") and b"w" in needle:
                    continue
                rng = np.random.default_rng(1000 * n + 16 * delim + mis)    # (one haystack per needle: rows differ in the filter bytes only)
                host = np.frombuffer((unit * ((L + 2 * G) // len(unit) + 1))[:L + 2 * G], dtype=np.uint8).copy()
                cuts = rng.integers(0, host.size, size=host.size // (40 if mis % 2 else 900))
                host[cuts] = delim                          # lines of ~40 or ~900 bytes of dense matches
                host[G + mis - 1] = delim
                dev = dev_of(host)
                view = host[G + mis:G + mis + L]
                wb, _, _ = check(s, dev[G + mis:G + mis + L], view, needle, delim, "%s delim %d mis %d" % (name, delim, mis))
                key = (needle, delim, mis)
                assert answers.setdefault(key, wb.size) == wb.size
                assert n == 1 or wb.size > 0


def test_capacity_contract(ss):
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    d = dev_of(data)
    needle = b"segment"
    s = make(ss, needle)
    wb, we, wn = ref_lines(data, needle, 10)
    total = wb.size
    assert total > 100
    for cap in (0, 1, 7, total - 1, total, total + 1, total + 500):
        for skip in (None, 0, 1, 2):
            bufs = [torch.full((cap + 16,), SENT, dtype=torch.int64, device="cuda") for _ in range(3)]
            args = [None if (k == skip or cap == 0) else bufs[k][8:8 + cap] for k in range(3)]
            assert s.find_lines_into(d, args[0], args[1], args[2], cap) == total
            k = min(cap, total)
            for j, w in enumerate((wb, we, wn)):
                h = bufs[j].cpu().numpy()
                assert (h[:8] == SENT).all() and (h[8 + k:] == SENT).all(), (cap, skip, j)
                if j == skip or cap == 0:
                    assert (h == SENT).all(), (cap, skip, j)
                else:
                    assert (h[8:8 + k] == w[:k]).all(), (cap, skip, j)
    b, e, n = s.find_lines(d, capacity=5)
    assert b.cpu().tolist() == wb[:5].tolist() and n.cpu().tolist() == wn[:5].tolist() and e.dtype == torch.int64


def test_async_count_on_a_side_stream_and_tuning_state(ss):
    n_bytes = 64 * MiB
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x11E5)
    needle = b"\x01\x02\x03"
    s = make(ss, needle)
    before = s.tuning_state(hay)
    want = s.count_lines(hay)
    host = hay.cpu().numpy()
    assert want == ref_lines(host, needle, 10)[0].size
    side = torch.cuda.Stream()
    out = torch.full((3,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(3):
            s.count_lines_async(hay, out[1:2])
    side.synchronize()
    assert out.cpu().tolist() == [SENT, want, SENT]
    s.count_lines_async(hay, out[1:2], delimiter=b"\x00", stream=side.cuda_stream)
    side.synchronize()
    assert out.cpu().tolist()[1] == s.count_lines(hay, 0) == ref_lines(host, needle, 0)[0].size
    b, e, n = s.find_lines(hay)
    assert b.numel() == want
    assert s.tuning_state(hay) == before                    # the calls neither start nor feed the census
    # a capturing stream is refused, as ss_count_batched refuses it
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.graph(g):
        out.zero_()                                         # (something to capture: the refused call adds nothing)
        try:
            s.count_lines_async(hay, out[1:2])
        except ss.SlicesliceError as err:
            refused = err
    assert refused is not None and refused.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(refused), refused
    assert s.count_lines(hay) == want                       # and the calls work as before afterwards
    del hay
    torch.cuda.empty_cache()


def test_above_four_gib(ss):
    n_bytes = (4 << 30) + 96 * MiB
    free, _ = torch.cuda.mem_get_info()
    if free < n_bytes + (1 << 30):
        pytest.skip("a haystack above 4 GiB needs %d MiB of device memory, %d MiB are free" % (n_bytes >> 20, free >> 20))
    hay = torch.full((n_bytes,), ord("x"), dtype=torch.uint8, device="cuda")
    needle = b"above four GiB"
    nt = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
    two32 = 1 << 32
    delims = sorted({5, 1000, two32 - 70000, two32 - 9, two32 + 40, two32 + 90000, n_bytes - 3 * TILE, n_bytes - 1} |
                    {k * 256 * MiB + 77 for k in range(1, 17)})
    plants = [7, two32 - 60000, two32 - 7, two32 + 100, two32 + 95000, n_bytes - 2 * TILE]   # (two32 - 7: across 2^32, inside one line)
    for p in delims:
        hay[p] = 10
    for p in plants:
        hay[p:p + len(needle)] = nt
    bounds = [-1] + delims
    want = []
    for k in range(1, len(bounds)):
        lo, hi = bounds[k - 1] + 1, bounds[k]
        if any(lo <= p and p + len(needle) <= hi for p in plants):
            want.append((lo, hi, k))
    assert len(want) >= 5 and any(b < two32 < e for b, e, _ in want) and any(b > two32 for b, _, _ in want)
    s = make(ss, needle)
    assert s.count_lines(hay) == len(want)
    b, e, n = (t.cpu().tolist() for t in s.find_lines(hay))
    assert list(zip(b, e, n)) == want
    assert make(ss, b"").count_lines(hay) == len(delims)            # the last byte is a delimiter: no line behind it
    assert make(ss, b"x").count_lines(hay) == sum(1 for k in range(1, len(bounds)) if bounds[k] - bounds[k - 1] > 1)
    del hay
    torch.cuda.empty_cache()
