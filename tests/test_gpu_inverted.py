"""GPU tests of the inverted line calls (include/sliceslice_hip_inverted.h, libsliceslice_hip_inverted.so):
ss_count_lines_inverted_device / _async and ss_find_lines_inverted_device against the rule restated on numpy arrays - every line of
the view minus the lines that tests/test_gpu_bounded.py's and tests/test_gpu_lines.py's rules call matching - against
tests/golden/inverted_kat.json, and against the library's own non-inverted and empty-needle calls: the two counts add up to the
number of lines and the two record sets merge into the empty needle's.  Every comparison is of integers and exact; every output
array is a window of a larger one whose sentinels on both sides must survive."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_gpu_bounded import (GOLDEN, LENGTHS, MiB, NEIGHBOURS, SENT, TILE, Window, _LOWER, dev_of, mixed_case, needle_of,
                              ref_lines as ref_bounded_lines)
from test_gpu_matches import _loaded, kernel_of, n_tiles, ref_offsets, tiles_per_workgroup

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# how -> the keywords of the Python methods; the bits of `how` are W = 1, X = 2, I = 4
HOWS = {"": {}, "i": dict(ignore_case=True), "w": dict(whole_word=True), "wi": dict(whole_word=True, ignore_case=True),
        "x": dict(whole_line=True), "xi": dict(whole_line=True, ignore_case=True)}


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with inverted_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "inverted_kat.json")))


@pytest.fixture(scope="module")
def manual():
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    return data, torch.from_numpy(data.copy()).cuda()


def inverted_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the inverted entry points, else `ss.inverted_build()`."""
    return _loaded() if getattr(ss.lib(), "has_inverted", False) else ss.inverted_build()


def make(ss, needle, position=None, triple=None):
    with inverted_lib(ss):
        s = ss.DynamicHipSearcher(needle, position)
        if triple is not None:
            s.set_filter(*triple)
        return s


# ---- the rule on numpy arrays ---------------------------------------------------------------------------------------------------
def every_line(h, delim):
    """(begin, end, number) of every line of h: cut at `delim`, an unterminated last line is a line, an empty h has none"""
    h = np.asarray(h, dtype=np.uint8)
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, h.size, dtype=np.int64)))
    if begins[-1] == h.size:
        begins, ends = begins[:-1], ends[:-1]
    return begins, ends, np.arange(1, begins.size + 1, dtype=np.int64)


def matching_numbers(h, needle, delim, how):
    """the 1-based numbers of the lines that MATCH under `how`: the non-inverted rule"""
    h = np.asarray(h, dtype=np.uint8)
    nocase = how.endswith("i")
    nd = bytes(needle).lower() if nocase else bytes(needle)
    if how[:1] in ("w", "x"):
        return ref_bounded_lines(h, nd, delim, how[0] == "x", nocase)[2]
    if len(nd) == 0:
        return every_line(h, delim)[2]
    if delim in nd or len(nd) > h.size:
        return np.zeros(0, dtype=np.int64)
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    offs = ref_offsets(_LOWER[h] if nocase else h, nd)
    first = np.searchsorted(dpos, offs, side="left")
    inside = np.searchsorted(dpos, offs + len(nd) - 1, side="right") == first       # (folded, a delimiter 'A' can look like a needle byte)
    return np.unique(first[inside]).astype(np.int64) + 1


def ref_inverted(h, needle, delim, how):
    """((begin, end, number) of the selected lines, of the matching lines, of every line)"""
    every = every_line(h, delim)
    hit = np.zeros(every[0].size, dtype=bool)
    hit[matching_numbers(h, needle, delim, how) - 1] = True
    return tuple(a[~hit] for a in every), tuple(a[hit] for a in every), every


def records(s, dev, delim, total, inverted, kw, what):
    """the records of find_lines(_inverted)_into at exact capacity, through sentinel windows; returns three numpy arrays"""
    ws = [Window(total) for _ in range(3)]
    fn = s.find_lines_inverted_into if inverted else s.find_lines_into
    assert fn(dev, ws[0].view, ws[1].view, ws[2].view, total, delim, **kw) == total, (what, inverted, kw)
    out = []
    for w in ws:
        h = w.buf.cpu().numpy()
        assert (h[:8] == SENT).all() and (h[8 + total:] == SENT).all(), (what, inverted, kw)
        out.append(h[8:8 + total])
    return out


_EMPTY = {}


def empty_needle(ss):
    if "s" not in _EMPTY:
        _EMPTY["s"] = make(ss, b"")
    return _EMPTY["s"]


def check(ss, s, dev, host, needle, delim, how, what, complement=True):
    """the inverted count and records against the rule; `complement`: against the library's own non-inverted and empty-needle calls
    too.  Returns the number of selected lines."""
    kw = HOWS[how]
    what = (what, bytes(needle)[:24], delim, how)
    sel, hit, every = ref_inverted(host, needle, delim, how)
    got = s.count_lines_inverted(dev, delim, **kw)
    assert got == sel[0].size, (what, got, sel[0].size, every[0].size)
    inv = records(s, dev, delim, got, True, kw, what)
    for g, w in zip(inv, sel):
        assert (g == w).all(), (what, g[:6], w[:6])
    if complement and not (len(needle) == 0 and how[:1] in ("w", "x")):
        e = empty_needle(ss)
        nlines = e.count_lines(dev, delim)
        plain = s.count_lines(dev, delim, **kw)
        assert plain == hit[0].size and plain + got == nlines == every[0].size, (what, plain, got, nlines, every[0].size)
        non = records(s, dev, delim, plain, False, kw, what)
        alls = records(e, dev, delim, nlines, False, {}, what)
        assert not set(non[2].tolist()) & set(inv[2].tolist()), what
        order = np.argsort(np.concatenate((non[2], inv[2])), kind="stable")
        for k in range(3):
            assert (np.concatenate((non[k], inv[k]))[order] == alls[k]).all() and (alls[k] == every[k]).all(), (what, k)
    return got


# ---- 1: the fixture -------------------------------------------------------------------------------------------------------------
def test_only_the_inverted_library_has_the_entry_points(ss):
    with ss.bounded_build() as L:
        assert not L.has_inverted
        t = ss.DynamicHipSearcher(b"abc")
    with ss.inverted_build() as L:
        assert L.has_inverted and L.has_bounded and L.has_nocase and L.has_lines and L.has_matches and not L.has_matches_batched
    d = dev_of(np.frombuffer(b"abc abc\nxyz", dtype=np.uint8))
    for call in (lambda: t.count_lines_inverted(d), lambda: t.find_lines_inverted(d, whole_word=True),
                 lambda: t.count_lines_inverted_async(d, d), lambda: t.find_lines_inverted_into(d, None, None, None, 0)):
        with pytest.raises(ss.SlicesliceError, match="inverted_build"):
            call()
    # a searcher of the inverted library takes every call it is built on
    s = make(ss, b"abc")
    assert (s.count(d), s.count_lines(d), s.count_lines(d, whole_line=True), s.count_lines_inverted(d), s.count_lines_inverted(d, whole_line=True)) == \
        (2, 1, 0, 1, 2)


def test_the_small_case_table(ss, kat):
    for c in kat["cases"]:
        hay, needle = bytes.fromhex(c["haystack"]), bytes.fromhex(c["needle"])
        kw = HOWS[c["how"]]
        s = make(ss, needle)
        h = np.frombuffer(hay, dtype=np.uint8)
        d = dev_of(h)
        assert s.count_lines_inverted(d, c["delimiter"], **kw) == len(c["records"]), c["what"]
        b, e, n = (t.cpu().tolist() for t in s.find_lines_inverted(d, bytes([c["delimiter"]]), **kw))
        assert [list(r) for r in zip(b, e, n)] == c["records"], (c["what"], b, e, n)
        # ... and the restatement of this file agrees with the fixture
        assert [list(r) for r in zip(*(a.tolist() for a in ref_inverted(h, needle, c["delimiter"], c["how"])[0]))] == c["records"], c["what"]


def test_every_golden_word_of_the_manual(ss, kat, manual):
    data, d = manual
    rows = [(w.encode("latin-1"), {how: kat["inverted"][how][j] for how in kat["hows"]}) for j, w in enumerate(kat["words"])]
    rows += [(w.encode(), t) for w, t in kat["table"].items()]
    assert len(rows) >= 40 and sorted(kat["hows"]) == sorted(HOWS)
    assert empty_needle(ss).count_lines(d) == kat["lines"]
    out = torch.full((3,), SENT, dtype=torch.int64, device="cuda")
    bad = []
    for w, want in rows:
        for how, kw in HOWS.items():
            nd = w.lower() if how.endswith("i") else w
            s = make(ss, nd)
            got = check(ss, s, d, data, nd, 10, how, "manual", complement=False)
            s.count_lines_inverted_async(d, out[1:2], **kw)
            torch.cuda.synchronize()
            if (got, out.cpu().tolist()) != (want[how], [SENT, want[how], SENT]):
                bad.append((w, how, got, out.cpu().tolist(), want[how]))
    assert not bad, bad[:10]
    assert kat["table"]["the"] == {"": 16053, "i": 15365, "w": 16438, "wi": 15984, "x": 20854, "xi": 20854}
    for how in ("", "w", "xi"):                                 # the complement on the manual, once per kind
        check(ss, make(ss, b"the"), d, data, b"the", 10, how, "manual")


# ---- 3: small views -------------------------------------------------------------------------------------------------------------
def test_small_views(ss):
    rng = np.random.default_rng(81)
    pool = np.frombuffer(b"ab \n", dtype=np.uint8)
    needles = [b"ab", b"zz", b"ab" * 21, b"a\nb", b""]           # present, absent, longer than every view, holding the delimiter, empty
    searchers = [(nd, make(ss, nd)) for nd in needles]
    rot = ["i", "w", "x", "wi", "xi"]
    seen = [0, 0]
    for L in range(0, 41):
        for trailing in (False, True):
            host = rng.choice(pool, size=L + 16, p=[0.3, 0.3, 0.2, 0.2])
            if L:
                host[8 + L - 1] = 10 if trailing else ord("b")
            host[7], host[8 + L] = 10, ord("a")                  # (a delimiter and a needle byte just outside)
            dev = dev_of(host)
            view, hv = dev[8:8 + L], host[8:8 + L]
            for j, (nd, s) in enumerate(searchers):
                for how in ("", rot[(L + j) % 5]):
                    if len(nd) == 0 and how[:1] in ("w", "x"):
                        continue
                    got = check(ss, s, view, hv, nd, 10, how, "small %d %s" % (L, trailing))
                    if nd in (b"ab" * 21, b"a\nb"):
                        assert got == every_line(hv, 10)[0].size, (L, nd)     # no line can match: every line, not 0
                    if nd == b"":
                        assert got == 0
                    seen[0] += got
                    seen[1] += 1
    assert seen[0] > 0 and seen[1] > 500
    # delimiter-only haystacks, and a single unterminated line that matches or does not
    a, z = make(ss, b"ab"), make(ss, b"zz")
    for L in (1, 2, 15, 16, 17, 40):
        host = np.full(L, 10, dtype=np.uint8)
        for how in HOWS:
            assert check(ss, a, dev_of(host), host, b"ab", 10, how, "delimiters only") == L
        line = np.frombuffer((b"xy ab " * 8)[:L], dtype=np.uint8) if L > 2 else np.frombuffer(b"ab"[:L], dtype=np.uint8)
        assert check(ss, a, dev_of(line), line, b"ab", 10, "", "one open line") == (0 if L >= 2 else 1)
        assert check(ss, z, dev_of(line), line, b"zz", 10, "w", "one open line") == 1


# ---- 4: carries across every border ---------------------------------------------------------------------------------------------
def text(rng, size, p_delim=0.03):
    return rng.choice(np.frombuffer(b"abAB \n", dtype=np.uint8), size=size, p=[0.3, 0.3, 0.1, 0.1, 0.2 - p_delim, p_delim])


def test_sizes_around_tiles_and_more_than_256_workgroups(ss):
    rng = np.random.default_rng(82)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = make(ss, b"abab")
    big = 5 * MiB
    # one tile per workgroup and more than 256 of them, so that lines_chunk_kernel has a second chunk: the launch shape of an
    # untuned search, as tests/test_gpu_matches.py restates it
    assert n_tiles(0, big, 4) == 320 and tiles_per_workgroup(320, cus, 0) == 1
    for L in (TILE - 1, TILE, TILE + 1, 2 * TILE, 5 * TILE, 5 * TILE + 333, big):
        host = text(rng, L)
        dev = dev_of(host)
        for how in (("", "wi") if L == big else HOWS):
            got = check(ss, s, dev, host, b"abab", 10, how, "size %d" % L)
            assert 0 < got < every_line(host, 10)[0].size or how[:1] == "x"
    # every byte a delimiter; no delimiter at all; a needle that holds the delimiter (the EVERY path) at the same sizes
    for L in (TILE + 1, 2 * TILE):
        host = np.full(L, 10, dtype=np.uint8)
        assert check(ss, s, dev_of(host), host, b"abab", 10, "", "all delimiters") == L
        host = text(rng, L, 0.0)
        assert check(ss, s, dev_of(host), host, b"abab", 10, "i", "no delimiter") == 0
        assert check(ss, make(ss, b"zzz"), dev_of(host), host, b"zzz", 10, "", "no delimiter, no match") == 1
        host = text(rng, L)
        assert check(ss, s, dev_of(host), host, b"abab", ord("b"), "", "needle holds the delimiter") == every_line(host, ord("b"))[0].size


def test_views_misaligned_at_both_ends(ss):
    rng = np.random.default_rng(83)
    G = 64
    searchers = [(nd, make(ss, nd)) for nd in (b"ab", b"abab", b"a")]
    hows = list(HOWS)
    for mis in range(1, 16):
        for L in (1, 2, 5, 16, 17, 33, 1025, TILE + 1, 2 * TILE + 16 - mis):
            host = text(rng, L + 2 * G, 0.08)
            v0 = G + mis
            if mis % 2:
                host[v0 - 5:v0] = np.frombuffer(b"\nabab", dtype=np.uint8)              # copies and delimiters just outside
                host[v0 + L:v0 + L + 5] = np.frombuffer(b"abab\n", dtype=np.uint8)
            else:
                host[v0 - 2:v0] = np.frombuffer(b"a\n", dtype=np.uint8)
                host[v0 + L:v0 + L + 2] = np.frombuffer(b"\nb", dtype=np.uint8)
            dev = dev_of(host)
            for j, (nd, s) in enumerate(searchers):
                check(ss, s, dev[v0:v0 + L], host[v0:v0 + L], nd, 10, hows[(mis + j + L) % 6], "mis %d len %d" % (mis, L))


def test_a_line_longer_than_tiles_workgroups_and_chunks(ss):
    rng = np.random.default_rng(84)
    nd = b"needle-z"
    s = make(ss, nd)
    for L, span in ((5 * TILE + 77, 3 * TILE + 500), (5 * MiB + 123, 4 * MiB + 300 * 1024)):
        p0 = TILE // 2 + 7                                       # the long line is [p0, p0 + span): no delimiter inside
        for where in ("first", "middle", "last", None):
            host = text(rng, L, 0.02)
            long = host[p0:p0 + span]
            long[long == 10] = ord(" ")
            host[p0 - 1] = host[p0 + span] = 10
            at = {"first": p0 + 3, "middle": p0 + span // 2, "last": p0 + span - len(nd) - 2, None: None}[where]
            if at is not None:
                host[at:at + len(nd)] = np.frombuffer(nd, dtype=np.uint8)
                host[at - 1] = host[at + len(nd)] = ord(" ")
            dev = dev_of(host)
            for how in ("", "w") if L > MiB else ("", "i", "w", "wi"):
                check(ss, s, dev, host, nd, 10, how, "long line %d %s" % (L, where))
                sel = ref_inverted(host, nd, 10, how)[0]
                assert int((sel[0] == p0).sum()) == (0 if where else 1), (L, where, how)    # absent, or once with the far-back begin
                if where is None:
                    assert sel[1][sel[0] == p0][0] == p0 + span


def test_delimiters_that_are_letters_needle_bytes_or_word_bytes(ss):
    rng = np.random.default_rng(85)
    L = 3 * TILE + 99
    host = rng.choice(np.frombuffer(b"aAbBx _0\n\x00", dtype=np.uint8), size=L, p=[0.2, 0.08, 0.2, 0.08, 0.14, 0.12, 0.06, 0.06, 0.03, 0.03])
    host[L - 4:] = np.frombuffer(b"\nbxb", dtype=np.uint8)
    dev = dev_of(host)
    for nd in (b"bxb", b"b", b"bx bx", b"b" * 17):
        s = make(ss, nd)
        for delim in (ord("a"), ord("A"), ord("_"), ord("0"), ord("x"), ord("b"), 0x00, 10):
            for how in HOWS:
                got = check(ss, s, dev, host, nd, delim, how, "delimiters")
                if delim in nd:
                    assert got == every_line(host, delim)[0].size


# ---- 5: all nine kernel choices in both units, without and with the neighbour test --------------------------------------------
def test_filter_shapes_all_nine_kernels_in_both_units(ss):
    rng = np.random.default_rng(86)
    L = 3 * TILE + 321
    base = needle_of(rng, 1400)
    rows = [("one byte", b"a", {}), ("mode0 q0", base[:40], dict(triple=(0, 2, 2))), ("mode0 q1", base[:40], dict(triple=(0, 5, 5))),
            ("mode0 q2", base[:40], dict(triple=(0, 9, 9))), ("mode0 q3", base[:40], dict(triple=(0, 13, 13))),
            ("mode0 q3 first at 2", base[:40], dict(triple=(2, 3, 15))),
            ("with_position 20", base[:48], dict(position=20)), ("with_position 47", base[:48], dict(position=47)),
            ("mode2 q0", base[:48], dict(triple=(0, 16, 16))), ("mode2 q1", base[:48], dict(triple=(3, 23, 23))),
            ("mode2 q2", base[:60], dict(triple=(0, 40, 40))), ("mode2 q3", base[:48], dict(triple=(5, 33, 33))),
            ("pair alone d=3", base[:70], dict(triple=(1, 61, 61))), ("far_off", base, dict(triple=(0, 1300, 1300)))]
    named = len(rows)
    rows += [("mode0 pair %d" % fb, base[:40], dict(triple=(0, fb, fb))) for fb in (1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15)]
    rows += [("mode0 triple %d %d" % (fb, fc), base[:40], dict(triple=(0, fb, fc))) for fb, fc in ((1, 2), (4, 5), (8, 9), (12, 13))]
    rows += [("length %d" % n, needle_of(rng, n), {}) for n in LENGTHS if n > 1]
    kernels = set()
    for k, (name, nd, kw) in enumerate(rows):
        s = make(ss, nd, **kw)
        if named <= k < named + 15 and kernel_of(s) in kernels:
            continue
        kernels.add(kernel_of(s))
        nl = len(nd)
        host = rng.choice(np.frombuffer(b"azmAZM \n_", dtype=np.uint8), size=L + 64, p=[0.14, 0.14, 0.14, 0.1, 0.1, 0.1, 0.14, 0.07, 0.07])
        at, j = 100, 0
        while at + nl + 64 < L:
            host[at:at + nl] = mixed_case(rng, nd) if j % 2 else np.frombuffer(nd, dtype=np.uint8)
            host[at - 1] = NEIGHBOURS[j % len(NEIGHBOURS)]
            host[at + nl] = NEIGHBOURS[(3 * j + 5) % len(NEIGHBOURS)]
            at, j = at + nl + int(rng.integers(20, 3000)), j + 1
        dev = dev_of(host)
        before = s.tuning_state(dev[:L])
        for mis in (0, 11):
            for how in ("", "i", "w", "wi") + (("x", "xi") if k < 2 else ()):       # both units, without and with the neighbour test
                got = check(ss, s, dev[mis:mis + L], host[mis:mis + L], nd, 10, how, "%s mis %d" % (name, mis), complement=mis == 0)
                assert got >= 1, (name, how)
        assert s.tuning_state(dev[:L]) == before, name
    want = {(q, m, False) for q in range(4) for m in (0, 2)} | {(0, 0, True)}
    assert kernels == want, sorted(want - kernels)


# ---- 6: capacity ----------------------------------------------------------------------------------------------------------------
def test_capacity_cuts_and_the_last_line_at_the_cut(ss):
    rng = np.random.default_rng(87)
    s = make(ss, b"bxb")
    for tail, what in ((b"\nb b", "an open last line that is selected"), (b"\nbxb", "an open last line that matches"), (b"bx\n", "closed")):
        host = rng.choice(np.frombuffer(b"bx \n", dtype=np.uint8), size=2 * TILE + 50, p=[0.4, 0.3, 0.2, 0.1])
        host[host.size - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
        dev = dev_of(host)
        for how in ("", "w", "xi"):
            kw = HOWS[how]
            ref = ref_inverted(host, b"bxb", 10, how)[0]
            total = ref[0].size
            assert total >= 3 and (ref[1][-1] == host.size) == (tail == b"\nb b"), (what, how)      # the open last line's record is the last one
            for cap in (0, 1, total - 1, total, total + 1):
                for skip in (None, 0, 1, 2):
                    ws = [Window(cap) for _ in range(3)]
                    args = [None if (k == skip or cap == 0) else ws[k].view for k in range(3)]
                    assert s.find_lines_inverted_into(dev, args[0], args[1], args[2], cap, **kw) == total, (what, how, cap, skip)
                    for k in range(3):
                        ws[k].check(ref[k][:0 if (k == skip or cap == 0) else min(cap, total)], (what, how, cap, skip, k))
            b, e, n = (t.cpu().numpy() for t in s.find_lines_inverted(dev, capacity=None, **kw))      # sized from the inverted count
            assert b.size == total and (b == ref[0]).all() and (e == ref[1]).all() and (n == ref[2]).all(), (what, how)
            check(ss, s, dev, host, b"bxb", 10, how, what)


# ---- 7: launch shapes -----------------------------------------------------------------------------------------------------------
def test_a_160_mib_haystack_of_40_chunks_at_one_tile_per_workgroup(ss):
    n_bytes = 160 * MiB                                     # (one tile per workgroup; the size and the construction of tests/test_gpu_bounded.py's twin)
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x0B0D)
    hay.masked_fill_(hay == ord("Q"), ord("r"))
    hay.masked_fill_(hay == ord("q"), ord("r"))
    hay.masked_fill_(hay == 10, 11)                         # delimiter-sparse: the only delimiters are the planted ones
    rng = np.random.default_rng(88)
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
        copy = np.concatenate((np.frombuffer(b"w" if k % 3 == 0 else (b" " if k % 3 == 1 else b"\n"), dtype=np.uint8),
                               mixed_case(rng, needle) if k % 2 else np.frombuffer(needle, dtype=np.uint8),
                               np.frombuffer(b"_" if k % 5 == 0 else b"\n", dtype=np.uint8)))
        hay[p - 1:p + n + 1] = torch.from_numpy(copy).cuda()
    for p in rng.integers(1, n_bytes - 100, size=200):      # lines without a copy
        hay[int(p)] = 10
    host = hay.cpu().numpy()
    before = s.tuning_state(hay)
    for sr, nd, hows in ((s, needle, ("", "wi", "x")), (s2, b"qz", ("i",))):
        for how in hows:
            got = check(ss, sr, hay, host, nd, 10, how, "large")
            assert 100 < got < every_line(host, 10)[0].size
    assert s.tuning_state(hay) == before
    # the async form on a side stream
    side = torch.cuda.Stream()
    out = torch.full((3,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s.count_lines_inverted_async(hay, out[1:2], whole_word=True)
    side.synchronize()
    assert out.cpu().tolist() == [SENT, ref_inverted(host, needle, 10, "w")[0][0].size, SENT]
    del hay
    torch.cuda.empty_cache()


def test_offsets_above_2_32(ss):
    """the construction of tests/test_gpu_bounded.py's twin, delimiter-sparse: runs of kept and not-kept copies and of delimiters
    around 2^32 and at the end of a haystack that holds neither elsewhere; the reference is built from host copies of the planted
    regions and of the delimiters' positions alone"""
    n_bytes = (1 << 32) + 64 * MiB
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0x0B33)
    step = 1 << 30
    for lo in range(0, n_bytes, step):                      # (in slices: the masks are temporaries of the slice's size)
        part = hay[lo:lo + step]
        part.masked_fill_(part == ord("q"), ord("r"))
        part.masked_fill_(part == 10, 11)
    needle = b"qz-needle"
    n = len(needle)
    seps = [b" ", b"_", b"", b"\n", b"\n", b"k", b".", b"\n\n", b" "]
    run = b"".join(seps[k % len(seps)] + needle for k in range(60)) + b"\n"
    starts = [(1 << 32) - 2000, (1 << 32) - len(run) // 2, (1 << 32) + 1000, (1 << 32) + 3 * TILE - 100, n_bytes - len(run) - 40]
    assert len(run) + 16 < 1000 - len(run) // 2
    tail = b"\n no copy here"                               # an unterminated last line that is selected
    planted = [(p, run) for p in starts] + [(n_bytes - len(tail), tail)]
    for p0, t in planted:
        hay[p0:p0 + len(t)] = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda()
    dpos = np.concatenate([(torch.nonzero(hay[lo:lo + step] == 10).flatten() + lo).cpu().numpy() for lo in range(0, n_bytes, step)])
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, n_bytes, dtype=np.int64)))
    numbers = np.arange(1, begins.size + 1, dtype=np.int64)
    assert begins[-1] < n_bytes and 50 < begins.size < 1000 and dpos.min() < (1 << 32) < dpos.max()
    s = make(ss, needle)
    from test_gpu_bounded import ref_kept
    for how in ("", "w", "x"):
        offs = []
        for p0, t in planted:
            lo, hi = p0 - 8, min(p0 + len(t) + 8, n_bytes)  # (the margins hold no 'q')
            window = hay[lo:hi].cpu().numpy()
            offs.append((ref_offsets(window, needle) if how == "" else ref_kept(window, needle, False, how == "x", 10)) + lo)
        hit = np.zeros(begins.size, dtype=bool)
        hit[np.searchsorted(dpos, np.concatenate(offs), side="left")] = True
        want = (begins[~hit], ends[~hit], numbers[~hit])
        kw = HOWS[how]
        total = want[0].size
        assert total >= 10 and want[1][-1] == n_bytes and s.count_lines_inverted(hay, **kw) == total, (how, total)
        assert s.count_lines(hay, **kw) + total == begins.size
        ws = [Window(total) for _ in range(3)]
        assert s.find_lines_inverted_into(hay, ws[0].view, ws[1].view, ws[2].view, total, **kw) == total, how
        for win, ref in zip(ws, want):
            win.check(ref, ("above 2^32", how))
    del hay, part
    torch.cuda.empty_cache()


# ---- 8: refusals, constructors, a pinned triple, a capturing stream ----------------------------------------------------------
def test_every_refusal_writes_nothing(ss):
    text_ = np.frombuffer(b"abc abc\nxyz\nabc", dtype=np.uint8)
    d = dev_of(text_)
    s, empty, upper = make(ss, b"abc"), make(ss, b""), make(ss, b"Abc")
    W, X, I = ss.searcher.SS_BOUND_WORD, ss.searcher.SS_BOUND_LINE, ss.searcher.SS_BOUND_NOCASE
    with inverted_lib(ss):
        L = ss.lib()
    out = Window(4)
    st = torch.cuda.current_stream().cuda_stream
    before = s.tuning_state(d)

    def refused(h, how, delim=10, match=()):
        c = ctypes.c_uint64(0xA5A5)
        p, n, o = d.data_ptr(), d.numel(), out.view.data_ptr()
        forms = {"count_lines_inverted_device": lambda: L.ss_count_lines_inverted_device(h, p, n, delim, how, st, ctypes.byref(c)),
                 "count_lines_inverted_device_async": lambda: L.ss_count_lines_inverted_device_async(h, p, n, delim, how, st, o),
                 "find_lines_inverted_device": lambda: L.ss_find_lines_inverted_device(h, p, n, delim, how, st, o, None, None, 4, ctypes.byref(c))}
        for name, call in forms.items():
            rc = call()
            msg = L.ss_last_error().decode()
            assert rc == ss.SS_ERR_ARGUMENT and c.value == 0xA5A5, (name, how, rc, c.value)
            for m in match:
                assert m in msg, (name, how, msg)
        torch.cuda.synchronize()
        out.check([], ("refusal", how))

    refused(s._h, W | X, match=("both", "inverted"))
    refused(s._h, W | X | I, match=("both",))
    for how in (8, W | 8, X | 0x100, 0x80000000, 0x80000000 | I):
        refused(s._h, how, match=("bits", "inverted"))
    for how in (W, X, W | I, X | I):
        refused(empty._h, how, match=("empty needle",))
    for how in (I, W | I, X | I):
        refused(upper._h, how, match=("ss_searcher_new_nocase",))
    for delim in (-1, 256, 1000):
        refused(s._h, 0, delim=delim, match=("delimiter",))
    with pytest.raises(ss.SlicesliceError, match="both") as e:
        s.count_lines_inverted(d, whole_word=True, whole_line=True)
    assert e.value.code == ss.SS_ERR_ARGUMENT
    with pytest.raises(ss.SlicesliceError, match="empty needle"):
        empty.find_lines_inverted(d, whole_line=True)
    # the same searchers are taken where the rule allows them
    assert (upper.count_lines_inverted(d), s.count_lines_inverted(d), s.count_lines_inverted(d, whole_line=True), empty.count_lines_inverted(d),
            empty.count_lines_inverted(d, ignore_case=True)) == (3, 1, 2, 0, 0)
    assert s.tuning_state(d) == before
    # the async count refuses a capturing stream, naming itself, and writes nothing
    lines = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    s.count_lines_inverted_async(d, probe)                  # (first use outside the capture)
    torch.cuda.synchronize()
    assert probe.item() == 1
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g):
        probe.fill_(7)
        try:
            s.count_lines_inverted_async(d, lines, whole_word=True)
        except ss.SlicesliceError as x:
            err = x
    assert err is not None and err.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(err) and "ss_count_lines_inverted_device_async" in str(err), err
    torch.cuda.synchronize()
    assert lines.item() == SENT


def test_every_constructor_and_a_pinned_triple_agree(ss):
    rng = np.random.default_rng(89)
    host = text(rng, 3 * TILE + 41, 0.04)
    dev = dev_of(host)
    nd = b"abab ab"
    with inverted_lib(ss):
        made = [ss.DynamicHipSearcher(nd), ss.DynamicHipSearcher.new(nd), ss.DynamicHipSearcher.with_position(nd, 3), ss.HipSearcher(nd),
                ss.HipSearcher(nd, 5), ss.DynamicHipSearcher.new_nocase(b"ABAB ab")]
        pinned = ss.DynamicHipSearcher(nd)
        pinned.set_filter(1, 4, 6)
        byte = ss.MemchrHipSearcher(ord("a"))
    for how in HOWS:
        want = ref_inverted(host, nd, 10, how)[0]
        for k, s in enumerate(made + [pinned]):
            before = s.tuning_state(dev)
            assert check(ss, s, dev, host, nd, 10, how, "constructor %d" % k, complement=k == 0) == want[0].size
            assert s.tuning_state(dev) == before, (how, k)
    want = ref_inverted(host, b"a", 10, "w")[0]
    assert byte.count_lines_inverted(dev, whole_word=True) == want[0].size
    b, e, n = (t.cpu().numpy() for t in byte.find_lines_inverted(dev, whole_word=True))
    assert (b == want[0]).all() and (e == want[1]).all() and (n == want[2]).all()
    w = Window(want[0].size)
    assert byte.find_lines_inverted_into(dev, None, w.view, None, want[0].size, whole_word=True) == want[0].size
    w.check(want[1], "memchr")
    out = torch.full((3,), SENT, dtype=torch.int64, device="cuda")
    byte.count_lines_inverted_async(dev, out[1:2], whole_word=True)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [SENT, want[0].size, SENT]
