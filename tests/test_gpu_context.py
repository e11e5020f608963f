"""GPU tests of the context calls (include/sliceslice_hip_context.h, libsliceslice_hip_context.so): ss_lines_around_device and
ss_find_lines_context_device against the rule restated on numpy arrays (tests/test_context_cpu.py: context_rule over the numbers the
models' rules select, the records of tests/test_gpu_inverted.py's every_line), against tests/golden/context_kat.json (GNU grep's
output) and against the library's own find_lines calls.  Every comparison is of integers and exact; every output array is a window
of a larger one whose sentinels on both sides must survive."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_context_cpu import U64_MAX, checksum, context_rule, separators
from test_gpu_bounded import GOLDEN, GUARD, SENT, Window, dev_of
from test_gpu_inverted import HOWS, every_line, matching_numbers
from test_gpu_matches import _loaded

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_SENT = 0xA5
NL = 10


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with context_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "context_kat.json")))


@pytest.fixture(scope="module")
def manual():
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    return data, torch.from_numpy(data.copy()).cuda(), every_line(data, NL)


def context_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the context entry points, else `ss.context_build()`."""
    return _loaded() if getattr(ss.lib(), "has_context", False) else ss.context_build()


def make(ss, needle, nocase=False):
    with context_lib(ss):
        return ss.DynamicHipSearcher.new_nocase(needle) if nocase else ss.DynamicHipSearcher(needle)


_ANY = {}


def any_searcher(ss):
    """lines_around looks at no needle: one searcher for all of its tests"""
    if "s" not in _ANY:
        _ANY["s"] = make(ss, b"unused")
    return _ANY["s"]


class KindWindow:
    """`cap` bytes inside a larger device array filled with a sentinel"""
    def __init__(self, cap):
        self.cap = cap
        self.buf = torch.full((cap + 2 * GUARD,), KIND_SENT, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + cap]

    def check(self, want, what):
        h = self.buf.cpu().numpy()
        k = len(want)
        assert (h[:GUARD] == KIND_SENT).all() and (h[GUARD + k:] == KIND_SENT).all(), what
        assert (h[GUARD:GUARD + k] == np.asarray(want, dtype=np.uint8)).all(), (what, h[GUARD:GUARD + min(k, 6)], want[:6])


def expected(host, delim, selected, before, after):
    """(begin, end, number, kind) of the rule for the lines `selected` of `host`"""
    every = every_line(host, delim)
    numbers, kinds = context_rule(selected, every[2].size, before, after)
    return every[0][numbers - 1], every[1][numbers - 1], numbers, kinds


def check_call(call, want, what, caps=None, skips=(None,)):
    """call(d_begin, d_end, d_number, d_kind, capacity) -> total.  The count-only forms, then every capacity of `caps` (default: the
    exact one) with each array of `skips` left out: the leftmost min(total, capacity) entries, sentinels everywhere else."""
    total = len(want[2])
    assert call(None, None, None, None, 0) == total, (what, "capacity 0")
    for cap in ([total] if caps is None else caps):
        for skip in skips:
            ws = [Window(cap), Window(cap), Window(cap), KindWindow(cap)]
            views = [None if skip == j else w.view for j, w in enumerate(ws)]
            assert call(*views, cap) == total, (what, cap, skip)
            k = min(total, cap)
            for j, w in enumerate(ws):
                w.check(want[j][:0] if skip == j else want[j][:k], (what, "capacity", cap, "without", skip, "array", j))
    if total:                                                   # a positive capacity and no array: count only
        assert call(None, None, None, None, total) == total, (what, "no arrays")


def check_around(ss, dev, host, numbers, before, after, what, delim=NL, caps=None, skips=(None,)):
    s = any_searcher(ss)
    want = expected(host, delim, numbers, before, after)
    check_call(lambda b, e, n, k, cap: s.lines_around_into(dev, numbers, b, e, n, k, cap, before, after, delim), want,
               (what, list(numbers)[:8], before, after), caps, skips)
    return want


# ---- gating ---------------------------------------------------------------------------------------------------------------------
def test_only_the_context_library_has_the_entry_points(ss):
    names = ("ss_lines_around_device", "ss_find_lines_context_device")
    for build in (ss.matches_build, ss.lines_build, ss.nocase_build, ss.bounded_build, ss.inverted_build):
        with build() as L:
            assert not any(hasattr(L, n) for n in names) and not L.has_context, build
            outsider = ss.DynamicHipSearcher(b"abc")
        for meth, args in (("find_lines_context", (b"abc\n",)), ("find_lines_context_into", (b"abc\n", None, None, None, None, 0)),
                           ("lines_around", (b"abc\n", [1])), ("lines_around_into", (b"abc\n", [1], None, None, None, None, 0))):
            with pytest.raises(ss.SlicesliceError, match="context_build") as e:
                getattr(outsider, meth)(*args)
            assert e.value.code == ss.SS_ERR_ARGUMENT
    assert not any(hasattr(ss.lib(), n) for n in names)
    with context_lib(ss):
        L = ss.lib()
        assert all(hasattr(L, n) for n in names) and L.has_context and L.has_inverted
        b, e, n, k = ss.lines_around(b"one\ntwo\nthree\n", [2], before=1)                 # the module-level helper
    assert (b.tolist(), e.tolist(), n.tolist(), k.tolist()) == ([0, 4], [3, 7], [1, 2], [0, 1])
    assert n.dtype == torch.int64 and k.dtype == torch.uint8
    m = make(ss, b"w")
    with context_lib(ss):
        memchr = ss.MemchrHipSearcher(ord("w"))
    for s in (m, memchr):
        b, e, n, k = s.find_lines_context(b"one\ntwo\nthree\n", after=1)
        assert (b.tolist(), e.tolist(), n.tolist(), k.tolist()) == ([4, 8], [7, 13], [2, 3], [1, 0])
        assert [t.tolist() for t in s.lines_around(b"one\ntwo\nthree\n", [3])] == [[8], [13], [3], [1]]


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_every_golden_row(ss, kat, manual):
    host, dev, every = manual
    assert every[2].size == kat["lines"]
    for r in kat["rows"]:
        what = (r["needle"], r["how"], r["invert"], r["before"], r["after"])
        nocase = r["how"].endswith("i")
        s = make(ss, r["needle"].encode().lower() if nocase else r["needle"].encode(), nocase)
        kw = dict(HOWS[r["how"]], invert=r["invert"])
        assert s.find_lines_context_into(dev, None, None, None, None, 0, r["before"], r["after"], **kw) == (r["printed"], r["selected"]), what
        begin, end, number, kind = [t.cpu().numpy() for t in s.find_lines_context(dev, r["before"], r["after"], **kw)]
        assert number.size == r["printed"] and int(kind.sum()) == r["selected"] and separators(number) == r["separators"], what
        pairs = [list(p) for p in zip(number.tolist(), kind.tolist())]
        assert pairs[:20] == r["first"] and pairs[-20:] == r["last"] and checksum(number, kind) == r["sha256"], what
        # the records are the empty needle's for those numbers
        assert (begin == every[0][number - 1]).all() and (end == every[1][number - 1]).all(), what
    lines = make(ss, b"").find_lines(dev)
    assert [t.cpu().numpy().tolist() for t in lines] == [a.tolist() for a in every]


# ---- identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("how", list(HOWS))
def test_identities_with_the_models(ss, manual, how, invert):
    P = ss.CONTEXT_PART_BYTES
    host = manual[0][:3 * P + 1234]                             # four parts, an unterminated last line
    dev = dev_of(host)
    needle = b"      ;" if how[:1] == "x" else b"the"             # (a line the manual's first pages repeat)
    s = make(ss, needle, how.endswith("i"))
    kw = HOWS[how]
    model = [t.cpu().numpy() for t in (s.find_lines_inverted if invert else s.find_lines)(dev, **kw)]
    hit = matching_numbers(host, needle, NL, how)
    every = every_line(host, NL)
    n_lines = every[2].size
    chosen = np.setdiff1d(every[2], hit) if invert else hit
    assert chosen.size and (model[2] == chosen).all(), (how, invert)
    # nothing around them: the model's own records, all of kind 1
    got = [t.cpu().numpy() for t in s.find_lines_context(dev, 0, 0, invert=invert, **kw)]
    for g, w in zip(got[:3], model):
        assert (g == w).all(), (how, invert)
    assert got[3].size == chosen.size and (got[3] == 1).all()
    # everything around them: the empty needle's records, kind = membership
    member = np.isin(every[2], chosen).astype(np.uint8)
    for amount in (n_lines, n_lines + 1, U64_MAX):
        got = [t.cpu().numpy() for t in s.find_lines_context(dev, amount, amount, invert=invert, **kw)]
        for g, w in zip(got, every + (member,)):
            assert g.size == w.size and (g == w).all(), (how, invert, amount)
    # nothing selected: nothing written, whatever the amounts are
    if invert:
        text = np.frombuffer(b"the\n" * 40000, dtype=np.uint8)              # every line matches in all six models
        quiet, hay = make(ss, b"the"), dev_of(text)
    else:
        quiet, hay = make(ss, b"no such phrase in the manual"), dev
    ws = [Window(4), Window(4), Window(4), KindWindow(4)]
    for amount in (0, 3, U64_MAX):
        assert quiet.find_lines_context_into(hay, ws[0].view, ws[1].view, ws[2].view, ws[3].view, 4, amount, amount, invert=invert, **kw) == (0, 0)
    for w in ws:
        w.check([], (how, invert, "empty selection"))


# ---- lines_around on hand-made number sets --------------------------------------------------------------------------------------
def _small_views(length):
    views = {"delimiters only": np.full(length, NL, dtype=np.uint8), "no delimiter": np.full(length, ord("a"), dtype=np.uint8)}
    mixed = np.full(length, ord("a"), dtype=np.uint8)
    mixed[1::3] = NL
    mixed[-1] = ord("z")
    views["unterminated last line"] = mixed
    closed = mixed.copy()
    closed[-1] = NL
    views["closed last line"] = closed
    return views


@pytest.mark.parametrize("length", [1, 2, 15, 16, 17])
def test_lines_around_on_small_views(ss, length):
    for name, host in _small_views(length).items():
        dev = dev_of(host)
        n = every_line(host, NL)[2].size
        sets = [[1], [n], [1, n], [0, 1], [n, n + 1], [0, n + 1], [0], [n + 1, n + 2], list(range(1, n + 1)), [n // 2 + 1, n // 2 + 2],
                [max(1, n - 1)], [2, n]]
        for numbers in sets:
            numbers = sorted(set(numbers))                      # (strictly ascending: n = 1 folds some of them)
            for before, after in ((0, 0), (1, 0), (0, 1), (2, 2), (U64_MAX, 0), (0, U64_MAX), (U64_MAX, U64_MAX), (n, n)):
                check_around(ss, dev, host, numbers, before, after, (name, length))


def test_groups_that_touch_and_groups_that_do_not(ss):
    host = np.frombuffer(b"".join(b"line %d\n" % k for k in range(1, 41)), dtype=np.uint8)
    dev = dev_of(host)
    before, after = 2, 1
    for gap, seps in ((after + before, 0), (after + before + 1, 0), (after + before + 2, 1), (1, 0), (2, 0)):
        want = check_around(ss, dev, host, [10, 10 + gap], before, after, ("gap", gap))
        assert separators(want[2]) == seps and int(want[3].sum()) == 2, gap
    check_around(ss, dev, host, [1, 2, 3, 39, 40], 5, 5, "adjacent matches at both ends")
    check_around(ss, dev, host, [1, 40], 100, 100, "past both ends")
    check_around(ss, dev, host, [0, 7, 8, 41, 50, U64_MAX >> 1], 1, 1, "entries 0 and above N")
    # a breach of the contract: nothing faults, the total is the sum of the entries' ranges, nothing is written outside the capacity
    s = any_searcher(ss)
    ws = [Window(6), Window(6), Window(6), KindWindow(6)]
    total = s.lines_around_into(dev, [9, 3, 3, 30], ws[0].view, ws[1].view, ws[2].view, ws[3].view, 6, 1, 1)
    assert total == 4 * 3
    for w in ws:
        h = w.buf.cpu().numpy()
        assert (h[:GUARD] == (KIND_SENT if h.dtype == np.uint8 else SENT)).all() and (h[GUARD + 6:] == (KIND_SENT if h.dtype == np.uint8 else SENT)).all()


# ---- part borders ---------------------------------------------------------------------------------------------------------------
def _border_layouts(P, length):
    a = np.full(length, ord("x"), dtype=np.uint8)
    for at in (5, P - 1, P, length - 3):                        # the last byte of a part and the first byte of the next
        if 0 <= at < length:
            a[at] = NL
    out = {"delimiters on both sides of a border": a}
    if length > 2 * P:
        b = np.full(length, ord("y"), dtype=np.uint8)
        b[7] = NL                                               # line 2 begins in part 0 and ends in part 2; part 1 holds no delimiter
        b[2 * P] = NL
        if length > 3 * P + 3:
            b[3 * P + 3] = NL
        out["a line across three parts"] = b
    return out


def test_part_borders(ss):
    P = ss.CONTEXT_PART_BYTES
    for length in (P - 1, P, P + 1, 2 * P + 1, 3 * P + 17):
        for name, host in _border_layouts(P, length).items():
            dev = dev_of(host)
            n = every_line(host, NL)[2].size
            for numbers in ([1], [2], [n], [1, n], list(range(1, n + 1)), [2, n]):
                numbers = sorted(set(k for k in numbers if k >= 1))
                for before, after in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    check_around(ss, dev, host, numbers, before, after, (name, length))


def test_many_parts_with_wanted_lines_in_the_first_and_the_last_only(ss):
    P = ss.CONTEXT_PART_BYTES
    parts = 300
    host = np.full(parts * P - 11, ord("q"), dtype=np.uint8)
    rng = np.random.default_rng(7)
    host[rng.integers(0, host.size, 5000)] = NL
    host[[3, 40, 41]] = NL
    dev = dev_of(host)
    every = every_line(host, NL)
    n = every[2].size
    first = every[2][every[1] < P]                              # the lines that end in the first part ...
    last = every[2][every[0] >= (parts - 1) * P]                # ... and those that begin in the last
    assert first.size >= 3 and last.size >= 2 and n > first.size + last.size + 256
    numbers = [1, 3, int(first[-1]) - 1, int(last[1]), n]
    want = check_around(ss, dev, host, numbers, 1, 0, "300 parts")
    assert ((want[1] < P) | (want[0] >= (parts - 1) * P)).all()
    # the bytes of the parts between change nothing but the numbers
    quiet = host.copy()
    quiet[P:(parts - 1) * P] = ord("q")
    shift = n - every_line(quiet, NL)[2].size
    moved = [k if k <= first[-1] else k - shift for k in numbers]
    calm = check_around(ss, dev_of(quiet), quiet, moved, 1, 0, "300 quiet parts")
    assert (calm[0] == want[0]).all() and (calm[1] == want[1]).all() and (calm[3] == want[3]).all()


# ---- misaligned views -----------------------------------------------------------------------------------------------------------
def test_misaligned_views_with_delimiters_and_needles_just_outside(ss):
    P = ss.CONTEXT_PART_BYTES
    needle = b"needle"
    s = make(ss, needle)
    rng = np.random.default_rng(11)
    for size in (200, P + 300):
        text = rng.choice(np.frombuffer(b"abcd \n", dtype=np.uint8), size + 64, p=[0.2, 0.2, 0.2, 0.2, 0.15, 0.05]).astype(np.uint8)
        for at in range(40, size, 97):
            text[at:at + len(needle)] = np.frombuffer(needle, dtype=np.uint8)
        whole = dev_of(text)
        assert whole.data_ptr() % 16 == 0
        for mis in range(1, 16):
            lo, hi = 16 + mis, 16 + size + (mis * 7) % 16
            buf = text.copy()
            # a delimiter and a copy of the needle that ends / begins just outside both ends of the view
            buf[lo - 1] = NL
            buf[lo - 1 - len(needle):lo - 1] = np.frombuffer(needle, dtype=np.uint8)
            buf[hi] = NL
            buf[hi + 1:hi + 1 + len(needle)] = np.frombuffer(needle, dtype=np.uint8)
            whole.copy_(torch.from_numpy(buf))
            host, dev = buf[lo:hi], whole[lo:hi]
            assert dev.data_ptr() % 16 == mis
            chosen = matching_numbers(host, needle, NL, "")
            want = expected(host, NL, chosen, 1, 2)
            check_call(lambda b, e, n, k, cap: s.find_lines_context_into(dev, b, e, n, k, cap, 1, 2)[0], want, ("misaligned", size, mis))
            n = every_line(host, NL)[2].size
            check_around(ss, dev, host, [1, n // 2, n], 1, 1, ("misaligned", size, mis))
            check_around(ss, dev, host, [1, n], 0, 0, ("misaligned records", size, mis))


# ---- capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity_cuts_with_each_array_left_out(ss, manual):
    P = ss.CONTEXT_PART_BYTES
    host = manual[0][:2 * P + 77]
    dev = dev_of(host)
    s = make(ss, b"the")
    chosen = matching_numbers(host, b"the", NL, "")
    want = expected(host, NL, chosen, 1, 2)
    total = want[2].size
    # a cut inside a group that falls on a selected line: the last entry kept is of kind 1 and the next number follows it directly
    inside = [c for c in range(2, total) if want[3][c - 1] == 1 and want[2][c] == want[2][c - 1] + 1]
    assert inside and total > 8
    caps = [0, 1, inside[len(inside) // 2], total - 1, total, total + 1]
    skips = (None, 0, 1, 2, 3)
    check_call(lambda b, e, n, k, cap: s.find_lines_context_into(dev, b, e, n, k, cap, 1, 2)[0], want, "context capacity", caps, skips)
    check_around(ss, dev, host, chosen, 1, 2, "around capacity", caps=caps, skips=skips)
    assert s.find_lines_context_into(dev, None, None, None, None, 0, 1, 2) == (total, chosen.size)


# ---- delimiter values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delim", [0x00, ord("e"), ord("_")])
def test_delimiter_values(ss, delim):
    P = ss.CONTEXT_PART_BYTES
    rng = np.random.default_rng(delim + 1)
    host = rng.choice(np.frombuffer(b"\x00e_\nab", dtype=np.uint8), 2 * P + 5).astype(np.uint8)
    dev = dev_of(host)
    n = every_line(host, delim)[2].size
    numbers = np.unique(rng.integers(1, n + 1, 300)).tolist()
    check_around(ss, dev, host, numbers, 1, 2, ("delimiter", delim), delim=delim)
    check_around(ss, dev, host, [1, n], 3, 3, ("delimiter", delim), delim=delim, caps=[5])
    s = make(ss, b"ab")
    chosen = matching_numbers(host, b"ab", delim, "")
    want = expected(host, delim, chosen, 2, 1)
    check_call(lambda b, e, nn, k, cap: s.find_lines_context_into(dev, b, e, nn, k, cap, 2, 1, delim)[0], want, ("context delimiter", delim))
    got = s.find_lines_context(dev, 2, 1, bytes([delim]))
    assert [t.cpu().numpy().tolist() for t in got] == [w.tolist() for w in want]


# ---- offsets above 2^32 ---------------------------------------------------------------------------------------------------------
def test_offsets_above_4_gib(ss):
    P = ss.CONTEXT_PART_BYTES
    length = (4 << 30) + 3 * P
    dev = torch.zeros(length, dtype=torch.uint8, device="cuda")
    q0 = (4 << 30) + 2 * P + 100                                # line 1: 4 GiB of zeros; then `a needle`, an empty line, `tail` unterminated
    tail = b"\na needle\n\ntail"
    dev[q0:q0 + len(tail)] = torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda()
    dev[q0 + len(tail):] = ord("t")
    lines = [(0, q0), (q0 + 1, q0 + 9), (q0 + 10, q0 + 10), (q0 + 11, length)]
    s = any_searcher(ss)

    def want(numbers, kinds):
        return (np.array([lines[k - 1][0] for k in numbers], dtype=np.int64), np.array([lines[k - 1][1] for k in numbers], dtype=np.int64),
                np.array(numbers, dtype=np.int64), np.array(kinds, dtype=np.uint8))
    check_call(lambda b, e, n, k, cap: s.lines_around_into(dev, [2, 4], b, e, n, k, cap, 1, 0), want([1, 2, 3, 4], [0, 1, 0, 1]), "4 GiB around")
    check_call(lambda b, e, n, k, cap: s.lines_around_into(dev, [3], b, e, n, k, cap, 0, 0), want([3], [1]), "4 GiB one record")
    f = make(ss, b"needle")
    check_call(lambda b, e, n, k, cap: f.find_lines_context_into(dev, b, e, n, k, cap, 1, 1)[0], want([1, 2, 3], [0, 1, 0]), "4 GiB context")
    assert f.find_lines_context_into(dev, None, None, None, None, 0, 0, U64_MAX) == (3, 1)
    del dev
    torch.cuda.empty_cache()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ss):
    host = np.frombuffer(b"The cat\nthe dog\n\nother\n", dtype=np.uint8)
    dev = dev_of(host)
    ws = [Window(4), Window(4), Window(4), KindWindow(4)]
    views = [w.view for w in ws]
    cases = [(b"the", dict(whole_word=True, whole_line=True), NL, "both"), (b"", dict(whole_word=True), NL, "empty needle"),
             (b"", dict(whole_line=True, invert=True), NL, "empty needle"), (b"the", {}, 256, "0 .. 255"), (b"the", {}, -1, "0 .. 255"),
             (b"The", dict(ignore_case=True), NL, "upper-case"), (b"The", dict(ignore_case=True, invert=True, whole_word=True), NL, "upper-case")]
    for needle, kw, delim, word in cases:
        s = make(ss, needle)
        with pytest.raises(ss.SlicesliceError, match=word) as e:
            s.find_lines_context_into(dev, *views, 4, 1, 1, delim, **kw)
        assert e.value.code == ss.SS_ERR_ARGUMENT, (needle, kw)
    s = make(ss, b"the")
    for delim in (256, -1):
        with pytest.raises(ss.SlicesliceError, match="0 .. 255"):
            s.lines_around_into(dev, [1], *views, 4, 1, 1, delim)
    # unknown bits in `how`, through the C function: the totals stay what they were
    L = s._L
    for how in (16, 8 | 32, 1 << 31):
        total, selected = ctypes.c_uint64(777), ctypes.c_uint64(888)
        rc = L.ss_find_lines_context_device(s._h, dev.data_ptr(), dev.numel(), NL, how, 1, 1, torch.cuda.current_stream().cuda_stream,
                                            views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), views[3].data_ptr(), 4,
                                            ctypes.byref(total), ctypes.byref(selected))
        assert rc == ss.SS_ERR_ARGUMENT and b"SS_CONTEXT_INVERT" in L.ss_last_error() and (total.value, selected.value) == (777, 888), how
    for w in ws:
        w.check([], "refusals")
    # ... and the same arrays take an accepted call
    assert s.find_lines_context_into(dev, *views, 4, 0, 1) == (3, 2)             # `the dog` and `other` hold the needle
    ws[0].check([8, 16, 17], "accepted")
    ws[1].check([15, 16, 22], "accepted")
    ws[2].check([2, 3, 4], "accepted")
    ws[3].check([1, 0, 1], "accepted")


# ---- the command-line tool ------------------------------------------------------------------------------------------------------
def test_grep_hip_prints_what_grep_prints(kat):
    path = os.path.join(GOLDEN, "data", "i386.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py"), "-C", "2", "--lines", "descriptor", path], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    if shutil.which("grep"):
        ref = subprocess.run(["grep", "-a", "-F", "-n", "-C", "2", "descriptor", path], capture_output=True, env=dict(os.environ, LC_ALL="C"))
        assert ref.returncode == 0 and out == ref.stdout
    data = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    chosen = matching_numbers(data, b"descriptor", NL, "")
    numbers, kinds = context_rule(chosen, kat["lines"], 2, 2)
    rows = out.split(b"\n")[:-1]
    assert rows.count(b"--") == separators(numbers) and len(rows) == numbers.size + separators(numbers)
    assert sum(1 for l in rows if l != b"--" and l[len(str(int(l.split(b":")[0].split(b"-")[0]))):][:1] == b":") == chosen.size == 337
