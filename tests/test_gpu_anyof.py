"""GPU tests of the several-needle calls (include/sliceslice_hip_anyof.h, libsliceslice_hip_anyof.so): ss_union_numbers_device against
np.union1d / np.setdiff1d, ss_count_lines_anyof_device and ss_find_lines_anyof_device against the rule restated on numpy arrays (the
union of tests/test_gpu_inverted.py's matching_numbers over the needles, or its complement, then tests/test_context_cpu.py's
context_rule), against tests/golden/anyof_kat.json (GNU grep's output) and against the library's own single-needle calls.  Every
comparison is of integers and exact; every output array is a window of a larger one whose sentinels on both sides must survive."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_context_cpu import U64_MAX, checksum, separators
from test_gpu_bounded import GOLDEN, GUARD, SENT, Window, dev_of
from test_gpu_context import KindWindow, check_call, expected
from test_gpu_inverted import HOWS, every_line, matching_numbers
from test_gpu_matches import _loaded

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 10
SEG = 65536
BORDERS = [1, 31, 32, 33, 64, 65, 65535, 65536, 65537, 131072, 131073]
NAMES = ("ss_union_numbers_device", "ss_count_lines_anyof_device", "ss_find_lines_anyof_device")


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with anyof_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "anyof_kat.json")))


@pytest.fixture(scope="module")
def manual():
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    return data, torch.from_numpy(data.copy()).cuda(), every_line(data, NL)


def anyof_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the anyof entry points, else `ss.anyof_build()`."""
    return _loaded() if getattr(ss.lib(), "has_anyof", False) else ss.anyof_build()


def make(ss, needle, nocase=False):
    with anyof_lib(ss):
        return ss.DynamicHipSearcher.new_nocase(needle) if nocase else ss.DynamicHipSearcher(needle)


def makes(ss, needles, how=""):
    """one searcher per needle (the tests' needles hold no upper-case byte unless they are folded here)"""
    return [make(ss, nd.lower() if how.endswith("i") else nd, how.endswith("i")) for nd in needles]


def selected_rule(host, needles, delim, how, invert):
    """the numbers the rule selects: the union of the single-needle rules, or its complement among all lines"""
    union = np.zeros(0, dtype=np.int64)
    for nd in needles:
        union = np.union1d(union, matching_numbers(host, nd, delim, how))
    return np.setdiff1d(every_line(host, delim)[2], union) if invert else union


# ---- the primitive --------------------------------------------------------------------------------------------------------------
def union_rule(lists, limit, complement):
    flat = np.concatenate([np.asarray(l, dtype=np.uint64).reshape(-1) for l in lists]) if lists else np.zeros(0, dtype=np.uint64)
    valid = np.unique(flat[(flat >= 1) & (flat <= limit)]).astype(np.int64)
    return np.setdiff1d(np.arange(1, limit + 1, dtype=np.int64), valid) if complement else valid


def check_union(ss, lists, limit, what, complements=(False, True), caps=None):
    """count only (capacity 0, and no array), then every capacity: the leftmost min(total, capacity) numbers, sentinels elsewhere"""
    with anyof_lib(ss):
        dev = [ss.searcher._device_numbers(l, torch.device("cuda", 0)) for l in lists]
        for complement in complements:
            want = union_rule(lists, limit, complement)
            total = want.size
            assert ss.union_numbers_into(dev, limit, None, 0, complement) == total, (what, complement, "capacity 0")
            assert ss.union_numbers_into(dev, limit, None, total + 3, complement) == total, (what, complement, "no array")
            for cap in ([total] if caps is None else caps(total)):
                w = Window(cap)
                assert ss.union_numbers_into(dev, limit, w.view if cap else None, cap, complement) == total, (what, complement, cap)
                w.check(want[:min(total, cap)], (what, complement, "capacity", cap))


def five_caps(total):
    return sorted({0, 1, max(total - 1, 0), total, total + 1})


def test_only_the_anyof_library_has_the_entry_points(ss):
    for build in (ss.lines_build, ss.inverted_build, ss.context_build):
        with build() as L:
            assert not any(hasattr(L, n) for n in NAMES) and not L.has_anyof, build
            outsider = ss.DynamicHipSearcher(b"abc")
            with pytest.raises(ss.SlicesliceError, match="anyof_build"):
                ss.union_numbers([[1]], 3)
        for fn, args in ((ss.count_lines_anyof, ([outsider], b"abc\n")), (ss.find_lines_anyof, ([outsider], b"abc\n")),
                         (ss.find_lines_anyof_into, ([outsider], b"abc\n", None, None, None, None, 0))):
            with pytest.raises(ss.SlicesliceError, match="anyof_build") as e:
                fn(*args)
            assert e.value.code == ss.SS_ERR_ARGUMENT
    assert not any(hasattr(ss.lib(), n) for n in NAMES)
    hay = b"one\ntwo\nthree\n"
    with anyof_lib(ss):
        L = ss.lib()
        assert all(hasattr(L, n) for n in NAMES) and L.has_anyof and L.has_context and L.has_inverted
        pair = [ss.DynamicHipSearcher(b"tw"), ss.MemchrHipSearcher(ord("r"))]
        assert ss.union_numbers([[1, 3], [2, 3]], 3).tolist() == [1, 2, 3] and ss.union_numbers([[2]], 3, complement=True).tolist() == [1, 3]
        assert ss.union_numbers([], 2, complement=True).tolist() == [1, 2] and ss.union_numbers([[5, 9]], 9, capacity=1).tolist() == [5]
    with ss.context_build():
        stranger = ss.DynamicHipSearcher(b"one")
    with pytest.raises(ss.SlicesliceError, match="one library"):
        ss.count_lines_anyof([pair[0], stranger], hay)
    assert ss.count_lines_anyof(pair, hay) == 2 and ss.count_lines_anyof(pair, hay, invert=True) == 1
    b, e, n, k = ss.find_lines_anyof(pair, hay)
    assert (b.tolist(), e.tolist(), n.tolist(), k.tolist()) == ([4, 8], [7, 13], [2, 3], [1, 1])
    assert n.dtype == torch.int64 and k.dtype == torch.uint8
    b, e, n, k = ss.find_lines_anyof(pair[:1], hay, before=1, invert=True)
    assert (b.tolist(), e.tolist(), n.tolist(), k.tolist()) == ([0, 4, 8], [3, 7, 13], [1, 2, 3], [1, 0, 1])
    assert ss.find_lines_anyof_into(pair, hay, None, None, None, None, 0, after=1) == (2, 2)


def test_union_at_the_borders_of_words_and_segments(ss):
    limit = 200000
    for v in BORDERS:
        check_union(ss, [[v]], limit, ("alone", v))
    for v in (32, 64, 65536, 131072):                           # the last bit of a word (and of a segment) and the first of the next
        check_union(ss, [[v, v + 1]], limit, ("one list across", v), complements=(False,))
        check_union(ss, [[v], [v + 1]], limit, ("two lists across", v))
        check_union(ss, [[v + 1], [v]], limit, ("two lists across, the later first", v), complements=(False,))
    check_union(ss, [BORDERS, [], BORDERS[::2], BORDERS[1::2]], limit, "the borders in several lists")
    check_union(ss, [[7, 65536, 65537]] * 5, limit, "the same numbers in every list")
    check_union(ss, [[], [], [3, 70000], [], [4], []], limit, "empty lists first, last and between")
    check_union(ss, [[], []], 40, "only empty lists")
    check_union(ss, [], 40, "no list")
    check_union(ss, [[0, 1, 5, 41, 42, 1 << 40, U64_MAX]], 40, "0 and numbers above the limit")
    check_union(ss, [[0], [41]], 40, "nothing valid")


@pytest.mark.parametrize("lists", [1, 2, 65, 300])
def test_union_of_many_lists(ss, lists):
    rng = np.random.default_rng(lists)
    limit = 150000
    pool = np.unique(rng.integers(1, limit + 1, 4000))
    owner = rng.integers(0, lists, pool.size)
    cut = [pool[owner == k] for k in range(lists)]              # (single-element and empty lists among them, when there are 300)
    if lists > 2:
        cut[1] = pool[::7]                                      # a list that repeats the others' numbers
        cut[2] = pool[:1]
    check_union(ss, cut, limit, ("lists", lists), caps=five_caps)


@pytest.mark.parametrize("limit", [1, 32, 33, 65536, 65537, 200000])
def test_union_limits_with_complement(ss, limit):
    rng = np.random.default_rng(limit)
    some = np.unique(rng.integers(1, limit + 1, max(1, limit // 3)))
    check_union(ss, [some[::2], some[1::2], [limit, limit + 1]], limit, ("limit", limit), caps=five_caps)
    check_union(ss, [[limit]], limit, ("only the limit", limit))
    check_union(ss, [np.arange(1, limit + 1)], limit, ("every number", limit))


def test_union_of_full_segments_and_capacity_cuts(ss):
    limit = 200000                                              # three full segments and one part full
    every = np.arange(1, limit + 1, dtype=np.int64)
    dealt = [every[k::3] for k in range(3)]
    caps = lambda total: sorted({0, 1, total - 1, total, total + 1, SEG, 2 * SEG, SEG + 1000} & set(range(total + 2)))       # noqa: E731
    check_union(ss, dealt, limit, "every number dealt to three lists", complements=(False,), caps=caps)
    check_union(ss, dealt, limit, "every number dealt to three lists", complements=(True,))
    # a sparse set: the rank of segment 1 is the number of entries below 65,537 - one cut exactly there, one inside segment 1
    rng = np.random.default_rng(5)
    some = np.unique(rng.integers(1, limit + 1, 30000))
    rank = int((some <= SEG).sum())
    check_union(ss, [some[::2], some[1::2]], limit, "capacity at and inside a segment", caps=lambda total: [rank, rank + 100, rank - 1])
    inverse = limit - some.size
    check_union(ss, [some], limit, "capacity cuts of the complement", complements=(True,),
                caps=lambda total: [SEG - rank, SEG - rank + 1, inverse - 1, inverse, inverse + 1])


def test_union_of_lists_that_break_the_contract(ss):
    limit = 100000
    with anyof_lib(ss):
        for lists in ([[70000, 3]], [[9, 3, 3, 80000, 5], [65537, 65536]], [[5, 5, 5]]):
            for complement in (False, True):
                for cap in (0, 2, 6):
                    w = Window(cap)
                    total = ss.union_numbers_into(lists, limit, w.view if cap else None, cap, complement)
                    assert total <= limit, (lists, complement, total)
                    h = w.buf.cpu().numpy()
                    k = min(cap, total)
                    assert (h[:GUARD] == SENT).all() and (h[GUARD + k:] == SENT).all(), (lists, complement, cap)
                    assert ((h[GUARD:GUARD + k] >= 1) & (h[GUARD:GUARD + k] <= limit)).all(), (lists, complement, cap)


# ---- the line calls -------------------------------------------------------------------------------------------------------------
def three_letter_lines():
    """132 KiB of two-byte lines over {a, b, c}: 67,584 lines - more than one union segment, more than two census parts"""
    rng = np.random.default_rng(21)
    host = np.full(132 * 1024, NL, dtype=np.uint8)
    host[0::2] = rng.choice(np.frombuffer(b"abc", dtype=np.uint8), host.size // 2)
    return host, [b"a", b"b"]


def two_letter_words():
    rng = np.random.default_rng(22)
    tokens = [b"ab", b"ba", b"bb", b"aa", b"abba", b"a_b"]
    parts = []
    for t, sep in zip(rng.integers(0, len(tokens), 9000), rng.choice([b" ", b"\n", b"-"], 9000, p=[0.6, 0.3, 0.1])):
        parts += [tokens[t], sep]
    host = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return host, [b"abba", b"ab", b"bb a", b"aa", b"zz"]        # (a prefix of another, one that holds a blank, one that is absent)


_TEXTS = {}


def misaligned(name, mis):
    """(host view, device view, needles) of text `name` at 16-byte misalignment `mis`, with a delimiter and a copy of a needle just
    outside both ends of the view; made once and left unchanged"""
    if (name, mis) not in _TEXTS:
        text, needles = (three_letter_lines if name == "lines" else two_letter_words)()
        buf = np.full(text.size + 64, ord("q"), dtype=np.uint8)
        lo = 32 + mis
        hi = lo + text.size - (mis * 5) % 16
        buf[lo:hi] = text[:hi - lo]
        nd = np.frombuffer(needles[0], dtype=np.uint8)
        buf[lo - 1] = NL
        buf[lo - 1 - nd.size:lo - 1] = nd
        buf[hi] = NL
        buf[hi + 1:hi + 1 + nd.size] = nd
        whole = dev_of(buf)
        assert whole.data_ptr() % 16 == 0
        _TEXTS[(name, mis)] = (buf[lo:hi].copy(), whole[lo:hi], needles)
        assert _TEXTS[(name, mis)][1].data_ptr() % 16 == mis
    return _TEXTS[(name, mis)]


_RULES = {}


def rule_of(name, mis, delim, how, invert):
    key = (name, mis, delim, how, invert)
    if key not in _RULES:
        host, _, needles = misaligned(name, mis)
        _RULES[key] = selected_rule(host, needles, delim, how, invert)
    return _RULES[key]


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("how", list(HOWS))
@pytest.mark.parametrize("name", ["lines", "words"])
def test_line_calls_against_the_rule(ss, name, how, invert):
    for mis in (0, 1, 15):
        host, dev, needles = misaligned(name, mis)
        searchers = makes(ss, needles, how)
        kw = dict(HOWS[how], invert=invert)
        chosen = rule_of(name, mis, NL, how, invert)
        if name == "lines":
            assert every_line(host, NL)[2].size > SEG and host.size > 2 * ss.CONTEXT_PART_BYTES
        assert ss.count_lines_anyof(searchers, dev, **kw) == chosen.size, (name, how, invert, mis)
        for before, after in ((0, 0), (1, 2), (U64_MAX, 0)):
            want = expected(host, NL, chosen, before, after)
            what = (name, how, invert, mis, before, after)
            check_call(lambda b, e, n, k, cap: ss.find_lines_anyof_into(searchers, dev, b, e, n, k, cap, before, after, **kw)[0], want, what)
            assert ss.find_lines_anyof_into(searchers, dev, None, None, None, None, 0, before, after, **kw) == (want[2].size, chosen.size), what
    # a delimiter that is a letter (and a byte of some needles)
    host, dev, needles = misaligned(name, 1)
    delim = ord("b")
    usable = [nd for nd in needles if how[:1] not in ("w", "x") or nd]
    searchers = makes(ss, usable, how)
    chosen = selected_rule(host, usable, delim, how, invert)
    want = expected(host, delim, chosen, 1, 2)
    check_call(lambda b, e, n, k, cap: ss.find_lines_anyof_into(searchers, dev, b, e, n, k, cap, 1, 2, delim, **kw)[0], want,
               (name, how, invert, "delimiter b"))
    assert ss.count_lines_anyof(searchers, dev, bytes([delim]), **kw) == chosen.size


def test_capacity_cuts_with_each_array_left_out(ss):
    host, dev, needles = misaligned("words", 1)
    searchers = makes(ss, needles)
    want = expected(host, NL, rule_of("words", 1, NL, "", False), 1, 2)
    total = want[2].size
    assert total > 8
    check_call(lambda b, e, n, k, cap: ss.find_lines_anyof_into(searchers, dev, b, e, n, k, cap, 1, 2)[0], want, "capacity",
               [0, 1, total // 2, total - 1, total, total + 1], (None, 0, 1, 2, 3))


# ---- relations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", list(HOWS))
def test_relations(ss, how):
    host, dev, needles = misaligned("words", 15)
    needles = [nd for nd in needles if nd]
    kw = HOWS[how]
    searchers = makes(ss, needles, how)
    n_lines = make(ss, b"").count_lines(dev)
    assert n_lines == every_line(host, NL)[2].size
    assert ss.count_lines_anyof(searchers, dev, **kw) + ss.count_lines_anyof(searchers, dev, invert=True, **kw) == n_lines, how
    # one needle: the context call's arrays, array for array
    for invert in (False, True):
        for s in searchers[:2]:
            one = [t.cpu().numpy() for t in ss.find_lines_anyof([s], dev, 1, 2, invert=invert, **kw)]
            model = [t.cpu().numpy() for t in s.find_lines_context(dev, 1, 2, invert=invert, **kw)]
            assert all(a.size == b.size and (a == b).all() for a, b in zip(one, model)), (how, invert)
            assert ss.count_lines_anyof([s], dev, invert=invert, **kw) == (s.count_lines_inverted if invert else s.count_lines)(dev, **kw)
    # the order of the needles and a needle given twice change nothing
    base = [t.cpu().numpy() for t in ss.find_lines_anyof(searchers, dev, 2, 0, **kw)]
    for other in (searchers[::-1], searchers + searchers[:2], [searchers[1]] * 3 + searchers):
        again = [t.cpu().numpy() for t in ss.find_lines_anyof(other, dev, 2, 0, **kw)]
        assert all(a.size == b.size and (a == b).all() for a, b in zip(base, again)), how
        assert ss.count_lines_anyof(other, dev, **kw) == int(base[3].sum())
    if how[:1] not in ("w", "x"):                               # the empty needle selects every line
        with_empty = searchers + [make(ss, b"", how.endswith("i"))]
        assert ss.count_lines_anyof(with_empty, dev, **kw) == n_lines and ss.count_lines_anyof(with_empty, dev, invert=True, **kw) == 0
        assert ss.find_lines_anyof_into(with_empty, dev, None, None, None, None, 0, 3, 3, invert=True, **kw) == (0, 0)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_every_golden_row(ss, kat, manual):
    host, dev, every = manual
    assert every[2].size == kat["lines"] and len(kat["rows"]) == 40 and len(kat["context_rows"]) >= 4
    for r in kat["rows"]:
        what = (r["needles"], r["how"], r["invert"])
        searchers = makes(ss, [n.encode() for n in r["needles"]], r["how"])
        kw = dict(HOWS[r["how"]], invert=r["invert"])
        assert ss.count_lines_anyof(searchers, dev, **kw) == r["selected"], what
        begin, end, number, kind = [t.cpu().numpy() for t in ss.find_lines_anyof(searchers, dev, **kw)]
        assert number.size == r["selected"] and (kind == 1).all(), what
        assert number[:20].tolist() == r["first"] and number[-20:].tolist() == r["last"], what
        assert hashlib.sha256("".join("%d\n" % n for n in number.tolist()).encode()).hexdigest() == r["sha256"], what
        assert (begin == every[0][number - 1]).all() and (end == every[1][number - 1]).all(), what
    for r in kat["context_rows"]:
        what = (r["needles"], r["how"], r["invert"], r["before"], r["after"])
        searchers = makes(ss, [n.encode() for n in r["needles"]], r["how"])
        kw = dict(HOWS[r["how"]], invert=r["invert"])
        assert ss.find_lines_anyof_into(searchers, dev, None, None, None, None, 0, r["before"], r["after"], **kw) == (r["printed"], r["selected"]), what
        begin, end, number, kind = [t.cpu().numpy() for t in ss.find_lines_anyof(searchers, dev, r["before"], r["after"], **kw)]
        assert number.size == r["printed"] and int(kind.sum()) == r["selected"] and separators(number) == r["separators"], what
        pairs = [list(p) for p in zip(number.tolist(), kind.tolist())]
        assert pairs[:20] == r["first"] and pairs[-20:] == r["last"] and checksum(number, kind) == r["sha256"], what
        assert (begin == every[0][number - 1]).all() and (end == every[1][number - 1]).all(), what


def test_the_word_list_as_a_pattern_file(ss, kat, manual):
    r = kat["words_row"]
    words = [w for w in open(os.path.join(GOLDEN, r["file"]), "rb").read().split(b"\n") if w]
    assert len(words) == r["needles"] == 4585
    assert ss.count_lines_anyof(makes(ss, words), manual[1]) == r["selected"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ss):
    host = np.frombuffer(b"The cat\nthe dog\n\nother\n", dtype=np.uint8)
    dev = dev_of(host)
    ws = [Window(4), Window(4), Window(4), KindWindow(4)]
    views = [w.view for w in ws]
    s, upper, empty = make(ss, b"the"), make(ss, b"The"), make(ss, b"")
    L = s._L
    stream = torch.cuda.current_stream().cuda_stream

    def c_find(table, needles, how=0, st=stream):
        total, selected = ctypes.c_uint64(777), ctypes.c_uint64(888)
        rc = L.ss_find_lines_anyof_device(table, needles, dev.data_ptr(), dev.numel(), NL, how, 1, 1, st, views[0].data_ptr(),
                                          views[1].data_ptr(), views[2].data_ptr(), views[3].data_ptr(), 4, ctypes.byref(total), ctypes.byref(selected))
        assert (total.value, selected.value) == (777, 888) or rc == ss.SS_OK
        return rc, L.ss_last_error()

    def c_count(table, needles, how=0):
        lines = ctypes.c_uint64(777)
        rc = L.ss_count_lines_anyof_device(table, needles, dev.data_ptr(), dev.numel(), NL, how, stream, ctypes.byref(lines))
        assert lines.value == 777 or rc == ss.SS_OK
        return rc, L.ss_last_error()
    one = (ctypes.c_void_p * 1)(s._h)
    holed = (ctypes.c_void_p * 3)(s._h, None, s._h)
    many = (ctypes.c_void_p * (ss.ANYOF_MAX_NEEDLES + 1))(*([s._h] * (ss.ANYOF_MAX_NEEDLES + 1)))
    for fn in (c_find, c_count):
        rc, msg = fn(one, 0)
        assert rc == ss.SS_ERR_ARGUMENT and b"no needles" in msg
        rc, msg = fn(holed, 3)
        assert rc == ss.SS_ERR_ARGUMENT and b"searchers[1] is NULL" in msg
        rc, msg = fn(many, ss.ANYOF_MAX_NEEDLES + 1)
        assert rc == ss.SS_ERR_ARGUMENT and b"65537 needles" in msg
        assert fn(None, 1)[0] == ss.SS_ERR_ARGUMENT
        for how in (16, 8 | 32, 1 << 31):
            rc, msg = fn(one, 1, how)
            assert rc == ss.SS_ERR_ARGUMENT and b"SS_CONTEXT_INVERT" in msg, how
    # the models' refusals pass through, whichever needle meets them
    for searchers, kw, word in (([s, upper], dict(ignore_case=True), "upper-case"), ([s, empty], dict(whole_word=True), "empty needle"),
                                ([empty, s], dict(whole_line=True, invert=True), "empty needle"), ([s], dict(whole_word=True, whole_line=True), "both")):
        for call in (lambda: ss.find_lines_anyof_into(searchers, dev, *views, 4, 1, 1, **kw), lambda: ss.count_lines_anyof(searchers, dev, **kw)):
            with pytest.raises(ss.SlicesliceError, match=word) as e:
                call()
            assert e.value.code == ss.SS_ERR_ARGUMENT, (kw, word)
    for delim in (256, -1):
        with pytest.raises(ss.SlicesliceError, match="0 .. 255"):
            ss.find_lines_anyof_into([s], dev, *views, 4, 1, 1, delim)
    # a capturing stream: refused before any launch, by the line calls and by the primitive
    out = Window(4)
    numbers = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    offsets = (ctypes.c_uint64 * 2)(0, 2)
    assert ss.count_lines_anyof([s], dev) == 2                                  # (first use outside the capture)
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.graph(graph):
        probe.fill_(7)                                                          # (something to capture: the refused calls add nothing)
        capturing = torch.cuda.current_stream().cuda_stream
        refused.append(c_find(one, 1, 0, capturing))
        total = ctypes.c_uint64(777)
        rc = L.ss_union_numbers_device(s._h, numbers.data_ptr(), offsets, 1, 5, 0, capturing, out.view.data_ptr(), 4, ctypes.byref(total))
        refused.append((rc, L.ss_last_error()))
    assert total.value == 777
    for rc, msg in refused:
        assert rc == ss.SS_ERR_ARGUMENT and b"cannot be captured" in msg, msg
    # the primitive's own refusals
    total = ctypes.c_uint64(777)
    down = (ctypes.c_uint64 * 3)(0, 2, 1)
    assert L.ss_union_numbers_device(s._h, numbers.data_ptr(), down, 2, 5, 0, stream, out.view.data_ptr(), 4, ctypes.byref(total)) == ss.SS_ERR_ARGUMENT
    assert b"offsets[1]" in L.ss_last_error()
    assert L.ss_union_numbers_device(s._h, numbers.data_ptr(), offsets, ss.ANYOF_MAX_NEEDLES + 1, 5, 0, stream, out.view.data_ptr(), 4,
                                     ctypes.byref(total)) == ss.SS_ERR_ARGUMENT
    assert L.ss_union_numbers_device(s._h, numbers.data_ptr(), offsets, 1, (1 << 31) * SEG, 0, stream, out.view.data_ptr(), 4,
                                     ctypes.byref(total)) == ss.SS_ERR_ARGUMENT and b"2^31 - 1" in L.ss_last_error()
    assert total.value == 777
    out.check([], "refused unions")
    for w in ws:
        w.check([], "refusals")
    # ... and the same arrays take accepted calls
    assert L.ss_union_numbers_device(s._h, numbers.data_ptr(), offsets, 1, 0, 1, stream, out.view.data_ptr(), 4, ctypes.byref(total)) == ss.SS_OK
    assert total.value == 0                                                      # limit 0: nothing, with no launch
    out.check([], "limit 0")
    assert ss.find_lines_anyof_into([s, make(ss, b"other")], dev, *views, 4, 0, 1) == (3, 2)
    ws[0].check([8, 16, 17], "accepted")
    ws[1].check([15, 16, 22], "accepted")
    ws[2].check([2, 3, 4], "accepted")
    ws[3].check([1, 0, 1], "accepted")


# ---- the command-line tool ------------------------------------------------------------------------------------------------------
def test_grep_hip_prints_what_the_fixture_records(kat, tmp_path):
    path = os.path.join(GOLDEN, "data", "i386.txt")
    tool = [sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")]
    row = [r for r in kat["context_rows"] if r["needles"] == ["the", "descriptor"] and r["how"] == "w" and r["before"] == r["after"] == 1][0]
    r = subprocess.run(tool + ["--lines", "-C", "1", "-w", "-e", "the", "-e", "descriptor", path], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = r.stdout.split(b"\n")[:-1]
    pairs = []
    for l in rows:
        if l != b"--":
            digits = len(l) - len(l.lstrip(b"0123456789"))
            pairs.append((int(l[:digits]), 1 if l[digits:digits + 1] == b":" else 0))
    assert rows.count(b"--") == row["separators"] and len(pairs) == row["printed"] and sum(k for _, k in pairs) == row["selected"]
    assert checksum(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])) == row["sha256"]
    data = open(path, "rb").read().split(b"\n")
    assert all(l == b"--" or l.split(b":" if b":" in l[:7] else b"-", 1)[1] == data[int(l[:len(l) - len(l.lstrip(b"0123456789"))]) - 1] for l in rows[:50])
    patterns = tmp_path / "patterns"
    patterns.write_bytes(b"the\ndescriptor\nintel\n")
    row = [r for r in kat["rows"] if r["needles"] == ["the", "descriptor", "intel"] and r["how"] == "" and r["invert"]][0]
    r = subprocess.run(tool + ["-v", "--count-lines", "-f", str(patterns), path], capture_output=True)
    assert r.returncode == 0 and int(r.stdout) == row["selected"] == 15892, r.stderr[-2000:]
