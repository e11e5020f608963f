"""GPU tests of the needle-set calls (include/sliceslice_hip_needleset.h, libsliceslice_hip_needleset.so): ss_count_lines_set_device and
ss_find_lines_set_device against ss_count_lines_anyof_device / ss_find_lines_anyof_device of the SAME build with searchers of the same
needles - value for value and array for array - against tests/golden/anyof_kat.json (GNU grep's output), and, where needles are
planted, against the rule restated on Python bytes.  Every comparison is of integers and exact; every output array is a window of a
larger one whose sentinels on both sides must survive."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_context_cpu import U64_MAX, checksum, separators
from test_gpu_bounded import GOLDEN, Window, dev_of
from test_gpu_context import KindWindow, check_call
from test_gpu_inverted import HOWS, every_line, matching_numbers
from test_gpu_matches import _loaded

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 10
PART = 128 * 1024                       # bytes of the view per workgroup of the set scan, from the aligned address below the view
NAMES = ("ss_needle_set_new", "ss_needle_set_free", "ss_needle_set_info", "ss_count_lines_set_device", "ss_find_lines_set_device")


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with set_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "anyof_kat.json")))


@pytest.fixture(scope="module")
def manual():
    data = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    return data, torch.from_numpy(data.copy()).cuda(), every_line(data, NL)


def set_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the set entry points, else `ss.needleset_build()`."""
    return _loaded() if getattr(ss.lib(), "has_needleset", False) else ss.needleset_build()


def pair(ss, needles, how=""):
    """(the set, one searcher per needle) of the same build; the searchers' needles are folded here, the set folds its own"""
    nocase = how.endswith("i")
    with set_lib(ss):
        searchers = [ss.DynamicHipSearcher.new_nocase(nd.lower()) if nocase else ss.DynamicHipSearcher(nd) for nd in needles]
        return ss.NeedleSet(needles, ignore_case=nocase), searchers


def flags(how, invert):
    kw = dict(HOWS[how], invert=invert)
    nocase = kw.pop("ignore_case", False)
    return kw, dict(kw, ignore_case=nocase)


def same(ss, needles, dev, how="", invert=False, contexts=((0, 0),), delim=NL, caps=None, skips=(None,), what=None, made=None):
    """the set's calls return what the anyof calls return; returns the anyof arrays of the last context"""
    st, searchers = made or pair(ss, needles, how)
    kw, akw = flags(how, invert)
    what = (what, how, invert)
    count = ss.count_lines_anyof(searchers, dev, bytes([delim]), **akw)
    assert st.count_lines(dev, bytes([delim]), **kw) == count, (what, "count")
    model = None
    for before, after in contexts:
        totals = ss.find_lines_anyof_into(searchers, dev, None, None, None, None, 0, before, after, delim, **akw)
        assert totals[1] == count and st.find_lines_into(dev, None, None, None, None, 0, before, after, delim, **kw) == totals, (what, before, after)
        model = [t.cpu().numpy() for t in ss.find_lines_anyof(searchers, dev, before, after, delim, **akw)]
        assert model[2].size == totals[0]
        check_call(lambda b, e, n, k, cap: st.find_lines_into(dev, b, e, n, k, cap, before, after, delim, **kw)[0], model,
                   (what, before, after), caps, skips)
    return model


def lines_with_any(host, needles, delim=NL):
    """the rule on Python bytes, for plain `how`: the numbers of the lines that hold a needle"""
    lines = bytes(host).split(bytes([delim]))
    if lines and lines[-1] == b"":
        lines.pop()
    return [k + 1 for k, l in enumerate(lines) if any(nd in l for nd in needles)]


# ---- the two texts of tests/test_gpu_anyof.py, rebuilt here ---------------------------------------------------------------------------
def three_letter_lines():
    """132 KiB of two-byte lines over {a, b, c}: 67,584 lines - more than 65,536, more than two 64 KiB parts, more than one workgroup"""
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


def test_only_the_needleset_library_has_the_entry_points(ss):
    for build in (ss.lines_build, ss.context_build, ss.anyof_build):
        with build() as L:
            assert not any(hasattr(L, n) for n in NAMES) and not L.has_needleset, build
            with pytest.raises(ss.SlicesliceError, match="needleset_build") as e:
                ss.NeedleSet([b"abc"])
            assert e.value.code == ss.SS_ERR_ARGUMENT
    assert not any(hasattr(ss.lib(), n) for n in NAMES)
    hay = b"one\ntwo\nthree\n"
    with set_lib(ss):
        L = ss.lib()
        assert all(hasattr(L, n) for n in NAMES) and L.has_needleset and L.has_anyof and L.has_context
        st = ss.NeedleSet([b"tw", b"r", b"tw", b"thr"])
    assert st.info() == dict(needles=4, distinct=3, blob_bytes=3, one_byte=1, two_byte=1, prefix_keys=1, largest_bucket=1, fold=0)
    assert st.count_lines(hay) == 2 and st.count_lines(hay, invert=True) == 1
    b, e, n, k = st.find_lines(hay)
    assert (b.tolist(), e.tolist(), n.tolist(), k.tolist()) == ([4, 8], [7, 13], [2, 3], [1, 1])
    assert n.dtype == torch.int64 and k.dtype == torch.uint8
    b, e, n, k = st.find_lines(hay, before=1, invert=True)
    assert (b.tolist(), e.tolist(), n.tolist(), k.tolist()) == ([0], [3], [1], [1])
    assert st.find_lines_into(hay, None, None, None, None, 0, after=1) == (2, 2)
    with set_lib(ss):
        folded = ss.NeedleSet([b"TW", b"One"], ignore_case=True)
    assert folded.info()["fold"] == 1 and folded.count_lines(b"ONE\ntwo\nthree\n") == 2
    st.close()
    st.close()


# ---- the texts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("how", list(HOWS))
@pytest.mark.parametrize("name", ["lines", "words"])
def test_set_calls_against_the_anyof_calls(ss, name, how, invert):
    contexts = ((0, 0), (1, 2), (U64_MAX, 0))
    for mis in (0, 1, 15):
        host, dev, needles = misaligned(name, mis)
        if name == "lines":
            assert every_line(host, NL)[2].size > 65536 and host.size > PART
        same(ss, needles, dev, how, invert, contexts, what=(name, mis))
    # a delimiter that is a letter (and a byte of some needles)
    host, dev, needles = misaligned(name, 1)
    same(ss, needles, dev, how, invert, ((1, 2), (0, 0)), delim=ord("b"), what=(name, "delimiter b"))
    if how == "" and not invert:
        st, _ = pair(ss, needles)
        assert st.find_lines(dev, delimiter=b"b")[2].tolist() == lines_with_any(host, needles, ord("b"))


# ---- every verification path at every border ------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 4, 5, 6, 7, 17, 2000]


def length_needles():
    """one needle per length, each with a first byte of its own"""
    return [(bytes([ord("A") + k]) + b"0123456789" * 200)[:n] for k, n in enumerate(LENGTHS)]


def dotted(size):
    """`size` bytes of dots in lines of 64"""
    host = np.full(size, ord("."), dtype=np.uint8)
    host[63::64] = NL
    return host


@pytest.mark.parametrize("mis", [0, 5])
def test_needles_of_every_length_across_lane_piece_wave_and_workgroup_borders(ss, mis):
    needles = length_needles()
    made = pair(ss, needles)
    size = 200 * 1024
    for k, nd in enumerate(needles):
        # stream position = hay index + mis: a lane border at a multiple of 16, a piece border of 1 KiB inside a wave's 4 KiB, a wave
        # border (the byte behind a wave's last one comes from memory) and the workgroup border
        borders = (16 * (300 + 7 * k), 1024 * (41 + 4 * k), 4096 * (20 + k), PART)
        for across in (len(nd) // 2, 1):                        # the border in the middle of the needle; behind its first byte
            if len(nd) == 1:
                across = across % 2                             # (one byte: the first behind the border; the last in front of it)
            buf = np.full(size + 64, ord("."), dtype=np.uint8)
            host = buf[32 + mis:32 + mis + size]
            host[:] = dotted(size)
            for border in borders:
                at = border - mis - across
                host[at:at + len(nd)] = np.frombuffer(nd, dtype=np.uint8)
            whole = dev_of(buf)
            dev = whole[32 + mis:32 + mis + size]
            assert dev.data_ptr() % 16 == mis
            want = lines_with_any(host, needles)
            assert len(want) == len(borders), (k, want)
            same(ss, needles, dev, "", False, ((0, 0), (0, 1)), what=("length", len(nd), mis, across), made=made)
            st = made[0]
            assert st.find_lines(dev)[2].tolist() == want, (len(nd), mis, across)
            assert st.count_lines(dev, invert=True) == every_line(host, NL)[2].size - len(want)
        same(ss, needles, dev, "", True, ((0, 0),), what=("length, inverted", len(nd), mis), made=made)


def test_a_needle_that_ends_at_len_and_one_that_starts_a_byte_too_late(ss):
    needles = length_needles()[:8]
    made = pair(ss, needles)
    for nd in needles:
        host = np.concatenate([dotted(5000 + len(nd)), np.frombuffer(nd, dtype=np.uint8)])
        whole = dev_of(np.concatenate([host, np.frombuffer(b"0123456789" * 3, dtype=np.uint8)]))     # (the needles' tails lie behind the view)
        for cut in (0, 1):
            dev = whole[:host.size - cut]
            want = lines_with_any(host[:host.size - cut], needles)
            assert len(want) == 1 - cut                         # (the needles begin with bytes of their own: no shorter one fits)
            same(ss, needles, dev, "", False, what=("at len", len(nd), cut), made=made)
            assert made[0].find_lines(dev)[2].tolist() == want, (len(nd), cut)
    # a two-byte needle cut to one byte is no one-byte needle's match
    st, _ = pair(ss, [b"B0", b"zzz"])
    dev = dev_of(np.frombuffer(b"..\n.B0", dtype=np.uint8))
    assert st.count_lines(dev) == 1 and st.count_lines(dev[:5]) == 0 and st.count_lines(dev[:5], invert=True) == 2


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_long_line_whose_only_match_lies_in_one_workgroup(ss, where):
    size = 200 * 1024
    needles = [b"needle", b"pin", b"xy", b"#"]
    made = pair(ss, needles)
    for nd in needles:
        host = np.full(size, ord("."), dtype=np.uint8)
        at = dict(first=5, middle=PART - 2, last=size - len(nd))[where]
        host[at:at + len(nd)] = np.frombuffer(nd, dtype=np.uint8)
        dev = dev_of(host)
        model = same(ss, needles, dev, "", False, what=(where, nd), made=made)
        assert [m.tolist() for m in model] == [[0], [size], [1], [1]]
        same(ss, needles, dev, "", True, what=(where, nd, "inverted"), made=made)
        assert made[0].count_lines(dev, invert=True) == 0


def test_the_last_needle_of_a_bucket_of_300(ss):
    needles = sorted({b"zz%03d%s" % (k * 3, b"q" * (k % 5)) for k in range(300)})
    assert len(needles) == 300
    st, searchers = pair(ss, needles)
    info = st.info()
    assert info["largest_bucket"] == 300 and info["prefix_keys"] == 1 and info["distinct"] == 300
    host = dotted(9000)
    last = needles[-1]
    host[4100:4100 + len(last)] = np.frombuffer(last, dtype=np.uint8)
    host[130:135] = np.frombuffer(b"zz000"[:4] + b".", dtype=np.uint8)           # (four bytes of the first one: no match)
    dev = dev_of(host)
    same(ss, needles, dev, "", False, ((0, 0), (1, 1)), made=(st, searchers))
    assert st.find_lines(dev)[2].tolist() == lines_with_any(host, needles) == [4100 // 64 + 1]


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("how", list(HOWS))
def test_long_needles_that_hold_a_letter_delimiter(ss, how, invert):
    """needles of 3 to 19 bytes with the delimiter letter, in either case, at index 2, 5, 6, 7, 10 or 16 - in front of, inside and behind
    the masked compare of bytes 2 .. 5 - on lines that are those needles as they are, with the other case and in one case throughout:
    folded, a needle that holds the delimiter matches nothing, and unfolded the other case is no delimiter"""
    needles = [b"q" * k + c + b"zz" for k in (2, 5, 6, 7, 10, 16) for c in (b"a", b"A")] + [b"qqqqqqqzz"]
    lines = []
    for nd in needles:
        lines += [nd, nd.swapcase(), nd.lower(), nd.upper(), b"-" + nd + b" " + nd.swapcase() + b"_"]
    host = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    dev = dev_of(host)
    made = pair(ss, needles, how)
    for delim in (ord("a"), ord("A"), NL):
        model = same(ss, needles, dev, how, invert, ((0, 0), (1, 1)), delim=delim, what=("letter delimiter", delim), made=made)
        union = np.zeros(0, dtype=np.int64)
        for nd in needles:
            union = np.union1d(union, matching_numbers(host, nd, delim, how))
        want = np.setdiff1d(every_line(host, delim)[2], union) if invert else union
        kw, _ = flags(how, invert)
        assert made[0].find_lines(dev, delimiter=bytes([delim]), **kw)[2].tolist() == want.tolist(), (how, invert, delim)
        assert int(model[3].sum()) == want.size


def test_a_and_ab_as_whole_words(ss):
    host = np.frombuffer(b"xab cab\nab\nabc\na b\nb a\n.ab.\nba\n", dtype=np.uint8)
    dev = dev_of(host)
    needles = [b"a", b"ab"]
    model = same(ss, needles, dev, "w", False, ((0, 0), (1, 0)))
    st, _ = pair(ss, needles, "w")
    assert st.find_lines(dev, whole_word=True)[2].tolist() == [2, 4, 5, 6]       # line 2 and 6: only `ab` passes the bound
    same(ss, needles, dev, "w", True)
    same(ss, needles, dev, "x", False)
    assert st.find_lines(dev, whole_line=True)[2].tolist() == [2]
    assert model[2].size == 6


# ---- capacities, order, the empty needle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
def test_capacity_cuts_with_each_array_left_out(ss, invert):
    host, dev, needles = misaligned("words", 1)
    made = pair(ss, needles)
    for context in ((0, 0), (1, 2)):
        kw, akw = flags("", invert)
        total = ss.find_lines_anyof_into(made[1], dev, None, None, None, None, 0, *context, **akw)[0]
        assert total > 8
        same(ss, needles, dev, "", invert, (context,), caps=[0, 1, total // 2, total - 1, total, total + 1], skips=(None, 0, 1, 2, 3), made=made)


@pytest.mark.parametrize("how", list(HOWS))
def test_order_duplicates_and_the_empty_needle(ss, how):
    host, dev, needles = misaligned("words", 15)
    needles = [nd for nd in needles if nd]
    kw, akw = flags(how, False)
    base = same(ss, needles, dev, how, False, ((2, 0),))
    for other in (needles[::-1], needles + needles[:2], [needles[1]] * 3 + needles, [nd.upper() for nd in needles] if how.endswith("i") else needles):
        st, _ = pair(ss, other, how)
        again = [t.cpu().numpy() for t in st.find_lines(dev, 2, 0, **kw)]
        assert all(a.size == b.size and (a == b).all() for a, b in zip(base, again)), how
        assert st.count_lines(dev, **kw) == int(base[3].sum())
    n_lines = every_line(host, NL)[2].size
    with_empty = needles + [b""]
    if how[:1] in ("w", "x"):
        st, _ = pair(ss, with_empty, how)
        with pytest.raises(ss.SlicesliceError, match="empty needle") as e:
            st.count_lines(dev, **kw)
        assert e.value.code == ss.SS_ERR_ARGUMENT
        return
    for context in ((0, 0), (3, 3)):
        same(ss, with_empty, dev, how, False, (context,), what="with the empty needle")
        same(ss, with_empty, dev, how, True, (context,), what="with the empty needle, inverted")
    st, _ = pair(ss, with_empty, how)
    kw.pop("invert")
    assert st.count_lines(dev, **kw) == n_lines and st.count_lines(dev, invert=True, **kw) == 0
    assert st.find_lines_into(dev, None, None, None, None, 0, 3, 3, invert=True, **kw) == (0, 0)
    assert st.count_lines(dev[:0], **kw) == 0 and st.find_lines_into(dev[:0], None, None, None, None, 0, **kw) == (0, 0)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def test_every_golden_row(ss, kat, manual):
    host, dev, every = manual
    assert every[2].size == kat["lines"] and len(kat["rows"]) == 40 and len(kat["context_rows"]) >= 4
    for r in kat["rows"]:
        what = (r["needles"], r["how"], r["invert"])
        st, _ = pair(ss, [n.encode() for n in r["needles"]], r["how"])
        kw, _ = flags(r["how"], r["invert"])
        assert st.count_lines(dev, **kw) == r["selected"], what
        begin, end, number, kind = [t.cpu().numpy() for t in st.find_lines(dev, **kw)]
        assert number.size == r["selected"] and (kind == 1).all(), what
        assert number[:20].tolist() == r["first"] and number[-20:].tolist() == r["last"], what
        assert hashlib.sha256("".join("%d\n" % n for n in number.tolist()).encode()).hexdigest() == r["sha256"], what
        assert (begin == every[0][number - 1]).all() and (end == every[1][number - 1]).all(), what
    for r in kat["context_rows"]:
        what = (r["needles"], r["how"], r["invert"], r["before"], r["after"])
        st, _ = pair(ss, [n.encode() for n in r["needles"]], r["how"])
        kw, _ = flags(r["how"], r["invert"])
        assert st.find_lines_into(dev, None, None, None, None, 0, r["before"], r["after"], **kw) == (r["printed"], r["selected"]), what
        begin, end, number, kind = [t.cpu().numpy() for t in st.find_lines(dev, r["before"], r["after"], **kw)]
        assert number.size == r["printed"] and int(kind.sum()) == r["selected"] and separators(number) == r["separators"], what
        pairs = [list(p) for p in zip(number.tolist(), kind.tolist())]
        assert pairs[:20] == r["first"] and pairs[-20:] == r["last"] and checksum(number, kind) == r["sha256"], what
        assert (begin == every[0][number - 1]).all() and (end == every[1][number - 1]).all(), what


def test_the_word_list_as_a_pattern_file(ss, kat, manual):
    r = kat["words_row"]
    words = [w for w in open(os.path.join(GOLDEN, r["file"]), "rb").read().split(b"\n") if w]
    assert len(words) == r["needles"] == 4585
    with set_lib(ss):
        st = ss.NeedleSet(words)
    info = st.info()
    assert info["needles"] == 4585 and info["one_byte"] == 44 and info["two_byte"] == 240 and info["distinct"] <= 4585
    assert st.count_lines(manual[1]) == r["selected"] == 14555
    number = st.find_lines(manual[1])[2].cpu().numpy()
    assert number.size == 14555 and (np.diff(number) > 0).all()
    assert st.count_lines(manual[1], invert=True) == kat["lines"] - 14555


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ss):
    host = np.frombuffer(b"The cat\nthe dog\n\nother\n", dtype=np.uint8)
    dev = dev_of(host)
    ws = [Window(4), Window(4), Window(4), KindWindow(4)]
    views = [w.view for w in ws]
    with set_lib(ss):
        L = ss.lib()
        st, folded, empty = ss.NeedleSet([b"the"]), ss.NeedleSet([b"The"], ignore_case=True), ss.NeedleSet([b"the", b""])
    stream = torch.cuda.current_stream().cuda_stream

    def c_find(h, how=0, st_=stream, delim=NL, lines=True, selected=True):
        total, chosen = ctypes.c_uint64(777), ctypes.c_uint64(888)
        rc = L.ss_find_lines_set_device(h, dev.data_ptr(), dev.numel(), delim, how, 1, 1, st_, views[0].data_ptr(), views[1].data_ptr(),
                                        views[2].data_ptr(), views[3].data_ptr(), 4, ctypes.byref(total) if lines else None,
                                        ctypes.byref(chosen) if selected else None)
        assert (total.value, chosen.value) == (777, 888) or rc == ss.SS_OK
        return rc, L.ss_last_error()

    def c_count(h, how=0, st_=stream, delim=NL, lines=True, selected=True):
        total = ctypes.c_uint64(777)
        rc = L.ss_count_lines_set_device(h, dev.data_ptr(), dev.numel(), delim, how, st_, ctypes.byref(total) if lines else None)
        assert total.value == 777 or rc == ss.SS_OK
        return rc, L.ss_last_error()
    for fn in (c_find, c_count):
        assert fn(None)[0] == ss.SS_ERR_ARGUMENT and fn(st._h, lines=False)[0] == ss.SS_ERR_ARGUMENT
        for how in (16, 8 | 32, 1 << 31):
            rc, msg = fn(st._h, how)
            assert rc == ss.SS_ERR_ARGUMENT and b"SS_CONTEXT_INVERT" in msg, how
        rc, msg = fn(st._h, ss.searcher.SS_BOUND_NOCASE)
        assert rc == ss.SS_ERR_ARGUMENT and b"SS_SET_NOCASE" in msg
        rc, msg = fn(folded._h, 0)
        assert rc == ss.SS_ERR_ARGUMENT and b"SS_SET_NOCASE" in msg
        rc, msg = fn(st._h, 1 | 2)
        assert rc == ss.SS_ERR_ARGUMENT and b"exclude" in msg
        for how in (1, 2, 2 | 8):
            rc, msg = fn(empty._h, how)
            assert rc == ss.SS_ERR_ARGUMENT and b"empty needle" in msg
        for delim in (256, -1):
            rc, msg = fn(st._h, 0, stream, delim)
            assert rc == ss.SS_ERR_ARGUMENT and b"0 .. 255" in msg
    assert c_find(st._h, selected=False)[0] == ss.SS_ERR_ARGUMENT
    # construction
    h = ctypes.c_void_p(5)
    one = (ctypes.c_void_p * 1)(ctypes.cast(ctypes.c_char_p(b"abc"), ctypes.c_void_p))
    lens = (ctypes.c_size_t * 1)(3)
    holed, holed_lens = (ctypes.c_void_p * 2)(one[0], None), (ctypes.c_size_t * 2)(3, 2)
    many = (ctypes.c_void_p * (ss.ANYOF_MAX_NEEDLES + 1))(*([one[0]] * (ss.ANYOF_MAX_NEEDLES + 1)))
    many_lens = (ctypes.c_size_t * (ss.ANYOF_MAX_NEEDLES + 1))(*([3] * (ss.ANYOF_MAX_NEEDLES + 1)))
    huge = (ctypes.c_size_t * 1)(1 << 32)
    for args, word in (((one, lens, 0, 0), b"no needles"), ((None, lens, 1, 0), b"NULL"), ((one, None, 1, 0), b"NULL"),
                       ((holed, holed_lens, 2, 0), b"needles[1] is NULL"), ((many, many_lens, ss.ANYOF_MAX_NEEDLES + 1, 0), b"65537 needles"),
                       ((one, lens, 1, 2), b"SS_SET_NOCASE"), ((one, huge, 1, 0), b"2^32")):
        assert L.ss_needle_set_new(*args, ctypes.byref(h)) == ss.SS_ERR_ARGUMENT and word in L.ss_last_error(), word
        assert h.value == 5
    assert L.ss_needle_set_new(one, lens, 1, 0, None) == ss.SS_ERR_ARGUMENT
    assert L.ss_needle_set_info(None, (ctypes.c_uint64 * 8)()) == ss.SS_ERR_ARGUMENT and L.ss_needle_set_info(st._h, None) == ss.SS_ERR_ARGUMENT
    L.ss_needle_set_free(None)
    # a capturing stream: refused before any launch
    assert st.count_lines(dev) == 2                                             # (first use outside the capture; `other` holds `the`)
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.graph(graph):
        probe.fill_(7)                                                          # (something to capture: the refused calls add nothing)
        capturing = torch.cuda.current_stream().cuda_stream
        refused.append(c_find(st._h, 0, capturing))
        refused.append(c_count(st._h, 0, capturing))
    for rc, msg in refused:
        assert rc == ss.SS_ERR_ARGUMENT and b"cannot be captured" in msg, msg
    for w in ws:
        w.check([], "refusals")
    # ... and the same arrays take accepted calls
    with set_lib(ss):
        two = ss.NeedleSet([b"the", b"other"])
    assert two.find_lines_into(dev, *views, 4, 0, 1) == (3, 2)
    ws[0].check([8, 16, 17], "accepted")
    ws[1].check([15, 16, 22], "accepted")
    ws[2].check([2, 3, 4], "accepted")
    ws[3].check([1, 0, 1], "accepted")


# ---- the command-line tool ------------------------------------------------------------------------------------------------------------
def test_grep_hip_one_pass_prints_what_the_fixture_records(kat, tmp_path):
    path = os.path.join(GOLDEN, "data", "i386.txt")
    tool = [sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")]
    row = [r for r in kat["context_rows"] if r["needles"] == ["the", "descriptor"] and r["how"] == "w" and r["before"] == r["after"] == 1][0]
    args = ["--lines", "-C", "1", "-w", "-e", "the", "-e", "descriptor", path]
    r = subprocess.run(tool + ["--one-pass"] + args, capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = r.stdout.split(b"\n")[:-1]
    pairs = []
    for l in rows:
        if l != b"--":
            digits = len(l) - len(l.lstrip(b"0123456789"))
            pairs.append((int(l[:digits]), 1 if l[digits:digits + 1] == b":" else 0))
    assert rows.count(b"--") == row["separators"] and len(pairs) == row["printed"] and sum(k for _, k in pairs) == row["selected"]
    assert checksum(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])) == row["sha256"]
    old = subprocess.run(tool + args, capture_output=True)
    assert old.returncode == 0 and old.stdout == r.stdout                       # byte for byte the same either way
    patterns = tmp_path / "patterns"
    patterns.write_bytes(b"the\ndescriptor\nintel\n")
    row = [r for r in kat["rows"] if r["needles"] == ["the", "descriptor", "intel"] and r["how"] == "" and r["invert"]][0]
    r = subprocess.run(tool + ["--one-pass", "-v", "--count-lines", "-f", str(patterns), path], capture_output=True)
    assert r.returncode == 0 and int(r.stdout) == row["selected"] == 15892, r.stderr[-2000:]
    row = [r for r in kat["rows"] if r["needles"] == ["the", "descriptor", "intel"] and r["how"] == "wi" and not r["invert"]][0]
    r = subprocess.run(tool + ["--one-pass", "-i", "-w", "--count-lines", "-f", str(patterns), path], capture_output=True)
    assert r.returncode == 0 and int(r.stdout) == row["selected"] == 5115, r.stderr[-2000:]
