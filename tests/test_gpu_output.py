"""GPU tests of the output calls (include/sliceslice_hip_output.h, libsliceslice_hip_output.so): ss_format_lines_device,
ss_gather_ranges_device and ss_grep_lines_device against the rule restated in Python (tests/golden/make_output_golden.format_rule)
on hand-made records aimed at the borders of SS_OUTPUT_CHUNK and SS_OUTPUT_BLOCK, and against tests/golden/output_kat.json (GNU
grep's stdout) on the manual's text.  Every comparison is of bytes or integers and exact; every output buffer is a window of a
larger one whose sentinels on both sides must survive.  The manual's text aside, no view is larger than 200,000 bytes and no list
longer than three blocks."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
from make_output_golden import format_rule      # noqa: E402  (the rule, restated there)

B = 4096                                # SS_OUTPUT_BLOCK
CH = 16384                              # SS_OUTPUT_CHUNK
GUARD = 64
SENT = 0xA5
SENT64 = -0x5A5A5A5A5A5A5A5B
MIS = (0, 1, 7, 15)
NL = 10
HOWS = {"": {}, "i": {"ignore_case": True}, "w": {"whole_word": True}, "wi": {"whole_word": True, "ignore_case": True},
        "x": {"whole_line": True}, "xi": {"whole_line": True, "ignore_case": True}}


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def out_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.output_build()`."""
    return _loaded() if getattr(ss.lib(), "has_output", False) else ss.output_build()


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    assert m.OUTPUT_BLOCK == B and m.OUTPUT_CHUNK == CH
    with out_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def manual():
    return open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()


@pytest.fixture(scope="module")
def d_manual(manual):
    return torch.from_numpy(np.frombuffer(manual, dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def text():
    """70,000 printable bytes without a period: a copy from the wrong offset shows"""
    rng = np.random.default_rng(20240517)
    return rng.integers(0x20, 0x7F, 70000, dtype=np.uint8).tobytes()


class Window:
    """`cap` slots inside a larger device array filled with a sentinel; `mis`: the 16-byte misalignment of the first slot"""
    def __init__(self, cap, dtype=torch.uint8, sent=SENT, mis=0):
        self.sent = sent
        self.buf = torch.full((cap + 2 * GUARD + 16,), sent, dtype=dtype, device="cuda")
        self.at = GUARD + ((mis - self.buf.data_ptr() - GUARD) % 16 if dtype == torch.uint8 else 0)
        self.view = self.buf[self.at:self.at + cap]
        assert dtype != torch.uint8 or self.view.data_ptr() % 16 == mis

    def check(self, want, what):
        """the first len(want) slots hold `want`, every other slot of the larger array the sentinel"""
        h = self.buf.cpu().numpy()
        want = np.frombuffer(want, dtype=np.uint8) if isinstance(want, (bytes, bytearray)) else np.asarray(want, dtype=h.dtype)
        k = len(want)
        assert (h[:self.at] == self.sent).all() and (h[self.at + k:] == self.sent).all(), what
        bad = np.flatnonzero(h[self.at:self.at + k] != want)
        assert bad.size == 0, (what, int(bad[0]), h[self.at + bad[0] - 8:self.at + bad[0] + 8].tolist(), want[max(bad[0] - 8, 0):bad[0] + 8].tolist())


def dev_view(host, mis=0, before=b"", after=b""):
    """the bytes of `host` on the device at 16-byte misalignment `mis`, with `before` and `after` just outside both ends"""
    host = np.frombuffer(bytes(host), dtype=np.uint8)
    buf = torch.full((host.size + 96,), ord("a"), dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + 32 + mis
    view = buf[at:at + host.size]
    if host.size:
        view.copy_(torch.from_numpy(host.copy()))
    if before:
        buf[at - len(before):at].copy_(torch.from_numpy(np.frombuffer(before, dtype=np.uint8).copy()))
    if after:
        buf[at + host.size:at + host.size + len(after)].copy_(torch.from_numpy(np.frombuffer(after, dtype=np.uint8).copy()))
    assert view.data_ptr() % 16 == mis
    return view


def dev64(values):
    """64-bit values (taken modulo 2^64) as an int64 device tensor holding the bit patterns"""
    return torch.from_numpy(np.asarray([int(v) & (2 ** 64 - 1) for v in values], dtype=np.uint64).view(np.int64).copy()).cuda()


def check_format(ss, data, view, begin, end, number=None, kind=None, terminator=NL, numbers=False, separators=False, out_mis=(0,), what=""):
    """the count-only call with d_starts, then the sized call into a window at every misalignment of `out_mis`"""
    want, starts = format_rule(data, begin, end, number, kind, terminator, numbers, separators)
    d_b, d_e = dev64(begin), dev64(end)
    d_n = dev64(number) if number is not None else None
    d_k = torch.tensor(list(kind), dtype=torch.uint8, device="cuda") if kind is not None else None
    kw = dict(number=d_n, kind=d_k, delimiter=None if terminator is None else bytes([terminator]), line_numbers=numbers, separators=separators)
    with out_lib(ss):
        ws = Window(len(begin) + 1, torch.int64, SENT64)
        assert ss.format_lines_into(view, d_b, d_e, None, d_starts=ws.view, **kw) == len(want), what
        ws.check(starts, (what, "starts"))
        assert starts[-1] == len(want)
        for m in out_mis:
            w = Window(len(want), mis=m)
            assert ss.format_lines_into(view, d_b, d_e, w.view, **kw) == len(want), (what, m)
            w.check(want, (what, m))
    return want


# ---- the copy pass ------------------------------------------------------------------------------------------------------------------
def border_cases(m):
    """(what, begin, end, number, numbers, separators) aimed at the chunk border at output offset P = CH - m, where m is d_out's
    misalignment: the chunks are cut from the 16-byte aligned address at or below d_out"""
    P = CH - m
    tail_b = [100 + 37 * k for k in range(300)]                       # 300 lines of 40 bytes behind: 2 to 3 chunks in all
    tail_e = [b + 40 for b in tail_b]
    cases = []
    for delta in (-1, 0, 1):                                          # the text ends one byte before, at and one byte after the border;
        cases.append(("text ends at border %+d" % delta, [3] + tail_b, [3 + P + delta] + tail_e, None, False, False))
    # (delta 0: the terminator is the first byte of a chunk)
    # `1:` + text + terminator = P - 3 bytes, then the digits of 1234567 lie on both sides of the border
    cases.append(("digits split", [5] + tail_b, [5 + P - 6] + tail_e, [1, 1234567] + list(range(1234568, 1234568 + 299)), True, False))
    for back in (1, 2):                                               # `--\n` begins 1 and 2 bytes in front of the border
        cases.append(("separator split %d" % back, [7] + tail_b, [7 + P - 3 - back] + tail_e, [1] + [5 + 2 * k for k in range(300)], True, True))
        cases.append(("separator split %d, no numbers" % back, [7] + tail_b, [7 + P - 1 - back] + tail_e, [1] + [5 + 2 * k for k in range(300)], False, True))
    ones = list(range(11, 16))
    cases.append(("3.5 chunks between one-byte records", ones + [20] + ones, [o + 1 for o in ones] + [20 + 7 * CH // 2] + [o + 1 for o in ones],
                  None, False, False))
    cases.append(("5,000 empty records", [9] * 5000, [9] * 5000, None, False, False))
    cases.append(("5,000 empty records with numbers", [9] * 5000, [4] * 5000, list(range(1, 5001)), True, False))
    return cases


@pytest.mark.parametrize("view_mis", MIS)
def test_copy_pass_borders(ss, text, view_mis):
    """records whose text, terminator, digits and separator meet the borders of SS_OUTPUT_CHUNK, one record of 3.5 chunks between
    one-byte records, and a chunk that holds more records than one LDS run - at every misalignment of the view and of d_out"""
    view = dev_view(text, view_mis)
    for m in MIS:
        for what, begin, end, number, numbers, separators in border_cases(m):
            want = check_format(ss, text, view, begin, end, number, None, NL, numbers, separators, out_mis=(m,), what=(what, view_mis, m))
            assert 5000 <= len(want) <= 4 * CH


def test_copy_pass_border_cases_meet_the_borders(text):
    """the cases above are what they say: the restated rule puts the bytes named at output offset CH - m"""
    for m in MIS:
        P = CH - m
        cases = {c[0]: c for c in border_cases(m)}
        for delta in (-1, 0, 1):
            _, b, e, n, nn, sp = cases["text ends at border %+d" % delta]
            out, starts = format_rule(text, b, e, n, None, NL, nn, sp)
            assert out[P + delta] == NL and starts[1] == P + delta + 1
        _, b, e, n, nn, sp = cases["digits split"]
        out, starts = format_rule(text, b, e, n, None, NL, nn, sp)
        assert out[P - 3:P + 5] == b"1234567:" and starts[1] == P - 3
        for back in (1, 2):
            for name in ("separator split %d" % back, "separator split %d, no numbers" % back):
                _, b, e, n, nn, sp = cases[name]
                out, starts = format_rule(text, b, e, n, None, NL, nn, sp)
                assert out[P - back:P - back + 3] == b"--\n" and starts[1] == P - back, name


# ---- the size passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, B - 1, B, B + 1, 2 * B + 1])
def test_size_pass_borders(ss, text, count):
    """d_starts against numpy.cumsum, d_starts[count] == out_len, and the output, around the borders of SS_OUTPUT_BLOCK"""
    rng = np.random.default_rng(count)
    lengths = rng.choice([0, 1, 15, 16, 17, 40], count)
    begin = rng.integers(0, len(text) - 40, count)
    number = np.cumsum(rng.integers(1, 3, count))
    kind = rng.integers(0, 2, count)
    view = dev_view(text, 3)
    for numbers, separators in ((False, False), (True, True)):
        want, starts = format_rule(text, begin, begin + lengths, number, kind, NL, numbers, separators)
        sizes = np.diff(np.asarray(starts))
        if not numbers:
            assert (sizes == lengths + 1).all()
        assert (np.concatenate([[0], np.cumsum(sizes)]) == np.asarray(starts)).all()
        check_format(ss, text, view, begin, begin + lengths, number, kind, NL, numbers, separators, out_mis=(5,), what=(count, numbers))


# ---- the digits -----------------------------------------------------------------------------------------------------------------------
def test_digits_kinds_and_separators(ss, text):
    """every digit count's ends as int64 bit patterns, kind 0 / 1 / NULL, separators at differences 1 and 2 and where numbers
    descend, repeat or stand at 2^64 - 1: the comparison is unsigned and does not wrap"""
    view = dev_view(text, 9)
    edge = [0, 9, 10, 99, 100, 2 ** 32 - 1, 2 ** 32, 10 ** 19, 2 ** 64 - 1]
    orders = [edge, edge[::-1], [5, 6, 8, 7, 7, 9, 2 ** 64 - 1, 0, 2, 2 ** 64 - 2, 2 ** 64 - 1, 1],
              [10 ** k - 1 for k in range(1, 20)] + [10 ** k for k in range(20)] + [10 ** k + 1 for k in range(20)]]
    for number in orders:
        begin = [13 * k for k in range(len(number))]
        end = [b + 5 + k % 3 for k, b in enumerate(begin)]
        for kind in ([0] * len(number), [1] * len(number), [k % 2 for k in range(len(number))], None):
            for separators in (False, True):
                want = check_format(ss, text, view, begin, end, number, kind, NL, True, separators, out_mis=(0, 3), what=(number[:3], kind, separators))
                assert want.startswith(b"%d" % number[0] + (b"-" if kind is not None and not kind[0] else b":"))
    out, _ = format_rule(text, [0, 0, 0, 0], [1, 1, 1, 1], [1, 2, 4, 3], None, NL, True, True)
    assert out.count(b"--\n") == 1                                              # (difference 1: none; 2: one; descending: none)
    out, _ = format_rule(text, [0, 0], [1, 1], [2 ** 64 - 1, 5], None, NL, True, True)
    assert b"--" not in out


# ---- capacity, clamping, free-form lists ------------------------------------------------------------------------------------------------
def test_a_short_capacity_writes_nothing(ss, text):
    view = dev_view(text, 1)
    begin, end, number = [0, 50, 20000], [40, 90, 60000], [1, 2, 9]
    want, starts = format_rule(text, begin, end, number, None, NL, True, True)
    assert len(want) > 2 * CH
    d = [dev64(x) for x in (begin, end, number)]
    with out_lib(ss):
        for m in MIS:
            w, ws = Window(len(want) - 1, mis=m), Window(4, torch.int64, SENT64)
            assert ss.format_lines_into(view, d[0], d[1], w.view, number=d[2], separators=True, d_starts=ws.view) == len(want)
            w.check(b"", ("short", m))
            ws.check(starts, "starts of the short call")
            w = Window(len(want), mis=m)
            assert ss.format_lines_into(view, d[0], d[1], w.view, number=d[2], separators=True) == len(want)
            w.check(want, ("exact", m))
            w = Window(len(want) + 100, mis=m)
            assert ss.format_lines_into(view, d[0], d[1], w.view, number=d[2], separators=True) == len(want)
            w.check(want, ("roomy", m))


def test_records_are_clamped_to_the_view(ss):
    """end > len, begin > len and begin > end: nothing outside the view is copied, whatever stands there"""
    rng = np.random.default_rng(7)
    data = rng.integers(0x30, 0x7B, 50000, dtype=np.uint8).tobytes()
    n = len(data)
    begin = [n - 20, n + 5, 300, 2 ** 63, n - 1, n, 0, 2 ** 64 - 1, 49990, 100]
    end = [n + 1000, n + 50, 200, 2 ** 64 - 1, 2 ** 64 - 1, n, 2 ** 64 - 1, 0, 50010, 20100]
    for mis in MIS:
        view = dev_view(data, mis, before=b"\x01" * 32, after=b"\x02" * 32)
        for terminator in (NL, None):
            want = check_format(ss, data, view, begin, end, None, None, terminator, out_mis=(0, 11), what=("clamp", mis, terminator))
            assert 1 not in want and 2 not in want and len(want) > n + 20000
    assert format_rule(data, [n - 20, 300, n + 5], [n + 1000, 200, n + 50], terminator=None)[0] == data[n - 20:]


def test_free_form_lists(ss, text):
    """overlapping, repeated and descending ranges through ss_gather_ranges_device, with its starts cut back into the ranges"""
    rng = np.random.default_rng(11)
    begin = [1000, 1000, 990, 5, 40000, 1000, 0, 69990] + [int(v) for v in rng.integers(0, 60000, 300)][::-1]
    end = [1100, 1100, 1050, 5, 69000, 1001, 70000, 70000] + [b + int(k) for b, k in zip(begin[8:], rng.integers(0, 200, 300))]
    view = dev_view(text, 7)
    with out_lib(ss):
        for terminator, tail in ((None, b""), (b"\x00", b"\x00"), (b"\n", b"\n")):
            want, starts = format_rule(text, begin, end, terminator=tail[0] if tail else None)
            out, got_starts = ss.gather_ranges(view, begin, end, terminator, return_starts=True)
            assert bytes(out.cpu().numpy()) == want and got_starts.cpu().tolist() == starts
            host = bytes(out.cpu().numpy())
            for i in (0, 1, 2, 3, 4, 6, 7, 100, 307):
                assert host[starts[i]:starts[i + 1]] == text[begin[i]:end[i]] + tail
            assert bytes(ss.gather_ranges(view, dev64(begin), dev64(end), terminator).cpu().numpy()) == want
        ws = Window(len(begin) + 1, torch.int64, SENT64)
        L, s = ss.lib(), ss.DynamicHipSearcher.new(b"")
        total = ctypes.c_uint64(0)
        d_b, d_e = dev64(begin), dev64(end)
        want, starts = format_rule(text, begin, end, terminator=NL)
        for m in MIS:
            w = Window(len(want), mis=m)
            rc = L.ss_gather_ranges_device(s._h, view.data_ptr(), view.numel(), d_b.data_ptr(), d_e.data_ptr(), len(begin), NL, 0, w.view.data_ptr(),
                                           len(want), ws.view.data_ptr(), ctypes.byref(total))
            assert rc == 0 and total.value == len(want)
            w.check(want, ("gather", m))
            ws.check(starts, "gather starts")


def test_no_records_and_an_empty_view(ss, text):
    view = dev_view(text, 2)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    with out_lib(ss):
        w, ws = Window(64), Window(1, torch.int64, SENT64)
        assert ss.format_lines_into(view, empty, empty, w.view, d_starts=ws.view) == 0
        w.check(b"", "no records")
        ws.check([0], "the one start of no records")
        assert ss.format_lines(view, [], []).numel() == 0 and ss.gather_ranges(view, [], []).numel() == 0
        out, starts = ss.gather_ranges(view, [], [], b"\n", return_starts=True)
        assert out.numel() == 0 and starts.cpu().tolist() == [0]
        nothing = view[:0]
        for hay in (nothing, (None, 0)):
            w, ws = Window(64), Window(4, torch.int64, SENT64)
            assert ss.format_lines_into(hay, [0, 5, 2], [9, 5, 1], w.view, number=[7, 8, 10], separators=True, d_starts=ws.view) == 13
            w.check(b"7:\n8:\n--\n10:\n", "an empty view")
            ws.check([0, 3, 6, 13], "an empty view's starts")
            assert ss.gather_ranges(hay, [0, 5], [9, 5]).numel() == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(ss, text):
    """every refusal of the header, each with its message and nothing written"""
    view = dev_view(text, 0)
    with out_lib(ss):
        L = ss.lib()
        s = ss.DynamicHipSearcher.new(b"the")
        d_b, d_e, d_n = dev64([0, 10]), dev64([5, 15]), dev64([1, 2])
        d_k = torch.ones(2, dtype=torch.uint8, device="cuda")
        w, ws = Window(64), Window(3, torch.int64, SENT64)
        total = ctypes.c_uint64(77)
        hay, n = view.data_ptr(), view.numel()

        def fmt(hay=hay, b=d_b.data_ptr(), e=d_e.data_ptr(), num=d_n.data_ptr(), kind=d_k.data_ptr(), count=2, term=NL, flags=3, stream=0,
                out=w.view.data_ptr(), cap=64, out_len=ctypes.byref(total)):
            return L.ss_format_lines_device(s._h, hay, n, b, e, num, kind, count, term, flags, stream, out, cap, ws.view.data_ptr(), out_len)

        def gather(b=d_b.data_ptr(), e=d_e.data_ptr(), count=2, term=NL, stream=0, out=w.view.data_ptr(), cap=64, out_len=ctypes.byref(total)):
            return L.ss_gather_ranges_device(s._h, hay, n, b, e, count, term, stream, out, cap, ws.view.data_ptr(), out_len)

        refused = [(dict(flags=4), "bits other than"), (dict(flags=7), "bits other than"), (dict(term=256), "terminator"), (dict(term=-2), "terminator"),
                   (dict(num=None, flags=1), "d_number is NULL"), (dict(num=None, flags=2), "d_number is NULL"), (dict(b=None), "d_begin or d_end is NULL"),
                   (dict(e=None), "d_begin or d_end is NULL"), (dict(out_len=None), "NULL argument"), (dict(count=2 ** 48), "fewer than 2^48"),
                   (dict(out=hay + 100, cap=64), "intersects the haystack"), (dict(out=hay - 32, cap=64), "intersects the haystack"),
                   (dict(out=hay + n - 1, cap=64), "intersects the haystack")]
        for kw, word in refused:
            rc = fmt(**kw)
            assert rc == ss.SS_ERR_ARGUMENT and word in L.ss_last_error().decode(), (kw, L.ss_last_error())
        for kw, word in ((dict(term=300), "terminator"), (dict(b=None), "d_begin or d_end is NULL"), (dict(out_len=None), "NULL argument"),
                         (dict(count=2 ** 48 + 5), "fewer than 2^48"), (dict(out=hay + 5), "intersects the haystack")):
            rc = gather(**kw)
            msg = L.ss_last_error().decode()
            assert rc == ss.SS_ERR_ARGUMENT and word in msg and (word == "NULL argument" or "ss_gather_ranges_device" in msg), (kw, msg)
        rc = L.ss_format_lines_device(None, hay, n, d_b.data_ptr(), d_e.data_ptr(), None, None, 2, NL, 0, 0, w.view.data_ptr(), 64, None, ctypes.byref(total))
        assert rc == ss.SS_ERR_ARGUMENT
        # the grep call: its own flags and range, and the context call's refusals passed through
        lines, selected = ctypes.c_uint64(77), ctypes.c_uint64(77)

        def grep(how=0, flags=3, out=w.view.data_ptr(), cap=64, stream=0, delimiter=NL, out_len=ctypes.byref(total)):
            return L.ss_grep_lines_device(s._h, hay, n, delimiter, how, 1, 1, flags, stream, out, cap, out_len, ctypes.byref(lines), ctypes.byref(selected))

        for kw, word in ((dict(flags=8), "bits other than SS_OUTPUT_NUMBER"), (dict(how=16), "bits other than SS_BOUND_WORD"), (dict(out_len=None), "NULL argument"),
                         (dict(out=hay + 3), "intersects the haystack"), (dict(delimiter=256), "delimiter")):
            rc = grep(**kw)
            assert rc == ss.SS_ERR_ARGUMENT and word in L.ss_last_error().decode(), (kw, L.ss_last_error())
        w.check(b"", "refusals")
        ws.check([], "refusals")
        assert total.value == 77 and lines.value == 77 and selected.value == 77
        assert fmt(cap=64, flags=0) == 0 and total.value == 12                   # (first use outside the capture)
        w.check(text[0:5] + b"\n" + text[10:15] + b"\n", "the one call that is not refused")
        w, ws = Window(64), Window(3, torch.int64, SENT64)
        total.value = 77
        probe = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            probe.fill_(7)                                                          # (something to capture: the refused calls add nothing)
            capturing = torch.cuda.current_stream().cuda_stream
            rcs = [fmt(stream=capturing), gather(stream=capturing)]
            msgs = [L.ss_last_error().decode()]
            rcs.append(grep(stream=capturing))
            msgs.append(L.ss_last_error().decode())
        assert rcs == [ss.SS_ERR_ARGUMENT] * 3 and all("cannot be captured" in m for m in msgs), (rcs, msgs)
        w.check(b"", "refusals")
        ws.check([], "refusals")
        assert total.value == 77 and lines.value == 77 and selected.value == 77
        for call in (lambda: ss.format_lines(view, [0], [1], separators=True), lambda: ss.format_lines(view, [0, 1], [1], number=[1, 2]),
                     lambda: ss.format_lines(view, [0], [1], delimiter=b"ab")):
            with pytest.raises((ss.SlicesliceError, ValueError)):
                call()


# ---- the manual's text --------------------------------------------------------------------------------------------------------------
def holds(row, got):
    return len(got) == row["length"] and hashlib.sha256(got).hexdigest() == row["sha256"] and got[:200].decode("latin-1") == row["first"] and \
        got[-200:].decode("latin-1") == row["last"]


def searcher(ss, needle, how):
    return ss.DynamicHipSearcher.new_nocase(needle.lower()) if how.endswith("i") else ss.DynamicHipSearcher.new(needle)


def test_grep_on_the_manual_is_gnu_greps_stdout(ss, manual, d_manual):
    """grep() for every row of tests/golden/output_kat.json; format_lines over find_lines_context's records equal to grep()"""
    kat = json.load(open(os.path.join(GOLDEN, "output_kat.json")))
    assert kat["grep_checked"] and len(kat["rows"]) == 15
    assert [r["length"] for r in kat["rows"] if (r["needle"], r["before"], r["after"]) == ("descriptor", 1, 2)] == [56185]
    with out_lib(ss):
        for row in kat["rows"]:
            s = searcher(ss, row["needle"].encode(), row["how"])
            kw = dict(HOWS[row["how"]], invert=row["invert"], before=row["before"], after=row["after"])
            got = s.grep(d_manual, line_numbers=row["line_numbers"], **kw)
            assert holds(row, bytes(got.cpu().numpy())), row["needle"]
            begin, end, number, kind = s.find_lines_context(d_manual, **kw)
            composed = ss.format_lines(d_manual, begin, end, number, kind, line_numbers=row["line_numbers"], separators=bool(row["before"] or row["after"]))
            assert torch.equal(composed, got), row["needle"]
        every = [r for r in kat["rows"] if r["needle"] == ""][0]
        assert every["length"] == len(manual) + sum(len(b"%d:" % k) for k in range(1, kat["lines"] + 1))
        # a capacity that is too short still reports the three counts
        L, s = ss.lib(), ss.DynamicHipSearcher.new(b"descriptor")
        out_len, lines, selected = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        w = Window(56184, mis=3)
        rc = L.ss_grep_lines_device(s._h, d_manual.data_ptr(), d_manual.numel(), NL, 0, 1, 2, 3, 0, w.view.data_ptr(), 56184, ctypes.byref(out_len),
                                    ctypes.byref(lines), ctypes.byref(selected))
        assert rc == 0 and out_len.value == 56185 and lines.value > selected.value > 0
        w.check(b"", "a short grep call")
        w = Window(56185, mis=3)
        rc = L.ss_grep_lines_device(s._h, d_manual.data_ptr(), d_manual.numel(), NL, 0, 1, 2, 3, 0, w.view.data_ptr(), 56185, ctypes.byref(out_len),
                                    ctypes.byref(lines), ctypes.byref(selected))
        assert rc == 0 and out_len.value == 56185
        assert holds(kat["rows"][0], bytes(w.view.cpu().numpy()))
        w.check(bytes(w.view.cpu().numpy()), "an exact grep call")


def test_grep_anyof_and_the_needle_set_on_the_manual(ss, manual, d_manual):
    """ss.grep_anyof for needle sets of tests/golden/anyof_kat.json: its records are the fixture's (GNU grep's), its bytes the rule's
    over those records; NeedleSet.grep equal to it byte for byte"""
    kat = json.load(open(os.path.join(GOLDEN, "anyof_kat.json")))
    rows = [dict(r, before=0, after=0) for r in kat["rows"][:6]] + kat["context_rows"]
    with out_lib(ss):
        for row in rows:
            needles = [nd.encode() for nd in row["needles"]]
            searchers = [searcher(ss, nd, row["how"]) for nd in needles]
            kw = dict({k: v for k, v in HOWS[row["how"]].items() if k != "ignore_case"}, invert=row["invert"], before=row["before"], after=row["after"])
            nocase = row["how"].endswith("i")
            begin, end, number, kind = [x.cpu().tolist() for x in ss.find_lines_anyof(searchers, d_manual, ignore_case=nocase, **kw)]
            pairs = "".join("%d:%d\n" % p for p in zip(number, kind)) if "printed" in row else "".join("%d\n" % k for k in number)
            assert sum(kind) == row["selected"] and len(number) == row.get("printed", row["selected"])
            if "printed" in row:
                assert hashlib.sha256(pairs.encode()).hexdigest() == row["sha256"]
            for line_numbers in (True, False):
                want = format_rule(manual, begin, end, number, kind, NL, line_numbers, bool(row["before"] or row["after"]))[0]
                got = ss.grep_anyof(searchers, d_manual, line_numbers=line_numbers, ignore_case=nocase, **kw)
                assert bytes(got.cpu().numpy()) == want, row["needles"]
                by_set = ss.NeedleSet(needles, ignore_case=nocase).grep(d_manual, line_numbers=line_numbers, **kw)
                assert torch.equal(by_set, got), row["needles"]


def test_grep_hip_device_output_is_the_output_without_the_flag(ss):
    """tools/grep_hip.py --device-output prints what GNU grep printed into the fixture, and - several patterns in one pass, inverted,
    with context - byte for byte what the tool prints without the flag"""
    import subprocess
    kat = json.load(open(os.path.join(GOLDEN, "output_kat.json")))
    path = os.path.join(GOLDEN, "data", "i386.txt")

    def grep(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True, timeout=600)

    row = kat["rows"][0]                                        # (three processes in all: each one loads torch and opens the GPU)
    got = grep("--device-output", "--lines", "-B", str(row["before"]), "-A", str(row["after"]), row["needle"], path)
    assert got.returncode == 0 and holds(row, got.stdout), got.stderr[-500:]
    args = ("--one-pass", "--lines", "-i", "-v", "-C", "1", "-e", "the", "-e", "descriptor", "-e", "a", path)
    plain, device = grep(*args), grep("--device-output", *args)
    assert plain.returncode == 0 and device.returncode == 0 and plain.stdout == device.stdout and len(plain.stdout) > 1000, device.stderr[-500:]


def test_gather_ranges_cut_back_into_lines(ss, manual, d_manual):
    """the gather of every 7th line with its starts, cut back at the starts, is the host's slices"""
    with out_lib(ss):
        begin, end, number = ss.DynamicHipSearcher.new(b"").find_lines(d_manual)
        begin, end = begin[::7].contiguous(), end[::7].contiguous()
        out, starts = ss.gather_ranges(d_manual, begin, end, b"\n", return_starts=True)
        host, st, b, e = bytes(out.cpu().numpy()), starts.cpu().tolist(), begin.cpu().tolist(), end.cpu().tolist()
        assert st[-1] == len(host) and len(st) == len(b) + 1
        assert all(host[st[i]:st[i + 1]] == manual[b[i]:e[i]] + b"\n" for i in range(len(b)))
