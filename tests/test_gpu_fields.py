"""GPU tests of the field calls (include/sliceslice_hip_fields.h, libsliceslice_hip_fields.so) against THE RULE restated in numpy
(tests/test_fields_cpu.py: rule_fields), against calls of the same build that exist, and against tests/golden/fields_kat.json (plain
Python).  Every comparison is of integers and exact; every output array is a window of a larger one whose sentinels on both sides
must survive.  The geometry's units are lane 16 B, piece 1 KiB, wave 4 KiB, tile 16 KiB and workgroup 128 KiB; the carry kernel walks
the workgroups' summaries FIELDS_CARRY_CHUNK = 256 at a time."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_classes_cpu import re_set, sets_of                                           # noqa: E402
from test_fields_cpu import EACH, KEEP_SHORT, MERGE, cut_bytes, rule_fields, words_of  # noqa: E402
from test_gpu_masked import LANE, PIECE, TILE, WAVE, WG, Arena, Window                  # noqa: E402
from test_gpu_runs import haystack                                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VIEW = 2 * WG + 3 * LANE
BLANKS = b" \t"


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def mk_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.fields_build()`."""
    return _loaded() if getattr(ss.lib(), "has_fields", False) else ss.fields_build()


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with mk_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def manual():
    return open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()


@pytest.fixture(scope="module")
def d_manual(manual):
    return torch.from_numpy(np.frombuffer(manual, dtype=np.uint8).copy()).cuda()


def make(ss, sep, mode, first, last, flags=0):
    with mk_lib(ss):
        return ss.FieldSelector(sep, first, last, merge=mode == MERGE, keep_short=bool(flags & KEEP_SHORT))


def check(ss, dev, host, sep, mode, first, last, flags=0, delimiter=10, what=None):
    """count and find of one selector on one view, against the rule"""
    what = (what, mode, first, last, flags, delimiter)
    begin, end, number, lines = rule_fields(host, sep, mode, first, last, flags, delimiter)
    selected = begin.size if not flags & KEEP_SHORT else rule_fields(host, sep, mode, first, last, 0, delimiter)[0].size
    sel = make(ss, sep, mode, first, last, flags)
    d = bytes([delimiter])
    assert sel.count(dev, d) == (selected, lines), (what, "count")
    n = begin.size
    wb, we, wn = Window(n + 2), Window(n + 2), Window(n + 2)
    assert sel.find_into(dev, wb.view, we.view, wn.view, n + 2, d) == n, (what, "find total")
    wb.check(begin, (what, "begin"))
    we.check(end, (what, "end"))
    wn.check(number, (what, "number"))
    return begin, end, number


# ---- 1. unit borders -------------------------------------------------------------------------------------------------------------------
LINES = {EACH: b"aa,bb,CCC,DD,ee\n\n", MERGE: b"aa  bb  CCC  DD  ee\n\n"}
# what lies at the border: (offset, length) inside the line - the separator in front of field 3, field 3, the separator that ends
# field 4, the delimiter (two of them: an empty line behind)
PARTS = {EACH: ((5, 1), (6, 3), (12, 1), (15, 2)), MERGE: ((6, 2), (8, 3), (15, 2), (19, 2))}
BACKGROUND = {EACH: b"q,r,,s,t u,v,w x\n", MERGE: b"q r  s\tt u  v w x \n"}


def planted(unit, mode, mis):
    """host buffers of the arena's size: every part of LINES on the last byte before a border of `unit`, on the first byte after it and
    across it; borders are multiples of `unit` from the 16-byte aligned address the view's first byte lies `mis` behind"""
    size = VIEW + 16
    borders = [b for b in range(unit, mis + VIEW - 64, unit) if b > mis + 64]
    borders = [borders[(k * len(borders)) // 12] for k in range(12)] if len(borders) > 12 else borders
    plants = [(off, n, where) for off, n in PARTS[mode] for where in ("before", "after", "across")]
    buffers = []
    for k in range(0, len(plants), len(borders)):
        host = np.frombuffer((BACKGROUND[mode] * (size // len(BACKGROUND[mode]) + 1))[:size], dtype=np.uint8).copy()
        for (off, n, where), border in zip(plants[k:k + len(borders)], borders):
            start = border - {"before": off + n, "after": off, "across": off + (n + 1) // 2}[where]
            text = b"\n" + LINES[mode]
            host[start - 1:start - 1 + len(text)] = np.frombuffer(text, dtype=np.uint8)
        buffers.append(host)
    return buffers


@pytest.mark.parametrize("unit", [LANE, PIECE, WAVE, TILE, WG])
def test_the_parts_of_a_record_on_both_sides_of_and_across_every_unit_border(ss, unit):
    sep = {EACH: b",", MERGE: BLANKS}
    for mode in (EACH, MERGE):
        for mis in range(16):
            for host in planted(unit, mode, mis):
                arena = Arena(host)
                dev, view = arena.view(mis, VIEW)
                check(ss, dev, view, sep[mode], mode, 3, 4, 0, 10, (unit, mis))
        # ... and with the other selections on the aligned view
        for host in planted(unit, mode, 0):
            dev, view = Arena(host).view(0, VIEW)
            for first, last, flags in ((3, 3, 0), (3, 0, 0), (1, 4, 0), (3, 4, KEEP_SHORT), (5, 5, KEEP_SHORT)):
                check(ss, dev, view, sep[mode], mode, first, last, flags, 10, (unit, "aligned"))


# ---- 2. the carry through workgroups without delimiter --------------------------------------------------------------------------------
def test_a_line_of_three_workgroups_carries_its_count_to_the_delimiter(ss):
    size = 3 * WG + 5
    seps = (WG // 2, WG + WG // 2, 2 * WG + WG // 2, 3 * WG + 2)
    host = np.full(size + 1, ord("x"), dtype=np.uint8)
    host[size] = 10
    bare = host.copy()
    host[list(seps)] = ord(",")
    dev, view = Arena(host).view(0, size + 1)
    for mode in (EACH, MERGE):
        for first in (1, 2, 3, 4, 5):
            for last in (first, 0, first + 1):
                for flags in (0, KEEP_SHORT):
                    begin, end, _ = check(ss, dev, view, b",", mode, first, last, flags, 10, "one separator per workgroup")
                    assert begin.size == 1
                    if 2 <= first <= 4:                     # the begin and, where the field ends at a separator, the end lie in
                        assert begin[0] // WG == first - 2 and begin[0] // WG != size // WG             # workgroups without the delimiter
                    if last and last <= 3:
                        assert end[0] // WG == last - 1 and end[0] // WG != size // WG
        begin, _, _ = check(ss, dev, view, b",", mode, 6, 6, 0, 10, "one field short")
        assert begin.size == 0
    dev, view = Arena(bare).view(0, size + 1)
    for mode in (EACH, MERGE):
        for first, last, flags, records in ((1, 1, 0, 1), (1, 0, 0, 1), (2, 2, 0, 0), (2, 0, KEEP_SHORT, 1), (1, 2, KEEP_SHORT, 1)):
            begin, end, _ = check(ss, dev, view, b",", mode, first, last, flags, 10, "no separator at all")
            assert begin.size == records and (records == 0 or end[0] == size)
    # ... and the same line without its delimiter: the view's end closes it
    dev, view = Arena(host).view(0, size)
    for mode in (EACH, MERGE):
        for first, last, flags in ((1, 1, 0), (4, 0, 0), (5, 5, 0), (5, 6, 0), (6, 6, KEEP_SHORT), (2, 3, 0)):
            check(ss, dev, view, b",", mode, first, last, flags, 10, "closed by the view's end")


# ---- 3. the carry kernel's own chunk border -------------------------------------------------------------------------------------------
def test_a_line_that_opens_in_the_first_chunk_of_summaries_and_closes_in_the_second(ss):
    """C = 256 workgroup summaries per step of fields_carry_kernel: kFieldsCarryChunk in fields_launch.hpp, SS_FIELDS_CARRY_CHUNK in
    the header, ss.FIELDS_CARRY_CHUNK here.  The view is (C + 2) * 128 KiB of zeros (field bytes in both modes); a line opens in
    workgroup 3, field 3 begins in workgroup C - 1, the last of chunk 0, and the delimiter lies in workgroup C + 1."""
    C = ss.FIELDS_CARRY_CHUNK
    size = (C + 2) * WG
    if size > 1 << 30:
        pytest.skip("a view of C + 2 = %d workgroups exceeds 1 GiB" % (C + 2))
    dev = torch.zeros(size, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0
    plants = {3 * WG: 10, 100 * WG + 5: ord(","), (C - 1) * WG + 77: ord(","), (C + 1) * WG + 100: 10}
    for at, byte in plants.items():
        dev[at] = byte
    host = dev.cpu().numpy()
    for mode, first, last, flags in ((EACH, 3, 3, KEEP_SHORT), (MERGE, 3, 0, 0), (EACH, 2, 2, 0)):
        begin, end, number = check(ss, dev, host, b",", mode, first, last, flags, 10, "chunk border")
        k = 1 if flags else 0
        assert number[k] == 2 and begin[k] == ((C - 1) * WG + 78 if first == 3 else 100 * WG + 6)
        assert end[k] == ((C + 1) * WG + 100 if first == 3 else (C - 1) * WG + 77)
        assert begin[k] // WG // C == 0 and ((C + 1) * WG + 100) // WG // C == 1


# ---- 4. dense cases -------------------------------------------------------------------------------------------------------------------
def test_dense_delimiters_and_separators_at_a_workgroup_and_seventeen_bytes(ss):
    size = WG + 17
    rng = np.random.default_rng(51)
    hosts = {"delimiters": np.full(size, 10, dtype=np.uint8), "separators": np.full(size, ord(","), dtype=np.uint8),
             "alternating": np.tile(np.frombuffer(b",\n", dtype=np.uint8), size // 2 + 1)[:size].copy()}
    for p in (0.5, 0.05):
        u = rng.random(size)
        hosts["random %.2f" % p] = np.where(u < p, ord(","), np.where(u < 2 * p, 10, ord("x"))).astype(np.uint8)
    for name, host in hosts.items():
        dev, view = Arena(host).view(0, size)
        for mode in (EACH, MERGE):
            for first in (1, 2, 17):
                for last in (first, 0):
                    begin, _, _ = check(ss, dev, view, b",", mode, first, last, 0, 10, name)
                    if name == "separators":                # EACH: one line of size + 1 empty fields; MERGE: no field
                        assert begin.size == (1 if mode == EACH else 0)
            check(ss, dev, view, b",", mode, 2, 3, KEEP_SHORT, 10, name)
    dev, view = Arena(hosts["separators"]).view(0, size)
    begin, end, _ = check(ss, dev, view, b",", EACH, size + 1, size + 1, 0, 10, "the last of size + 1 empty fields")
    assert (begin[0], end[0]) == (size, size)
    check(ss, dev, view, b",", EACH, size + 2, 0, 0, 10, "one field more than there are")
    # ... and text-like random bytes under both paths of the membership test: one range, and a set of five
    for sep in (b" ", b" \t,;:"):
        host = haystack(words_of(sep + b"\n"), 0.2, size, rng)
        host[host == 10] = ord(" ")
        host[rng.random(size) < 0.02] = 10
        for mis in (0, 7):
            dev, view = Arena(host).view(mis, size - 16)
            for mode in (EACH, MERGE):
                for first, last in ((1, 1), (2, 2), (3, 0), (2, 5)):
                    check(ss, dev, view, sep, mode, first, last, 0, 10, (sep, mis))


# ---- 5. capacity and NULL arrays ------------------------------------------------------------------------------------------------------
def test_capacities_with_each_array_left_out_and_the_sizing_call(ss, manual):
    text = np.frombuffer(manual[:VIEW], dtype=np.uint8)
    dev, view = Arena(text).view(3, VIEW - 16)
    for mode, first, last, flags in ((EACH, 2, 2, 0), (MERGE, 2, 4, 0), (MERGE, 3, 0, KEEP_SHORT)):
        begin, end, number, _ = rule_fields(view, b" ", mode, first, last, flags)
        total = begin.size
        assert total > 1000
        sel = make(ss, b" ", mode, first, last, flags)
        assert sel.find_into(dev, None, None, None, 0) == total                                    # sizing: all three NULL
        for cap in (0, 1, total - 1, total, total + 1):
            w = [Window(max(cap, 1)) for _ in range(3)]
            p = [x.view[:cap] if cap else None for x in w]
            assert sel.find_into(dev, p[0], p[1], p[2], cap) == total, cap
            for x, want in zip(w, (begin, end, number)):
                x.check(want[:cap], (mode, cap))
        for left_out in range(3):
            w = [Window(total) for _ in range(3)]
            p = [None if k == left_out else w[k].view for k in range(3)]
            assert sel.find_into(dev, p[0], p[1], p[2], total) == total
            for k, want in enumerate((begin, end, number)):
                w[k].check([] if k == left_out else want, (mode, "left out", left_out))
        b, e, n = sel.find(dev)
        assert (b.cpu().numpy() == begin).all() and (e.cpu().numpy() == end).all() and (n.cpu().numpy() == number).all()
        b, e, n = sel.find(dev, capacity=5)
        assert b.cpu().tolist() == begin[:5].tolist() and e.cpu().tolist() == end[:5].tolist() and n.cpu().tolist() == number[:5].tolist()


# ---- 6. corner views ------------------------------------------------------------------------------------------------------------------
def test_corner_views(ss):
    for mode in (EACH, MERGE):
        for flags in (0, KEEP_SHORT):
            sel = make(ss, b",", mode, 1, 1, flags)
            assert sel.count((0, 0)) == (0, 0) and sel.find_into((0, 0), None, None, None, 0) == 0          # an empty view
            w = Window(4)
            assert sel.find_into((0, 0), w.view, None, None, 4) == 0
            w.check([], "empty view")
            for byte in (b"x", b",", b"\n"):                # one byte of each kind
                host = np.frombuffer(b"," * 16 + byte + b"," * 16, dtype=np.uint8)
                for first, last in ((1, 1), (2, 2), (1, 0), (2, 0)):
                    dev, view = Arena(host).view(16, 1)
                    check(ss, dev, view, b",", mode, first, last, flags, 10, byte)
    # a view with no final delimiter; separators and delimiters just outside both ends of the view do not count
    body = b"a,b c\nd e,f\n\n,g h"
    for pad in (b",", b"\n", b" ", b",\n ,\n"):
        host = np.frombuffer((pad * 40)[:37] + body + (pad * 40)[:40], dtype=np.uint8)
        for mis_shift in (0, 5):
            arena = Arena(np.concatenate((np.zeros(mis_shift, dtype=np.uint8), host)))
            dev, view = arena.view(mis_shift + 37, len(body))
            assert view.tobytes() == body
            for sep in (b",", b" ,"):
                for mode in (EACH, MERGE):
                    for first, last, flags in ((1, 1, 0), (2, 2, 0), (2, 0, 0), (3, 3, KEEP_SHORT), (1, 2, 0)):
                        check(ss, dev, view, sep, mode, first, last, flags, 10, (pad, sep))
    # a delimiter that is a member of the set does not separate, and info reports it
    host = np.frombuffer(b"a,b;c,d;e;;f,g", dtype=np.uint8)
    dev, view = Arena(host).view(0, host.size)
    for mode in (EACH, MERGE):
        for first, last in ((1, 1), (2, 2), (2, 0)):
            got = check(ss, dev, view, b",;", mode, first, last, 0, ord(";"), "the delimiter is a member")
            same = rule_fields(view, b",", mode, first, last, 0, ord(";"))
            assert all((x == y).all() for x, y in zip(got, same))
    sel = make(ss, b",;", EACH, 2, 0, KEEP_SHORT)
    assert sel.info(b";") == {"mode": 0, "first": 2, "last": 0, "flags": 1, "members": 2, "accepts_delimiter": 1}
    assert sel.info(b"\n")["accepts_delimiter"] == 0 and sel.info()["accepts_delimiter"] == 0
    assert make(ss, r"[ \t]", MERGE, 7, None).info() == {"mode": 1, "first": 7, "last": 7, "flags": 0, "members": 2, "accepts_delimiter": 0}
    assert make(ss, words_of(b"abc"), EACH, 1, 9).info()["members"] == 3


# ---- 7. relations with calls that exist, on the manual ----------------------------------------------------------------------------------
def test_relations_with_calls_that_exist_on_the_manual(ss, manual, d_manual):
    with mk_lib(ss):
        empty = ss.DynamicHipSearcher.new(b"")
        lb, le, ln = (x.cpu().numpy() for x in empty.find_lines(d_manual))
        lines = empty.count_lines(d_manual)
        tokens = ss.RunPattern(r"[^ \t\n]+").find_all(d_manual)[0].cpu().numpy()
    # every line whole: EACH, 1-, KEEP_SHORT gives the records of the empty needle's matching lines
    b, e, n = (x.cpu().numpy() for x in make(ss, b" ", EACH, 1, 0, KEEP_SHORT).find(d_manual))
    assert (b == lb).all() and (e == le).all() and (n == ln).all() and b.size == lines == 20854
    for sel in (make(ss, b" ", EACH, 2, 2), make(ss, BLANKS, MERGE, 7, 0, KEEP_SHORT)):
        assert sel.count(d_manual)[1] == lines
    # awk's fields, one selector per k, are the runs of non-blanks cut at \n: here the first 2,000 lines
    head = manual[:int(le[1999]) + 1]
    d_head = d_manual[:len(head)]
    want = tokens[tokens < len(head)]
    begins, k = [], 1
    while True:
        b = make(ss, BLANKS, MERGE, k, k).find(d_head)[0].cpu().numpy()
        if b.size == 0:
            break
        begins.append(b)
        k += 1
    assert k - 1 == max(len([t for t in re.split(rb"[ \t]+", line) if t]) for line in head.split(b"\n")) and k > 3
    assert (np.sort(np.concatenate(begins)) == want).all()
    # cut
    for sep, mode, first, last, flags in ((b" ", EACH, 2, 2, 0), (BLANKS, MERGE, 2, 3, KEEP_SHORT), (b".", EACH, 1, 2, 0)):
        out = make(ss, sep, mode, first, last, flags).cut(d_head)
        assert out.cpu().numpy().tobytes() == cut_bytes(head, sep, mode, first, last, flags), (sep, mode)
    assert make(ss, b" ", EACH, 2, 2).cut(d_head, terminator=None).cpu().numpy().tobytes() == cut_bytes(head, b" ", EACH, 2, 2, terminator=b"")


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_argument_error_and_write_nothing(ss):
    with mk_lib(ss):
        L = ss.lib()
        sel = ss.FieldSelector(b",", 2)
        only = ss.FieldSelector(b"\n", 1)
        for make_it in (lambda: ss.FieldSelector(b"", 1), lambda: ss.FieldSelector(b",", 0), lambda: ss.FieldSelector(b",", 3, 2),
                        lambda: ss.FieldSelector(np.zeros(4, dtype=np.uint64), 1)):
            with pytest.raises(ss.SlicesliceError) as e:
                make_it()
            assert e.value.code == ss.SS_ERR_ARGUMENT
        with pytest.raises(ValueError):
            ss.FieldSelector(np.zeros(3, dtype=np.uint64), 1)
        with pytest.raises(ValueError):
            ss.FieldSelector("ab", 1)
        dev = torch.full((64,), ord("a"), dtype=torch.uint8, device="cuda")
        o = Window(4)
        out, out2 = ctypes.c_uint64(77), ctypes.c_uint64(78)
        h = ctypes.c_void_p(1234)
        comma = words_of(b",")
        P, Q = ctypes.byref(out), ctypes.byref(out2)
        calls = [
            lambda: L.ss_fields_new(None, 0, 1, 1, 0, ctypes.byref(h)),
            lambda: L.ss_fields_new(comma.ctypes.data, 0, 1, 1, 0, None),
            lambda: L.ss_fields_new(comma.ctypes.data, 2, 1, 1, 0, ctypes.byref(h)),                          # an unknown mode
            lambda: L.ss_fields_new(comma.ctypes.data, 0, 1, 1, 4, ctypes.byref(h)),                          # an unknown flag
            lambda: L.ss_fields_new(comma.ctypes.data, 0, 0, 0, 0, ctypes.byref(h)),                          # first == 0
            lambda: L.ss_fields_new(comma.ctypes.data, 1, 5, 4, 0, ctypes.byref(h)),                          # last below first
            lambda: L.ss_fields_new(np.zeros(4, dtype=np.uint64).ctypes.data, 0, 1, 1, 0, ctypes.byref(h)),  # an empty set
            lambda: L.ss_fields_info(None, -1, P),
            lambda: L.ss_fields_info(sel._h, -1, None),
            lambda: L.ss_fields_info(sel._h, 256, P),
            lambda: L.ss_fields_parse(b"1,2", P, Q),
            lambda: L.ss_count_fields_device(None, dev.data_ptr(), 64, 10, None, P, Q),
            lambda: L.ss_count_fields_device(sel._h, dev.data_ptr(), 64, 10, None, None, Q),
            lambda: L.ss_count_fields_device(sel._h, dev.data_ptr(), 64, 10, None, P, None),
            lambda: L.ss_count_fields_device(sel._h, None, 64, 10, None, P, Q),
            lambda: L.ss_count_fields_device(sel._h, dev.data_ptr(), 64, 256, None, P, Q),
            lambda: L.ss_count_fields_device(sel._h, dev.data_ptr(), 64, -1, None, P, Q),
            lambda: L.ss_count_fields_device(only._h, dev.data_ptr(), 64, 10, None, P, Q),                    # a set that is only the delimiter
            lambda: L.ss_find_fields_device(None, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, P),
            lambda: L.ss_find_fields_device(sel._h, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, None),
            lambda: L.ss_find_fields_device(sel._h, dev.data_ptr(), 64, 10, None, None, None, None, 4, P),
            lambda: L.ss_find_fields_device(sel._h, None, 64, 10, None, o.view.data_ptr(), None, None, 4, P),
            lambda: L.ss_find_fields_device(sel._h, dev.data_ptr(), 64, 300, None, o.view.data_ptr(), None, None, 4, P),
            lambda: L.ss_find_fields_device(only._h, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, P),
        ]
        for k, call in enumerate(calls):
            assert call() == ss.SS_ERR_ARGUMENT and L.ss_last_error(), k
        # a capturing stream: both calls wait
        graph = torch.cuda.CUDAGraph()
        probe = torch.zeros(1, dtype=torch.int64, device="cuda")
        errs = []
        with torch.cuda.graph(graph):                                       # one stream, no parallel branches
            probe.fill_(7)
            for call in (lambda: sel.count(dev), lambda: sel.find_into(dev, o.view, None, None, 4)):
                try:
                    call()
                except ss.SlicesliceError as x:
                    errs.append(x)
        torch.cuda.synchronize()
        assert len(errs) == 2 and all(e.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(e) for e in errs), errs
        assert out.value == 77 and out2.value == 78 and h.value == 1234
        o.check([], "refused")
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                other = torch.zeros(64, dtype=torch.uint8, device="cuda:1")
                assert L.ss_count_fields_device(sel._h, other.data_ptr(), 64, 10, None, P, Q) == ss.SS_ERR_ARGUMENT
                assert b"device" in L.ss_last_error()
        # the delimiter-only set is fine under another delimiter
        assert only.count(dev, b";") == (1, 1) and sel.count(dev) == (0, 1)


# ---- 9. the fixture -------------------------------------------------------------------------------------------------------------------
def test_every_row_of_the_fixture_on_the_manual(ss, manual, d_manual):
    kat = json.load(open(os.path.join(GOLDEN, "fields_kat.json")))
    assert kat["bytes"] == len(manual) and len(kat["cases"]) == 12
    for c in kat["cases"]:
        with mk_lib(ss):
            first, last = ss.parse_fields(c["fields"])
            sel = ss.FieldSelector(c["separator"], first, last, merge=c["mode"] == MERGE, keep_short=c["keep_short"])
        assert (first, last) == (c["first"], c["last"]) and sel.count(d_manual) == (c["selected"], c["lines"]), c["name"]
        b, e, n = (x.cpu().numpy() for x in sel.find(d_manual))
        assert b.size == c["records"] and int((e - b).sum()) == c["bytes_selected"], c["name"]
        assert hashlib.sha256(b.astype("<i8").tobytes() + e.astype("<i8").tobytes() + n.astype("<i8").tobytes()).hexdigest() == c["sha256"], c["name"]


# ---- 10. tools/grep_hip.py --fields ---------------------------------------------------------------------------------------------------
def test_grep_hip_fields_prints_the_selected_fields(ss, tmp_path):
    path = tmp_path / "table.csv"
    path.write_bytes(b"id,name,,city\n7,ann\nlonely\n\n,x,y,z,\n9,bob,3,rome")
    tab = tmp_path / "table.txt"
    tab.write_bytes(b"  a  b c\n\n d\ne   f  ")

    def run(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True)

    for extra in ((), ("--device-output",)):
        r = run("--fields", "2", "-d", ",", *extra, str(path))
        assert r.returncode == 0 and r.stdout == b"name\nann\n\n\nx\nbob\n", (r.stdout, r.stderr[-300:])
        r = run("--fields", "2", "-d", ",", "-s", *extra, str(path))
        assert r.returncode == 0 and r.stdout == b"name\nann\nx\nbob\n", (r.stdout, r.stderr[-300:])
        r = run("--fields", "3-", "-d", ",", "-s", *extra, str(path))
        assert r.returncode == 0 and r.stdout == b",city\ny,z,\n3,rome\n", (r.stdout, r.stderr[-300:])
        r = run("--fields", "-2", "-d", ",", *extra, str(path))
        assert r.returncode == 0 and r.stdout == b"id,name\n7,ann\nlonely\n\n,x\n9,bob\n", (r.stdout, r.stderr[-300:])
        r = run("--fields", "2", "-d", r"[ \t]", "--merge", *extra, str(tab))
        assert r.returncode == 0 and r.stdout == b"b\n\n\nf\n", (r.stdout, r.stderr[-300:])
        r = run("--fields", "2-3", "-d", " ", "--merge", "-s", *extra, str(tab))
        assert r.returncode == 0 and r.stdout == b"b c\nf  \n", (r.stdout, r.stderr[-300:])
    r = run("--fields", "1,3", "-d", ",", str(path))                # refused with the column, nothing printed
    assert r.returncode != 0 and r.stdout == b"" and b"column 2" in r.stderr and b"one call per range" in r.stderr, r.stderr[-300:]
