"""GPU tests of the five libraries that share needleset_launch.hpp's launch geometry - needleset, setmatches, masked, classes, runs -
at the grids the rest of their tests do not reach: more than one chunk of lines_chunk_kernel (256 parts of 128 KiB), a line and a
carried match across a chunk border, a chunk without a delimiter, a last chunk of one part, launch_set_prefix at two parts per thread
with idle trailing threads, capacities that end inside a later chunk, and scratch that grows from a small call to a large one.

  shape A   258 parts, 33.8 MB: two chunks, the second of two parts; views at misalignment 0 and 5
  shape B   1,537 parts, 201 MB: seven chunks, the last of one part; the prefix at per = 2 with a one-part last run

One device buffer of shape B holds one filler byte; shape A is a slice of it.  Every pattern of tests/test_set_sparse_cpu.py's
PATTERNS plants the scenes of tests/_set_sparse.py in six rotations, so that each border sees each kind, and erases them again.  The
reference is worked out from the scene list alone, which tests/test_set_sparse_cpu.py holds against the dense rules.  Every
comparison is of integers and exact; every output array is a window of a larger one whose sentinels on both sides must survive."""
import time

import numpy as np
import pytest

from _set_sparse import (CHUNK, DELIM, END_A, FILLER, LEN_B, ROTATIONS, WG, Parts, buffer_scenes, sparse_lines, view_scenes)
from test_gpu_masked import GUARD, Window
from test_gpu_matches import _loaded
from test_gpu_setmatches import Window as RankWindow, distinct, given_ranks
from test_set_sparse_cpu import PATTERNS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VIEWS = (("A, mis 0", 0, END_A, (258, 2, 1)), ("A, mis 5", 5, END_A, (258, 2, 1)), ("B", 0, LEN_B, (1537, 7, 2)))
SMALL = 5000                                                # the first call of every library: a view of a few KiB, one part


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    return m


@pytest.fixture(scope="module")
def buf():
    hay = torch.full((LEN_B,), FILLER, dtype=torch.uint8, device="cuda")
    assert hay.data_ptr() % 16 == 0
    yield hay
    del hay
    torch.cuda.empty_cache()


def lib_of(ss, feature):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else the feature's own build."""
    return _loaded() if getattr(ss.lib(), "has_" + feature, False) else getattr(ss, feature + "_build")()


def make(ss, p):
    """the device side of pattern p; for a needle set (the set of the needleset build for the line calls, the set of the setmatches
    build for the occurrence calls)"""
    how = p.how
    if p.lib == "masked":
        with lib_of(ss, "masked"):
            return ss.MaskedPattern(how["value"], how["mask"])
    if p.lib == "classes":
        with lib_of(ss, "classes"):
            pat = ss.ClassPattern(how["text"])
        assert (np.asarray(pat.sets) == how["sets"]).all()
        return pat
    if p.lib in ("runs", "gaps"):
        with lib_of(ss, "runs"):
            pat = ss.RunPattern.from_set(how["words"], how["lo"], how["hi"], how["bitmap"])
        info = pat.info()
        assert (info["path"], info["min_len"], info["max_len"]) == (1 if how["bitmap"] else 0, how["lo"], how["hi"] or 0), info
        return pat
    with lib_of(ss, "needleset"):
        lines = ss.NeedleSet(how["needles"])
    with lib_of(ss, "setmatches"):
        occurrences = ss.NeedleSet(how["needles"])
    assert (occurrences.ranks() == given_ranks(how["needles"])).all()
    return lines, occurrences


def plant(hay, scenes, erase=False):
    """the scenes into the device buffer in one scatter; erase: the filler back over them"""
    idx = np.concatenate([np.arange(o, o + len(b), dtype=np.int64) for o, b in scenes])
    val = np.frombuffer(b"".join(b for _, b in scenes), dtype=np.uint8).copy()
    if erase:
        val[:] = FILLER
    hay[torch.from_numpy(idx).cuda()] = torch.from_numpy(val).cuda()


def expect(w, want, what, pt):
    """the first len(want) slots of window w hold `want`, every other slot of the larger array the sentinel; a difference is named
    by the part of the view that the first wrong record lies in"""
    h = w.buf.cpu().numpy()
    k = len(want)
    assert (h[:GUARD] == w.sent).all() and (h[GUARD + k:] == w.sent).all(), (what, "sentinels")
    got = h[GUARD:GUARD + k]
    bad = np.flatnonzero(got != np.asarray(want, dtype=h.dtype))
    if bad.size:
        j = int(bad[0])
        raise AssertionError((what, "record %d of %d: want %s, got %s" % (j, k, list(want[j:j + 3]), got[j:j + 3].tolist()),
                              "parts and ranks start to differ near part %s" % pt.part_of(min(int(want[j]), pt.length - 1))))


def capacities(total, rank):
    """the total and its neighbours, the rank at the border of chunk 1 - a cut inside a later chunk: every part behind it returns
    early - and its neighbours, and 1"""
    return sorted({c for c in (total, total - 1, total + 1, rank, rank - 1, rank + 1, 1) if c >= 0})


# ---- the calls of one pattern on one view against the reference ------------------------------------------------------------------
def check_occurrences(made, p, view, spans, pt, what, caps=True, asynchronous=False):
    s, e, g = spans
    total = s.size
    rank = int((s < pt.border(CHUNK)).sum()) if pt.parts > CHUNK else total // 2
    caps = capacities(total, rank) if caps else [total]
    if p.lib == "sets":
        st, word = made[1], p.how["word"]
        counts = np.bincount(g, minlength=len(distinct(p.how["needles"])))
        assert st.count_total(view, whole_word=word) == total, (what, "count_total")
        got = st.count(view, whole_word=word).cpu().numpy()
        assert (got == counts[given_ranks(p.how["needles"])]).all(), (what, "count", got, counts)
        for cap in caps:
            wo, wr = Window(cap), RankWindow(cap, torch.int32)
            assert st.find_all_into(view, wo.view if cap else None, wr.view if cap else None, cap, whole_word=word) == total, (what, cap)
            expect(wo, s[:cap], (what, cap, "offsets"), pt)
            expect(wr, g[:cap], (what, cap, "ranks"), pt)
        return
    assert made.count(view) == total, (what, "count")
    if asynchronous:
        w = Window(1)
        made.count_async(view, w.view)
        torch.cuda.synchronize()
        expect(w, [total], (what, "count_async"), pt)
    if p.lib in ("masked", "classes"):
        for cap in caps:
            w = Window(cap)
            assert made.find_all_into(view, w.view if cap else None, cap) == total, (what, cap)
            expect(w, s[:cap], (what, cap, "offsets"), pt)
        return
    for cap in caps:
        for skip in (None, 0, 1) if cap in (total, rank) else (None,):     # each array left out once
            if cap == 0 and skip is not None:
                continue
            ws = [Window(cap), Window(cap)]
            args = [None if (k == skip or cap == 0) else ws[k].view for k in range(2)]
            assert made.find_all_into(view, args[0], args[1], cap) == total, (what, cap, skip)
            for k, want in enumerate((s, e)):
                expect(ws[k], want[:0 if (k == skip or cap == 0) else cap], (what, cap, skip, ("begin", "end")[k]), pt)


def find_lines(made, p, view, args, cap, invert=False):
    if p.lib == "sets":
        total, selected = made[0].find_lines_into(view, args[0], args[1], args[2], None, cap, 0, 0, DELIM, whole_word=p.how["word"], invert=invert)
        assert total == selected
        return total
    assert not invert
    return made.find_lines_into(view, args[0], args[1], args[2], cap)


def check_lines(made, p, view, lines, pt, what, caps=True, invert=False):
    total = lines[0].size
    rank = int((lines[1] < pt.border(CHUNK)).sum()) if pt.parts > CHUNK else total // 2
    if p.lib == "sets":
        assert made[0].count_lines(view, whole_word=p.how["word"], invert=invert) == total, (what, "count_lines")
    else:
        assert made.count_lines(view) == total, (what, "count_lines")
    for cap in capacities(total, rank) if caps else [total]:
        for skip in (None, 0, 1, 2) if cap == rank else (None,):
            if cap == 0 and skip is not None:
                continue
            ws = [Window(cap) for _ in range(3)]
            args = [None if (k == skip or cap == 0) else ws[k].view for k in range(3)]
            assert find_lines(made, p, view, args, cap, invert) == total, (what, cap, skip)
            for k, want in enumerate(lines):
                expect(ws[k], want[:0 if (k == skip or cap == 0) else cap], (what, cap, skip, ("begin", "end", "number")[k]), pt)


def check_view(made, p, view, scenes, pt, what, cache, caps=True, asynchronous=False, invert=False):
    """every call of pattern p on `view`, whose scenes are `scenes`; returns (occurrences, lines) of the reference"""
    assert view.numel() == pt.length and view.data_ptr() % 16 == pt.mis % 16
    spans = p.spans(scenes, pt.length, cache)
    cut = spans if p.line_rule is p.rule else p.spans(scenes, pt.length, cache, lines=True)
    lines = sparse_lines(scenes, pt.length, cut)
    assert spans[0].size > 0 and lines[0].size > 0
    check_occurrences(made, p, view, spans, pt, what, caps, asynchronous)
    check_lines(made, p, view, lines, pt, what, caps)
    if invert:
        others = sparse_lines(scenes, pt.length, cut, inverted=True)
        assert others[0].size > 0
        check_lines(made, p, view, others, pt, what + ("inverted",), caps, invert=True)
    return spans[0].size, lines[0].size


# ---- the scratch lease grows -------------------------------------------------------------------------------------------------------
def test_the_first_call_of_each_library_is_small_and_the_next_at_shape_a(ss, buf):
    """Call order: each library's first call in this module is made on a view of 5,000 bytes (one part) and the next at shape A
    (258 parts, 2 chunks, per 1), so that the scratch lease of the line calls and of the find-all calls has to grow."""
    t0 = time.time()
    name, lo, hi, shape = VIEWS[0]
    nscenes = 0
    for p in (PATTERNS[1], PATTERNS[3], PATTERNS[5], PATTERNS[9]):
        made = make(ss, p)
        scenes = buffer_scenes(p.kit, 0)
        plant(buf, scenes)
        try:
            cache = {}
            for length in (SMALL, hi - lo):
                pt = Parts(length, WG, lo)
                assert (pt.parts, pt.chunks, pt.per) == ((1, 1, 1) if length == SMALL else shape)
                sc = view_scenes(scenes, lo, lo + length)
                nscenes += len(sc)
                check_view(made, p, buf[lo:lo + length], sc, pt, (p.name, length), cache, invert=p.lib == "sets")
        finally:
            plant(buf, scenes, erase=True)
    print("scratch growth: shapes (1, 1, 1) then %s, %d scenes, %.2f s" % (shape, nscenes, time.time() - t0))


# ---- every pattern at both shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PATTERNS, ids=[p.name for p in PATTERNS])
def test_both_shapes_in_six_rotations(ss, buf, p):
    """Shape A at misalignment 0 and 5 and shape B, asserted as (parts, chunks, per) = (258, 2, 1) and (1537, 7, 2) before any launch.
    count and find_all_into, count_lines and find_lines_into under the capacities of `capacities`; for the run calls and the line
    calls each array left out once; count_async into a device word at shape A for the three pattern classes; one inverted pass for
    the needle set of three."""
    t0 = time.time()
    made = make(ss, p)
    cache, nscenes, records = {}, [], 0
    for rot in range(ROTATIONS):
        scenes = buffer_scenes(p.kit, rot)
        nscenes.append(len(scenes))
        plant(buf, scenes)
        try:
            for name, lo, hi, shape in VIEWS:
                pt = Parts(hi - lo, WG, lo)
                assert (pt.parts, pt.chunks, pt.per) == shape, (name, pt)
                got = check_view(made, p, buf[lo:hi], view_scenes(scenes, lo, hi), pt, (p.name, rot, name), cache,
                                 asynchronous=p.lib != "sets" and name != "B", invert=p.name == "3 needles" and rot % 3 == 0)
                records += sum(got)
        finally:
            plant(buf, scenes, erase=True)
    print("%s: shapes %s, %d rotations of %d scenes, %d reference records, %.2f s" % (p.name, [v[3] for v in VIEWS], ROTATIONS, nscenes[0],
                                                                                       records, time.time() - t0))


def test_the_buffer_is_left_as_it_was(ss, buf):
    """every test above erased its scenes: the runs of [^\\n]+ on the whole buffer are one"""
    with lib_of(ss, "runs"):
        pat = ss.RunPattern(r"[^\n]+")
    wb, we = Window(2), Window(2)
    assert pat.find_all_into(buf, wb.view, we.view, 2) == 1
    wb.check([0], "begin")
    we.check([LEN_B], "end")
    assert int((buf != FILLER).sum()) == 0
