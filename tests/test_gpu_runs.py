"""GPU tests of the run calls (include/sliceslice_hip_runs.h, libsliceslice_hip_runs.so) against THE RULE restated in numpy
(tests/test_runs_cpu.py: rule_runs, rule_lines), against calls of the same build that exist, and against tests/golden/runs_kat.json
(Python's re).  Every comparison is of integers and exact; every output array is a window of a larger one whose sentinels on both
sides must survive.  The geometry's units are lane 16 B, piece 1 KiB, wave 4 KiB, tile 16 KiB and workgroup 128 KiB, so - the
manual's text aside - no view is larger than 300 KiB (two workgroups and a tail); views of more than one chunk of 256 workgroups are
tests/test_gpu_set_grids.py's."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_classes_cpu import members, re_set, sets_of                                  # noqa: E402
from test_gpu_masked import LANE, PIECE, TILE, WAVE, WG, Arena, Window                  # noqa: E402
from test_runs_cpu import G, rule_lines, rule_runs                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BOUNDS = ((1, None), (2, None), (1, 1), (3, 3), (16, None), (17, None), (33, 40), (4096, None), (1, 4096), (4096, 4096))
WORD = sets_of(re_set(r"\w"))[0]                # 4 ranges: the range path
FULL = np.full(4, ~np.uint64(0))


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def mk_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.runs_build()`."""
    return _loaded() if getattr(ss.lib(), "has_runs", False) else ss.runs_build()


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


def make(ss, words, lo=1, hi=None, bitmap=False):
    with mk_lib(ss):
        return ss.RunPattern.from_set(words, lo, hi, bitmap)


def parsed(ss, text, ignore_case=False):
    with mk_lib(ss):
        return ss.RunPattern(text, ignore_case)


def haystack(words, p, size, rng):
    """bytes that are members of the set with probability p"""
    table = members(np.asarray(words).reshape(1, 4))[0]
    inside, outside = np.flatnonzero(table).astype(np.uint8), np.flatnonzero(~table).astype(np.uint8)
    return np.where(rng.random(size) < p, rng.choice(inside, size), rng.choice(outside, size)).astype(np.uint8)


def check_runs(pat, dev, begin, end, what):
    n = begin.size
    assert pat.count(dev) == n, (what, "count")
    wb, we = Window(n + 2), Window(n + 2)
    assert pat.find_all_into(dev, wb.view, we.view, n + 2) == n, (what, "find_all total")
    wb.check(begin, (what, "begin"))
    we.check(end, (what, "end"))


def check_lines(pat, dev, want, delimiter, what):
    begin, end, number = want
    assert pat.count_lines(dev, bytes([delimiter])) == begin.size, (what, "count_lines")
    wb, we, wn = Window(begin.size + 2), Window(begin.size + 2), Window(begin.size + 2)
    assert pat.find_lines_into(dev, wb.view, we.view, wn.view, begin.size + 2, bytes([delimiter])) == begin.size, (what, "find_lines total")
    wb.check(begin, (what, "begin"))
    we.check(end, (what, "end"))
    wn.check(number, (what, "number"))


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.98, 0.02])
def test_the_rule_over_borders_bounds_misalignments_and_both_paths(ss, p):
    rng = np.random.default_rng(31)
    lengths = [0, 1, 15, 16, 17] + [u + d for u in (PIECE, WAVE, TILE, WG) for d in (-1, 0, 1)] + [2 * WG + 17]
    arena = Arena(haystack(WORD, p, 2 * WG + 17 + 16, rng))
    pats = [(lo, hi, bitmap, make(ss, WORD, lo, hi, bitmap)) for lo, hi in BOUNDS for bitmap in (False, True)]
    assert {pat.info()["path"] for _, _, bitmap, pat in pats if not bitmap} == {0} and {pat.info()["path"] for _, _, bitmap, pat in pats if bitmap} == {1}
    for mis in (0, 1, 15):
        for length in lengths:
            dev, host = arena.view(mis, length)
            table = members(WORD.reshape(1, 4))[0][host]
            d = np.diff(np.concatenate([[False], table, [False]]).astype(np.int8))
            b, e = np.flatnonzero(d == 1).astype(np.int64), np.flatnonzero(d == -1).astype(np.int64)
            assert (b == rule_runs(host, WORD)[0]).all()
            for lo, hi, bitmap, pat in pats:
                keep = (e - b >= lo) & ((e - b <= hi) if hi else True)
                what = (p, mis, length, lo, hi, bitmap)
                if length in (0, 17, TILE + 1, 2 * WG + 17) or (lo, hi) == (1, None):
                    check_runs(pat, dev, b[keep], e[keep], what)
                else:                                               # (one call instead of two: the total of find_all is the count)
                    wb, we = Window(int(keep.sum()) + 1), Window(int(keep.sum()) + 1)
                    assert pat.find_all_into(dev, wb.view, we.view, int(keep.sum()) + 1) == keep.sum(), what
                    wb.check(b[keep], what)
                    we.check(e[keep], what)


@pytest.mark.parametrize("border", [LANE, 2 * LANE, PIECE, WAVE, TILE, WG])
def test_a_run_planted_across_each_border_is_selected_by_its_length_alone(ss, border):
    letters = sets_of(re_set(r"[a-z]"))[0]
    where = border if border >= 64 else border + 64             # (80 and 96: room for 17 bytes in front of the two small borders)
    host = np.zeros(where + 64, dtype=np.uint8)
    for mis in (0, 5):
        for k in (0, 1, 15, 16, 17):
            for j in (0, 1, 15, 16, 17):
                length = k + j
                if length == 0:
                    continue
                host[:] = ord("-")
                # the arena's offset `where` is a border of the geometry, which starts at the 16-byte aligned address below the view
                at = where
                host[at - k:at + j] = ord("q")
                arena = Arena(host)
                dev, view = arena.view(mis, host.size - 16)
                begin = at - k - mis
                assert dev.data_ptr() % 16 == mis % 16 and view[begin] == ord("q") and (begin == 0 or view[begin - 1] != ord("q"))
                for bitmap in (False, True):
                    queries = [(length, None, 1), (length + 1, None, 0), (1, length, 1), (length, length, 1)] + ([(1, length - 1, 0)] if length > 1 else [])
                    for lo, hi, want in queries:
                        pat = make(ss, letters, lo, hi, bitmap)
                        what = (border, mis, k, j, lo, hi, bitmap)
                        check_runs(pat, dev, np.array([begin][:want]), np.array([begin + length][:want]), what)


def test_absent_bytes_are_no_members_whatever_memory_holds(ss):
    size = 300 * 1024
    arena = Arena(np.full(size + 64, ord("x"), dtype=np.uint8))        # member bytes in front of the view and behind it
    for mis in (0, 7, 17):
        dev, host = arena.view(mis, size)
        for bitmap in (False, True):
            check_runs(make(ss, FULL, 1, None, bitmap), dev, np.array([0]), np.array([size]), (mis, bitmap, "one run is the whole view"))
            check_runs(make(ss, FULL, 4096, None, bitmap), dev, np.array([0]), np.array([size]), (mis, bitmap, "min 4096"))
            check_runs(make(ss, FULL, 1, 4096, bitmap), dev, np.array([]), np.array([]), (mis, bitmap, "too long for max 4096"))
            check_lines(make(ss, FULL, 1, None, bitmap), dev, (np.array([0]), np.array([size]), np.array([1])), 10, (mis, bitmap, "one line"))
            short, _ = arena.view(mis, 100)
            check_runs(make(ss, FULL, 100, 100, bitmap), short, np.array([0]), np.array([100]), (mis, bitmap, "exactly the view"))
            check_runs(make(ss, FULL, 101, None, bitmap), short, np.array([]), np.array([]), (mis, bitmap, "min above the view"))
            check_runs(make(ss, FULL, 1, 99, bitmap), short, np.array([]), np.array([]), (mis, bitmap, "max below the view"))


def test_capacities_with_either_array_left_out_and_a_run_across_the_workgroup_border(ss):
    rng = np.random.default_rng(33)
    host = haystack(WORD, 0.6, 2 * WG + 5000, rng)
    host[WG - 40:WG + 3 + 40] = ord("w")                            # a run across the 128 KiB border of the view below (mis 3)
    arena = Arena(host)
    dev, view = arena.view(3, host.size - 3)
    for lo, hi in ((1, None), (3, None), (2, 6)):
        pat = make(ss, WORD, lo, hi)
        begin, end = rule_runs(view, WORD, lo, hi)
        total = begin.size
        nb0, ne0 = int((begin < WG - 3).sum()), int((end <= WG - 3).sum())
        if (lo, hi) != (2, 6):
            assert nb0 == ne0 + 1                                   # the first workgroup holds a begin whose end the second one holds
        for cap in (0, 1, ne0 - 1, ne0, nb0, nb0 + 1, nb0 + 700, total - 1, total, total + 1):
            for which in ("both", "begin", "end"):
                wb, we = Window(max(cap, 1)), Window(max(cap, 1))
                args = (wb.view if which != "end" and cap else None, we.view if which != "begin" and cap else None)
                assert pat.find_all_into(dev, args[0], args[1], cap) == total, (lo, hi, cap, which)
                k = min(cap, total)
                wb.check(begin[:k] if args[0] is not None else [], (lo, hi, cap, which, "begin"))
                we.check(end[:k] if args[1] is not None else [], (lo, hi, cap, which, "end"))
        b, e = pat.find_all(dev)
        assert (b.cpu().numpy() == begin).all() and (e.cpu().numpy() == end).all()
        b, e = pat.find_all(dev, capacity=5)
        assert b.cpu().tolist() == begin[:5].tolist() and e.cpu().tolist() == end[:5].tolist()


def test_the_line_calls_under_capacities_with_each_array_left_out(ss):
    """find_lines_into on the two-workgroup haystack above: no room, one record, the lines closed in the first workgroup and one
    fewer and one more, all but one, all; each of begin, end and number left out in turn.  The total is returned every time."""
    rng = np.random.default_rng(33)
    host = haystack(WORD, 0.6, 2 * WG + 5000, rng)
    host[WG - 40:WG + 3 + 40] = ord("w")
    arena = Arena(host)
    dev, view = arena.view(3, host.size - 3)
    for lo, hi, bitmap in ((1, None, False), (3, None, True), (2, 6, False)):
        pat = make(ss, WORD, lo, hi, bitmap)
        want = rule_lines(view, WORD, lo, hi, 10)
        total = want[0].size
        first = int((want[1] < WG - 3).sum())                       # the delimiter lies in the first workgroup
        assert 2 < first < total - 2 and int((want[1] >= 2 * WG - 3).sum()) > 0
        for cap in sorted({0, 1, first - 1, first, first + 1, total - 1, total}):
            for skip in (None, 0, 1, 2) if cap else (None,):
                ws = [Window(max(cap, 1)) for _ in range(3)]
                args = [None if (k == skip or cap == 0) else ws[k].view for k in range(3)]
                assert pat.find_lines_into(dev, args[0], args[1], args[2], cap) == total, (lo, hi, cap, skip)
                for k, name in enumerate(("begin", "end", "number")):
                    ws[k].check(want[k][:cap] if args[k] is not None else [], (lo, hi, bitmap, cap, skip, name))


# ---- runs that the 32-bit window leaves undecided -------------------------------------------------------------------------------
WALKS = (((33, 40), (32, 33, 40, 41)), ((4096, None), (4095, 4096)), ((1, 4096), (4096, 4097)), ((4096, 4096), (4095, 4096, 4097)))


@pytest.mark.parametrize("bounds,lengths", WALKS, ids=["%d-%s" % b for b, _ in WALKS])
def test_runs_that_only_a_walk_decides_across_every_border_and_cut_by_the_view(ss, bounds, lengths):
    """Runs of [a-z] as long as the bounds, one byte shorter and one byte longer, laid across a piece, a wave, a tile and a workgroup
    border with 1, 16, 17 and L - 1 bytes in front, on both paths at misalignment 0 and 5.  Then every run cut by a view: one that
    begins k bytes into it (the member bytes that memory holds in front of the view are absent) and one that ends k bytes before
    its end, with k such that lo - 1, lo, hi and hi + 1 bytes stay visible."""
    letters = sets_of(re_set(r"[a-z]"))[0]
    lo, hi = bounds
    pats = [make(ss, letters, lo, hi, bitmap) for bitmap in (False, True)]
    assert [p.info()["path"] for p in pats] == [0, 1]
    borders = (5 * PIECE, 3 * WAVE, 2 * TILE, WG)                   # each a border of its unit and of no larger one
    assert all(x % u == 0 and x % (4 * u) != 0 for x, u in zip(borders, (PIECE, WAVE, TILE, WG)))
    size = WG + 4200 + 16
    cuts = 0
    for length in lengths:
        selected = lo <= length <= (hi or length)
        for front in (1, 16, 17, length - 1):
            host = np.full(size, ord("-"), dtype=np.uint8)
            for x in borders:
                host[x - front:x - front + length] = ord("q")
            b, e = rule_runs(host, letters)
            assert b.tolist() == [x - front for x in borders] and (e - b == length).all()
            arena = Arena(host)
            for mis in (0, 5):                                      # the arena's offsets are the geometry's: the borders stay
                dev, view = arena.view(mis, size - 16)
                want = rule_runs(view, letters, lo, hi)
                assert want[0].size == (4 if selected else 0)
                for pat in pats:
                    check_runs(pat, dev, want[0], want[1], (bounds, length, front, mis, pat.info()["path"]))
            for rb in b.tolist():
                for visible in sorted({lo - 1, lo} | ({hi, hi + 1} if hi else set())):
                    k = length - visible
                    if not 0 < k < length:
                        continue
                    views = [arena.view(rb + k, length - k + 64)]                       # begins k bytes into the run
                    for mis in (0, 5):                                                  # ends k bytes before the run's end
                        begin = (rb - 64) // 16 * 16 + mis
                        views.append(arena.view(begin, rb + length - k - begin))
                    for j, (dev, view) in enumerate(views):
                        want = rule_runs(view, letters, lo, hi)
                        assert want[0].size == (1 if lo <= visible <= (hi or visible) else 0)
                        if want[0].size:
                            assert (want[0][0], want[1][0]) == ((0, visible) if j == 0 else (view.size - visible, view.size))
                        for pat in pats:
                            check_runs(pat, dev, want[0], want[1], (bounds, length, front, rb, visible, j, pat.info()["path"]))
                        cuts += 1
    assert cuts >= 3 * 4 * 4                                        # (some run was cut on both sides at every border and front)


def test_the_two_paths_agree_on_sets_of_one_to_four_ranges_and_info_reports_the_path(ss):
    rng = np.random.default_rng(34)
    size = WG + 3000
    for trial in range(24):
        nranges = 1 + trial % 4
        table = np.zeros(256, dtype=bool)
        cuts = np.sort(rng.choice(np.arange(1, 255), 2 * nranges, replace=False)) if trial % 8 < 6 else None
        if cuts is None:                                            # ranges that touch 0x00, 0x7F / 0x80 and 0xFF
            cuts = np.array([0, 5, 0x70, 0x7F, 0x80, 0x90, 0xF0, 0xFF][:2 * nranges])
        for r in range(nranges):
            table[cuts[2 * r]:cuts[2 * r + 1] + (1 if trial % 8 >= 6 else 0)] = True
        words = sets_of(table)[0]
        host = rng.integers(0, 256, size, dtype=np.uint8) if trial % 2 else haystack(words, 0.7, size, rng)
        arena = Arena(host)
        dev, view = arena.view(trial % 16, size - 16)
        for lo, hi in ((1, None), (2, 9), (20, None)):
            ranged, bitmap = make(ss, words, lo, hi, False), make(ss, words, lo, hi, True)
            info = ranged.info()
            want_ranges = int((np.diff(np.concatenate([[0], table.astype(np.int8)])) == 1).sum())
            assert (info["path"], info["ranges"], info["members"], info["min_len"], info["max_len"]) == (0, want_ranges, int(table.sum()), lo, hi or 0)
            assert bitmap.info()["path"] == 1 and bitmap.info()["ranges"] == want_ranges <= 4
            begin, end = rule_runs(view, words, lo, hi)
            check_runs(ranged, dev, begin, end, (trial, lo, hi, "ranges"))
            check_runs(bitmap, dev, begin, end, (trial, lo, hi, "bitmap"))
    # five ranges and more take the bitmap path unasked
    vowels = sets_of(re_set(r"[aeiou]"))[0]
    pat = make(ss, vowels, 2)
    assert pat.info()["path"] == 1 and pat.info()["ranges"] == 5 and pat.info(b"a")["accepts_delimiter"] == 1 and pat.info(b"b")["accepts_delimiter"] == 0
    host = haystack(vowels, 0.5, 5000, rng)
    arena = Arena(host)
    dev, view = arena.view(1, 4990)
    check_runs(pat, dev, *rule_runs(view, vowels, 2), "five ranges")


# ---- relations within the same build, on the manual --------------------------------------------------------------------------------
def test_relations_with_calls_that_exist_on_the_manual(ss, manual, d_manual):
    assert parsed(ss, r"\S+").count(d_manual) == 119666 == len(manual.split())
    begin, end = parsed(ss, r"\w+").find_all(d_manual)
    with mk_lib(ss):
        eight = ss.ClassPattern(r"\w{8}").count(d_manual)
        every_line = ss.DynamicHipSearcher.new(b"").find_lines(d_manual)
    assert int(torch.clamp(end - begin - 7, min=0).sum()) == eight == 46025
    lb, le, _ = every_line
    keep = le > lb
    begin, end = parsed(ss, r"[^\n]+").find_all(d_manual)
    assert torch.equal(begin, lb[keep]) and torch.equal(end, le[keep])


# ---- lines ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delimiter", [10, 0, ord("e")])
def test_lines_under_three_delimiters_with_a_set_that_holds_the_delimiter(ss, delimiter):
    rng = np.random.default_rng(35)
    table = re_set(r"\w").copy()
    table[delimiter] = True                                         # the set holds the delimiter; a run is cut there all the same
    words = sets_of(table)[0]
    size = 2 * WG + 1000
    alphabet = np.frombuffer(b"eeew_ 09-\n\x00\x00", dtype=np.uint8)
    for kind in ("dense", "sparse", "text"):
        host = rng.choice(alphabet, size) if kind == "dense" else haystack(words, 0.9, size, rng)
        if kind == "sparse":
            host[host == delimiter] = ord("x")
            host[[0, 700, WG - 1, WG, 2 * WG + 17]] = delimiter
        arena = Arena(host)
        dev, view = arena.view(5, size - 16)
        for lo, hi in ((1, None), (3, None), (2, 4), (40, None)):
            for bitmap in (False, True):
                pat = make(ss, words, lo, hi, bitmap)
                assert pat.info(bytes([delimiter]))["accepts_delimiter"] == 1
                check_lines(pat, dev, rule_lines(view, words, lo, hi, delimiter), delimiter, (kind, delimiter, lo, hi, bitmap))
    only = np.zeros(256, dtype=bool)
    only[delimiter] = True
    for bitmap in (False, True):
        pat = make(ss, sets_of(only)[0], 1, None, bitmap)
        check_lines(pat, dev, (np.array([]), np.array([]), np.array([])), delimiter, ("a set that is only the delimiter", bitmap))
        assert pat.count(dev) == rule_runs(view, sets_of(only)[0])[0].size > 0


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_every_case_of_the_fixture_on_the_manual(ss, manual, d_manual):
    kat = json.load(open(os.path.join(GOLDEN, "runs_kat.json")))
    assert kat["bytes"] == len(manual)
    for c in kat["cases"]:
        pat = parsed(ss, c["pattern"], c["ignore_case"])
        assert pat.count(d_manual) == c["count"], c["name"]
        begin, end = pat.find_all(d_manual)
        runs = list(zip(begin.cpu().tolist(), end.cpu().tolist()))
        assert len(runs) == c["count"] and G.list_hash(runs) == c["runs_sha256"], c["name"]
        assert [list(r) for r in runs[:G.KEEP]] == c["first"] and [list(r) for r in runs[-G.KEEP:]] == c["last"], c["name"]
        assert pat.count_lines(d_manual, bytes([c["delimiter"]])) == c["lines"], c["name"]
        assert pat.find_lines(d_manual, bytes([c["delimiter"]]))[0].numel() == c["lines"], c["name"]


# ---- graph capture -------------------------------------------------------------------------------------------------------------------
def test_the_async_count_is_captured_once_and_replayed_on_two_contents(ss):
    rng = np.random.default_rng(37)
    size = WG + 5000
    first, second = haystack(WORD, 0.5, size, rng), haystack(WORD, 0.8, size, rng)
    pat = make(ss, WORD, 3, None)
    arena = Arena(first)
    dev, _ = arena.view(9, size - 9)
    wants = [rule_runs(h[9:], WORD, 3)[0].size for h in (first, second)]
    assert wants[0] != wants[1]
    w = Window(1)
    assert pat.count_async(dev, w.view) is w.view                  # (first use outside the capture)
    torch.cuda.synchronize()
    w.check([wants[0]], "before the capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # one stream, no parallel branches
        pat.count_async(dev, w.view)
    for content, want in ((first, wants[0]), (second, wants[1]), (first, wants[0])):
        arena.buf[arena.at:arena.at + size].copy_(torch.from_numpy(content.copy()))
        w.view.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        w.check([want], "replayed")
    assert int(pat.count_async(dev).cpu()[0]) == wants[0]
    # the waiting calls refuse a capturing stream and write nothing
    g2 = torch.cuda.CUDAGraph()
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    errs, o = [], Window(4)
    with torch.cuda.graph(g2):
        probe.fill_(7)
        for call in (lambda: pat.count(dev), lambda: pat.find_all_into(dev, o.view, None, 4), lambda: pat.count_lines(dev),
                     lambda: pat.find_lines_into(dev, o.view, None, None, 4)):
            try:
                call()
            except ss.SlicesliceError as x:
                errs.append(x)
    torch.cuda.synchronize()
    assert len(errs) == 4 and all(e.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(e) for e in errs), errs
    o.check([], "refused while capturing")
    assert pat.count(dev) == wants[0]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_argument_error_and_write_nothing(ss):
    import ctypes
    with mk_lib(ss):
        L = ss.lib()
        pat = ss.RunPattern(r"a+")
        for make_it in (lambda: ss.RunPattern.from_set(np.zeros(4, dtype=np.uint64)), lambda: ss.RunPattern.from_set(WORD, 0),
                        lambda: ss.RunPattern.from_set(WORD, 4097), lambda: ss.RunPattern.from_set(WORD, 1, 4097), lambda: ss.RunPattern.from_set(WORD, 5, 4)):
            with pytest.raises(ss.SlicesliceError) as e:
                make_it()
            assert e.value.code == ss.SS_ERR_ARGUMENT
        with pytest.raises(ValueError):
            ss.RunPattern.from_set(np.zeros(3, dtype=np.uint64))
        assert ss.RunPattern.from_set(WORD, 4096, 4096).info()["max_len"] == 4096
        dev = torch.full((64,), ord("a"), dtype=torch.uint8, device="cuda")
        o = Window(4)
        out = ctypes.c_uint64(77)
        h = ctypes.c_void_p(1234)
        one = np.array([1, 0, 0, 0], dtype=np.uint64)
        calls = [
            lambda: L.ss_runs_new(None, 1, 0, 0, ctypes.byref(h)),
            lambda: L.ss_runs_new(one.ctypes.data, 1, 0, 0, None),
            lambda: L.ss_runs_new(np.zeros(4, dtype=np.uint64).ctypes.data, 1, 0, 0, ctypes.byref(h)),
            lambda: L.ss_runs_new(one.ctypes.data, 0, 0, 0, ctypes.byref(h)),
            lambda: L.ss_runs_new(one.ctypes.data, 4097, 0, 0, ctypes.byref(h)),
            lambda: L.ss_runs_new(one.ctypes.data, 2, 1, 0, ctypes.byref(h)),
            lambda: L.ss_runs_new(one.ctypes.data, 1, 0, 2, ctypes.byref(h)),
            lambda: L.ss_runs_info(None, -1, ctypes.byref(out)),
            lambda: L.ss_runs_info(pat._h, -1, None),
            lambda: L.ss_runs_info(pat._h, 256, ctypes.byref(out)),
            lambda: L.ss_count_runs_device(None, dev.data_ptr(), 64, None, ctypes.byref(out)),
            lambda: L.ss_count_runs_device(pat._h, dev.data_ptr(), 64, None, None),
            lambda: L.ss_count_runs_device(pat._h, None, 64, None, ctypes.byref(out)),
            lambda: L.ss_count_runs_device_async(pat._h, dev.data_ptr(), 64, None, None),
            lambda: L.ss_count_runs_device_async(None, dev.data_ptr(), 64, None, o.view.data_ptr()),
            lambda: L.ss_find_all_runs_device(None, dev.data_ptr(), 64, None, o.view.data_ptr(), None, 4, ctypes.byref(out)),
            lambda: L.ss_find_all_runs_device(pat._h, dev.data_ptr(), 64, None, o.view.data_ptr(), None, 4, None),
            lambda: L.ss_find_all_runs_device(pat._h, dev.data_ptr(), 64, None, None, None, 4, ctypes.byref(out)),
            lambda: L.ss_find_all_runs_device(pat._h, None, 64, None, o.view.data_ptr(), None, 4, ctypes.byref(out)),
            lambda: L.ss_count_lines_runs_device(None, dev.data_ptr(), 64, 10, None, ctypes.byref(out)),
            lambda: L.ss_count_lines_runs_device(pat._h, dev.data_ptr(), 64, 10, None, None),
            lambda: L.ss_count_lines_runs_device(pat._h, dev.data_ptr(), 64, 256, None, ctypes.byref(out)),
            lambda: L.ss_count_lines_runs_device(pat._h, dev.data_ptr(), 64, -1, None, ctypes.byref(out)),
            lambda: L.ss_find_lines_runs_device(None, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, ctypes.byref(out)),
            lambda: L.ss_find_lines_runs_device(pat._h, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, None),
        ]
        for k, call in enumerate(calls):
            assert call() == ss.SS_ERR_ARGUMENT and L.ss_last_error(), k
        torch.cuda.synchronize()
        assert out.value == 77 and h.value == 1234
        o.check([], "refused")
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                other = torch.zeros(64, dtype=torch.uint8, device="cuda:1")
                assert L.ss_count_runs_device(pat._h, other.data_ptr(), 64, None, ctypes.byref(out)) == ss.SS_ERR_ARGUMENT
                assert b"device" in L.ss_last_error()
        assert pat.count(dev) == 1 and ss.RunPattern(r"a{65,}").count(dev) == 0 and ss.RunPattern(r"a{64}").count(dev) == 1
        # an empty view: nothing, whatever the pointer
        assert pat.count((0, 0)) == 0 and pat.find_all_into((0, 0), None, None, 0) == 0 and pat.count_lines((0, 0)) == 0


# ---- tools/grep_hip.py --runs --------------------------------------------------------------------------------------------------------
def test_grep_hip_runs_prints_what_the_fixture_records(ss, manual):
    import subprocess
    import sys
    cases = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "runs_kat.json")))["cases"]}
    path = os.path.join(GOLDEN, "data", "i386.txt")

    def run(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True)

    c = cases["three_digits_or_more"]
    r = run("--runs", c["pattern"], "--count-lines", path)
    assert r.returncode == 0 and int(r.stdout) == c["lines"], r.stderr[-300:]
    r = run("--runs", c["pattern"], "--offsets", path)
    pairs = [[int(x) for x in line.split(b":")] for line in r.stdout.split()]
    assert r.returncode == 0 and len(pairs) == c["count"] and pairs[:G.KEEP] == c["first"] and pairs[-G.KEEP:] == c["last"], r.stderr[-300:]
    r = run("--runs", c["pattern"], "-o", path)                     # what grep -o -E prints when there is no maximum
    assert r.returncode == 0 and r.stdout == b"".join(manual[b:e] + b"\n" for b, e in pairs), r.stderr[-300:]
    arr = np.frombuffer(manual, dtype=np.uint8)
    capitals = sets_of(re_set(r"[A-Z]", True))[0]
    begin, end, number = rule_lines(arr, capitals, 12, None, 10)
    want = b"".join(b"%d:%s\n" % (n, manual[b:e]) for b, e, n in zip(begin.tolist(), end.tolist(), number.tolist()))
    r = run("--runs", "[A-Z]{12,}", "-i", "--lines", "--device-output", path)
    assert r.returncode == 0 and r.stdout == want and len(number) > 0, r.stderr[-300:]
    r = run("--runs", r"\w*", "--count", path)                      # refused with the column, nothing printed
    assert r.returncode != 0 and r.stdout == b"" and b"column 3" in r.stderr, r.stderr[-300:]
