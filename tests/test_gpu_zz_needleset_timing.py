"""What the needle set saves against one model call per needle.  One process, the manual's text tiled to 256 MiB, the calls alternating,
a host clock around synchronised calls, warmed up (the form of tests/test_gpu_zz_anyof_timing.py).

(a) find_lines_anyof_into of sixteen needles, with room for every line, against the set's find_lines_into of the same needles.
(b) count_lines_anyof of the same searchers against the set's count_lines.

Both ratios are the anyof call's time / the set call's time: the model is the existing call of the same build (the yardstick, not
the code under test), and both calls' arrays are compared before anything is timed.  A floor is the lowest ratio of 10 runs, one
process each, less their spread (max - min), rounded down, never below 1: profiles/needleset/timing_test_spread.jsonl,
DESIGN.md 5.14."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import timing_log
from test_gpu_matches import _loaded

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SIZE = 256 * MiB
SIXTEEN = (b"the", b"descriptor", b"intel", b"segment", b"protect", b"mode", b"386", b"register", b"page", b"task", b"gate", b"stack",
           b"flag", b"address", b"privilege", b"interrupt")
# the anyof call's time over the set call's time
FLOORS = {
    "find_lines_anyof_over_set_find_lines": 5,    # observed 5.19 / 5.25 / 5.31 (min / median / max): 5.19 - 0.12 = 5.07
    "count_lines_anyof_over_set_count_lines": 8,    # observed 8.84 / 9.06 / 9.24 (min / median / max): 8.84 - 0.40 = 8.44
}


def _wall(fns, reps, warm=1):
    """medians of the wall times of the calls `fns`, alternating, each between two synchronisations; and their last results"""
    out, times = [None] * len(fns), [[] for _ in fns]
    for k in range(reps + warm):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[j] = fn()
            torch.cuda.synchronize()
            if k >= warm:                                       # (the first round allocates scratch)
                times[j].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in times], out


def test_the_set_against_one_model_call_per_needle():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_needleset", False) else ss.needleset_build
    with lib():
        searchers = [ss.DynamicHipSearcher(n) for n in SIXTEEN]
        st = ss.NeedleSet(SIXTEEN)
    total, selected = ss.find_lines_anyof_into(searchers, hay, None, None, None, None, 0)
    assert st.find_lines_into(hay, None, None, None, None, 0) == (total, selected) and total == selected > 0
    mine = [torch.empty(total, dtype=torch.int64, device="cuda") for _ in range(3)] + [torch.empty(total, dtype=torch.uint8, device="cuda")]
    theirs = [torch.empty_like(t) for t in mine]
    (t_set, t_any), _ = _wall([lambda: st.find_lines_into(hay, *mine, total), lambda: ss.find_lines_anyof_into(searchers, hay, *theirs, total)], 3)
    for g, w in zip(mine, theirs):
        assert torch.equal(g, w)
    (c_set, c_any), (got, want) = _wall([lambda: st.count_lines(hay), lambda: ss.count_lines_anyof(searchers, hay)], 3)
    assert got == want == selected
    r_a, r_b = t_any / t_set, c_any / c_set
    timing_log("needleset", find_lines_anyof_over_set_find_lines=round(r_a, 2), count_lines_anyof_over_set_count_lines=round(r_b, 2),
               set_find_lines_ms=round(t_set, 3), find_lines_anyof_ms=round(t_any, 3), set_count_lines_ms=round(c_set, 3),
               count_lines_anyof_ms=round(c_any, 3), selected=int(selected), needles=len(SIXTEEN))
    print("needleset: find_lines_anyof %.3f ms against the set's %.3f (%.2fx); count_lines_anyof %.3f ms against the set's %.3f (%.2fx)" %
          (t_any, t_set, r_a, c_any, c_set, r_b))
    del hay, mine, theirs
    torch.cuda.empty_cache()
    assert r_a >= FLOORS["find_lines_anyof_over_set_find_lines"], (r_a, t_any, t_set)          # (a)
    assert r_b >= FLOORS["count_lines_anyof_over_set_count_lines"], (r_b, c_any, c_set)        # (b)
