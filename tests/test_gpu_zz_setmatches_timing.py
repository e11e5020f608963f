"""What the needle set's occurrence calls save against one per-needle call per needle.  One process, the manual's text tiled to
256 MiB, the calls alternating, a host clock around synchronised calls, warmed up (the form of tests/test_gpu_zz_needleset_timing.py).

(a) the loop of sixteen per-needle `count` calls against the set's `count` of the same needles.
(b) the loop of sixteen per-needle `find_all_into` calls, each with room for its offsets, against the set's `find_all_into` with room
    for every pair.

Both ratios are the loop's time / the set call's time: the yardstick is the existing calls of the same build, not the code under
test, and all arrays are compared before anything is timed - the counts needle by needle, the pairs against the per-needle lists
merged by (offset, rank).  A floor is the lowest ratio of 10 runs, one process each, less their spread (max - min), rounded down,
never below 1: profiles/setmatches/timing_test_spread.jsonl, DESIGN.md 5.15."""
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
# the loop's time over the set call's time
FLOORS = {
    "count_loop_over_set_count": 3,          # observed 3.64 / 3.67 / 3.72 (min / median / max): 3.64 - 0.08 = 3.56
    "find_all_loop_over_set_find_all": 1,    # observed 1.44 / 1.45 / 1.46 (min / median / max): 1.44 - 0.02 = 1.42
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


def test_the_set_against_one_per_needle_call_per_needle():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_setmatches", False) else ss.setmatches_build
    with lib():
        searchers = [ss.DynamicHipSearcher(n) for n in SIXTEEN]
        st = ss.NeedleSet(SIXTEEN)
    ranks = st.ranks()
    # every array first: the counts, then the pairs against the merged per-needle lists
    want = [s.count(hay) for s in searchers]
    assert st.count(hay).cpu().tolist() == want and min(want) > 0
    total = sum(want)
    assert st.count_total(hay) == total
    offsets, rank = torch.empty(total, dtype=torch.int64, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda")
    theirs = torch.empty(total, dtype=torch.int64, device="cuda")
    cuts = np.concatenate([[0], np.cumsum(want)])

    def loop_find():
        return [s.find_all_into(hay, theirs[cuts[k]:cuts[k + 1]]) for k, s in enumerate(searchers)]

    assert st.find_all_into(hay, offsets, rank, total) == total and loop_find() == want
    which = torch.cat([torch.full((want[k],), int(ranks[k]), dtype=torch.int64, device="cuda") for k in range(len(SIXTEEN))])
    order = torch.argsort(theirs * len(SIXTEEN) + which)        # by (offset, rank): no two needles share both
    assert torch.equal(offsets, theirs[order]) and torch.equal(rank.long(), which[order])
    del which, order
    (c_set, c_loop), (got, _) = _wall([lambda: st.count(hay), lambda: [s.count(hay) for s in searchers]], 3)
    assert got.cpu().tolist() == want
    (f_set, f_loop), (n, each) = _wall([lambda: st.find_all_into(hay, offsets, rank, total), loop_find], 3)
    assert n == total and each == want
    r_a, r_b = c_loop / c_set, f_loop / f_set
    timing_log("setmatches", count_loop_over_set_count=round(r_a, 2), find_all_loop_over_set_find_all=round(r_b, 2),
               set_count_ms=round(c_set, 3), count_loop_ms=round(c_loop, 3), set_find_all_ms=round(f_set, 3),
               find_all_loop_ms=round(f_loop, 3), pairs=int(total), needles=len(SIXTEEN))
    print("setmatches: the loop of counts %.3f ms against the set's %.3f (%.2fx); the loop of find_all %.3f ms against the set's %.3f (%.2fx)" %
          (c_loop, c_set, r_a, f_loop, f_set, r_b))
    del hay, offsets, rank, theirs
    torch.cuda.empty_cache()
    assert r_a >= FLOORS["count_loop_over_set_count"], (r_a, c_loop, c_set)                     # (a)
    assert r_b >= FLOORS["find_all_loop_over_set_find_all"], (r_b, f_loop, f_set)               # (b)
