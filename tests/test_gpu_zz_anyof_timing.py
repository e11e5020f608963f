"""What the several-needle calls save against the route a caller had before them.  One process, the manual's text tiled to 256 MiB,
the calls alternating, a host clock around synchronised calls, warmed up (the form of tests/test_gpu_zz_context_timing.py).

(a) find_lines_anyof of {the, descriptor, intel} against the OLD ROUTE: three find_lines, the three number arrays copied to the
    host, np.union1d, the union copied back, lines_around - what a caller had with the context library, whose objects this library
    links unchanged (the yardstick, not the code under test).
(b) union_numbers on the same three device arrays against np.union1d on the host including both copies.

Both ratios are old time / new time.  A floor is the lowest ratio of 10 runs, one process each, less their spread (max - min),
rounded down, never below 1: profiles/anyof/timing_test_spread.jsonl, DESIGN.md 5.13."""
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
NEEDLES = (b"the", b"descriptor", b"intel")
# old time over new time.  Floor = the lowest ratio of 10 runs less their spread (max - min), rounded down, never below 1.
FLOORS = {
    "old_route_over_find_lines_anyof": 3,       # observed 5.34 / 5.65 / 7.32 (min / median / max): 5.34 - 1.98 = 3.36
    "union1d_over_union_numbers": 33,           # observed 55.75 / 61.92 / 77.96: 55.75 - 22.21 = 33.54
}


def _old_route(searchers, hay):
    """the records of the lines that hold any needle the way a caller got them before"""
    numbers = [s.find_lines(hay)[2].cpu().numpy() for s in searchers]
    union = numbers[0]
    for n in numbers[1:]:
        union = np.union1d(union, n)
    return searchers[0].lines_around(hay, torch.from_numpy(union).cuda())


def _host_union(lists):
    union = lists[0].cpu().numpy()
    for l in lists[1:]:
        union = np.union1d(union, l.cpu().numpy())
    return torch.from_numpy(union).cuda()


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


def test_anyof_against_the_old_route_and_the_union_against_numpy():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_anyof", False) else ss.anyof_build
    with lib():
        searchers = [ss.DynamicHipSearcher(n) for n in NEEDLES]
    (t_new, t_old), (got, want) = _wall([lambda: ss.find_lines_anyof(searchers, hay), lambda: _old_route(searchers, hay)], 3)
    assert got[0].numel() == want[0].numel() > 0
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    lists = [s.find_lines(hay)[2] for s in searchers]
    limit = int(got[2][-1])
    with lib():
        (t_union, t_numpy), (mine, theirs) = _wall([lambda: ss.union_numbers(lists, limit, capacity=got[2].numel()), lambda: _host_union(lists)], 5)
    assert torch.equal(mine, theirs) and torch.equal(mine, got[2])
    r_a, r_b = t_old / t_new, t_numpy / t_union
    timing_log("anyof", old_route_over_find_lines_anyof=round(r_a, 2), union1d_over_union_numbers=round(r_b, 2),
               find_lines_anyof_ms=round(t_new, 3), old_route_ms=round(t_old, 3), union_numbers_ms=round(t_union, 4),
               union1d_ms=round(t_numpy, 3), selected=int(got[0].numel()), listed=int(sum(l.numel() for l in lists)))
    print("anyof: old route %.3f ms against %.3f (%.2fx); np.union1d with its copies %.3f ms against union_numbers %.4f (%.1fx)" %
          (t_old, t_new, r_a, t_numpy, t_union, r_b))
    del hay, got, want, lists, mine, theirs
    torch.cuda.empty_cache()
    assert r_a >= FLOORS["old_route_over_find_lines_anyof"], (r_a, t_old, t_new)            # (a)
    assert r_b >= FLOORS["union1d_over_union_numbers"], (r_b, t_numpy, t_union)             # (b)
