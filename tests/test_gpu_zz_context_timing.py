"""What the context calls save against the routes a caller had before them.  One process, the manual's text tiled to 256 MiB, the
calls alternating, a host clock around synchronised calls, warmed up (the form of tests/test_gpu_zz_inverted_timing.py).

(a) find_lines_context(before = after = 2) of `descriptor` against the OLD ROUTE: find_lines for the matching records, find_lines
    with the empty needle for every line's record, both record sets copied to the host, the context lines indexed there with numpy.
(b) lines_around of one number with capacity 0 - the delimiter census and its prefix, nothing else of weight - against count_lines
    of the empty needle of the same build: the byte-wise pass that was the only way to the number of lines (the lines library's
    objects, which this library links unchanged: the yardstick, not the code under test).

Both ratios (old time / new time) must stay above a floor = the lowest ratio of 10 runs, one process each, less their spread
(max - min), rounded down, never below 1: profiles/context/timing_test_spread.jsonl, DESIGN.md 5.12."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import timing_log
from test_context_cpu import context_rule
from test_gpu_matches import _loaded

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SIZE = 256 * MiB
# old time over new time.  Floor = the lowest ratio of 10 runs less their spread (max - min), rounded down, never below 1.
FLOORS = {
    "old_route_over_find_lines_context": 1,     # observed 3.66 / 13.81 / 40.46 (min / median / max): 3.66 - 36.80 is below 1
    "count_lines_over_census": 26,              # observed 37.20 / 46.48 / 47.42: 37.20 - 10.22 = 26.98
}


def _old_route(s, every, hay, before, after):
    """the records of the matching lines and their context lines the way a caller got them before"""
    hit = [t.cpu().numpy() for t in s.find_lines(hay)]
    lines = [t.cpu().numpy() for t in every.find_lines(hay)]
    numbers, kinds = context_rule(hit[2], lines[2].size, before, after)
    return lines[0][numbers - 1], lines[1][numbers - 1], numbers, kinds


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


def test_context_against_the_old_route_and_the_census_against_the_byte_wise_pass():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    with (_loaded() if getattr(ss.lib(), "has_context", False) else ss.context_build()):
        s, every = ss.DynamicHipSearcher(b"descriptor"), ss.DynamicHipSearcher(b"")
    (t_new, t_old), (got, want) = _wall([lambda: s.find_lines_context(hay, 2, 2), lambda: _old_route(s, every, hay, 2, 2)], 3)
    assert got[0].numel() == want[0].size > 0
    for g, w in zip(got, want):
        assert (g.cpu().numpy() == w).all()
    one = torch.ones(1, dtype=torch.int64, device="cuda")
    (t_census, t_count), (n_one, n_lines) = _wall([lambda: s.lines_around_into(hay, one, None, None, None, None, 0),
                                                   lambda: every.count_lines(hay)], 9, warm=2)
    assert n_one == 1 and n_lines >= int(want[2][-1])
    r_a, r_b = t_old / t_new, t_count / t_census
    timing_log("context", old_route_over_find_lines_context=round(r_a, 2), count_lines_over_census=round(r_b, 2),
               find_lines_context_ms=round(t_new, 3), old_route_ms=round(t_old, 3), census_ms=round(t_census, 4),
               count_lines_ms=round(t_count, 4), census_gb_per_s=round(SIZE / t_census / 1e6, 1), printed=int(got[0].numel()), lines=int(n_lines))
    print("context: old route %.3f ms against %.3f (%.1fx); empty needle's count_lines %.4f ms against census %.4f (%.1fx)" %
          (t_old, t_new, r_a, t_count, t_census, r_b))
    del hay, got, want
    torch.cuda.empty_cache()
    assert r_a >= FLOORS["old_route_over_find_lines_context"], (r_a, t_old, t_new)          # (a)
    assert r_b >= FLOORS["count_lines_over_census"], (r_b, t_count, t_census)               # (b)
