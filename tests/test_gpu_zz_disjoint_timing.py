"""What the non-overlapping calls cost against what a caller had before.  One process, the manual's text tiled to 256 MiB, the calls
alternating, a host clock around synchronised calls, warmed up (the form of tests/test_gpu_zz_setmatches_timing.py).

(a) the two-space needle, which overlaps itself: the old route - `find_all` of every overlapping occurrence, the offsets to the host
    and the greedy walk in numpy (vectorised where a run's gaps are uniform, which they all are here) - against `count_disjoint`.
    The ratio is the old route's time over the new call's and has a FLOOR.
(b) `the`, whose border is 0: `count_disjoint` against `count` of the same build.  The call IS its model - the same launches - so the
    expectation from the code is 1; the ratio is the new call's time over the model's and has a CEILING.

All results are compared before anything is timed.  The floor is the lowest ratio of 10 runs, one process each, less their spread
(max - min), rounded down, never below 1; the ceiling the highest ratio plus the spread: profiles/disjoint/timing_test_spread.jsonl,
DESIGN.md 5.16.  Observed over those 10 runs (min / median / max): (a) 135.68 / 139.01 / 142.31 - count_disjoint 2.69 ms against
372 ms for the host route, 39,188,999 overlapping occurrences of which 21,306,875 are selected - floor 129; (b) 0.997 / 1.004 /
1.008 - 0.241 ms against 0.240 ms - ceiling 1.019."""
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
FLOOR_HOST_ROUTE_OVER_COUNT_DISJOINT = 129      # observed 135.68 / 139.01 / 142.31 (min / median / max): 135.68 - 6.63 = 129.05
CEILING_COUNT_DISJOINT_OVER_COUNT = 1.019       # observed 0.997 / 1.004 / 1.008 (min / median / max): 1.008 + 0.011 = 1.019


def host_walk(offsets, n):
    """the greedy selection over ascending offsets in numpy: runs are cut at the heads, a run of one offset is one selection, a run
    whose gaps are all d selects every ceil(n / d)-th entry, and only a run with mixed gaps is walked offset by offset"""
    if offsets.size == 0:
        return 0
    gaps = np.diff(offsets)
    heads = np.flatnonzero(np.concatenate([[True], gaps >= n]))
    ends = np.concatenate([heads[1:], [offsets.size]])
    lens = ends - heads
    total = int((lens == 1).sum())
    multi = np.flatnonzero(lens > 1)
    if multi.size:
        g = np.concatenate([gaps, [0]])
        idx = np.stack([heads[multi], ends[multi] - 1], axis=1).ravel()
        lo, hi = np.minimum.reduceat(g, idx)[::2], np.maximum.reduceat(g, idx)[::2]
        uniform = lo == hi
        step = -(-n // lo[uniform])
        total += int((-(-lens[multi][uniform] // step)).sum())
        for r in multi[~uniform]:
            nxt = -1
            for p in offsets[heads[r]:ends[r]].tolist():
                if p >= nxt:
                    total += 1
                    nxt = p + n
    return total


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


def test_count_disjoint_against_the_host_route_and_against_its_model():
    import sliceslice_rs_amd as ss
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    hay = torch.from_numpy(manual).cuda().repeat(SIZE // manual.size + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_disjoint", False) else ss.disjoint_build
    with lib():
        spaces, the = ss.DynamicHipSearcher(b"  "), ss.DynamicHipSearcher(b"the")
    # every result first
    overlapping = spaces.count(hay)
    offsets = torch.empty(overlapping, dtype=torch.int64, device="cuda")

    def host_route():
        spaces.find_all_into(hay, offsets)
        return host_walk(offsets.cpu().numpy(), 2)

    want = spaces.count_disjoint(hay)
    assert want == hay.cpu().numpy().tobytes().count(b"  ") < overlapping
    assert host_route() == want
    kept = spaces.find_all_disjoint(hay)
    assert kept.numel() == want and host_walk(kept.cpu().numpy(), 2) == want        # (already disjoint: the walk keeps every one)
    assert the.count_disjoint(hay) == the.count(hay) > 0
    del kept
    (new_a, old_a), (got, host) = _wall([lambda: spaces.count_disjoint(hay), host_route], 3)
    assert got == host == want
    (new_b, model_b), (c1, c2) = _wall([lambda: the.count_disjoint(hay), lambda: the.count(hay)], 7)
    assert c1 == c2
    r_a, r_b = old_a / new_a, new_b / model_b
    timing_log("disjoint", host_route_over_count_disjoint=round(r_a, 2), count_disjoint_over_count=round(r_b, 3),
               count_disjoint_ms=round(new_a, 3), host_route_ms=round(old_a, 3), border0_count_disjoint_ms=round(new_b, 3),
               border0_count_ms=round(model_b, 3), overlapping=int(overlapping), disjoint=int(want))
    print("disjoint: the host route %.3f ms against count_disjoint's %.3f (%.2fx); count_disjoint of a border-0 needle %.3f ms against "
          "count's %.3f (%.3fx)" % (old_a, new_a, r_a, new_b, model_b, r_b))
    del hay, offsets
    torch.cuda.empty_cache()
    assert r_a >= FLOOR_HOST_ROUTE_OVER_COUNT_DISJOINT, (r_a, old_a, new_a)                 # (a)
    assert r_b <= CEILING_COUNT_DISJOINT_OVER_COUNT, (r_b, new_b, model_b)                  # (b)
