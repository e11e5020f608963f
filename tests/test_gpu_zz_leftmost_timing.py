"""What the leftmost-longest calls cost against what a caller had before.  One process, the manual's text tiled to 256 MiB, the calls
alternating, a host clock around synchronised calls, warmed up (the form of tests/test_gpu_zz_disjoint_timing.py).

(a) {the, then, there, he, here}: the host route - the set's `find_all`, both arrays to the host, the candidates and every
    candidate's successor by numpy's searchsorted, the greedy walk over the successors - against `count_leftmost`.  The ratio is the
    host route's time over the new call's and has a FLOOR.
(b) the one-needle set {the}: `NeedleSet.replace` against `DynamicHipSearcher.replace` of `the`.  The ratio is the set call's time
    over the searcher's and has a CEILING.  The copy pass stores 16 bytes where `replace_kernel` stores one, which predicts a ratio
    below 1; it comes out ABOVE 1, because `the` has border 0 - the searcher's call is its model plus one kernel - while the set
    lists its pairs and selects among them.  The ceiling documents that.

All results are compared before anything is timed.  The floor is the lowest ratio of 10 runs, one process each, less their spread
(max - min), rounded down, never below 1; the ceiling the highest ratio plus the spread: profiles/leftmost/timing_test_spread.jsonl,
DESIGN.md 5.18.  Observed over those 10 runs (min / median / max): (a) 79.79 / 81.78 / 84.22 - count_leftmost 3.45 ms
against 282 ms for the host route, 5,360,599 pairs of which 2,950,154 are selected - floor 75; (b) 1.604 / 1.617 / 1.631 - 2.63 ms
against 1.62 ms - ceiling 1.658."""
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
NEEDLES = [b"the", b"then", b"there", b"he", b"here"]
FLOOR_HOST_ROUTE_OVER_COUNT_LEFTMOST = 75           # observed 79.79 / 81.78 / 84.22 (min / median / max): 79.79 - 4.43 = 75.36
CEILING_SET_REPLACE_OVER_SEARCHER_REPLACE = 1.658   # observed 1.604 / 1.617 / 1.631 (min / median / max): 1.631 + 0.027 = 1.658


def host_walk(offsets, lengths):
    """the selection over the (offset, length) pairs in numpy: the last pair of every offset is its candidate, every candidate's
    successor is the first candidate at or beyond its end (one searchsorted), and the greedy walk follows the successors"""
    if offsets.size == 0:
        return 0
    last = np.ones(offsets.size, dtype=bool)
    last[:-1] = offsets[1:] != offsets[:-1]
    o, l = offsets[last], lengths[last]
    succ = np.searchsorted(o, o + l, side="left").tolist()
    total, j, n = 0, 0, len(succ)
    while j < n:
        total += 1
        j = succ[j]
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


def test_count_leftmost_against_the_host_route_and_the_set_replace_against_the_searchers():
    import sliceslice_rs_amd as ss
    torch.cuda.synchronize()
    torch.cuda.empty_cache()            # (the calls take temporary device memory: not beside what earlier tests of the process left cached)
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    hay = torch.from_numpy(manual).cuda().repeat(SIZE // manual.size + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_leftmost", False) else ss.leftmost_build
    with lib():
        five, one, the = ss.NeedleSet(NEEDLES), ss.NeedleSet([b"the"]), ss.DynamicHipSearcher(b"the")
    lens = np.array([len(n) for n in NEEDLES], dtype=np.int64)

    def host_route():
        offsets, which = five.find_all(hay)
        return host_walk(offsets.cpu().numpy(), lens[which.cpu().numpy()])

    # every result first
    want = five.count_leftmost(hay)
    pairs = five.count_total(hay)
    assert host_route() == want and 0 < want < pairs
    chosen, which = five.find_all_leftmost(hay)
    assert chosen.numel() == want and host_walk(chosen.cpu().numpy(), lens[which.cpu().numpy()]) == want   # (already selected: all are kept)
    del chosen, which
    by_set, by_searcher = one.replace(hay, [b"THE"]), the.replace(hay, b"THE")
    assert torch.equal(by_set, by_searcher) and by_set.numel() == SIZE and not torch.equal(by_set, hay)
    del by_set, by_searcher
    (new_a, old_a), (got, host) = _wall([lambda: five.count_leftmost(hay), host_route], 7)      # (a median of 3 gave way to one disturbed pair)
    assert got == host == want
    (new_b, old_b), (r1, r2) = _wall([lambda: one.replace(hay, [b"THE"]), lambda: the.replace(hay, b"THE")], 5)
    assert r1.numel() == r2.numel() == SIZE
    del r1, r2
    r_a, r_b = old_a / new_a, new_b / old_b
    timing_log("leftmost", host_route_over_count_leftmost=round(r_a, 2), set_replace_over_searcher_replace=round(r_b, 3),
               count_leftmost_ms=round(new_a, 3), host_route_ms=round(old_a, 3), set_replace_ms=round(new_b, 3),
               searcher_replace_ms=round(old_b, 3), pairs=int(pairs), selected=int(want))
    print("leftmost: the host route %.3f ms against count_leftmost's %.3f (%.2fx); replace of the one-needle set %.3f ms against the "
          "searcher's %.3f (%.3fx)" % (old_a, new_a, r_a, new_b, old_b, r_b))
    del hay
    torch.cuda.empty_cache()
    assert r_a >= FLOOR_HOST_ROUTE_OVER_COUNT_LEFTMOST, (r_a, old_a, new_a)                         # (a)
    assert r_b <= CEILING_SET_REPLACE_OVER_SEARCHER_REPLACE, (r_b, new_b, old_b)                    # (b)
