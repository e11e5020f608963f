"""What the grouping call costs against the route a caller had before, and against the tokenising call it stands on.  One process, the
manual's text tiled to 64 MiB, a host clock around synchronised calls, warmed up (the form of tests/test_gpu_zz_fields_timing.py).

(a) `RunPattern(r"\\w+").groups` against the earlier route: `find_all`, both arrays copied to the host, a `collections.Counter` over
    the slices of the text.  The assertion is only that the device call is faster: new / old < 1; no tighter bound was known before
    it was measured.  The old route takes seconds, so it is timed once, in the run that checks the answer.
    Measured 0.001271 / 0.001392 / 0.001447 (min / median / max of 10 runs): about 1.64 ms against 1183 ms.
(b) `RunPattern(r"\\w+").groups` - one ss_group_runs_device - against `RunPattern(r"\\w+").find_all` of the same pattern, build and
    buffer, its model and lower bound: the call tokenises exactly so, and then reads every token again.  The ratio is groups /
    find_all.  Measured 7.110 / 7.299 / 7.409 (min / median / max of 10 runs): 1.635 ms against 0.225 ms; the ceiling is
    1.1 * 7.409 = 8.1499, rounded up to 8.15.  (With the wave's ballot loop alone, before the count kernel had its LDS table, the
    ratio was 10.557 / 11.008 / 11.227.)

The yardsticks are existing calls of the same build, never the code under test, and every row is compared before anything is timed:
profiles/groups/timing_test_spread.jsonl, DESIGN.md 5.24."""
import collections
import os
import time

import numpy as np
import pytest
import torch

from conftest import timing_log
from test_gpu_matches import _loaded
from test_gpu_zz_masked_timing import _wall

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SIZE = 64 * MiB
CEILING_NEW_OVER_OLD_ROUTE = 1.0         # (a) the issue's bound: faster than the earlier route
CEILING_GROUPS_OVER_FIND_ALL = 8.15      # (b) observed 7.110 / 7.299 / 7.409 (min / median / max): 1.1 * 7.409 = 8.1499


def test_the_grouping_against_the_earlier_route_and_against_find_all():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    host = hay.cpu().numpy().tobytes()
    lib = _loaded if getattr(ss.lib(), "has_groups", False) else ss.groups_build
    with lib():
        pat = ss.RunPattern(r"\w+")

    def old_route():
        begin, end = (x.cpu().tolist() for x in pat.find_all(hay))
        return collections.Counter(host[b:e] for b, e in zip(begin, end))

    def new_route():
        return pat.groups(hay)

    # every row first; the old route is timed here, once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = old_route()
    old_ms = (time.perf_counter() - t0) * 1e3
    begin, end, count = (x.cpu().tolist() for x in new_route())
    assert [(host[b:e], c) for b, e, c in zip(begin, end, count)] == list(want.items()) and len(want) > 5000
    tokens = sum(count)
    del want
    (new_ms, find_ms), (_, found) = _wall([new_route, lambda: pat.find_all(hay)], 5)
    assert found[0].numel() == tokens
    r_a, r_b = new_ms / old_ms, new_ms / find_ms
    timing_log("groups", groups_over_old_route=round(r_a, 6), groups_over_find_all=round(r_b, 3), groups_ms=round(new_ms, 3),
               old_route_ms=round(old_ms, 1), find_all_ms=round(find_ms, 3), tokens=int(tokens), groups=len(begin))
    print("groups: %.3f ms against the earlier route's %.1f (%.6f of it) and find_all's %.3f (%.2fx)" % (new_ms, old_ms, r_a, find_ms, r_b))
    del hay
    torch.cuda.empty_cache()
    assert r_a < CEILING_NEW_OVER_OLD_ROUTE, (r_a, new_ms, old_ms)                              # (a)
    assert r_b <= CEILING_GROUPS_OVER_FIND_ALL, (r_b, new_ms, find_ms)                          # (b)
