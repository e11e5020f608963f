"""What the field calls cost against the route a caller had before, and against a one-pass streaming count that exists.  One process,
the manual's text tiled to 256 MiB, the calls alternating, a host clock around synchronised calls, warmed up (the form of
tests/test_gpu_zz_runs_timing.py).

(a) `FieldSelector(b" ", 2).find` with room for every record against the earlier route: `find_lines` of the empty needle, `find_all`
    of the separator, both copied to the host, a `numpy.searchsorted` join.  The assertion is only that the new call is faster:
    new / old < 1; no tighter bound was known before it was measured.  Measured 0.00143 / 0.00164 / 0.00187 (min / median / max of 10 runs): about 1.07 ms
    against 688 ms.
(b) `FieldSelector(b" ", 2).count` against `RunPattern(r"[^ \\n]+").count` of the same build and view, the nearest one-pass model.
    The ratio is fields / runs.  Measured 2.292 / 2.362 / 2.384 (min / median / max of 10 runs): 0.240 ms against 0.101 ms; the ceiling is
    1.1 * 2.384 = 2.6224, rounded up to 2.63.

The yardsticks are existing calls of the same build, never the code under test, and every array is compared before anything is
timed.  The ceiling of (b) is 1.1 times the highest ratio of 10 runs, one process each, rounded up to two decimals, the margin the
sibling timing tests document: profiles/fields/timing_test_spread.jsonl, DESIGN.md 5.23."""
import os

import numpy as np
import pytest
import torch

from conftest import timing_log
from test_gpu_matches import _loaded
from test_gpu_zz_masked_timing import _wall

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SIZE = 256 * MiB
CEILING_NEW_OVER_OLD_ROUTE = 1.0         # (a) the issue's bound: faster than the earlier route
CEILING_FIELDS_OVER_RUNS_COUNT = 2.63    # (b) observed 2.292 / 2.362 / 2.384 (min / median / max): 1.1 * 2.384 = 2.6224


def test_the_field_find_against_the_earlier_route_and_the_count_against_the_run_count():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_fields", False) else ss.fields_build
    with lib():
        sel = ss.FieldSelector(b" ", 2)
        empty, blank = ss.DynamicHipSearcher.new(b""), ss.DynamicHipSearcher.new(b" ")
        tokens = ss.RunPattern(r"[^ \n]+")

    def old_route():
        lb, le, ln = (x.cpu().numpy() for x in empty.find_lines(hay))
        sp = blank.find_all(hay).cpu().numpy()                  # every separator byte, copied to the host
        k = np.searchsorted(sp, lb)                             # the first separator at or behind each line's begin
        k0, k1 = np.minimum(k, sp.size - 1), np.minimum(k + 1, sp.size - 1)
        has1 = (k < sp.size) & (sp[k0] < le)                    # the line has a second field
        has2 = (k + 1 < sp.size) & (sp[k1] < le)                # ... and a separator that ends it
        return (sp[k0] + 1)[has1], np.where(has2, sp[k1], le)[has1], ln[has1]

    def new_route():
        return sel.find(hay)

    # every array first
    want = old_route()
    got = [x.cpu().numpy() for x in new_route()]
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and want[0].size > 0
    selected, lines = sel.count(hay)
    assert selected == want[0].size and lines == empty.count_lines(hay) and tokens.count(hay) > selected
    del got
    (new_ms, old_ms), (_, again) = _wall([new_route, old_route], 3)
    assert np.array_equal(again[0], want[0])
    (count_ms, runs_ms), (pair, n_runs) = _wall([lambda: sel.count(hay), lambda: tokens.count(hay)], 9)
    assert pair == (selected, lines) and n_runs > 0
    r_a, r_b = new_ms / old_ms, count_ms / runs_ms
    timing_log("fields", find_over_old_route=round(r_a, 5), fields_count_over_runs_count=round(r_b, 3), find_ms=round(new_ms, 3),
               old_route_ms=round(old_ms, 3), fields_count_ms=round(count_ms, 3), runs_count_ms=round(runs_ms, 3), records=int(selected))
    print("fields: find %.3f ms against the earlier route's %.3f (%.5f of it); count %.3f ms against the run count's %.3f (%.3fx)" %
          (new_ms, old_ms, r_a, count_ms, runs_ms, r_b))
    del hay
    torch.cuda.empty_cache()
    assert r_a < CEILING_NEW_OVER_OLD_ROUTE, (r_a, new_ms, old_ms)                              # (a)
    assert r_b <= CEILING_FIELDS_OVER_RUNS_COUNT, (r_b, count_ms, runs_ms)                      # (b)
