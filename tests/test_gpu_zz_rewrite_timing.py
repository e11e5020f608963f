"""What the rewrite call costs against the route a caller had before, and against the run count of the same pattern.  One process,
the manual's text tiled to 256 MiB, the calls alternating, a host clock around synchronised calls, warmed up (the form of
tests/test_gpu_zz_runs_timing.py).

(a) ` {2,}` -> ` ` through RunPattern.replace_into against the earlier route of the same build: RunPattern.find_all, the
    complementary ranges by torch arithmetic, ss.gather_ranges with the blank as terminator, the last blank trimmed.  The ratio is
    old / new.
(b) the same call against RunPattern.count of the same pattern: one pass that writes nothing.  The ratio is replace / count.

The yardsticks are existing calls of the same build, never the code under test, and every array is compared before anything is
timed.  The floor of (a) is 0.8 times the lowest ratio of 10 runs, one process each, rounded down; the ceiling of (b) 1.1 times the
highest, rounded up to two decimals: profiles/rewrite/timing_test_spread.jsonl, DESIGN.md 5.22."""
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
FLOOR_OLD_ROUTE_OVER_REPLACE = 1.8       # (a) observed 2.26 / 2.27 / 2.28 (min / median / max): 0.8 * 2.26 = 1.81
CEILING_REPLACE_OVER_COUNT = 5.97        # (b) observed 5.255 / 5.344 / 5.424 (min / median / max): 1.1 * 5.424 = 5.9664


def test_the_rewrite_against_the_earlier_route_and_against_the_run_count():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_rewrite", False) else ss.rewrite_build
    with lib():
        blanks = ss.RunPattern(r" {2,}")

        def old_route():
            begin, end = blanks.find_all(hay)
            kept_begin = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), end])
            kept_end = torch.cat([begin, torch.full((1,), SIZE, dtype=torch.int64, device="cuda")])
            out = ss.gather_ranges(hay, kept_begin, kept_end, b" ")
            return out[:out.numel() - 1]

        # every array first
        want = old_route()
        out_len, count = blanks.replace_into(hay, b" ", None)
        assert count == blanks.count(hay) > 0 and out_len == want.numel() < SIZE
        out = torch.empty(out_len, dtype=torch.uint8, device="cuda")
        assert blanks.replace_into(hay, b" ", out) == (out_len, count) and torch.equal(out, want)
        del want
        (new_ms, old_ms), (got_new, got_old) = _wall([lambda: blanks.replace_into(hay, b" ", out), old_route], 5)
        assert got_new == (out_len, count) and got_old.numel() == out_len
        del got_old
        (replace_ms, count_ms), (got_new, n) = _wall([lambda: blanks.replace_into(hay, b" ", out), lambda: blanks.count(hay)], 9)
        assert got_new == (out_len, count) and n == count
    r_a, r_b = old_ms / new_ms, replace_ms / count_ms
    timing_log("rewrite", old_route_over_replace=round(r_a, 2), replace_over_count=round(r_b, 3), replace_ms=round(new_ms, 3),
               old_route_ms=round(old_ms, 3), replace_again_ms=round(replace_ms, 3), count_ms=round(count_ms, 3), runs=int(count), out_len=int(out_len))
    print("rewrite:  {2,} ->   %.3f ms against the earlier route's %.3f (%.2fx); against the count's %.3f (%.3fx)" %
          (new_ms, old_ms, r_a, count_ms, r_b))
    del hay, out
    torch.cuda.empty_cache()
    assert r_a >= FLOOR_OLD_ROUTE_OVER_REPLACE, (r_a, old_ms, new_ms)                           # (a)
    assert r_b <= CEILING_REPLACE_OVER_COUNT, (r_b, replace_ms, count_ms)                       # (b)
