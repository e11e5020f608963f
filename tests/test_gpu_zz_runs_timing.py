"""What the run count costs against the route a caller had before, and against a one-pass streaming count that exists.  One process,
the manual's text tiled to 256 MiB, the calls alternating, a host clock around synchronised calls, warmed up (the form of
tests/test_gpu_zz_classes_timing.py).

(a) `\\w{8,}` through RunPattern.count against the earlier route: ClassPattern(r"\\w{8}").find_all - every position at which eight
    word bytes begin - a copy of every offset to the host, then consecutive offsets collapsed into runs in numpy.  The ratio is
    old / new.
(b) `\\w+` through RunPattern.count against MaskedPattern.from_hex of `d?scr??tor` counted in the same build: a one-pass streaming
    call that exists.  The ratio is runs / masked.

The yardsticks are existing calls of the same build, never the code under test, and every array is compared before anything is
timed.  The floor of (a) is 0.8 times the lowest ratio of 10 runs, one process each, rounded down; the ceiling of (b) 1.1 times the
highest, rounded up to two decimals: profiles/runs/timing_test_spread.jsonl, DESIGN.md 5.21."""
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
FLOOR_OLD_ROUTE_OVER_RUNS = 313          # (a) observed 391.71 / 418.27 / 464.51 (min / median / max): 0.8 * 391.71 = 313.37
CEILING_RUNS_OVER_MASKED = 1.28          # (b) observed 1.127 / 1.146 / 1.155 (min / median / max): 1.1 * 1.155 = 1.2705


def test_the_run_count_against_the_earlier_route_and_against_the_masked_count():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_runs", False) else ss.runs_build
    with lib():
        long_words, words = ss.RunPattern(r"\w{8,}"), ss.RunPattern(r"\w+")
        eight = ss.ClassPattern(r"\w{8}")
        masked = ss.MaskedPattern.from_hex("64 ?? 73 63 72 ?? ?? 74 6f 72")
    assert long_words.info()["path"] == 0 and words.info()["ranges"] == 4

    def old_route():
        offsets = eight.find_all(hay).cpu().numpy()             # every place eight word bytes begin, copied to the host
        first = np.ones(offsets.size, dtype=bool)
        first[1:] = offsets[1:] != offsets[:-1] + 1             # a run of k >= 8 word bytes shows as k - 7 consecutive offsets
        last = np.ones(offsets.size, dtype=bool)
        last[:-1] = first[1:]
        return offsets[first], offsets[last] + 8

    # every array first
    want_begin, want_end = old_route()
    assert long_words.count(hay) == want_begin.size > 0
    begin, end = long_words.find_all(hay)
    assert np.array_equal(begin.cpu().numpy(), want_begin) and np.array_equal(end.cpu().numpy(), want_end)
    del begin, end
    begin, end = words.find_all(hay)
    assert words.count(hay) == begin.numel() > 0 and int(torch.clamp(end - begin - 7, min=0).sum()) == eight.count(hay)
    del begin, end
    assert masked.count(hay) > 0
    (new_ms, old_ms), (n_new, got) = _wall([lambda: long_words.count(hay), old_route], 5)
    assert n_new == want_begin.size and np.array_equal(got[0], want_begin)
    (runs_ms, masked_ms), (n_runs, n_masked) = _wall([lambda: words.count(hay), lambda: masked.count(hay)], 9)
    assert n_runs > n_masked > 0
    r_a, r_b = old_ms / new_ms, runs_ms / masked_ms
    timing_log("runs", old_route_over_run_count=round(r_a, 2), runs_over_masked_count=round(r_b, 3), run_long_words_ms=round(new_ms, 3),
               old_route_ms=round(old_ms, 3), run_words_ms=round(runs_ms, 3), masked_descriptor_ms=round(masked_ms, 3), runs=int(want_begin.size))
    print("runs: \\w{8,} %.3f ms against the earlier route's %.3f (%.2fx); \\w+ %.3f ms against the masked kernel's %.3f (%.3fx)" %
          (new_ms, old_ms, r_a, runs_ms, masked_ms, r_b))
    del hay
    torch.cuda.empty_cache()
    assert r_a >= FLOOR_OLD_ROUTE_OVER_RUNS, (r_a, old_ms, new_ms)                              # (a)
    assert r_b <= CEILING_RUNS_OVER_MASKED, (r_b, runs_ms, masked_ms)                           # (b)
