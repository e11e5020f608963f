"""What a pattern with unknown bytes costs, and what it saves against the route a caller had before.  One process, the manual's text
tiled to 256 MiB, the calls alternating, a host clock around synchronised calls, warmed up (the form of
tests/test_gpu_zz_setmatches_timing.py).

(a) `t?e` through MaskedPattern.count against the earlier route: find_all of the pattern's longest literal run (`t`), a copy of
    every offset to the host and the numpy check of the remaining byte.  The ratio is old / new.
(b) an all-FF pattern of `descriptor` against DynamicHipSearcher.count of the same needle.  The ratio is masked / model: what a
    caller WITHOUT wildcards loses by using the masked kernel instead of the exact scan.

The yardsticks are existing calls of the same build, never the code under test, and every array is compared before anything is
timed.  The floor of (a) is the lowest ratio of 10 runs, one process each, less their spread (max - min), rounded down, never below 1;
the ceiling of (b) the highest plus their spread, rounded up to one decimal: profiles/masked/timing_test_spread.jsonl, DESIGN.md 5.19."""
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
FLOOR_OLD_ROUTE_OVER_MASKED = 274        # (a) observed 335.82 / 373.33 / 397.58 (min / median / max): 335.82 - 61.76 = 274.06
CEILING_MASKED_OVER_SEARCHER = 0.7       # (b) observed 0.62 / 0.64 / 0.65 (min / median / max): 0.65 + 0.03 = 0.68


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


def test_the_masked_count_against_the_earlier_route_and_against_the_exact_scan():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_masked", False) else ss.masked_build
    with lib():
        t_any_e, exact = ss.MaskedPattern.from_hex("74 ?? 65"), ss.MaskedPattern(b"descriptor")
        t_alone, model = ss.DynamicHipSearcher(b"t"), ss.DynamicHipSearcher(b"descriptor")
    host = hay.cpu().numpy()

    def old_route():
        offsets = t_alone.find_all(hay).cpu().numpy()           # every `t` of the haystack, copied to the host
        offsets = offsets[offsets + 2 < host.size]
        return offsets[host[offsets + 2] == ord("e")]

    # every array first
    want = old_route()
    assert t_any_e.count(hay) == want.size and want.size > 0
    assert np.array_equal(t_any_e.find_all(hay).cpu().numpy(), want)
    assert exact.count(hay) == model.count(hay) > 0
    assert torch.equal(exact.find_all(hay), model.find_all(hay))
    (new_ms, old_ms), (n_new, got) = _wall([lambda: t_any_e.count(hay), old_route], 3)
    assert n_new == want.size and np.array_equal(got, want)
    (masked_ms, model_ms), (n_masked, n_model) = _wall([lambda: exact.count(hay), lambda: model.count(hay)], 5)
    assert n_masked == n_model
    r_a, r_b = old_ms / new_ms, masked_ms / model_ms
    timing_log("masked", old_route_over_masked_count=round(r_a, 2), masked_over_searcher_count=round(r_b, 2), masked_t_any_e_ms=round(new_ms, 3),
               old_route_ms=round(old_ms, 3), masked_descriptor_ms=round(masked_ms, 3), searcher_descriptor_ms=round(model_ms, 3),
               occurrences=int(want.size))
    print("masked: t?e %.3f ms against the earlier route's %.3f (%.2fx); descriptor %.3f ms against the searcher's %.3f (%.2fx)" %
          (new_ms, old_ms, r_a, masked_ms, model_ms, r_b))
    del hay, host
    torch.cuda.empty_cache()
    assert r_a >= FLOOR_OLD_ROUTE_OVER_MASKED, (r_a, old_ms, new_ms)                            # (a)
    assert r_b <= CEILING_MASKED_OVER_SEARCHER, (r_b, masked_ms, model_ms)                      # (b)
