"""What the delimiter filter and the segmented combine cost on top of the all-matches scan: count_lines against count of the SAME
build (libsliceslice_hip_lines.so holds both; count is the matches library's code, unchanged), alternating on one buffer in one
process, hipEvents around the stream-ordered calls.  The floors follow the practice of tests/test_gpu_zz_timing.py: the lowest
ratio observed over repeated runs less the run-to-run spread (profiles/lines/timing_test_spread.jsonl)."""
import os

import numpy as np
import pytest
import torch

from conftest import timing_log

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GiB = 1 << 30
# count's time over count_lines' time (1.0 = the lines cost nothing).  Floor = the lowest ratio of 10 runs less their spread (max - min).
FLOORS = {
    "text": 1.31,          # observed 1.371 / 1.388 / 1.422 (min / median / max)
    "random": 0.55,        # observed 0.570 / 0.581 / 0.590
}


def _ratio(s, hay, rounds=9):
    """median over `rounds` of (count ms, count_lines ms), alternating"""
    d = torch.zeros(2, dtype=torch.int64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tc, tl = [], []
    for k in range(rounds + 2):
        ev[0].record()
        s.count_async(hay, d[0:1])
        ev[1].record()
        s.count_lines_async(hay, d[1:2])
        ev[2].record()
        torch.cuda.synchronize()
        if k >= 2:                                  # (the first rounds allocate scratch)
            tc.append(ev[0].elapsed_time(ev[1]))
            tl.append(ev[1].elapsed_time(ev[2]))
    return float(np.median(tc)), float(np.median(tl)), d.cpu().tolist()


@pytest.mark.parametrize("kind", ["text", "random"])
def test_count_lines_against_count(kind):
    import sliceslice_rs_amd as ss
    hay = torch.empty(GiB, dtype=torch.uint8, device="cuda")
    if kind == "text":
        text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
        reps = GiB // text.numel() + 1
        hay.copy_(text.repeat(reps)[:GiB])
        needle = b"descriptor"
    else:
        ss.fill_random_device(hay, 0x11E5)
        needle = b"the"
        hay.masked_fill_(hay == ord("t"), ord("u"))         # a `the`-like needle that does not occur
    with ss.lines_build():
        s = ss.DynamicHipSearcher(needle)
    t_count, t_lines, (n_count, n_lines) = _ratio(s, hay)
    assert 0 <= n_lines <= n_count and (kind == "text") == (n_lines > 0)
    ratio = t_count / t_lines
    gbs = GiB / t_lines / 1e6
    timing_log("count_lines_vs_count_" + kind, count_over_count_lines=round(ratio, 4), count_ms=round(t_count, 4),
               count_lines_ms=round(t_lines, 4), count_lines_gb_per_s=round(gbs, 1))
    print("count_lines_vs_count", kind, "count %.4f ms, count_lines %.4f ms, ratio %.4f, %.0f GB/s" % (t_count, t_lines, ratio, gbs))
    del hay
    torch.cuda.empty_cache()
    assert ratio >= FLOORS[kind], (kind, ratio, t_count, t_lines)

