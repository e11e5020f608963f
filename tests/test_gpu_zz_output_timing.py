"""What writing grep's output on the device costs against what a caller had before, and whether the copy pass is balanced.  One process,
the manual's text tiled to 64 MiB, every line with its line number, the calls alternating, a host clock around synchronised calls,
warmed up (the form of tests/test_gpu_zz_disjoint_timing.py).

(a) THE TORCH ROUTE.  What tools/grep_hip.py did before the output library: cumsum of the lengths, `repeat_interleave` into one int64
    index per output byte, an index gather - WITHOUT its host loop, which would only add to it - against `ss.format_lines` of the same
    records, which also writes the numbers and the terminators.  Asserted: the ratio of the old route's time over the new call's is
    above 1, nothing more.
(b) BALANCE.  `ss.gather_ranges` of the whole view as ONE record against `ss.gather_ranges` of the same bytes as its lines (every line
    with its delimiter, no terminator: both outputs are the view).  The grid runs over the output, so one long record is spread over
    the machine as the lines are, and it reads less metadata: it has no reason to be slower.  Asserted: one record takes no longer
    than the lines times a margin, and the margin is the recorded run-to-run spread of that call - max over min of
    `gather_one_record_ms` in profiles/output/timing_test_spread.jsonl - not a number taken from the code under test.

All results are compared before anything is timed.  Noise model (profiles/output/timing_test_spread.jsonl: 10 runs of this file under
tools/timing_spread.py, one process each, all green; min / median / max): (a) 1.71 / 2.15 / 2.25 - format_lines
0.539 / 0.567 / 0.731 ms against 1.206 / 1.213 / 1.252 ms for the torch route, 1,631,927 lines: the lowest ratio seen stands 0.71
above the bound, more than the whole spread of the ratio (0.54); (b) 0.290 / 0.315 / 0.332 - one record 0.115 / 0.121 / 0.125 ms against
0.370 / 0.393 / 0.400 ms as lines; the margin read from the file is 0.125 / 0.115 = 1.087, so the bound is 1.087 and the highest
ratio seen stands at a third of it."""
import json
import os
import time

import numpy as np
import pytest
import torch

from conftest import timing_log

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SIZE = 64 * MiB
SPREAD = os.path.join(ROOT, "profiles", "output", "timing_test_spread.jsonl")


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


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


def recorded_spread(quantity):
    """max over min of `quantity` over the recorded runs of this test"""
    rows = [json.loads(l) for l in open(SPREAD)]
    row = [r for r in rows if r.get("test") == "output" and r.get("quantity") == quantity][0]
    assert row["samples"] >= 10 and row["min"] > 0
    return row["max"] / row["min"]


def test_format_lines_against_the_torch_route_and_one_record_against_its_lines():
    import sliceslice_rs_amd as ss
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    hay = torch.from_numpy(manual).cuda().repeat(SIZE // manual.size + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_output", False) else ss.output_build
    with lib():
        begin, end, number = ss.DynamicHipSearcher(b"").find_lines(hay)

        def torch_route():
            length = end - begin
            start = torch.cumsum(length, 0) - length
            idx = torch.repeat_interleave(begin - start, length) + torch.arange(int(length.sum()), device=hay.device)
            return hay[idx]

        def new_call():
            return ss.format_lines(hay, begin, end, number)

        whole_b, whole_e = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), SIZE, dtype=torch.int64, device="cuda")
        with_delimiter = end + 1                                # (clamped to the view where the last line has none)

        def one_record():
            return ss.gather_ranges(hay, whole_b, whole_e)

        def as_lines():
            return ss.gather_ranges(hay, begin, with_delimiter)

        # every result first
        lines = begin.numel()
        packed, text = torch_route(), new_call()
        assert packed.numel() == int((end - begin).sum()) and text.numel() == packed.numel() + lines + sum(len("%d:" % k) for k in range(1, lines + 1))
        host = text[:4096].cpu().numpy().tobytes()
        assert host.startswith(b"1:" + manual[:int(end[0])].tobytes() + b"\n2:")
        assert torch.equal(one_record(), hay) and torch.equal(as_lines(), hay)
        del packed, text
        (old_a, new_a), _ = _wall([torch_route, new_call], 5)
        (one_b, lines_b), _ = _wall([one_record, as_lines], 7)
    r_a, r_b = old_a / new_a, one_b / lines_b
    timing_log("output", torch_route_over_format_lines=round(r_a, 2), one_record_over_lines=round(r_b, 3), format_lines_ms=round(new_a, 3),
               torch_route_ms=round(old_a, 3), gather_one_record_ms=round(one_b, 3), gather_lines_ms=round(lines_b, 3), lines=int(lines))
    print("output: the torch route %.3f ms against format_lines' %.3f (%.2fx); the gather of one record %.3f ms against %.3f as %d lines "
          "(%.3fx)" % (old_a, new_a, r_a, one_b, lines_b, lines, r_b))
    del hay
    torch.cuda.empty_cache()
    assert r_a > 1, (r_a, old_a, new_a)                                                     # (a)
    margin = recorded_spread("gather_one_record_ms")
    assert one_b <= lines_b * margin, (one_b, lines_b, margin)                              # (b)
