#!/usr/bin/env python3
"""./context_bench.py [--gib 1] [--reps 15] - rates of the context calls (libsliceslice_hip_context.so), a measurement aid: one JSON
line per row, medians of `reps`.  The manual's text tiled to the size asked for.
  census    lines_around of one number with capacity 0 - the delimiter census and its prefix - beside the plain-read ceiling of
            libsliceslice_hip_tools.so on the same buffer and beside count_lines of the empty needle (the byte-wise pass)
  context   find_lines_context_into with room for every output line against its model's find_lines_into, for `descriptor`, `the`
            and a needle that does not occur, before = after in {0, 2, 100}; the share of the parts that the select pass reads
            again (those that hold an end or a beginning of an output line), worked out from the records; and, once per needle, the
            route a caller had before: find_lines, find_lines of the empty needle, both record sets to the host, a numpy index."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from lines_bench import wall_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def old_route(s, every, hay, amount):
    hit = [t.cpu().numpy() for t in s.find_lines(hay)]
    lines = [t.cpu().numpy() for t in every.find_lines(hay)]
    n = lines[2].size
    if hit[2].size == 0:
        return 0
    edge = np.zeros(n + 2, dtype=np.int64)
    np.add.at(edge, np.maximum(1, hit[2] - amount), 1)
    np.add.at(edge, np.minimum(n, hit[2] + amount) + 1, -1)
    numbers = np.flatnonzero(np.cumsum(edge)[:n + 1] > 0)
    return int(lines[0][numbers - 1].size + lines[1][numbers - 1].size) // 2


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 15
    n_bytes = int(gib * (1 << 30))
    P = ss.CONTEXT_PART_BYTES
    parts = (n_bytes + P - 1) // P
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(n_bytes // text.numel() + 1)[:n_bytes].contiguous()
    with ss.context_build():
        every = ss.DynamicHipSearcher(b"")
    one = torch.ones(1, dtype=torch.int64, device="cuda")
    census = wall_ms(lambda: every.lines_around_into(hay, one, None, None, None, None, 0), reps)
    count = wall_ms(lambda: every.count_lines(hay), reps)
    lines = every.count_lines(hay)
    print(json.dumps({"row": "census", "gib": gib, "lines": lines, "parts": parts, "census_ms": round(census, 4),
                      "census_gb_per_s": round(n_bytes / census / 1e6, 1), "read_ceiling_gb_per_s": round(ss.read_ceiling_gbps(hay), 1),
                      "empty_needle_count_lines_ms": round(count, 4), "count_lines_over_census": round(count / census, 2)}), flush=True)
    for needle in (b"descriptor", b"the", b"no such phrase in the manual"):
        with ss.context_build():
            s = ss.DynamicHipSearcher(needle)
        selected = s.count_lines(hay)
        cap = max(selected, 1)
        model_bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)]
        model = wall_ms(lambda: s.find_lines_into(hay, model_bufs[0], model_bufs[1], model_bufs[2], cap), reps)
        for amount in (0, 2, 100):
            total, _ = s.find_lines_context_into(hay, None, None, None, None, 0, amount, amount)
            cap = max(total, 1)
            bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)] + [torch.empty(cap, dtype=torch.uint8, device="cuda")]
            ms = wall_ms(lambda: s.find_lines_context_into(hay, bufs[0], bufs[1], bufs[2], bufs[3], cap, amount, amount), reps)
            row = {"row": "context", "gib": gib, "needle": needle.decode(), "before_after": amount, "selected": selected, "printed": total,
                   "find_lines_context_ms": round(ms, 4), "model_find_lines_ms": round(model, 4), "context_over_model": round(ms / model, 3)}
            if total:
                touched = torch.unique(torch.cat((bufs[1][:total] // P, (bufs[0][:total][bufs[0][:total] > 0] - 1) // P)))
                row["parts_read_again_share"] = round(float(touched[touched < parts].numel()) / parts, 4)
            else:
                row["parts_read_again_share"] = 0.0
            if amount == 2:
                t0 = time.perf_counter()
                assert old_route(s, every, hay, amount) == total, row
                row["old_route_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                row["old_route_over_find_lines_context"] = round(row["old_route_ms"] / ms, 1)
            del bufs
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
