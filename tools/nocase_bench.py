#!/usr/bin/env python3
"""./nocase_bench.py [--gib 1] [--reps 15] - rates of the calls that ignore ASCII case (libsliceslice_hip_nocase.so) against their
case-sensitive models of the SAME build and against the route a caller had before them - lower-case the haystack into a second
buffer with torch, then count on the copy - a measurement aid: one JSON line per (haystack, needle).  hipEvent pairs around the
stream-ordered calls; medians.  Haystacks: the manual's text tiled, and generator bytes (a `the`-like needle that does not occur)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from lines_bench import event_ms, wall_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fold_copy(hay, out):
    """the cheapest torch expression found for lower-casing into a second buffer: out = hay | ((hay - 'A' < 26) << 5), in uint8
    wrap-around arithmetic (tests/test_gpu_zz_nocase_timing.py measures it against a table gather and takes the faster)"""
    torch.bitwise_or(hay, ((hay - 65) < 26).to(torch.uint8) << 5, out=out)


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 15
    n_bytes = int(gib * (1 << 30))
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    low = torch.empty_like(hay)
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    for kind, needles in (("text", [b"descriptor", b"the", b"e", b"no such phrase"]), ("random", [b"the", b"a needle of 16 b"])):
        if kind == "text":
            hay.copy_(text.repeat(n_bytes // text.numel() + 1)[:n_bytes])
        else:
            ss.fill_random_device(hay, 0x11E5)
            hay.masked_fill_(hay == ord("t"), ord("u"))
            hay.masked_fill_(hay == ord("T"), ord("u"))
        fold_ms = round(event_ms(lambda: fold_copy(hay, low), max(3, reps // 3)), 4)
        for needle in needles:
            with ss.nocase_build():
                s = ss.DynamicHipSearcher.new_nocase(needle)
            row = {"haystack": kind, "gib": gib, "needle": needle.decode("latin-1"), "count": s.count(hay),
                   "count_nocase": s.count(hay, ignore_case=True), "count_lines": s.count_lines(hay),
                   "count_lines_nocase": s.count_lines(hay, ignore_case=True)}
            assert row["count_nocase"] == s.count(low), row
            row["count_ms"] = round(event_ms(lambda: s.count_async(hay, d[0:1]), reps), 4)
            row["count_nocase_ms"] = round(event_ms(lambda: s.count_async(hay, d[1:2], ignore_case=True), reps), 4)
            row["count_lines_ms"] = round(event_ms(lambda: s.count_lines_async(hay, d[2:3]), reps), 4)
            row["count_lines_nocase_ms"] = round(event_ms(lambda: s.count_lines_async(hay, d[3:4], ignore_case=True), reps), 4)
            row["torch_fold_copy_ms"] = fold_ms
            row["fold_copy_then_count_ms"] = round(event_ms(lambda: (fold_copy(hay, low), s.count_async(low, d[0:1])), max(3, reps // 3)), 4)
            for k in ("count", "count_nocase", "count_lines", "count_lines_nocase"):
                row[k + "_gb_per_s"] = round(n_bytes / row[k + "_ms"] / 1e6, 1)
            cap = 1 << 20
            out = torch.empty(cap, dtype=torch.int64, device="cuda")
            row["find_all_cap_1m_ms"] = round(wall_ms(lambda: s.find_all_into(hay, out), reps), 4)
            row["find_all_nocase_cap_1m_ms"] = round(wall_ms(lambda: s.find_all_into(hay, out, ignore_case=True), reps), 4)
            bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)]
            row["find_lines_nocase_cap_1m_ms"] = round(wall_ms(lambda: s.find_lines_into(hay, bufs[0], bufs[1], bufs[2], cap, ignore_case=True), reps), 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
