#!/usr/bin/env python3
"""./lines_bench.py [--gib 1] [--reps 15] - rates of the matching-lines calls (libsliceslice_hip_lines.so) against count / find_all
of the SAME build, a measurement aid: one JSON line per (haystack, needle).  hipEvent pairs around the stream-ordered counts, wall
time of the synchronous find calls; medians.  Haystacks: the manual's text tiled, and generator bytes (a `the`-like needle that
does not occur; a newline every 256 bytes on average)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sliceslice_rs_amd as ss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for k in range(reps + 2):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= 2:
            out.append(a.elapsed_time(b))
    return float(np.median(out))


def wall_ms(fn, reps):
    out = []
    for k in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 15
    n_bytes = int(gib * (1 << 30))
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    d = torch.zeros(2, dtype=torch.int64, device="cuda")
    for kind, needles in (("text", [b"descriptor", b"the", b"e", b"no such phrase", b""]), ("random", [b"the", b"\x00", b"a needle of 16 b"])):
        if kind == "text":
            hay.copy_(text.repeat(n_bytes // text.numel() + 1)[:n_bytes])
        else:
            ss.fill_random_device(hay, 0x11E5)
            hay.masked_fill_(hay == ord("t"), ord("u"))
        for needle in needles:
            with ss.lines_build():
                s = ss.DynamicHipSearcher(needle)
            row = {"haystack": kind, "gib": gib, "needle": needle.decode("latin-1"), "count": s.count(hay), "count_lines": s.count_lines(hay)}
            row["count_ms"] = round(event_ms(lambda: s.count_async(hay, d[0:1]), reps), 4)
            row["count_lines_ms"] = round(event_ms(lambda: s.count_lines_async(hay, d[1:2]), reps), 4)
            row["count_gb_per_s"] = round(n_bytes / row["count_ms"] / 1e6, 1)
            row["count_lines_gb_per_s"] = round(n_bytes / row["count_lines_ms"] / 1e6, 1)
            cap = 1 << 20
            if needle:
                out = torch.empty(cap, dtype=torch.int64, device="cuda")
                row["find_all_cap_1m_ms"] = round(wall_ms(lambda: s.find_all_into(hay, out), reps), 4)
            bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)]
            row["find_lines_cap_1m_ms"] = round(wall_ms(lambda: s.find_lines_into(hay, bufs[0], bufs[1], bufs[2], cap), reps), 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
