#!/usr/bin/env python3
"""./bounded_bench.py [--gib 1] [--reps 15] - rates of the whole-word / whole-line calls (libsliceslice_hip_bounded.so) against
their unbounded models of the SAME build and against the route a caller had before them - find_all into a device array sized by
count, a copy of every offset to the host, the rule applied there with numpy - a measurement aid: one JSON line per (haystack,
needle).  hipEvent pairs around the stream-ordered calls, wall clock around the blocking ones; medians.  Haystacks: the manual's
text tiled, and generator bytes (a `the`-like needle that does not occur)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from lines_bench import event_ms, wall_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD = np.zeros(256, dtype=bool)
WORD[list(b"0123456789_") + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B))] = True


def old_route(s, hay, host):
    """whole-word occurrences the way a caller counted them before: every offset to the host, the neighbour test there"""
    offs = s.find_all(hay).cpu().numpy()
    n, L = len(s.needle), host.size
    left = np.where(offs > 0, host[np.maximum(offs - 1, 0)], 0x20)
    right = np.where(offs + n < L, host[np.minimum(offs + n, L - 1)], 0x20)
    return int(np.count_nonzero(~WORD[left] & ~WORD[right]))


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 15
    n_bytes = int(gib * (1 << 30))
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    d = torch.zeros(6, dtype=torch.int64, device="cuda")
    for kind, needles in (("text", [b"descriptor", b"the", b"e", b"no such phrase"]), ("random", [b"the", b"a needle of 16 b"])):
        if kind == "text":
            hay.copy_(text.repeat(n_bytes // text.numel() + 1)[:n_bytes])
        else:
            ss.fill_random_device(hay, 0x11E5)
            hay.masked_fill_(hay == ord("t"), ord("u"))
            hay.masked_fill_(hay == ord("T"), ord("u"))
        host = hay.cpu().numpy()
        for needle in needles:
            with ss.bounded_build():
                s = ss.DynamicHipSearcher(needle)
            row = {"haystack": kind, "gib": gib, "needle": needle.decode("latin-1"), "count": s.count(hay),
                   "count_word": s.count(hay, whole_word=True), "count_word_nocase": s.count(hay, ignore_case=True, whole_word=True),
                   "count_lines": s.count_lines(hay), "count_lines_word": s.count_lines(hay, whole_word=True),
                   "count_lines_line": s.count_lines(hay, whole_line=True)}
            row["count_ms"] = round(event_ms(lambda: s.count_async(hay, d[0:1]), reps), 4)
            row["count_word_ms"] = round(event_ms(lambda: s.count_async(hay, d[1:2], whole_word=True), reps), 4)
            row["count_nocase_ms"] = round(event_ms(lambda: s.count_async(hay, d[4:5], ignore_case=True), reps), 4)
            row["count_word_nocase_ms"] = round(event_ms(lambda: s.count_async(hay, d[5:6], ignore_case=True, whole_word=True), reps), 4)
            row["count_lines_ms"] = round(event_ms(lambda: s.count_lines_async(hay, d[2:3]), reps), 4)
            row["count_lines_word_ms"] = round(event_ms(lambda: s.count_lines_async(hay, d[3:4], whole_word=True), reps), 4)
            row["count_lines_line_ms"] = round(event_ms(lambda: s.count_lines_async(hay, d[3:4], whole_line=True), reps), 4)
            for k in ("count", "count_word", "count_word_nocase", "count_lines", "count_lines_word", "count_lines_line"):
                row[k + "_gb_per_s"] = round(n_bytes / row[k + "_ms"] / 1e6, 1)
            t0 = time.perf_counter()
            assert old_route(s, hay, host) == row["count_word"], row
            row["old_route_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            row["count_word_blocking_ms"] = round(wall_ms(lambda: s.count(hay, whole_word=True), reps), 4)
            cap = 1 << 20
            out = torch.empty(cap, dtype=torch.int64, device="cuda")
            row["find_all_cap_1m_ms"] = round(wall_ms(lambda: s.find_all_into(hay, out), reps), 4)
            row["find_all_word_cap_1m_ms"] = round(wall_ms(lambda: s.find_all_into(hay, out, whole_word=True), reps), 4)
            bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)]
            row["find_lines_word_cap_1m_ms"] = round(wall_ms(lambda: s.find_lines_into(hay, bufs[0], bufs[1], bufs[2], cap, whole_word=True), reps), 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
