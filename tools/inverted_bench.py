#!/usr/bin/env python3
"""./inverted_bench.py [--gib 1] [--reps 15] - rates of the inverted line calls (libsliceslice_hip_inverted.so) against their
non-inverted models of the SAME build and buffer, and against the route a caller had before them - find_lines for the matching
lines, find_lines with the empty needle for all lines, both record sets copied to the host, a numpy set difference - a measurement
aid: one JSON line per (haystack, needle).  hipEvent pairs around the stream-ordered calls, wall clock around the blocking ones;
medians.  Haystacks: the manual's text tiled, and generator bytes (a `the`-like needle that does not occur)."""
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


def old_route(s, every, hay):
    hit = [t.cpu().numpy() for t in s.find_lines(hay)]
    lines = [t.cpu().numpy() for t in every.find_lines(hay)]
    keep = ~np.isin(lines[2], hit[2], assume_unique=True)
    return int(np.count_nonzero(keep))


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 15
    n_bytes = int(gib * (1 << 30))
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    d = torch.zeros(8, dtype=torch.int64, device="cuda")
    cap = 1 << 20
    bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)]
    with ss.inverted_build():
        every = ss.DynamicHipSearcher(b"")
    for kind, needles in (("text", [b"descriptor", b"the", b"e", b"no such phrase"]), ("random", [b"the", b"a needle of 16 b"])):
        if kind == "text":
            hay.copy_(text.repeat(n_bytes // text.numel() + 1)[:n_bytes])
        else:
            ss.fill_random_device(hay, 0x11E5)
            hay.masked_fill_(hay == ord("t"), ord("u"))
            hay.masked_fill_(hay == ord("T"), ord("u"))
        for needle in needles:
            with ss.inverted_build():
                s = ss.DynamicHipSearcher(needle)
            row = {"haystack": kind, "gib": gib, "needle": needle.decode("latin-1"), "lines": every.count_lines(hay)}
            for tag, kw in (("", {}), ("_word", dict(whole_word=True)), ("_nocase", dict(ignore_case=True))):
                row["count_lines" + tag] = s.count_lines(hay, **kw)
                row["count_lines_inverted" + tag] = s.count_lines_inverted(hay, **kw)
                assert row["count_lines" + tag] + row["count_lines_inverted" + tag] == row["lines"], row
                a = event_ms(lambda: s.count_lines_async(hay, d[0:1], **kw), reps)
                b = event_ms(lambda: s.count_lines_inverted_async(hay, d[1:2], **kw), reps)
                row["count_lines%s_ms" % tag], row["count_lines_inverted%s_ms" % tag] = round(a, 4), round(b, 4)
                row["count_lines%s_over_inverted" % tag] = round(a / b, 4)
                row["count_lines_inverted%s_gb_per_s" % tag] = round(n_bytes / b / 1e6, 1)
            a = wall_ms(lambda: s.find_lines_into(hay, bufs[0], bufs[1], bufs[2], cap), reps)
            b = wall_ms(lambda: s.find_lines_inverted_into(hay, bufs[0], bufs[1], bufs[2], cap), reps)
            row["find_lines_cap_1m_ms"], row["find_lines_inverted_cap_1m_ms"] = round(a, 4), round(b, 4)
            row["find_lines_inverted_over_find_lines_cap_1m"] = round(b / a, 3)
            t0 = time.perf_counter()
            b, e, n = s.find_lines_inverted(hay)
            torch.cuda.synchronize()
            row["find_lines_inverted_all_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            del b, e, n
            t0 = time.perf_counter()
            assert old_route(s, every, hay) == row["count_lines_inverted"], row
            row["old_route_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            row["old_route_over_find_lines_inverted_all"] = round(row["old_route_ms"] / row["find_lines_inverted_all_ms"], 2)
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
