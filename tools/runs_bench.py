#!/usr/bin/env python3
"""What the run calls (include/sliceslice_hip_runs.h) cost, one JSON line per row:
    python tools/runs_bench.py [--gib 1] [--reps 5] > profiles/runs/runs_bench_1gib.jsonl

On --gib of the manual's text (tiled) and of generator bytes (fill_random_device), hipEvents around stream-ordered counts
(`count_async`), medians of --reps after one warm-up call, beside the plain-read ceiling (ss_read_ceiling):
  * `\\w+`, `\\S+`, `[0-9]+` - min_len 1 and no maximum: a popcount, no byte is read twice;
  * `[0-9]{3,}`, `\\w{8,}`, `[A-Z]{2,5}`, ` {2,}` - settled in the 32-bit window, a few walks;
  * `[^\\n]{80,}` - the walk's bad case: every line longer than the window walks up to 80 bytes of memory;
  * every set again FORCED to the bitmap path (sixteen LDS reads per lane instead of the range arithmetic);
  * `find_all` with room for everything (wall time: count pass, two prefix sums, emit pass, the wait);
  * `\\w{8,}` beside ClassPattern(r"\\w{8}").count of the same build (a different question - every position, not every run - and
    the route a caller had before);
  * `[^\\n]+` beside the context library's delimiter census (lines_around with capacity 0), which reads the same bytes for the
    same delimiters."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from masked_bench import _loaded, events_ms, wall_ms  # noqa: E402

PATTERNS = [r"\w+", r"\S+", r"[0-9]+", r"[0-9]{3,}", r"\w{8,}", r"[A-Z]{2,5}", r" {2,}", r"[^\n]{80,}"]


def rows(name, hay, reps):
    size = hay.numel()
    ceiling = ss.read_ceiling_gbps(hay)
    out = torch.zeros(1, dtype=torch.int64, device="cuda")

    def timed(pat):
        ms = events_ms(lambda: pat.count_async(hay, out), reps)
        return ms, int(out.cpu()[0])

    for text in PATTERNS:
        words, lo, hi = ss.parse_runs(text)
        ranged, bitmap = ss.RunPattern.from_set(words, lo, hi), ss.RunPattern.from_set(words, lo, hi, bitmap=True)
        ms, count = timed(ranged)
        bms, bcount = timed(bitmap)
        assert count == bcount
        r = {"haystack": name, "bytes": size, "pattern": text, "info": ranged.info(), "count": count, "count_ms": round(ms, 3),
             "count_gbps": round(size / ms / 1e6, 1), "read_ceiling_gbps": round(ceiling, 1), "share_of_read_ceiling": round(size / ms / 1e6 / ceiling, 3),
             "bitmap_count_ms": round(bms, 3), "bitmap_share_of_read_ceiling": round(size / bms / 1e6 / ceiling, 3),
             "count_wall_ms": round(wall_ms(lambda: ranged.count(hay), reps), 3)}
        if count * 16 <= 6 << 30:
            begin = torch.empty(max(count, 1), dtype=torch.int64, device="cuda")
            end = torch.empty(max(count, 1), dtype=torch.int64, device="cuda")
            r["find_all_wall_ms"] = round(wall_ms(lambda: ranged.find_all_into(hay, begin, end, count), reps), 3)
            del begin, end
        if text == r"\w{8,}":
            eight = ss.ClassPattern(r"\w{8}")
            theirs = torch.zeros(1, dtype=torch.int64, device="cuda")
            r["class_w8_count_ms"] = round(events_ms(lambda: eight.count_async(hay, theirs), reps), 3)
            r["class_w8_count"] = int(theirs.cpu()[0])
            r["class_w8_over_runs"] = round(r["class_w8_count_ms"] / ms, 2)
        print(json.dumps(r), flush=True)
    lines = ss.RunPattern(r"[^\n]+")
    ms, count = timed(lines)
    every = ss.DynamicHipSearcher(b"")
    one = torch.ones(1, dtype=torch.int64, device="cuda")
    census = wall_ms(lambda: every.lines_around_into(hay, one, None, None, None, None, 0), reps)
    print(json.dumps({"haystack": name, "bytes": size, "pattern": r"[^\n]+", "count": count, "count_ms": round(ms, 3),
                      "count_wall_ms": round(wall_ms(lambda: lines.count(hay), reps), 3), "share_of_read_ceiling": round(size / ms / 1e6 / ceiling, 3),
                      "census_wall_ms": round(census, 3), "read_ceiling_gbps": round(ceiling, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    size = int(a.gib * (1 << 30))
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    ctx = _loaded() if getattr(ss.lib(), "has_runs", False) else ss.runs_build()
    with ctx:
        hay = torch.from_numpy(manual).cuda().repeat(size // manual.size + 1)[:size].contiguous()
        rows("manual", hay, a.reps)
        ss.fill_random_device(hay, 0x5EED0001)
        rows("generator", hay, a.reps)


if __name__ == "__main__":
    main()
