#!/usr/bin/env python3
"""What the byte-class calls (include/sliceslice_hip_classes.h) cost, one JSON line per row:
    python tools/classes_bench.py [--gib 1] [--reps 5] > profiles/classes/classes_bench_1gib.jsonl

On --gib of the manual's text (tiled) and of generator bytes (fill_random_device), hipEvents around stream-ordered counts
(`count_async`), medians of --reps after one warm-up call, beside the plain-read ceiling (ss_read_ceiling):
  * `[0-9A-F]{4}H` and `\\d\\d:\\d\\d`;
  * `[0-9]{3}` beside `3? 3? 3?` masked - the superset a caller had before;
  * `[^a-z]the[^a-z]` beside the searcher's `count(whole_word=True)` of `the` (a different rule: the word form also matches at the
    ends of the view and takes digits and `_` as word bytes, so the counts differ and both are printed);
  * the two WIDE cases, `\\w{8}` and `[0-9A-F]{4}`: their covers accept 128 values, every ASCII position is a candidate that is
    settled byte by byte, and this is where the class kernel loses."""
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


def rows(name, hay, reps):
    size = hay.numel()
    ceiling = ss.read_ceiling_gbps(hay)
    out = torch.zeros(1, dtype=torch.int64, device="cuda")

    def row(what, pat, beside=None, beside_name=None, beside_kw=None):
        ms = events_ms(lambda: pat.count_async(hay, out), reps)
        count = int(out.cpu()[0])
        r = {"haystack": name, "bytes": size, "pattern": what, "info": pat.info(), "count": count, "count_ms": round(ms, 3),
             "count_gbps": round(size / ms / 1e6, 1), "read_ceiling_gbps": round(ceiling, 1), "share_of_read_ceiling": round(size / ms / 1e6 / ceiling, 3)}
        if beside is not None:
            theirs = torch.zeros(1, dtype=torch.int64, device="cuda")
            r[beside_name + "_count_ms"] = round(events_ms(lambda: beside.count_async(hay, theirs, **(beside_kw or {})), reps), 3)
            r[beside_name + "_count"] = int(theirs.cpu()[0])
            r["classes_over_" + beside_name] = round(ms / r[beside_name + "_count_ms"], 2)
        r["count_wall_ms"] = round(wall_ms(lambda: pat.count(hay), reps), 3)
        print(json.dumps(r), flush=True)

    row(r"[0-9A-F]{4}H", ss.ClassPattern(r"[0-9A-F]{4}H"))
    row(r"\d\d:\d\d", ss.ClassPattern(r"\d\d:\d\d"))
    row(r"[0-9]{3}", ss.ClassPattern(r"[0-9]{3}"), ss.MaskedPattern.from_hex("3? 3? 3?"), "masked_nibbles")
    row(r"[^a-z]the[^a-z]", ss.ClassPattern(r"[^a-z]the[^a-z]"), ss.DynamicHipSearcher(b"the"), "whole_word_searcher", {"whole_word": True})
    row(r"\w{8} (wide)", ss.ClassPattern(r"\w{8}"))
    row(r"[0-9A-F]{4} (wide)", ss.ClassPattern(r"[0-9A-F]{4}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    size = int(a.gib * (1 << 30))
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    ctx = _loaded() if getattr(ss.lib(), "has_classes", False) else ss.classes_build()
    with ctx:
        hay = torch.from_numpy(manual).cuda().repeat(size // manual.size + 1)[:size].contiguous()
        rows("manual", hay, a.reps)
        ss.fill_random_device(hay, 0x5EED0001)
        rows("generator", hay, a.reps)


if __name__ == "__main__":
    main()
