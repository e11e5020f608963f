#!/usr/bin/env python3
"""What the masked-pattern calls (include/sliceslice_hip_masked.h) cost, one JSON line per row:
    python tools/masked_bench.py [--gib 1] [--reps 5] > profiles/masked/masked_bench_1gib.jsonl

On --gib of the manual's text (tiled) and of generator bytes (fill_random_device), hipEvents around stream-ordered counts
(`count_async`), medians of --reps after one warm-up call:
  * `count` of an all-FF pattern (`descriptor`) against the searcher's `count` of the same needle - where the masked kernel LOSES to
    the exact scan for a pattern without wildcards;
  * `count` of `d?scr??tor` and `t?e`;
  * `count` of a nibble-only pattern (`3? 3? 3?`) and of `??`, the worst case: every position is a candidate;
  * `count` of the letter-mask pattern of `intel` against the searcher's `count(ignore_case=True)`;
  * `find_all` with room for everything (a host clock around the waiting call);
  * the host route a caller had before for `t?e` (find_all of `t`, every offset to the host, the numpy check), once;
  * the count's device time as a share of the plain-read ceiling (ss_read_ceiling)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sliceslice_rs_amd as ss  # noqa: E402


def events_ms(fn, reps):
    """median device time of the stream-ordered call `fn` between two events"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def wall_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def rows(name, hay, reps, host_route):
    size = hay.numel()
    ceiling = ss.read_ceiling_gbps(hay)
    out = torch.zeros(1, dtype=torch.int64, device="cuda")

    def row(what, pat, model=None, model_kw=None):
        ms = events_ms(lambda: pat.count_async(hay, out), reps)
        count = int(out.cpu()[0])
        r = {"haystack": name, "bytes": size, "pattern": what, "info": pat.info(), "count": count, "count_ms": round(ms, 3),
             "count_gbps": round(size / ms / 1e6, 1), "read_ceiling_gbps": round(ceiling, 1), "share_of_read_ceiling": round(size / ms / 1e6 / ceiling, 3)}
        if model is not None:
            kw = model_kw or {}
            theirs = torch.zeros(1, dtype=torch.int64, device="cuda")
            r["searcher_count_ms"] = round(events_ms(lambda: model.count_async(hay, theirs, **kw), reps), 3)
            assert int(theirs.cpu()[0]) == count, (what, int(theirs.cpu()[0]), count)
            r["masked_over_searcher"] = round(ms / r["searcher_count_ms"], 2)
        if count <= 1 << 28:
            room = torch.empty(max(count, 1), dtype=torch.int64, device="cuda")
            assert pat.find_all_into(hay, room, count) == count
            r["find_all_ms"] = round(wall_ms(lambda: pat.find_all_into(hay, room, count), reps), 3)
            r["count_wall_ms"] = round(wall_ms(lambda: pat.count(hay), reps), 3)
            del room
        print(json.dumps(r), flush=True)
        return count

    row("descriptor (all FF)", ss.MaskedPattern(b"descriptor"), ss.DynamicHipSearcher(b"descriptor"))
    row("d?scr??tor", ss.MaskedPattern.from_hex("64 ?? 73 63 72 ?? ?? 74 6f 72"))
    t_any_e = ss.MaskedPattern.from_hex("74 ?? 65")
    want = row("t?e", t_any_e)
    row("3? 3? 3? (nibbles only)", ss.MaskedPattern.from_hex("3? 3? 3?"))
    row("?? (every position)", ss.MaskedPattern.from_hex("??"))
    row("intel (letter masks)", ss.MaskedPattern.from_bytes(b"intel", ignore_case=True), ss.DynamicHipSearcher(b"intel"), {"ignore_case": True})
    if host_route:
        t_alone = ss.DynamicHipSearcher(b"t")
        host = hay.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        offsets = t_alone.find_all(hay).cpu().numpy()
        offsets = offsets[offsets + 2 < size]
        got = int((host[offsets + 2] == ord("e")).sum())
        ms = (time.perf_counter() - t0) * 1e3
        assert got == want, (got, want)
        print(json.dumps({"haystack": name, "bytes": size, "pattern": "t?e", "host_route_ms": round(ms, 1), "literal_offsets": int(offsets.size),
                          "host_route_over_masked_count_wall": round(ms / wall_ms(lambda: t_any_e.count(hay), reps), 1)}), flush=True)


class _loaded:
    """the library SLICESLICE_HIP_LIB loaded, where it has the entry points"""
    def __enter__(self):
        return ss.lib()

    def __exit__(self, *a):
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    size = int(a.gib * (1 << 30))
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    ctx = _loaded() if getattr(ss.lib(), "has_masked", False) else ss.masked_build()
    with ctx:
        hay = torch.from_numpy(manual).cuda().repeat(size // manual.size + 1)[:size].contiguous()
        rows("manual", hay, a.reps, True)
        ss.fill_random_device(hay, 0x5EED0001)
        rows("generator", hay, a.reps, False)


if __name__ == "__main__":
    main()
