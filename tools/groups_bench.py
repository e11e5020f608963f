#!/usr/bin/env python3
"""The grouping calls (include/sliceslice_hip_groups.h) on the manual's text tiled to SIZE (default 1 GiB) and on generator bytes:
`RunPattern.groups` for `\\w+`, `[0-9]+` and `\\S+` and `group_lines` - wall time of the waiting call (median of 3 after a warm-up)
beside `find_all` of the same pattern alone and the plain-read ceiling; the share of the device time in each of the four steps
(hash, insert, count, rank and emit) from torch's profiler; the route a caller had before - `find_all`, both arrays to the host, a
Counter over slices - on the first 64 MiB; and the two extremes: one group (one byte repeated: `x+` tokens of equal length) and all
keys distinct.

    python tools/groups_bench.py [GIB=1] > profiles/groups/groups_bench_1gib.jsonl"""
import collections
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from fuzz_masked import _loaded  # noqa: E402

MiB = 1 << 20
STEPS = (("groups_hash_kernel", "hash"), ("groups_insert_kernel", "insert"), ("groups_count_kernel", "count"), ("groups_rank_kernel", "rank_emit"),
         ("groups_number_kernel", "rank_emit"), ("prefix_kernel", "rank_emit"))


def wall(fn, reps=3, warm=1):
    times, out = [], None
    for k in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warm:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def shares(fn):
    """the share of the device time of one call in each step, and in everything else (the tokenising scan, memsets, copies)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    by, total = collections.Counter(), 0.0
    for ev in prof.key_averages():
        t = float(getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0))
        total += t
        by[next((step for name, step in STEPS if name in ev.key), "tokenise_and_other")] += t
    return {k: round(v / total, 3) for k, v in by.items()} if total else {}


def measure(name, hay, group, find, ceiling_gbps):
    ms, rows = wall(group)
    row = {"case": name, "bytes": hay.numel(), "groups": int(rows[0].numel()), "keys": int(rows[-1].sum()), "groups_ms": round(ms, 3),
           "ceiling_ms": round(hay.numel() / (ceiling_gbps * 1e6), 3), "share_of_ceiling": round(hay.numel() / (ceiling_gbps * 1e6) / ms, 4)}
    if find is not None:
        find_ms, _ = wall(find)
        row.update(find_all_ms=round(find_ms, 3), groups_over_find_all=round(ms / find_ms, 2))
    try:
        row["device_time_shares"] = shares(group)
    except Exception as e:                                          # (the profiler is a convenience: the times above stand without it)
        row["device_time_shares"] = "profiler: %s" % e
    print(json.dumps(row), flush=True)


def main():
    gib = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    size = int(gib * 1024) * MiB
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(size // text.numel() + 1)[:size].contiguous()
    ceiling = ss.read_ceiling_gbps(hay)
    print(json.dumps({"device": ss.device_info(), "bytes": size, "read_ceiling_gbps": round(ceiling, 1)}), flush=True)
    # (SLICESLICE_HIP_LIB=<the groups library> is used as it is)
    with _loaded() if getattr(ss.lib(), "has_groups", False) else ss.groups_build():
        for text_pattern in (r"\w+", "[0-9]+", r"\S+"):
            pat = ss.RunPattern(text_pattern)
            measure("manual, " + text_pattern, hay, lambda: pat.groups(hay), lambda: pat.find_all(hay), ceiling)
        measure("manual, \\w+ folded", hay, lambda: ss.RunPattern(r"\w+").groups(hay, ignore_case=True), None, ceiling)
        measure("manual, lines", hay, lambda: ss.group_lines(hay), None, ceiling)
        # the route a caller had before, on the first 64 MiB
        small = hay[:64 * MiB]
        host = small.cpu().numpy().tobytes()
        pat = ss.RunPattern(r"\w+")
        t0 = time.perf_counter()
        begin, end = (x.cpu().tolist() for x in pat.find_all(small))
        want = collections.Counter(host[b:e] for b, e in zip(begin, end))
        old_ms = (time.perf_counter() - t0) * 1e3
        new_ms, rows = wall(lambda: pat.groups(small))
        assert [(host[b:e], c) for b, e, c in zip(*(x.cpu().tolist() for x in rows))] == list(want.items())
        print(json.dumps({"case": "host route at 64 MiB, \\w+", "old_route_ms": round(old_ms, 1), "groups_ms": round(new_ms, 3),
                          "groups_over_old_route": round(new_ms / old_ms, 6)}), flush=True)
        del want, begin, end
        # generator bytes: few tokens, long and all different
        rnd = torch.empty(size // 4, dtype=torch.uint8, device="cuda")
        ss.fill_random_device(rnd, 0x5EED0002)
        pat = ss.RunPattern(r"\w+")
        measure("generator bytes, \\w+, %d MiB" % (rnd.numel() // MiB), rnd, lambda: pat.groups(rnd), lambda: pat.find_all(rnd), ceiling)
        # one group: `x+` tokens of equal length, 64 MiB
        one = torch.from_numpy(np.frombuffer(b"xxxxxxx " * (8 * MiB), dtype=np.uint8).copy()).cuda()
        pat = ss.RunPattern("x+")
        measure("one group, x+ tokens of 7 bytes, 64 MiB", one, lambda: pat.groups(one), lambda: pat.find_all(one), ceiling)
        # all distinct: 8-digit numbers, each once, 72 MiB
        n = 8 * MiB
        digits = (np.arange(n, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1) % 10 + 48).astype(np.uint8)
        distinct = torch.from_numpy(np.concatenate((digits, np.full((n, 1), 10, np.uint8)), axis=1).reshape(-1)).cuda()
        pat = ss.RunPattern("[0-9]+")
        measure("all distinct, 8-digit tokens, 72 MiB", distinct, lambda: pat.groups(distinct), lambda: pat.find_all(distinct), ceiling)


if __name__ == "__main__":
    main()
