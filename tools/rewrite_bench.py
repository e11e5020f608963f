#!/usr/bin/env python3
"""What the rewrite call (include/sliceslice_hip_rewrite.h) costs, one JSON line per row:
    python tools/rewrite_bench.py [--gib 1] [--reps 5] > profiles/rewrite/rewrite_bench_1gib.jsonl

On --gib of the manual's text (tiled), medians of --reps after one warm-up call.  The call waits for its stream twice (the sizes come
back before the write pass is launched), so its time is wall time around the call; the time between two events on the stream is
beside it.  Per row:
  * `\\r+` deleted (`tr -d '\\r'` on text that holds none: no member, a pure copy), ` {2,}` -> ` `, `[0-9]+` -> `N`, `\\s+` -> ` `
    per line (delimiter `\\n`), `\\w+` deleted, `[^\\n]{80,}` -> `...`;
  * the sizing call alone (NULL output: one pass and three prefix sums);
  * the output rate, beside the plain-read ceiling (ss_read_ceiling) and a `copy_` of as many bytes as the output holds;
  * the share of lanes that keep all 16 of their bytes and begin no run (ONE 16-byte store), counted on the host over the first
    8 MiB, the view 16-byte aligned as torch allocates it;
  * the route a caller had before in the same build - find_all, the complementary ranges by torch, gather_ranges with the text as
    terminator where it is one byte (none where it is empty), the last one trimmed - and, on the first 64 MiB, the host's route:
    copy to the host, `re.sub`, copy back."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from masked_bench import _loaded, events_ms, wall_ms  # noqa: E402

# (pattern, text, delimiter)
ROWS = [(r"\r+", b"", None), (r" {2,}", b" ", None), (r"[0-9]+", b"N", None), (r"\s+", b" ", 10), (r"\w+", b"", None), (r"[^\n]{80,}", b"...", None)]
HOST_BYTES = 64 << 20
SHARE_BYTES = 8 << 20


def plain_lane_share(host, words, lo, hi, delimiter):
    """the share of 16-byte lanes that keep every byte and begin no run"""
    row = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little").astype(bool)
    if delimiter is not None:
        row[delimiter] = False
    d = np.diff(np.concatenate([[False], row[host], [False]]).astype(np.int8))
    begin, end = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    keep = (end - begin >= lo) & ((end - begin <= hi) if hi else True)
    removed = np.zeros(host.size + 1, dtype=np.int32)
    np.add.at(removed, begin[keep], 1)
    np.add.at(removed, end[keep], -1)
    inside = np.cumsum(removed[:-1]) > 0
    lanes = inside[:host.size // 16 * 16].reshape(-1, 16)
    return float((~lanes.any(axis=1)).mean())


def old_route(pat, hay, text):
    begin, end = pat.find_all(hay)
    kept_begin = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), end])
    kept_end = torch.cat([begin, torch.full((1,), hay.numel(), dtype=torch.int64, device="cuda")])
    out = ss.gather_ranges(hay, kept_begin, kept_end, text or None)
    return out[:out.numel() - len(text)]


def rows(name, hay, reps):
    size = hay.numel()
    ceiling = ss.read_ceiling_gbps(hay)
    for pattern, text, delimiter in ROWS:
        words, lo, hi = ss.parse_runs(pattern)
        pat = ss.RunPattern.from_set(words, lo, hi)
        out_len, count = pat.replace_into(hay, text, None, delimiter)
        out = torch.empty(max(out_len, 1), dtype=torch.uint8, device="cuda")
        ms = wall_ms(lambda: pat.replace_into(hay, text, out[:out_len], delimiter), reps)
        copy_ms = events_ms(lambda: out[:out_len].copy_(hay[:out_len]), reps)
        r = {"haystack": name, "bytes": size, "pattern": pattern, "text": text.decode("latin-1"), "delimiter": delimiter, "info": pat.info(),
             "count": count, "out_len": out_len, "replace_wall_ms": round(ms, 3),
             "replace_events_ms": round(events_ms(lambda: pat.replace_into(hay, text, out[:out_len], delimiter), reps), 3),
             "size_wall_ms": round(wall_ms(lambda: pat.replace_into(hay, text, None, delimiter), reps), 3),
             "read_gbps": round(size / ms / 1e6, 1), "out_gbps": round(out_len / ms / 1e6, 1), "read_ceiling_gbps": round(ceiling, 1),
             "share_of_read_ceiling": round(size / ms / 1e6 / ceiling, 3), "copy_of_out_bytes_ms": round(copy_ms, 3),
             "replace_over_copy": round(ms / copy_ms, 2), "count_wall_ms": round(wall_ms(lambda: pat.count(hay), reps), 3),
             "plain_lane_share": round(plain_lane_share(hay[:SHARE_BYTES].cpu().numpy(), words, lo, hi, delimiter), 4)}
        if delimiter is None and len(text) <= 1 and count * 16 <= 8 << 30:
            got = old_route(pat, hay, text)
            assert torch.equal(got, out[:out_len])
            del got
            r["old_route_wall_ms"] = round(wall_ms(lambda: old_route(pat, hay, text), max(reps // 2, 1)), 3)
            r["old_over_new"] = round(r["old_route_wall_ms"] / ms, 2)
        part = hay[:min(HOST_BYTES, size)]
        rx = re.compile(pattern.encode("latin-1"), re.S)
        t0 = time.perf_counter()
        data = part.cpu().numpy().tobytes()
        if delimiter is None:
            done = rx.sub(lambda m: text, data)
        else:
            item = pattern[:-1].encode("latin-1")
            done = re.sub(b"(?:(?!\\n)" + item + b")+", lambda m: text, data, flags=re.S)
        back = torch.frombuffer(bytearray(done), dtype=torch.uint8).cuda() if done else None
        torch.cuda.synchronize()
        r["host_route_bytes"] = part.numel()
        r["host_route_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        del back
        print(json.dumps(r), flush=True)
        del out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    size = int(a.gib * (1 << 30))
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    ctx = _loaded() if getattr(ss.lib(), "has_rewrite", False) else ss.rewrite_build()
    with ctx:
        hay = torch.from_numpy(manual).cuda().repeat(size // manual.size + 1)[:size].contiguous()
        rows("manual", hay, a.reps)


if __name__ == "__main__":
    main()
