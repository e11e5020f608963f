#!/usr/bin/env python3
"""./disjoint_bench.py [--gib 1] [--reps 5] - rates of the non-overlapping calls (libsliceslice_hip_disjoint.so), a measurement aid:
one JSON line per row, medians of `reps`.  Three haystacks: the manual's text tiled to the size asked for (needles: two spaces,
which overlap themselves, and `the`, which cannot), the generator's bytes of the same size (ss.fill_random_device) with an absent
needle, and a quarter of that size of one repeated byte with `aa` - every block of the selection without a head, its worst case,
which needs 16 bytes of temporary device memory per overlapping occurrence (8 for the list, 8 for the selection's records).
Per row:
  count / find_all   count_disjoint and find_all_disjoint_into against the model `count` / `find_all_into` of the same build
  host route         the route a caller had before: find_all, the offsets to the host, the greedy walk in numpy
  replace            replace (same length, so the output has the haystack's size) against bytes.replace on the host including both
                     copies, and its device time by stream events as a rate beside the plain-read ceiling (ss.read_ceiling_gbps)
  selection          the share of find_all_disjoint_into spent in ss_select_disjoint_device (timed alone on the overlapping list)
Rows are printed as they come, those where the new call loses included."""
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
from needleset_bench import device_ms, once_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_walk(offsets, n):
    """The greedy selection over ascending offsets in numpy, as fast as the host does it: the list is cut into runs at the heads
    (an offset n or more beyond its predecessor); a run of one offset is one selection, a run whose gaps are all d selects every
    ceil(n / d)-th entry - both vectorised - and only a run with mixed gaps is walked offset by offset."""
    if offsets.size == 0:
        return 0
    gaps = np.diff(offsets)
    heads = np.flatnonzero(np.concatenate([[True], gaps >= n]))
    ends = np.concatenate([heads[1:], [offsets.size]])
    lens = ends - heads
    total = int((lens == 1).sum())
    multi = np.flatnonzero(lens > 1)
    if multi.size:
        g = np.concatenate([gaps, [0]])
        idx = np.stack([heads[multi], ends[multi] - 1], axis=1).ravel()
        lo, hi = np.minimum.reduceat(g, idx)[::2], np.maximum.reduceat(g, idx)[::2]
        uniform = lo == hi
        step = -(-n // lo[uniform])
        total += int((-(-lens[multi][uniform] // step)).sum())
        for r in multi[~uniform]:
            nxt = -1
            for p in offsets[heads[r]:ends[r]].tolist():
                if p >= nxt:
                    total += 1
                    nxt = p + n
    return total


def row(name, hay, needle, gib, reps, ceiling):
    n, n_bytes = len(needle), hay.numel()
    with ss.disjoint_build():
        s = ss.DynamicHipSearcher.new(needle)
    over, sel = s.count(hay), s.count_disjoint(hay)
    model_count = wall_ms(lambda: s.count(hay), reps)
    new_count = wall_ms(lambda: s.count_disjoint(hay), reps)
    all_offsets = torch.empty(max(over, 1), dtype=torch.int64, device="cuda")
    kept = torch.empty(max(sel, 1), dtype=torch.int64, device="cuda")
    model_find = wall_ms(lambda: s.find_all_into(hay, all_offsets), reps)
    new_find = wall_ms(lambda: s.find_all_disjoint_into(hay, kept), reps)
    with ss.disjoint_build():
        assert ss.select_disjoint_into(all_offsets[:over], n, kept) == sel if over else True
        select = wall_ms(lambda: ss.select_disjoint_into(all_offsets[:over], n, kept), reps) if over else 0.0

    def host_route():
        s.find_all_into(hay, all_offsets)
        return host_walk(all_offsets[:over].cpu().numpy(), n)
    assert host_route() == sel
    host_ms = once_ms(host_route)
    rep = bytes(c ^ 1 for c in needle)                          # (other bytes, the same length)
    out = s.replace(hay, rep)
    new_replace = wall_ms(lambda: s.replace(hay, rep), reps)
    replace_dev = device_ms(lambda: s.replace(hay, rep), reps)

    def host_replace():
        return torch.from_numpy(np.frombuffer(hay.cpu().numpy().tobytes().replace(needle, rep), dtype=np.uint8)).cuda()
    t0 = time.perf_counter()
    ref = host_replace()
    torch.cuda.synchronize()
    host_replace_ms = (time.perf_counter() - t0) * 1e3
    assert torch.equal(out, ref)
    print(json.dumps({"row": "disjoint", "haystack": name, "gib": round(n_bytes / (1 << 30), 3), "needle": needle.decode("latin-1"),
                      "overlapping": over, "disjoint": sel, "temporary_bytes": 16 * over if over != sel or n_bytes == 0 else 0,
                      "count_ms": round(model_count, 3), "count_disjoint_ms": round(new_count, 3),
                      "count_disjoint_over_count": round(new_count / model_count, 2),
                      "find_all_ms": round(model_find, 3), "find_all_disjoint_ms": round(new_find, 3),
                      "find_all_disjoint_over_find_all": round(new_find / model_find, 2),
                      "select_ms": round(select, 3), "select_share_of_find_all_disjoint": round(select / new_find, 3),
                      "host_route_ms": round(host_ms, 3), "host_route_over_count_disjoint": round(host_ms / new_count, 2),
                      "replace_ms": round(new_replace, 3), "host_replace_ms": round(host_replace_ms, 3),
                      "host_replace_over_replace": round(host_replace_ms / new_replace, 2), "replace_device_ms": round(replace_dev, 3),
                      "replace_gb_per_s": round(n_bytes / replace_dev / 1e6, 1), "read_ceiling_gb_per_s": round(ceiling, 1),
                      "replace_share_of_ceiling": round(n_bytes / replace_dev / 1e6 / ceiling, 3), "reps": reps}), flush=True)
    del all_offsets, kept, out, ref
    torch.cuda.empty_cache()


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    n_bytes = int(gib * (1 << 30))
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(n_bytes // text.numel() + 1)[:n_bytes].contiguous()
    ceiling = ss.read_ceiling_gbps(hay)
    row("manual", hay, b"  ", gib, reps, ceiling)
    row("manual", hay, b"the", gib, reps, ceiling)
    ss.fill_random_device(hay, 0x5EED0001)
    row("generator", hay, b"no such needle", gib, reps, ceiling)
    del hay
    torch.cuda.empty_cache()
    hay = torch.full((n_bytes // 4,), ord("a"), dtype=torch.uint8, device="cuda")
    row("one byte repeated", hay, b"aa", gib, reps, ss.read_ceiling_gbps(hay))


if __name__ == "__main__":
    main()
