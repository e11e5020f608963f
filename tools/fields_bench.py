#!/usr/bin/env python3
"""The field calls (include/sliceslice_hip_fields.h) on the manual's text tiled to SIZE (default 1 GiB): count and find for ` ` EACH 2,
`[ \\t]` MERGE 2, MERGE 7- and MERGE 2 with KEEP_SHORT - wall time of the waiting call (median of 5 after a warm-up) beside the
plain-read ceiling, and the share of workgroups that hold a record begin or end, which the find reads a second time.  Then, at
256 MiB, the route a caller had before - `find_lines` of the empty needle, `find_all` of the separator, both copied to the host, a
`numpy.searchsorted` join - and the two cases expected to lose: a view of one-byte lines and MERGE on separator-dense text.

    python tools/fields_bench.py [GIB=1] > profiles/fields/fields_bench_1gib.jsonl"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sliceslice_rs_amd as ss  # noqa: E402

MiB, WG = 1 << 20, 131072


def wall(fn, reps=5, warm=1):
    times, out = [], None
    for k in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warm:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def measure(name, sel, hay, ceiling_gbps, room):
    """one row: count and find (room for every record) of one selector on one view"""
    count_ms, (selected, total) = wall(lambda: sel.count(hay))
    records = total if sel.keep_short else selected
    out = torch.empty((3, max(records, 1)), dtype=torch.int64, device="cuda") if room else None
    row = {"case": name, "bytes": hay.numel(), "selected": selected, "lines": total, "records": records, "count_ms": round(count_ms, 3),
           "ceiling_ms": round(hay.numel() / (ceiling_gbps * 1e6), 3), "count_share_of_ceiling": round(hay.numel() / (ceiling_gbps * 1e6) / count_ms, 3)}
    if room:
        find_ms, n = wall(lambda: sel.find_into(hay, out[0], out[1], out[2], records))
        assert n == records
        parts = (hay.numel() + WG - 1) // WG
        twice = torch.unique(torch.cat((out[0, :records] // WG, torch.clamp(out[1, :records] - 1, min=0) // WG))).numel()
        row.update(find_ms=round(find_ms, 3), find_share_of_ceiling=round(hay.numel() / (ceiling_gbps * 1e6) / find_ms, 3),
                   workgroups_read_twice=round(twice / parts, 4))
    print(json.dumps(row), flush=True)
    return row


def main():
    gib = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    size = int(gib * 1024) * MiB
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(size // text.numel() + 1)[:size].contiguous()
    ceiling = ss.read_ceiling_gbps(hay)
    print(json.dumps({"device": ss.device_info(), "bytes": size, "read_ceiling_gbps": round(ceiling, 1)}), flush=True)
    # (SLICESLICE_HIP_LIB=<the fields library> is used as it is)
    with open(os.devnull) if getattr(ss.lib(), "has_fields", False) else ss.fields_build():
        cases = [("' ' EACH 2", ss.FieldSelector(b" ", 2)), ("[ \\t] MERGE 2", ss.FieldSelector(r"[ \t]", 2, merge=True)),
                 ("[ \\t] MERGE 7-", ss.FieldSelector(r"[ \t]", 7, 0, merge=True)),
                 ("[ \\t] MERGE 2 KEEP_SHORT", ss.FieldSelector(r"[ \t]", 2, merge=True, keep_short=True))]
        for name, sel in cases:
            measure(name, sel, hay, ceiling, True)
        # the route a caller had before, at 256 MiB: both lists to the host and a join there
        small = hay[:256 * MiB]
        sel = ss.FieldSelector(b" ", 2)
        empty = ss.DynamicHipSearcher.new(b"")
        one = ss.DynamicHipSearcher.new(b" ")

        def old_route():
            lb, le, ln = (x.cpu().numpy() for x in empty.find_lines(small))
            sp = one.find_all(small).cpu().numpy()                  # every separator byte
            k = np.searchsorted(sp, lb)                             # the first separator at or behind each line's begin
            has1 = (k < sp.size) & (sp[np.minimum(k, sp.size - 1)] < le)
            has2 = (k + 1 < sp.size) & (sp[np.minimum(k + 1, sp.size - 1)] < le)
            begin = sp[np.minimum(k, sp.size - 1)] + 1
            end = np.where(has2, sp[np.minimum(k + 1, sp.size - 1)], le)
            return begin[has1], end[has1], ln[has1]

        def new_route():
            return sel.find(small)

        want = old_route()
        got = [x.cpu().numpy() for x in new_route()]
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        old_ms, _ = wall(old_route, 3)
        new_ms, _ = wall(new_route, 5)
        print(json.dumps({"case": "baseline route at 256 MiB, ' ' EACH 2", "old_route_ms": round(old_ms, 2), "find_ms": round(new_ms, 3),
                          "find_over_old_route": round(new_ms / old_ms, 5)}), flush=True)
        runs_ms, _ = wall(lambda: ss.RunPattern(r"[^ \n]+").count(small))
        count_ms, _ = wall(lambda: sel.count(small))
        print(json.dumps({"case": "count against RunPattern('[^ \\n]+').count at 256 MiB", "count_ms": round(count_ms, 3), "runs_count_ms": round(runs_ms, 3),
                          "count_over_runs_count": round(count_ms / runs_ms, 3)}), flush=True)
        del want, got
        # the cases expected to lose, at 64 MiB
        lines1 = torch.from_numpy(np.frombuffer(b"x\n" * (32 * MiB), dtype=np.uint8).copy()).cuda()
        measure("one-byte lines, ',' EACH 1, 64 MiB", ss.FieldSelector(b",", 1), lines1, ceiling, True)
        dense = torch.from_numpy(np.frombuffer((b" a" * 31 + b" \n") * MiB, dtype=np.uint8).copy()).cuda()
        measure("separator-dense, ' ' MERGE 2, 64 MiB", ss.FieldSelector(b" ", 2, merge=True), dense, ceiling, True)
        measure("separator-dense, ' ' EACH 2, 64 MiB", ss.FieldSelector(b" ", 2), dense, ceiling, True)
        measure("the manual's first 64 MiB, ' ' MERGE 2", ss.FieldSelector(b" ", 2, merge=True), hay[:64 * MiB], ceiling, True)


if __name__ == "__main__":
    main()
