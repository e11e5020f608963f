#!/usr/bin/env python3
"""./anyof_bench.py [--gib 1] [--reps 9] - rates of the several-needle calls (libsliceslice_hip_anyof.so), a measurement aid: one JSON
line per row, medians of `reps`.  The manual's text tiled to the size asked for.
  anyof     find_lines_anyof_into with room for every line, for 1, 3 and 16 needles, against the SUM of its models' find_lines_into
            times (one call per needle, the single-needle route's scans); the union alone and the census alone on the same
            numbers, and their share of the call
  union     union_numbers_into on the three needles' device arrays against np.union1d on the host including both copies"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from lines_bench import wall_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIXTEEN = [b"the", b"descriptor", b"intel", b"segment", b"protect", b"mode", b"386", b"register", b"page", b"task", b"gate", b"stack",
           b"flag", b"address", b"privilege", b"interrupt"]


def host_union(lists):
    union = lists[0].cpu().numpy()
    for l in lists[1:]:
        union = np.union1d(union, l.cpu().numpy())
    return torch.from_numpy(union).cuda()


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 9
    n_bytes = int(gib * (1 << 30))
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(n_bytes // text.numel() + 1)[:n_bytes].contiguous()
    one = torch.ones(1, dtype=torch.int64, device="cuda")
    with ss.anyof_build():
        for k in (1, 3, 16):
            searchers = [ss.DynamicHipSearcher(n) for n in SIXTEEN[:k]]
            total, selected = ss.find_lines_anyof_into(searchers, hay, None, None, None, None, 0)
            cap = max(total, 1)
            bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)] + [torch.empty(cap, dtype=torch.uint8, device="cuda")]
            ms = wall_ms(lambda: ss.find_lines_anyof_into(searchers, hay, bufs[0], bufs[1], bufs[2], bufs[3], cap), reps)
            models, lists = 0.0, []
            for s in searchers:
                n = max(s.count_lines(hay), 1)
                out = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(3)]
                models += wall_ms(lambda: s.find_lines_into(hay, out[0], out[1], out[2], n), reps)
                lists.append(out[2])
                del out
            n_lines = searchers[0].lines_around_into(hay, one, None, None, None, None, 0, 0, 2 ** 64 - 1)
            union = wall_ms(lambda: ss.union_numbers_into(lists, n_lines, bufs[2], cap), reps)
            census = wall_ms(lambda: searchers[0].lines_around_into(hay, one, None, None, None, None, 0, 0, 2 ** 64 - 1), reps)
            print(json.dumps({"row": "anyof", "gib": gib, "needles": k, "lines": n_lines, "selected": selected, "listed": int(sum(l.numel() for l in lists)),
                              "find_lines_anyof_ms": round(ms, 3), "sum_of_models_find_lines_ms": round(models, 3),
                              "anyof_over_models": round(ms / models, 3), "union_ms": round(union, 4), "census_ms": round(census, 4),
                              "union_and_census_share": round((union + census) / ms, 4)}), flush=True)
            if k == 3:
                t_numpy = wall_ms(lambda: host_union(lists), max(reps // 3, 3))
                assert torch.equal(host_union(lists), bufs[2][:selected])
                print(json.dumps({"row": "union", "gib": gib, "lists": k, "listed": int(sum(l.numel() for l in lists)), "union": selected,
                                  "union_numbers_ms": round(union, 4), "np_union1d_with_copies_ms": round(t_numpy, 3),
                                  "union1d_over_union_numbers": round(t_numpy / union, 1)}), flush=True)
            del bufs, lists
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
