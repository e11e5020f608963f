#!/usr/bin/env python3
"""./needleset_bench.py [--gib 1] [--reps 9] [--no-words] - rates of the needle-set calls (libsliceslice_hip_needleset.so), a
measurement aid: one JSON line per row, medians of `reps`.  Two haystacks of the size asked for: the manual's text tiled, and the
generator's bytes (ss.fill_random_device).  Per haystack, for 1, 3 and 16 needles and for the 4,585-word list:
  find      the set's find_lines_into with room for every selected line against find_lines_anyof_into of the same build
  count     the set's count_lines against count_lines_anyof
  scan      the device time of the set's count call by stream events - the scan kernel and the two combine launches behind it,
            which take microseconds - as a rate, beside the plain-read ceiling of the same buffer (ss.read_ceiling_gbps)
The word list's anyof calls are 4,585 scans each: they run ONCE, not `reps` times, and --no-words leaves the row out."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from anyof_bench import SIXTEEN  # noqa: E402
from lines_bench import wall_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_ms(fn, reps):
    out = []
    for k in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= 2:
            out.append(a.elapsed_time(b))
    return float(np.median(out))


def once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 9
    n_bytes = int(gib * (1 << 30))
    golden = os.path.join(ROOT, "tests", "golden", "data")
    words = [w for w in open(os.path.join(golden, "words.txt"), "rb").read().split(b"\n") if w]
    text = torch.from_numpy(np.fromfile(os.path.join(golden, "i386.txt"), dtype=np.uint8)).cuda()
    sets = [("1", SIXTEEN[:1]), ("3", SIXTEEN[:3]), ("16", SIXTEEN)] + ([] if "--no-words" in argv else [("words", words)])
    for name in ("manual", "generator"):
        if name == "manual":
            hay = text.repeat(n_bytes // text.numel() + 1)[:n_bytes].contiguous()
        else:
            hay = ss.fill_random_device(torch.empty(n_bytes, dtype=torch.uint8, device="cuda"), 0x5EED0001)
        ceiling = ss.read_ceiling_gbps(hay)
        with ss.needleset_build():
            for label, needles in sets:
                once = label == "words"
                st = ss.NeedleSet(needles)
                searchers = [ss.DynamicHipSearcher(n) for n in needles]
                total, selected = st.find_lines_into(hay, None, None, None, None, 0)
                cap = max(total, 1)
                bufs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)] + [torch.empty(cap, dtype=torch.uint8, device="cuda")]
                set_find = wall_ms(lambda: st.find_lines_into(hay, bufs[0], bufs[1], bufs[2], bufs[3], cap), reps)
                set_count = wall_ms(lambda: st.count_lines(hay), reps)
                scan = device_ms(lambda: st.count_lines(hay), reps)
                mine = bufs[2][:total].clone()
                find = (lambda: ss.find_lines_anyof_into(searchers, hay, bufs[0], bufs[1], bufs[2], bufs[3], cap))
                count = (lambda: ss.count_lines_anyof(searchers, hay))
                any_find = once_ms(find) if once else wall_ms(find, reps)
                assert torch.equal(mine, bufs[2][:total]) and ss.count_lines_anyof(searchers, hay) == selected == total
                any_count = once_ms(count) if once else wall_ms(count, reps)
                print(json.dumps({"row": "needleset", "haystack": name, "gib": gib, "needles": len(needles), "selected": selected,
                                  "info": st.info(), "set_find_lines_ms": round(set_find, 3), "find_lines_anyof_ms": round(any_find, 3),
                                  "anyof_over_set_find": round(any_find / set_find, 2), "set_count_lines_ms": round(set_count, 3),
                                  "count_lines_anyof_ms": round(any_count, 3), "anyof_over_set_count": round(any_count / set_count, 2),
                                  "anyof_timed": "once" if once else "median of %d" % reps, "scan_device_ms": round(scan, 3),
                                  "scan_gb_per_s": round(n_bytes / scan / 1e6, 1), "read_ceiling_gb_per_s": round(ceiling, 1),
                                  "scan_share_of_ceiling": round(n_bytes / scan / 1e6 / ceiling, 3)}), flush=True)
                st.close()
                del bufs, searchers, mine
                torch.cuda.empty_cache()
        del hay
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
