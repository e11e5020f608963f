#!/usr/bin/env python3
"""./setmatches_bench.py [--gib 1] [--reps 9] [--no-words] - rates of the occurrence calls of a needle set
(libsliceslice_hip_setmatches.so), a measurement aid: one JSON line per row, medians of `reps`.  Two haystacks of the size asked
for: the manual's text tiled, and the generator's bytes (ss.fill_random_device).  Per haystack, for 1, 3 and 16 needles and for the
4,585-word list:
  count     the set's count (one bin per needle) against the loop of per-needle `count` calls of the same build
  find_all  the set's find_all_into with room for every pair against the loop of per-needle `find_all_into` calls (unmerged: the
            loop is given the advantage of not ordering its lists)
  batched   the same counts from ONE count_batched call of libsliceslice_hip_matches_batched.so, a library of its own
  scan      the device time of the set's count call by stream events - two memsets and the scan kernel - as a rate, beside the
            plain-read ceiling of the same buffer (ss.read_ceiling_gbps)
The word list's loops are 4,585 scans each: they run ONCE, not `reps` times, and --no-words leaves the row out."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from anyof_bench import SIXTEEN  # noqa: E402
from lines_bench import wall_ms  # noqa: E402
from needleset_bench import device_ms, once_ms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
        for label, needles in sets:
            once = label == "words"
            with ss.setmatches_build():
                st = ss.NeedleSet(needles)
                searchers = [ss.DynamicHipSearcher(n) for n in needles]
            by_rank = torch.empty(st.info()["distinct"], dtype=torch.int64, device="cuda")
            total_dev = torch.empty(1, dtype=torch.int64, device="cuda")
            counts = st.count(hay)
            total = st.count_total(hay)
            set_count = wall_ms(lambda: st.count(hay), reps)
            scan = device_ms(lambda: st.count_async(hay, by_rank, total_dev), reps)
            cap = max(total, 1)
            offsets, ranks = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
            set_find = wall_ms(lambda: st.find_all_into(hay, offsets, ranks, cap), reps)
            loop_count = (lambda: [s.count(hay) for s in searchers])
            assert loop_count() == counts.cpu().tolist()
            loop_count_ms = once_ms(loop_count) if once else wall_ms(loop_count, reps)

            def loop_find():
                at = 0
                for s, c in zip(searchers, per_needle):
                    s.find_all_into(hay, offsets[at:at + max(c, 1)])
                    at += c
            per_needle = counts.cpu().tolist()
            if sum(per_needle) <= cap:                          # (duplicates in the list would need more room than the pairs)
                loop_find_ms = once_ms(loop_find) if once else wall_ms(loop_find, reps)
            else:
                loop_find_ms = None
            # one count_batched call, in its own library: every needle against the whole haystack
            blob = torch.from_numpy(np.frombuffer(b"".join(needles) + b"\x00", dtype=np.uint8).copy()).cuda()
            cuts = torch.from_numpy(np.cumsum([0] + [len(p) for p in needles]).astype(np.int64)).cuda()
            hb = torch.zeros(len(needles), dtype=torch.int64, device="cuda")
            he = torch.full((len(needles),), n_bytes, dtype=torch.int64, device="cuda")
            with ss.matches_batched_build():
                def batched():
                    out = ss.count_batched(hay, None, blob, cuts, hay_ranges=(hb, he))
                    torch.cuda.synchronize()
                    return out
                assert torch.equal(batched(), counts)
                batched_ms = once_ms(batched) if once else wall_ms(batched, reps)
            print(json.dumps({"row": "setmatches", "haystack": name, "gib": gib, "needles": len(needles), "pairs": total, "info": st.info(),
                              "set_count_ms": round(set_count, 3), "loop_count_ms": round(loop_count_ms, 3),
                              "loop_over_set_count": round(loop_count_ms / set_count, 2), "count_batched_ms": round(batched_ms, 3),
                              "batched_over_set_count": round(batched_ms / set_count, 2), "set_find_all_ms": round(set_find, 3),
                              "loop_find_all_ms": None if loop_find_ms is None else round(loop_find_ms, 3),
                              "loop_over_set_find_all": None if loop_find_ms is None else round(loop_find_ms / set_find, 2),
                              "loops_timed": "once" if once else "median of %d" % reps, "scan_device_ms": round(scan, 3),
                              "scan_gb_per_s": round(n_bytes / scan / 1e6, 1), "read_ceiling_gb_per_s": round(ceiling, 1),
                              "scan_share_of_ceiling": round(n_bytes / scan / 1e6 / ceiling, 3)}), flush=True)
            st.close()
            del offsets, ranks, searchers, blob, cuts, hb, he
            torch.cuda.empty_cache()
        del hay
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
