#!/usr/bin/env python3
"""./matches_bench.py [--gib 1,8] [--reps 20] - rates of every-occurrence search (libsliceslice_hip_matches.so), a measurement aid
(nothing here is asserted).  One JSON line per case:
  absent     random bytes, a 16-byte needle that does not occur: count and search_in ALTERNATING in one process on one buffer with
             autotune off (the same filter over the same loads), and find_all (count pass + prefix + an emit grid that leaves at once)
  density    planted needles at 1 per MiB and 1 per KiB (1 GiB of random bytes): count and find_all
  text       common words of tests/golden/data/i386.txt, the text tiled to 1 GiB: count and find_all (candidate-dense, no early exit)
Times are hipEvent pairs around the synchronous call (launches included), median of --reps.
./matches_bench.py --batched [--reps 20] - the batched calls (libsliceslice_hip_matches_batched.so), one JSON line per case:
  batched_absent   4,096 x 1 MiB of random bytes, 16-byte needles that do not occur: count_batched and search_batched ALTERNATING in
                   one process on one blob, and find_all_batched (count pass + prefix + rows + an emit grid that leaves at once)
  batched_i386     the reference's bench loop as a table: 4,585 words against tests/golden/data/i386.txt - ONE count_batched call,
                   ONE find_all_batched call (every offset), and the loop of 4,585 count() calls, wall clock
  batched_density  1,024 x 1 MiB, the needle planted once per KiB: count_batched and find_all_batched (every offset)"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sliceslice_rs_amd as ss  # noqa: E402


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def emit(row):
    print(json.dumps(row), flush=True)


def batched(reps):
    import time
    needle = bytes(range(0x61, 0x71))
    with ss.matches_batched_build():
        def csr(count, each):
            return torch.arange(0, (count + 1) * each, each, dtype=torch.int64, device="cuda")
        # (a) absent needles on random bytes
        count, each = 4096, 1 << 20
        hay = torch.empty(count * each, dtype=torch.uint8, device="cuda")
        ss.fill_random_device(hay, 0x5EED0779)
        nd = torch.tensor(list(needle) * count, dtype=torch.uint8, device="cuda")
        ho, no = csr(count, each), csr(count, 16)
        assert int(ss.count_batched(hay, ho, nd, no).sum()) == 0
        for _ in range(3):                                  # (search_batched samples the blob's bytes in front of its second call)
            ss.search_batched(hay, ho, nd, no)
        c_ms, s_ms = [], []
        for _ in range(reps):                               # alternating
            c_ms.append(timed(lambda: ss.count_batched(hay, ho, nd, no), 1))
            s_ms.append(timed(lambda: ss.search_batched(hay, ho, nd, no), 1))
        f_ms = timed(lambda: ss.find_all_batched(hay, ho, nd, no, capacity=1024), reps)
        c, se = statistics.median(c_ms), statistics.median(s_ms)
        emit({"case": "batched_absent", "problems": count, "bytes_each": each, "count_batched_ms": c, "search_batched_ms": se,
              "count_over_search_rate": se / c, "find_all_batched_ms": f_ms, "find_all_minus_count_us": (f_ms - c) * 1e3,
              "count_gbps": count * each / c / 1e6})
        # (c) one match per KiB
        count = 1024
        hay = hay[:count * each]
        hay.view(-1, 1024)[:, 100:116] = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
        ho, no, nd = csr(count, each), csr(count, 16), nd[:count * 16]
        total = int(ss.count_batched(hay, ho, nd, no).sum())
        c = timed(lambda: ss.count_batched(hay, ho, nd, no), reps)
        f = timed(lambda: ss.find_all_batched(hay, ho, nd, no, capacity=total), reps)
        emit({"case": "batched_density", "problems": count, "bytes_each": each, "per": "1/KiB", "matches": total, "count_batched_ms": c,
              "find_all_batched_ms": f, "count_gbps": count * each / c / 1e6, "find_all_gbps": count * each / f / 1e6})
        del hay
        # (b) the i386 table
        gd = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "data")
        text = open(os.path.join(gd, "i386.txt"), "rb").read()
        words = [w for w in open(os.path.join(gd, "words.txt"), "rb").read().split(b"\n") if w]
        d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        nd = torch.from_numpy(np.frombuffer(b"".join(words) + b"\x00", dtype=np.uint8).copy()).cuda()
        no = torch.from_numpy(np.cumsum([0] + [len(w) for w in words]).astype(np.int64)).cuda()
        hr = (torch.zeros(len(words), dtype=torch.int64, device="cuda"), torch.full((len(words),), len(text), dtype=torch.int64, device="cuda"))
        total = int(ss.count_batched(d_text, None, nd, no, hay_ranges=hr).sum())
        c = timed(lambda: ss.count_batched(d_text, None, nd, no, hay_ranges=hr), reps)
        f = timed(lambda: ss.find_all_batched(d_text, None, nd, no, hay_ranges=hr, capacity=total), reps)
        sb = timed(lambda: ss.search_batched(d_text, None, nd, no, hay_ranges=hr), reps)
        searchers = [ss.DynamicHipSearcher.new(w) for w in words]
        loop = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = sum(s.count(d_text) for s in searchers)
            loop.append((time.perf_counter() - t0) * 1e3)
        assert got == total
        emit({"case": "batched_i386", "words": len(words), "text_bytes": len(text), "matches": total, "count_batched_ms": c,
              "find_all_batched_ms": f, "search_batched_ms": sb, "loop_of_count_calls_ms": statistics.median(loop),
              "loop_over_count_batched": statistics.median(loop) / c})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", default="1,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batched", action="store_true")
    args = ap.parse_args()
    if args.batched:
        return batched(args.reps)
    needle = bytes(range(0x61, 0x71))
    with ss.matches_build():
        ss.set_autotune(False)                          # (the matches library's own switch: it is a library of its own)
        s = ss.DynamicHipSearcher.new(needle)
    for gib in [float(g) for g in args.gib.split(",")]:
        n_bytes = int(gib * (1 << 30))
        hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
        ss.fill_random_device(hay, 0x5EED0777)
        assert s.count(hay) == 0
        c_ms, s_ms = [], []
        for _ in range(args.reps):                      # alternating
            c_ms.append(timed(lambda: s.count(hay), 1))
            s_ms.append(timed(lambda: s.search_in(hay), 1))
        f_ms = timed(lambda: s.find_all(hay, capacity=1024), args.reps)
        c, se = statistics.median(c_ms), statistics.median(s_ms)
        emit({"case": "absent", "gib": gib, "count_ms": c, "search_in_ms": se, "count_over_search_rate": se / c, "find_all_ms": f_ms,
              "find_all_minus_count_us": (f_ms - c) * 1e3, "count_gbps": n_bytes / c / 1e6})
        del hay
        torch.cuda.empty_cache()
    n_bytes = 1 << 30
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    nt = torch.tensor(list(needle), dtype=torch.uint8, device="cuda")
    for per, label in ((1 << 20, "1/MiB"), (1 << 10, "1/KiB")):
        ss.fill_random_device(hay, 0x5EED0778)
        hay.view(-1, per)[:, 100:116] = nt
        total = s.count(hay)
        c = timed(lambda: s.count(hay), args.reps)
        f = timed(lambda: s.find_all(hay, capacity=total), args.reps)
        emit({"case": "density", "per": label, "matches": total, "count_ms": c, "find_all_ms": f, "count_gbps": n_bytes / c / 1e6,
              "find_all_gbps": n_bytes / f / 1e6})
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "data", "i386.txt"), "rb").read()
    reps_t = n_bytes // len(text) + 1
    hay = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda().repeat(reps_t)[:n_bytes].contiguous()
    for w in (b"the", b"instruction", b"register", b"Intel"):
        with ss.matches_build():
            sw = ss.DynamicHipSearcher.new(w)
        total = sw.count(hay)
        c = timed(lambda: sw.count(hay), args.reps)
        f = timed(lambda: sw.find_all(hay, capacity=total), args.reps)
        emit({"case": "text", "word": w.decode(), "matches": total, "count_ms": c, "find_all_ms": f, "count_gbps": n_bytes / c / 1e6,
              "find_all_gbps": n_bytes / f / 1e6})


if __name__ == "__main__":
    main()
