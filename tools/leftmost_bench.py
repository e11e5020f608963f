#!/usr/bin/env python3
"""What the leftmost-longest calls (include/sliceslice_hip_leftmost.h) cost, one JSON line per row:
    python tools/leftmost_bench.py [--gib 1] [--reps 5] > profiles/leftmost/leftmost_bench_1gib.jsonl

Rows "set": on the manual's text tiled to --gib, for 1, 3 and 16 needles and the 4,585-word list of tests/golden/data/words.txt -
`count_leftmost`, `find_all_leftmost` and `replace` (every needle replaced by its upper-case form plus `!`) against the set's own
`count_total` / `find_all`, their model and so a lower bound; the selection alone (`select_leftmost_into` on the resident pairs) and
its share of `find_all_leftmost`; the host route (the set's `find_all`, both arrays to the host, candidates and successors by
numpy's searchsorted, the walk; once, and only below --host-pairs pairs); `ss_replace_set_device` with the buffer given against the
same call with capacity 0, which does everything but the copy pass - the difference is the copy pass, given as a share of the call
and as a rate over the output bytes beside `copy_` of those bytes; for one needle, beside `ss_replace_device` of the same needle.
Rows "dense": a haystack of spaces with the sets {" "} (every entry a head), {" ", "xx"} and {" ", 5,000 x "x"} (no head but the
first: the chain pass walks every block, and one lane walks each block of the emit pass).  Medians of --reps, a host clock around
synchronised calls, after one warm-up call."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sliceslice_rs_amd as ss  # noqa: E402

SIXTEEN = [b"the", b"then", b"there", b"he", b"here", b"segment", b"segments", b"descriptor", b"descriptors", b"table", b"in", b"int",
           b"interrupt", b"interrupts", b"  ", b" "]


def timed(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 3)


def host_walk(offsets, lengths):
    if offsets.size == 0:
        return 0
    last = np.ones(offsets.size, dtype=bool)
    last[:-1] = offsets[1:] != offsets[:-1]
    o, l = offsets[last], lengths[last]
    succ = np.searchsorted(o, o + l, side="left").tolist()
    total, j, n = 0, 0, len(succ)
    while j < n:
        total += 1
        j = succ[j]
    return total


def replace_call(L, nset, hay, texts, out, capacity):
    reps = (ctypes.c_char_p * len(texts))(*texts)
    lens = (ctypes.c_size_t * len(texts))(*[len(t) for t in texts])
    out_len, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = L.ss_replace_set_device(nset._h, hay.data_ptr(), hay.numel(), 0, ctypes.cast(reps, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p),
                                 len(texts), torch.cuda.current_stream().cuda_stream, out.data_ptr() if out is not None else None, capacity,
                                 ctypes.byref(out_len), ctypes.byref(count))
    assert rc == 0, L.ss_last_error()
    return out_len.value


def set_row(L, name, needles, hay, reps, host_pairs):
    nset = ss.NeedleSet(needles)
    pairs, selected = nset.count_total(hay), nset.count_leftmost(hay)
    row = {"row": "set", "needles": name, "count": len(needles), "bytes": hay.numel(), "pairs": pairs, "selected": selected,
           "temporary_bytes": pairs * 20}
    row["count_total_ms"] = timed(lambda: nset.count_total(hay), reps)
    row["count_leftmost_ms"] = timed(lambda: nset.count_leftmost(hay), reps)
    row["count_leftmost_over_count_total"] = round(row["count_leftmost_ms"] / row["count_total_ms"], 2)
    d_off = torch.empty(max(pairs, 1), dtype=torch.int64, device="cuda")
    d_rank = torch.empty(max(pairs, 1), dtype=torch.int32, device="cuda")
    row["find_all_ms"] = timed(lambda: nset.find_all_into(hay, d_off, d_rank, pairs), reps)
    s_off = torch.empty(max(selected, 1), dtype=torch.int64, device="cuda")
    s_rank = torch.empty(max(selected, 1), dtype=torch.int32, device="cuda")
    row["find_all_leftmost_ms"] = timed(lambda: nset.find_all_leftmost_into(hay, s_off, s_rank, selected), reps)
    row["find_all_leftmost_over_find_all"] = round(row["find_all_leftmost_ms"] / row["find_all_ms"], 2)
    # the selection alone, on the resident pairs
    d_len = torch.from_numpy(nset.lengths()).cuda()[d_rank[:pairs].long()]
    s_which = torch.empty(max(selected, 1), dtype=torch.int64, device="cuda")
    assert ss.select_leftmost_into(d_off[:pairs], d_len, s_off, s_which, selected) == selected
    row["select_ms"] = timed(lambda: ss.select_leftmost_into(d_off[:pairs], d_len, s_off, s_which, selected), reps)
    row["select_share_of_find_all_leftmost"] = round(row["select_ms"] / row["find_all_leftmost_ms"], 3)
    if pairs <= host_pairs:
        by_rank = nset.lengths()
        t0 = time.perf_counter()
        nset.find_all_into(hay, d_off, d_rank, pairs)
        got = host_walk(d_off[:pairs].cpu().numpy(), by_rank[d_rank[:pairs].cpu().numpy()])
        row["host_route_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert got == selected, (got, selected)
        row["host_route_over_count_leftmost"] = round(row["host_route_ms"] / row["count_leftmost_ms"], 1)
    else:
        row["host_route_ms"] = None                                     # (above --host-pairs: not run)
    del d_off, d_rank, d_len, s_off, s_rank, s_which
    torch.cuda.empty_cache()
    # replace: the call with its buffer, the call without (everything but the copy pass), copy_ of the output's bytes
    texts = [n.upper() + b"!" for n in needles]
    out_len = replace_call(L, nset, hay, texts, None, 0)
    out = torch.empty(out_len, dtype=torch.uint8, device="cuda")
    row["replace_out_bytes"] = out_len
    row["replace_sizing_call_ms"] = timed(lambda: replace_call(L, nset, hay, texts, None, 0), reps)
    row["replace_call_ms"] = timed(lambda: replace_call(L, nset, hay, texts, out, out_len), reps)
    copy_pass = max(row["replace_call_ms"] - row["replace_sizing_call_ms"], 1e-3)
    row["copy_pass_ms"] = round(copy_pass, 3)
    row["copy_pass_share_of_replace_call"] = round(copy_pass / row["replace_call_ms"], 3)
    row["copy_pass_gbps"] = round(out_len / copy_pass / 1e6, 1)
    row["replace_call_gbps"] = round(out_len / row["replace_call_ms"] / 1e6, 1)
    other = torch.empty_like(out)
    row["copy_ms"] = timed(lambda: other.copy_(out), reps)
    row["copy_gbps"] = round(out_len / row["copy_ms"] / 1e6, 1)
    row["python_replace_ms"] = timed(lambda: nset.replace(hay, texts), reps)       # (sizes first: the route twice)
    if len(needles) == 1:
        s = ss.DynamicHipSearcher(needles[0])
        assert torch.equal(s.replace(hay, texts[0]), out)
        row["searcher_replace_ms"] = timed(lambda: s.replace(hay, texts[0]), reps)
        row["python_replace_over_searcher_replace"] = round(row["python_replace_ms"] / row["searcher_replace_ms"], 2)
    del out, other
    torch.cuda.empty_cache()
    print(json.dumps(row), flush=True)


def dense_row(mib, reps):
    n = mib << 20
    spaces = torch.full((n,), 32, dtype=torch.uint8, device="cuda")
    row = {"row": "dense", "bytes": n, "blocks": n // ss.LEFTMOST_BLOCK}
    for name, needles in (("one_byte_alone", [b" "]), ("beside_two_bytes", [b" ", b"xx"]), ("beside_5000_bytes", [b" ", b"x" * 5000])):
        nset = ss.NeedleSet(needles)
        assert nset.count_leftmost(spaces) == n
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        row[name + "_count_total_ms"] = timed(lambda: nset.count_total(spaces), reps)
        row[name + "_count_leftmost_ms"] = timed(lambda: nset.count_leftmost(spaces), reps)
        row[name + "_find_all_leftmost_ms"] = timed(lambda: nset.find_all_leftmost_into(spaces, out, None, n), reps)
        del out
    print(json.dumps(row), flush=True)


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
    ap.add_argument("--host-pairs", type=int, default=100_000_000)
    ap.add_argument("--dense-mib", type=int, nargs="*", default=[64, 256])
    a = ap.parse_args()
    size = int(a.gib * (1 << 30))
    manual = np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)
    words = [w for w in open(os.path.join(ROOT, "tests", "golden", "data", "words.txt"), "rb").read().split(b"\n") if w]
    ctx = _loaded() if getattr(ss.lib(), "has_leftmost", False) else ss.leftmost_build()
    with ctx as L:
        hay = torch.from_numpy(manual).cuda().repeat(size // manual.size + 1)[:size].contiguous()
        for name, needles in (("1", SIXTEEN[:1]), ("3", SIXTEEN[:3]), ("16", SIXTEEN), ("words", words)):
            set_row(L, name, needles, hay, a.reps if name != "words" else min(a.reps, 2), a.host_pairs)
        del hay
        torch.cuda.empty_cache()
        for mib in a.dense_mib:
            dense_row(mib, a.reps)


if __name__ == "__main__":
    main()
