#!/usr/bin/env python3
"""Randomised differential test of the run calls (include/sliceslice_hip_runs.h) on the GPU against THE RULE restated in numpy
below: ss_count_runs_device, ss_find_all_runs_device, ss_count_lines_runs_device and ss_find_lines_runs_device.
    python tools/fuzz_runs.py SECONDS SEED [GIB]

Haystacks are fuzz_masked.py's, or bytes that are members with a probability drawn per case (so that runs of every length occur).
Sets are drawn from fuzz_classes.py's pool - single values cut from the view, exact masks, ranges, unions of ranges, negated singles,
`.` and random sets - and every set is asked on BOTH paths (range tests where it has at most four ranges, the bitmap forced), which
must agree.  Lengths around 1, 16, 17, 32, 33 and 4,096, with and without a maximum.  Views at every misalignment and around the
16 B, 1 KiB, 4 KiB, 16 KiB and 128 KiB borders; the find calls write into windows of larger buffers whose sentinels on both sides
must survive, at capacities that cut the lists, with either array left out.  Delimiters: a newline, zero, a byte of the text.  With
GIB (a size in GiB above 4) one buffer of that size is filled with a short period, and views that END above offset 2^32 are checked
against the period's arithmetic and, near the end, numpy.
Prints one JSON line; on the first mismatch a reproducer and exit 1."""
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
from fuzz_classes import random_set, sets_of  # noqa: E402
from fuzz_masked import BORDERS, Mismatch, _loaded, held, random_haystack, window  # noqa: E402

LENGTHS = [1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 64, 100, 4095, 4096]


def rule_runs(data, row, lo, hi, delimiter=None):
    if delimiter is not None:
        row = row.copy()
        row[delimiter] = False
    d = np.diff(np.concatenate([[False], row[data], [False]]).astype(np.int8))
    begin, end = np.flatnonzero(d == 1).astype(np.int64), np.flatnonzero(d == -1).astype(np.int64)
    keep = (end - begin >= lo) & ((end - begin <= hi) if hi else True)
    return begin[keep], end[keep]


def rule_lines(data, row, lo, hi, delimiter):
    begin, _ = rule_runs(data, row, lo, hi, delimiter)
    delims = np.flatnonzero(data == delimiter).astype(np.int64)
    ends = np.append(delims, data.size) if (delims.size == 0 or delims[-1] != data.size - 1) and data.size else delims
    begins = np.concatenate([[0], delims + 1])[:ends.size]
    sel = np.unique(np.searchsorted(ends, begin, side="left"))
    return begins[sel], ends[sel], sel + 1


def random_bounds(rng):
    lo = int(rng.choice(LENGTHS, p=[.2, .1, .08, .05, .08, .08, .05, .04, .06, .06, .04, .04, .04, .04, .04]))
    pick = rng.integers(0, 4)
    hi = None if pick < 2 else lo if pick == 2 else min(4096, lo + int(rng.choice([1, 2, 15, 16, 17, 100, 4096])))
    return lo, hi


def one_case(rng, stats):
    size = int(rng.choice([600, 5000, 20000, 140000, 280000], p=[.3, .3, .2, .1, .1]))
    host = random_haystack(rng, size + 32)
    row = random_set(rng, host)
    if rng.integers(0, 2) and not row.all():                        # members with probability p: long runs at p near 1
        p = float(rng.choice([0.5, 0.9, 0.98, 0.999, 0.02]))
        inside, outside = np.flatnonzero(row).astype(np.uint8), np.flatnonzero(~row).astype(np.uint8)
        host = np.where(rng.random(size + 32) < p, rng.choice(inside, size + 32), rng.choice(outside, size + 32)).astype(np.uint8)
    words = sets_of(row)[0]
    lo, hi = random_bounds(rng)
    nranges = int((np.diff(np.concatenate([[0], row.astype(np.int8)])) == 1).sum())
    pats = [ss.RunPattern.from_set(words, lo, hi, bitmap) for bitmap in (False, True)]
    info = pats[0].info()
    if (info["ranges"], info["path"], info["members"], pats[1].info()["path"]) != (nranges, 0 if nranges <= 4 else 1, int(row.sum()), 1):
        raise Mismatch(dict(call="info", info=info, ranges=nranges))
    stats["by_ranges"][str(min(nranges, 5))] = stats["by_ranges"].get(str(min(nranges, 5)), 0) + 1
    buf = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16
    buf[at:at + host.size].copy_(torch.from_numpy(host))
    views = [(stats["cases"] % 16, size)]                           # (every misalignment in turn)
    for _ in range(3):
        mis = int(rng.integers(0, 16))
        pick = rng.integers(0, 3)
        if pick == 0:
            length = max(0, lo + int(rng.integers(-1, 3)))
        elif pick == 1:
            b = int(rng.choice(BORDERS))
            length = max(0, b * int(rng.integers(1, 3)) - mis + int(rng.integers(-lo - 1, lo + 2)))
        else:
            length = int(rng.integers(0, size + 1))
        views.append((mis, min(length, size)))
    where = dict(set=[int(x) for x in words], min_len=lo, max_len=hi)
    for mis, length in views:
        dev, hv = buf[at + mis:at + mis + length], host[mis:mis + length]
        begin, end = rule_runs(hv, row, lo, hi)
        delimiter = int(rng.choice([10, 0, int(hv[rng.integers(0, hv.size)]) if hv.size else 10]))
        lb, le, ln = rule_lines(hv, row, lo, hi, delimiter)
        for path, pat in enumerate(pats):
            got = pat.count(dev)
            stats["calls"] += 1
            if got != begin.size:
                raise Mismatch(dict(call="count", path=path, got=got, want=int(begin.size), mis=mis, length=length, **where))
            cap = int(rng.choice([0, 1, max(begin.size - 1, 0), begin.size, begin.size + 1, int(rng.integers(0, begin.size + 2))]))
            (bbuf, bview), (ebuf, eview) = window(max(cap, 1)), window(max(cap, 1))
            leave = int(rng.integers(0, 3)) if cap else 3          # 1: no begins, 2: no ends, 3 (capacity 0): neither
            total = pat.find_all_into(dev, bview if leave not in (1, 3) else None, eview if leave not in (2, 3) else None, cap)
            stats["calls"] += 1
            if total != begin.size or not held(bbuf, begin, 0 if leave in (1, 3) else cap) or not held(ebuf, end, 0 if leave in (2, 3) else cap):
                raise Mismatch(dict(call="find_all", path=path, total=total, want=int(begin.size), cap=cap, leave=leave, mis=mis, length=length, **where))
            got = pat.count_lines(dev, bytes([delimiter]))
            stats["calls"] += 1
            if got != lb.size:
                raise Mismatch(dict(call="count_lines", path=path, got=got, want=int(lb.size), delimiter=delimiter, mis=mis, length=length, **where))
            cap = int(rng.choice([1, lb.size, lb.size + 1, int(rng.integers(0, lb.size + 2))]))
            w = [window(max(cap, 1)) for _ in range(3)]
            total = pat.find_lines_into(dev, w[0][1], w[1][1], w[2][1], cap, bytes([delimiter]))
            stats["calls"] += 1
            if total != lb.size or not all(held(w[k][0], x, cap) for k, x in enumerate((lb, le, ln))):
                raise Mismatch(dict(call="find_lines", path=path, total=total, want=int(lb.size), cap=cap, delimiter=delimiter, mis=mis, length=length, **where))
        stats["views"] += 1
        stats["runs"] += int(begin.size)
    stats["cases"] += 1


def large_cases(rng, gib, stats):
    """runs above offset 2^32: a buffer of a period of 7 bytes (one line each); the views begin at a line's first byte and end behind
    a delimiter, so that counts and lines follow by arithmetic"""
    size = int(gib * (1 << 30))
    period = np.frombuffer(b"abcabd\n", dtype=np.uint8)
    hay = torch.from_numpy(period.copy()).cuda().repeat(size // 7 + 1)[:size].contiguous()
    # (pattern, runs per period, lines per period, the runs of one period as (begin, end))
    for text, per_period, lines_per_period, spans in ((r"[ab]+", 2, 1, [(0, 2), (3, 5)]), (r"[ab]{2}", 2, 1, [(0, 2), (3, 5)]), (r"[ab]{3,}", 0, 0, []),
                                                    (r"\w+", 1, 1, [(0, 6)]), (r"\w{6}", 1, 1, [(0, 6)]), (r"\w{7,}", 0, 0, []), (r"[cd]+", 2, 1, [(2, 3), (5, 6)])):
        for bitmap in (False, True):
            words, lo, hi = ss.parse_runs(text)
            pat = ss.RunPattern.from_set(words, lo, hi, bitmap)
            row = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little").astype(bool)
            for start in (0, 7, 21):                                # misalignments 0, 7 and 5
                periods = (size - start) // 7 - int(rng.integers(0, 5))
                length = 7 * periods
                dev = hay[start:start + length]
                got = pat.count(dev)
                stats["calls"] += 1
                if got != per_period * periods:
                    raise Mismatch(dict(call="count above 2^32", got=got, want=per_period * periods, pattern=text, bitmap=bitmap, start=start, length=length))
                lines = pat.count_lines(dev)
                stats["calls"] += 1
                if lines != lines_per_period * periods:
                    raise Mismatch(dict(call="count_lines above 2^32", got=lines, want=lines_per_period * periods, pattern=text, start=start, length=length))
                assert start + length - 7 * 9000 > 1 << 32, "the buffer must be larger than 4 GiB"
                tail = hay[start + length - 7 * 9000:start + length]
                tb, te = rule_runs(tail.cpu().numpy(), row, lo, hi)
                (bbuf, bview), (ebuf, eview) = window(tb.size + 1), window(tb.size + 1)
                total = pat.find_all_into(tail, bview, eview, tb.size + 1)
                b, e = pat.find_all(dev, capacity=2 * per_period)
                stats["calls"] += 2
                want_first = [s for k in range(2) for s in ([(x + 7 * k, y + 7 * k) for x, y in spans])][:2 * per_period]
                if total != tb.size or not held(bbuf, tb, tb.size + 1) or not held(ebuf, te, tb.size + 1) or \
                        list(zip(b.cpu().tolist(), e.cpu().tolist())) != want_first:
                    raise Mismatch(dict(call="find_all above 2^32", pattern=text, bitmap=bitmap, start=start))
    stats["large_gib"] = gib
    del hay
    torch.cuda.empty_cache()


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
    rng = np.random.default_rng(seed)
    stats = {"fuzz": "runs", "seed": seed, "seconds": seconds, "cases": 0, "views": 0, "calls": 0, "runs": 0, "by_ranges": {}, "large_gib": 0,
             "mismatches": 0}
    ctx = _loaded() if getattr(ss.lib(), "has_runs", False) else ss.runs_build()
    with ctx:
        try:
            if gib:
                large_cases(rng, gib, stats)
            t0 = time.time()
            while time.time() - t0 < seconds:
                one_case(rng, stats)
        except Mismatch as m:
            stats["mismatches"] = 1
            stats["reproducer"] = m.args[0]
            print(json.dumps(stats))
            sys.exit(1)
    stats["by_ranges"] = dict(sorted(stats["by_ranges"].items()))
    print(json.dumps(stats))


if __name__ == "__main__":
    main()
