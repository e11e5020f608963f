#!/usr/bin/env python3
"""Randomised differential test of the grouping calls (include/sliceslice_hip_groups.h) on the GPU against THE RULE restated in
Python below: ss_group_ranges_device, ss_group_runs_device and ss_group_lines_device.
    python tools/fuzz_groups.py SECONDS SEED [GIB]

Tokens are the runs of a set drawn from fuzz_runs.py's pool (fuzz_classes.py's random_set) on fuzz_masked.py's haystacks, so that
few distinct keys of every length occur; range lists are those tokens, random ranges - overlapping, repeated, descending, reaching
beyond the view - and lists with runs of equal keys laid around the 4,096-range block borders.  Both flags, capacities that cut the
rows, arrays left out, windows of larger buffers whose sentinels on both sides must survive.  With GIB (a size in GiB above 4) one
buffer of that size is filled with a short period and keys above offset 2^32 are grouped.
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
from fuzz_masked import Mismatch, _loaded, held, random_haystack, window  # noqa: E402
from fuzz_runs import rule_runs  # noqa: E402

BLOCK = 4096


def rule_groups(data, begin, end, fold):
    """(first, count, group): the key of range k is data[b:e], e = min(end, len), b = min(begin, e); groups in first-member order"""
    n = len(data)
    index, first, count, group = {}, [], [], []
    for k, (b, e) in enumerate(zip(begin, end)):
        e = min(int(e), n)
        b = min(int(b), e)
        key = data[b:e].lower() if fold else data[b:e]
        j = index.setdefault(key, len(first))
        if j == len(first):
            first.append(k)
            count.append(0)
        count[j] += 1
        group.append(j)
    return np.array(first, dtype=np.int64), np.array(count, dtype=np.int64), np.array(group, dtype=np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64).view(np.int64))).cuda()


def check_ranges(rng, stats, view, data, begin, end, where):
    fold, weak = bool(rng.integers(0, 2)), bool(rng.integers(0, 4) == 0) and len(begin) <= 8000
    first, count, group = rule_groups(data, begin, end, fold)
    g, n = first.size, len(begin)
    cap = int(rng.choice([0, 1, max(g - 1, 0), g, g + 1, int(rng.integers(0, g + 2))]))
    w = [window(max(cap, 1)), window(max(cap, 1)), window(n + 1)]
    leave = int(rng.integers(0, 5))                                 # the array left out (3, 4: none)
    p = [None if k == leave else w[k][1] for k in range(3)]
    got = ss.group_ranges_into(view, dev(begin), dev(end), p[0], p[1], p[2], capacity=cap, ignore_case=fold, weak_hash=weak)
    stats["calls"] += 1
    stats["ranges"] += n
    if got != g or not (held(w[0][0], first, 0 if p[0] is None else cap) and held(w[1][0], count, 0 if p[1] is None else cap) and
                        held(w[2][0], group, 0 if p[2] is None else n + 1)):
        raise Mismatch(dict(call="ranges", got=got, want=int(g), cap=cap, leave=leave, fold=fold, weak=weak, n=n, **where))


def one_case(rng, stats):
    size = int(rng.choice([600, 5000, 20000, 60000], p=[.4, .3, .2, .1]))
    host = random_haystack(rng, size + 32)
    row = random_set(rng, host)
    words = sets_of(row)[0]
    buf = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16
    buf[at:at + host.size].copy_(torch.from_numpy(host))
    mis = stats["cases"] % 16                                       # (every misalignment in turn)
    length = size if rng.integers(0, 3) else int(rng.integers(0, size + 1))
    view, hv = buf[at + mis:at + mis + length], host[mis:mis + length]
    data = hv.tobytes()
    where = dict(set=[int(x) for x in words], mis=mis, length=length)
    # the tokens of the set: the range call on them, and the run form in one call
    tb, te = rule_runs(hv, row, 1, None)
    check_ranges(rng, stats, view, data, tb.tolist(), te.tolist(), dict(kind="tokens", **where))
    fold = bool(rng.integers(0, 2))
    first, count, _ = rule_groups(data, tb.tolist(), te.tolist(), fold)
    g = first.size
    cap = int(rng.choice([0, g, g + 1, int(rng.integers(0, g + 2))]))
    w = [window(max(cap, 1)) for _ in range(3)]
    pat = ss.RunPattern.from_set(words)
    got = pat.groups_into(view, w[0][1], w[1][1], w[2][1], cap, fold, weak_hash=bool(rng.integers(0, 4) == 0) and tb.size <= 8000)
    stats["calls"] += 1
    if got != (g, tb.size) or not (held(w[0][0], tb[first], cap) and held(w[1][0], te[first], cap) and held(w[2][0], count, cap)):
        raise Mismatch(dict(call="runs", got=list(got), want=[int(g), int(tb.size)], cap=cap, fold=fold, **where))
    # the lines
    delimiter = int(rng.choice([10, 0, int(host[rng.integers(0, host.size)])]))
    stops = np.flatnonzero(hv == delimiter)
    if hv.size and hv[-1] != delimiter:
        stops = np.append(stops, hv.size)
    starts = np.concatenate(([0], stops[:-1] + 1)) if stops.size else stops
    # (the fold never touches the delimiter: it cuts the lines before keys are compared)
    first, count, _ = rule_groups(data, starts.tolist(), stops.tolist(), fold)
    g = first.size
    cap = int(rng.choice([0, g, g + 1, int(rng.integers(0, g + 2))]))
    w = [window(max(cap, 1)) for _ in range(4)]
    got = ss.group_lines_into(view, w[0][1], w[1][1], w[2][1], w[3][1], cap, bytes([delimiter]), fold)
    stats["calls"] += 1
    if got != (g, stops.size) or not (held(w[0][0], starts[first], cap) and held(w[1][0], stops[first], cap) and held(w[2][0], first + 1, cap) and
                                      held(w[3][0], count, cap)):
        raise Mismatch(dict(call="lines", got=list(got), want=[int(g), int(stops.size)], cap=cap, fold=fold, delimiter=delimiter, **where))
    # random ranges: overlapping, repeated, descending, beyond the view
    n = int(rng.choice([0, 1, 7, 300, 5000]))
    begin = rng.integers(0, length + 4, n)
    end = begin + rng.choice([0, 1, 2, 3, 5, 17, 130, 300], n) - rng.integers(0, 2, n) * 3
    begin, end = np.maximum(begin, 0).tolist(), np.maximum(end, 0).tolist()
    check_ranges(rng, stats, view, data, begin, end, dict(kind="random", **where))
    # runs of equal keys around the block borders: a list of 2 or 3 blocks whose keys change at, one before and one behind a border
    if tb.size >= 2 and stats["cases"] % 4 == 0:
        n = BLOCK * int(rng.integers(2, 4)) + int(rng.integers(-2, 3))
        cuts = sorted({0, n} | {min(max(BLOCK * j + d, 0), n) for j in (1, 2, 3) for d in (-1, 0, 1, int(rng.integers(-70, 70)))})
        pick = np.zeros(n, dtype=np.int64)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            pick[lo:hi] = rng.integers(0, min(tb.size, 6))
        check_ranges(rng, stats, view, data, tb[pick].tolist(), te[pick].tolist(), dict(kind="borders", n=n, **where))
    stats["cases"] += 1


def large_cases(rng, gib, stats):
    """keys above offset 2^32: a buffer with a period of 8 bytes, `ab cd ab`; the words of its tail and ranges spread over all of it"""
    size = int(gib * (1 << 30))
    assert size > (1 << 32) + (1 << 20), "the buffer must be larger than 4 GiB"
    period = np.frombuffer(b"ab cd Ab", dtype=np.uint8)
    hay = torch.from_numpy(period.copy()).cuda().repeat(size // 8 + 1)[:size].contiguous()
    periods = size // 8
    picks = np.concatenate((rng.integers(0, periods, 3000), np.arange(periods - 3000, periods)))
    begin = np.concatenate((picks * 8, picks * 8 + 3, picks * 8 + 6))
    end = begin + 2
    for fold in (False, True):
        for weak in (False, True):
            f, c, g = ss.group_ranges(hay, dev(begin), dev(end), ignore_case=fold, want_group=True, weak_hash=weak)
            stats["calls"] += 1
            want_first = [0, picks.size] + ([] if fold else [2 * picks.size])
            want_count = [2 * picks.size, picks.size] if fold else [picks.size] * 3
            want_group = np.repeat([0, 1, 0 if fold else 2], picks.size)
            if f.cpu().tolist() != want_first or c.cpu().tolist() != want_count or not np.array_equal(g.cpu().numpy(), want_group):
                raise Mismatch(dict(call="ranges above 2^32", fold=fold, weak=weak, first=f.cpu().tolist(), count=c.cpu().tolist()))
    tail = hay[size - 8 * 4000:]
    assert size - 8 * 4000 > 1 << 32
    b, e, c = ss.RunPattern(r"\w+").groups(tail)
    stats["calls"] += 1
    shift = (size - 8 * 4000) % 8                                   # (the tail begins inside a period)
    data = tail.cpu().numpy().tobytes()
    word = np.array([48 <= x <= 57 or 65 <= x <= 90 or 97 <= x <= 122 or x == 95 for x in range(256)])
    tb, te = rule_runs(np.frombuffer(data, dtype=np.uint8), word, 1, None)
    first, count, _ = rule_groups(data, tb.tolist(), te.tolist(), False)
    if b.cpu().tolist() != tb[first].tolist() or e.cpu().tolist() != te[first].tolist() or c.cpu().tolist() != count.tolist():
        raise Mismatch(dict(call="runs above 2^32", shift=shift))
    stats["large_gib"] = gib
    del hay
    torch.cuda.empty_cache()


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
    rng = np.random.default_rng(seed)
    stats = {"fuzz": "groups", "seed": seed, "seconds": seconds, "cases": 0, "calls": 0, "ranges": 0, "large_gib": 0, "mismatches": 0}
    ctx = _loaded() if getattr(ss.lib(), "has_groups", False) else ss.groups_build()
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
    print(json.dumps(stats))


if __name__ == "__main__":
    main()
