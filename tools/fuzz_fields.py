#!/usr/bin/env python3
"""Randomised differential test of the field calls (include/sliceslice_hip_fields.h) on the GPU against THE RULE restated in numpy
below: ss_count_fields_device and ss_find_fields_device.
    python tools/fuzz_fields.py SECONDS SEED [GIB]

Separator sets are drawn from fuzz_runs.py's pool (fuzz_classes.py's random_set); haystacks are fuzz_masked.py's, or bytes that are
separators and delimiters with probabilities drawn per case, so that lines and fields of every length occur.  Both modes, with and
without KEEP_SHORT; `first` and `last` around 1, 2, 16, 17 and at random, `last` equal to `first`, open and above it; delimiters: a
newline, zero, a byte of the text.  Views at every misalignment and around the 16 B, 1 KiB, 4 KiB, 16 KiB and 128 KiB borders; the
find call writes into windows of larger buffers whose sentinels on both sides must survive, at capacities that cut the list, with
arrays left out.  With GIB (a size in GiB above 4) one buffer of that size is filled with a short period, and views that END above
offset 2^32 are checked against the period's arithmetic and, near the end, numpy.
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

NUMBERS = [1, 2, 3, 15, 16, 17, 18, 33]


def rule_fields(a, row, merge, first, last, keep, delimiter):
    """(begin, end, number, lines): `row` is the separator set as 256 booleans"""
    n = a.size
    empty = np.zeros(0, dtype=np.int64)
    if n == 0:
        return empty, empty, empty, 0
    row = row.copy()
    row[delimiter] = False
    isd, sep = a == delimiter, row[a]
    stop = np.flatnonzero(isd)
    if not isd[-1]:
        stop = np.append(stop, n)
    start = np.concatenate(([0], stop[:-1] + 1))
    line_of = np.cumsum(isd) - isd
    begin, end = np.full(stop.size, -1, dtype=np.int64), stop.astype(np.int64).copy()

    def ordinals(mask):
        at = np.flatnonzero(mask)
        before = np.concatenate(([0], np.cumsum(mask)))
        return at, line_of[at], before[at] - before[start[line_of[at]]], before[stop] - before[start]

    if not merge:
        at, line, k, count = ordinals(sep)
        fields = count + 1
        if first == 1:
            begin[:] = start
        else:
            begin[line[k == first - 2]] = at[k == first - 2] + 1
        if last:
            end[line[k == last - 1]] = at[k == last - 1]
    else:
        field = ~sep & ~isd
        at, line, k, fields = ordinals(field & ~np.concatenate(([False], field[:-1])))
        begin[line[k == first - 1]] = at[k == first - 1]
        if last:
            at, line, k, _ = ordinals(field & ~np.concatenate((field[1:], [False])))
            end[line[k == last - 1]] = at[k == last - 1] + 1
    selected = fields >= first
    number = np.arange(1, stop.size + 1, dtype=np.int64)
    if keep:
        return np.where(selected, begin, stop).astype(np.int64), np.where(selected, end, stop).astype(np.int64), number, stop.size
    return begin[selected], end[selected], number[selected], stop.size


def random_selection(rng):
    first = int(rng.choice(NUMBERS)) if rng.integers(0, 4) else int(rng.integers(1, 200))
    pick = rng.integers(0, 3)
    last = first if pick == 0 else 0 if pick == 1 else first + int(rng.choice([1, 2, 15, 16, 100]))
    return first, last


def one_case(rng, stats):
    size = int(rng.choice([600, 5000, 20000, 140000, 280000], p=[.3, .3, .2, .1, .1]))
    host = random_haystack(rng, size + 32)
    row = random_set(rng, host)
    base_delim = int(rng.choice([10, 0, int(host[rng.integers(0, host.size)])]))
    if rng.integers(0, 2) and not row.all():                        # separators with probability p, delimiters with probability q
        p, q = float(rng.choice([0.5, 0.2, 0.05, 0.9, 0.002])), float(rng.choice([0.5, 0.05, 0.01, 0.0005]))
        inside, outside = np.flatnonzero(row).astype(np.uint8), np.flatnonzero(~row).astype(np.uint8)
        u = rng.random(size + 32)
        host = np.where(u < p, rng.choice(inside, size + 32), rng.choice(outside, size + 32)).astype(np.uint8)
        host[rng.random(size + 32) < q] = base_delim
    words = sets_of(row)[0]
    buf = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16
    buf[at:at + host.size].copy_(torch.from_numpy(host))
    views = [(stats["cases"] % 16, size)]                           # (every misalignment in turn)
    for _ in range(3):
        mis = int(rng.integers(0, 16))
        pick = rng.integers(0, 3)
        if pick == 0:
            length = int(rng.integers(0, 40))
        elif pick == 1:
            length = max(0, int(rng.choice(BORDERS)) * int(rng.integers(1, 3)) - mis + int(rng.integers(-3, 4)))
        else:
            length = int(rng.integers(0, size + 1))
        views.append((mis, min(length, size)))
    for mis, length in views:
        dev, hv = buf[at + mis:at + mis + length], host[mis:mis + length]
        for merge in (False, True):
            first, last = random_selection(rng)
            keep = bool(rng.integers(0, 2))
            delimiter = int(rng.choice([10, 0, base_delim]))
            where = dict(set=[int(x) for x in words], merge=merge, first=first, last=last, keep=keep, delimiter=delimiter, mis=mis, length=length)
            if row[delimiter] and row.sum() == 1:
                continue                                            # (refused: the set is only the delimiter)
            sel = ss.FieldSelector(words, first, last, merge=merge, keep_short=keep)
            begin, end, number, lines = rule_fields(hv, row, merge, first, last, keep, delimiter)
            selected = begin.size if not keep else rule_fields(hv, row, merge, first, last, False, delimiter)[0].size
            got = sel.count(dev, bytes([delimiter]))
            stats["calls"] += 1
            if got != (selected, lines):
                raise Mismatch(dict(call="count", got=list(got), want=[selected, lines], **where))
            n = begin.size
            cap = int(rng.choice([0, 1, max(n - 1, 0), n, n + 1, int(rng.integers(0, n + 2))]))
            w = [window(max(cap, 1)) for _ in range(3)]
            leave = int(rng.integers(0, 4)) if cap else 7           # the array left out (3: none); capacity 0: all three
            p = [None if (k == leave or leave == 7) else w[k][1] for k in range(3)]
            total = sel.find_into(dev, p[0], p[1], p[2], cap, bytes([delimiter]))
            stats["calls"] += 1
            if total != n or not all(held(w[k][0], x, 0 if p[k] is None else cap) for k, x in enumerate((begin, end, number))):
                raise Mismatch(dict(call="find", total=total, want=int(n), cap=cap, leave=leave, **where))
            stats["records"] += int(n)
        stats["views"] += 1
    stats["cases"] += 1


def large_cases(rng, gib, stats):
    """lines above offset 2^32: a buffer of a period of 8 bytes, one line `ab,c d\\n` each... counts follow by arithmetic, the last
    lines are compared with numpy"""
    size = int(gib * (1 << 30))
    period = np.frombuffer(b"ab,c  d\n", dtype=np.uint8)
    hay = torch.from_numpy(period.copy()).cuda().repeat(size // 8 + 1)[:size].contiguous()
    row = np.zeros(256, dtype=bool)
    row[[ord(","), ord(" ")]] = True
    words = sets_of(row)[0]
    # (merge, first, last, selected per line, the record of one line)
    for merge, first, last, per_line, span in ((False, 1, 1, 1, (0, 2)), (False, 2, 3, 1, (3, 5)), (False, 4, 0, 1, (6, 7)), (False, 5, 5, 0, None),
                                               (True, 2, 2, 1, (3, 4)), (True, 3, 0, 1, (6, 7)), (True, 4, 4, 0, None), (True, 1, 2, 1, (0, 4))):
        for keep in (False, True):
            sel = ss.FieldSelector(words, first, last, merge=merge, keep_short=keep)
            for start in (0, 8, 24):
                periods = (size - start) // 8 - int(rng.integers(0, 5))
                length = 8 * periods
                dev = hay[start:start + length]
                got = sel.count(dev)
                stats["calls"] += 1
                if got != (per_line * periods, periods):
                    raise Mismatch(dict(call="count above 2^32", got=list(got), want=[per_line * periods, periods], merge=merge, first=first, last=last))
                assert start + length - 8 * 9000 > 1 << 32, "the buffer must be larger than 4 GiB"
                tail = hay[start + length - 8 * 9000:start + length]
                tb, te, tn, _ = rule_fields(tail.cpu().numpy(), row, merge, first, last, keep, 10)
                w = [window(tb.size + 1) for _ in range(3)]
                total = sel.find_into(tail, w[0][1], w[1][1], w[2][1], tb.size + 1)
                b, e, n = sel.find(dev, capacity=2)
                stats["calls"] += 2
                if per_line:
                    want_first = [(span[0] + 8 * k, span[1] + 8 * k, k + 1) for k in range(2)]
                else:
                    want_first = [(7 + 8 * k, 7 + 8 * k, k + 1) for k in range(2)] if keep else []
                if total != tb.size or not all(held(w[k][0], x, tb.size + 1) for k, x in enumerate((tb, te, tn))) or \
                        list(zip(b.cpu().tolist(), e.cpu().tolist(), n.cpu().tolist())) != want_first:
                    raise Mismatch(dict(call="find above 2^32", merge=merge, first=first, last=last, keep=keep, start=start))
                # ... and the last records of the whole view: offsets and numbers above 2^32
                records = (periods if keep else per_line * periods)
                if records:
                    out = torch.empty((3, records), dtype=torch.int64, device="cuda")
                    total = sel.find_into(dev, out[0], out[1], out[2], records)
                    stats["calls"] += 1
                    k = periods - 1
                    want_last = (span[0] + 8 * k, span[1] + 8 * k, k + 1) if per_line else (7 + 8 * k, 7 + 8 * k, k + 1)
                    if total != records or tuple(out[:, -1].cpu().tolist()) != want_last:
                        raise Mismatch(dict(call="the last record above 2^32", merge=merge, first=first, last=last, keep=keep, start=start,
                                            got=out[:, -1].cpu().tolist(), want=list(want_last)))
                    del out
    stats["large_gib"] = gib
    del hay
    torch.cuda.empty_cache()


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
    rng = np.random.default_rng(seed)
    stats = {"fuzz": "fields", "seed": seed, "seconds": seconds, "cases": 0, "views": 0, "calls": 0, "records": 0, "large_gib": 0, "mismatches": 0}
    ctx = _loaded() if getattr(ss.lib(), "has_fields", False) else ss.fields_build()
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
