#!/usr/bin/env python3
"""Randomised differential test of the byte-class calls (include/sliceslice_hip_classes.h) on the GPU against THE RULE restated in
numpy below: ss_count_classes_device, ss_find_all_classes_device, ss_count_lines_classes_device and ss_find_lines_classes_device.
    python tools/fuzz_classes.py SECONDS SEED [GIB]

Haystacks are fuzz_masked.py's.  Patterns of 1 .. 4,096 positions (mostly short) whose sets are drawn from a pool made per case:
single values cut from the view, exact masks, ranges, unions of ranges, negated singles, `.` and random sets, the pool sized so that
the limit of 64 distinct inexact sets is met and sometimes exceeded (such a pattern must be refused with the limit's name, and so
must one with more than 1,024 inexact positions).  Views at every misalignment and of every length around the pattern's, and
around the 16 B, 1 KiB, 4 KiB, 16 KiB and 128 KiB borders; the find calls write into windows of larger buffers whose sentinels on
both sides must survive, at capacities that cut the list.  Delimiters: a newline, zero, a byte of the text.  With GIB (a size in
GiB above 4) one buffer of that size is filled with a short period so that a dense pattern has occurrences everywhere, and views
that END above offset 2^32 are checked against the period's arithmetic and, near the end, numpy.
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
from fuzz_masked import BORDERS, Mismatch, _loaded, held, random_haystack, window  # noqa: E402


def members(sets):
    return np.unpackbits(np.ascontiguousarray(sets, dtype="<u8").view(np.uint8).reshape(-1, 32), axis=1, bitorder="little").astype(bool)


def sets_of(table):
    return np.ascontiguousarray(np.packbits(np.asarray(table, dtype=bool).reshape(-1, 256), axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(-1, 4)


def rule_offsets(data, table):
    n = len(table)
    if data.size < n:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(data.size - n + 1, dtype=bool)
    for i in range(n):
        if not table[i].all():
            ok &= table[i][data[i:data.size - n + 1 + i]]
    return np.flatnonzero(ok).astype(np.int64)


def rule_lines(data, table, delimiter):
    n, offs = len(table), rule_offsets(data, table)
    delims = np.flatnonzero(data == delimiter).astype(np.int64)
    ends = np.append(delims, data.size) if (delims.size == 0 or delims[-1] != data.size - 1) and data.size else delims
    begins = np.concatenate([[0], delims + 1])[:ends.size]
    if ends.size == 0:
        return begins, ends, ends
    line = np.searchsorted(ends, offs, side="left")
    sel = np.unique(line[offs + n <= ends[np.minimum(line, ends.size - 1)]])
    return begins[sel], ends[sel], sel + 1


def random_set(rng, host, inexact_only=False):
    """one row of 256 bools; inexact_only: a union of ranges or half of all values, which no (value, mask) pair accepts exactly"""
    row = np.zeros(256, dtype=bool)
    kind = rng.choice([3, 7]) if inexact_only else rng.integers(0, 8)
    seen = int(host[rng.integers(0, host.size)])
    if kind == 0:
        row[seen] = True                                            # a single value of the view
    elif kind == 1:
        m = int(rng.choice([0xDF, 0xF0, 0x0F, 0xFE, 0x7F]))
        row[(np.arange(256) & m) == (seen & m)] = True             # an exact mask
    elif kind == 2:
        lo = max(0, seen - int(rng.integers(0, 12)))
        row[lo:min(256, lo + int(rng.integers(2, 30)))] = True     # a range around a byte of the view
    elif kind == 3:
        for _ in range(int(rng.integers(2, 4))):                    # a union of ranges
            lo = int(rng.integers(0, 250))
            row[lo:lo + int(rng.integers(1, 20))] = True
        row[seen] = True
    elif kind == 4:
        row[:] = True
        row[int(host[rng.integers(0, host.size)])] = False         # a negated single
    elif kind == 5:
        row[:] = True                                               # `.`
    elif kind == 6:
        row[rng.integers(0, 256, int(rng.integers(1, 6)))] = True   # a few values
        row[seen] = True
    else:
        row = rng.integers(0, 2, 256).astype(bool)                  # half of all values
        row[seen] = True
    return row


def inexact_rows(table):
    cover_bits = np.zeros(len(table), dtype=np.int64)
    for i, row in enumerate(table):
        values = np.flatnonzero(row)
        cover_bits[i] = bin(int(np.bitwise_or.reduce(values ^ values[0]))).count("1")
    return table.sum(axis=1) != (1 << cover_bits)


def random_pattern(rng, host):
    n = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 18, 31, 33, 64, 100, 257, 1000, 4096],
                       p=[.08, .1, .12, .1, .08, .06, .06, .05, .05, .05, .05, .04, .04, .04, .03, .02, .02, .01]))
    size = int(rng.choice([1, 2, 4, 8, 40, 64, 66, 90], p=[.15, .2, .25, .2, .08, .04, .04, .04]))
    if size >= 40:                                                  # at, around and beyond the limit of 64 distinct inexact sets
        n = int(rng.choice([257, 1000]))
        pool = np.array([random_set(rng, host, inexact_only=True) for _ in range(size)])
        table = pool[rng.integers(0, size, n)]
        table[:size] = pool                                         # (every set of the pool stands somewhere)
        return table
    pool = np.array([random_set(rng, host) for _ in range(size)])
    table = pool[rng.integers(0, size, n)]
    if n > 64 and rng.integers(0, 3):                               # long patterns: mostly `.`, so that the limits are usually met
        table[rng.random(n) < 0.8] = True
    return table


def one_case(rng, stats):
    size = int(rng.choice([600, 5000, 20000, 140000, 280000], p=[.3, .3, .2, .1, .1]))
    host = random_haystack(rng, size + 32)
    table = random_pattern(rng, host)
    n = len(table)
    if n >= 257 and size > 20000:                                   # (the numpy rule costs n passes over the view)
        size, host = 20000, host[:20032]
    inexact = inexact_rows(table)
    distinct = len({row.tobytes() for row in table[inexact]})
    try:
        pat = ss.ClassPattern.from_sets(sets_of(table))
    except ss.SlicesliceError as e:
        limit = "SS_CLASSES_MAX_INEXACT" if inexact.sum() > 1024 else "SS_CLASSES_MAX_DISTINCT" if distinct > 64 else None
        if limit is None or e.code != ss.SS_ERR_ARGUMENT or limit not in str(e):
            raise Mismatch(dict(call="new", error=str(e), n=n, inexact=int(inexact.sum()), distinct=distinct))
        stats["refused_" + limit[11:].lower()] += 1
        return host
    info = pat.info()
    if (info["inexact"], info["distinct"]) != (int(inexact.sum()), distinct) or inexact.sum() > 1024 or distinct > 64:
        raise Mismatch(dict(call="info", info=info, inexact=int(inexact.sum()), distinct=distinct))
    stats["by_distance"][str(info["distance"])] = stats["by_distance"].get(str(info["distance"]), 0) + 1
    stats["max_distinct"] = max(stats["max_distinct"], distinct)
    stats["max_inexact"] = max(stats["max_inexact"], int(inexact.sum()))
    buf = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16
    buf[at:at + host.size].copy_(torch.from_numpy(host))
    views = [(stats["cases"] % 16, size)]                           # (every misalignment in turn)
    for _ in range(3):
        mis = int(rng.integers(0, 16))
        pick = rng.integers(0, 3)
        if pick == 0:
            length = max(0, n + int(rng.integers(-1, 3)))
        elif pick == 1:
            b = int(rng.choice(BORDERS))
            length = max(0, b * int(rng.integers(1, 3)) - mis + int(rng.integers(-n - 1, n + 2)))
        else:
            length = int(rng.integers(0, size + 1))
        views.append((mis, min(length, size)))
    where = dict(sets=[int(x) for x in sets_of(table).ravel()] if n <= 8 else "n=%d" % n)
    for mis, length in views:
        dev, hv = buf[at + mis:at + mis + length], host[mis:mis + length]
        want = rule_offsets(hv, table)
        got = pat.count(dev)
        stats["calls"] += 1
        if got != want.size:
            raise Mismatch(dict(call="count", got=got, want=int(want.size), mis=mis, length=length, **where))
        cap = int(rng.choice([0, 1, max(want.size - 1, 0), want.size, want.size + 1, int(rng.integers(0, want.size + 2))]))
        wbuf, wview = window(max(cap, 1))
        total = pat.find_all_into(dev, wview if cap else None, cap)
        stats["calls"] += 1
        if total != want.size or not held(wbuf, want, cap):
            raise Mismatch(dict(call="find_all", total=total, want=int(want.size), cap=cap, mis=mis, length=length, **where))
        delimiter = int(rng.choice([10, 0, int(hv[rng.integers(0, hv.size)]) if hv.size else 10]))
        begin, end, number = rule_lines(hv, table, delimiter)
        got = pat.count_lines(dev, bytes([delimiter]))
        stats["calls"] += 1
        if got != begin.size:
            raise Mismatch(dict(call="count_lines", got=got, want=int(begin.size), delimiter=delimiter, mis=mis, length=length, **where))
        cap = int(rng.choice([1, begin.size, begin.size + 1, int(rng.integers(0, begin.size + 2))]))
        w = [window(max(cap, 1)) for _ in range(3)]
        total = pat.find_lines_into(dev, w[0][1], w[1][1], w[2][1], cap, bytes([delimiter]))
        stats["calls"] += 1
        if total != begin.size or not all(held(w[k][0], x, cap) for k, x in enumerate((begin, end, number))):
            raise Mismatch(dict(call="find_lines", total=total, want=int(begin.size), cap=cap, delimiter=delimiter, mis=mis, length=length, **where))
        stats["views"] += 1
    stats["cases"] += 1
    return host


def large_cases(rng, gib, stats):
    """dense occurrences above offset 2^32: a buffer of a period of 7 bytes (one line each), patterns that occur at fixed phases of it;
    the views begin at a line's first byte and end behind a delimiter, so that counts and lines follow by arithmetic"""
    size = int(gib * (1 << 30))
    period = np.frombuffer(b"abcabd\n", dtype=np.uint8)
    hay = torch.from_numpy(period.copy()).cuda().repeat(size // 7 + 1)[:size].contiguous()
    for text, lines_per_period in ((r"[a-b][b-c].", 1), (r"[^\n]b[cd]", 1), (r"[c-e]\s", 0), (r"\w", 1), (r"[ac][^a]", 1)):
        pat = ss.ClassPattern(text)
        table = members(pat.sets)
        n = len(table)
        phases = [p for p in range(7) if all(table[i][period[(p + i) % 7]] for i in range(n))]
        per_line = [p for p in phases if p + n <= 6]                # (occurrences that hold no delimiter)
        assert bool(per_line) == bool(lines_per_period)
        for start in (0, 7, 21):                                    # misalignments 0, 7 and 5
            periods = (size - start) // 7 - int(rng.integers(0, 5))
            length = 7 * periods
            dev = hay[start:start + length]
            want = sum(len(range(ph, length - n + 1, 7)) for ph in phases)
            got = pat.count(dev)
            stats["calls"] += 1
            if got != want:
                raise Mismatch(dict(call="count above 2^32", got=got, want=want, pattern=text, start=start, length=length))
            lines = pat.count_lines(dev)
            stats["calls"] += 1
            if lines != lines_per_period * periods:
                raise Mismatch(dict(call="count_lines above 2^32", got=lines, want=lines_per_period * periods, pattern=text, start=start, length=length))
            first = pat.find_all(dev, capacity=len(phases) * 2).cpu().numpy()
            tail = hay[start + length - 7 * 9000:start + length]
            assert start + length - 7 * 9000 > 1 << 32, "the buffer must be larger than 4 GiB"
            tw = rule_offsets(tail.cpu().numpy(), table)
            wbuf, wview = window(tw.size + 1)
            total = pat.find_all_into(tail, wview, tw.size + 1)
            stats["calls"] += 2
            if total != tw.size or not held(wbuf, tw, tw.size + 1) or first.tolist() != sorted(phases + [p + 7 for p in phases]):
                raise Mismatch(dict(call="find_all above 2^32", pattern=text, start=start, first=first.tolist()))
            if lines_per_period:
                w = [window(4) for _ in range(3)]
                short = hay[start + length - 7 * 3:start + length]
                total = pat.find_lines_into(short, w[0][1], w[1][1], w[2][1], 4)
                stats["calls"] += 1
                if total != 3 or not held(w[0][0], np.array([0, 7, 14]), 4) or not held(w[1][0], np.array([6, 13, 20]), 4):
                    raise Mismatch(dict(call="find_lines above 2^32", pattern=text, start=start))
    stats["large_gib"] = gib
    del hay
    torch.cuda.empty_cache()


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
    rng = np.random.default_rng(seed)
    stats = {"fuzz": "classes", "seed": seed, "seconds": seconds, "cases": 0, "views": 0, "calls": 0, "refused_max_inexact": 0,
             "refused_max_distinct": 0, "max_inexact": 0, "max_distinct": 0, "by_distance": {}, "large_gib": 0, "mismatches": 0}
    ctx = _loaded() if getattr(ss.lib(), "has_classes", False) else ss.classes_build()
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
    stats["by_distance"] = dict(sorted(stats["by_distance"].items(), key=lambda kv: int(kv[0])))
    print(json.dumps(stats))


if __name__ == "__main__":
    main()
