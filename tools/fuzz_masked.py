#!/usr/bin/env python3
"""Randomised differential test of the masked-pattern calls (include/sliceslice_hip_masked.h) on the GPU against THE RULE restated in
numpy below: ss_count_masked_device, ss_find_all_masked_device, ss_count_lines_masked_device and ss_find_lines_masked_device.
    python tools/fuzz_masked.py SECONDS SEED [GIB]

Haystacks: random bytes, two and three letters (uniform and with long runs), text with delimiters.  Patterns of 1 .. 4,096 bytes
(mostly short) cut from the view or drawn at random, with masks of 0xFF, 0x00, nibbles, the letter mask and random bits in random
proportions, so that both filter distances up to 16 and single filter bytes occur.  Views at every misalignment and of every
length around the pattern's, and around the 16 B, 1 KiB, 4 KiB, 16 KiB and 128 KiB borders; the find calls write into windows of
larger buffers whose sentinels on both sides must survive, at capacities that cut the list.  Delimiters: a newline, zero, a letter
of the text.  With GIB (a size in GiB above 4) one buffer of that size is filled with a short period so that a dense pattern has
occurrences everywhere, and views that END above offset 2^32 are checked against the period's arithmetic and, near the end, numpy.
Prints one JSON line; on the first mismatch a reproducer and exit 1."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sliceslice_rs_amd as ss  # noqa: E402

SENT64 = -0x5A5A5A5A5A5A5A5B
GUARD = 64
BORDERS = (16, 1024, 4096, 16384, 131072)


class Mismatch(Exception):
    pass


class _loaded:
    """the library SLICESLICE_HIP_LIB loaded, where it has the entry points"""
    def __enter__(self):
        return ss.lib()

    def __exit__(self, *a):
        return False


def rule_offsets(data, value, mask):
    n = len(value)
    if data.size < n:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(data.size - n + 1, dtype=bool)
    for i, (v, m) in enumerate(zip(value, mask)):
        if m:
            ok &= (data[i:data.size - n + 1 + i] & m) == (v & m)
    return np.flatnonzero(ok).astype(np.int64)


def rule_lines(data, value, mask, delimiter):
    n, offs = len(value), rule_offsets(data, value, mask)
    delims = np.flatnonzero(data == delimiter).astype(np.int64)
    ends = np.append(delims, data.size) if (delims.size == 0 or delims[-1] != data.size - 1) and data.size else delims
    begins = np.concatenate([[0], delims + 1])[:ends.size]
    if ends.size == 0:
        return begins, ends, ends
    line = np.searchsorted(ends, offs, side="left")
    sel = np.unique(line[offs + n <= ends[np.minimum(line, ends.size - 1)]])
    return begins[sel], ends[sel], sel + 1


def window(cap):
    buf = torch.full((cap + 2 * GUARD,), SENT64, dtype=torch.int64, device="cuda")
    return buf, buf[GUARD:GUARD + cap]


def held(buf, want, cap):
    h = buf.cpu().numpy()
    k = min(len(want), cap)
    return (h[:GUARD] == SENT64).all() and (h[GUARD + k:] == SENT64).all() and (h[GUARD:GUARD + k] == want[:k]).all()


def random_haystack(rng, size):
    kind = rng.integers(0, 5)
    if kind == 0:
        return rng.integers(0, 256, size, dtype=np.uint8)
    letters = np.frombuffer((b"ab", b"abc", b"ab\n", b"a\x00b ", b"the \nTHE")[rng.integers(0, 5)], dtype=np.uint8)
    if kind in (1, 2):
        return rng.choice(letters, size)
    runs = np.repeat(rng.choice(letters, size // 5 + 1), rng.integers(1, 11, size // 5 + 1))
    return np.ascontiguousarray(np.resize(runs, size))


def random_pattern(rng, host):
    n = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 18, 31, 33, 64, 100, 257, 1000, 4096],
                       p=[.08, .1, .12, .1, .08, .06, .06, .05, .05, .05, .05, .04, .04, .04, .03, .02, .02, .01]))
    if host.size > n and rng.integers(0, 4):
        at = int(rng.integers(0, host.size - n))
        value = host[at:at + n].copy()
    else:
        value = rng.integers(0, 256, n, dtype=np.uint8)
    style = rng.integers(0, 5)
    if style == 0:
        mask = np.full(n, 0xFF, dtype=np.uint8)
    elif style == 1:
        mask = rng.choice(np.array([0xFF, 0x00], dtype=np.uint8), n, p=[.3, .7])
    elif style == 2:
        mask = rng.choice(np.array([0xFF, 0x00, 0xF0, 0x0F, 0xDF], dtype=np.uint8), n)
    elif style == 3:
        mask = np.zeros(n, dtype=np.uint8)
        mask[rng.integers(0, n, min(n, int(rng.integers(0, 3))))] = 0xFF
    else:
        mask = rng.integers(0, 256, n, dtype=np.uint8)
    return value.tobytes(), mask.tobytes()


def one_case(rng, stats):
    size = int(rng.choice([600, 5000, 20000, 140000, 280000], p=[.3, .3, .2, .1, .1]))
    host = random_haystack(rng, size + 32)
    value, mask = random_pattern(rng, host)
    n = len(value)
    pat = ss.MaskedPattern(value, mask)
    info = pat.info()
    stats["by_distance"][str(info["distance"])] = stats["by_distance"].get(str(info["distance"]), 0) + 1
    buf = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16
    buf[at:at + host.size].copy_(torch.from_numpy(host))
    views = [(int(rng.integers(0, 16)), size)]
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
    for mis, length in views:
        dev, hv = buf[at + mis:at + mis + length], host[mis:mis + length]
        want = rule_offsets(hv, pat.value, pat.mask)
        got = pat.count(dev)
        stats["calls"] += 1
        if got != want.size:
            raise Mismatch(dict(call="count", got=got, want=int(want.size), value=value.hex(), mask=mask.hex(), mis=mis, length=length))
        cap = int(rng.choice([0, 1, max(want.size - 1, 0), want.size, want.size + 1, int(rng.integers(0, want.size + 2))]))
        wbuf, wview = window(max(cap, 1))
        total = pat.find_all_into(dev, wview if cap else None, cap)
        stats["calls"] += 1
        if total != want.size or not held(wbuf, want, cap):
            raise Mismatch(dict(call="find_all", total=total, want=int(want.size), cap=cap, value=value.hex(), mask=mask.hex(), mis=mis, length=length))
        delimiter = int(rng.choice([10, 0, int(hv[rng.integers(0, hv.size)]) if hv.size else 10]))
        begin, end, number = rule_lines(hv, pat.value, pat.mask, delimiter)
        got = pat.count_lines(dev, bytes([delimiter]))
        stats["calls"] += 1
        if got != begin.size:
            raise Mismatch(dict(call="count_lines", got=got, want=int(begin.size), delimiter=delimiter, value=value.hex(), mask=mask.hex(), mis=mis, length=length))
        cap = int(rng.choice([1, begin.size, begin.size + 1, int(rng.integers(0, begin.size + 2))]))
        w = [window(max(cap, 1)) for _ in range(3)]
        total = pat.find_lines_into(dev, w[0][1], w[1][1], w[2][1], cap, bytes([delimiter]))
        stats["calls"] += 1
        if total != begin.size or not all(held(w[k][0], x, cap) for k, x in enumerate((begin, end, number))):
            raise Mismatch(dict(call="find_lines", total=total, want=int(begin.size), cap=cap, delimiter=delimiter, value=value.hex(), mask=mask.hex(),
                                mis=mis, length=length))
        stats["views"] += 1
    stats["cases"] += 1
    return host


def large_cases(rng, gib, stats):
    """dense occurrences above offset 2^32: a buffer of a period of 7 bytes (one line each), patterns that occur at fixed phases of it;
    the views begin at a line's first byte and end behind a delimiter, so that counts and lines follow by arithmetic"""
    size = int(gib * (1 << 30))
    period = np.frombuffer(b"abcabd\n", dtype=np.uint8)
    hay = torch.from_numpy(period.copy()).cuda().repeat(size // 7 + 1)[:size].contiguous()
    for text, lines_per_period in (("61 62 ??", 1), ("?? 62 64", 1), ("64 0a", 0), ("??", 1)):
        pat = ss.MaskedPattern.from_hex(text)
        n = len(pat.value)
        phases = [p for p in range(7) if all((period[(p + i) % 7] & pat.mask[i]) == pat.value[i] for i in range(n))]
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
            # the first offsets, and the last ones through a view that lies wholly above 2^32
            first = pat.find_all(dev, capacity=len(phases) * 2).cpu().numpy()
            tail = hay[start + length - 7 * 9000:start + length]
            assert start + length - 7 * 9000 > 1 << 32, "the buffer must be larger than 4 GiB"
            tw = rule_offsets(tail.cpu().numpy(), pat.value, pat.mask)
            wbuf, wview = window(tw.size + 1)
            total = pat.find_all_into(tail, wview, tw.size + 1)
            stats["calls"] += 2
            if total != tw.size or not held(wbuf, tw, tw.size + 1) or first.tolist() != sorted(phases + [p + 7 for p in phases]):
                raise Mismatch(dict(call="find_all above 2^32", pattern=text, start=start, first=first.tolist()))
            # ... and the LAST offsets of the whole view, whose values exceed 2^32: the capacity holds everything only for the sparse patterns,
            # so the records of the last lines stand in for them
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
    stats = {"fuzz": "masked", "seed": seed, "seconds": seconds, "cases": 0, "views": 0, "calls": 0, "by_distance": {}, "large_gib": 0, "mismatches": 0}
    ctx = _loaded() if getattr(ss.lib(), "has_masked", False) else ss.masked_build()
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
