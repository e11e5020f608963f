#!/usr/bin/env python3
"""Randomised differential test of the rewrite call (include/sliceslice_hip_rewrite.h) on the GPU against `re.sub`:
ss_replace_runs_device.
    python tools/fuzz_rewrite.py SECONDS SEED [GIB]

Haystacks, sets and bounds are fuzz_runs.py's: every set is asked on BOTH paths (range tests where it has at most four ranges, the
bitmap forced), which must agree; lengths around 1, 16, 17, 32, 33 and 4,096, with and without a maximum.  The reference is Python's
`re`: the set becomes a character class [C] and the selection (?<![C])[C]{min,max}(?![C]), handed to re.sub; with a delimiter the
view is split at it, every piece substituted on its own and the pieces joined by it again.  Texts of 0 to 40 bytes and of 4,096;
delimiters -1, 10, 0 and a member of the set; the haystack at every misalignment in turn and the output at a random one; the output
is a window of a larger buffer whose sentinels on both sides must survive; capacities short by one write nothing and report both
numbers.  With GIB (a size in GiB above 4) one buffer of that size is filled with a short period and views that END above offset
2^32 are checked against the period's arithmetic: the numbers, and the head and the tail of the output.
Prints one JSON line; on the first mismatch a reproducer and exit 1."""
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from fuzz_classes import random_set, sets_of  # noqa: E402
from fuzz_masked import BORDERS, Mismatch, _loaded, random_haystack  # noqa: E402
from fuzz_runs import random_bounds  # noqa: E402

SENT, GUARD = 0xA5, 64


def regex_of(row, lo, hi, delimiter=None):
    """the header's `re` form of the selection, for the set `row` (256 booleans) without the delimiter"""
    if delimiter is not None:
        row = row.copy()
        row[delimiter] = False
    if not row.any():
        return None
    c = b"[" + b"".join(b"\\x%02x" % b for b in np.flatnonzero(row)) + b"]"
    return re.compile(b"(?<!" + c + b")" + c + (b"{%d,%d}" % (lo, hi) if hi else b"{%d,}" % lo) + b"(?!" + c + b")", re.S)


def re_sub(data, row, lo, hi, text, delimiter=None):
    """(the output, the number of selected runs) by re.sub"""
    rx = regex_of(row, lo, hi, delimiter)
    if rx is None:
        return bytes(data), 0
    if delimiter is None:
        return rx.subn(lambda m: text, data)
    d = bytes([delimiter])
    pieces = [rx.subn(lambda m: text, piece) for piece in data.split(d)]
    return d.join(p for p, _ in pieces), sum(k for _, k in pieces)


def byte_window(cap, mis):
    buf = torch.full((cap + 2 * GUARD + 16,), SENT, dtype=torch.uint8, device="cuda")
    at = GUARD + (mis - buf.data_ptr() - GUARD) % 16
    return buf, at, buf[at:at + cap]


def held(buf, at, want):
    h = buf.cpu().numpy()
    return bool((h[:at] == SENT).all() and (h[at + len(want):] == SENT).all() and h[at:at + len(want)].tobytes() == want)


def one_case(rng, stats):
    size = int(rng.choice([600, 5000, 20000, 140000, 280000], p=[.3, .3, .2, .1, .1]))
    host = random_haystack(rng, size + 32)
    row = random_set(rng, host)
    if rng.integers(0, 2) and not row.all():                        # members with probability p: long runs at p near 1
        p = float(rng.choice([0.5, 0.9, 0.98, 0.999, 0.02, 0.05]))
        inside, outside = np.flatnonzero(row).astype(np.uint8), np.flatnonzero(~row).astype(np.uint8)
        host = np.where(rng.random(size + 32) < p, rng.choice(inside, size + 32), rng.choice(outside, size + 32)).astype(np.uint8)
    words = sets_of(row)[0]
    lo, hi = random_bounds(rng)
    pats = [ss.RunPattern.from_set(words, lo, hi, bitmap) for bitmap in (False, True)]
    buf = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16
    buf[at:at + host.size].copy_(torch.from_numpy(host))
    views = [(stats["cases"] % 16, size)]                           # (every misalignment in turn)
    for _ in range(2):
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
        data = hv.tobytes()
        n = int(rng.choice([0, 1, 2, int(rng.integers(0, 41)), 16, 17, 40, 4096], p=[.2, .2, .1, .2, .08, .08, .08, .06]))
        text = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        member = int(rng.choice(np.flatnonzero(row)))
        delimiter = [None, 10, 0, member][int(rng.integers(0, 4))]
        if delimiter is not None and row[delimiter] and row.sum() == 1:
            delimiter = None                                        # (a set that is only the delimiter is refused)
        if n == 4096 and length > 20000:                            # (keep the longest text's outputs small)
            dev, hv, data = dev[:20000], hv[:20000], data[:20000]
        want, count = re_sub(data, row, lo, hi, text, delimiter)
        for path, pat in enumerate(pats):
            omis = int(rng.integers(0, 16))
            got = pat.replace_into(dev, text, None, delimiter)
            stats["calls"] += 1
            if got != (len(want), count):
                raise Mismatch(dict(call="size", path=path, got=got, want=(len(want), count), text=n, delimiter=delimiter, mis=mis, length=len(data), **where))
            if want:
                sbuf, sat, sview = byte_window(len(want) - 1, omis)
                got = pat.replace_into(dev, text, sview, delimiter)
                stats["calls"] += 1
                if got != (len(want), count) or not held(sbuf, sat, b""):
                    raise Mismatch(dict(call="short by one", path=path, got=got, text=n, delimiter=delimiter, mis=mis, omis=omis, length=len(data), **where))
            obuf, oat, oview = byte_window(len(want), omis)
            got = pat.replace_into(dev, text, oview, delimiter)
            stats["calls"] += 1
            if got != (len(want), count) or not held(obuf, oat, want):
                raise Mismatch(dict(call="replace", path=path, got=got, want=(len(want), count), text=n, delimiter=delimiter, mis=mis, omis=omis,
                                    length=len(data), **where))
        stats["views"] += 1
        stats["runs"] += count
        stats["out_bytes"] += len(want)
    stats["cases"] += 1


def large_cases(rng, gib, stats):
    """runs above offset 2^32: a buffer of a period of 7 bytes; the views hold whole periods, so that the numbers follow by arithmetic
    and the output is periodic too"""
    size = int(gib * (1 << 30))
    period = b"abcabd\n"
    hay = torch.from_numpy(np.frombuffer(period, dtype=np.uint8).copy()).cuda().repeat(size // 7 + 1)[:size].contiguous()
    for pattern, text, delimiter in ((r"[ab]+", b"", None), (r"[ab]{2}", b"xyz", None), (r"[ab]{3,}", b"!", None), (r"\w+", b"", None),
                                     (r"[\w\n]+", b"0123456789abcdefXYZ", 10), (r"[cd]+", b"#", None)):
        words, lo, hi = ss.parse_runs(pattern)
        row = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little").astype(bool)
        one, per_period = re_sub(period, row, lo, hi, text, delimiter)
        for bitmap in (False, True):
            pat = ss.RunPattern.from_set(words, lo, hi, bitmap)
            for start in (0, 7, 21):                                # misalignments 0, 7 and 5
                periods = (size - start) // 7 - int(rng.integers(0, 5))
                length = 7 * periods
                assert start + length > (1 << 32) + 7 * 9000, "the buffer must be larger than 4 GiB"
                dev = hay[start:start + length]
                want = (len(one) * periods, per_period * periods)
                got = pat.replace_into(dev, text, None, delimiter)
                stats["calls"] += 1
                if got != want:
                    raise Mismatch(dict(call="size above 2^32", got=got, want=want, pattern=pattern, bitmap=bitmap, start=start, length=length))
                obuf, oat, oview = byte_window(want[0], int(rng.integers(0, 16)))
                got = pat.replace_into(dev, text, oview, delimiter)
                stats["calls"] += 1
                k = 9000 * len(one)
                head, tail = oview[:k].cpu().numpy().tobytes(), oview[want[0] - k:].cpu().numpy().tobytes()
                edges = torch.cat([obuf[:oat], obuf[oat + want[0]:]]).cpu().numpy()
                if got != want or head != one * 9000 or tail != one * 9000 or not (edges == SENT).all():
                    raise Mismatch(dict(call="replace above 2^32", got=got, want=want, pattern=pattern, bitmap=bitmap, start=start, length=length))
                del obuf, oview
    stats["large_gib"] = gib
    del hay
    torch.cuda.empty_cache()


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
    rng = np.random.default_rng(seed)
    stats = {"fuzz": "rewrite", "seed": seed, "seconds": seconds, "cases": 0, "views": 0, "calls": 0, "runs": 0, "out_bytes": 0, "large_gib": 0,
             "mismatches": 0}
    ctx = _loaded() if getattr(ss.lib(), "has_rewrite", False) else ss.rewrite_build()
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
