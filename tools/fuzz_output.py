#!/usr/bin/env python3
"""Randomised differential test of the output calls (include/sliceslice_hip_output.h) on the GPU against the rule restated here in
Python: ss_format_lines_device and ss_gather_ranges_device on random records, ss_grep_lines_device against find_lines_context
followed by the restated rule.
    python tools/fuzz_output.py SECONDS SEED [GIB]

Records: lines of a text in order, random ranges (overlapping, repeated, descending), ranges out of contract (begin > end, end and
begin beyond the view, values at the top of 64 bits), empty ranges, a few long ones among many short ones; 1 to a little over three
blocks of them.  Numbers: ascending by 1 and 2, random 64-bit values, the ends of every digit count.  Every flag combination, every
terminator (none, and each byte value), kinds given and NULL.  Both buffers stand at every misalignment; bytes that occur nowhere in
the view stand just outside both of its ends.  The capacity is exact, roomy or cut short; the output is a window of a larger buffer
whose sentinels on both sides must survive, and so are the starts.  With GIB the haystack holds that many GiB and records begin above
2^32.  Prints one JSON line; on the first mismatch a reproducer and exit 1."""
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from fuzz_matches import Mismatch  # noqa: E402

SENT64, SENT8 = -0x5A5A5A5A5A5A5A5B, 0xA5
GUARD = 64
B, CH = ss.OUTPUT_BLOCK, ss.OUTPUT_CHUNK
U64 = (1 << 64) - 1


def rule(data, begin, end, number, kind, terminator, numbers, separators):
    """(the output, the count + 1 starts): include/sliceslice_hip_output.h's rule, record by record"""
    out, starts, tail = bytearray(), [], (b"" if terminator is None else bytes([terminator]))
    for i in range(len(begin)):
        starts.append(len(out))
        if separators and i > 0 and number[i] > number[i - 1] + 1:
            out += b"--" + tail
        if numbers:
            out += b"%d" % number[i] + (b":" if kind is None or kind[i] else b"-")
        e = min(end[i], len(data))
        b = min(begin[i], e)
        out += data[b:e] + tail
    starts.append(len(out))
    return bytes(out), starts


def dev64(values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64).copy()).cuda()


def draw_records(rng, L, big):
    count = rng.choice([1, 2, 7, 300, B - 1, B, B + 1, 2 * B + 1, 3 * B + 7, rng.randrange(1, 2 * B)])
    shape = rng.choice(["lines", "random", "out of contract", "empty", "long among short", "one long"])
    lengths = [0, 1, 15, 16, 17, 40, 100]
    low = (1 << 32) + 5 if big and L > (1 << 32) + (1 << 20) else 0
    if shape == "one long":
        count = rng.choice([1, 3])
    begin, end = [], []
    at = low
    for i in range(count):
        n = rng.choice(lengths)
        if shape == "lines":
            b, e = at, at + n
            at = e + 1 if e + 1 < L else low
        elif shape == "random":
            b = rng.randrange(low, max(L, low + 1))
            e = b + n
        elif shape == "out of contract":
            b = rng.choice([rng.randrange(low, max(L, low + 1)), L, L + 3, U64, 1 << 63, rng.randrange(U64)])
            e = rng.choice([b + n if b + n <= U64 else U64, L + 7, U64, 0, rng.randrange(max(L, 1)), b])
        elif shape == "empty":
            b = e = rng.randrange(low, max(L, low + 1))
        elif shape == "long among short":
            b = rng.randrange(low, max(L, low + 1))
            e = b + (rng.choice([CH - 1, CH, CH + 1, 3 * CH + CH // 2, 100000]) if rng.random() < 0.01 else n)
        else:
            b = rng.randrange(low, max(L - 1, low + 1))
            e = L if i == count // 2 else b + n
        begin.append(b)
        end.append(e)
    numbering = rng.choice(["by one", "by one and two", "random", "edges"])
    if numbering == "by one":
        first = rng.choice([1, 9, 99998, (1 << 32) - 5])
        number = [first + i for i in range(count)]
    elif numbering == "by one and two":
        number, v = [], rng.choice([0, 1, 95, (1 << 32) - 100])
        for _ in range(count):
            v += rng.choice([1, 1, 1, 2, 3])
            number.append(v)
    elif numbering == "random":
        number = [rng.randrange(U64 + 1) for _ in range(count)]
    else:
        edges = [0, U64, U64 - 1] + [10 ** k + d for k in range(20) for d in (-1, 0, 1) if 0 <= 10 ** k + d <= U64]
        number = [rng.choice(edges) for _ in range(count)]
    kind = None if rng.random() < 0.25 else [rng.randrange(2) for _ in range(count)]
    return shape, numbering, begin, end, number, kind


def window(cap, mis):
    buf = torch.full((cap + 2 * GUARD + 16,), SENT8, dtype=torch.uint8, device="cuda")
    at = GUARD + (mis - buf.data_ptr() - GUARD) % 16
    return buf, at


def check_records(rng, hay, host, info, big):
    shape, numbering, begin, end, number, kind = draw_records(rng, len(host), big)
    flags = rng.randrange(4)
    terminator = rng.choice([None, 10, 0, rng.randrange(256)])
    numbers, separators = bool(flags & 1), bool(flags & 2)
    gather = flags == 0 and rng.random() < 0.5
    want, starts = rule(host, begin, end, number, kind, terminator, numbers, separators)
    info = dict(info, shape=shape, numbering=numbering, count=len(begin), flags=flags, terminator=terminator, kinds=kind is not None, gather=gather)
    d_b, d_e, d_n = dev64(begin), dev64(end), dev64(number)
    d_k = torch.tensor(kind, dtype=torch.uint8, device="cuda") if kind is not None else None
    delimiter = None if terminator is None else bytes([terminator])
    calls = 0
    for cap in {len(want), len(want) + rng.randrange(1, 100), max(len(want) - 1, 0), rng.randrange(len(want) + 1)}:
        mis = rng.randrange(16)
        buf, at = window(cap, mis)
        sbuf = torch.full((len(begin) + 1 + 16,), SENT64, dtype=torch.int64, device="cuda")
        d_starts = sbuf[8:8 + len(begin) + 1] if rng.random() < 0.7 else None
        with ss.output_build():
            if gather:
                total = ss.searcher._format_into(ss.lib(), hay, d_b, d_e, None, None, delimiter, 0, buf[at:at + cap], d_starts, None, gather=True)
            else:
                total = ss.format_lines_into(hay, d_b, d_e, buf[at:at + cap], number=d_n if flags or rng.random() < 0.5 else None, kind=d_k,
                                             delimiter=delimiter, line_numbers=numbers, separators=separators, d_starts=d_starts)
        calls += 1
        h = buf.cpu().numpy()
        k = len(want) if cap >= len(want) else 0
        ok = total == len(want) and (h[:at] == SENT8).all() and (h[at + k:] == SENT8).all() and h[at:at + k].tobytes() == want[:k]
        if d_starts is not None:
            s = sbuf.cpu().tolist()
            ok = ok and s[8:8 + len(starts)] == starts and all(v == SENT64 for v in s[:8] + s[8 + len(starts):])
        if not ok:
            raise Mismatch(dict(info, call="gather_ranges" if gather else "format_lines_into", capacity=cap, out_mis=mis, got=total, want=len(want),
                                begin=begin[:8], end=end[:8], number=number[:8]))
    return calls


def check_grep(rng, hay, host, info):
    nd = rng.choice([b"", b"e", b"the", b"\n", b"zq", host[rng.randrange(max(len(host) - 5, 1)):][:rng.randrange(1, 6)]])
    before, after = rng.choice([0, 0, 1, 3, U64]), rng.choice([0, 0, 2, 5])
    line_numbers, invert = rng.random() < 0.6, rng.random() < 0.3
    with ss.output_build():
        s = ss.DynamicHipSearcher.new(nd)
        got = bytes(s.grep(hay, before, after, line_numbers=line_numbers, invert=invert).cpu().numpy())
        rec = [x.cpu().tolist() for x in s.find_lines_context(hay, before, after, invert=invert)]
    want, _ = rule(host, rec[0], rec[1], rec[2], rec[3], 10, line_numbers, bool(before or after))
    if got != want:
        raise Mismatch(dict(info, call="grep", needle=nd.hex(), before=before, after=after, line_numbers=line_numbers, invert=invert,
                            got=len(got), want=len(want)))
    return 1


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 0
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = greps = 0
    try:
        while time.time() < t_end:
            L = int(gib * (1 << 30)) if gib else rng.choice([0, 1, 17, 300, CH - 1, CH, CH + 1, 65536, 131072 + 5, rng.randrange(1, 400000)])
            # text: letters, spaces and newlines; the bytes 1 and 2 stand just outside the view and nowhere inside
            host_a = nrng.choice(np.frombuffer(b"etaoin shrdlu\n\n,.THE", dtype=np.uint8), size=L)
            mis = rng.randrange(16)
            buf = torch.empty(L + 2 * GUARD + 32, dtype=torch.uint8, device="cuda")
            at = (-buf.data_ptr()) % 16 + 16 + mis
            buf[at:at + GUARD] = 1
            buf[at + GUARD + L:at + 2 * GUARD + L] = 2
            hay = buf[at + GUARD:at + GUARD + L]
            if L:
                hay.copy_(torch.from_numpy(host_a))
            host = host_a.tobytes()
            info = dict(seed=seed, case=cases, len=L, mis=mis)
            for _ in range(2 if gib else 6):
                calls += check_records(rng, hay, host, info, bool(gib))
                cases += 1
            if not gib:
                greps += check_grep(rng, hay, host, info)
    except Mismatch as e:
        print(json.dumps({"fuzz": "output", "mismatch": e.args[0]}))
        sys.exit(1)
    print(json.dumps({"fuzz": "output", "seed": seed, "seconds": seconds, "gib": gib, "cases": cases, "greps": greps, "calls": calls + greps,
                      "mismatches": 0}))


if __name__ == "__main__":
    main()
