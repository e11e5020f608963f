#!/usr/bin/env python3
"""Randomised differential test of the calls that ignore ASCII case (include/sliceslice_hip_nocase.h) on the GPU against the rule
restated in numpy: fold the haystack and the needle with ``bytes.lower()``'s table, count overlapping occurrences, cut the UNFOLDED
view at every delimiter byte, and a line matches when an occurrence lies wholly inside it.    python tools/fuzz_nocase.py SECONDS SEED

Haystacks: tools/fuzz_lines.py's kinds plus mixed-case two-letter text and text over the bytes next to the letter ranges ('@' '['
'`' '{') and their bit-7 twins; lengths from 0 to a few MiB, misalignments 0..15; needles of 0..3000 bytes cut from the view (folded,
in a random case through new_nocase, or with one byte changed) through every constructor and filter triple tools/fuzz_matches.py
knows; delimiters include letters of both cases; needle copies in another case sit just outside both ends of the view; the record
calls write into windows of larger buffers whose sentinels must survive.  Prints one JSON line; on the first mismatch a reproducer
and exit 1."""
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
from fuzz_lines import make_haystack  # noqa: E402
from fuzz_matches import GUARD, SENTINEL, TILE, Mismatch, draw_len, draw_needle_len, inner, make_searcher, ref_offsets  # noqa: E402

LOWER = np.frombuffer(bytes(range(256)).lower(), dtype=np.uint8)
EDGES = np.frombuffer(b"@AZ[`az{\xc1\xda\xe1\xfa\n", dtype=np.uint8)


def ref_lines(h, nd, delim):
    """(begin, end, number) of the matching lines of h ignoring case; nd is the folded needle"""
    L = h.size
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, L, dtype=np.int64)))
    if begins[-1] == L:
        begins, ends = begins[:-1], ends[:-1]
    if len(nd) == 0:
        k = np.arange(begins.size, dtype=np.int64)
    elif delim in nd:
        k = np.zeros(0, dtype=np.int64)
    else:
        offs = ref_offsets(LOWER[h], nd)
        first = np.searchsorted(dpos, offs, side="left")
        inside = np.searchsorted(dpos, offs + len(nd) - 1, side="right") == first      # (a delimiter 'A' folds onto a needle's 'a')
        k = np.unique(first[inside]).astype(np.int64)
    return begins[k], ends[k], k + 1


def haystack(rng, nrng, kind, L, delim):
    if kind == "abAB":
        a = nrng.choice(np.frombuffer(b"abAB", dtype=np.uint8), size=L)
    elif kind == "edges":
        a = nrng.choice(EDGES, size=L)
    else:
        return make_haystack(rng, nrng, kind, L, delim)
    if L:
        a[nrng.integers(0, L, size=max(1, L // rng.choice([7, 40, 300, 5000])))] = delim
    return a


def check_calls(s, hay, offs, lines, delim, rng, info):
    s = inner(s)
    total = int(offs.size)
    got = s.count(hay, ignore_case=True)
    if got != total:
        raise Mismatch(dict(info, call="count", got=got, want=total))
    d = torch.full((4,), SENTINEL, dtype=torch.int64, device=hay.device)
    s.count_async(hay, d[1:2], ignore_case=True)
    s.count_lines_async(hay, d[2:3], delim, ignore_case=True)
    if d.cpu().tolist() != [SENTINEL, total, int(lines[0].size), SENTINEL]:
        raise Mismatch(dict(info, call="count_async / count_lines_async", got=d.cpu().tolist(), want=[total, int(lines[0].size)]))
    cap = rng.choice([0, 1, max(total - 1, 0), total, total + 1, rng.randrange(total + 2)])
    buf = torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device=hay.device)
    ret = s.find_all_into(hay, buf[8:8 + cap], ignore_case=True)
    h, k = buf.cpu().numpy(), min(cap, total)
    if ret != total or not ((h[:8] == SENTINEL).all() and (h[8 + k:] == SENTINEL).all() and (h[8:8 + k] == offs[:k]).all()):
        raise Mismatch(dict(info, call="find_all_into", capacity=cap, returned=ret, want=total, got_near=h[8:16].tolist(), want_near=offs[:8].tolist()))
    wb, we, wn = lines
    nl = int(wb.size)
    got = s.count_lines(hay, delim, ignore_case=True)
    if got != nl:
        raise Mismatch(dict(info, call="count_lines", got=got, want=nl))
    cap = rng.choice([0, 1, max(nl - 1, 0), nl, nl + 1, rng.randrange(nl + 2)])
    skip = rng.choice([None, None, 0, 1, 2])
    bufs = [torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device=hay.device) for _ in range(3)]
    args = [None if (j == skip or cap == 0) else bufs[j][8:8 + cap] for j in range(3)]
    ret = s.find_lines_into(hay, args[0], args[1], args[2], cap, delim, ignore_case=True)
    k = min(cap, nl)
    ok = ret == nl
    for j, w in enumerate((wb, we, wn)):
        h = bufs[j].cpu().numpy()
        ok = ok and (h[:8] == SENTINEL).all() and (h[8 + k:] == SENTINEL).all()
        ok = ok and ((h[8:8 + k] == SENTINEL).all() if (j == skip or cap == 0) else (h[8:8 + k] == w[:k]).all())
    if not ok:
        raise Mismatch(dict(info, call="find_lines_into", capacity=cap, left_out=skip, returned=ret, want=nl))
    return 7


def run(seconds, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = haystacks = 0
    with ss.nocase_build():
        while time.time() < t_end:
            kind = rng.choice(["abAB", "edges", "text", "text", "ab", "runs", "random", "dense", "free"])
            delim = rng.choice([0x0A, 0x0A, 0x00, 0xFF, rng.randrange(256), ord("a"), ord("A"), ord("B"), ord("Z"), ord("[")])
            n0 = draw_needle_len(rng)
            L = min(draw_len(rng, n0), 8 << 20)
            mis = rng.randrange(16)
            host = nrng.integers(0, 256, size=L + 2 * GUARD, dtype=np.uint8)
            v0 = GUARD + mis - (GUARD % 16)
            host[v0:v0 + L] = haystack(rng, nrng, kind, L, delim)
            dev = torch.from_numpy(host).cuda()
            hay = dev[v0:v0 + L]
            haystacks += 1
            for _ in range(8):
                if time.time() >= t_end:
                    break
                n = n0 if rng.random() < 0.5 else draw_needle_len(rng)
                if rng.random() < 0.04:
                    n = 0
                view = host[v0:v0 + L]
                if n and n <= L and rng.random() < 0.8:
                    at = rng.choice([0, L - n, rng.randrange(L - n + 1)])
                    nd = bytearray(view[at:at + n].tobytes())
                    if rng.random() < 0.25:                         # one byte changed: to its bit-5 or bit-7 twin, or to anything
                        k = rng.randrange(n)
                        nd[k] = rng.choice([nd[k] ^ 0x20, nd[k] ^ 0x80, nd[k] ^ 0xA0, (nd[k] + 1 + rng.randrange(254)) & 0xFF])
                else:
                    nd = bytearray(nrng.choice(EDGES, size=n).tobytes())
                nd = bytes(nd)
                folded = nd.lower()
                e = v0 + L
                if n:                                               # copies in the other case just outside both ends
                    host[v0 - n:v0] = np.frombuffer(nd.swapcase(), dtype=np.uint8)
                    host[e:e + n] = np.frombuffer(nd.upper(), dtype=np.uint8)
                if rng.random() < 0.7:
                    host[v0 - rng.choice([1, 1, 2, n + 1])] = delim
                    host[e + rng.choice([0, 0, 1, n])] = delim
                dev.copy_(torch.from_numpy(host))
                if n == 0 or rng.random() < 0.4:
                    s, desc = ss.DynamicHipSearcher.new_nocase(nd), "new_nocase"
                else:
                    s, desc = make_searcher(rng, folded)           # any constructor, on a needle without upper-case bytes
                view = host[v0:v0 + L]
                offs = ref_offsets(LOWER[view], folded)
                info = {"MISMATCH": True, "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis, "delimiter": delim,
                        "needle": nd.hex() if n <= 128 else nd[:64].hex() + "..", "needle_len": n, "searcher": desc}
                calls += check_calls(s, hay, offs, ref_lines(view, folded, delim), delim, rng, info)
                cases += 1
            del dev, hay
    return {"fuzz_nocase": "ok", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases, "calls": calls, "tile_bytes": TILE}


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    try:
        out = run(seconds, seed)
    except Mismatch as m:
        print(json.dumps(m.args[0], default=str))
        sys.exit(1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
