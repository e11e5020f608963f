#!/usr/bin/env python3
"""Randomised differential test of the matching-lines calls on the GPU (include/sliceslice_hip_lines.h: ss_count_lines_device /
_async, ss_find_lines_device) against the rule restated in numpy: cut the view at every delimiter byte, drop a trailing empty
piece, a line matches when the needle occurs inside it.    python tools/fuzz_lines.py SECONDS SEED

Haystacks: random bytes, two-letter text, runs and periodic patterns, the manual's text, delimiter-dense and delimiter-free ones;
lengths from 0 to a few MiB (mostly multiples of 1, 4, 16 or 32 KiB, give or take), misalignments 0..15; needles of 0..3000 bytes
through every constructor and filter triple tools/fuzz_matches.py knows, with and without the delimiter inside; delimiters and
needle copies sit just outside both ends of the view; find_lines writes into windows of larger buffers whose sentinels on both
sides must survive, with capacity cuts and each of the three arrays left out in turn.  Prints one JSON line; on the first mismatch
a reproducer and exit 1."""
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
from fuzz_matches import GUARD, SENTINEL, TILE, Mismatch, draw_len, draw_needle_len, inner, make_searcher, ref_offsets  # noqa: E402


def ref_lines(h, nd, delim):
    """(begin, end, number) int64 arrays of the matching lines of h."""
    h = np.asarray(h, dtype=np.uint8)
    L = h.size
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, L, dtype=np.int64)))
    if begins[-1] == L:                                   # nothing behind the last delimiter (or an empty view): no such line
        begins, ends = begins[:-1], ends[:-1]
    if len(nd) == 0:
        k = np.arange(begins.size, dtype=np.int64)
    elif delim in bytes(nd):
        k = np.zeros(0, dtype=np.int64)
    else:
        k = np.unique(np.searchsorted(dpos, ref_offsets(h, nd), side="left")).astype(np.int64)
    return begins[k], ends[k], k + 1


def make_haystack(rng, nrng, kind, L, delim):
    if kind == "random":
        return nrng.integers(0, 256, size=L, dtype=np.uint8)
    if kind == "ab":                                      # two-letter text with delimiters every few dozen bytes
        a = nrng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=L)
        if L:
            a[nrng.integers(0, L, size=max(1, L // rng.choice([7, 40, 300, 5000])))] = delim
        return a
    if kind == "runs":                                    # a short period repeated, delimiters sprinkled in
        per = nrng.integers(0, 256, size=rng.choice([1, 2, 3, 5, 17]), dtype=np.uint8)
        a = np.resize(per, L).copy()
        if L:
            a[nrng.integers(0, L, size=max(1, L // rng.choice([3, 64, 1024, 20000])))] = delim
        return a
    if kind == "text":
        t = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "data", "i386.txt"), "rb").read()
        return np.resize(np.frombuffer(t, dtype=np.uint8), L).copy()
    if kind == "dense":                                   # mostly delimiters
        a = np.full(L, delim, dtype=np.uint8)
        if L:
            idx = nrng.integers(0, L, size=max(1, L // 3))
            a[idx] = nrng.integers(0, 256, size=idx.size, dtype=np.uint8)
        return a
    a = nrng.integers(0, 256, size=L, dtype=np.uint8)     # "free": no delimiter at all (or one, somewhere)
    a[a == delim] = (delim + 1) & 0xFF
    if L and rng.random() < 0.5:
        a[rng.randrange(L)] = delim
    return a


def check_calls(s, hay, want, delim, cap_choice, rng, info):
    wb, we, wn = want
    total = int(wb.size)
    s = inner(s)
    got = s.count_lines(hay, delim)
    if got != total:
        raise Mismatch(dict(info, call="count_lines", got=got, want=total))
    d = torch.full((3,), SENTINEL, dtype=torch.int64, device=hay.device)
    s.count_lines_async(hay, d[1:2], delim)
    dv = d.cpu().tolist()
    if dv[1] != total or dv[0] != SENTINEL or dv[2] != SENTINEL:
        raise Mismatch(dict(info, call="count_lines_async", got=dv, want=total))
    b, e, n = (t.cpu().numpy() for t in s.find_lines(hay, delim))
    for name, g, w in (("begin", b, wb), ("end", e, we), ("number", n, wn)):
        if g.size != total or not (g == w).all():
            m = min(g.size, total)
            bad = int(np.flatnonzero(g[:m] != w[:m])[:1].sum()) if m else 0
            raise Mismatch(dict(info, call="find_lines", array=name, got_size=int(g.size), want=total, first_diff=bad,
                                got_near=g[max(0, bad - 2):bad + 3].tolist(), want_near=w[max(0, bad - 2):bad + 3].tolist()))
    cap = {"0": 0, "1": 1, "total-1": max(total - 1, 0), "total": total, "total+1": total + 1,
           "random": rng.randrange(total + 2)}[cap_choice]
    skip = rng.choice([None, None, 0, 1, 2])              # one of the three arrays not wanted
    bufs = [torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device=hay.device) for _ in range(3)]
    args = [None if k == skip else bufs[k][8:8 + cap] for k in range(3)]
    if cap == 0:
        args = [None, None, None]
    ret = s.find_lines_into(hay, args[0], args[1], args[2], cap, delim)
    k = min(cap, total)
    ok = ret == total
    for j, w in enumerate((wb, we, wn)):
        h = bufs[j].cpu().numpy()
        ok = ok and (h[:8] == SENTINEL).all() and (h[8 + k:] == SENTINEL).all()
        ok = ok and ((h[8:8 + k] == SENTINEL).all() if (j == skip or cap == 0) else (h[8:8 + k] == w[:k]).all())
    if not ok:
        raise Mismatch(dict(info, call="find_lines_into", capacity=cap, left_out=skip, returned=ret, want=total))
    return 4


def run(seconds, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = haystacks = 0
    with ss.lines_build():
        while time.time() < t_end:
            kind = rng.choice(["random", "ab", "runs", "text", "dense", "free"])
            delim = rng.choice([0x0A, 0x0A, 0x00, 0xFF, rng.randrange(256), ord("a")])
            n0 = draw_needle_len(rng)
            L = min(draw_len(rng, n0), 8 << 20)
            mis = rng.randrange(16)
            host = nrng.integers(0, 256, size=L + 2 * GUARD, dtype=np.uint8)
            v0 = GUARD + mis - (GUARD % 16)                          # the view starts `mis` bytes past a 16-byte boundary
            host[v0:v0 + L] = make_haystack(rng, nrng, kind, L, delim)
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
                r = rng.random()
                if n and n <= L and r < 0.75:                             # cut from the view, maybe with one byte changed
                    at = rng.choice([0, L - n, rng.randrange(L - n + 1)])
                    if r < 0.4:                                           # ... from inside a line, so that it can match
                        dp = np.flatnonzero(view[at:at + 4 * n + 64] == delim)
                        room = int(dp[0]) if dp.size else min(L - at, 4 * n + 64)
                        n = max(1, min(n, room)) if room else n
                    nd = bytearray(view[at:at + n].tobytes())
                    if rng.random() < 0.2:
                        k = rng.randrange(n)
                        nd[k] = (nd[k] + 1 + rng.randrange(254)) & 0xFF
                else:
                    nd = bytearray(nrng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
                if n and rng.random() < 0.08:
                    nd[rng.randrange(n)] = delim                          # a needle that holds the delimiter matches no line
                nd = bytes(nd)
                arr = np.frombuffer(nd, dtype=np.uint8)
                # needle copies and delimiters just outside both ends of the view
                e = v0 + L
                if n:
                    host[v0 - n:v0] = arr
                    host[e:e + n] = arr
                if rng.random() < 0.7:
                    host[v0 - rng.choice([1, 1, 2, n + 1])] = delim
                    host[e + rng.choice([0, 0, 1, n])] = delim
                dev.copy_(torch.from_numpy(host))
                if n == 0:
                    s, desc = ss.DynamicHipSearcher(b""), "empty"
                else:
                    s, desc = make_searcher(rng, nd)
                want = ref_lines(host[v0:v0 + L], nd, delim)
                cap_choice = rng.choice(["0", "1", "total-1", "total", "total+1", "random"])
                info = {"MISMATCH": True, "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis, "delimiter": delim,
                        "needle": nd.hex() if n <= 128 else nd[:64].hex() + "..", "needle_len": n, "searcher": desc,
                        "capacity": cap_choice}
                calls += check_calls(s, hay, want, delim, cap_choice, rng, info)
                cases += 1
            del dev, hay
    return {"fuzz_lines": "ok", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases, "calls": calls,
            "tile_bytes": TILE}


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
