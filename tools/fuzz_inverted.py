#!/usr/bin/env python3
"""Randomised differential test of the inverted line calls (include/sliceslice_hip_inverted.h) on the GPU against the rule restated
in numpy: the view cut at every delimiter byte (an unterminated last line is a line, an empty view has none), minus the lines that
match under `how` - plain, ignoring case, whole word, whole line, the latter two also ignoring case - by tools/fuzz_bounded.py's
and tools/fuzz_lines.py's rules.  A needle longer than the view or one that holds the delimiter matches no line (every line is
selected); the empty needle matches every line (none is).    python tools/fuzz_inverted.py SECONDS SEED

Haystacks: tools/fuzz_bounded.py's kinds; lengths from 0 to a few MiB, misalignments 0..15; needles of 0..3000 bytes, cut out of the
view (as they are, folded, or with one byte changed), through every constructor and filter triple tools/fuzz_matches.py knows;
delimiters include word bytes of every kind and needle bytes; needle copies and delimiters sit just outside both ends of the view;
the record calls write into windows of larger buffers whose sentinels must survive, at capacities around the total and with each
array left out in turn.  Every case also checks the complement against the library itself: inverted count + non-inverted count =
the empty needle's count.  Prints one JSON line; on the first mismatch a reproducer and exit 1."""
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
from fuzz_bounded import EDGES, LOWER, haystack, ref_lines as ref_bounded_lines  # noqa: E402
from fuzz_matches import GUARD, SENTINEL, TILE, Mismatch, draw_len, draw_needle_len, inner, make_searcher, ref_offsets  # noqa: E402

HOWS = {"": {}, "i": dict(ignore_case=True), "w": dict(whole_word=True), "wi": dict(whole_word=True, ignore_case=True),
        "x": dict(whole_line=True), "xi": dict(whole_line=True, ignore_case=True)}


def ref_inverted(h, nd, delim, how):
    """((begin, end, number) of the lines of h that do NOT match, the number of lines)"""
    L = h.size
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, L, dtype=np.int64)))
    if begins[-1] == L:
        begins, ends = begins[:-1], ends[:-1]
    nocase = how.endswith("i")
    hit = np.zeros(begins.size, dtype=bool)
    if how[:1] in ("w", "x"):
        hit[ref_bounded_lines(h, nd, delim, nocase, how[0] == "x")[2] - 1] = True
    elif len(nd) == 0:
        hit[:] = True
    elif delim not in nd and len(nd) <= L:
        offs = ref_offsets(LOWER[h] if nocase else h, nd)
        first = np.searchsorted(dpos, offs, side="left")
        inside = np.searchsorted(dpos, offs + len(nd) - 1, side="right") == first
        hit[np.unique(first[inside])] = True
    keep = ~hit
    return (begins[keep], ends[keep], np.flatnonzero(keep).astype(np.int64) + 1), int(begins.size)


def check_calls(s, every, hay, view, nd, delim, how, rng, info):
    s = inner(s)
    kw = HOWS[how]
    (wb, we, wn), nlines = ref_inverted(view, nd, delim, how)
    nl = int(wb.size)
    got = s.count_lines_inverted(hay, delim, **kw)
    if got != nl:
        raise Mismatch(dict(info, call="count_lines_inverted", got=got, want=nl))
    d = torch.full((3,), SENTINEL, dtype=torch.int64, device=hay.device)
    s.count_lines_inverted_async(hay, d[1:2], delim, **kw)
    if d.cpu().tolist() != [SENTINEL, nl, SENTINEL]:
        raise Mismatch(dict(info, call="count_lines_inverted_async", got=d.cpu().tolist(), want=nl))
    plain, total = s.count_lines(hay, delim, **kw), every.count_lines(hay, delim)
    if plain + nl != total or total != nlines:
        raise Mismatch(dict(info, call="complement", inverted=nl, non_inverted=plain, lines=total, want_lines=nlines))
    cap = rng.choice([0, 1, max(nl - 1, 0), nl, nl + 1, rng.randrange(nl + 2)])
    skip = rng.choice([None, None, 0, 1, 2])
    bufs = [torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device=hay.device) for _ in range(3)]
    args = [None if (j == skip or cap == 0) else bufs[j][8:8 + cap] for j in range(3)]
    ret = s.find_lines_inverted_into(hay, args[0], args[1], args[2], cap, delim, **kw)
    k = min(cap, nl)
    ok = ret == nl
    for j, w in enumerate((wb, we, wn)):
        h = bufs[j].cpu().numpy()
        ok = ok and (h[:8] == SENTINEL).all() and (h[8 + k:] == SENTINEL).all()
        ok = ok and ((h[8:8 + k] == SENTINEL).all() if (j == skip or cap == 0) else (h[8:8 + k] == w[:k]).all())
    if not ok:
        raise Mismatch(dict(info, call="find_lines_inverted_into", capacity=cap, left_out=skip, returned=ret, want=nl))
    return 5


def run(seconds, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = haystacks = 0
    with ss.inverted_build():
        every = ss.DynamicHipSearcher(b"")
        while time.time() < t_end:
            kind = rng.choice(["word edges", "words", "words", "abAB", "edges", "text", "text", "ab", "runs", "random", "dense", "free"])
            delim = rng.choice([0x0A, 0x0A, 0x00, 0xFF, rng.randrange(256), ord("a"), ord("A"), ord("_"), ord("0"), ord(" "), ord("[")])
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
                how = rng.choice(list(HOWS))
                n = n0 if rng.random() < 0.5 else draw_needle_len(rng)
                if rng.random() < 0.03 and how[:1] not in ("w", "x"):
                    n = 0                                           # the empty needle: every line matches
                n = max(n, 1) if how[:1] in ("w", "x") else n       # (refused with a bound: out of scope)
                nocase = how.endswith("i")
                view = host[v0:v0 + L]
                if 0 < n <= L and rng.random() < 0.8:
                    at = rng.choice([0, L - n, rng.randrange(L - n + 1)])
                    nd = bytearray(view[at:at + n].tobytes())
                    if rng.random() < 0.2:
                        k = rng.randrange(n)
                        nd[k] = rng.choice([nd[k] ^ 0x20, nd[k] ^ 0x80, (nd[k] + 1 + rng.randrange(254)) & 0xFF])
                else:
                    nd = bytearray(nrng.choice(EDGES, size=n).tobytes())   # (also: longer than the view)
                nd = bytes(nd).lower() if nocase else bytes(nd)
                e = v0 + L
                if n and rng.random() < 0.5:
                    m = min(n, GUARD - 16)
                    host[v0 - m:v0] = np.frombuffer(nd[-m:], dtype=np.uint8)
                    host[e:e + m] = np.frombuffer(nd[:m], dtype=np.uint8)
                else:
                    host[v0 - 1], host[e] = delim, delim
                dev.copy_(torch.from_numpy(host))
                s, desc = make_searcher(rng, nd) if n else (ss.DynamicHipSearcher(b""), "new")
                view = host[v0:v0 + L]
                info = {"MISMATCH": True, "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis, "delimiter": delim, "how": how,
                        "needle": nd.hex() if n <= 128 else nd[:64].hex() + "..", "needle_len": n, "searcher": desc}
                calls += check_calls(s, every, hay, view, nd, delim, how, rng, info)
                cases += 1
            del dev, hay
    return {"fuzz_inverted": "ok", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases, "calls": calls, "tile_bytes": TILE}


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
