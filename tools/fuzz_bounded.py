#!/usr/bin/env python3
"""Randomised differential test of the whole-word / whole-line calls (include/sliceslice_hip_bounded.h) on the GPU against the rule
restated in numpy: the (overlapping) occurrences of the needle - both sides through ``bytes.lower()``'s table where case is ignored
- kept where each neighbour byte, read as it is, is absent (index -1 or len of the view), no word byte ([0-9A-Za-z_]; WORD) or
the delimiter (the line forms; LINE takes nothing else); the view cut at every delimiter byte, and a line matches when a kept
occurrence lies wholly inside it.    python tools/fuzz_bounded.py SECONDS SEED

Haystacks: tools/fuzz_nocase.py's kinds plus text over the word bytes' neighbours ('/' ':' '@' '[' '`' '{', '_', 0x80, bytes with a
letter's low seven bits) and blank-separated words; lengths from 0 to a few MiB, misalignments 0..15; needles of 1..3000 bytes,
cut out of the view (as they are, folded, or with one byte changed), through every constructor and filter triple
tools/fuzz_matches.py knows; delimiters include word bytes of every kind; needle copies and word bytes sit just outside both ends
of the view; the record calls write into windows of larger buffers whose sentinels must survive.  Prints one JSON line; on the
first mismatch a reproducer and exit 1."""
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
from fuzz_nocase import haystack as nocase_haystack  # noqa: E402

LOWER = np.frombuffer(bytes(range(256)).lower(), dtype=np.uint8)
WORD = np.zeros(256, dtype=bool)
WORD[list(b"0123456789_") + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B))] = True
EDGES = np.frombuffer(b"/09:@AZ[_`az{\x80\xc1\xe1\xff \n", dtype=np.uint8)


def ref_kept(h, nd, nocase, line, delim):
    """offsets of the kept occurrences of nd (already folded where nocase) in h; delim None: the occurrence forms"""
    offs = ref_offsets(LOWER[h] if nocase else h, nd)
    if offs.size == 0:
        return offs
    keep = np.ones(offs.size, dtype=bool)
    for at in (offs - 1, offs + len(nd)):
        absent = (at < 0) | (at >= h.size)
        b = h[np.clip(at, 0, h.size - 1)]
        ok = np.zeros(offs.size, dtype=bool) if line else ~WORD[b]
        if delim is not None:
            ok |= b == delim
        keep &= absent | ok
    return offs[keep]


def ref_lines(h, nd, delim, nocase, line):
    """(begin, end, number) of the lines of h that hold a kept occurrence"""
    L = h.size
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, L, dtype=np.int64)))
    if begins[-1] == L:
        begins, ends = begins[:-1], ends[:-1]
    if delim in nd:
        k = np.zeros(0, dtype=np.int64)
    else:
        offs = ref_kept(h, nd, nocase, line, delim)
        first = np.searchsorted(dpos, offs, side="left")
        inside = np.searchsorted(dpos, offs + len(nd) - 1, side="right") == first      # (a delimiter 'A' folds onto a needle's 'a')
        k = np.unique(first[inside]).astype(np.int64)
    return begins[k], ends[k], k + 1


def haystack(rng, nrng, kind, L, delim):
    if kind == "word edges":
        a = nrng.choice(EDGES, size=L)
    elif kind == "words":
        a = nrng.choice(np.frombuffer(b"abAB_1  \n.", dtype=np.uint8), size=L)
    else:
        return nocase_haystack(rng, nrng, kind, L, delim)
    if L:
        a[nrng.integers(0, L, size=max(1, L // rng.choice([7, 40, 300, 5000])))] = delim
    return a


def check_calls(s, hay, view, nd, delim, nocase, rng, info):
    s = inner(s)
    offs = ref_kept(view, nd, nocase, False, None)
    total = int(offs.size)
    line = rng.random() < 0.4
    kw = dict(ignore_case=nocase, whole_word=not line, whole_line=line)
    wb, we, wn = ref_lines(view, nd, delim, nocase, line)
    nl = int(wb.size)
    info = dict(info, whole_line=line)
    got = s.count(hay, ignore_case=nocase, whole_word=True)
    if got != total:
        raise Mismatch(dict(info, call="count", got=got, want=total))
    d = torch.full((4,), SENTINEL, dtype=torch.int64, device=hay.device)
    s.count_async(hay, d[1:2], ignore_case=nocase, whole_word=True)
    s.count_lines_async(hay, d[2:3], delim, **kw)
    if d.cpu().tolist() != [SENTINEL, total, nl, SENTINEL]:
        raise Mismatch(dict(info, call="count_async / count_lines_async", got=d.cpu().tolist(), want=[total, nl]))
    cap = rng.choice([0, 1, max(total - 1, 0), total, total + 1, rng.randrange(total + 2)])
    buf = torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device=hay.device)
    ret = s.find_all_into(hay, buf[8:8 + cap], ignore_case=nocase, whole_word=True)
    h, k = buf.cpu().numpy(), min(cap, total)
    if ret != total or not ((h[:8] == SENTINEL).all() and (h[8 + k:] == SENTINEL).all() and (h[8:8 + k] == offs[:k]).all()):
        raise Mismatch(dict(info, call="find_all_into", capacity=cap, returned=ret, want=total, got_near=h[8:16].tolist(), want_near=offs[:8].tolist()))
    got = s.count_lines(hay, delim, **kw)
    if got != nl:
        raise Mismatch(dict(info, call="count_lines", got=got, want=nl))
    cap = rng.choice([0, 1, max(nl - 1, 0), nl, nl + 1, rng.randrange(nl + 2)])
    skip = rng.choice([None, None, 0, 1, 2])
    bufs = [torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device=hay.device) for _ in range(3)]
    args = [None if (j == skip or cap == 0) else bufs[j][8:8 + cap] for j in range(3)]
    ret = s.find_lines_into(hay, args[0], args[1], args[2], cap, delim, **kw)
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
    with ss.bounded_build():
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
                n = max(1, n0 if rng.random() < 0.5 else draw_needle_len(rng))       # (the empty needle is refused: out of scope)
                nocase = rng.random() < 0.5
                view = host[v0:v0 + L]
                if n <= L and rng.random() < 0.8:
                    at = rng.choice([0, L - n, rng.randrange(L - n + 1)])
                    nd = bytearray(view[at:at + n].tobytes())
                    if rng.random() < 0.2:                          # one byte changed: to its bit-5 or bit-7 twin, or to anything
                        k = rng.randrange(n)
                        nd[k] = rng.choice([nd[k] ^ 0x20, nd[k] ^ 0x80, (nd[k] + 1 + rng.randrange(254)) & 0xFF])
                else:
                    nd = bytearray(nrng.choice(EDGES, size=n).tobytes())
                nd = bytes(nd).lower() if nocase else bytes(nd)    # (the folding calls take a needle without upper-case bytes)
                e = v0 + L
                # just outside both ends: copies of the needle, or word bytes - absent neighbours and no occurrences all the same
                if rng.random() < 0.5:
                    host[v0 - n:v0] = np.frombuffer(nd, dtype=np.uint8)
                    host[e:e + n] = np.frombuffer(nd, dtype=np.uint8)
                else:
                    host[v0 - 1], host[e] = rng.choice(b"azAZ09_"), rng.choice(b"azAZ09_")
                dev.copy_(torch.from_numpy(host))
                s, desc = make_searcher(rng, nd)
                view = host[v0:v0 + L]
                info = {"MISMATCH": True, "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis, "delimiter": delim,
                        "ignore_case": nocase, "needle": nd.hex() if n <= 128 else nd[:64].hex() + "..", "needle_len": n, "searcher": desc}
                calls += check_calls(s, hay, view, nd, delim, nocase, rng, info)
                cases += 1
            del dev, hay
    return {"fuzz_bounded": "ok", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases, "calls": calls, "tile_bytes": TILE}


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
