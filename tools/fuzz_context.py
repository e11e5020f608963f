#!/usr/bin/env python3
"""Randomised differential test of the context calls (include/sliceslice_hip_context.h) on the GPU against the rule restated in
numpy: S = the numbers of the lines the model selects (tools/fuzz_inverted.py's rule, or its complement), N = the number of lines;
the output is every line in the union over s in S of [max(1, s - before), min(N, s + after)], once and ascending, with kind 1 for
the lines of S; the records are those of the view cut at every delimiter byte.    python tools/fuzz_context.py SECONDS SEED

Haystacks: tools/fuzz_inverted.py's kinds, lengths and misalignments, with needle copies and delimiters just outside both ends of
the view; all six `how` values, inverted or not; before and after from {0, 1, 2, 7, N - 1, N, 2^64 - 1} and at random; the record
calls write into windows of larger buffers whose sentinels must survive, at capacities around the total and with each of the four
arrays left out in turn.  Every case also runs lines_around on a random ascending set of numbers that may hold 0 and numbers above
N.  Prints one JSON line; on the first mismatch a reproducer and exit 1."""
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
from fuzz_bounded import EDGES, haystack  # noqa: E402
from fuzz_inverted import HOWS, ref_inverted  # noqa: E402
from fuzz_matches import GUARD, SENTINEL, TILE, Mismatch, draw_len, draw_needle_len, inner, make_searcher  # noqa: E402

U64_MAX = (1 << 64) - 1
KIND_SENTINEL = 0xA5


def every_line(h, delim):
    dpos = np.flatnonzero(h == delim).astype(np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, h.size, dtype=np.int64)))
    if begins[-1] == h.size:
        begins, ends = begins[:-1], ends[:-1]
    return begins, ends


def context_rule(selected, n_lines, before, after):
    """(numbers, kinds) - an amount of n_lines or more reaches the end of the view, which is what saturating arithmetic gives"""
    sel = np.asarray([int(s) for s in selected if 1 <= int(s) <= n_lines], dtype=np.int64)
    if sel.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8)
    b, a = min(before, n_lines), min(after, n_lines)
    edge = np.zeros(n_lines + 2, dtype=np.int64)
    np.add.at(edge, np.maximum(1, sel - b), 1)
    np.add.at(edge, np.minimum(n_lines, sel + a) + 1, -1)
    numbers = np.flatnonzero(np.cumsum(edge)[:n_lines + 1] > 0).astype(np.int64)
    chosen = np.zeros(n_lines + 1, dtype=np.uint8)
    chosen[sel] = 1
    return numbers, chosen[numbers]


def draw_amount(rng, n_lines):
    return rng.choice([0, 1, 2, 7, max(n_lines - 1, 0), n_lines, U64_MAX, rng.randrange(n_lines + 3), rng.randrange(1 << 64)])


def check_into(call, want, rng, info):
    """call(d_begin, d_end, d_number, d_kind, capacity) -> total, through sentinel windows at a capacity around the total"""
    total = int(want[2].size)
    cap = rng.choice([0, 1, max(total - 1, 0), total, total + 1, rng.randrange(total + 2)])
    skip = rng.choice([None, None, 0, 1, 2, 3])
    bufs = [torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(3)]
    bufs.append(torch.full((cap + 16,), KIND_SENTINEL, dtype=torch.uint8, device="cuda"))
    args = [None if (j == skip or cap == 0) else bufs[j][8:8 + cap] for j in range(4)]
    ret = call(args[0], args[1], args[2], args[3], cap)
    k = min(cap, total)
    ok = ret == total
    for j, w in enumerate(want):
        h = bufs[j].cpu().numpy()
        sent = KIND_SENTINEL if j == 3 else SENTINEL
        ok = ok and (h[:8] == sent).all() and (h[8 + k:] == sent).all()
        ok = ok and ((h[8:8 + k] == sent).all() if (j == skip or cap == 0) else (h[8:8 + k] == w[:k]).all())
    if not ok:
        raise Mismatch(dict(info, capacity=cap, left_out=skip, returned=ret, want=total))


def check_calls(s, hay, view, nd, delim, how, invert, rng, info):
    s = inner(s)
    kw = dict(HOWS[how], invert=invert)
    begins, ends = every_line(view, delim)
    n_lines = int(begins.size)
    (_, _, not_matching), _ = ref_inverted(view, nd, delim, how)
    selected = not_matching if invert else np.setdiff1d(np.arange(1, n_lines + 1, dtype=np.int64), not_matching)
    before, after = draw_amount(rng, n_lines), draw_amount(rng, n_lines)
    numbers, kinds = context_rule(selected, n_lines, before, after)
    want = (begins[numbers - 1], ends[numbers - 1], numbers, kinds)
    info = dict(info, before=before, after=after, invert=invert, selected=int(selected.size))
    got = s.find_lines_context_into(hay, None, None, None, None, 0, before, after, delim, **kw)
    if got != (numbers.size, selected.size):
        raise Mismatch(dict(info, call="find_lines_context_into capacity 0", got=got, want=(int(numbers.size), int(selected.size))))
    check_into(lambda b, e, n, k, cap: s.find_lines_context_into(hay, b, e, n, k, cap, before, after, delim, **kw)[0], want, rng,
               dict(info, call="find_lines_context_into"))
    # lines_around on numbers of its own: some of the selected lines, a few others, 0 and numbers above N
    pool = set(rng.sample(selected.tolist(), min(int(selected.size), rng.randrange(1, 40)))) if selected.size else set()
    pool |= {rng.randrange(n_lines + 3) for _ in range(rng.randrange(4))}
    if rng.random() < 0.3:
        pool |= {0, n_lines + 1, n_lines + 1 + rng.randrange(1 << 40)}
    listed = sorted(pool)
    numbers, kinds = context_rule(listed, n_lines, before, after)
    want = (begins[numbers - 1], ends[numbers - 1], numbers, kinds)
    check_into(lambda b, e, n, k, cap: s.lines_around_into(hay, listed, b, e, n, k, cap, before, after, delim), want, rng,
               dict(info, call="lines_around_into", numbers=listed[:16]))
    return 3


def run(seconds, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = haystacks = 0
    with ss.context_build():
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
                invert = rng.random() < 0.4
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
                calls += check_calls(s, hay, view, nd, delim, how, invert, rng, info)
                cases += 1
            del dev, hay
    return {"fuzz_context": "ok", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases, "calls": calls, "tile_bytes": TILE,
            "part_bytes": ss.CONTEXT_PART_BYTES}


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
