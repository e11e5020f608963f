#!/usr/bin/env python3
"""Randomised differential test of the several-needle calls (include/sliceslice_hip_anyof.h) on the GPU against the rule restated in
numpy: S_k = the numbers of the lines the non-inverted model selects for needle k (tools/fuzz_inverted.py's rule), U their union,
N the number of lines; the selected set is U, or 1 .. N without U when inverted; the find call returns what the context rule
(tools/fuzz_context.py) gives for it.    python tools/fuzz_anyof.py SECONDS SEED

Haystacks: tools/fuzz_inverted.py's kinds, lengths and misalignments, with needle copies and delimiters just outside both ends of
the view; 1 to 12 needles cut from the view, some of them prefixes of others, some given twice, some changed in one byte; all six
`how` values, inverted or not; before and after as in tools/fuzz_context.py; the record calls write into windows of larger buffers
whose sentinels must survive, at capacities around the total and with each of the four arrays left out in turn.  Every case also
runs union_numbers on random ascending lists (with 0 and numbers above the limit among them, with and without complement, through a
window at a capacity around the total).  Prints one JSON line; on the first mismatch a reproducer and exit 1."""
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
from fuzz_context import check_into, context_rule, draw_amount, every_line  # noqa: E402
from fuzz_inverted import HOWS, ref_inverted  # noqa: E402
from fuzz_matches import GUARD, SENTINEL, TILE, Mismatch, draw_len, draw_needle_len, inner, make_searcher  # noqa: E402


def draw_needles(rng, nrng, view, how, n0):
    """1 to 12 needles: cut from the view (at its ends and inside), prefixes of earlier ones, repeats, one byte changed, absent"""
    L, bounded = view.size, how[:1] in ("w", "x")
    out = []
    for _ in range(rng.randrange(1, 13)):
        r = rng.random()
        if out and r < 0.2:
            nd = rng.choice(out)                                    # given twice
        elif out and r < 0.4 and len(out[-1]) > 1:
            nd = out[-1][:rng.randrange(1, len(out[-1]))]           # a prefix of another
        else:
            n = n0 if rng.random() < 0.5 else draw_needle_len(rng)
            if rng.random() < 0.03 and not bounded:
                n = 0                                               # the empty needle: every line matches
            if 0 < n <= L and rng.random() < 0.8:
                at = rng.choice([0, L - n, rng.randrange(L - n + 1)])
                nd = bytearray(view[at:at + n].tobytes())
                if rng.random() < 0.2:
                    k = rng.randrange(n)
                    nd[k] = rng.choice([nd[k] ^ 0x20, nd[k] ^ 0x80, (nd[k] + 1 + rng.randrange(254)) & 0xFF])
                nd = bytes(nd)
            else:
                nd = nrng.choice(EDGES, size=n).tobytes()           # (also: longer than the view)
        if bounded and not nd:
            nd = b"a"                                               # (refused with a bound: out of scope)
        out.append(nd.lower() if how.endswith("i") else nd)
    return out


def check_union(rng, limit, info):
    lists = []
    for _ in range(rng.randrange(0, 6)):
        pool = {rng.randrange(1, limit + 1) for _ in range(rng.randrange(0, 200))} if limit else set()
        if rng.random() < 0.3:
            pool |= {0, limit + 1, limit + 1 + rng.randrange(1 << 40)}
        lists.append(sorted(pool))
    complement = rng.random() < 0.5
    flat = np.asarray(sorted({v for l in lists for v in l if 1 <= v <= limit}), dtype=np.int64)
    want = np.setdiff1d(np.arange(1, limit + 1, dtype=np.int64), flat) if complement else flat
    total = int(want.size)
    cap = rng.choice([0, 1, max(total - 1, 0), total, total + 1, rng.randrange(total + 2)])
    buf = torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    ret = ss.union_numbers_into(lists, limit, buf[8:8 + cap] if cap else None, cap, complement)
    h, k = buf.cpu().numpy(), min(cap, total)
    if ret != total or not ((h[:8] == SENTINEL).all() and (h[8 + k:] == SENTINEL).all() and (h[8:8 + k] == want[:k]).all()):
        raise Mismatch(dict(info, call="union_numbers_into", lists=[l[:16] for l in lists], limit=limit, complement=complement, capacity=cap,
                            returned=ret, want=total))


def check_calls(searchers, hay, view, needles, delim, how, invert, rng, info):
    kw = dict(HOWS[how], invert=invert)
    begins, ends = every_line(view, delim)
    n_lines = int(begins.size)
    every = np.arange(1, n_lines + 1, dtype=np.int64)
    union = np.zeros(0, dtype=np.int64)
    for nd in needles:
        (_, _, not_matching), _ = ref_inverted(view, nd, delim, how)
        union = np.union1d(union, np.setdiff1d(every, not_matching))
    selected = np.setdiff1d(every, union) if invert else union
    before, after = draw_amount(rng, n_lines), draw_amount(rng, n_lines)
    numbers, kinds = context_rule(selected, n_lines, before, after)
    want = (begins[numbers - 1], ends[numbers - 1], numbers, kinds)
    info = dict(info, before=before, after=after, invert=invert, selected=int(selected.size))
    got = ss.count_lines_anyof(searchers, hay, delim, **kw)
    if got != selected.size:
        raise Mismatch(dict(info, call="count_lines_anyof", got=got, want=int(selected.size)))
    got = ss.find_lines_anyof_into(searchers, hay, None, None, None, None, 0, before, after, delim, **kw)
    if got != (numbers.size, selected.size):
        raise Mismatch(dict(info, call="find_lines_anyof_into capacity 0", got=got, want=(int(numbers.size), int(selected.size))))
    check_into(lambda b, e, n, k, cap: ss.find_lines_anyof_into(searchers, hay, b, e, n, k, cap, before, after, delim, **kw)[0], want, rng,
               dict(info, call="find_lines_anyof_into"))
    check_union(rng, rng.choice([0, 1, 31, 32, 33, n_lines, 65536, 65537, 70000 + rng.randrange(100000)]), info)
    return 4


def run(seconds, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = haystacks = needles_sum = 0
    with ss.anyof_build():
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
            for _ in range(6):
                if time.time() >= t_end:
                    break
                how = rng.choice(list(HOWS))
                invert = rng.random() < 0.4
                view = host[v0:v0 + L]
                needles = draw_needles(rng, nrng, view, how, n0)
                nd, e = needles[0], v0 + L
                if nd and rng.random() < 0.5:
                    m = min(len(nd), GUARD - 16)
                    host[v0 - m:v0] = np.frombuffer(nd[-m:], dtype=np.uint8)
                    host[e:e + m] = np.frombuffer(nd[:m], dtype=np.uint8)
                else:
                    host[v0 - 1], host[e] = delim, delim
                dev.copy_(torch.from_numpy(host))
                searchers, descs = [], []
                for nd in needles:
                    s, desc = make_searcher(rng, nd) if nd else (ss.DynamicHipSearcher(b""), "new")
                    searchers.append(inner(s))
                    descs.append(desc)
                view = host[v0:v0 + L]
                info = {"MISMATCH": True, "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis, "delimiter": delim, "how": how,
                        "needles": [n.hex() if len(n) <= 64 else n[:32].hex() + ".." for n in needles], "searchers": descs}
                calls += check_calls(searchers, hay, view, needles, delim, how, invert, rng, info)
                needles_sum += len(needles)
                cases += 1
            del dev, hay
    return {"fuzz_anyof": "ok", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases, "calls": calls, "needles": needles_sum,
            "tile_bytes": TILE, "segment_lines": ss.ANYOF_SEGMENT_LINES}


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
