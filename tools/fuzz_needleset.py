#!/usr/bin/env python3
"""Randomised differential test of the needle-set calls (include/sliceslice_hip_needleset.h) on the GPU against the several-needle
calls of the SAME build (include/sliceslice_hip_anyof.h) with one searcher per needle: ss_count_lines_set_device against
ss_count_lines_anyof_device, ss_find_lines_set_device against ss_find_lines_anyof_device - value for value and array for array.
    python tools/fuzz_needleset.py SECONDS SEED

Haystacks, misalignments, needles (1 to 12, cut from the view at its ends and inside, prefixes of others, repeats, one byte
changed, absent, the empty one) and delimiters are tools/fuzz_anyof.py's, with needle copies and delimiters just outside both ends
of the view; every fifth case takes 40 to 400 needles, most of them two to five bytes cut from the view, so that buckets fill and
one-byte and two-byte needles stand beside long ones.  All six `how` values, inverted or not; with the fold the set is given the
needles with some letters in upper case.  before and after as in tools/fuzz_context.py; the set's record call writes into windows of
larger buffers whose sentinels must survive, at capacities around the total and with each of the four arrays left out in turn.
Prints one JSON line; on the first mismatch a reproducer and exit 1."""
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
from fuzz_anyof import draw_needles  # noqa: E402
from fuzz_bounded import haystack  # noqa: E402
from fuzz_context import check_into, draw_amount  # noqa: E402
from fuzz_inverted import HOWS  # noqa: E402
from fuzz_matches import GUARD, TILE, Mismatch, draw_len, draw_needle_len, inner, make_searcher  # noqa: E402


def many_needles(rng, view, how):
    """40 to 400 short needles cut from the view (and a few long ones), so that buckets fill"""
    L, out = view.size, []
    for _ in range(rng.randrange(40, 401)):
        n = rng.choice([1, 2, 2, 3, 3, 3, 4, 4, 5, 6, 7, 9, 17, 40])
        if n > L:
            continue
        at = rng.randrange(L - n + 1)
        nd = bytearray(view[at:at + n].tobytes())
        if rng.random() < 0.3:
            nd[-1] = (nd[-1] + 1 + rng.randrange(254)) & 0xFF
        out.append(bytes(nd).lower() if how.endswith("i") else bytes(nd))
    return out or [b"a"]


def some_upper(rng, nd):
    return bytes(b - 0x20 if 0x61 <= b <= 0x7A and rng.random() < 0.3 else b for b in nd)


def check_calls(st, searchers, hay, n_hint, delim, how, invert, rng, info):
    kw = dict(HOWS[how], invert=invert)
    skw = {k: v for k, v in kw.items() if k != "ignore_case"}
    before, after = (0, 0) if rng.random() < 0.4 else (draw_amount(rng, n_hint), draw_amount(rng, n_hint))
    info = dict(info, before=before, after=after, invert=invert)
    want = ss.count_lines_anyof(searchers, hay, delim, **kw)
    got = st.count_lines(hay, delim, **skw)
    if got != want:
        raise Mismatch(dict(info, call="count_lines", got=got, want=want))
    want = ss.find_lines_anyof_into(searchers, hay, None, None, None, None, 0, before, after, delim, **kw)
    got = st.find_lines_into(hay, None, None, None, None, 0, before, after, delim, **skw)
    if got != want:
        raise Mismatch(dict(info, call="find_lines_into capacity 0", got=got, want=want))
    model = tuple(t.cpu().numpy() for t in ss.find_lines_anyof(searchers, hay, before, after, delim, **kw))
    check_into(lambda b, e, n, k, cap: st.find_lines_into(hay, b, e, n, k, cap, before, after, delim, **skw)[0], model, rng,
               dict(info, call="find_lines_into"))
    return 3


def run(seconds, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = haystacks = needles_sum = largest = 0
    with ss.needleset_build():
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
                needles = many_needles(rng, view, how) if cases % 5 == 4 and L else draw_needles(rng, nrng, view, how, n0)
                nd, e = needles[0], v0 + L
                if nd and rng.random() < 0.5:
                    m = min(len(nd), GUARD - 16)
                    host[v0 - m:v0] = np.frombuffer(nd[-m:], dtype=np.uint8)
                    host[e:e + m] = np.frombuffer(nd[:m], dtype=np.uint8)
                else:
                    host[v0 - 1], host[e] = delim, delim
                dev.copy_(torch.from_numpy(host))
                searchers = [inner(make_searcher(rng, nd)[0] if nd else ss.DynamicHipSearcher(b"")) for nd in needles]
                nocase = how.endswith("i")
                st = ss.NeedleSet([some_upper(rng, nd) for nd in needles] if nocase else needles, ignore_case=nocase)
                largest = max(largest, st.info()["largest_bucket"])
                info = {"MISMATCH": True, "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis, "delimiter": delim, "how": how,
                        "needles": [n.hex() if len(n) <= 64 else n[:32].hex() + ".." for n in needles[:40]], "count": len(needles)}
                calls += check_calls(st, searchers, hay, max(int((view == delim).sum()), 1), delim, how, invert, rng, info)
                st.close()
                needles_sum += len(needles)
                cases += 1
            del dev, hay
    return {"fuzz_needleset": "ok", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases, "calls": calls,
            "needles": needles_sum, "largest_bucket": largest, "tile_bytes": TILE, "oracle": "the anyof calls of the same build"}


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
