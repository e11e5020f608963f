#!/usr/bin/env python3
"""Randomised differential test of the occurrence calls of a needle set (include/sliceslice_hip_setmatches.h) on the GPU against
the per-needle calls of the SAME build, merged on the host: ss_count_set_device / _async against one `count` per distinct needle,
ss_find_all_set_device against the `find_all` lists merged by (offset, rank) - on a prefix of the view where it holds more than 1.5 million pairs -
ss_needle_set_ranks against Python's sorted set.
    python tools/fuzz_setmatches.py SECONDS SEED [GIB]

Haystacks, misalignments and needles are tools/fuzz_needleset.py's (1 to 12 needles cut from the view at its ends and inside,
prefixes of others, repeats, one byte changed, absent; every fifth case 40 to 400 short needles so that buckets fill) without the
empty needle, which these calls refuse; every twentieth case is a set LARGER than the 4,096 bins of a workgroup's histogram: up to
6,000 needles of two to four bytes cut from the view.  With and without the fold (the set is given some letters in upper case),
`how` 0 and whole words; needle copies and word bytes stand just outside both ends of the view.  The pair call writes into windows
of larger buffers whose sentinels must survive, at capacities around the total and with each of the two arrays left out.
GIB (more than 4): one more case at the start - a haystack of that many GiB of a byte no needle holds, with dense regions planted
above offset 2^32, checked the same way.
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
from fuzz_matches import GUARD, TILE, Mismatch, draw_len, draw_needle_len  # noqa: E402
from fuzz_needleset import many_needles, some_upper  # noqa: E402

SENT64, SENT32 = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B
HOT_SLOTS = 4096
PAIRS_MOST = 1500000


def larger_than_the_bins(rng, view):
    """up to 6,000 needles of two to four bytes cut from the view: more distinct ones than bins where the view allows it"""
    L, out = view.size, []
    for _ in range(6000):
        n = rng.choice([2, 3, 3, 3, 4, 4])
        if n <= L:
            at = rng.randrange(L - n + 1)
            out.append(view[at:at + n].tobytes())
    return out or [b"a"]


def window(cap, dtype):
    sent = SENT64 if dtype == torch.int64 else SENT32
    buf = torch.full((cap + 16,), sent, dtype=dtype, device="cuda")
    return buf, buf[8:8 + cap], sent


def check_case(st, given, hay, nocase, word, rng, info):
    fold = (lambda b: b.lower()) if nocase else (lambda b: b)
    ds = sorted(set(fold(n) for n in given))
    rank_of = {nd: r for r, nd in enumerate(ds)}
    ranks = np.asarray([rank_of[fold(n)] for n in given], dtype=np.int64)
    if not (st.ranks() == ranks).all() or st.info()["distinct"] != len(ds):
        raise Mismatch(dict(info, call="ranks"))
    searchers = [ss.DynamicHipSearcher.new_nocase(nd) if nocase else ss.DynamicHipSearcher(nd) for nd in ds]
    kw = dict(ignore_case=nocase, whole_word=word)
    counts = np.asarray([s.count(hay, **kw) for s in searchers], dtype=np.int64)
    total = int(counts.sum())
    got = st.count(hay, whole_word=word).cpu().numpy()
    if not (got == counts[ranks]).all():
        k = int(np.flatnonzero(got != counts[ranks])[0])
        raise Mismatch(dict(info, call="count", needle=given[k].hex(), got=int(got[k]), want=int(counts[ranks[k]])))
    if st.count_total(hay, whole_word=word) != total:
        raise Mismatch(dict(info, call="count_total", want=total))
    cbuf, cview, _ = window(len(ds), torch.int64)
    tbuf, tview, _ = window(1, torch.int64)
    st.count_async(hay, cview, tview if rng.random() < 0.7 else None, whole_word=word)
    torch.cuda.synchronize()
    c = cbuf.cpu().numpy()
    if not ((c[8:-8] == counts).all() and (c[:8] == SENT64).all() and (c[-8:] == SENT64).all() and int(tbuf[8].item()) in (total, SENT64)):
        raise Mismatch(dict(info, call="count_async"))
    # the pairs: on the whole view, or - where it holds more than PAIRS_MOST of them - on a prefix of it that holds about that many
    # (merging and comparing tens of millions of pairs on the host would take a case minutes)
    if total > PAIRS_MOST:
        hay = hay[:max(1, int(hay.numel() * (PAIRS_MOST / total)))]
        info = dict(info, pairs_on_prefix=hay.numel())
    lists = [s.find_all(hay, **kw).cpu().numpy() for s in searchers]
    total = int(sum(l.size for l in lists))
    offs = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
    rk = np.concatenate([np.full(l.size, r, dtype=np.int64) for r, l in enumerate(lists)])
    order = np.lexsort((rk, offs))
    offs, rk = offs[order], rk[order]
    calls = 4 + 2 * len(ds)
    for cap in {total, rng.randrange(total + 1), total + 3, 0, min(total, 1)}:
        obuf, oview, _ = window(cap, torch.int64)
        rbuf, rview, _ = window(cap, torch.int32)
        skip = rng.choice([None, None, "offsets", "ranks"])
        n = st.find_all_into(hay, None if skip == "offsets" or not cap else oview, None if skip == "ranks" or not cap else rview, cap, whole_word=word)
        k = min(cap, total)
        o, r = obuf.cpu().numpy(), rbuf.cpu().numpy()
        want_o = np.concatenate([np.full(8, SENT64), offs[:k] if skip != "offsets" else np.full(k, SENT64), np.full(cap - k + 8, SENT64)])
        want_r = np.concatenate([np.full(8, SENT32), rk[:k] if skip != "ranks" else np.full(k, SENT32), np.full(cap - k + 8, SENT32)])
        if n != total or not (o == want_o).all() or not (r == want_r).all():
            raise Mismatch(dict(info, call="find_all_into", capacity=cap, left_out=skip, got=n, want=total))
        calls += 1
    return calls


def above_four_gib(gib, rng, seed):
    """dense regions above offset 2^32 in a haystack of `gib` GiB of zero bytes"""
    n = int(gib * (1 << 30))
    hay = torch.zeros(n, dtype=torch.uint8, device="cuda")
    needles = [b"a", b"ab", b"aba", b"abab", b"ba", b"bab", b"abababab", b"b"]
    wide = torch.from_numpy(np.frombuffer(b"ab" * (1 << 14), dtype=np.uint8).copy()).cuda()
    for at in ((1 << 32) - 7, (1 << 32) + (1 << 20) + 5, n - wide.numel()):
        hay[at:at + wide.numel()] = wide
    st = ss.NeedleSet(needles)
    info = {"MISMATCH": True, "seed": seed, "case": "above 4 GiB", "len": n}
    return check_case(st, needles, hay, False, False, rng, info)


def run(seconds, seed, gib=0.0):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    cases = calls = haystacks = needles_sum = largest = most_distinct = 0
    with ss.setmatches_build():
        if gib > 4:
            calls += above_four_gib(gib, rng, seed)
            cases += 1
        t_end = time.time() + seconds
        while time.time() < t_end:
            kind = rng.choice(["word edges", "words", "words", "abAB", "edges", "text", "text", "ab", "runs", "random", "dense", "free"])
            n0 = draw_needle_len(rng)
            L = min(draw_len(rng, n0), 2 << 20)
            mis = rng.randrange(16)
            host = nrng.integers(0, 256, size=L + 2 * GUARD, dtype=np.uint8)
            v0 = GUARD + mis - (GUARD % 16)
            host[v0:v0 + L] = haystack(rng, nrng, kind, L, 0x0A)
            dev = torch.from_numpy(host).cuda()
            hay = dev[v0:v0 + L]
            haystacks += 1
            for _ in range(4):
                if time.time() >= t_end:
                    break
                nocase, word = rng.random() < 0.4, rng.random() < 0.4
                how = ("w" if word else "") + ("i" if nocase else "")
                view = host[v0:v0 + L]
                if cases % 20 == 19 and L:
                    needles = larger_than_the_bins(rng, view)
                    needles = [n.lower() for n in needles] if nocase else needles
                elif cases % 5 == 4 and L:
                    needles = many_needles(rng, view, how)
                else:
                    needles = draw_needles(rng, nrng, view, how, n0)
                needles = [n for n in needles if n] or [b"a"]
                nd, e = needles[0], v0 + L
                m = min(len(nd), GUARD - 16)
                if rng.random() < 0.5:                          # needle copies just outside both ends
                    host[v0 - m:v0] = np.frombuffer(nd[-m:], dtype=np.uint8)
                    host[e:e + m] = np.frombuffer(nd[:m], dtype=np.uint8)
                else:                                           # word bytes
                    host[v0 - 1], host[e] = ord("x"), ord("_")
                dev.copy_(torch.from_numpy(host))
                given = [some_upper(rng, n) for n in needles] if nocase else needles
                st = ss.NeedleSet(given, ignore_case=nocase)
                stats = st.info()
                largest, most_distinct = max(largest, stats["largest_bucket"]), max(most_distinct, stats["distinct"])
                info = {"MISMATCH": True, "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis, "ignore_case": nocase, "whole_word": word,
                        "needles": [n.hex() if len(n) <= 64 else n[:32].hex() + ".." for n in given[:40]], "count": len(given)}
                calls += check_case(st, given, hay, nocase, word, rng, info)
                st.close()
                needles_sum += len(given)
                cases += 1
            del dev, hay
    return {"fuzz_setmatches": "ok", "seconds": seconds, "seed": seed, "gib": gib, "haystacks": haystacks, "cases": cases, "calls": calls,
            "needles": needles_sum, "largest_bucket": largest, "most_distinct": most_distinct, "hot_slots": HOT_SLOTS, "tile_bytes": TILE,
            "oracle": "count / find_all of one searcher per distinct needle of the same build, merged on the host"}


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
    try:
        out = run(seconds, seed, gib)
    except Mismatch as m:
        print(json.dumps(m.args[0], default=str))
        sys.exit(1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
