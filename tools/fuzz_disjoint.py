#!/usr/bin/env python3
"""Randomised differential test of the non-overlapping calls (include/sliceslice_hip_disjoint.h) on the GPU against Python's own
bytes.count, re.finditer and bytes.replace: ss_count_disjoint_device, ss_find_all_disjoint_device, ss_replace_device and - on the
overlapping list the same build's find_all gives, and on random ascending lists - ss_select_disjoint_device against the obvious loop.
    python tools/fuzz_disjoint.py SECONDS SEED

Haystacks: one letter, two letters (uniform and with long runs), a short period repeated, text of few letters with word edges and
upper case.  Needles: periodic ones over the haystack's letters (`aa`, `abab`, ...), needles built as x + y + x, needles cut from
the view at its ends and inside, one byte changed, absent.  Every `how`: plain, ignore_case, whole_word and both; the needle's
copies and word bytes stand just outside both ends of the view, at every misalignment.  The find call and the primitive write into
windows of larger buffers whose sentinels on both sides must survive, at capacities that cut the list; replace writes into such a
window too, with replacements shorter than, as long as and longer than the needle, the empty one included.
Prints one JSON line; on the first mismatch a reproducer and exit 1."""
import json
import os
import random
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliceslice_rs_amd as ss  # noqa: E402
from fuzz_matches import Mismatch  # noqa: E402

SENT64, SENT8 = -0x5A5A5A5A5A5A5A5B, 0x5A
GUARD = 64
W = rb"[0-9A-Za-z_]"
B = ss.DISJOINT_BLOCK


def window(cap, dtype=torch.int64):
    sent = SENT64 if dtype == torch.int64 else SENT8
    buf = torch.full((cap + 16,), sent, dtype=dtype, device="cuda")
    return buf, buf[8:8 + cap], sent


def intact(buf, k, sent):
    """the slots in front of the window and behind its first k hold the sentinel"""
    return bool((buf[:8] == sent).all()) and bool((buf[8 + k:] == sent).all())


def draw_haystack(rng, nrng, L):
    kind = rng.choice(["one letter", "two letters", "runs", "period", "words"])
    if kind == "one letter":
        a = np.full(L, ord("a"), dtype=np.uint8)
        for _ in range(rng.randrange(3)):
            if L:
                a[rng.randrange(L)] = ord("b")
    elif kind == "two letters":
        a = nrng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=L, p=rng.choice([[0.5, 0.5], [0.9, 0.1], [0.99, 0.01]]))
    elif kind == "runs":
        a = np.repeat(nrng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=L // 50 + 1), nrng.integers(1, 100, size=L // 50 + 1))[:L]
        a = np.resize(a, L) if a.size < L else a
    elif kind == "period":
        p = rng.choice([1, 2, 3, 4, 5, 7, 12])
        a = np.resize(nrng.choice(np.frombuffer(b"aab", dtype=np.uint8), size=p), L)
    else:
        a = nrng.choice(np.frombuffer(b"aaaAAbB_ -.\n", dtype=np.uint8), size=L)
    return kind, np.ascontiguousarray(a, dtype=np.uint8)


def draw_needle(rng, view):
    L = view.size
    r = rng.random()
    letters = [b"a", b"b", b"A", b"_", b" ", b"-"]
    if r < 0.3:                                                 # periodic
        unit = b"".join(rng.choice(letters[:2]) for _ in range(rng.choice([1, 1, 2, 2, 3])))
        return (unit * rng.choice([2, 2, 3, 4, 5, 9, 40]))[:rng.choice([2, 3, 4, 5, 8, 17, 100])]
    if r < 0.5:                                                 # x + y + x
        x = b"".join(rng.choice(letters[:3]) for _ in range(rng.randrange(1, 5)))
        y = b"".join(rng.choice(letters) for _ in range(rng.randrange(0, 4)))
        return x + y + x
    if r < 0.9 and L:                                           # cut from the view
        n = min(L, rng.choice([1, 2, 2, 3, 3, 4, 5, 8, 16, 33, 200, 5000]))
        at = rng.choice([0, L - n, rng.randrange(L - n + 1)])
        nd = bytearray(view[at:at + n].tobytes())
        if rng.random() < 0.15:
            nd[rng.randrange(n)] ^= 1
        return bytes(nd)
    return rng.choice([b"c", b"zz", b"abc", b"a" * 300])


def rule(hb, nd, nocase, word):
    pat = re.escape(nd)
    if word:
        pat = rb"(?<!" + W + rb")" + pat + rb"(?!" + W + rb")"
    return re.compile(pat, re.I if nocase else 0)


def greedy(offsets, n):
    out, nxt = [], -1
    for p in offsets:
        if p >= nxt:
            out.append(p)
            nxt = p + n
    return out


def check_case(rng, hay, hb, nd, nocase, word, info):
    kw = dict(ignore_case=nocase, whole_word=word)
    pat = rule(hb, nd, nocase, word)
    want = [m.start() for m in pat.finditer(hb)]
    if not nocase and not word and len(want) != hb.count(nd):
        raise Mismatch(dict(info, call="the reference disagrees with itself"))
    with ss.disjoint_build():
        s = ss.DynamicHipSearcher.new_nocase(nd) if nocase else ss.DynamicHipSearcher.new(nd)
    got = s.count_disjoint(hay, **kw)
    if got != len(want):
        raise Mismatch(dict(info, call="count_disjoint", got=got, want=len(want)))
    for cap in {0, 1, max(len(want) - 1, 0), len(want), len(want) + 3, rng.randrange(len(want) + 1)}:
        buf, view, sent = window(cap)
        total = s.find_all_disjoint_into(hay, view, **kw)
        k = min(cap, len(want))
        if total != len(want) or buf[8:8 + k].cpu().tolist() != want[:k] or not intact(buf, k, sent):
            raise Mismatch(dict(info, call="find_all_disjoint_into", capacity=cap, got=total, want=len(want)))
    # the primitive on the overlapping list of the same build
    over = s.find_all(hay, **kw)
    sel = greedy(over.cpu().tolist(), len(nd))
    if sel != want:
        raise Mismatch(dict(info, call="the obvious loop over find_all", got=len(sel), want=len(want)))
    cap = rng.choice([0, len(want), rng.randrange(len(want) + 1)])
    buf, view, sent = window(cap)
    with ss.disjoint_build():
        total = ss.select_disjoint_into(over, len(nd), view)
    k = min(cap, len(want))
    if total != len(want) or buf[8:8 + k].cpu().tolist() != want[:k] or not intact(buf, k, sent):
        raise Mismatch(dict(info, call="select_disjoint_into", capacity=cap, got=total, want=len(want)))
    # replace
    n = len(nd)
    for rl in {0, n, rng.choice([max(n - 1, 0), n + 1, 3 * n, rng.randrange(0, 40)])}:
        rep = bytes(rng.choice(b"xyzXYZ.") for _ in range(rl))
        ref = pat.sub(rep.replace(b"\\", b"\\\\"), hb)
        out = s.replace(hay, rep, **kw)
        if bytes(out.cpu().numpy()) != ref:
            raise Mismatch(dict(info, call="replace", replacement=rep.hex(), got=out.numel(), want=len(ref)))
    return 5 + 3


def check_lists(rng, nrng):
    """the primitive on random strictly ascending lists around the block borders"""
    count = rng.choice([1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B + 7, rng.randrange(1, 5 * B)])
    gaps = nrng.choice(rng.choice([[1], [1, 2], [1, 1, 1, 9], [1, 2, 3, 4, 5, 50], [3, 4]]), size=count)
    offsets = np.cumsum(gaps).astype(np.int64) + rng.choice([0, 5, (1 << 32) - B, 1 << 40])
    n = rng.choice([1, 2, 3, 4, 5, 9, 50, 1000, B, 3 * B, 1 << 33])
    want = greedy(offsets.tolist(), n)
    cap = rng.choice([0, 1, len(want) - 1, len(want), len(want) + 5, rng.randrange(len(want) + 1)])
    buf, view, sent = window(max(cap, 0))
    with ss.disjoint_build():
        total = ss.select_disjoint_into(torch.from_numpy(offsets).cuda(), n, view)
    k = min(max(cap, 0), len(want))
    if total != len(want) or buf[8:8 + k].cpu().tolist() != want[:k] or not intact(buf, k, sent):
        raise Mismatch(dict(call="select_disjoint_into on a list", count=count, n=n, capacity=cap, got=total, want=len(want),
                            first=int(offsets[0]), gaps=sorted(set(gaps.tolist()))))


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = lists = 0
    hows = {}
    try:
        while time.time() < t_end:
            L = rng.choice([0, 1, 17, 300, 4096, 65535, 65536, 65537, 131072 + 5, rng.randrange(1, 400000)])
            kind, host = draw_haystack(rng, nrng, L)
            mis = rng.randrange(16)
            for _ in range(4):
                nd = draw_needle(rng, host)
                nocase, word = rng.random() < 0.4, rng.random() < 0.4
                if nocase:
                    nd = nd.lower()
                pad = (b"a_" * GUARD + nd)[-GUARD:], (nd + b"_a" * GUARD)[:GUARD]      # copies of the needle just outside
                buf = torch.empty(L + 2 * GUARD + 32, dtype=torch.uint8, device="cuda")
                at = (-buf.data_ptr()) % 16 + 16 + mis
                whole = np.concatenate([np.frombuffer(pad[0], dtype=np.uint8), host, np.frombuffer(pad[1], dtype=np.uint8)])
                buf[at:at + whole.size].copy_(torch.from_numpy(whole))
                hay = buf[at + GUARD:at + GUARD + L]
                info = dict(seed=seed, case=cases, kind=kind, len=L, mis=mis, needle=nd.hex() if len(nd) < 64 else "%d bytes" % len(nd),
                            ignore_case=nocase, whole_word=word)
                calls += check_case(rng, hay, host.tobytes(), nd, nocase, word, info)
                hows[(nocase, word)] = hows.get((nocase, word), 0) + 1
                cases += 1
            check_lists(rng, nrng)
            lists += 1
    except Mismatch as e:
        print(json.dumps({"fuzz": "disjoint", "mismatch": e.args[0]}))
        sys.exit(1)
    print(json.dumps({"fuzz": "disjoint", "seed": seed, "seconds": seconds, "cases": cases, "lists": lists, "calls": calls + lists,
                      "by_how": {"%s%s" % ("i" if k[0] else "-", "w" if k[1] else "-"): v for k, v in sorted(hows.items())}, "mismatches": 0}))


if __name__ == "__main__":
    main()
