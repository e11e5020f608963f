#!/usr/bin/env python3
"""Randomised differential test of the leftmost-longest calls (include/sliceslice_hip_leftmost.h) on the GPU against the rule restated
in Python below (the byte-wise loop of tests/golden/make_leftmost_golden.py, word for word): ss_count_leftmost_set_device, ss_find_all_leftmost_set_device,
ss_replace_set_device and - on random lists of (offset, length) entries - ss_select_leftmost_device against the obvious loop.
    python tools/fuzz_leftmost.py SECONDS SEED

Haystacks: one letter, two letters (uniform and with long runs), a short period repeated, text of few letters with word edges and
upper case.  Needle sets: prefixes of one another (`a`, `aa`, `aaa`), infixes, self-overlapping needles, needles cut from the view,
duplicates and needles equal after the fold.  Every `how`: plain, ignore_case (a property of the set), whole_word and both; a needle's
copy and word bytes stand just outside both ends of the view, at every misalignment.  The find call and the primitive write into
windows of larger buffers whose sentinels on both sides must survive, at capacities that cut the list; replace writes into such a
window at every misalignment, with texts shorter than, as long as and longer than their needles, the empty one included, and one
byte short of the output.  Lists: ascending offsets with runs of equal offsets, dense and sparse, around the block borders.
Prints one JSON line; on the first mismatch a reproducer and exit 1."""
import ctypes
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sliceslice_rs_amd as ss  # noqa: E402

SENT64, SENT32, SENT8 = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B, 0x5A
GUARD = 64
B = ss.LEFTMOST_BLOCK


class Mismatch(Exception):
    pass


class _loaded:
    """the library SLICESLICE_HIP_LIB loaded, where it has the entry points"""
    def __enter__(self):
        return ss.lib()

    def __exit__(self, *a):
        return False


def leftmost_lib():
    return _loaded() if getattr(ss.lib(), "has_leftmost", False) else ss.leftmost_build()


_FOLD = bytes(b | 0x20 if 0x41 <= b <= 0x5A else b for b in range(256))
_WORD = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")


def rule(data, needles, ignore_case=False, whole_word=False):
    """[(offset, index of the needle as given)] of the leftmost-longest, non-overlapping selection: at every free offset the longest
    needle that stands there (folded, with ignore_case; a whole word, with whole_word), else one byte on.  Of equal needles the
    smallest index is named."""
    text = data.translate(_FOLD) if ignore_case else data
    folded = [bytes(n).translate(_FOLD) if ignore_case else bytes(n) for n in needles]
    order = sorted(range(len(folded)), key=lambda k: (-len(folded[k]), k))
    firsts = frozenset(n[:1] for n in folded)
    out, p, end = [], 0, len(text)
    while p < end:
        hit = None
        if text[p:p + 1] in firsts:
            for k in order:
                n = folded[k]
                if not n or not text.startswith(n, p):
                    continue
                if whole_word and ((p > 0 and data[p - 1] in _WORD) or (p + len(n) < end and data[p + len(n)] in _WORD)):
                    continue
                hit = k
                break
        if hit is None:
            p += 1
        else:
            out.append((p, hit))
            p += len(folded[hit])
    return out


def substitute(data, needles, replacements, selected):
    out, at = bytearray(), 0
    for p, k in selected:
        out += data[at:p] + replacements[k]
        at = p + len(needles[k])
    return bytes(out + data[at:])


def window(cap, dtype=torch.int64):
    sent = {torch.int64: SENT64, torch.int32: SENT32, torch.uint8: SENT8}[dtype]
    buf = torch.full((cap + 16,), sent, dtype=dtype, device="cuda")
    return buf, buf[8:8 + cap], sent


def check_window(buf, sent, want, info, what):
    h = buf.cpu().numpy()
    k = len(want)
    if not ((h[:8] == sent).all() and (h[8 + k:] == sent).all() and (h[8:8 + k] == np.asarray(want, dtype=h.dtype)).all()):
        raise Mismatch(dict(info, what=what, got=h[8:8 + min(k, 8)].tolist(), want=list(want[:8])))


def make_haystack(rng, nrng):
    kind = rng.choice(["one", "two", "runs", "period", "text"])
    n = rng.choice([0, 1, 2, 15, 16, 17, rng.randrange(1, 400), rng.randrange(400, 20000), rng.randrange(20000, 70000)])
    if kind == "one":
        host = np.full(n, ord("a"), dtype=np.uint8)
    elif kind == "two":
        host = nrng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=n)
    elif kind == "runs":
        host = np.repeat(nrng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=n // 3 + 1), nrng.integers(1, 9, size=n // 3 + 1))[:n]
    elif kind == "period":
        unit = bytes(rng.choice(b"abc") for _ in range(rng.randrange(1, 6)))
        host = np.frombuffer((unit * (n // len(unit) + 1))[:n], dtype=np.uint8)
    else:
        host = nrng.choice(np.frombuffer(b"abAB _-\n", dtype=np.uint8), size=n, p=[.3, .2, .1, .05, .2, .05, .05, .05])
    return kind, np.ascontiguousarray(host, dtype=np.uint8)


def make_needles(rng, host):
    count = rng.randrange(1, 7)
    needles = []
    for _ in range(count):
        how = rng.randrange(6)
        if how == 0 and needles:                                        # a prefix or an extension of an earlier one
            base = rng.choice(needles)
            n = base[:rng.randrange(1, len(base) + 1)] if rng.random() < 0.5 else base + bytes(rng.choice(b"ab ") for _ in range(rng.randrange(1, 4)))
        elif how == 1 and needles:                                      # an infix, a duplicate, the other case
            base = rng.choice(needles)
            at = rng.randrange(len(base))
            n = rng.choice([base[at:at + rng.randrange(1, len(base) - at + 1)], base, base.swapcase()])
        elif how == 2 and host.size > 2:                                # cut from the view
            at = rng.randrange(host.size - 1)
            n = host[at:at + rng.choice([1, 2, 3, 7, 16, 17, 40])].tobytes()
        elif how == 3:                                                  # x + y + x
            x, y = (bytes(rng.choice(b"ab") for _ in range(rng.randrange(1, 4))) for _ in range(2))
            n = x + y + x
        else:
            n = bytes(rng.choice(b"abAB _") for _ in range(rng.randrange(1, 6)))
        needles.append(n)
    return needles


def check_case(rng, L, hay, host, needles, ignore_case, whole_word, info):
    want = rule(host, needles, ignore_case, whole_word)
    nset = ss.NeedleSet(needles, ignore_case=ignore_case)
    ranks = nset.ranks()
    calls = 1
    got = nset.count_leftmost(hay, whole_word)
    if got != len(want):
        raise Mismatch(dict(info, what="count_leftmost", got=got, want=len(want)))
    for cap in {len(want), rng.randrange(len(want) + 2), 0}:
        k = min(cap, len(want))
        ob, ov, os_ = window(cap)
        rb, rv, rs = window(cap, torch.int32)
        total = nset.find_all_leftmost_into(hay, ov if cap else None, rv if cap else None, cap, whole_word)
        if total != len(want):
            raise Mismatch(dict(info, what="find_all_leftmost_into total", cap=cap, got=total, want=len(want)))
        check_window(ob, os_, [p for p, _ in want[:k]], info, "offsets at capacity %d" % cap)
        check_window(rb, rs, [int(ranks[i]) for _, i in want[:k]], info, "ranks at capacity %d" % cap)
        calls += 1
    # replace: a text per needle, equal for needles of one rank
    by_rank = {}
    texts = []
    for i, n in enumerate(needles):
        r = int(ranks[i])
        if r not in by_rank:
            size = rng.choice([0, 0, 1, max(len(n) - 1, 0), len(n), len(n) + 1, 15, 16, 17, 40])
            by_rank[r] = bytes(rng.choice(b"xyz<>") for _ in range(size))
        texts.append(by_rank[r])
    out = substitute(host, needles, texts, want)
    mis = rng.randrange(16)
    buf = torch.full((len(out) + 96,), SENT8, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + 32 + mis
    reps = (ctypes.c_char_p * len(texts))(*texts)
    lens = (ctypes.c_size_t * len(texts))(*[len(t) for t in texts])
    for cap in ([len(out), len(out) - 1] if out else [0]):
        buf.fill_(SENT8)
        out_len, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = L.ss_replace_set_device(nset._h, hay.data_ptr() if hay.numel() else None, hay.numel(), nset._occurrence_how(whole_word),
                                     ctypes.cast(reps, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p), len(texts),
                                     torch.cuda.current_stream().cuda_stream, buf[at:].data_ptr(), cap, ctypes.byref(out_len), ctypes.byref(count))
        if (rc, out_len.value, count.value) != (0, len(out), len(want)):
            raise Mismatch(dict(info, what="replace results", cap=cap, got=[rc, out_len.value, count.value], want=[0, len(out), len(want)]))
        h = buf.cpu().numpy()
        written = out if cap == len(out) else b""
        if not (bytes(h[at:at + len(written)]) == written and (h[:at] == SENT8).all() and (h[at + len(written):] == SENT8).all()):
            raise Mismatch(dict(info, what="replace bytes", cap=cap, out_mis=mis, texts=[t.hex() for t in texts]))
        calls += 1
    return calls


def check_lists(rng, nrng):
    """the primitive on a random list with runs of equal offsets, its size around the block borders"""
    n = rng.choice([1, 2, B - 1, B, B + 1, 2 * B - 1, 2 * B + 1, rng.randrange(1, 3 * B + 50)])
    step = rng.choice([1, 2, 3, 50, 5000])
    offsets = np.cumsum(nrng.integers(0, step + 1, size=n)).astype(np.int64) + rng.choice([0, 1 << 33])
    longest = rng.choice([1, 2, 7, 60, B + 5])
    lengths = nrng.integers(1, longest + 1, size=n).astype(np.int64)
    for j in range(1, n):                                               # ascending within a run
        if offsets[j] == offsets[j - 1] and lengths[j] <= lengths[j - 1]:
            lengths[j] = lengths[j - 1] + 1
    want, nxt = [], 0
    o, l = offsets.tolist(), lengths.tolist()
    for j in range(n):
        if (j + 1 < n and o[j + 1] == o[j]) or o[j] < nxt:
            continue
        want.append(j)
        nxt = o[j] + l[j]
    info = dict(what="select_leftmost", n=n, step=step, longest=longest)
    d_off, d_len = torch.from_numpy(offsets).cuda(), torch.from_numpy(lengths).cuda()
    for cap in {len(want), rng.randrange(len(want) + 2), 0}:
        k = min(cap, len(want))
        sb, sv, s1 = window(cap)
        wb, wv, s2 = window(cap)
        total = ss.select_leftmost_into(d_off, d_len, sv if cap else None, wv if cap else None, cap)
        if total != len(want):
            raise Mismatch(dict(info, cap=cap, got=total, want=len(want)))
        check_window(sb, s1, [o[j] for j in want[:k]], info, "selected at capacity %d" % cap)
        check_window(wb, s2, want[:k], info, "which at capacity %d" % cap)


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    cases = lists = calls = 0
    hows = {}
    t_end = time.time() + seconds
    try:
        with leftmost_lib() as L:
            while time.time() < t_end:
                kind, host = make_haystack(rng, nrng)
                for _ in range(3):
                    needles = make_needles(rng, host)
                    ignore_case, whole_word = rng.random() < 0.4, rng.random() < 0.4
                    mis = rng.randrange(16)
                    pad = (b"a_" * GUARD + needles[0])[-GUARD:], (needles[0] + b"_a" * GUARD)[:GUARD]      # copies of a needle just outside
                    buf = torch.empty(host.size + 2 * GUARD + 32, dtype=torch.uint8, device="cuda")
                    at = (-buf.data_ptr()) % 16 + 16 + mis
                    whole = np.concatenate([np.frombuffer(pad[0], dtype=np.uint8), host, np.frombuffer(pad[1], dtype=np.uint8)])
                    buf[at:at + whole.size].copy_(torch.from_numpy(whole))
                    hay = buf[at + GUARD:at + GUARD + host.size]
                    info = dict(seed=seed, case=cases, kind=kind, len=int(host.size), mis=mis, needles=[n.hex() for n in needles],
                                ignore_case=ignore_case, whole_word=whole_word)
                    calls += check_case(rng, L, hay, host.tobytes(), needles, ignore_case, whole_word, info)
                    hows[(ignore_case, whole_word)] = hows.get((ignore_case, whole_word), 0) + 1
                    cases += 1
                check_lists(rng, nrng)
                lists += 1
    except Mismatch as e:
        print(json.dumps({"fuzz": "leftmost", "mismatch": e.args[0]}))
        sys.exit(1)
    print(json.dumps({"fuzz": "leftmost", "seed": seed, "seconds": seconds, "cases": cases, "lists": lists, "calls": calls + lists,
                      "by_how": {"%s%s" % ("i" if k[0] else "-", "w" if k[1] else "-"): v for k, v in sorted(hows.items())}, "mismatches": 0}))


if __name__ == "__main__":
    main()
