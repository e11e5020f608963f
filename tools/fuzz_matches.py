#!/usr/bin/env python3
"""Randomised differential test of every-occurrence search on the GPU (include/sliceslice_hip_matches.h: ss_count_device /
_async, ss_find_all_device) against a plain overlapping restatement in numpy, and of the calls' relations to search_in / find
against Python's bytes.find.    python tools/fuzz_matches.py SECONDS SEED [GIB]

Small mode: random haystack kinds, lengths from 0 to ~40 MiB (mostly multiples of 1, 4, 16 or 32 KiB, give or take 1 or n),
misalignments 0..15, needles of 1..3000 bytes (self-overlapping ones included) through `new`, `with_position`, filter triples
(near, d > 0 pairs, far pairs, pairs alone) and MemchrHipSearcher; the needle, its prefix or its suffix sits just outside both ends
of the view, and find_all writes into a window of a larger buffer whose sentinels on both sides must survive.
Big mode (GIB): a random haystack of GIB GiB from which one byte value is scrubbed; every needle holds that byte, so only dense match
regions written at random places (around 2^32, in the last workgroup, across the tile borders inside two-tile workgroups) match,
and the reference is built from host copies of the regions.  Prints one JSON line; on the first mismatch a reproducer and exit 1."""
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sliceslice_rs_amd as ss  # noqa: E402

SENTINEL = -0x5A5A5A5A5A5A5A5B
GUARD = 4096                  # bytes on both sides of a small-mode view: room for a needle copy plus the misalignment
TILE = 16384                  # bytes of candidates per tile (256 threads, U = 4: 16 pieces of 1 KiB)


def ref_offsets(h, n):
    """Every i with h[i:i+len(n)] == n (overlapping), ascending."""
    h = np.asarray(h, dtype=np.uint8)
    n = np.frombuffer(bytes(n), dtype=np.uint8)
    L, m = h.size, n.size
    if m == 0:
        return np.arange(L + 1, dtype=np.int64)
    if m > L:
        return np.zeros(0, dtype=np.int64)
    cand = np.flatnonzero(h[:L - m + 1] == n[0])
    for k in range(1, m):
        if cand.size == 0:
            break
        cand = cand[h[cand + k] == n[k]]
    return cand.astype(np.int64)


class Mismatch(Exception):
    pass


def lib_ctx():
    """The build under test: SLICESLICE_HIP_LIB when it names a library with the matches entry points, else the matches build."""
    class _Keep:
        def __enter__(self):
            return ss.lib()

        def __exit__(self, *a):
            return False
    return _Keep() if getattr(ss.lib(), "has_matches", False) else ss.matches_build()


def make_searcher(rng, nd):
    """(searcher, description): the constructors and filter triples a caller can reach."""
    n = len(nd)
    with lib_ctx():
        if n == 1:
            r = rng.random()
            if r < 0.35:
                return ss.MemchrHipSearcher(nd[0]), "memchr"
            return ss.DynamicHipSearcher(nd, 0 if r < 0.6 else None), "new" if r >= 0.6 else "with_position 0"
        r = rng.random()
        if r < 0.3:
            return ss.DynamicHipSearcher(nd), "new"
        if r < 0.5:
            p = rng.randrange(min(n, 16)) if rng.random() < 0.6 else rng.randrange(n)
            return ss.DynamicHipSearcher(nd, p), "with_position %d" % p
        s = ss.DynamicHipSearcher(nd)
        kinds = ["near", "pair_alone"] + (["d_pair"] if n >= 17 else []) + (["far_pair"] if n >= 1010 else [])
        kind = rng.choice(kinds)
        if kind == "near":                           # a triple within 15 bytes of the first
            a = rng.randrange(min(n - 1, 16))
            b = rng.randrange(a + 1, min(n, a + 16))
            c = rng.randrange(a + 1, min(n, a + 16))
            if c == b:
                s.set_filter(a, b)
            else:
                s.set_filter(a, b, c)
        elif kind == "pair_alone":                   # a plain pair: the device adds its own third byte
            a = rng.randrange(min(n - 1, 16))
            s.set_filter(a, rng.randrange(a + 1, min(n, a + 16)))
        elif kind == "d_pair":                       # 16 .. 1007 apart: the cross-lane kernels
            a = rng.randrange(min(n - 16, 16))
            s.set_filter(a, rng.randrange(a + 16, min(n, a + 1008)))
        else:                                        # farther: the caller's byte is tested in memory
            a = rng.randrange(min(n - 1008, 16))
            s.set_filter(a, rng.randrange(a + 1008, n))
        return s, "%s %r" % (kind, s.filter3)


def inner(s):
    return s._inner if isinstance(s, ss.MemchrHipSearcher) else s


def check_calls(s, hay, want, bf, cap_choice, rng, info):
    """count, count_async, find_all, find_all_into (sentinels on both sides) against `want`; search_in / find against `bf` (bytes.find
    in small mode, the reference's first offset or -1 in big mode).  Returns the number of calls checked."""
    total = int(want.size)
    got = s.count(hay)
    if got != total:
        raise Mismatch(dict(info, call="count", got=got, want=total))
    d = torch.full((3,), SENTINEL, dtype=torch.int64, device=hay.device)
    inner(s).count_async(hay, d[1:2])
    dv = d.cpu().tolist()
    if dv[1] != total or dv[0] != SENTINEL or dv[2] != SENTINEL:
        raise Mismatch(dict(info, call="count_async", got=dv, want=total))
    fa = s.find_all(hay).cpu().numpy()
    if fa.size != total or not (fa == want).all():
        bad = int(np.flatnonzero(fa[:min(fa.size, total)] != want[:min(fa.size, total)])[:1].sum()) if min(fa.size, total) else 0
        raise Mismatch(dict(info, call="find_all", got_size=int(fa.size), want=total, first_diff=bad,
                            got_near=fa[max(0, bad - 2):bad + 3].tolist(), want_near=want[max(0, bad - 2):bad + 3].tolist()))
    cap = {"0": 0, "1": 1, "total-1": max(total - 1, 0), "total": total, "total+1": total + 1,
           "random": rng.randrange(total + 2)}[cap_choice]
    buf = torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device=hay.device)
    ret = inner(s).find_all_into(hay, buf[8:8 + cap])
    b = buf.cpu().numpy()
    k = min(cap, total)
    if ret != total or not (b[8:8 + k] == want[:k]).all() or not (b[:8] == SENTINEL).all() or not (b[8 + k:] == SENTINEL).all():
        raise Mismatch(dict(info, call="find_all_into", capacity=cap, returned=ret, want=total,
                            window_ok=bool((b[8:8 + k] == want[:k]).all()), front_ok=bool((b[:8] == SENTINEL).all()),
                            back_ok=bool((b[8 + k:] == SENTINEL).all())))
    si, fd = s.search_in(hay), s.find(hay)           # the search side: count > 0 exactly when search_in, find_all[0] == find
    if si != (bf >= 0) or fd != (bf if bf >= 0 else None) or (total > 0) != (bf >= 0) or (total and int(want[0]) != bf):
        raise Mismatch(dict(info, call="relations", search_in=si, find=fd, bytes_find=bf, count=total,
                            first=int(want[0]) if total else None))
    return 6


def make_haystack(rng, nrng, kind, L):
    if kind == "random":
        return nrng.integers(0, 256, size=L, dtype=np.uint8)
    if kind == "abcd":
        a = np.resize(nrng.choice(np.frombuffer(b"abcd", dtype=np.uint8), size=max(1, min(L, 4096))), L).copy()
        if L:
            a[nrng.integers(0, L, size=max(1, L // 997))] = ord("e")
        return a
    if kind == "ab":
        a = np.full(L, ord("a"), dtype=np.uint8)
        if L:
            a[nrng.integers(0, L, size=max(1, L // 257))] = ord("b")
        return a
    if kind == "text":
        t = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "data", "i386.txt"), "rb").read()
        return np.resize(np.frombuffer(t, dtype=np.uint8), L).copy()
    if kind == "zeros":
        a = np.zeros(L, dtype=np.uint8)
        if L:
            a[rng.randrange(L)] = 1
        return a
    return nrng.integers(0, 255, size=L, dtype=np.uint8)            # "ff_free": 0xFF never occurs; needles are planted


def draw_len(rng, n0):
    if rng.random() < 0.08:
        return rng.randrange(0, 80)
    unit = rng.choice([1024, 4096, 16384, 32768])
    top = (40 << 20) if rng.random() < 0.06 else (1 << 20) if rng.random() < 0.7 else (6 << 20)
    L = unit * rng.randrange(1, top // unit + 1)
    L += rng.choice([0, 0, 1, -1, n0, -n0, n0 + 1, -n0 - 1, rng.randrange(-16, 17)])
    return max(0, L)


def draw_needle_len(rng):
    r = rng.random()
    if r < 0.45:
        return rng.choice([1, 2, 3, 4, 5, 7, 8])
    if r < 0.8:
        return rng.choice([9, 12, 13, 15, 16, 17, 20, 24, 31, 32, 33, 40, 64])
    if r < 0.93:
        return rng.choice([65, 100, 127, 257, 500, 1000])
    return rng.randrange(1001, 3001)


def small(seconds, seed):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    t_end = time.time() + seconds
    cases = calls = haystacks = 0
    dense_kinds = ("abcd", "ab", "text", "zeros")
    while time.time() < t_end:
        kind = rng.choice(["random", "abcd", "ab", "text", "zeros", "ff_free"])
        n0 = draw_needle_len(rng)
        L = draw_len(rng, n0)
        mis = rng.randrange(16)
        host = np.empty(L + 2 * GUARD, dtype=np.uint8)
        host[:] = nrng.integers(0, 256, size=host.size, dtype=np.uint8)
        v0 = GUARD + mis - (GUARD % 16)                          # the view starts `mis` bytes past a 16-byte boundary
        host[v0:v0 + L] = make_haystack(rng, nrng, kind, L)
        dev = torch.from_numpy(host).cuda()
        hay = dev[v0:v0 + L]
        haystacks += 1
        for _ in range(8):
            if time.time() >= t_end:
                break
            n = n0 if rng.random() < 0.5 else draw_needle_len(rng)
            if kind in dense_kinds and L * n > 3e8:      # keep the numpy reference within a second or so
                n = max(1, min(n, int(3e8 // max(L, 1))))
            view = host[v0:v0 + L]
            r = rng.random()
            if kind == "ff_free" or (r < 0.25 and n <= L):
                nd = bytearray(nrng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
                if kind == "ff_free":
                    nd[rng.randrange(n)] = 0xFF
                    for _ in range(rng.choice([0, 1, 3, 20])):   # planted copies (they may overlap each other)
                        if n <= L:
                            p = rng.choice([0, L - n, rng.randrange(L - n + 1)])
                            view[p:p + n] = np.frombuffer(bytes(nd), dtype=np.uint8)
            elif r < 0.45:                                        # self-overlapping: a short period repeated
                per = bytes(nrng.integers(0, 256, size=rng.choice([1, 2, 3, 5]), dtype=np.uint8))
                nd = bytearray((per * (n // len(per) + 1))[:n])
                if n <= L and rng.random() < 0.7:                 # ... and a dense run of it inside the view
                    ln = rng.randrange(n, min(L, n + 4 * TILE) + 1)
                    p = rng.randrange(L - ln + 1)
                    view[p:p + ln] = np.frombuffer((per * (ln // len(per) + 1))[:ln], dtype=np.uint8)
            elif n <= L:                                          # cut from the view, maybe with one byte changed
                at = rng.choice([0, L - n, rng.randrange(L - n + 1)])
                nd = bytearray(view[at:at + n].tobytes())
                if rng.random() < 0.3:
                    k = rng.randrange(n)
                    nd[k] = (nd[k] + 1 + rng.randrange(254)) & 0xFF
            else:
                nd = bytearray(nrng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
            nd = bytes(nd)
            arr = np.frombuffer(nd, dtype=np.uint8)
            # the needle, or its prefix / suffix, just outside both ends of the view (straddling copies reach into it)
            front = rng.choice(["whole", "straddle", "suffix"])
            j = rng.randrange(1, n) if n > 1 else 1
            if front == "whole" or n == 1:
                host[v0 - n:v0] = arr
            elif front == "straddle":                             # starts n - j... bytes before the view: j bytes inside
                jj = min(j, L)
                host[v0 - (n - jj):v0 + jj] = arr[:n]
            else:
                host[v0 - j:v0] = arr[:j]                         # a prefix of the needle ending at the view's start
            back = rng.choice(["whole", "straddle", "prefix"])
            e = v0 + L
            if back == "whole" or n == 1:
                host[e:e + n] = arr
            elif back == "straddle":
                jj = min(j, L)
                host[e - jj:e - jj + n] = arr
            else:
                host[e:e + n - j] = arr[j:]                       # a suffix of the needle starting at the view's end
            dev.copy_(torch.from_numpy(host))
            s, desc = make_searcher(rng, nd)
            want = ref_offsets(host[v0:v0 + L], nd)
            cap_choice = rng.choice(["0", "1", "total-1", "total", "total+1", "random"])
            info = {"MISMATCH": True, "mode": "small", "seed": seed, "case": cases, "kind": kind, "len": L, "mis": mis,
                    "needle": nd.hex() if n <= 128 else nd[:64].hex() + "..", "needle_len": n, "searcher": desc,
                    "capacity": cap_choice, "front": front, "back": back, "j": j}
            calls += check_calls(s, hay, want, host[v0:v0 + L].tobytes().find(nd), cap_choice, rng, info)
            cases += 1
        del dev, hay
    return {"fuzz_matches": "ok", "mode": "small", "seconds": seconds, "seed": seed, "haystacks": haystacks, "cases": cases,
            "calls": calls}


def big(seconds, seed, gib):
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    n_bytes = int(gib * (1 << 30))
    cus = ss.device_info()["compute_units"]
    hay = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ss.fill_random_device(hay, 0xA11 + seed)
    scrub = rng.randrange(256)
    step = 256 << 20
    for a in range(0, n_bytes, step):                             # no byte of value `scrub` in the background
        v = hay[a:a + step]
        v.masked_fill_(v == scrub, (scrub + 1) & 0xFF)
    torch.cuda.synchronize()
    t_end = time.time() + seconds
    rounds = calls = regions_total = 0
    while time.time() < t_end:
        n = rng.choice([1, 2, 3, 5, 8, 12, 16, 17, 24, 40, 64, 100, 300, 1100])
        per = nrng.integers(0, 256, size=rng.choice([1, 2, 3, 4, 7]) if n > 1 else 1, dtype=np.uint8)
        per[rng.randrange(per.size)] = scrub                      # every needle holds the scrubbed byte
        unit = per.tobytes()
        nd = (unit * (n // len(unit) + 1))[:n]
        if scrub not in nd:
            nd = nd[:-1] + bytes([scrub])
        s, desc = make_searcher(rng, nd)
        # dense regions: a repeat of the needle's period (every period offset matches), some of them broken by a changed byte
        spots = []
        for _ in range(rng.choice([3, 10, 40])):
            t = rng.randrange(max(1, n_bytes // TILE))
            spots.append(t * TILE + rng.randrange(-600, 600))    # across a tile border (inside or between workgroups)
        spots += [n_bytes - rng.randrange(n, 3 * TILE), rng.randrange(0, 300), n_bytes - n]
        if n_bytes > (1 << 32) + 4 * TILE:
            spots += [(1 << 32) - rng.randrange(0, 2000), (1 << 32) + rng.randrange(-n, 40)]
        regions = []
        for p in sorted(spots):
            ln = rng.choice([n, n + 1, 2 * n + 7, 1200, 5000])
            p = max(0, min(p, n_bytes - ln))
            if regions and p < regions[-1][0] + regions[-1][1] + 1:
                continue
            regions.append((p, ln))
        saved = [hay[p:p + ln].clone() for p, ln in regions]
        for p, ln in regions:
            body = np.frombuffer((unit * (ln // len(unit) + 2))[:ln], dtype=np.uint8).copy()
            if rng.random() < 0.2:
                body[rng.randrange(ln)] ^= 0x5A
            hay[p:p + ln] = torch.from_numpy(body).cuda()
        want = []
        for p, ln in regions:                                     # host copies, widened by n on both sides
            a, b = max(0, p - n), min(n_bytes, p + ln + n)
            want.append(ref_offsets(hay[a:b].cpu().numpy(), nd) + a)
        want = np.unique(np.concatenate(want)) if want else np.zeros(0, dtype=np.int64)
        cap_choice = rng.choice(["total", "total", "total-1", "random", "1"])
        info = {"MISMATCH": True, "mode": "big", "seed": seed, "round": rounds, "gib": gib, "compute_units": cus, "scrubbed": scrub,
                "needle": nd.hex(), "needle_len": n, "searcher": desc, "capacity": cap_choice, "regions": regions[:50]}
        calls += check_calls(s, hay, want, int(want[0]) if want.size else -1, cap_choice, rng, info)
        for (p, ln), sv in zip(regions, saved):
            hay[p:p + ln] = sv
        regions_total += len(regions)
        rounds += 1
    del hay
    torch.cuda.empty_cache()
    return {"fuzz_matches": "ok", "mode": "big", "gib": gib, "seconds": seconds, "seed": seed, "rounds": rounds, "regions": regions_total,
            "calls": calls}


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    try:
        out = big(seconds, seed, float(sys.argv[3])) if len(sys.argv) > 3 else small(seconds, seed)
    except Mismatch as m:
        print(json.dumps(m.args[0], default=str))
        sys.exit(1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
