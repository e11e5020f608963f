#!/usr/bin/env python3
"""Randomised differential test of the batched every-occurrence calls on the GPU (include/sliceslice_hip_matches_batched.h:
ss_count_batched, ss_find_all_batched) against a plain overlapping restatement in numpy.
    python tools/fuzz_matches_batched.py SECONDS SEED

Every round builds one batch inside ONE haystack blob and ONE needle blob: 1 .. 300 problems (so the grid goes from hundreds of
slices per problem down to a few dozen), haystack ranges of 0 bytes to a few MiB at odd begins - disjoint, aliased (many needles,
one haystack) or overlapping - over random bytes, two-letter text, runs of one byte and periodic patterns; needles of 0 .. 2,000
bytes cut from their own haystack (present, usually many times in the low-entropy kinds), mutated (absent or nearly), longer than
the haystack, one byte, self-overlapping; copies of a needle straddling both ends of its range.  Ranges go in as CSR offsets or as
explicit (begin, end) pairs.  Checked per round: count_batched == the reference counts; find_all_batched's counts, row_begin,
total and every offset; a capacity cut at a random place with sentinels in front of and behind the caller's window; the relations
to search_batched and find_batched.  Prints one JSON line; on the first mismatch a reproducer and exit 1."""
import ctypes
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


def make_blob(rng, nprng, size):
    kind = rng.choice(["random", "two_letters", "run", "periodic", "text16"])
    if kind == "random":
        return kind, nprng.integers(0, 256, size, dtype=np.uint8)
    if kind == "two_letters":
        return kind, nprng.choice(np.frombuffer(b"ab", dtype=np.uint8), size)
    if kind == "run":
        blob = np.full(size, rng.randrange(256), dtype=np.uint8)
        for _ in range(rng.randrange(4)):                       # a few foreign bytes break the run
            blob[rng.randrange(size)] = rng.randrange(256)
        return kind, blob
    if kind == "periodic":
        p = rng.choice([2, 3, 5, 16, 17, 64, 1000])
        return kind, np.resize(nprng.integers(0, 256, p, dtype=np.uint8), size)
    return kind, nprng.choice(np.frombuffer(b"etaoin shrdlu,.\n", dtype=np.uint8), size)


def pick_len(rng, most):
    r = rng.random()
    if r < 0.08:
        return 0
    if r < 0.3:
        return rng.randrange(1, 64)
    if r < 0.6:
        return min(most, rng.choice([1, 2, 3, 4, 8]) * rng.choice([1024, 4096, TILE, 2 * TILE]) + rng.choice([-1, 0, 0, 1, 7]))
    if r < 0.9:
        return rng.randrange(1, min(most, 40 * TILE) + 1)
    return rng.randrange(1, most + 1)


def one_round(rng, nprng, stats):
    count = rng.choice([1, 2, 3, 7, 30, 100, 300])
    most = rng.choice([4 * TILE, 64 * TILE, 256 * TILE]) if count <= 30 else 8 * TILE
    layout = rng.choice(["disjoint", "csr", "aliased", "overlapping"])
    hay_ranges = []
    if layout == "aliased":
        size = pick_len(rng, most) + 64
        kind, blob = make_blob(rng, nprng, size)
        b = rng.randrange(0, 33)
        hay_ranges = [(b, size - rng.randrange(0, 17))] * count
    else:
        lens = [pick_len(rng, most) for _ in range(count)]
        size = sum(lens) + 40 * count + 64
        kind, blob = make_blob(rng, nprng, size)
        at = rng.randrange(0, 17)
        for L in lens:
            if layout == "overlapping" and hay_ranges and rng.random() < 0.5:
                pb, pe = hay_ranges[-1]
                nb = rng.randrange(pb, pe + 1)
                hay_ranges.append((nb, min(size, nb + L)))
            else:
                hay_ranges.append((at, at + L))
                at += L + (0 if layout == "csr" else rng.randrange(0, 40))
    needles, nd_ranges = bytearray(b"\x00" * rng.randrange(0, 9)), []
    for i, (hb, he) in enumerate(hay_ranges):
        L = he - hb
        r = rng.random()
        if r < 0.06:
            nd = b""
        elif r < 0.12 and L + 1 <= 2000:
            nd = bytes(nprng.integers(0, 256, L + rng.randrange(1, 5), dtype=np.uint8))          # n > len
        elif L == 0:
            nd = bytes([rng.randrange(256)])
        else:
            n = min(L, rng.choice([1, 1, 2, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64, 200, 1000, 2000]))
            o = rng.choice([0, L - n, rng.randrange(0, L - n + 1)])
            nd = bytearray(blob[hb + o:hb + o + n].tobytes())
            if rng.random() < 0.3:
                nd[rng.randrange(n)] ^= 1 << rng.randrange(8)                                     # absent, or nearly
            nd = bytes(nd)
            if len(nd) > 1 and rng.random() < 0.3:
                # a copy straddling an end of the range (the reference below is taken from the bytes as they end up): no match of
                # this problem, and the neighbour that begins there does not see its front part
                src = np.frombuffer(nd, dtype=np.uint8)
                cut = rng.randrange(1, len(nd))
                at_ = he - cut if rng.random() < 0.5 else hb - cut
                if at_ >= 0 and at_ + len(nd) <= size:
                    blob[at_:at_ + len(nd)] = src
        nd_ranges.append((len(needles), len(needles) + len(nd)))
        needles += nd
        if layout != "csr" and rng.random() < 0.3:
            needles += b"\xAA" * rng.randrange(1, 5)
    needles += b"\x00"
    # the reference, from the host bytes as they are now
    want = [ref_offsets(blob[hb:he], bytes(needles[nb:ne])) for (hb, he), (nb, ne) in zip(hay_ranges, nd_ranges)]
    want_counts = np.array([w.size for w in want], dtype=np.int64)
    want_rows = np.concatenate([[0], np.cumsum(want_counts)]).astype(np.int64)
    want_all = np.concatenate(want) if want else np.zeros(0, dtype=np.int64)
    total = int(want_rows[-1])
    d_hay = torch.from_numpy(blob).cuda()
    d_nd = torch.from_numpy(np.frombuffer(bytes(needles), dtype=np.uint8).copy()).cuda()
    hb_t = torch.tensor([r[0] for r in hay_ranges], dtype=torch.int64, device="cuda")
    he_t = torch.tensor([r[1] for r in hay_ranges], dtype=torch.int64, device="cuda")
    nb_t = torch.tensor([r[0] for r in nd_ranges], dtype=torch.int64, device="cuda")
    ne_t = torch.tensor([r[1] for r in nd_ranges], dtype=torch.int64, device="cuda")
    kw = dict(hay_ranges=(hb_t, he_t), needle_ranges=(nb_t, ne_t))
    args = (d_hay, None, d_nd, None)
    if layout == "csr":
        args = (d_hay, torch.tensor([r[0] for r in hay_ranges] + [hay_ranges[-1][1]], dtype=torch.int64, device="cuda"), d_nd,
                torch.tensor([r[0] for r in nd_ranges] + [nd_ranges[-1][1]], dtype=torch.int64, device="cuda"))
        kw = {}
        stats["csr"] += 1
    what = dict(kind=kind, layout=layout, count=count, hay_ranges=hay_ranges[:8], nd_ranges=nd_ranges[:8])

    def bad(msg, **more):
        raise Mismatch(json.dumps(dict(what, error=msg, **more), default=str))

    got = ss.count_batched(*args, **kw).cpu().numpy()
    stats["calls"] += 1
    if not np.array_equal(got, want_counts):
        i = int(np.flatnonzero(got != want_counts)[0])
        bad("count_batched", problem=i, got=int(got[i]), want=int(want_counts[i]), hay=hay_ranges[i], needle=bytes(needles[nd_ranges[i][0]:nd_ranges[i][1]])[:64])
    counts, rows, offs = ss.find_all_batched(*args, **kw)
    stats["calls"] += 2
    if not np.array_equal(counts.cpu().numpy(), want_counts) or not np.array_equal(rows.cpu().numpy(), want_rows):
        bad("find_all_batched counts / rows")
    if not np.array_equal(offs.cpu().numpy(), want_all):
        g = offs.cpu().numpy()
        k = int(np.flatnonzero(g != want_all[:g.size])[0]) if g.size == want_all.size else -1
        bad("find_all_batched offsets", at=k, got_size=int(g.size), want_size=int(want_all.size))
    # a capacity cut: a window of a larger buffer whose sentinels must survive
    cap = rng.choice([0, 1, total, total + 3, rng.randrange(0, total + 1)])
    buf = torch.full((cap + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    L = ss.lib()
    hbp, hep, _ = ss.searcher._ranges(args[1], *(kw.get("hay_ranges") or (None, None)))
    nbp, nep, _ = ss.searcher._ranges(args[3], *(kw.get("needle_ranges") or (None, None)))
    rows2 = torch.empty(count + 1, dtype=torch.int64, device="cuda")
    tot = ss.searcher._u64(0)
    rc = L.ss_find_all_batched(d_hay.data_ptr(), hbp, hep, d_nd.data_ptr(), nbp, nep, count, ss.searcher._current_stream_handle(), None,
                               rows2.data_ptr(), buf.data_ptr() + 64 if cap else None, cap, ctypes.byref(tot))
    stats["calls"] += 1
    if rc != 0 or tot.value != total or not np.array_equal(rows2.cpu().numpy(), want_rows):
        bad("capacity cut: rc / total / rows", cap=cap, rc=rc, total=tot.value)
    b = buf.cpu().numpy()
    k = min(cap, total)
    if not np.array_equal(b[8:8 + k], want_all[:k]) or (b[:8] != SENTINEL).any() or (b[8 + k:] != SENTINEL).any():
        bad("capacity cut: offsets / sentinels", cap=cap)
    # relations to the bool and leftmost-offset forms
    flags = ss.search_batched(*args, **kw).cpu().numpy()
    first = ss.find_batched(*args, **kw).cpu().numpy()
    stats["calls"] += 2
    if not np.array_equal(flags != 0, want_counts > 0):
        bad("search_batched disagrees with the counts")
    want_first = np.array([int(w[0]) if w.size else -1 for w in want], dtype=np.int64)
    if not np.array_equal(first, want_first):
        bad("find_batched disagrees with the first offsets")
    stats["rounds"] += 1
    stats["problems"] += count
    stats["matches"] += total


def lib_ctx():
    """The build under test: SLICESLICE_HIP_LIB when it names a library with the batched entry points, else the batched build."""
    class _Keep:
        def __enter__(self):
            return ss.lib()

        def __exit__(self, *a):
            return False
    return _Keep() if getattr(ss.lib(), "has_matches_batched", False) else ss.matches_batched_build()


def campaign(seconds, seed):
    rng = random.Random(seed)
    nprng = np.random.default_rng(seed)
    stats = dict(rounds=0, calls=0, problems=0, matches=0, csr=0)
    t_end = time.time() + seconds
    with lib_ctx():
        while time.time() < t_end:
            one_round(rng, nprng, stats)
    return stats


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    try:
        stats = campaign(seconds, seed)
    except Mismatch as e:
        print("MISMATCH (seed %d): %s" % (seed, e))
        sys.exit(1)
    print(json.dumps(dict(fuzz_matches_batched="ok", seed=seed, seconds=seconds, **stats)))


if __name__ == "__main__":
    main()
