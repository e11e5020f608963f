"""What inverting costs, and what it saves against the only route a caller had before it.  One process, one 1 GiB buffer, the calls
alternating, hipEvents around the stream-ordered forms (the form of tests/test_gpu_zz_bounded_timing.py).

(1) count_lines_async of the SAME build (the lines library's objects, which this library links unchanged: the yardstick, not the
    code under test) against count_lines_inverted_async: the same launches plus one single-thread kernel, so the ratio non-inverted
    time / inverted time is expected at about 1 and must stay above a floor.  Two haystacks:
        absent      generator bytes and a needle that does not occur - every line is selected
        descriptor  the manual's text tiled, `descriptor` (337 matching lines of 20,854 per copy of the text)
    Floor = the lowest ratio of 10 runs, one process each, less their spread (max - min):
    profiles/inverted/timing_test_spread.jsonl, DESIGN.md 5.11.
(2) find_lines_inverted against the OLD ROUTE: find_lines for the matching lines, find_lines with the empty needle for all lines,
    both record sets copied to the host, a numpy set difference there.  No margin is fixed; the inverted call only has to be
    faster, and the ratio is logged."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import timing_log
from test_gpu_matches import _loaded

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GiB = 1 << 30
# non-inverted time over inverted time (1.0 = inverting costs nothing).  Floor = the lowest ratio of 10 runs less their spread.
FLOORS = {
    "absent": 0.99,             # observed 1.0237 / 1.0315 / 1.0475 (min / median / max): 1.0237 - 0.0238 = 0.9999
    "descriptor": 0.99,         # observed 1.0143 / 1.0245 / 1.0378: 1.0143 - 0.0235 = 0.9908
}


def _measure(s, hay, rounds=9):
    """medians over `rounds` of count_lines_async and count_lines_inverted_async, alternating"""
    d = torch.zeros(2, dtype=torch.int64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t = [[], []]
    for k in range(rounds + 2):
        ev[0].record()
        s.count_lines_async(hay, d[0:1])
        ev[1].record()
        s.count_lines_inverted_async(hay, d[1:2])
        ev[2].record()
        torch.cuda.synchronize()
        if k >= 2:                                  # (the first rounds allocate scratch)
            for j in range(2):
                t[j].append(ev[j].elapsed_time(ev[j + 1]))
    return [float(np.median(x)) for x in t], d.cpu().tolist()


def _old_route(s, every, hay):
    """the line numbers of the lines without the needle the way a caller got them before: both record sets to the host, the
    difference there"""
    hit = [t.cpu().numpy() for t in s.find_lines(hay)]
    lines = [t.cpu().numpy() for t in every.find_lines(hay)]
    keep = ~np.isin(lines[2], hit[2], assume_unique=True)
    return lines[0][keep], lines[1][keep], lines[2][keep]


def _wall(fn, reps):
    out, times = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


@pytest.mark.parametrize("kind", ["absent", "descriptor"])
def test_inverting_against_the_model_and_against_the_old_route(kind):
    import sliceslice_rs_amd as ss
    hay = torch.empty(GiB, dtype=torch.uint8, device="cuda")
    if kind == "absent":
        ss.fill_random_device(hay, 0x11E5)
        needle = b"the"
        hay.masked_fill_(hay == ord("t"), ord("u"))         # a `the`-like needle that does not occur
    else:
        text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
        hay.copy_(text.repeat(GiB // text.numel() + 1)[:GiB])
        needle = kind.encode()
    with (_loaded() if getattr(ss.lib(), "has_inverted", False) else ss.inverted_build()):
        s, every = ss.DynamicHipSearcher(needle), ss.DynamicHipSearcher(b"")
    (t_l, t_v), (n_l, n_v) = _measure(s, hay)
    nlines = every.count_lines(hay)
    assert n_l + n_v == nlines and (kind == "absent") == (n_l == 0)
    t_new, got = _wall(lambda: s.find_lines_inverted(hay), 3)
    t_old, want = _wall(lambda: _old_route(s, every, hay), 3)
    assert got[0].numel() == n_v == want[0].size
    for g, w in zip(got, want):
        assert (g.cpu().numpy() == w).all(), kind
    ratio, r_old = t_l / t_v, t_old / t_new
    timing_log("inverted_" + kind, count_lines_over_count_lines_inverted=round(ratio, 4), old_route_over_find_lines_inverted=round(r_old, 2),
               count_lines_ms=round(t_l, 4), count_lines_inverted_ms=round(t_v, 4), find_lines_inverted_ms=round(t_new, 3),
               old_route_ms=round(t_old, 3), count_lines_inverted_gb_per_s=round(GiB / t_v / 1e6, 1), matching=n_l, selected=n_v)
    print("inverted", kind, "count_lines %.4f / %.4f ms (ratio %.4f), old route %.3f ms against %.3f (%.1fx find_lines_inverted)" %
          (t_l, t_v, ratio, t_old, t_new, r_old))
    del hay, got, want
    torch.cuda.empty_cache()
    assert t_new < t_old, (kind, t_new, t_old)                                           # (2)
    assert ratio >= FLOORS[kind], (kind, ratio, t_l, t_v)                                # (1)
