"""What the neighbour test costs inside the scan kernels, and what it saves against the only route a caller had before it.  One
process, one 1 GiB buffer, the calls alternating, hipEvents around the stream-ordered forms (the form of
tests/test_gpu_zz_nocase_timing.py).

(1) count_async / count_lines_async of the SAME build (the matches and lines libraries' objects, which this library links
    unchanged: the yardstick, not the code under test) against their whole_word forms: the ratio unbounded time / bounded time
    must stay above a floor.  Three haystacks:
        absent      generator bytes and a needle that does not occur - no confirmed match anywhere, so the bounded kernels execute
                    nothing the unbounded ones do not
        descriptor  the manual's text tiled, `descriptor` (355 occurrences per copy of the text, 286 of them words)
        e           the manual's text tiled, `e`: the one-byte kernel at its densest, a confirmed match in most lanes
    Floor = the lowest ratio of 10 runs, one process each, less their spread (max - min):
    profiles/bounded/timing_test_spread.jsonl, DESIGN.md 5.10.
(2) count(whole_word=True) against the OLD ROUTE: find_all into a device array sized by count, a copy of every offset to the host,
    and the rule applied there with numpy.  No margin is fixed; the bounded count only has to be faster, and the ratio is logged."""
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
_WORD = np.zeros(256, dtype=bool)
_WORD[list(b"0123456789_") + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B))] = True
# unbounded time over bounded time (1.0 = the neighbour test costs nothing).  Floor = the lowest ratio of 10 runs less their spread.
FLOORS = {
    ("count", "absent"): 0.95,              # observed 1.017 / 1.039 / 1.078 (min / median / max)
    ("count_lines", "absent"): 0.90,        # observed 0.960 / 0.987 / 1.018
    ("count", "descriptor"): 0.94,          # observed 1.024 / 1.059 / 1.104
    ("count_lines", "descriptor"): 0.85,    # observed 0.866 / 0.872 / 0.880
    ("count", "e"): 0.67,                   # observed 0.699 / 0.707 / 0.720
    ("count_lines", "e"): 0.72,             # observed 0.727 / 0.729 / 0.733
}


def _measure(s, hay, rounds=9):
    """medians over `rounds` of: count, count whole_word, count_lines, count_lines whole_word - alternating"""
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    t = [[] for _ in range(4)]
    for k in range(rounds + 2):
        ev[0].record()
        s.count_async(hay, d[0:1])
        ev[1].record()
        s.count_async(hay, d[1:2], whole_word=True)
        ev[2].record()
        s.count_lines_async(hay, d[2:3])
        ev[3].record()
        s.count_lines_async(hay, d[3:4], whole_word=True)
        ev[4].record()
        torch.cuda.synchronize()
        if k >= 2:                                  # (the first rounds allocate scratch)
            for j in range(4):
                t[j].append(ev[j].elapsed_time(ev[j + 1]))
    return [float(np.median(x)) for x in t], d.cpu().tolist()


def _old_route(s, hay, host):
    """every offset to the host, then the rule there: what a caller who wanted whole words had to do"""
    offs = s.find_all(hay).cpu().numpy()
    n, L = len(s.needle), host.size
    left = np.where(offs > 0, host[np.maximum(offs - 1, 0)], 0x20)
    right = np.where(offs + n < L, host[np.minimum(offs + n, L - 1)], 0x20)
    return int(np.count_nonzero(~_WORD[left] & ~_WORD[right]))


def _wall(fn, reps):
    out, times = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


@pytest.mark.parametrize("kind", ["absent", "descriptor", "e"])
def test_the_neighbour_test_against_the_unbounded_calls_and_against_the_old_route(kind):
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
    with (_loaded() if getattr(ss.lib(), "has_bounded", False) else ss.bounded_build()):
        s = ss.DynamicHipSearcher(needle)
    (t_c, t_cw, t_l, t_lw), (n_c, n_cw, n_l, n_lw) = _measure(s, hay)
    assert n_cw <= n_c and n_lw <= n_l and n_lw <= n_cw and (kind == "absent") == (n_c == 0) and (kind == "absent") == (n_cw == 0)
    host = hay.cpu().numpy()
    reps = 5 if kind != "e" else 1                         # (the old route moves 8 bytes per occurrence: seconds for `e`)
    t_new, got = _wall(lambda: s.count(hay, whole_word=True), reps)
    t_old, want = _wall(lambda: _old_route(s, hay, host), reps)
    assert got == want == n_cw, (kind, got, want, n_cw)
    r_count, r_lines, r_old = t_c / t_cw, t_l / t_lw, t_old / t_new
    timing_log("bounded_" + kind, count_over_count_word=round(r_count, 4), count_lines_over_count_lines_word=round(r_lines, 4),
               old_route_over_count_word=round(r_old, 2), count_ms=round(t_c, 4), count_word_ms=round(t_cw, 4),
               count_lines_ms=round(t_l, 4), count_lines_word_ms=round(t_lw, 4), count_word_blocking_ms=round(t_new, 4),
               old_route_ms=round(t_old, 3), count_word_gb_per_s=round(GiB / t_cw / 1e6, 1),
               count_lines_word_gb_per_s=round(GiB / t_lw / 1e6, 1), occurrences=n_c, words=n_cw)
    print("bounded", kind, "count %.4f / %.4f ms (ratio %.4f), count_lines %.4f / %.4f ms (ratio %.4f), old route %.3f ms against %.4f "
          "(%.1fx the bounded count)" % (t_c, t_cw, r_count, t_l, t_lw, r_lines, t_old, t_new, r_old))
    del hay, host
    torch.cuda.empty_cache()
    assert t_new < t_old, (kind, t_new, t_old)                                           # (2)
    assert r_count >= FLOORS[("count", kind)], (kind, r_count, t_c, t_cw)                # (1)
    assert r_lines >= FLOORS[("count_lines", kind)], (kind, r_lines, t_l, t_lw)
