"""What the case fold costs inside the scan kernels, and what it saves against the only route a caller had before it.  One process,
one 1 GiB buffer, the calls alternating, hipEvents around the stream-ordered forms (the form of tests/test_gpu_zz_lines_timing.py).

(a) count(ignore_case=True) against FOLD-THEN-COUNT: lower-case the haystack into a second buffer with torch, then the
    case-sensitive count on the copy.  Two torch expressions are timed and the cheaper one is the yardstick:
        arith   torch.bitwise_or(hay, ((hay - 65) < 26).to(torch.uint8) << 5, out=low)     (uint8 wrap-around arithmetic)
        table   torch.take(table, hay.long(), out=low)                                     (a 256-entry table gathered by the bytes)
    `arith` is the cheaper of the two on an MI355X (five elementwise launches over 1 GiB; the gather reads an int64 index per
    byte).  No margin is fixed - the copy alone moves twice the bytes - the folding count only has to be faster; the ratio is logged.
(b) count / count_lines of the SAME build (the matches and lines libraries' code, which this library links unchanged) against their
    ignore_case forms: the ratio case-sensitive time / folding time must stay above a floor.  Floor = the lowest ratio of 10 runs,
    one process each, less their spread (max - min): profiles/nocase/timing_test_spread.jsonl, DESIGN.md 5.9."""
import os

import numpy as np
import pytest
import torch

from conftest import timing_log

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GiB = 1 << 30
# case-sensitive time over folding time (1.0 = the fold costs nothing).  Floor = the lowest ratio of 10 runs less their spread.
FLOORS = {
    ("count", "text"): 0.76,            # observed 0.899 / 0.912 / 1.036 (min / median / max)
    ("count", "random"): 0.72,          # observed 0.818 / 0.857 / 0.911
    ("count_lines", "text"): 0.74,      # observed 0.747 / 0.751 / 0.753
    ("count_lines", "random"): 0.76,    # observed 0.776 / 0.781 / 0.785
}


def _fold_arith(hay, low):
    torch.bitwise_or(hay, ((hay - 65) < 26).to(torch.uint8) << 5, out=low)


def _fold_table(hay, low, table):
    torch.take(table, hay.long(), out=low)


def _measure(s, hay, low, rounds=9):
    """medians over `rounds` of: count, count nocase, count_lines, count_lines nocase, fold-then-count (arith), (table) - alternating"""
    d = torch.zeros(6, dtype=torch.int64, device="cuda")
    table = torch.frombuffer(bytearray(bytes(range(256)).lower()), dtype=torch.uint8).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    t = [[] for _ in range(6)]
    for k in range(rounds + 2):
        ev[0].record()
        s.count_async(hay, d[0:1])
        ev[1].record()
        s.count_async(hay, d[1:2], ignore_case=True)
        ev[2].record()
        s.count_lines_async(hay, d[2:3])
        ev[3].record()
        s.count_lines_async(hay, d[3:4], ignore_case=True)
        ev[4].record()
        _fold_arith(hay, low)
        s.count_async(low, d[4:5])
        ev[5].record()
        _fold_table(hay, low, table)
        s.count_async(low, d[5:6])
        ev[6].record()
        torch.cuda.synchronize()
        if k >= 2:                                  # (the first rounds allocate scratch and torch's temporaries)
            for j in range(6):
                t[j].append(ev[j].elapsed_time(ev[j + 1]))
    return [float(np.median(x)) for x in t], d.cpu().tolist()


@pytest.mark.parametrize("kind", ["text", "random"])
def test_the_fold_against_the_copy_and_against_the_case_sensitive_calls(kind):
    import sliceslice_rs_amd as ss
    hay = torch.empty(GiB, dtype=torch.uint8, device="cuda")
    low = torch.empty_like(hay)
    if kind == "text":
        text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
        hay.copy_(text.repeat(GiB // text.numel() + 1)[:GiB])
        needle = b"descriptor"
    else:
        ss.fill_random_device(hay, 0x11E5)
        needle = b"the"
        hay.masked_fill_(hay == ord("t"), ord("u"))         # a `the`-like needle that does not occur, in either case
        hay.masked_fill_(hay == ord("T"), ord("u"))
    with ss.nocase_build():
        s = ss.DynamicHipSearcher.new_nocase(needle)
    (t_c, t_cf, t_l, t_lf, t_arith, t_table), (n_c, n_cf, n_l, n_lf, n_arith, n_table) = _measure(s, hay, low)
    assert n_arith == n_table == n_cf >= n_c and n_lf >= n_l and n_lf <= n_cf and (kind == "text") == (n_cf > n_c > 0)
    t_copy = min(t_arith, t_table)
    r_count, r_lines, r_copy = t_c / t_cf, t_l / t_lf, t_copy / t_cf
    timing_log("nocase_" + kind, count_over_count_nocase=round(r_count, 4), count_lines_over_count_lines_nocase=round(r_lines, 4),
               fold_then_count_over_count_nocase=round(r_copy, 4), count_ms=round(t_c, 4), count_nocase_ms=round(t_cf, 4),
               count_lines_ms=round(t_l, 4), count_lines_nocase_ms=round(t_lf, 4), fold_arith_then_count_ms=round(t_arith, 4),
               fold_table_then_count_ms=round(t_table, 4), count_nocase_gb_per_s=round(GiB / t_cf / 1e6, 1),
               count_lines_nocase_gb_per_s=round(GiB / t_lf / 1e6, 1))
    print("nocase", kind, "count %.4f / %.4f ms (ratio %.4f), count_lines %.4f / %.4f ms (ratio %.4f), fold-then-count arith %.4f table %.4f ms "
          "(%.1fx the folding count)" % (t_c, t_cf, r_count, t_l, t_lf, r_lines, t_arith, t_table, r_copy))
    del hay, low
    torch.cuda.empty_cache()
    assert t_cf < t_copy, (kind, t_cf, t_arith, t_table)                                 # (a)
    assert r_count >= FLOORS[("count", kind)], (kind, r_count, t_c, t_cf)                # (b)
    assert r_lines >= FLOORS[("count_lines", kind)], (kind, r_lines, t_l, t_lf)
