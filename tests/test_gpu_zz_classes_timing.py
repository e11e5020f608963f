"""What an exact class costs against the route a caller had before, and what the class kernel's tables cost a pattern that needs
none of them.  One process, the manual's text tiled to 256 MiB, the calls alternating, a host clock around synchronised calls, warmed
up (the form of tests/test_gpu_zz_masked_timing.py).

(a) `[0-9]{3}` through ClassPattern.count against the earlier route: MaskedPattern(cover).find_all - the superset `3? 3? 3?` - a copy
    of every offset to the host and the numpy class check of the three bytes.  The ratio is old / new.
(b) `t?e` through ClassPattern.from_masked against MaskedPattern of the same pattern and build.  The ratio is class / masked: what the
    added tables and the skipped exact test cost a pattern without inexact positions.

The yardsticks are existing calls of the same build, never the code under test, and every array is compared before anything is
timed.  The floor of (a) is 0.8 times the lowest ratio of 10 runs, one process each, rounded down; the ceiling of (b) 1.1 times the
highest, rounded up to two decimals: profiles/classes/timing_test_spread.jsonl, DESIGN.md 5.20.

The spread of (a) is wide and is written down as it was measured: the class count comes right behind the earlier route's host
work, during which the device sits idle for some 20 ms, and its wall time in that place was 0.38 ms in one run and 4 to 7 ms in the
others (0.80 ms of device time by events at four times this size, tools/classes_bench.py), while the earlier route took 22.8 to 28.0 ms in all
ten.  (b) alternates two device calls without such a gap and moved by 2 %: 0.134 to 0.136 ms against 0.133 to 0.135 ms."""
import os

import numpy as np
import pytest
import torch

from conftest import timing_log
from test_gpu_matches import _loaded
from test_gpu_zz_masked_timing import _wall

pytestmark = [pytest.mark.gpu, pytest.mark.timing]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SIZE = 256 * MiB
FLOOR_OLD_ROUTE_OVER_CLASSES = 2.6       # (a) observed 3.27 / 8.95 / 61.12 (min / median / max): 0.8 * 3.27 = 2.616
CEILING_CLASSES_OVER_MASKED = 1.13       # (b) observed 1.002 / 1.008 / 1.020 (min / median / max): 1.1 * 1.020 = 1.122


def test_the_class_count_against_the_earlier_route_and_against_the_masked_count():
    import sliceslice_rs_amd as ss
    text = torch.from_numpy(np.fromfile(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), dtype=np.uint8)).cuda()
    hay = text.repeat(SIZE // text.numel() + 1)[:SIZE].contiguous()
    lib = _loaded if getattr(ss.lib(), "has_classes", False) else ss.classes_build
    with lib():
        digits = ss.ClassPattern(r"[0-9]{3}")
        nibbles = ss.MaskedPattern(*ss.classes_cover(digits.sets))
        value, mask = ss.parse_hex("74 ?? 65")
        as_class, as_masked = ss.ClassPattern.from_masked(value, mask), ss.MaskedPattern(value, mask)
    assert (nibbles.value, nibbles.mask) == (b"000", b"\xf0\xf0\xf0") and digits.info()["inexact"] == 3 and as_class.info()["inexact"] == 0
    host = hay.cpu().numpy()

    def old_route():
        offsets = nibbles.find_all(hay).cpu().numpy()           # every place the nibble masks accept, copied to the host
        keep = np.ones(offsets.size, dtype=bool)
        for i in range(3):
            keep &= host[offsets + i] <= ord("9")               # (the high nibble is 3: the class is the low nibble up to 9)
        return offsets[keep]

    # every array first
    want = old_route()
    assert digits.count(hay) == want.size and want.size > 0
    assert np.array_equal(digits.find_all(hay).cpu().numpy(), want)
    assert as_class.count(hay) == as_masked.count(hay) > 0
    assert torch.equal(as_class.find_all(hay), as_masked.find_all(hay))
    (new_ms, old_ms), (n_new, got) = _wall([lambda: digits.count(hay), old_route], 5)
    assert n_new == want.size and np.array_equal(got, want)
    (class_ms, masked_ms), (n_class, n_masked) = _wall([lambda: as_class.count(hay), lambda: as_masked.count(hay)], 9)
    assert n_class == n_masked
    r_a, r_b = old_ms / new_ms, class_ms / masked_ms
    timing_log("classes", old_route_over_class_count=round(r_a, 2), class_over_masked_count=round(r_b, 3), class_three_digits_ms=round(new_ms, 3),
               old_route_ms=round(old_ms, 3), class_t_any_e_ms=round(class_ms, 3), masked_t_any_e_ms=round(masked_ms, 3),
               occurrences=int(want.size))
    print("classes: [0-9]{3} %.3f ms against the earlier route's %.3f (%.2fx); t?e %.3f ms against the masked kernel's %.3f (%.3fx)" %
          (new_ms, old_ms, r_a, class_ms, masked_ms, r_b))
    del hay, host
    torch.cuda.empty_cache()
    assert r_a >= FLOOR_OLD_ROUTE_OVER_CLASSES, (r_a, old_ms, new_ms)                           # (a)
    assert r_b <= CEILING_CLASSES_OVER_MASKED, (r_b, class_ms, masked_ms)                       # (b)
