"""GPU tests of the byte-class calls (include/sliceslice_hip_classes.h, libsliceslice_hip_classes.so) against THE RULE restated in
numpy (tests/test_classes_cpu.py: rule_offsets, rule_lines), against the searchers and the masked patterns of the same build, and
against tests/golden/classes_kat.json (Python's re).  Every comparison is of integers and exact; every output array is a window of
a larger one whose sentinels on both sides must survive.  The geometry's units are lane 16 B, piece 1 KiB, wave 4 KiB, tile 16 KiB
and workgroup 128 KiB, so - the manual's text aside - no view is larger than 300,000 bytes (two workgroups and a tail); views of
more than one chunk of 256 workgroups are tests/test_gpu_set_grids.py's."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_classes_cpu import members, rule_lines, rule_offsets, sets_of                # noqa: E402
from test_gpu_masked import LANE, PIECE, TILE, WAVE, WG, Arena, Window                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 18, 33, 64, 257, 4096)
UNITS = (LANE, PIECE, WAVE, TILE, WG)
# the six kinds of position: single value, exact mask, range, union of ranges, negated single, `.`
KINDS = {"single": r"7", "mask": r"[Ff]", "range": r"[0-9]", "union": r"[0-9A-F]", "negated": r"[^z]", "any": r"."}
ALPHABET = b"0799:AFGfz`_ \n\xe9"


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def mk_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.classes_build()`."""
    return _loaded() if getattr(ss.lib(), "has_classes", False) else ss.classes_build()


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with mk_lib(m):
        pass
    return m


@pytest.fixture(scope="module")
def manual():
    return open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()


@pytest.fixture(scope="module")
def d_manual(manual):
    return torch.from_numpy(np.frombuffer(manual, dtype=np.uint8).copy()).cuda()


def make(ss, text, ignore_case=False):
    with mk_lib(ss):
        return ss.ClassPattern(text, ignore_case)


def plant(host, sets, at, rng):
    """a copy of the pattern at `at`: a random member of every position's set"""
    table = members(sets)
    host[at:at + len(table)] = [int(rng.choice(np.flatnonzero(row))) for row in table]


def inside(offsets, begin, length, n):
    """the occurrences of the arena that lie wholly inside the view [begin, begin + length), as offsets of the view"""
    return offsets[(offsets >= begin) & (offsets + n <= begin + length)] - begin


def check_occurrences(pat, dev, want, what):
    assert pat.count(dev) == want.size, (what, "count")
    w = Window(want.size + 2)
    assert pat.find_all_into(dev, w.view, want.size + 2) == want.size, (what, "find_all total")
    w.check(want, (what, "find_all"))


def check_lines(pat, dev, host, delimiter, what):
    begin, end, number = rule_lines(host, pat.sets, delimiter)
    assert pat.count_lines(dev, bytes([delimiter])) == begin.size, (what, "count_lines")
    wb, we, wn = Window(begin.size + 2), Window(begin.size + 2), Window(begin.size + 2)
    assert pat.find_lines_into(dev, wb.view, we.view, wn.view, begin.size + 2, bytes([delimiter])) == begin.size, (what, "find_lines total")
    wb.check(begin, (what, "begin"))
    we.check(end, (what, "end"))
    wn.check(number, (what, "number"))


def arrangement(which, n, rng):
    """the pattern text of one arrangement for n positions, or None where it needs a longer pattern"""
    inexact = [KINDS["range"], KINDS["union"], KINDS["negated"]]
    pick = lambda pool: pool[int(rng.integers(0, len(pool)))]                  # noqa: E731
    if which == "inexact_only":
        # (beyond 1,024 inexact positions the library refuses: every fourth position of the longest pattern)
        return "".join(pick(inexact) if n <= 1024 or i % 4 == 0 else "." for i in range(n))
    if which == "mixed":
        items = [pick(list(KINDS.values())) for _ in range(n)]
        items[n // 2] = pick(inexact)
        if n > 1024:
            items = [x if i % 4 == 0 or x not in inexact else "." for i, x in enumerate(items)]
        return "".join(items)
    if which == "inexact_at_filter":                                # the only two positions that are not `.` are inexact
        if n < 2:
            return None
        d = min(n - 1, int(rng.integers(1, 17)))
        s = (n - 1 - d) // 2
        return "".join(pick(inexact[:2]) if i in (s, s + d) else "." for i in range(n))
    assert which == "only_nonwild_inexact"
    return "".join(pick(inexact[:2]) if i == n // 2 else "." for i in range(n))


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["inexact_only", "mixed", "inexact_at_filter", "only_nonwild_inexact"])
def test_the_rule_over_lengths_kinds_arrangements_misalignments_and_view_lengths(ss, which):
    rng = np.random.default_rng(21)
    full = TILE + 3000 + 13                                        # two tiles of one workgroup, an odd tail
    for n in LENGTHS:
        if n > 64 and which in ("inexact_at_filter", "only_nonwild_inexact"):
            continue
        text = arrangement(which, n, rng)
        if text is None:
            continue
        pat = make(ss, text)
        info = pat.info()
        assert info["n"] == n == len(pat) and info["inexact"] >= 1
        if which == "inexact_at_filter":
            assert info["distance"] != 0 and info["inexact"] == 2 and info["masked"] == n - 2
        if which == "only_nonwild_inexact":
            assert (info["anchor"], info["distance"], info["inexact"]) == (n // 2, 0, 1)
        size = (WG if n <= 64 else full) + 2 * n + 64
        host = rng.choice(np.frombuffer(ALPHABET, dtype=np.uint8), size)
        for at in (0, 1, 15, 16, full - n, full - n + 1, full - n + 15, TILE - n // 2, TILE - n // 2 + 1, 5000, 5001 + n // 2):
            if 0 <= at and at + n <= host.size:
                plant(host, pat.sets, at, rng)
        arena = Arena(host)
        every = rule_offsets(host, pat.sets)
        assert every.size >= 3
        views = [(mis, length) for mis in range(16) for length in (0, n - 1, n, n + 1, full)]
        if n <= 64:
            views += [(mis, unit + k) for mis in (0, 7) for unit in UNITS for k in (-1, 0, 1)]
        for mis, length in views:
            dev, hv = arena.view(mis, length)
            check_occurrences(pat, dev, inside(every, mis, length, n), (which, n, mis, length))
            if length == full and n <= 64 and mis in (0, 5, 15):
                check_lines(pat, dev, hv, 10, (which, n, mis, length, "lines"))


# ---- near misses ---------------------------------------------------------------------------------------------------------------------
def near_miss_host(sets, i, near, size, mis, rng):
    """An arena of 0xFF (which passes no cover of these patterns but `.`) with ten copies that hold `near` at position i - that
    byte on both sides of a border of every unit - and a true copy behind each; the offsets of both kinds in the view at `mis`."""
    n = len(sets)
    host = np.full(size + 16, 0xFF, dtype=np.uint8)
    good, bad = [], []
    for unit, lo, hi in ((LANE, 50, 100), (PIECE, 3, 5), (WAVE, 2, 3), (TILE, 1, 3), (WG, 1, 2)):
        for multiple, side in ((lo, -1), (hi, 0)):
            p = unit * multiple + side - i                          # the arena's index is the stream position of the wrong byte
            plant(host, sets, p, rng)
            host[p + i] = near
            bad.append(p - mis)
            plant(host, sets, p + n + 7, rng)
            good.append(p + n + 7 - mis)
    return host, good, bad


@pytest.mark.parametrize("text", [r"[0-9]\w[0-9A-F]x[0-9][Ff]\w{2}[0-9A-F]", r"[0-9].{14}\w[0-9A-F]{2}.{19}[Ff][0-9]"])
def test_a_byte_the_cover_accepts_and_the_set_does_not_fails_at_every_inexact_position_and_border(ss, text):
    """What a missing or wrong exact test fails: beside every planted copy stands a copy that differs in ONE inexact position by a
    byte the cover accepts and the set does not, with that byte on both sides of every border from 16 B to 128 KiB."""
    rng = np.random.default_rng(22)
    wrong = {KINDS["range"]: ord(":"), KINDS["union"]: ord("G"), r"\w": ord("`")}
    size = 2 * WG + 37000
    with mk_lib(ss):
        pat = ss.ClassPattern(text)
        cover = ss.MaskedPattern(*ss.classes_cover(pat.sets))
        by_item = {item: ss.parse_classes(item)[0] for item in wrong}
    table, n = members(pat.sets), len(pat)
    value, mask = np.frombuffer(cover.value, dtype=np.uint8), np.frombuffer(cover.mask, dtype=np.uint8)
    inexact = [i for i in range(n) if table[i].sum() != 1 << bin(~mask[i] & 0xFF).count("1")]
    assert len(inexact) == pat.info()["inexact"] >= 5
    for i in inexact:
        near = next(b for item, b in wrong.items() if (by_item[item] == pat.sets[i]).all())
        assert not table[i][near] and (near & mask[i]) == value[i]
        for mis in (0, 5):
            host, good, bad = near_miss_host(pat.sets, i, near, size, mis, rng)
            dev, hv = Arena(host).view(mis, size)
            want = rule_offsets(hv, pat.sets)
            assert want.tolist() == sorted(good) and len(good) == len(bad) == 10
            check_occurrences(pat, dev, want, ("near miss", i, mis))
            assert cover.count(dev) - pat.count(dev) == len(bad), (i, mis)
            assert sorted(set(cover.find_all(dev).cpu().tolist()) - set(want.tolist())) == sorted(bad)
            check_lines(pat, dev, hv, 10, ("near miss", i, mis, "lines"))


# ---- the ends of the view ------------------------------------------------------------------------------------------------------------
def test_copies_that_begin_before_the_view_or_end_behind_it_never_count(ss):
    rng = np.random.default_rng(23)
    for text in (r"[0-9]", r"[0-9][0-9A-F]", r"\w{16}", r"[0-9A-F].{31}[0-9]", r"[0-9]{257}"):
        pat = make(ss, text)
        n = len(pat)
        for mis in (0, 1, 15):
            for length in (n + 40, WAVE + 5):
                lo = (n + 31) // 16 * 16 + mis                      # the view's first byte at misalignment `mis`
                hi = lo + length
                host = np.full(hi + n + 16, 0xFF, dtype=np.uint8)
                plant(host, pat.sets, lo - 1, rng)                  # begins one byte before the view
                plant(host, pat.sets, hi - n + 1, rng)              # ends one byte behind it
                if n > 1:
                    host[lo + n - 1] = host[hi - n] = 0xFF          # (so that neither runs on inside)
                plant(host, pat.sets, lo - n, rng)                  # just before, just behind
                plant(host, pat.sets, hi, rng)
                dev, hv = Arena(host).view(lo, length)
                assert dev.data_ptr() % 16 == mis
                want = rule_offsets(hv, pat.sets)
                if n > 1 and "." not in text:
                    assert want.size == 0
                check_occurrences(pat, dev, want, ("ends", text, mis, length))
                assert pat.count_lines(dev) == rule_lines(hv, pat.sets, 10)[0].size
                for at in (lo, hi - n):                              # ... and a whole copy inside, touching either end, counts
                    plant(host, pat.sets, at, rng)
                    dev, hv = Arena(host).view(lo, length)
                    want = rule_offsets(hv, pat.sets)
                    assert at - lo in want.tolist()
                    check_occurrences(pat, dev, want, ("ends, inside", text, mis, length, at))


# ---- capacity ------------------------------------------------------------------------------------------------------------------------
def test_capacities_with_each_optional_array_left_out_in_turn(ss):
    rng = np.random.default_rng(24)
    size = 2 * WG + 30000
    pat = make(ss, r"q[0-9]z")
    host = rng.choice(np.frombuffer(b"abc:", dtype=np.uint8), size + 16)
    spots = [5, 100, 103, 4000, TILE - 1, WG - 2, WG + 7, 2 * WG + 1, 2 * WG + 20000, size - 3]
    for p in spots:
        plant(host, pat.sets, p, rng)
    host[[200, 201, 202]] = np.frombuffer(b"q:z", dtype=np.uint8)   # (a near miss)
    dev, hv = Arena(host).view(0, size)
    want = rule_offsets(hv, pat.sets)
    total = want.size
    assert want.tolist() == spots and pat.count(dev) == total
    assert pat.find_all_into(dev, None, 0) == total
    for cap in (0, 1, 4, total - 1, total, total + 1):             # (4: reached inside the first workgroup, occurrences in the third)
        w = Window(total + 4)
        assert pat.find_all_into(dev, w.view, cap) == total, cap
        w.check(want[:cap], ("capacity", cap))                      # nothing at index `cap` or beyond
    assert pat.find_all(dev).cpu().tolist() == spots and pat.find_all(dev, capacity=3).cpu().tolist() == spots[:3]
    host[[50, 3000, WG + 100, 2 * WG + 10]] = 10
    dev, hv = Arena(host).view(0, size)
    records = rule_lines(hv, pat.sets, 10)
    total = records[0].size
    assert total == 5
    for cap in (0, 1, total - 1, total, total + 1):
        for left_out in (None, 0, 1, 2):
            windows = [None if k == left_out else Window(8) for k in range(3)]
            views = [None if w is None else w.view for w in windows]
            assert pat.find_lines_into(dev, views[0], views[1], views[2], cap) == total, (cap, left_out)
            for w, rec in zip(windows, records):
                if w is not None:
                    w.check(rec[:cap], ("line capacity", cap, left_out))
    assert pat.find_lines_into(dev, None, None, None, 0) == total and pat.find_lines_into(dev, None, None, None, 3) == total
    assert [x.cpu().tolist() for x in pat.find_lines(dev)] == [r.tolist() for r in records]


# ---- relations -----------------------------------------------------------------------------------------------------------------------
def test_literals_equal_the_searchers_and_masked_patterns_equal_the_masked_calls_of_the_same_build(ss, manual, d_manual):
    with mk_lib(ss):
        for word in (b"descriptor", b"the", b"e", b"  ", b"segment register", b"no such phrase in the manual"):
            s, pat = ss.DynamicHipSearcher.new(word), ss.ClassPattern.from_bytes(word)
            assert pat.info()["single"] == len(word) and pat.info()["inexact"] == 0
            assert pat.count(d_manual) == s.count(d_manual) == len(pat.find_all(d_manual)), word
            assert torch.equal(pat.find_all(d_manual), s.find_all(d_manual)), word
        for word in (b"intel", b"Segment", b"80386", b"gdt", b"x"):
            # (the folding searcher takes its needle without upper-case letters)
            s, pat = ss.DynamicHipSearcher.new(word.lower()), ss.ClassPattern.from_bytes(word, ignore_case=True)
            assert pat.info()["inexact"] == 0 and pat.count(d_manual) == s.count(d_manual, ignore_case=True), word
        for hexes in ("74 ?? 65", "3? 3? 3?", "64 ?? 73 63 72 ?? ?? 74 6f 72", "?0 ?d", "??", "2e ?? 0a"):
            value, mask = ss.parse_hex(hexes)
            m, pat = ss.MaskedPattern(value, mask), ss.ClassPattern.from_masked(value, mask)
            assert pat.info()["inexact"] == 0 and ss.classes_cover(pat.sets) == (m.value, m.mask)
            assert (pat.info()["anchor"], pat.info()["distance"]) == (m.info()["anchor"], m.info()["distance"])
            assert pat.count(d_manual) == m.count(d_manual) and int(pat.count_async(d_manual).cpu()[0]) == int(m.count_async(d_manual).cpu()[0])
            assert torch.equal(pat.find_all(d_manual), m.find_all(d_manual)), hexes
            for delimiter in (b"\n", b" "):
                assert pat.count_lines(d_manual, delimiter) == m.count_lines(d_manual, delimiter), hexes
                for got, want in zip(pat.find_lines(d_manual, delimiter), m.find_lines(d_manual, delimiter)):
                    assert torch.equal(got, want), hexes
        assert ss.ClassPattern.from_masked(b"ab").count(d_manual) == ss.DynamicHipSearcher.new(b"ab").count(d_manual)
        # the exact class finds a subset of what its nibble masks find
        exact, nibbles = ss.ClassPattern(r"[0-9]{3}"), ss.MaskedPattern.from_hex("3? 3? 3?")
        a, b = set(exact.find_all(d_manual).cpu().tolist()), set(nibbles.find_all(d_manual).cpu().tolist())
        assert a < b and (len(a), len(b)) == (3504, 3951)


# ---- lines ---------------------------------------------------------------------------------------------------------------------------
def test_lines_under_three_delimiters_with_sets_that_accept_the_delimiter(ss):
    rng = np.random.default_rng(26)
    with mk_lib(ss):
        patterns = [ss.ClassPattern(t) for t in (r"a.b", r"a[^x]b", r"\s\s", r"[0-9][^0-9]", r"[ab]{3}", r"[^a]{17}")]
        for pat in patterns[:2]:
            for text, lines in ((b"a\nb", 0), (b"a\nb\n", 0), (b"ayb", 1), (b"\nayb", 1), (b"ayb\n", 1), (b"a\nbayb", 1), (b"", 0), (b"\n\n\n", 0),
                                (b"axb", 1 if pat is patterns[0] else 0)):
                dev, hv = Arena(np.frombuffer(text, dtype=np.uint8)).view(0, len(text))
                assert pat.count_lines(dev) == lines, text
                check_lines(pat, dev, hv, 10, text)
            assert pat.info(b"\n")["accepts_delimiter"] == 1 and pat.info(b"a")["accepts_delimiter"] == 1
        assert patterns[1].info(b"x")["accepts_delimiter"] == 0 and patterns[2].info(b"\n")["accepts_delimiter"] == 1
        assert patterns[2].info(b"a")["accepts_delimiter"] == 0 and ss.ClassPattern(r"[0-9]").info(b"\n")["accepts_delimiter"] == 0
        for text, lines in ((b" \n ", 0), (b"  \n", 1), (b"\t \n \x0b", 2), (b"a \n\n b", 0)):
            dev, hv = Arena(np.frombuffer(text, dtype=np.uint8)).view(0, len(text))
            assert patterns[2].count_lines(dev) == lines, text
        size = WG + 9000
        for delimiter in (10, 0, ord("a")):
            dense = rng.choice(np.frombuffer(bytes([delimiter, ord("a"), ord("b"), ord(" "), ord("7")]), dtype=np.uint8), size + 16)
            free = rng.choice(np.frombuffer(b"bcd 7x" if delimiter == ord("a") else b"abc 7x", dtype=np.uint8), size + 16)
            for name, host in (("dense", dense), ("free", free)):
                arena = Arena(host)
                for mis, length in ((0, size), (7, size - 100), (15, TILE + 1)):
                    dev, hv = arena.view(mis, length)               # (`free` ends in an unterminated last line)
                    for k, pat in enumerate(patterns):
                        check_lines(pat, dev, hv, delimiter, (name, delimiter, mis, length, k))
        # an occurrence in the first workgroup whose line is closed in the second, and one whose line never closes
        wild = patterns[1]
        host = np.full(2 * WG + 500, ord("c"), dtype=np.uint8)
        host[WG - 30:WG - 27] = np.frombuffer(b"ayb", dtype=np.uint8)
        host[100] = host[WG + 4000] = 10
        host[2 * WG + 100:2 * WG + 103] = np.frombuffer(b"a\nb", dtype=np.uint8)
        host[2 * WG + 200:2 * WG + 203] = np.frombuffer(b"axb", dtype=np.uint8)
        host[2 * WG + 300:2 * WG + 303] = np.frombuffer(b"ayb", dtype=np.uint8)
        dev, hv = Arena(host).view(0, host.size)
        begin, end, number = rule_lines(hv, wild.sets, 10)
        assert begin.tolist() == [101, 2 * WG + 102] and end.tolist() == [WG + 4000, host.size] and number.tolist() == [2, 4]
        check_lines(wild, dev, hv, 10, "across workgroups")


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_every_case_of_the_fixture_on_the_manual(ss, manual, d_manual):
    kat = json.load(open(os.path.join(GOLDEN, "classes_kat.json")))
    assert kat["bytes"] == len(manual) and sum(c["ignore_case"] for c in kat["cases"]) == 2
    for c in kat["cases"]:
        pat = make(ss, c["pattern"], c["ignore_case"])
        assert pat.count(d_manual) == c["count"], c["name"]
        offsets = pat.find_all(d_manual).cpu().tolist()
        assert len(offsets) == c["count"], c["name"]
        if "offsets" in c:
            assert offsets == c["offsets"], c["name"]
        else:
            digest = hashlib.sha256(np.asarray(offsets, dtype="<u8").tobytes()).hexdigest()
            assert digest == c["offsets_sha256"] and offsets[:16] == c["first"] and offsets[-16:] == c["last"], c["name"]
        assert pat.count_lines(d_manual, bytes([c["delimiter"]])) == c["lines"], c["name"]
        assert pat.find_lines(d_manual, bytes([c["delimiter"]]))[0].numel() == c["lines"], c["name"]


# ---- the limits on the device -------------------------------------------------------------------------------------------------------
def test_a_pattern_at_both_limits_and_the_full_length_finds_its_planted_copies(ss):
    rng = np.random.default_rng(27)
    tables = np.zeros((4096, 256), dtype=bool)
    ids = np.arange(4096) % 64
    tables[np.arange(4096), 4 * ids] = True
    tables[np.arange(1024), 4 * ids[:1024] + 3] = True              # {b, b + 3}: the cover also accepts b + 1 and b + 2
    sets = sets_of(tables)
    with mk_lib(ss):
        pat = ss.ClassPattern.from_sets(sets)
        cover = ss.MaskedPattern(*ss.classes_cover(sets))
    info = pat.info()
    assert (info["n"], info["single"], info["masked"], info["inexact"], info["distinct"]) == (4096, 3072, 0, 1024, 64)
    host = np.full(3 * 4096 + 100, 0xFF, dtype=np.uint8)
    plant(host, sets, 7, rng)
    plant(host, sets, 4096 + 50, rng)
    host[4096 + 50 + 1023] = 253                                    # the last inexact position: {252, 255} does not hold 253, its cover does
    plant(host, sets, 2 * 4096 + 60, rng)
    host[2 * 4096 + 60] = 1                                         # the first: {0, 3} does not hold 1, its cover does
    dev, hv = Arena(host).view(3, host.size - 3)
    want = rule_offsets(hv, sets)
    assert want.tolist() == [4]
    check_occurrences(pat, dev, want, "limits")
    assert cover.count(dev) == 3 and pat.count_lines(dev) == 1


# ---- the async form in a graph ------------------------------------------------------------------------------------------------------
def test_the_async_count_is_captured_and_replayed_on_two_contents(ss):
    rng = np.random.default_rng(28)
    size = WG + 5000
    first = rng.choice(np.frombuffer(b"a7", dtype=np.uint8), size)
    second = rng.choice(np.frombuffer(b"a7:", dtype=np.uint8), size)
    pat = make(ss, r"a[0-9]a")
    arena = Arena(first)
    dev, _ = arena.view(9, size - 9)
    wants = [rule_offsets(h[9:], pat.sets).size for h in (first, second)]
    assert wants[0] != wants[1]
    w = Window(1)
    assert pat.count_async(dev, w.view) is w.view                  # (first use outside the capture)
    torch.cuda.synchronize()
    w.check([wants[0]], "before the capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # one stream, no parallel branches
        pat.count_async(dev, w.view)
    for content, want in ((first, wants[0]), (second, wants[1]), (first, wants[0])):
        arena.buf[arena.at:arena.at + size].copy_(torch.from_numpy(content.copy()))
        w.view.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        w.check([want], "replayed")
    assert int(pat.count_async(dev).cpu()[0]) == wants[0]
    # the waiting calls refuse a capturing stream and write nothing
    g2 = torch.cuda.CUDAGraph()
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    errs, o = [], Window(4)
    with torch.cuda.graph(g2):
        probe.fill_(7)
        for call in (lambda: pat.count(dev), lambda: pat.find_all_into(dev, o.view, 4), lambda: pat.count_lines(dev),
                     lambda: pat.find_lines_into(dev, o.view, None, None, 4)):
            try:
                call()
            except ss.SlicesliceError as x:
                errs.append(x)
    torch.cuda.synchronize()
    assert len(errs) == 4 and all(e.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(e) for e in errs), errs
    o.check([], "refused while capturing")
    assert pat.count(dev) == wants[0]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_argument_error_and_write_nothing(ss):
    import ctypes
    with mk_lib(ss):
        L = ss.lib()
        pat = ss.ClassPattern(r"a[0-9]")
        one = sets_of(np.ones((2, 256), dtype=bool))
        dev = torch.full((64,), ord("a"), dtype=torch.uint8, device="cuda")
        o = Window(4)
        out = ctypes.c_uint64(77)
        h = ctypes.c_void_p(1234)
        empty = np.zeros((2, 4), dtype=np.uint64)
        empty[0, 0] = 1
        long = sets_of(np.ones((4097, 256), dtype=bool))
        many = sets_of(np.tile(members(ss.parse_classes(r"[0-9]"))[0], (1025, 1)))
        calls = [
            lambda: L.ss_classes_new(None, 2, ctypes.byref(h)),
            lambda: L.ss_classes_new(one.ctypes.data, 2, None),
            lambda: L.ss_classes_new(one.ctypes.data, 0, ctypes.byref(h)),
            lambda: L.ss_classes_new(long.ctypes.data, 4097, ctypes.byref(h)),
            lambda: L.ss_classes_new(empty.ctypes.data, 2, ctypes.byref(h)),
            lambda: L.ss_classes_new(many.ctypes.data, 1025, ctypes.byref(h)),
            lambda: L.ss_classes_info(None, -1, ctypes.byref(out)),
            lambda: L.ss_classes_info(pat._h, -1, None),
            lambda: L.ss_classes_info(pat._h, 256, ctypes.byref(out)),
            lambda: L.ss_classes_cover(None, 2, None, None),
            lambda: L.ss_count_classes_device(None, dev.data_ptr(), 64, None, ctypes.byref(out)),
            lambda: L.ss_count_classes_device(pat._h, dev.data_ptr(), 64, None, None),
            lambda: L.ss_count_classes_device(pat._h, None, 64, None, ctypes.byref(out)),
            lambda: L.ss_count_classes_device_async(pat._h, dev.data_ptr(), 64, None, None),
            lambda: L.ss_count_classes_device_async(None, dev.data_ptr(), 64, None, o.view.data_ptr()),
            lambda: L.ss_find_all_classes_device(None, dev.data_ptr(), 64, None, o.view.data_ptr(), 4, ctypes.byref(out)),
            lambda: L.ss_find_all_classes_device(pat._h, dev.data_ptr(), 64, None, o.view.data_ptr(), 4, None),
            lambda: L.ss_find_all_classes_device(pat._h, dev.data_ptr(), 64, None, None, 4, ctypes.byref(out)),
            lambda: L.ss_count_lines_classes_device(None, dev.data_ptr(), 64, 10, None, ctypes.byref(out)),
            lambda: L.ss_count_lines_classes_device(pat._h, dev.data_ptr(), 64, 10, None, None),
            lambda: L.ss_count_lines_classes_device(pat._h, dev.data_ptr(), 64, 256, None, ctypes.byref(out)),
            lambda: L.ss_count_lines_classes_device(pat._h, dev.data_ptr(), 64, -1, None, ctypes.byref(out)),
            lambda: L.ss_find_lines_classes_device(None, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, ctypes.byref(out)),
            lambda: L.ss_find_lines_classes_device(pat._h, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, None),
        ]
        for k, call in enumerate(calls):
            assert call() == ss.SS_ERR_ARGUMENT and L.ss_last_error(), k
        torch.cuda.synchronize()
        assert out.value == 77 and h.value == 1234
        o.check([], "refused")
        L.ss_classes_free(None)                                     # (NULL is allowed)
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                other = torch.zeros(64, dtype=torch.uint8, device="cuda:1")
                assert L.ss_count_classes_device(pat._h, other.data_ptr(), 64, None, ctypes.byref(out)) == ss.SS_ERR_ARGUMENT
                assert b"device" in L.ss_last_error()
        assert pat.count(dev) == 0 and ss.ClassPattern(r"[a-c]a").count(dev) == 63 and ss.ClassPattern.from_sets(long[:4096]).info()["n"] == 4096


def test_a_pattern_made_on_the_product_build_is_refused_by_name(ss):
    import sys
    product = ss.searcher._load(sys.modules["sliceslice_rs_amd._build"].build())
    assert not product.has_classes
    saved, ss.searcher._lib = ss.searcher._lib, product
    try:
        for call in (lambda: ss.ClassPattern(r"[0-9]{3}"), lambda: ss.ClassPattern.from_bytes(b"abc"), lambda: ss.parse_classes(r"\d")):
            with pytest.raises(ss.SlicesliceError, match=r"ss\.classes_build\(\)") as e:
                call()
            assert e.value.code == ss.SS_ERR_ARGUMENT and "libsliceslice_hip_classes.so" in str(e.value)
    finally:
        ss.searcher._lib = saved
    with mk_lib(ss):
        assert ss.ClassPattern(r"[0-9]{3}").info()["inexact"] == 3


# ---- tools/grep_hip.py --classes ----------------------------------------------------------------------------------------------------
def test_grep_hip_classes_prints_what_the_fixture_records(ss, manual):
    import subprocess
    import sys
    cases = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "classes_kat.json")))["cases"]}
    path = os.path.join(GOLDEN, "data", "i386.txt")

    def run(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True)

    case = cases["hex_word"]
    r = run("--classes", case["pattern"], "--offsets", path)
    assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == case["offsets"], r.stderr[-300:]
    with mk_lib(ss):
        sets = ss.parse_classes(case["pattern"])
    begin, end, number = rule_lines(np.frombuffer(manual, dtype=np.uint8), sets, 10)
    want = b"".join(b"%d:%s\n" % (n, manual[b:e]) for b, e, n in zip(begin.tolist(), end.tolist(), number.tolist()))
    r = run("--classes", case["pattern"], "--lines", "--device-output", path)
    assert r.returncode == 0 and r.stdout == want and len(number) == case["lines"], r.stderr[-300:]
    r = run("--classes", "[a-c]x", "-i", "--count", path)
    assert r.returncode == 0 and int(r.stdout) == cases["a_to_c_x_nocase"]["count"], r.stderr[-300:]
    r = run("--classes", "[0-9", "--count", path)                  # refused with the column, nothing printed
    assert r.returncode != 0 and r.stdout == b"" and b"column 1" in r.stderr, r.stderr[-300:]
    r = run("--classes", "a", "--count", "-w", path)
    assert r.returncode != 0 and r.stdout == b"" and b"--classes" in r.stderr
