"""GPU tests of the masked-pattern calls (include/sliceslice_hip_masked.h, libsliceslice_hip_masked.so) against THE RULE restated in
numpy (tests/test_masked_cpu.py: rule_offsets, rule_lines), against the searchers of the same build, and against
tests/golden/masked_kat.json (Python's re).  Every comparison is of integers and exact; every output array is a window of a larger
one whose sentinels on both sides must survive.  The geometry's units are lane 16 B, piece 1 KiB, wave 4 KiB, tile 16 KiB and
workgroup 128 KiB, so - the manual's text aside - no view is larger than 300,000 bytes (two workgroups and a tail); views of more than
one chunk of 256 workgroups are tests/test_gpu_set_grids.py's."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_masked_cpu import rule_lines, rule_offsets            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GUARD = 8
SENT64 = -0x5A5A5A5A5A5A5A5B
LANE, PIECE, WAVE, TILE, WG = 16, 1024, 4096, 16384, 131072
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 18, 33, 64, 257, 4096)
KINDS = ("ff", "00", "nibbles", "first", "middle", "last", "two1", "two15", "two16", "two17", "two40")


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def mk_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.masked_build()`."""
    return _loaded() if getattr(ss.lib(), "has_masked", False) else ss.masked_build()


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


class Window:
    """`cap` slots inside a larger device array filled with a sentinel"""
    def __init__(self, cap, dtype=torch.int64, sent=SENT64):
        self.sent = sent
        self.buf = torch.full((cap + 2 * GUARD,), sent, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + cap]

    def check(self, want, what):
        """the first len(want) slots hold `want`, every other slot of the larger array the sentinel"""
        h = self.buf.cpu().numpy()
        k = len(want)
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + k:] == self.sent).all(), what
        assert (h[GUARD:GUARD + k] == np.asarray(want, dtype=h.dtype)).all(), (what, h[GUARD:GUARD + min(k, 8)], list(want[:8]))


class Arena:
    """Host bytes on the device behind a 16-byte aligned address, so that any slice is a view of known misalignment whose
    neighbours are real bytes of the same text."""
    def __init__(self, host):
        self.host = np.frombuffer(bytes(host), dtype=np.uint8) if not isinstance(host, np.ndarray) else host
        self.buf = torch.empty(self.host.size + 16, dtype=torch.uint8, device="cuda")
        self.at = (-self.buf.data_ptr()) % 16
        self.buf[self.at:self.at + self.host.size].copy_(torch.from_numpy(self.host.copy()))

    def view(self, begin, length):
        v = self.buf[self.at + begin:self.at + begin + length]
        assert length == 0 or v.data_ptr() % 16 == begin % 16
        return v, self.host[begin:begin + length]


def make(ss, value, mask=None):
    with mk_lib(ss):
        return ss.MaskedPattern(value, mask)


def pattern_of(kind, n, letters, rng):
    """(value, mask) of one of KINDS for n bytes, or None where the kind needs a longer pattern"""
    value = bytes(int(x) for x in rng.choice(np.frombuffer(letters, dtype=np.uint8), n))
    mask = bytearray(n)
    if kind == "ff":
        mask = bytearray(b"\xff" * n)
    elif kind == "nibbles":
        mask = bytearray((0xF0, 0x0F)[i & 1] for i in range(n))
    elif kind in ("first", "middle", "last"):
        mask[{"first": 0, "middle": n // 2, "last": n - 1}[kind]] = 0xFF
    elif kind.startswith("two"):
        d = int(kind[3:])
        if n < d + 1:
            return None
        s = (n - 1 - d) // 2
        mask[s] = mask[s + d] = 0xFF
    return value, bytes(mask)


def plant(host, value, mask, at, rng):
    """a copy of the pattern at `at`: value where the mask has bits, the text's own bits elsewhere"""
    n = len(value)
    v, m = np.frombuffer(value, dtype=np.uint8), np.frombuffer(mask, dtype=np.uint8)
    host[at:at + n] = (v & m) | (host[at:at + n] & ~m)


def check_occurrences(pat, dev, host, value, mask, what):
    want = rule_offsets(host, value, mask)
    assert pat.count(dev) == want.size, (what, "count")
    w = Window(want.size + 2)
    assert pat.find_all_into(dev, w.view, want.size + 2) == want.size, (what, "find_all total")
    w.check(want, (what, "find_all"))
    return want


def check_lines(pat, dev, host, value, mask, delimiter, what):
    begin, end, number = rule_lines(host, value, mask, delimiter)
    assert pat.count_lines(dev, bytes([delimiter])) == begin.size, (what, "count_lines")
    wb, we, wn = Window(begin.size + 2), Window(begin.size + 2), Window(begin.size + 2)
    assert pat.find_lines_into(dev, wb.view, we.view, wn.view, begin.size + 2, bytes([delimiter])) == begin.size, (what, "find_lines total")
    wb.check(begin, (what, "begin"))
    we.check(end, (what, "end"))
    wn.check(number, (what, "number"))


def haystack(kind, size, rng):
    if kind == "random":
        return rng.integers(0, 256, size, dtype=np.uint8)
    if kind == "two_letter":
        return rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size)
    runs = np.repeat(rng.choice(np.frombuffer(b"ab\n", dtype=np.uint8), size // 7 + 1), rng.integers(1, 14, size // 7 + 1))
    return np.ascontiguousarray(np.resize(runs, size))


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hay_kind", ["random", "two_letter", "runs"])
def test_the_rule_over_lengths_masks_misalignments_and_view_lengths(ss, hay_kind):
    rng = np.random.default_rng(11)
    full = TILE + 3000 + 13                                        # two tiles of one workgroup, an odd tail
    letters = bytes(range(256)) if hay_kind == "random" else b"ab"
    for n in LENGTHS:
        for kind in KINDS:
            pm = pattern_of(kind, n, letters, rng)
            if pm is None:
                continue
            value, mask = pm
            host = haystack(hay_kind, full + 64, rng).copy()
            # copies at the view's ends for every misalignment, across the tile border and overlapping one another
            for at in (0, 1, 15, 16, full - n, full - n + 1, full - n + 15, TILE - n // 2, TILE - n // 2 + 1, 5000, 5001 + n // 2):
                if 0 <= at and at + n <= host.size:
                    plant(host, value, mask, at, rng)
            arena = Arena(host)
            pat = make(ss, value, mask)
            assert pat.info()["n"] == n
            for mis in (0, 1, 15):
                for length in (0, n - 1, n, n + 1, full):
                    dev, hv = arena.view(mis, length)
                    want = check_occurrences(pat, dev, hv, pat.value, pat.mask, (hay_kind, n, kind, mis, length))
                    if kind == "00":
                        assert want.size == max(0, length - n + 1)
                    if length == full:
                        assert want.size >= 3
                        if n <= 64:
                            check_lines(pat, dev, hv, pat.value, pat.mask, 10, (hay_kind, n, kind, mis, length, "lines"))


# ---- borders -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "anchor", "second", "last"])
def test_key_bytes_on_both_sides_of_every_border(ss, which):
    rng = np.random.default_rng(12)
    size = 2 * WG + 37000
    n = 40
    for value, mask in ((bytes(rng.integers(1, 256, n, dtype=np.uint8)), bytes(0xFF if i in (0, 23, 39) else 0x00 for i in range(n))),
                        (bytes(rng.integers(1, 256, n, dtype=np.uint8)), None)):
        pat = make(ss, value, mask)
        info = pat.info()
        key = {"first": 0, "anchor": info["anchor"], "second": info["anchor"] + info["distance"], "last": n - 1}[which]
        if mask is not None:
            assert (info["anchor"], info["distance"]) == (23, 16)  # (the only two fixed bytes within 16 of one another)
        for mis in (0, 5):
            host = np.zeros(size + 16, dtype=np.uint8)              # (no pattern byte is zero: the background cannot match a fixed byte)
            planted = []
            for unit, lo, hi in ((LANE, 50, 100), (PIECE, 3, 5), (WAVE, 2, 3), (TILE, 1, 3), (WG, 1, 2)):
                for multiple, side in ((lo, -1), (hi, 0)):
                    # the arena's index is the stream position: the key byte goes to unit * multiple + side
                    p = unit * multiple + side - key
                    plant(host, pat.value, pat.mask, p, rng)
                    planted.append(p - mis)
            arena = Arena(host)
            dev, hv = arena.view(mis, size)
            want = check_occurrences(pat, dev, hv, pat.value, pat.mask, (which, mis))
            assert set(planted) <= set(want.tolist()) and len(planted) >= 9
            check_lines(pat, dev, hv, pat.value, pat.mask, 10, (which, mis, "lines"))


# ---- near misses ---------------------------------------------------------------------------------------------------------------------
def test_one_flipped_bit_inside_the_mask_fails_and_one_outside_it_matches(ss):
    rng = np.random.default_rng(13)
    for n in (1, 2, 5, 17, 40):
        value = bytes(rng.integers(1, 256, n, dtype=np.uint8))
        mask = bytes(int(rng.choice([0xFF, 0xF0, 0x0F, 0xDF, 0x81, 0x00])) if n > 1 else 0xF0 for _ in range(n))
        if not any(mask):
            mask = b"\xff" + mask[1:]
        pat = make(ss, value, mask)
        gap = 64
        host = np.full((2 * n + 2) * gap + 7, 0, dtype=np.uint8)
        # a background byte that fails the first position with a mask, so that only the copies can match
        k0 = next(i for i in range(n) if pat.mask[i])
        host[:] = (pat.value[k0] ^ (pat.mask[k0] & -pat.mask[k0])) & 0xFF
        must, must_not = [], []
        for i in range(n):
            m = pat.mask[i]
            for inside in (True, False):
                bits = m if inside else (~m & 0xFF)
                if bits == 0:
                    continue
                at = (2 * i + (0 if inside else 1) + 1) * gap + 3
                copy = bytearray(pat.value)
                copy[i] ^= bits & -bits                             # the lowest such bit
                host[at:at + n] = np.frombuffer(bytes(copy), dtype=np.uint8)
                (must_not if inside else must).append(at)
        dev, hv = Arena(host).view(3, host.size - 3)
        want = check_occurrences(pat, dev, hv, pat.value, pat.mask, ("near miss", n))
        got = set(want.tolist())
        assert {p - 3 for p in must} <= got and not ({p - 3 for p in must_not} & got), n


# ---- the ends of the view ------------------------------------------------------------------------------------------------------------
def test_copies_outside_the_view_or_cut_by_its_ends_never_count(ss):
    rng = np.random.default_rng(14)
    for n in (2, 16, 33, 257):
        value = bytes(rng.integers(1, 256, n, dtype=np.uint8))
        for mask in (None, bytes(0xFF if i in (0, n - 1) else 0 for i in range(n)), bytes(0xFF if i == n // 2 else 0x0F for i in range(n))):
            pat = make(ss, value, mask)
            for mis in (0, 1, 15):
                for length in (n + 40, WAVE + 5):
                    lo = (n + 31) // 16 * 16 + mis                  # the view's first byte at misalignment `mis`
                    hi = lo + length
                    host = np.zeros(hi + n + 16, dtype=np.uint8)
                    host[lo - n:lo] = np.frombuffer(pat.value, dtype=np.uint8)              # just before
                    host[hi:hi + n] = np.frombuffer(pat.value, dtype=np.uint8)              # just behind
                    cut = n - 1
                    if cut and length >= 2 * cut + 8:
                        host[lo:lo + cut] = np.frombuffer(pat.value, dtype=np.uint8)[1:]    # cut by the first end
                        host[hi - cut:hi] = np.frombuffer(pat.value, dtype=np.uint8)[:cut]  # cut by the last end
                    dev, hv = Arena(host).view(lo, length)
                    assert dev.data_ptr() % 16 == mis
                    want = check_occurrences(pat, dev, hv, pat.value, pat.mask, ("ends", n, mis, length))
                    if mask is None:
                        assert want.size == 0 and pat.count_lines(dev) == 0
                    # ... and a whole copy inside, touching either end, counts
                    for at in (lo, hi - n):
                        host[at:at + n] = np.frombuffer(pat.value, dtype=np.uint8)
                        dev, hv = Arena(host).view(lo, length)
                        want = check_occurrences(pat, dev, hv, pat.value, pat.mask, ("ends, inside", n, mis, length, at))
                        assert at - lo in want.tolist()


# ---- capacity ------------------------------------------------------------------------------------------------------------------------
def test_capacities_and_a_capacity_reached_in_the_first_workgroup(ss):
    rng = np.random.default_rng(15)
    size = 2 * WG + 30000
    value, mask = b"q\x00z", b"\xff\x00\xff"
    host = rng.choice(np.frombuffer(b"abc", dtype=np.uint8), size + 16)
    spots = [5, 100, 101, 4000, TILE - 1, WG - 2, WG + 7, 2 * WG + 1, 2 * WG + 20000, size - 3]
    for p in spots:
        plant(host, value, mask, p, rng)
    pat = make(ss, value, mask)
    dev, hv = Arena(host).view(0, size)
    want = rule_offsets(hv, value, mask)
    total = want.size
    assert want.tolist() == spots and pat.count(dev) == total
    assert pat.find_all_into(dev, None, 0) == total
    for cap in (1, 4, total - 1, total, total + 1):                # (4: reached inside the first workgroup, occurrences in the third)
        w = Window(total + 4)
        assert pat.find_all_into(dev, w.view, cap) == total, cap
        w.check(want[:cap], ("capacity", cap))                      # nothing at index `cap` or beyond
    assert pat.find_all(dev).cpu().tolist() == spots and pat.find_all(dev, capacity=3).cpu().tolist() == spots[:3]
    # the line calls under the same capacities
    host[[50, 3000, WG + 100, 2 * WG + 10]] = 10
    dev, hv = Arena(host).view(0, size)
    begin, end, number = rule_lines(hv, value, mask, 10)
    assert begin.size == 5
    for cap in (1, 2, 4, 5, 6):
        wb, we, wn = Window(8), Window(8), Window(8)
        assert pat.find_lines_into(dev, wb.view, we.view, wn.view, cap) == 5
        wb.check(begin[:cap], ("line capacity", cap))
        we.check(end[:cap], ("line capacity", cap))
        wn.check(number[:cap], ("line capacity", cap))
    assert pat.find_lines_into(dev, None, None, None, 0) == 5
    assert [x.cpu().tolist() for x in pat.find_lines(dev)] == [begin.tolist(), end.tolist(), number.tolist()]


# ---- relations -----------------------------------------------------------------------------------------------------------------------
def test_patterns_without_wildcards_equal_the_searchers_of_the_same_build(ss, manual, d_manual):
    with mk_lib(ss):
        for word in (b"descriptor", b"the", b"e", b"  ", b"segment register", b"no such phrase in the manual"):
            s, pat = ss.DynamicHipSearcher.new(word), ss.MaskedPattern(word)
            assert pat.count(d_manual) == s.count(d_manual) == len(pat.find_all(d_manual)), word
            assert torch.equal(pat.find_all(d_manual), s.find_all(d_manual)), word
            assert pat.count_lines(d_manual) == s.count_lines(d_manual), word
            for got, want in zip(pat.find_lines(d_manual), s.find_lines(d_manual)):
                assert torch.equal(got, want), word
        for word in (b"intel", b"Segment", b"80386", b"gdt", b"x"):
            # (the folding searcher takes its needle without upper-case letters)
            s, pat = ss.DynamicHipSearcher.new(word.lower()), ss.MaskedPattern.from_bytes(word, ignore_case=True)
            assert pat.count(d_manual) == s.count(d_manual, ignore_case=True), word
        # one more fixed byte finds a subset
        wide, narrow = ss.MaskedPattern.from_hex("74 ?? 65"), ss.MaskedPattern.from_hex("74 68 65")
        a, b = set(wide.find_all(d_manual).cpu().tolist()), set(narrow.find_all(d_manual).cpu().tolist())
        assert b < a and len(b) == 7398 and len(a) == wide.count(d_manual)


# ---- lines ---------------------------------------------------------------------------------------------------------------------------
def test_lines_under_three_delimiters_dense_sparse_and_across_workgroups(ss):
    rng = np.random.default_rng(16)
    with mk_lib(ss):
        wild = ss.MaskedPattern.from_hex("61 ?? 62")
        for text, lines in ((b"a\nb", 0), (b"a\nb\n", 0), (b"axb", 1), (b"\naxb", 1), (b"axb\n", 1), (b"a\nbaxb", 1), (b"", 0), (b"\n\n\n", 0)):
            dev, hv = Arena(np.frombuffer(text, dtype=np.uint8)).view(0, len(text))
            assert wild.count_lines(dev) == lines, text
            check_lines(wild, dev, hv, wild.value, wild.mask, 10, text)
        assert wild.info(b"\n")["accepts_delimiter"] == 1 and wild.info(b"a")["accepts_delimiter"] == 1 and wild.info(b"c")["accepts_delimiter"] == 1
        assert ss.MaskedPattern(b"ab").info(b"\n")["accepts_delimiter"] == 0
        patterns = [wild, ss.MaskedPattern.from_hex("??"), ss.MaskedPattern.from_hex("?? ?? ??"), ss.MaskedPattern.from_hex("61 61"),
                    ss.MaskedPattern.from_hex("6? 0? 6?"), ss.MaskedPattern(b"b" * 17, b"\xff" + b"\x00" * 15 + b"\xff")]
        size = WG + 9000
        for delimiter in (10, 0, ord("a")):
            dense = rng.choice(np.frombuffer(bytes([delimiter, ord("a"), ord("b")]), dtype=np.uint8), size + 16)
            free = rng.choice(np.frombuffer(b"bcd" if delimiter == ord("a") else b"abc", dtype=np.uint8), size + 16)
            for name, host in (("dense", dense), ("free", free)):
                arena = Arena(host)
                for mis, length in ((0, size), (7, size - 100), (15, TILE + 1)):
                    dev, hv = arena.view(mis, length)
                    for k, pat in enumerate(patterns):
                        check_lines(pat, dev, hv, pat.value, pat.mask, delimiter, (name, delimiter, mis, length, k))
        # an occurrence in the first workgroup whose line is closed in the second, and one whose line never closes
        host = np.full(2 * WG + 500, ord("c"), dtype=np.uint8)
        host[WG - 30:WG - 27] = np.frombuffer(b"axb", dtype=np.uint8)
        host[100] = host[WG + 4000] = 10
        host[2 * WG + 100:2 * WG + 103] = np.frombuffer(b"a\nb", dtype=np.uint8)
        host[2 * WG + 300:2 * WG + 303] = np.frombuffer(b"ayb", dtype=np.uint8)
        dev, hv = Arena(host).view(0, host.size)
        begin, end, number = rule_lines(hv, wild.value, wild.mask, 10)
        assert begin.tolist() == [101, 2 * WG + 102] and end.tolist() == [WG + 4000, host.size] and number.tolist() == [2, 4]
        check_lines(wild, dev, hv, wild.value, wild.mask, 10, "across workgroups")


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_every_case_of_the_fixture_on_the_manual(ss, manual, d_manual):
    kat = json.load(open(os.path.join(GOLDEN, "masked_kat.json")))
    assert kat["bytes"] == len(manual)
    for c in kat["cases"]:
        pat = make(ss, bytes.fromhex(c["value"]), bytes.fromhex(c["mask"]))
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
    with mk_lib(ss):
        assert ss.MaskedPattern.from_hex("64 ?? 73 63 72 ?? ?? 74 6f 72").count(d_manual) == 355


# ---- the async form in a graph ------------------------------------------------------------------------------------------------------
def test_the_async_count_is_captured_and_replayed_on_two_contents(ss):
    rng = np.random.default_rng(17)
    size = WG + 5000
    value, mask = b"a\x00b", b"\xff\x00\xff"
    first = rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size)
    second = rng.choice(np.frombuffer(b"abc", dtype=np.uint8), size)
    wants = [rule_offsets(h, value, mask).size for h in (first, second)]
    assert wants[0] != wants[1]
    pat = make(ss, value, mask)
    arena = Arena(first)
    dev, _ = arena.view(9, size - 9)
    wants = [rule_offsets(h[9:], value, mask).size for h in (first, second)]
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
        pat = ss.MaskedPattern(b"ab")
        for make_it in (lambda: ss.MaskedPattern(b""), lambda: ss.MaskedPattern(b"x" * 4097), lambda: ss.MaskedPattern(b"x" * 5000, b"\0" * 5000)):
            with pytest.raises(ss.SlicesliceError) as e:
                make_it()
            assert e.value.code == ss.SS_ERR_ARGUMENT
        assert ss.MaskedPattern(b"x" * 4096).info()["n"] == 4096
        with pytest.raises(ValueError):
            ss.MaskedPattern(b"abc", b"\xff")
        dev = torch.full((64,), ord("a"), dtype=torch.uint8, device="cuda")
        o = Window(4)
        out = ctypes.c_uint64(77)
        h = ctypes.c_void_p(1234)
        calls = [
            lambda: L.ss_masked_new(None, None, 2, ctypes.byref(h)),
            lambda: L.ss_masked_new(b"ab", None, 2, None),
            lambda: L.ss_masked_new(b"ab", None, 0, ctypes.byref(h)),
            lambda: L.ss_masked_new(b"ab", None, 4097, ctypes.byref(h)),
            lambda: L.ss_masked_info(None, -1, ctypes.byref(out)),
            lambda: L.ss_masked_info(pat._h, -1, None),
            lambda: L.ss_count_masked_device(None, dev.data_ptr(), 64, None, ctypes.byref(out)),
            lambda: L.ss_count_masked_device(pat._h, dev.data_ptr(), 64, None, None),
            lambda: L.ss_count_masked_device(pat._h, None, 64, None, ctypes.byref(out)),
            lambda: L.ss_count_masked_device_async(pat._h, dev.data_ptr(), 64, None, None),
            lambda: L.ss_count_masked_device_async(None, dev.data_ptr(), 64, None, o.view.data_ptr()),
            lambda: L.ss_find_all_masked_device(None, dev.data_ptr(), 64, None, o.view.data_ptr(), 4, ctypes.byref(out)),
            lambda: L.ss_find_all_masked_device(pat._h, dev.data_ptr(), 64, None, o.view.data_ptr(), 4, None),
            lambda: L.ss_find_all_masked_device(pat._h, dev.data_ptr(), 64, None, None, 4, ctypes.byref(out)),
            lambda: L.ss_count_lines_masked_device(None, dev.data_ptr(), 64, 10, None, ctypes.byref(out)),
            lambda: L.ss_count_lines_masked_device(pat._h, dev.data_ptr(), 64, 10, None, None),
            lambda: L.ss_count_lines_masked_device(pat._h, dev.data_ptr(), 64, 256, None, ctypes.byref(out)),
            lambda: L.ss_count_lines_masked_device(pat._h, dev.data_ptr(), 64, -1, None, ctypes.byref(out)),
            lambda: L.ss_find_lines_masked_device(None, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, ctypes.byref(out)),
            lambda: L.ss_find_lines_masked_device(pat._h, dev.data_ptr(), 64, 10, None, o.view.data_ptr(), None, None, 4, None),
        ]
        for k, call in enumerate(calls):
            assert call() == ss.SS_ERR_ARGUMENT and L.ss_last_error(), k
        torch.cuda.synchronize()
        assert out.value == 77 and h.value == 1234
        o.check([], "refused")
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                other = torch.zeros(64, dtype=torch.uint8, device="cuda:1")
                assert L.ss_count_masked_device(pat._h, other.data_ptr(), 64, None, ctypes.byref(out)) == ss.SS_ERR_ARGUMENT
                assert b"device" in L.ss_last_error()
        assert pat.count(dev) == 0 and ss.MaskedPattern(b"aa").count(dev) == 63


# ---- tools/grep_hip.py --hex --------------------------------------------------------------------------------------------------------
def test_grep_hip_hex_prints_what_the_fixture_records(ss, manual):
    import subprocess
    import sys
    case = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "masked_kat.json")))["cases"]}["descriptor_gaps"]
    value, mask = bytes.fromhex(case["value"]), bytes.fromhex(case["mask"])
    path = os.path.join(GOLDEN, "data", "i386.txt")

    def run(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True)

    r = run("--hex", "64 ?? 73 63 72 ?? ?? 74 6f 72", "--offsets", path)
    assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == case["offsets"], r.stderr[-300:]
    begin, end, number = rule_lines(np.frombuffer(manual, dtype=np.uint8), value, mask, 10)
    want = b"".join(b"%d:%s\n" % (n, manual[b:e]) for b, e, n in zip(begin.tolist(), end.tolist(), number.tolist()))
    r = run("--hex", "64??7363 72????746f72", "--lines", "--device-output", path)
    assert r.returncode == 0 and r.stdout == want and len(number) == case["lines"], r.stderr[-300:]
    r = run("--hex", "64 ?? 7", "--count", path)                   # refused with the column, nothing printed
    assert r.returncode != 0 and r.stdout == b"" and b"column 8" in r.stderr, r.stderr[-300:]
    r = run("--hex", "64 ??", "--count", "-i", path)
    assert r.returncode != 0 and r.stdout == b"" and b"--hex" in r.stderr
