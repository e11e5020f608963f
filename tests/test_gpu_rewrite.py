"""GPU tests of the rewrite call (include/sliceslice_hip_rewrite.h, libsliceslice_hip_rewrite.so) against THE RULE restated in numpy
(tests/test_rewrite_cpu.py: rule_replace, which that file checks against re.sub), against calls of the same build that exist, and
against tests/golden/rewrite_kat.json (Python's re).  Every comparison is of bytes and integers and exact; every output is a window
of a larger buffer whose sentinels on both sides must survive.  The geometry's units are lane 16 B, piece 1 KiB, wave 4 KiB, tile
16 KiB and workgroup 128 KiB, so - the manual's text aside - no view is larger than 300 KiB (two workgroups and a tail)."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_classes_cpu import members, re_set, sets_of                                  # noqa: E402
from test_gpu_masked import LANE, PIECE, TILE, WAVE, WG, Arena                          # noqa: E402
from test_gpu_runs import BOUNDS, FULL, WORD, haystack                                  # noqa: E402
from test_rewrite_cpu import G, rule_replace                                            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GUARD, SENT = 64, 0xA5
VIEW = 300 << 10
TEXTS = (b"", b"#", b"<q_>")            # (the last one consists of members and non-members of \w: a replacement is not rescanned)


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def mk_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry point, else `ss.rewrite_build()`."""
    return _loaded() if getattr(ss.lib(), "has_rewrite", False) else ss.rewrite_build()


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


def make(ss, words, lo=1, hi=None, bitmap=False):
    with mk_lib(ss):
        return ss.RunPattern.from_set(words, lo, hi, bitmap)


class ByteWindow:
    """`cap` bytes at misalignment `mis` inside a larger device buffer filled with a sentinel"""
    def __init__(self, cap, mis=0):
        self.buf = torch.full((cap + 2 * GUARD + 16,), SENT, dtype=torch.uint8, device="cuda")
        self.at = GUARD + (mis - self.buf.data_ptr() - GUARD) % 16
        self.view = self.buf[self.at:self.at + cap]
        assert cap == 0 or self.view.data_ptr() % 16 == mis

    def check(self, want, what):
        """the first len(want) bytes are `want`, every other byte of the larger buffer the sentinel"""
        h = self.buf.cpu().numpy()
        k = len(want)
        assert (h[:self.at] == SENT).all() and (h[self.at + k:] == SENT).all(), (what, "sentinels")
        assert h[self.at:self.at + k].tobytes() == bytes(want), (what, "bytes")


def check(pat, dev, host, text, delimiter=None, omis=0, what=None):
    """one call into a window of exactly the output's size, against the rule"""
    want, count = rule_replace(host, pat.set, text, pat.min_len, pat.max_len, delimiter)
    w = ByteWindow(len(want), omis)
    assert pat.replace_into(dev, text, w.view if len(want) else None, delimiter) == (len(want), count), (what, "out_len, count")
    w.check(want, what)
    return want, count


# ---- units ---------------------------------------------------------------------------------------------------------------------------
def planted(unit):
    """host buffers of VIEW bytes of '-' with runs of 'q' that end on, begin on and straddle borders of `unit`, of every length"""
    spacing = {LANE: 16 * 513, PIECE: 9 * PIECE, WAVE: 3 * WAVE, TILE: TILE, WG: WG}[unit]
    borders = [b for b in range(spacing, VIEW - 4200, spacing) if b >= 4200]
    plants = [(length, how) for length in (1, 15, 16, 17, 33, 4096) for how in ("ends", "begins", "straddles")]
    hosts = []
    for k in range(0, len(plants), len(borders)):
        host = np.full(VIEW, ord("-"), dtype=np.uint8)
        for border, (length, how) in zip(borders, plants[k:k + len(borders)]):
            begin = {"ends": border - length, "begins": border, "straddles": border - (length + 1) // 2}[how]
            host[begin:begin + length] = ord("q")
        hosts.append(host)
    assert sum(min(len(borders), len(plants) - k) for k in range(0, len(plants), len(borders))) == 18
    return hosts


@pytest.mark.parametrize("unit", [LANE, PIECE, WAVE, TILE, WG])
def test_runs_that_end_begin_and_straddle_at_every_unit_border(ss, unit):
    pats = [make(ss, WORD, lo, hi, bitmap) for lo, hi in BOUNDS for bitmap in (False, True)]
    assert {p.info()["path"] for p in pats} == {0, 1}
    for host in planted(unit):
        arena = Arena(host)
        for mis in ((0, 5) if unit != WG else (5,)):
            # the arena's offsets are the geometry's: it starts at the 16-byte aligned address below the view
            dev, view = arena.view(mis, VIEW - 16)
            for k, pat in enumerate(pats):
                _, count = check(pat, dev, view, TEXTS[k % 3], None, (3 * k) % 16, (unit, mis, pat.min_len, pat.max_len, k & 1))
                assert count <= 18
    # ... and the same borders in text that is half members, one bound per path
    rng = np.random.default_rng(unit)
    arena = Arena(haystack(WORD, 0.5, 2 * unit + 33 if unit != WG else VIEW, rng))
    for length in (unit - 1, unit, unit + 1, min(2 * unit + 17, VIEW - 16)):
        dev, view = arena.view(3, length)
        for pat in (pats[2], pats[7]):                              # {2,} on the range path, {3} on the bitmap
            check(pat, dev, view, b"=", None, 9, (unit, length))


# ---- open workgroups -----------------------------------------------------------------------------------------------------------------
def test_a_run_that_covers_a_workgroup_and_more(ss):
    letters = sets_of(re_set(r"[a-z]"))[0]
    selected, too_long = make(ss, letters, 2, None), make(ss, letters, 2, 4096)
    for layout in ("covers", "closes_and_opens"):
        host = np.frombuffer(b"x-" * (VIEW // 2), dtype=np.uint8).copy()          # short runs of one byte everywhere else
        if layout == "covers":                                                      # begins in the first workgroup, ends in the third
            host[10000:10000 + (260 << 10)] = ord("m")
            assert 10000 < WG and 10000 + (260 << 10) > 2 * WG
        else:                                                                       # closes on a workgroup's last byte, opens on a first
            host[5000:WG] = ord("m")
            host[WG] = ord("-")
            host[2 * WG - 1] = ord("-")
            host[2 * WG:2 * WG + 5000] = ord("m")
        arena = Arena(host)
        for mis in (0, 7):
            dev, view = arena.view(mis, VIEW - 16)
            for text in (b"", b"Q", b"m" * 40):
                want, count = check(selected, dev, view, text, None, 5, (layout, mis, len(text)))
                assert count == (1 if layout == "covers" else 2)
                want, count = check(too_long, dev, view, text, None, 11, (layout, mis, len(text), "too long"))
                assert count == 0 and want == view.tobytes()                        # the output equals the input


# ---- placement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.05])
def test_every_haystack_and_output_misalignment_on_both_store_paths(ss, p):
    rng = np.random.default_rng(41)
    size = 5 * 1024
    host = haystack(WORD, p, size + 32, rng)
    host[2048:2048 + 160] = ord("-")                                    # ten lanes that keep all 16 bytes, whatever p is
    arena = Arena(host)
    pat = make(ss, WORD, 2, None)
    table = members(WORD.reshape(1, 4))[0]
    for hmis in range(16):
        dev, view = arena.view(hmis, size)
        # by construction of the input some lane (16 aligned bytes of the arena) keeps everything and some lane is mixed
        lanes = table[host[16:16 + size - 16]].reshape(-1, 16)
        assert (~lanes).all(axis=1).any() and (lanes.any(axis=1) & ~lanes.all(axis=1)).any()
        want, count = rule_replace(view, WORD, b"=", 2, None)
        assert 0 < count and len(want) < size
        for omis in range(16):
            w = ByteWindow(len(want), omis)
            assert pat.replace_into(dev, b"=", w.view) == (len(want), count), (p, hmis, omis)
            w.check(want, (p, hmis, omis))


# ---- texts ---------------------------------------------------------------------------------------------------------------------------
def test_texts_of_every_length_and_a_replacement_of_members_is_not_rescanned(ss):
    rng = np.random.default_rng(43)
    arena = Arena(haystack(WORD, 0.5, 5 * 1024 + 16, rng))
    dev, view = arena.view(3, 5 * 1024)
    for bitmap in (False, True):
        for lo in (1, 2):
            pat = make(ss, WORD, lo, None, bitmap)
            for n in (0, 1, 2, 15, 16, 17, 40):
                text = bytes(rng.choice(np.frombuffer(b"abcXYZ_09", dtype=np.uint8), n))     # members, every one
                want, count = check(pat, dev, view, text, None, n % 16, (bitmap, lo, n))
                assert count > 300
    # the longest text on alternating member / non-member: 2,048 runs and about 8 MiB of output
    text = bytes(rng.integers(0, 256, ss.SS_REWRITE_MAX_TEXT, dtype=np.uint8))
    arena = Arena(np.frombuffer(b"-a" * 2048 + b"-" * 16, dtype=np.uint8))
    dev, view = arena.view(1, 4096)
    want, count = check(make(ss, WORD), dev, view, text, None, 7, "4096")
    assert count == 2048 and len(want) == 2048 + 2048 * 4096
    with pytest.raises(ss.SlicesliceError, match="SS_REWRITE_MAX_TEXT"):
        make(ss, WORD).replace_into(dev, text + b"x", None)


# ---- delimiter -----------------------------------------------------------------------------------------------------------------------
def test_a_delimiter_is_never_a_member_and_is_always_copied(ss):
    rng = np.random.default_rng(47)
    words = sets_of(re_set(r"[\w\n\x00]"))[0]
    host = rng.choice(np.frombuffer(b"qqqqz_\n\x00-- ", dtype=np.uint8), 3 * TILE + 16)
    arena = Arena(host)
    dev, view = arena.view(9, 3 * TILE - 5)
    for lo, hi in ((1, None), (2, None), (3, 3), (2, 5)):
        for bitmap in (False, True):
            pat = make(ss, words, lo, hi, bitmap)
            for delimiter in (None, 10, 0, ord("q")):
                for text in (b"", b" ", b"\n_"):
                    want, count = check(pat, dev, view, text, delimiter, 2, (lo, hi, bitmap, delimiter, text))
                if delimiter is not None:
                    # the count of the pattern with that byte taken out of its set
                    less = words.copy()
                    less[delimiter >> 6] &= ~(np.uint64(1) << np.uint64(delimiter & 63))
                    assert count == make(ss, less, lo, hi, bitmap).count(dev) and pat.info(delimiter)["accepts_delimiter"] == 1
                    assert bytes(want).count(bytes([delimiter])) >= view.tobytes().count(bytes([delimiter]))
                else:
                    assert count == pat.count(dev)
    # a delimiter the set does not hold changes nothing, and keeps the range path's answer
    pat = make(ss, WORD, 2, None)
    assert check(pat, dev, view, b"+", ord("-"), 0, "no member") == check(pat, dev, view, b"+", None, 0, "none")
    only = sets_of(re_set(r"\n"))[0]
    for delimiter, ok in ((10, False), (None, True), (0, True)):
        if ok:
            check(make(ss, only), dev, view, b"$", delimiter, 0, "only")
        else:
            with pytest.raises(ss.SlicesliceError, match="only the delimiter") as e:
                make(ss, only).replace_into(dev, b"$", None, delimiter)
            assert e.value.code == ss.SS_ERR_ARGUMENT


# ---- capacity ------------------------------------------------------------------------------------------------------------------------
def test_capacities_sizing_and_the_corner_views(ss):
    rng = np.random.default_rng(53)
    arena = Arena(haystack(WORD, 0.5, WG + 4096 + 16, rng))
    dev, view = arena.view(5, WG + 4000)
    pat = make(ss, WORD, 2, None)
    for text in (b"", b"ab", b"0123456789abcdefXYZ"):
        want, count = rule_replace(view, WORD, text, 2, None)
        assert pat.replace_into(dev, text, None) == (len(want), count)                      # NULL / 0 sizes
        short = ByteWindow(len(want) - 1, 3)
        assert pat.replace_into(dev, text, short.view) == (len(want), count)                # short by one: nothing written, both reported
        short.check(b"", (text, "short by one"))
        exact = ByteWindow(len(want), 3)
        assert pat.replace_into(dev, text, exact.view) == (len(want), count)
        exact.check(want, (text, "exact"))
        roomy = ByteWindow(len(want) + 100, 3)
        assert pat.replace_into(dev, text, roomy.view) == (len(want), count)
        roomy.check(want, (text, "roomy"))
    w = ByteWindow(8)
    assert pat.replace_into(dev[:0], b"xyz", w.view) == (0, 0) and pat.replace_into(dev[:0], b"xyz", None) == (0, 0)     # len == 0
    w.check(b"", "empty view")
    assert pat.replace(dev[:0], b"xyz").numel() == 0 and pat.delete(dev[:0]).numel() == 0
    for length in (1, 15, 16, 17, 1024, WAVE + 1, WG + 17):
        none = Arena(np.full(length + 32, ord("-"), dtype=np.uint8)).view(3, length)
        want, count = check(pat, none[0], none[1], b"xyz", None, 1, ("no member", length))
        assert count == 0 and want == none[1].tobytes()                                     # no member: the input
        every = Arena(np.full(length + 32, ord("w"), dtype=np.uint8)).view(3, length)
        plus = make(ss, WORD)
        assert check(plus, every[0], every[1], b"xyz", None, 1, ("members only", length)) == (b"xyz", 1)
        assert plus.delete(every[0]).numel() == 0 and check(plus, every[0], every[1], b"", None, 1, ("deleted", length)) == (b"", 1)
    for bitmap in (False, True):                                                            # the full set: one run, the whole view
        assert check(make(ss, FULL, 1, None, bitmap), dev, view, b"!", None, 0, "full") == (b"!", 1)


# ---- relations -----------------------------------------------------------------------------------------------------------------------
def test_relations_to_count_find_all_the_old_route_and_between_the_python_paths(ss, manual):
    rng = np.random.default_rng(59)
    arena = Arena(haystack(WORD, 0.6, VIEW, rng))
    dev, view = arena.view(11, VIEW - 16)
    text_bytes = (b"", b"ab", b"<word>")
    with mk_lib(ss):
        for lo, hi in ((1, None), (3, None), (2, 5), (3, 3)):
            pat = make(ss, WORD, lo, hi)
            begin, end = pat.find_all(dev)
            for text in text_bytes:
                out_len, count = pat.replace_into(dev, text, None)
                assert count == pat.count(dev) == begin.numel()
                assert out_len == view.size - int((end - begin).sum()) + count * len(text)
                got = pat.replace(dev, text)
                # the old route: the complementary ranges, gathered with the text behind each, the last text trimmed
                kept_begin = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), end])
                kept_end = torch.cat([begin, torch.full((1,), view.size, dtype=torch.int64, device="cuda")])
                if len(text) == 1 or not text:
                    old = ss.gather_ranges(dev, kept_begin, kept_end, text or None)
                    old = old[:old.numel() - len(text)]
                    assert torch.equal(got, old), (lo, hi, text)
                assert got.cpu().numpy().tobytes() == rule_replace(view, WORD, text, lo, hi)[0], (lo, hi, text)
                # the single call (len(text) <= min_len) and the sizing path give the same tensor
                sized = torch.empty(out_len, dtype=torch.uint8, device="cuda")
                assert pat.replace_into(dev, text, sized) == (out_len, count) and torch.equal(got, sized), (lo, hi, text)
        blanks = ss.RunPattern(r" {2,}")
        d_manual = torch.from_numpy(np.frombuffer(manual, dtype=np.uint8).copy()).cuda()
        begin, end = blanks.find_all(d_manual)
        kept_begin = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), end])
        kept_end = torch.cat([begin, torch.full((1,), len(manual), dtype=torch.int64, device="cuda")])
        old = ss.gather_ranges(d_manual, kept_begin, kept_end, b" ")
        assert torch.equal(blanks.replace(d_manual, b" "), old[:old.numel() - 1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_results_and_the_output_alone(ss):
    rng = np.random.default_rng(61)
    arena = Arena(haystack(WORD, 0.5, 4096 + 16, rng))
    dev, view = arena.view(0, 4096)
    pat = make(ss, WORD)
    L = pat._L
    st = torch.cuda.current_stream().cuda_stream
    out_len, count = ctypes.c_uint64(77), ctypes.c_uint64(78)
    ol, c = ctypes.byref(out_len), ctypes.byref(count)
    w = ByteWindow(8192)
    text = ctypes.create_string_buffer(b"xy")
    for args, said in (((pat._h, None, 4096, -1, text, 2, st, None, 0, ol, c), "haystack is NULL"),
                       ((pat._h, dev.data_ptr(), 4096, -1, text, 2, st, None, 100, ol, c), "d_out is NULL"),
                       ((pat._h, dev.data_ptr(), 4096, -1, None, 2, st, w.view.data_ptr(), 8192, ol, c), "replacement is NULL"),
                       ((pat._h, dev.data_ptr(), 4096, 300, text, 2, st, w.view.data_ptr(), 8192, ol, c), "delimiter 300"),
                       ((pat._h, dev.data_ptr(), 4096, -1, text, 2, st, w.view.data_ptr(), 8192, None, c), "NULL"),
                       ((pat._h, dev.data_ptr(), 4096, -1, text, 2, st, w.view.data_ptr(), 8192, ol, None), "NULL"),
                       ((None, dev.data_ptr(), 4096, -1, text, 2, st, w.view.data_ptr(), 8192, ol, c), "runs is NULL"),
                       # d_out ranges that intersect the haystack's: its tail, its head, all of it
                       ((pat._h, dev.data_ptr(), 4096, -1, text, 2, st, dev.data_ptr() + 4095, 8192, ol, c), "intersects"),
                       ((pat._h, dev.data_ptr() + 2048, 2048, -1, text, 2, st, dev.data_ptr(), 2049, ol, c), "intersects"),
                       ((pat._h, dev.data_ptr(), 4096, -1, text, 2, st, dev.data_ptr(), 4096, ol, c), "intersects")):
        assert L.ss_replace_runs_device(*args) == ss.SS_ERR_ARGUMENT, said
        assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
        assert (out_len.value, count.value) == (77, 78), said
    # ... and ranges that only touch it are served
    assert L.ss_replace_runs_device(pat._h, dev.data_ptr() + 2048, 2048, -1, text, 0, st, dev.data_ptr(), 2048, ol, c) == ss.SS_OK
    arena = Arena(arena.host)
    dev, view = arena.view(0, 4096)
    out_len.value, count.value = 77, 78
    # a capturing stream
    graph = torch.cuda.CUDAGraph()
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    errs = []
    with torch.cuda.graph(graph):                                       # one stream, no parallel branches
        probe.fill_(7)
        for call in (lambda: pat.replace_into(dev, b"xy", w.view), lambda: pat.replace_into(dev, b"xy", None)):
            try:
                call()
            except ss.SlicesliceError as x:
                errs.append(x)
    torch.cuda.synchronize()
    assert len(errs) == 2 and all(e.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(e) for e in errs), errs
    if torch.cuda.device_count() > 1:                                   # a handle made on another device
        with torch.cuda.device(1):
            elsewhere = torch.zeros(4096, dtype=torch.uint8, device="cuda:1")
            with pytest.raises(ss.SlicesliceError, match="was made on device"):
                pat.replace_into(elsewhere, b"xy", None)
    w.check(b"", "refusals")


# ---- the fixture and the front end ---------------------------------------------------------------------------------------------------
def test_every_row_of_the_fixture_on_the_manual(ss, manual):
    kat = json.load(open(os.path.join(GOLDEN, "rewrite_kat.json")))
    d_manual = torch.from_numpy(np.frombuffer(manual, dtype=np.uint8).copy()).cuda()
    assert len(kat["cases"]) == 8
    with mk_lib(ss):
        for case in kat["cases"]:
            pat = ss.RunPattern(case["pattern"])
            text = case["text"].encode("latin-1")
            w = ByteWindow(case["out_len"], 13)
            assert pat.replace_into(d_manual, text, w.view, case["delimiter"]) == (case["out_len"], case["count"]), case["name"]
            h = w.buf.cpu().numpy()
            out = h[w.at:w.at + case["out_len"]].tobytes()
            assert hashlib.sha256(out).hexdigest() == case["sha256"], case["name"]
            assert out[:G.KEEP].hex() == case["first"] and out[-G.KEEP:].hex() == case["last"], case["name"]
            assert (h[:w.at] == SENT).all() and (h[w.at + case["out_len"]:] == SENT).all(), case["name"]
            got = pat.replace(d_manual, text, case["delimiter"])
            assert got.numel() == case["out_len"] and hashlib.sha256(got.cpu().numpy().tobytes()).hexdigest() == case["sha256"], case["name"]


def test_the_front_end_prints_what_re_sub_gives(manual):
    path = os.path.join(GOLDEN, "data", "i386.txt")

    def run(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True)

    r = run("--runs", " {2,}", "--replace", " ", path)
    assert r.returncode == 0 and r.stdout == re.sub(rb" {2,}", b" ", manual), r.stderr[-300:]
    r = run("--runs", r"\s+", "--replace", "", "--per-line", path)              # an empty text deletes; line by line, as sed does
    assert r.returncode == 0 and r.stdout == b"\n".join(re.sub(rb"\s+", b"", line) for line in manual.split(b"\n")), r.stderr[-300:]
    r = run("--runs", "[0-9]+", "--replace", "N", "--count", path)              # not combined with the listing modes
    assert r.returncode != 0 and r.stdout == b"" and b"not combined with --count" in r.stderr, r.stderr[-300:]
