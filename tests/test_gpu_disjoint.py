"""GPU tests of the non-overlapping calls (include/sliceslice_hip_disjoint.h, libsliceslice_hip_disjoint.so):
ss_select_disjoint_device on hand-made lists aimed at the borders of SS_DISJOINT_BLOCK, ss_count_disjoint_device /
ss_find_all_disjoint_device and ss_replace_device against Python's own bytes.count, re.finditer and bytes.replace, and against
tests/golden/disjoint_kat.json (GNU grep -o -b -F).  Every comparison is of integers or bytes and exact; every output array is a
window of a larger one whose sentinels on both sides must survive.  The manual's text aside, no view is larger than 200,000 bytes
and no list longer than four blocks."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
B = 4096                                # SS_DISJOINT_BLOCK
PART = 65536                            # SS_CONTEXT_PART_BYTES
GUARD = 8
SENT64 = -0x5A5A5A5A5A5A5A5B
W = rb"[0-9A-Za-z_]"


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def dj_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.disjoint_build()`."""
    return _loaded() if getattr(ss.lib(), "has_disjoint", False) else ss.disjoint_build()


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    assert m.DISJOINT_BLOCK == B
    with dj_lib(m):
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


def dev_view(host, mis=0, before=b"", after=b""):
    """the bytes of `host` on the device at 16-byte misalignment `mis`, with `before` and `after` just outside both ends"""
    host = np.frombuffer(bytes(host), dtype=np.uint8)
    buf = torch.full((host.size + 96,), ord("a"), dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + 32 + mis
    view = buf[at:at + host.size]
    if host.size:
        view.copy_(torch.from_numpy(host.copy()))
    if before:
        buf[at - len(before):at].copy_(torch.from_numpy(np.frombuffer(before, dtype=np.uint8).copy()))
    if after:
        buf[at + host.size:at + host.size + len(after)].copy_(torch.from_numpy(np.frombuffer(after, dtype=np.uint8).copy()))
    assert view.data_ptr() % 16 == mis
    return view


def holds(case, offsets):
    """the fixture's list is `offsets`: given in full, or - a long list - by its SHA-256 as little-endian 64-bit words and its ends"""
    offsets = [int(o) for o in offsets]
    if "offsets" in case:
        return offsets == case["offsets"]
    digest = hashlib.sha256(np.asarray(offsets, dtype="<u8").tobytes()).hexdigest()
    return digest == case["offsets_sha256"] and offsets[:16] == case["first"] and offsets[-16:] == case["last"] and len(offsets) == case["count"]


def greedy(offsets, n):
    """the obvious loop"""
    out = []
    for p in offsets:
        if not out or p - out[-1] >= n:
            out.append(p)
    return out


def rule(hb, nd, ignore_case=False, whole_word=False):
    """the offsets re.finditer gives for the needle between two lookarounds"""
    pat = re.escape(nd)
    if whole_word:
        pat = rb"(?<!" + W + rb")" + pat + rb"(?!" + W + rb")"
    return [m.start() for m in re.finditer(pat, hb, re.I if ignore_case else 0)]


# ---- the primitive ------------------------------------------------------------------------------------------------------------------
def select_case(ss, offsets, n, what, caps=None):
    want = greedy(offsets, n)
    total = len(want)
    d = torch.from_numpy(np.asarray(offsets, dtype=np.uint64).view(np.int64).copy()).cuda()
    with dj_lib(ss):
        assert ss.select_disjoint_into(d, n, None) == total, what
        for cap in (caps if caps is not None else sorted({0, 1, max(total - 1, 0), total})):
            w = Window(cap)
            assert ss.select_disjoint_into(d, n, w.view) == total, (what, cap)
            w.check(np.asarray(want[:cap], dtype=np.uint64).view(np.int64), (what, cap))
    return total


def test_select_nothing_and_one(ss):
    assert select_case(ss, [], 3, "empty") == 0
    assert select_case(ss, [7], 3, "one") == 1
    assert select_case(ss, [7], 2 ** 64 - 1, "one, the longest n") == 1


@pytest.mark.parametrize("n", [2, 3, 7, B])
def test_select_consecutive_offsets_across_two_block_borders(ss, n):
    """every block without a head but the first: the chain kernel walks them one after another"""
    count = 2 * B + 5
    assert select_case(ss, list(range(count)), n, "consecutive n=%d" % n) == (count + n - 1) // n


def test_select_an_exit_that_skips_a_whole_block(ss):
    assert select_case(ss, list(range(3 * B + 11)), 10000, "n = 10,000") == 2
    assert select_case(ss, list(range(100, 4 * B + 100)), 3 * B + 1, "n = 3B + 1") == 2


def test_select_gaps_alternating_three_and_four(ss):
    offsets = np.cumsum([5] + [3 + (k & 1) for k in range(2 * B + 2)]).tolist()
    assert len(offsets) == 2 * B + 3
    select_case(ss, offsets, 5, "gaps 3, 4 with n = 5")
    select_case(ss, offsets, 4, "gaps 3, 4 with n = 4")


@pytest.mark.parametrize("at", [B, 2 * B - 1, B + 1])
def test_select_a_head_at_a_blocks_first_last_and_second_entry(ss, at):
    """consecutive offsets but for one gap of n in front of entry `at`"""
    n = 3
    for start in (0, 1, 2):                                     # the chain meets the head in every phase
        offsets = [start + k + (n if k >= at else 0) for k in range(2 * B + 7)]
        select_case(ss, offsets, n, "head at %d, start %d" % (at, start), caps=None if start == 0 else [len(greedy(offsets, n))])


def test_select_isolated_offsets_and_offsets_above_two_to_the_32(ss):
    count = 2 * B + 100
    assert select_case(ss, [10 * k for k in range(count)], 10, "all heads") == count
    assert select_case(ss, [10 * k for k in range(count)], 11, "no head but the first") == (count + 1) // 2
    high = [(1 << 32) - 5 + 2 * k for k in range(B + 50)] + [(1 << 40) + 3 * k for k in range(50)] + [2 ** 64 - 7, 2 ** 64 - 4, 2 ** 64 - 1]
    select_case(ss, high, 5, "above 2^32")
    select_case(ss, high, 2 ** 63, "above 2^32, n = 2^63")


def test_select_a_list_that_breaks_the_contract_stays_inside_its_window(ss):
    rng = np.random.default_rng(5)
    offsets = rng.integers(0, 5000, size=2 * B + 9).astype(np.int64)
    d = torch.from_numpy(offsets).cuda()
    with dj_lib(ss):
        for cap in (0, 1, 1000, 3000, 2 * B + 20):
            w = Window(cap)
            total = ss.select_disjoint_into(d, 4, w.view)           # (unspecified, but the bound of what may be written)
            assert 1 <= total <= offsets.size
            h = w.buf.cpu().numpy()
            assert (h[:GUARD] == SENT64).all() and (h[GUARD + min(cap, total):] == SENT64).all(), cap


def test_select_refusals(ss):
    d = torch.arange(10, dtype=torch.int64, device="cuda")
    with dj_lib(ss):
        with pytest.raises(ss.SlicesliceError, match="in place") as e:
            ss.select_disjoint_into(d, 2, d)
        assert e.value.code == ss.SS_ERR_ARGUMENT and d.cpu().tolist() == list(range(10))
        with pytest.raises(ss.SlicesliceError, match="n is 0"):
            ss.select_disjoint_into(d, 0, None)
        assert ss.select_disjoint(list(range(10)), 4).cpu().tolist() == [0, 4, 8]
        assert ss.select_disjoint(d, 4, capacity=2).cpu().tolist() == [0, 4]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
HAYSTACKS = {"a": b"a" * 40000, "ab": b"ab" * 20000, "aabaaabaabaa": (b"aabaaabaabaa" * 3334)[:40000]}


@pytest.mark.parametrize("needle", [b"aa", b"aaa", b"abab", b"aabaa"])
@pytest.mark.parametrize("name", sorted(HAYSTACKS))
def test_periodic_needles_at_three_misalignments(ss, needle, name):
    hb = HAYSTACKS[name]
    want = rule(hb, needle)
    assert len(want) == hb.count(needle)
    with dj_lib(ss):
        s = ss.DynamicHipSearcher.new(needle)
        for mis in (0, 1, 15):
            view = dev_view(hb, mis, before=needle, after=needle)
            assert s.count_disjoint(view) == len(want), (name, mis)
            for cap in sorted({0, 1, max(len(want) - 1, 0), len(want)}):
                w = Window(cap)
                assert s.find_all_disjoint_into(view, w.view) == len(want), (name, mis, cap)
                w.check(want[:cap], (name, mis, cap))


def test_the_fixture_on_the_manual(ss, manual, d_manual):
    kat = json.load(open(os.path.join(GOLDEN, "disjoint_kat.json")))
    assert kat["bytes"] == len(manual)
    with dj_lib(ss):
        for case in kat["cases"]:
            needle, flags = case["needle"].encode(), case["flags"]
            kw = dict(ignore_case="-i" in flags, whole_word="-w" in flags)
            s = ss.DynamicHipSearcher.new(needle)
            assert s.count_disjoint(d_manual, **kw) == case["count"], case["name"]
            assert holds(case, s.find_all_disjoint(d_manual, **kw).cpu().tolist()), case["name"]
            if case["overlapping"] is not None:
                assert s.count(d_manual, ignore_case=kw["ignore_case"]) == case["overlapping"], case["name"]


def test_a_needle_without_a_border_is_its_model(ss, d_manual):
    with dj_lib(ss):
        s = ss.DynamicHipSearcher.new(b"the")
        for kw in (dict(), dict(ignore_case=True), dict(whole_word=True), dict(ignore_case=True, whole_word=True)):
            assert s.count_disjoint(d_manual, **kw) == s.count(d_manual, **kw)
            assert torch.equal(s.find_all_disjoint(d_manual, **kw), s.find_all(d_manual, **kw))
            assert torch.equal(s.find_all_disjoint(d_manual, capacity=5, **kw), s.find_all(d_manual, capacity=5, **kw))


def test_ignore_case_and_whole_word_against_the_lookaround_regex(ss):
    with dj_lib(ss):
        for hb, needle in ((b".. ... ....", b".."), (b"aaa aa -aa-aa- aa", b"aa"), (b"aAaA AA_aa aaaa-AAaa aa" * 700, b"aa"),
                           (b"xx.x xx xxxx x_x xx-xx xxx " * 900, b"xx"), ((b"AbA" * 7 + b" ") * 500, b"aba")):
            s = ss.DynamicHipSearcher.new(needle)
            view = dev_view(hb, 3, before=needle, after=needle)
            for ic in (False, True):
                for ww in (False, True):
                    want = rule(hb, needle, ic, ww)
                    assert s.count_disjoint(view, ignore_case=ic, whole_word=ww) == len(want), (hb[:20], ic, ww)
                    assert s.find_all_disjoint(view, ignore_case=ic, whole_word=ww).cpu().tolist() == want, (hb[:20], ic, ww)
    assert rule(b".. ... ....", b"..", whole_word=True) == [0, 3, 7, 9]          # (what GNU grep -o -b -w -F prints)
    assert rule(b"aaa aa -aa-aa- aa", b"aa", whole_word=True) == [4, 8, 11, 15]


def test_the_empty_needle(ss):
    with dj_lib(ss):
        s = ss.DynamicHipSearcher.new(b"")
        view = dev_view(b"abc" * 100, 5)
        assert s.count_disjoint(view) == 301 == s.count(view)
        assert s.find_all_disjoint(view).cpu().tolist() == list(range(301))
        for kw in (dict(ignore_case=True), dict(whole_word=True)):
            with pytest.raises(ss.SlicesliceError, match="empty needle") as e:
                s.count_disjoint(view, **kw)
            assert e.value.code == ss.SS_ERR_ARGUMENT
        with pytest.raises(ss.SlicesliceError, match="empty needle"):
            s.replace(view, b"x")


def test_refusals_write_nothing(ss):
    import ctypes
    with dj_lib(ss):
        L = ss.lib()
        s = ss.DynamicHipSearcher.new(b"aa")
        view = dev_view(b"aaaa" * 100, 0)
        w = Window(16)
        total = ctypes.c_uint64(77)
        for how, word in ((2, "SS_BOUND_LINE"), (8, "SS_CONTEXT_INVERT"), (16, "bits other than"), (1 | 2, "SS_BOUND_LINE")):
            rc = L.ss_find_all_disjoint_device(s._h, view.data_ptr(), view.numel(), how, 0, w.view.data_ptr(), 16, ctypes.byref(total))
            assert rc == ss.SS_ERR_ARGUMENT and word in L.ss_last_error().decode(), how
            rc = L.ss_count_disjoint_device(s._h, view.data_ptr(), view.numel(), how, 0, ctypes.byref(total))
            assert rc == ss.SS_ERR_ARGUMENT and word in L.ss_last_error().decode(), how
        upper = ss.DynamicHipSearcher.new(b"AA")
        rc = L.ss_find_all_disjoint_device(upper._h, view.data_ptr(), view.numel(), 4, 0, w.view.data_ptr(), 16, ctypes.byref(total))
        assert rc == ss.SS_ERR_ARGUMENT and "upper-case" in L.ss_last_error().decode()      # (the model's refusal)
        assert s.count_disjoint(view) == 200                                       # (first use outside the capture)
        probe = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            probe.fill_(7)                                                          # (something to capture: the refused call adds nothing)
            capturing = torch.cuda.current_stream().cuda_stream
            rc = L.ss_count_disjoint_device(s._h, view.data_ptr(), view.numel(), 0, capturing, ctypes.byref(total))
            msg = L.ss_last_error().decode()
        assert rc == ss.SS_ERR_ARGUMENT and "cannot be captured" in msg
        w.check([], "refusals")
        assert total.value == 77


# ---- replace ----------------------------------------------------------------------------------------------------------------------
def replace_haystack(needle):
    """3 * PART + 5 bytes: an occurrence at each end of the view, one straddling each part border (from the aligned address of a
    view at misalignment 0), a run of overlapping occurrences and scattered ones"""
    n = len(needle)
    size = 3 * PART + 5
    hb = bytearray(b"." * size)
    for at in (PART - 1, 2 * PART - n + 1, 3 * PART - 1, 1000, 1000 + n, 70000, 0, size - n):
        hb[at:at + n] = needle
    hb[5000:5000 + 9 * n] = needle * 9
    if needle == b"aa":
        hb[9000:9011] = b"a" * 11
    return bytes(hb)


@pytest.mark.parametrize("needle", [b"aa", b"abcab", b"q"])
def test_replace_against_bytes_replace(ss, needle):
    n = len(needle)
    hb = replace_haystack(needle)
    assert hb.startswith(needle) and hb.endswith(needle)
    with dj_lib(ss):
        s = ss.DynamicHipSearcher.new(needle)
        for mis in (0, 7):
            view = dev_view(hb, mis, before=needle, after=needle)
            for rl in sorted({0, n - 1, n, n + 1, 3 * n}):
                rep = (b"XYZWVUTSRQPONML" * 2)[:rl]
                want = hb.replace(needle, rep)
                got = s.replace(view, rep)
                assert got.dtype == torch.uint8 and got.device == view.device
                assert bytes(got.cpu().numpy()) == want, (needle, mis, rl)


def test_replace_without_an_occurrence_and_at_its_capacities(ss):
    import ctypes
    hb = replace_haystack(b"aa")
    with dj_lib(ss):
        L = ss.lib()
        view = dev_view(hb, 9)
        absent = ss.DynamicHipSearcher.new(b"no such")
        assert bytes(absent.replace(view, b"whatever").cpu().numpy()) == hb
        s = ss.DynamicHipSearcher.new(b"aa")
        want = hb.replace(b"aa", b"xyz")
        out_len, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rep = ctypes.create_string_buffer(b"xyz", 3)
        # one short: nothing written
        w = Window(len(want), dtype=torch.uint8, sent=0x5A)
        rc = L.ss_replace_device(s._h, view.data_ptr(), view.numel(), 0, rep, 3, 0, w.view.data_ptr(), len(want) - 1, ctypes.byref(out_len),
                                 ctypes.byref(count))
        assert rc == ss.SS_OK and out_len.value == len(want) and count.value == hb.count(b"aa")
        w.check([], "one short")
        # exact, with the sentinels behind it
        rc = L.ss_replace_device(s._h, view.data_ptr(), view.numel(), 0, rep, 3, 0, w.view.data_ptr(), len(want), ctypes.byref(out_len),
                                 ctypes.byref(count))
        assert rc == ss.SS_OK and out_len.value == len(want)
        w.check(np.frombuffer(want, dtype=np.uint8), "exact")
        # the output inside the haystack's buffer
        big = torch.full((4 * view.numel(),), ord("a"), dtype=torch.uint8, device="cuda")
        inner = big[100:100 + view.numel()]
        for at in (0, 50, 100 + view.numel() - 1):
            rc = L.ss_replace_device(s._h, inner.data_ptr(), inner.numel(), 0, rep, 3, 0, big.data_ptr() + at, 2 * view.numel(), ctypes.byref(out_len),
                                     ctypes.byref(count))
            assert rc == ss.SS_ERR_ARGUMENT and "intersects" in L.ss_last_error().decode(), at
        assert bool((big == ord("a")).all())
        # ignore_case and whole_word reach replace
        text = b"aa AA aaa Aa-aA" * 50
        t = dev_view(text, 2)
        assert bytes(s.replace(t, b"<>", ignore_case=True, whole_word=True).cpu().numpy()) == \
            re.sub(rb"(?<!" + W + rb")aa(?!" + W + rb")", b"<>", text, flags=re.I)


# ---- the command-line tool ------------------------------------------------------------------------------------------------------------
def test_grep_hip_only_matching_and_replace(ss, manual):
    """tools/grep_hip.py -o prints what grep -o -b -F printed into the fixture, --replace what bytes.replace gives"""
    import subprocess
    import sys
    kat = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "disjoint_kat.json")))["cases"]}
    path = os.path.join(GOLDEN, "data", "i386.txt")

    def grep(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True, timeout=600)

    case = kat["the_w"]                                         # (three processes in all: each one loads torch and opens the GPU)
    got = grep("-o", "--offsets", *case["flags"], case["needle"], path)
    lines = got.stdout.split(b"\n")
    assert got.returncode == 0 and lines[-1] == b"" and all(l.endswith(b":the") for l in lines[:-1]), got.stderr[-500:]
    assert holds(case, [int(l[:-4]) for l in lines[:-1]])
    case = kat["intel_i"]
    counted = grep("--only-matching", "--count", *case["flags"], case["needle"], path)
    assert counted.returncode == 0 and counted.stdout == b"%d\n" % case["count"], counted.stderr[-500:]
    replaced = grep("--replace", "<-->", "  ", path)
    assert replaced.returncode == 0 and replaced.stdout == manual.replace(b"  ", b"<-->"), replaced.stderr[-500:]
