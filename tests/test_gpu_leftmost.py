"""GPU tests of the leftmost-longest calls (include/sliceslice_hip_leftmost.h, libsliceslice_hip_leftmost.so):
ss_select_leftmost_device on hand-made lists aimed at the borders of SS_LEFTMOST_BLOCK, ss_count_leftmost_set_device /
ss_find_all_leftmost_set_device and ss_replace_set_device against the rule restated in Python
(tests/golden/make_leftmost_golden.py: a byte-wise loop, and a ``re`` alternation sorted longest first) and against
tests/golden/leftmost_kat.json (GNU grep -o -b -F).  Every comparison is of integers or bytes and exact; every output array and
buffer is a window of a larger one whose sentinels on both sides must survive.  The manual's text aside, no view is larger than
200,000 bytes."""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
B = 4096                                # SS_LEFTMOST_BLOCK
CHUNK = 16384                           # SS_OUTPUT_CHUNK
GUARD = 8
SENT64 = -0x5A5A5A5A5A5A5A5B
SENT32 = -0x5A5A5A5B
SENT8 = 0xA5

sys.path.insert(0, GOLDEN)
try:
    import make_leftmost_golden as G
finally:
    sys.path.remove(GOLDEN)


class _loaded:
    def __init__(self, L):
        self.L = L

    def __enter__(self):
        return self.L

    def __exit__(self, *a):
        return False


def lm_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.leftmost_build()`."""
    L = ss.lib()
    return _loaded(L) if getattr(L, "has_leftmost", False) else ss.leftmost_build()


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    assert m.LEFTMOST_BLOCK == B and m.OUTPUT_CHUNK == CHUNK
    return m


@pytest.fixture(scope="module")
def manual():
    return open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()


@pytest.fixture(scope="module")
def d_manual(manual):
    return torch.from_numpy(np.frombuffer(manual, dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "leftmost_kat.json")))


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
    buf = torch.full((host.size + 160,), ord("~"), dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + 64 + mis
    if before:
        buf[at - len(before):at] = torch.from_numpy(np.frombuffer(before, dtype=np.uint8).copy()).cuda()
    if after:
        buf[at + host.size:at + host.size + len(after)] = torch.from_numpy(np.frombuffer(after, dtype=np.uint8).copy()).cuda()
    if host.size:
        buf[at:at + host.size] = torch.from_numpy(host.copy()).cuda()
    return buf[at:at + host.size]


def select_rule(offsets, lengths):
    """indices of the selected entries: the rule of the primitive as a loop"""
    out, nxt, n = [], 0, len(offsets)
    for j in range(n):
        if j + 1 < n and offsets[j + 1] == offsets[j]:
            continue
        if offsets[j] < nxt:
            continue
        out.append(j)
        nxt = offsets[j] + lengths[j]
    return out


def check_select(ss, offsets, lengths, what, capacities=None):
    offsets, lengths = [int(x) for x in offsets], [int(x) for x in lengths]
    want = select_rule(offsets, lengths)
    d_off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lengths, dtype=torch.int64, device="cuda")
    with lm_lib(ss):
        assert ss.select_leftmost_into(d_off, d_len, None, None, 0) == len(want), what
        for cap in capacities if capacities is not None else [len(want)]:
            k = min(cap, len(want))
            sel, which = Window(cap), Window(cap)
            assert ss.select_leftmost_into(d_off, d_len, sel.view if cap else None, which.view if cap else None, cap) == len(want), (what, cap)
            sel.check([offsets[j] for j in want[:k]], (what, cap, "offsets"))
            which.check(want[:k], (what, cap, "which"))
            if cap:                                                     # each array left out in turn
                only = Window(cap)
                assert ss.select_leftmost_into(d_off, d_len, only.view, None, cap) == len(want)
                only.check([offsets[j] for j in want[:k]], (what, cap, "offsets alone"))
                only = Window(cap)
                assert ss.select_leftmost_into(d_off, d_len, None, only.view, cap) == len(want)
                only.check(want[:k], (what, cap, "which alone"))
    return want


# ---- the primitive ----------------------------------------------------------------------------------------------------------------
def test_nothing_and_one_entry(ss):
    check_select(ss, [], [], "nothing", [0, 3])
    check_select(ss, [7], [3], "one entry", [0, 1, 2])
    check_select(ss, [7, 7, 7], [1, 2, 3], "one run", [0, 1, 2])


@pytest.mark.parametrize("length", [2, 3, 7, B])
def test_consecutive_offsets_across_two_block_borders(ss, length):
    """offsets 0, 1, 2, ...: the only head is the first entry, so the chain walks two head-less blocks"""
    n = 2 * B + 37
    want = check_select(ss, range(100, 100 + n), [length] * n, ("consecutive", length))
    assert len(want) == (n + length - 1) // length


def test_lengths_alternating_1_and_a_block_and_5_where_an_exit_skips_a_whole_block(ss):
    n = 3 * B + 11
    lengths = [1 if j % 2 == 0 else B + 5 for j in range(n)]
    want = check_select(ss, range(n), lengths, "alternating")
    assert want[:3] == [0, 1, B + 6]
    lengths = [B + 5 if j % 2 == 0 else 1 for j in range(n)]
    check_select(ss, range(n), lengths, "alternating, long first")


@pytest.mark.parametrize("at", [0, 1, B - 1])
def test_a_head_at_a_blocks_first_last_and_second_entry(ss, at):
    """dense offsets with lengths 3; one gap of 1000 in front of entry B + at makes it the second block's only head"""
    n = 2 * B + 100
    offsets = [j if j < B + at else j + 1000 for j in range(n)]
    check_select(ss, offsets, [3] * n, ("head at", at))
    # ... and with a long entry in the list, so that the gap must reach its length
    lengths = [3] * n
    lengths[5] = 900
    check_select(ss, offsets, lengths, ("head at, one long", at))
    lengths[5] = 1001
    check_select(ss, offsets, lengths, ("no head but the first", at))


def test_runs_of_equal_offsets_at_block_borders(ss):
    # a run of five equal offsets straddling the border: three in the first block, two in the second
    offsets = list(range(B - 3)) + [B + 10] * 5 + list(range(B + 11, 2 * B + 50))
    lengths = [2] * (B - 3) + [1, 2, 3, 4, 9] + [2] * (B + 39)
    want = check_select(ss, offsets, lengths, "run across the border")
    assert B + 1 in want
    # a run that is a block's last entries
    offsets = list(range(B - 4)) + [B + 10] * 4 + list(range(B + 11, 2 * B + 50))
    lengths = [2] * (B - 4) + [1, 2, 3, 4] + [2] * (B + 39)
    want = check_select(ss, offsets, lengths, "run at the end of a block")
    assert B - 1 in want
    # every offset twice, the longer one blocking the next offset
    offsets = [j // 2 for j in range(2 * B + 6)]
    lengths = [1 + (j % 2) for j in range(2 * B + 6)]
    want = check_select(ss, offsets, lengths, "every offset twice")
    assert want[:3] == [1, 5, 9]


def test_equal_offsets_where_the_longest_is_not_a_whole_block_away(ss):
    offsets, lengths = [], []
    for p in range(0, 3 * B, 3):
        for l in (1, 2, 5, 7)[:1 + p % 4]:
            offsets.append(p)
            lengths.append(l)
    check_select(ss, offsets, lengths, "mixed runs", [0, 1, 17])
    rng = np.random.default_rng(5)
    offsets = np.sort(rng.integers(0, 40000, size=3 * B + 123)).tolist()
    lengths, run = [], 0
    for j, p in enumerate(offsets):
        run = run + 1 if j and offsets[j - 1] == p else 0
        lengths.append(1 + run * 3 + (int(rng.integers(0, 30)) if run == 0 else 0))
    lengths = [lengths[j] if not (j and offsets[j - 1] == offsets[j]) else max(lengths[j], lengths[j - 1]) for j in range(len(offsets))]
    for j in range(1, len(offsets)):                                    # ascending within a run
        if offsets[j] == offsets[j - 1] and lengths[j] < lengths[j - 1]:
            lengths[j] = lengths[j - 1]
    check_select(ss, offsets, lengths, "random runs")


def test_offsets_above_2_to_the_32(ss):
    base = (1 << 40) + 12345
    n = B + 500
    offsets = [base + 3 * j for j in range(n)] + [base + (1 << 33) + j for j in range(300)]
    lengths = [4 + j % 5 for j in range(n)] + [2] * 300
    want = check_select(ss, offsets, lengths, "large offsets")
    assert offsets[want[-1]] > (1 << 40) + (1 << 33)


def test_a_list_that_breaks_the_contract_stays_inside_its_window(ss):
    rng = np.random.default_rng(11)
    n = 2 * B + 77
    offsets = rng.integers(0, 5000, size=n).astype(np.int64)            # not ascending
    lengths = rng.integers(0, 9, size=n).astype(np.int64)               # zeros among them
    d_off, d_len = torch.from_numpy(offsets).cuda(), torch.from_numpy(lengths).cuda()
    with lm_lib(ss):
        total = ss.select_leftmost_into(d_off, d_len, None, None, 0)
        assert 0 <= total <= n
        for cap in (0, 1, 100, n):
            sel, which = Window(cap), Window(cap)
            assert ss.select_leftmost_into(d_off, d_len, sel.view if cap else None, which.view if cap else None, cap) == total
            for w in (sel, which):                                      # the values are unspecified; the sentinels are not
                h = w.buf.cpu().numpy()
                assert (h[:GUARD] == SENT64).all() and (h[GUARD + cap:] == SENT64).all() and (h[GUARD + min(cap, total):] == SENT64).all()


def test_capacities(ss):
    n = B + 900
    offsets = [2 * j for j in range(n)]
    lengths = [3 if j % 3 else 1 for j in range(n)]
    total = len(select_rule(offsets, lengths))
    check_select(ss, offsets, lengths, "capacities", [0, 1, total - 1, total, total + 5])


def test_the_primitive_refusals(ss):
    with lm_lib(ss) as L:
        s = ss.searcher._scratch_set(L)
        d = torch.arange(8, dtype=torch.int64, device="cuda")
        ones = torch.ones(8, dtype=torch.int64, device="cuda")
        out = Window(8)
        total = ctypes.c_uint64(77)
        st = torch.cuda.current_stream().cuda_stream

        def call(set_, off, lens, count, sel, which, cap, result=total):
            return L.ss_select_leftmost_device(set_, off, lens, count, st, sel, which, cap, ctypes.byref(result) if result is not None else None)

        for args, why in (((None, d.data_ptr(), ones.data_ptr(), 8, out.view.data_ptr(), None, 8), "set is NULL"),
                          ((s._h, None, ones.data_ptr(), 8, out.view.data_ptr(), None, 8), "NULL"),
                          ((s._h, d.data_ptr(), None, 8, out.view.data_ptr(), None, 8), "NULL"),
                          ((s._h, d.data_ptr(), ones.data_ptr(), 8, d.data_ptr(), None, 8), "in place"),
                          ((s._h, d.data_ptr(), ones.data_ptr(), 1 << 48, out.view.data_ptr(), None, 8), "2^48")):
            assert call(*args) == ss.SS_ERR_ARGUMENT and why in L.ss_last_error().decode(), why
            assert total.value == 77
        assert call(s._h, d.data_ptr(), ones.data_ptr(), 8, out.view.data_ptr(), None, 8, None) == ss.SS_ERR_ARGUMENT
        out.check([], "refusals write nothing")
        assert ss.select_leftmost_into(d, ones, None, None, 0) == 8                 # (first use outside the capture)
        probe = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            probe.fill_(7)                                                          # (something to capture: the refused call adds nothing)
            capturing = torch.cuda.current_stream().cuda_stream
            rc = L.ss_select_leftmost_device(s._h, d.data_ptr(), ones.data_ptr(), 8, capturing, out.view.data_ptr(), None, 8, ctypes.byref(total))
            msg = L.ss_last_error().decode()
        assert rc == ss.SS_ERR_ARGUMENT and "cannot be captured" in msg
        out.check([], "a capturing stream writes nothing")


# ---- the haystack calls -----------------------------------------------------------------------------------------------------------
def check_find(ss, host, needles, what, ignore_case=False, whole_word=False, mis=0, before=b"", after=b"", capacities=None):
    want = G.rule(host, needles, ignore_case, whole_word)
    view = dev_view(host, mis, before, after)
    with lm_lib(ss):
        nset = ss.NeedleSet(needles, ignore_case=ignore_case)
        assert nset.count_leftmost(view, whole_word) == len(want), what
        ranks = nset.ranks()
        for cap in capacities if capacities is not None else [len(want)]:
            k = min(cap, len(want))
            off, rk = Window(cap), Window(cap, torch.int32, SENT32)
            assert nset.find_all_leftmost_into(view, off.view if cap else None, rk.view if cap else None, cap, whole_word) == len(want), (what, cap)
            off.check([p for p, _ in want[:k]], (what, cap, "offsets"))
            rk.check([int(ranks[i]) for _, i in want[:k]], (what, cap, "ranks"))
            if cap:
                only = Window(cap)
                assert nset.find_all_leftmost_into(view, only.view, None, cap, whole_word) == len(want)
                only.check([p for p, _ in want[:k]], (what, cap, "offsets alone"))
                only = Window(cap, torch.int32, SENT32)
                assert nset.find_all_leftmost_into(view, None, only.view, cap, whole_word) == len(want)
                only.check([int(ranks[i]) for _, i in want[:k]], (what, cap, "ranks alone"))
        offsets, which = nset.find_all_leftmost(view, whole_word)
        assert offsets.cpu().tolist() == [p for p, _ in want] and which.cpu().tolist() == [i for _, i in want], what
    return want


def test_the_fixture_on_the_manual(ss, manual, d_manual, kat):
    assert kat["grep_checked"] and "3.7" in kat["grep_version"]
    with lm_lib(ss):
        sets = {}
        for row in kat["rows"]:
            key = (row["set"], row["ignore_case"])
            if key not in sets:
                sets[key] = ss.NeedleSet([n.encode("latin-1") for n in kat["sets"][row["set"]]], ignore_case=row["ignore_case"])
            nset = sets[key]
            assert nset.count_leftmost(d_manual, row["whole_word"]) == row["count"], row
            offsets, which = nset.find_all_leftmost(d_manual, row["whole_word"])
            pairs = list(zip(offsets.cpu().tolist(), which.cpu().tolist()))
            assert len(pairs) == row["count"] and [list(x) for x in pairs[:8]] == row["first"] and [list(x) for x in pairs[-8:]] == row["last"], row
            assert G.list_hash(pairs) == row["sha256"], row


@pytest.mark.parametrize("mis", [0, 5, 15])
def test_prefixes_infixes_and_self_overlap_on_one_and_two_letter_haystacks(ss, mis):
    rng = np.random.default_rng(100 + mis)
    one = b"a" * 20011
    two = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=30007, p=[0.7, 0.3]))
    for needles in ([b"a", b"aa", b"aaa"], [b"aa", b"aaaaa"], [b"ab", b"aba", b"abab", b"b"], [b"aab", b"a", b"ba", b"baab"],
                    [b"abaab", b"baa", b"aa"], [b"a" * 40, b"a" * 7, b"b"]):
        check_find(ss, one, needles, ("one letter", needles, mis), mis=mis)
        check_find(ss, two, needles, ("two letters", needles, mis), mis=mis, capacities=[0, 1, 1000])


def test_ignore_case_and_whole_word_against_the_lookaround_regex(ss, manual):
    part = manual[200000:320000]
    for needles in ([b"the", b"then", b"there", b"he", b"here"], [b"Segment", b"segment descriptor", b"seg", b"descriptor table"],
                    [b"a", b"an", b"and", b"any"]):
        for ignore_case in (False, True):
            for whole_word in (False, True):
                want = check_find(ss, part, needles, (needles, ignore_case, whole_word), ignore_case, whole_word, mis=3)
                assert want == G.rule_regex(part, needles, ignore_case, whole_word)


def test_the_longest_at_an_offset_is_no_word_and_a_shorter_one_is(ss):
    host = b"in int int_ interrupt interrupts;interrupted in" * 50
    needles = [b"int", b"interrupt", b"in", b"interrupts", b"int_"]
    want = check_find(ss, host, needles, "shorter whole word", whole_word=True)
    assert (0, 2) in want and (3, 0) in want
    host = b"foo-bar foo-barx foo " * 40
    want = check_find(ss, host, [b"foo", b"foo-bar", b"foo-barx "], "the longest is no word", whole_word=True)
    assert want[:3] == [(0, 1), (8, 0), (17, 0)]


def test_a_needle_copy_just_outside_both_ends_of_the_view(ss):
    needles = [b"needle", b"need", b"dle"]
    for mis in (0, 9):
        host = b"xx needle yy need" + b"z" * 3000 + b"nee"
        check_find(ss, host, needles, ("outside", mis), mis=mis, before=b"needle", after=b"dle")
        check_find(ss, host, needles, ("outside, words", mis), whole_word=True, mis=mis, before=b"needle", after=b"dle")
        check_find(ss, b"eedle" + host + b"need", needles, ("cut at both ends", mis), mis=mis, before=b"n", after=b"le")


def test_a_single_needle_set_equals_find_all_disjoint(ss, d_manual):
    with lm_lib(ss):
        for needle, kw in ((b"  ", {}), (b"the", {"whole_word": True}), (b"---", {}), (b"ss", {})):
            nset = ss.NeedleSet([needle])
            want = ss.DynamicHipSearcher.new(needle).find_all_disjoint(d_manual, **kw)
            got, which = nset.find_all_leftmost(d_manual, kw.get("whole_word", False))
            assert torch.equal(got, want) and int(which.max()) == 0 and want.numel() > 0, needle
            assert nset.count_leftmost(d_manual, kw.get("whole_word", False)) == want.numel()


def test_a_set_whose_needles_cannot_overlap_equals_find_all(ss, d_manual):
    with lm_lib(ss):
        nset = ss.NeedleSet([b"descriptor", b"privilege", b"Figure", b"80386"])
        want_off, want_which = nset.find_all(d_manual)
        got_off, got_which = nset.find_all_leftmost(d_manual)
        assert torch.equal(got_off, want_off) and torch.equal(got_which, want_which) and want_off.numel() > 1000


def test_the_haystack_calls_refusals_write_nothing(ss, d_manual):
    with lm_lib(ss) as L:
        nset, folded, empty = ss.NeedleSet([b"the", b"he"]), ss.NeedleSet([b"the"], ignore_case=True), ss.NeedleSet([b"the", b""])
        off, rk = Window(16), Window(16, torch.int32, SENT32)
        total = ctypes.c_uint64(77)
        st = torch.cuda.current_stream().cuda_stream
        n = d_manual.numel()

        def find(h, how, result=total, ptr=d_manual.data_ptr()):
            return L.ss_find_all_leftmost_set_device(h, ptr, n, how, st, off.view.data_ptr(), rk.view.data_ptr(), 16,
                                                     ctypes.byref(result) if result is not None else None)

        for refused, why in ((lambda: find(None, 0), "NULL"), (lambda: find(nset._h, 0, None), "NULL"),
                             (lambda: find(nset._h, ss.searcher.SS_BOUND_LINE), "SS_BOUND_LINE"),
                             (lambda: find(nset._h, ss.SS_CONTEXT_INVERT), "SS_CONTEXT_INVERT"), (lambda: find(nset._h, 64), "bits other than"),
                             (lambda: find(nset._h, ss.searcher.SS_BOUND_NOCASE), "SS_SET_NOCASE"), (lambda: find(folded._h, 0), "SS_SET_NOCASE"),
                             (lambda: find(empty._h, 0), "empty needle"), (lambda: find(nset._h, 0, total, None), "haystack is NULL")):
            rc = refused()
            assert rc == ss.SS_ERR_ARGUMENT and why in L.ss_last_error().decode(), (why, L.ss_last_error())
            assert total.value == 77
        assert L.ss_count_leftmost_set_device(empty._h, d_manual.data_ptr(), n, 0, st, ctypes.byref(total)) == ss.SS_ERR_ARGUMENT
        off.check([], "refusals write nothing")
        rk.check([], "refusals write nothing")
        assert nset.lengths().tolist() == [2, 3] and nset.ranks().tolist() == [1, 0]


# ---- replace ----------------------------------------------------------------------------------------------------------------------
def replace_into(ss, L, nset, view, texts, out_view, capacity, whole_word=False):
    """ss_replace_set_device into out_view[0, capacity) (None: no buffer); (rc, out_len, count)"""
    reps = (ctypes.c_char_p * len(texts))(*texts)
    lens = (ctypes.c_size_t * len(texts))(*[len(t) for t in texts])
    out_len, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = L.ss_replace_set_device(nset._h, view.data_ptr() if view.numel() else None, view.numel(), nset._occurrence_how(whole_word),
                                 ctypes.cast(reps, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p), len(texts),
                                 torch.cuda.current_stream().cuda_stream, out_view.data_ptr() if out_view is not None else None, capacity,
                                 ctypes.byref(out_len), ctypes.byref(count))
    return rc, out_len.value, count.value


def check_replace(ss, host, needles, texts, what, ignore_case=False, whole_word=False, hay_mis=0, out_mis=(0,)):
    want = G.substitute(host, needles, texts, ignore_case, whole_word)
    selected = len(G.rule(host, needles, ignore_case, whole_word))
    view = dev_view(host, hay_mis)
    with lm_lib(ss) as L:
        nset = ss.NeedleSet(needles, ignore_case=ignore_case)
        got = nset.replace(view, texts, whole_word)
        assert bytes(got.cpu().numpy()) == want, what
        assert bytes(nset.replace(view, dict(zip(needles, texts)), whole_word).cpu().numpy()) == want, (what, "mapping")
        for mis in out_mis:
            buf = torch.full((len(want) + 96,), SENT8, dtype=torch.uint8, device="cuda")
            at = (-buf.data_ptr()) % 16 + 32 + mis
            rc, out_len, count = replace_into(ss, L, nset, view, texts, buf[at:], len(want), whole_word)
            assert (rc, out_len, count) == (ss.SS_OK, len(want), selected), (what, mis)
            h = buf.cpu().numpy()
            assert bytes(h[at:at + len(want)]) == want and (h[:at] == SENT8).all() and (h[at + len(want):] == SENT8).all(), (what, mis)
            if want:                                                    # one byte short: the length and the count, and nothing written
                buf.fill_(SENT8)
                rc, out_len, count = replace_into(ss, L, nset, view, texts, buf[at:], len(want) - 1, whole_word)
                assert (rc, out_len, count) == (ss.SS_OK, len(want), selected) and bool((buf == SENT8).all()), (what, mis)
    return want


def test_replace_against_re_sub_with_mixed_replacement_lengths(ss, manual):
    part = manual[100000:230000]
    needles = [b"the", b"then", b"there", b"he", b"here", b"segment"]
    texts = [b"", b"1", b"0123456789abcde", b"0123456789abcdef", b"0123456789abcdefg", b"0123456789abcdefghijklmnopqrstuvwxyzABCD"]
    assert [len(t) for t in texts] == [0, 1, 15, 16, 17, 40]
    want = check_replace(ss, part, needles, texts, "mixed lengths", out_mis=(0, 1, 8, 15))
    by_needle = dict(zip(needles, texts))
    pattern = b"|".join(re.escape(n) for n in sorted(needles, key=len, reverse=True))
    assert want == re.sub(pattern, lambda m: by_needle[m.group(0)], part)
    folded = {n: t for n, t in zip(needles, texts)}
    want = check_replace(ss, part, needles, texts, "mixed lengths, -i -w", ignore_case=True, whole_word=True)
    assert want == re.sub(rb"(?<![0-9A-Za-z_])(?:" + pattern + rb")(?![0-9A-Za-z_])", lambda m: folded[m.group(0).lower()], part, flags=re.I)


@pytest.mark.parametrize("hay_mis", [0, 3, 15])
def test_replace_edges_adjacent_selections_and_misalignments(ss, hay_mis):
    needles, texts = [b"ab", b"abc", b"x"], [b"<two>", b"", b"a long text in place of one x"]
    for host in (b"ab" + b"-" * 50 + b"abc",                           # selections at offset 0 and ending at len
                 b"ababcabxxabc" * 30,                                  # adjacent selections: empty gaps
                 b"abc" * 100,                                          # nothing is left at all
                 b"abcabc" + b"q" * 100,
                 b"x"):
        check_replace(ss, host, needles, texts, (host[:12], hay_mis), hay_mis=hay_mis, out_mis=(0, 1, 8, 15))
    check_replace(ss, b"abc" * 10, [b"abc"], [b""], "an empty output")


def test_replace_where_a_replacement_and_a_gap_straddle_chunk_borders(ss):
    long_text = bytes(65 + k % 26 for k in range(2 * CHUNK + 500))       # straddles two borders
    mid_text = bytes(97 + k % 26 for k in range(300))
    needles, texts = [b"#1", b"#22", b"#"], [mid_text, long_text, b""]
    gap = bytes(48 + k % 10 for k in range(CHUNK - 150))
    host = gap + b"#1" + gap[:200] + b"#" + gap + gap + b"#22" + gap[:77] + b"#1#1" + gap * 2 + b"#22"
    for mis in (0, 1, 15):
        check_replace(ss, host, needles, texts, ("chunk borders", mis), out_mis=(mis,))


def test_replace_without_a_selection_is_a_copy(ss, manual):
    part = manual[5000:150000]
    assert check_replace(ss, part, [b"no such phrase", b"nor this one"], [b"a", b"b"], "copy", hay_mis=7, out_mis=(0, 5)) == part
    assert check_replace(ss, b"", [b"a"], [b"b"], "empty view") == b""


def test_replace_of_a_single_needle_set_equals_the_searchers_replace(ss, d_manual):
    with lm_lib(ss):
        for needle, text in ((b"the", b"THE"), (b"  ", b" "), (b"descriptor", b""), (b"--", b"a much longer text than two hyphens")):
            want = ss.DynamicHipSearcher.new(needle).replace(d_manual, text)
            got = ss.NeedleSet([needle]).replace(d_manual, [text])
            assert torch.equal(got, want) and want.numel() > 1000, needle


def test_the_replace_fixture_rows(ss, d_manual, kat):
    with lm_lib(ss):
        for row in kat["replace"]:
            nset = ss.NeedleSet([n.encode("latin-1") for n in kat["sets"][row["set"]]], ignore_case=row["ignore_case"])
            got = nset.replace(d_manual, [r.encode("latin-1") for r in row["replacements"]], row["whole_word"])
            assert got.numel() == row["length"] and hashlib.sha256(bytes(got.cpu().numpy())).hexdigest() == row["sha256"], row


def test_replace_refusals_write_nothing(ss, d_manual):
    with lm_lib(ss) as L:
        nset, twice = ss.NeedleSet([b"the", b"he"]), ss.NeedleSet([b"the", b"he", b"the"])
        folded = ss.NeedleSet([b"the", b"The"], ignore_case=True)
        buf = torch.full((4096,), SENT8, dtype=torch.uint8, device="cuda")
        part = d_manual[:2000]
        for refused, why in ((lambda: replace_into(ss, L, nset, part, [b"a"], buf, 4096), "1 replacements for a set of 2"),
                             (lambda: replace_into(ss, L, twice, part, [b"a", b"b", b"c"], buf, 4096), "shares its rank"),
                             (lambda: replace_into(ss, L, folded, part, [b"a", b"b"], buf, 4096), "shares its rank"),
                             (lambda: replace_into(ss, L, nset, part, [b"a", b"b"], part[100:], 1000), "intersects the haystack")):
            rc = refused()[0]
            assert rc == ss.SS_ERR_ARGUMENT and why in L.ss_last_error().decode(), (why, L.ss_last_error())
        reps = (ctypes.c_char_p * 2)(None, b"b")
        lens = (ctypes.c_size_t * 2)(3, 1)
        out_len, count = ctypes.c_uint64(77), ctypes.c_uint64(77)
        rc = L.ss_replace_set_device(nset._h, part.data_ptr(), part.numel(), 0, ctypes.cast(reps, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p),
                                     2, torch.cuda.current_stream().cuda_stream, buf.data_ptr(), 4096, ctypes.byref(out_len), ctypes.byref(count))
        assert rc == ss.SS_ERR_ARGUMENT and "is NULL and its length is 3" in L.ss_last_error().decode() and (out_len.value, count.value) == (77, 77)
        assert bool((buf == SENT8).all())
        assert bytes(twice.replace(part, [b"a", b"b", b"a"]).cpu().numpy()) == G.substitute(bytes(part.cpu().numpy()), [b"the", b"he"], [b"a", b"b"])
        with pytest.raises(ValueError):
            nset.replace(part, [b"a"])


# ---- tools/grep_hip.py --------------------------------------------------------------------------------------------------------------
def test_grep_hip_set_forms_against_the_fixture(ss, manual, kat, tmp_path):
    import subprocess
    tool = os.path.join(ROOT, "tools", "grep_hip.py")
    path = os.path.join(GOLDEN, kat["file"])

    def grep(*args):
        ran = subprocess.run([sys.executable, tool] + list(args), capture_output=True, timeout=600)
        assert ran.returncode == 0, ran.stderr[-2000:]
        return ran.stdout

    row = [r for r in kat["rows"] if (r["set"], r["ignore_case"], r["whole_word"]) == (0, True, True)][0]
    needles = [n.encode("latin-1") for n in kat["sets"][0]]
    patterns = [x for n in needles[:3] for x in ("-e", n.decode())]
    rest = tmp_path / "needles.txt"
    rest.write_bytes(b"\n".join(needles[3:]) + b"\n")
    assert int(grep("-o", "--count", "-i", "-w", *patterns, "-f", str(rest), path)) == row["count"] == 8134
    printed = grep("-o", "--offsets", "-i", "-w", *patterns, "-f", str(rest), path)
    want = G.rule(manual, needles, True, True)
    assert printed == b"".join(b"%d:%s\n" % (p, manual[p:p + len(needles[k])]) for p, k in want)      # (what grep -o -b -F -i -w prints)
    plain = grep("--only-matching", "--offsets", *[x for n in kat["sets"][2] for x in ("-e", n)], path)
    assert plain.count(b"\n") == 519 and plain.startswith(b"%d:" % G.rule(manual, [n.encode() for n in kat["sets"][2]])[0][0])
    fixture = kat["replace"][3]
    pairs = tmp_path / "map.txt"
    pairs.write_bytes(b"".join(n.encode("latin-1") + b"\t" + r.encode("latin-1") + b"\n" for n, r in zip(kat["sets"][fixture["set"]], fixture["replacements"])))
    out = grep("--replace-map", str(pairs), "-i", path)
    assert (fixture["ignore_case"], fixture["whole_word"]) == (True, False)
    assert len(out) == fixture["length"] and hashlib.sha256(out).hexdigest() == fixture["sha256"]
