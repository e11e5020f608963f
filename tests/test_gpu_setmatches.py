"""GPU tests of the occurrence calls of a needle set (include/sliceslice_hip_setmatches.h, libsliceslice_hip_setmatches.so):
ss_needle_set_ranks, ss_count_set_device / _async and ss_find_all_set_device against the rule restated on Python bytes, against
arithmetic where the text is uniform, against `count` / `find_all` of one searcher per needle of the SAME build merged by
(offset, rank), and against tests/golden/bounded_kat.json.  Every comparison is of integers and exact; every output array is a
window of a larger one whose sentinels on both sides must survive.  The manual's text aside, no view is larger than three workgroups;
views of more than one chunk of 256 workgroups are tests/test_gpu_set_grids.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PART = 128 * 1024                       # bytes of the view per workgroup, from the aligned address below the view
GUARD = 8
SENT64, SENT32 = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B
_WORD = np.zeros(256, dtype=bool)
_WORD[list(b"0123456789_") + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B))] = True


@pytest.fixture(scope="module")
def ss():
    import sliceslice_rs_amd as m
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    with set_lib(m):
        pass
    return m


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def set_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.setmatches_build()`."""
    return _loaded() if getattr(ss.lib(), "has_setmatches", False) else ss.setmatches_build()


class Window:
    """`cap` slots inside a larger device array filled with a sentinel"""
    def __init__(self, cap, dtype=torch.int64):
        self.sent = SENT64 if dtype == torch.int64 else SENT32
        self.buf = torch.full((cap + 2 * GUARD,), self.sent, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + cap]

    def check(self, want, what):
        """the first len(want) slots hold `want`, every other slot of the larger array the sentinel"""
        h = self.buf.cpu().numpy()
        k = len(want)
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + k:] == self.sent).all(), what
        assert (h[GUARD:GUARD + k] == np.asarray(want, dtype=h.dtype)).all(), (what, h[GUARD:GUARD + min(k, 8)], want[:8])


def dev_view(host, mis=0):
    """the bytes of `host` on the device at 16-byte misalignment `mis`, inside a buffer of hostile bytes"""
    host = np.frombuffer(bytes(host), dtype=np.uint8) if isinstance(host, (bytes, bytearray)) else np.asarray(host, dtype=np.uint8)
    buf = torch.full((host.size + 64,), ord("a"), dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + 16 + mis
    view = buf[at:at + host.size]
    if host.size:
        view.copy_(torch.from_numpy(host.copy()))
    assert host.size == 0 or view.data_ptr() % 16 == mis
    return view


def occurrences(hb, nd):
    out, at = [], hb.find(nd)
    while at >= 0:
        out.append(at)
        at = hb.find(nd, at + 1)
    return np.asarray(out, dtype=np.int64)


def distinct(needles, nocase=False):
    return sorted(set(bytes(n).lower() if nocase else bytes(n) for n in needles))


def rule(host, needles, nocase=False, word=False):
    """(counts per rank, offsets, ranks) by the rule of the header, on Python bytes"""
    host = np.asarray(host, dtype=np.uint8)
    hb = host.tobytes()
    if nocase:
        hb = hb.lower()
    ds = distinct(needles, nocase)
    offs, ranks, counts = [], [], np.zeros(len(ds), dtype=np.int64)
    for r, nd in enumerate(ds):
        o = occurrences(hb, nd)
        if word and o.size:
            keep = np.ones(o.size, dtype=bool)
            for at in (o - 1, o + len(nd)):
                keep &= (at < 0) | (at >= host.size) | ~_WORD[host[np.clip(at, 0, host.size - 1)]]
            o = o[keep]
        counts[r] = o.size
        offs.append(o)
        ranks.append(np.full(o.size, r, dtype=np.int64))
    offs, ranks = np.concatenate(offs), np.concatenate(ranks)
    order = np.lexsort((ranks, offs))
    return counts, offs[order], ranks[order]


def given_ranks(needles, nocase=False):
    rank_of = {nd: r for r, nd in enumerate(distinct(needles, nocase))}
    return np.asarray([rank_of[bytes(n).lower() if nocase else bytes(n)] for n in needles], dtype=np.int64)


def check_set(ss, needles, dev, want, nocase=False, word=False, what=None, caps=None, made=None):
    """every call of the set on `dev` against want = (counts per rank, offsets, ranks)"""
    counts, offs, ranks = want
    what = (what, nocase, word)
    with set_lib(ss):
        st = made or ss.NeedleSet(needles, ignore_case=nocase)
    gr = given_ranks(needles, nocase)
    assert (st.ranks() == gr).all() and st.info()["distinct"] == counts.size, what
    total = int(counts.sum())
    assert st.count_total(dev, whole_word=word) == total, what
    got = st.count(dev, whole_word=word).cpu().numpy()
    assert got.dtype == np.int64 and (got == counts[gr]).all(), (what, got[:8], counts[gr][:8])
    # the async form: bins and total, then each alone, all inside windows
    wc, wt = Window(counts.size), Window(1)
    st.count_async(dev, wc.view, wt.view, whole_word=word)
    torch.cuda.synchronize()
    wc.check(counts, (what, "async bins"))
    wt.check([total], (what, "async total"))
    wc, wt = Window(counts.size), Window(1)
    st.count_async(dev, wc.view, None, whole_word=word)
    st.count_async(dev, None, wt.view, whole_word=word)
    torch.cuda.synchronize()
    wc.check(counts, (what, "async bins alone"))
    wt.check([total], (what, "async total alone"))
    for cap in (caps if caps is not None else sorted({0, 1, total // 2, max(total - 1, 0), total, total + 5})):
        wo, wr = Window(cap), Window(cap, torch.int32)
        assert st.find_all_into(dev, wo.view if cap else None, wr.view if cap else None, cap, whole_word=word) == total, (what, cap)
        k = min(cap, total)
        wo.check(offs[:k], (what, cap, "offsets"))
        wr.check(ranks[:k], (what, cap, "ranks"))
    o, idx = st.find_all(dev, whole_word=word)
    first = np.full(counts.size, len(needles), dtype=np.int64)
    np.minimum.at(first, gr, np.arange(len(needles)))
    assert (o.cpu().numpy() == offs).all() and (idx.cpu().numpy() == first[ranks]).all(), what
    return st


def test_only_the_setmatches_library_has_the_entry_points(ss):
    assert not getattr(ss.lib(), "has_setmatches", False)
    with ss.needleset_build() as L:
        assert not L.has_setmatches
        old = ss.NeedleSet([b"abc"])
    with ss.setmatches_build() as L:
        assert L.has_setmatches and L.has_needleset and L.has_anyof and L.has_matches and not L.has_matches_batched
    for call in (old.ranks, lambda: old.count(dev_view(b"abc")), lambda: old.count_total(dev_view(b"abc")),
                 lambda: old.find_all(dev_view(b"abc")), lambda: old.find_all_into(dev_view(b"abc"), None, None, 0),
                 lambda: old.count_async(dev_view(b"abc"), None, torch.zeros(1, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ss.SlicesliceError, match="setmatches_build") as e:
            call()
        assert e.value.code == ss.SS_ERR_ARGUMENT


# ---- borders ------------------------------------------------------------------------------------------------------------------------
BORDER_NEEDLES = [b"q", b"rs", b"tuv", b"abcdef", b"ghijklm", b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789!#$%"]
BORDERS = (16, 1024, 4096, 16 * 1024, PART)        # lane, piece, wave run, tile, workgroup: in bytes of the aligned stream


@pytest.mark.parametrize("mis", [0, 1, 15])
def test_needles_start_at_every_offset_around_every_kind_of_border(ss, mis):
    size = 260 * 1024
    assert [len(n) for n in BORDER_NEEDLES] == [1, 2, 3, 6, 7, 40]
    # every (border kind, needle, start) once: the needle starts at stream position border + s, s = -(n - 1) .. 0
    todo = [(kind, r, s) for kind in BORDERS for r, nd in enumerate(BORDER_NEEDLES) for s in range(-(len(nd) - 1), 1)]
    with set_lib(ss):
        st = ss.NeedleSet(BORDER_NEEDLES)
    ds = distinct(BORDER_NEEDLES)
    rounds = 0
    while todo:
        rounds += 1
        host = np.full(size, ord("."), dtype=np.uint8)
        used = np.zeros(size, dtype=bool)
        planted, later, next_border = [], [], {kind: kind for kind in BORDERS}
        for kind, r, s in todo:
            nd = BORDER_NEEDLES[r]
            border, at = next_border[kind], None
            while border + len(nd) + 1 < size + mis:
                at = border + s - mis                           # the hay index
                if at >= 1 and not used[at - 1:at + len(nd) + 1].any():
                    break
                border, at = border + kind, None
            if at is None:
                later.append((kind, r, s))
                continue
            next_border[kind] = border + kind if kind > 16 else border + 16 * 4
            host[at:at + len(nd)] = np.frombuffer(nd, dtype=np.uint8)
            used[at:at + len(nd)] = True
            planted.append((at, ds.index(nd)))
        assert planted and len(later) < len(todo)
        todo = later
        want = rule(host, BORDER_NEEDLES)
        assert sorted(planted) == sorted(zip(want[1].tolist(), want[2].tolist()))     # each needle once, at its place
        check_set(ss, BORDER_NEEDLES, dev_view(host, mis), want, what=("borders", mis, rounds), caps=(len(planted),), made=st)
    assert rounds <= 40


# ---- dense pairs --------------------------------------------------------------------------------------------------------------------
def test_four_pairs_at_every_position_and_the_capacity_cuts(ss):
    n = 132 * 1024
    needles = [b"a", b"aa", b"aaa", b"aaaaaaa"]
    lens = np.asarray([1, 2, 3, 7])
    counts = n - lens + 1                                       # arithmetic
    offs, ranks = np.repeat(np.arange(n, dtype=np.int64), 4), np.tile(np.arange(4, dtype=np.int64), n)
    keep = offs + lens[ranks] <= n
    offs, ranks = offs[keep], ranks[keep]
    total = int(counts.sum())
    assert total == offs.size == 4 * n - 9
    dev = dev_view(np.full(n, ord("a"), dtype=np.uint8))
    first = 4 * (PART - dev.data_ptr() % 16)                    # the pairs of the first workgroup: more than 2^16
    assert first > 1 << 16
    st = check_set(ss, needles, dev, (counts, offs, ranks), what="dense",
                   caps=(0, 1, 17, first - 1, first, first + 1, total - 1, total, total + 5))
    # each of the two arrays left out in turn
    wo, wr = Window(total), Window(total, torch.int32)
    assert st.find_all_into(dev, wo.view, None, total) == total and st.find_all_into(dev, None, wr.view, total) == total
    wo.check(offs, "offsets alone")
    wr.check(ranks, "ranks alone")
    wo = Window(17)
    assert st.find_all_into(dev, wo.view, None, 17) == total
    wo.check(offs[:17], "offsets alone, cut")


# ---- prefixes, duplicates, the fold -------------------------------------------------------------------------------------------------
def two_letter_words():
    """the text of tests/test_gpu_needleset.py, rebuilt, with a tail of bytes next to the letter ranges and their bit-7 twins"""
    rng = np.random.default_rng(22)
    tokens = [b"ab", b"ba", b"bb", b"aa", b"abba", b"a_b"]
    parts = []
    for t, sep in zip(rng.integers(0, len(tokens), 9000), rng.choice([b" ", b"\n", b"-"], 9000, p=[0.6, 0.3, 0.1])):
        parts += [tokens[t], sep]
    tokens += [b"AB", b"Abb", b"aBBa", b"abb", b"ABBA"]          # ... and a stretch in both cases
    for t, sep in zip(rng.integers(0, len(tokens), 1500), rng.choice([b" ", b"\n", b"-"], 1500, p=[0.6, 0.3, 0.1])):
        parts += [tokens[t], sep]
    for x in (0x40, 0x5B, 0x60, 0x7B, 0xC1, 0xE1, 0xC2, 0xE2, 0x2F, 0x3A, 0x5F, 0x80):
        b = bytes([x])
        parts += [b, b"ab", b, b" ", b"ab", b, b"b ", b, b"abba ", bytes([0x41 | 0x80, 0x62]), b" ", bytes([0x61, 0x42 | 0x80]), b" a", bytes([x & 0x7F | 0x20]), b" "]
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


@pytest.mark.parametrize("nocase", [False, True])
@pytest.mark.parametrize("word", [False, True])
def test_prefixes_duplicates_and_the_fold_against_one_searcher_per_needle(ss, nocase, word):
    needles = [b"ab", b"abb", b"abba", b"ab", b"AB"]
    host = two_letter_words()
    dev = dev_view(host, 3)
    want = rule(host, needles, nocase, word)
    assert want[0].min() > 0 or not nocase
    st = check_set(ss, needles, dev, want, nocase, word, what="prefixes")
    got = st.count(dev, whole_word=word).cpu().numpy()
    assert got[0] == got[3] and (not nocase or got[4] == got[0])                # duplicates show equal values
    # ... and against the per-needle calls of the same build, merged by (offset, rank)
    gr = given_ranks(needles, nocase)
    offs, ranks = [], []
    with set_lib(ss):
        for k, nd in enumerate(needles):
            s = ss.DynamicHipSearcher.new_nocase(nd.lower()) if nocase else ss.DynamicHipSearcher(nd)
            assert s.count(dev, ignore_case=nocase, whole_word=word) == got[k], (k, nd)
            if list(gr).index(gr[k]) == k:                                      # (each rank once)
                o = s.find_all(dev, ignore_case=nocase, whole_word=word).cpu().numpy()
                offs.append(o)
                ranks.append(np.full(o.size, gr[k], dtype=np.int64))
    offs, ranks = np.concatenate(offs), np.concatenate(ranks)
    order = np.lexsort((ranks, offs))
    assert (offs[order] == want[1]).all() and (ranks[order] == want[2]).all()


# ---- both routes of the histogram ---------------------------------------------------------------------------------------------------
def test_more_needles_than_bins_and_short_needles_beside_them(ss):
    letters = np.frombuffer(b"abcdefghijklmnopq", dtype=np.uint8)
    rng = np.random.default_rng(23)
    n = 132 * 1024
    code = rng.integers(0, 17, n)
    host = letters[code]
    dev = dev_view(host, 5)
    three = [bytes(letters[[a, b, c]]) for a in range(17) for b in range(17) for c in range(17)]         # in rank order
    key3 = code[:-2] * 289 + code[1:-1] * 17 + code[2:]
    want3 = np.bincount(key3, minlength=4913)
    perm = rng.permutation(4913)
    with set_lib(ss):
        st = ss.NeedleSet([three[k] for k in perm])
    assert st.info()["distinct"] == 4913 > 4096 and (st.ranks() == perm).all()
    assert (st.count(dev).cpu().numpy() == want3[perm]).all() and st.count_total(dev) == n - 2
    wo, wr = Window(n - 2), Window(n - 2, torch.int32)
    assert st.find_all_into(dev, wo.view, wr.view, n - 2) == n - 2
    wo.check(np.arange(n - 2), "three-byte offsets")
    wr.check(key3, "three-byte ranks")
    # the same set with 200 one- and two-byte needles added: every pair of letters but 89 of them, and 11 single letters
    two = [bytes(letters[[a, b]]) for a in range(17) for b in range(17)]
    short = [two[k] for k in rng.permutation(289)[:189]] + [bytes(letters[[a]]) for a in rng.permutation(17)[:11]]
    assert len(short) == 200
    needles = short + three
    ds = distinct(needles)
    rank_of = {nd: r for r, nd in enumerate(ds)}
    offs, ranks = [np.arange(n - 2)], [np.asarray([rank_of[t] for t in three])[key3]]
    has2 = np.asarray([rank_of.get(t, -1) for t in two])
    r2 = has2[code[:-1] * 17 + code[1:]]
    offs.append(np.flatnonzero(r2 >= 0))
    ranks.append(r2[r2 >= 0])
    has1 = np.asarray([rank_of.get(bytes(letters[[a]]), -1) for a in range(17)])
    r1 = has1[code]
    offs.append(np.flatnonzero(r1 >= 0))
    ranks.append(r1[r1 >= 0])
    offs, ranks = np.concatenate(offs), np.concatenate(ranks)
    order = np.lexsort((ranks, offs))
    counts = np.bincount(ranks, minlength=len(ds))
    total = offs.size
    check_set(ss, needles, dev, (counts, offs[order], ranks[order]), what="both routes", caps=(total,))


# ---- ends ---------------------------------------------------------------------------------------------------------------------------
def test_the_ends_of_the_view(ss):
    needles = [b"ab", b"abc", b"c", b"abcabcabc", b"bca"]
    with set_lib(ss):
        st = ss.NeedleSet(needles)
    # the view inside a buffer whose bytes around it are needle copies and word bytes
    around = np.frombuffer(b"abcabcabcabcabcabcabcabc", dtype=np.uint8)
    for body in (b"", b"c", b"a", b"ab", b"bc", b"abc", b" abc", b"abc ", b"abcabcabc", b"abcabcab", b"xabcabcabc", b" ab abc c ", b"ab" * 9, b"-c-"):
        host = np.frombuffer(body, dtype=np.uint8)
        wide = np.concatenate([around, host, around])
        for mis in (0, 7, 15):
            dev = dev_view(wide, (mis + 16 - around.size % 16) % 16)[around.size:around.size + host.size]
            for word in (False, True):
                want = rule(host, needles, False, word)
                if host.size:
                    assert dev.data_ptr() % 16 == mis
                check_set(ss, needles, dev, want, False, word, what=("ends", body, mis), caps=(int(want[0].sum()), int(want[0].sum()) + 3), made=st)
    # a needle flush against len and one byte beyond it, far from the start of the last workgroup
    host = np.full(PART + 300, ord("."), dtype=np.uint8)
    host[-9:] = np.frombuffer(b"abcabcabc", dtype=np.uint8)
    dev = dev_view(np.concatenate([host, around]), 0)
    for cut in (0, 1, 2, 9):
        view = dev[:host.size - cut]
        check_set(ss, needles, view, rule(host[:host.size - cut], needles), what=("flush", cut), made=st)


# ---- the manual's text --------------------------------------------------------------------------------------------------------------
def test_the_word_list_as_one_set_on_the_manual(ss, corpus):
    kat = json.load(open(os.path.join(GOLDEN, "bounded_kat.json")))["table"]
    words = [w for w in corpus["words"] if w]
    assert len(words) == 4585
    host = np.frombuffer(corpus["i386"], dtype=np.uint8)
    dev = dev_view(host)
    with set_lib(ss):
        st = ss.NeedleSet(words)
        folded = ss.NeedleSet(words, ignore_case=True)
        got = st.count(dev).cpu().numpy()
        loop = np.asarray([ss.DynamicHipSearcher(w).count(dev) for w in words])
    assert (got == loop).all(), np.flatnonzero(got != loop)[:8]
    by_word = st.count(dev, whole_word=True).cpu().numpy()
    nocase_word = folded.count(dev, whole_word=True).cpu().numpy()
    for w, (plain, as_word) in {b"the": (7398, 6524), b"descriptor": (355, 286), b"intel": (5, 1)}.items():
        k = words.index(w)
        t = kat[w.decode()]
        assert (t["count"], t["word_count"]) == (plain, as_word)
        assert got[k] == plain and by_word[k] == as_word, (w, got[k], by_word[k])
        assert nocase_word[k] == t["word_count_nocase"], (w, nocase_word[k])
    assert nocase_word[words.index(b"intel")] == 37
    # the sum over the DISTINCT needles is the number of pairs, and the pairs are ordered
    distinct_total = int(got[np.unique(st.ranks(), return_index=True)[1]].sum())
    assert st.count_total(dev) == distinct_total
    o, idx = st.find_all(dev)
    o, idx = o.cpu().numpy(), idx.cpu().numpy()
    assert o.size == distinct_total and (np.diff(o) >= 0).all()
    r = st.ranks()[idx]
    same = np.diff(o) == 0
    assert (np.diff(r)[same] > 0).all()
    assert (np.bincount(r, minlength=st.info()["distinct"])[st.ranks()] == got).all()
    # every 40th word as a word and ignoring case, against the per-needle calls
    with set_lib(ss):
        for k in range(0, len(words), 40):
            assert ss.DynamicHipSearcher(words[k]).count(dev, whole_word=True) == by_word[k], words[k]
            assert ss.DynamicHipSearcher.new_nocase(words[k].lower()).count(dev, ignore_case=True, whole_word=True) == nocase_word[k], words[k]


def _grep(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True, text=True)


def test_grep_hip_frequencies_prints_what_count_prints(ss):
    manual = os.path.join(GOLDEN, "data", "i386.txt")
    patterns = ["-e", "the", "-e", "descriptor", "-e", "intel", "-e", "the"]
    table, counts = _grep("--frequencies", *patterns, manual), _grep("--count", *patterns, manual)
    assert table.returncode == 0 and counts.returncode == 0, (table.stderr[-500:], counts.stderr[-500:])
    assert table.stdout == counts.stdout == "7398\n355\n5\n7398\n"                  # byte for byte, a pattern given twice included
    assert _grep("--frequencies", "-i", "--word-regexp", *patterns, manual).stdout == "7755\n393\n37\n7755\n"


# ---- the async form in a graph ------------------------------------------------------------------------------------------------------
def test_the_async_count_is_captured_and_replayed_and_two_runs_agree(ss):
    host = two_letter_words()
    needles = [b"ab", b"abb", b"abba", b"bb", b"a", b"b a"]
    dev = dev_view(host, 9)
    counts, offs, ranks = rule(host, needles)
    with set_lib(ss):
        st = ss.NeedleSet(needles)
    wc, wt = Window(counts.size), Window(1)
    st.count_async(dev, wc.view, wt.view)                       # (first use outside the capture)
    torch.cuda.synchronize()
    wc.check(counts, "before the capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.count_async(dev, wc.view, wt.view)
    wc.view.fill_(7)
    wt.view.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    wc.check(counts, "replayed bins")
    wt.check([int(counts.sum())], "replayed total")
    # two runs give identical arrays
    runs = []
    for _ in range(2):
        o, r = Window(offs.size), Window(offs.size, torch.int32)
        st.find_all_into(dev, o.view, r.view, offs.size)
        runs.append((o.buf.cpu().numpy(), r.buf.cpu().numpy(), st.count(dev).cpu().numpy()))
    assert all((a == b).all() for a, b in zip(*runs))
    # the waiting calls refuse a capturing stream and write nothing
    g2 = torch.cuda.CUDAGraph()
    probe = torch.zeros(1, dtype=torch.int64, device="cuda")
    errs = []
    o = Window(4)
    with torch.cuda.graph(g2):
        probe.fill_(7)
        for call in (lambda: st.count_total(dev), lambda: st.find_all_into(dev, o.view, None, 4)):
            try:
                call()
            except ss.SlicesliceError as x:
                errs.append(x)
    torch.cuda.synchronize()
    assert len(errs) == 2 and all(e.code == ss.SS_ERR_ARGUMENT and "hipGraph" in str(e) for e in errs), errs
    assert "ss_count_set_device" in str(errs[0]) and "ss_find_all_set_device" in str(errs[1])
    o.check([], "refused while capturing")
    assert st.count_total(dev) == int(counts.sum())             # and the calls work as before afterwards


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_alone(ss):
    import ctypes
    dev = dev_view(b"ab abc AB")
    with set_lib(ss):
        L = ss.lib()
        st = ss.NeedleSet([b"ab", b"abc"])
        folded = ss.NeedleSet([b"ab"], ignore_case=True)
        empty = ss.NeedleSet([b"ab", b""])
    assert (empty.ranks() == [1, 0]).all()                      # (the ranks of such a set are still told)
    bins, tot, offs, rk = Window(2), Window(1), Window(4), Window(4, torch.int32)
    total = ctypes.c_uint64(77)

    def calls(s, how, hay=dev.data_ptr(), n=dev.numel()):
        return [("ss_count_set_device", lambda: L.ss_count_set_device(s, hay, n, how, None, bins.view.data_ptr(), ctypes.byref(total))),
                ("ss_count_set_device_async", lambda: L.ss_count_set_device_async(s, hay, n, how, None, bins.view.data_ptr(), tot.view.data_ptr())),
                ("ss_find_all_set_device", lambda: L.ss_find_all_set_device(s, hay, n, how, None, offs.view.data_ptr(), rk.view.data_ptr(), 4, ctypes.byref(total)))]

    refused = [("SS_BOUND_LINE", calls(st._h, ss.searcher.SS_BOUND_LINE)), ("SS_CONTEXT_INVERT", calls(st._h, ss.SS_CONTEXT_INVERT)),
               ("bits other than", calls(st._h, 64)), ("SS_BOUND_NOCASE", calls(st._h, ss.searcher.SS_BOUND_NOCASE)),
               ("SS_BOUND_NOCASE", calls(folded._h, 0)), ("empty needle", calls(empty._h, 0)), ("set is NULL", calls(None, 0)),
               ("haystack is NULL", calls(st._h, 0, None, 5))]
    for word, group in refused:
        for name, call in group:
            assert call() == ss.SS_ERR_ARGUMENT, (word, name)
            msg = L.ss_last_error().decode()
            assert word in msg and name in msg, (word, name, msg)
    assert L.ss_count_set_device_async(st._h, dev.data_ptr(), dev.numel(), 0, None, None, None) == ss.SS_ERR_ARGUMENT
    assert "both NULL" in L.ss_last_error().decode()
    assert L.ss_count_set_device(st._h, dev.data_ptr(), dev.numel(), 0, None, None, None) == ss.SS_ERR_ARGUMENT
    assert L.ss_find_all_set_device(st._h, dev.data_ptr(), dev.numel(), 0, None, None, None, 0, None) == ss.SS_ERR_ARGUMENT
    assert L.ss_needle_set_ranks(None, None) == ss.SS_ERR_ARGUMENT
    torch.cuda.synchronize()
    for w in (bins, tot, offs, rk):
        w.check([], "refused")
    assert total.value == 77
    # a NULL haystack with len == 0 is no error, and SS_BOUND_NOCASE that equals the fold is accepted
    assert L.ss_count_set_device(st._h, None, 0, 0, None, bins.view.data_ptr(), ctypes.byref(total)) == ss.searcher.SS_OK and total.value == 0
    bins.check([0, 0], "len 0")
    assert L.ss_count_set_device(folded._h, dev.data_ptr(), dev.numel(), ss.searcher.SS_BOUND_NOCASE, None, None, ctypes.byref(total)) == ss.searcher.SS_OK
    assert total.value == 3
    if torch.cuda.device_count() > 1:                           # a set of another device
        with torch.cuda.device(1):
            assert L.ss_count_set_device(st._h, dev.data_ptr(), dev.numel(), 0, None, None, ctypes.byref(total)) == ss.SS_ERR_ARGUMENT
            assert "device" in L.ss_last_error().decode()
