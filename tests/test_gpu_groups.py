"""GPU tests of the grouping calls (include/sliceslice_hip_groups.h, libsliceslice_hip_groups.so) against THE RULE restated in Python
(tests/test_groups_cpu.py: rule_groups) and against tests/golden/groups_kat.json (plain Python).  Every comparison is of integers
and exact; every output array is a window of a larger one whose sentinels on both sides must survive.  The units: 64 ranges per wave,
256 per workgroup, GROUPS_BLOCK = 4,096 per rank block; a key of more than GROUPS_LANE_MAX = 128 bytes is hashed and compared by the
whole wave."""
import collections
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_masked import Arena, Window                                              # noqa: E402
from test_groups_cpu import G, rule_groups                                             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


class _loaded:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def mk_lib(ss):
    """The build under test: the library SLICESLICE_HIP_LIB loaded when it has the entry points, else `ss.groups_build()`."""
    return _loaded() if getattr(ss.lib(), "has_groups", False) else ss.groups_build()


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


@pytest.fixture(scope="module")
def kat():
    return {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "groups_kat.json")))["cases"]}


@pytest.fixture(scope="module")
def words(manual):
    """the manual's \\w+ tokens and what the rule says about them, computed once"""
    spans = np.array(G.ranges(manual, rb"\w+"), dtype=np.int64)
    return spans, rule_groups(manual, spans[:, 0], spans[:, 1], False), rule_groups(manual, spans[:, 0], spans[:, 1], True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64).view(np.int64))).cuda()


def call(ss, view, begin, end, fold=False, weak=False, capacity=None, want=(True, True, True)):
    """one ss_group_ranges_device into sentinel windows: (groups, first window, count window, group window)"""
    b, e = dev(begin), dev(end)
    n = b.numel()
    cap = n + 2 if capacity is None else capacity
    wf, wc, wg = Window(max(cap, 1)), Window(max(cap, 1)), Window(n + 2)
    with mk_lib(ss):
        groups = ss.group_ranges_into(view, b, e, wf.view if want[0] else None, wc.view if want[1] else None, wg.view if want[2] else None,
                                      capacity=cap, ignore_case=fold, weak_hash=weak)
    return groups, wf, wc, wg


def check(ss, view, host, begin, end, fold=False, what=None, weak=(False, True)):
    """the call against the rule, with the real hash and with the weak one"""
    first, count, group = rule_groups(host, begin, end, fold)
    for w in weak:
        groups, wf, wc, wg = call(ss, view, begin, end, fold, w)
        assert groups == first.size, (what, fold, w, groups, first.size)
        wf.check(first, (what, fold, w, "first"))
        wc.check(count, (what, fold, w, "count"))
        wg.check(group, (what, fold, w, "group"))
    return first, count, group


# ---- 1. the manual ---------------------------------------------------------------------------------------------------------------
def test_the_manuals_words_give_the_fixtures_groups(ss, manual, d_manual, kat, words):
    spans, plain, folded = words
    assert spans.shape[0] == kat["word"]["keys"] == 119587 and -(-spans.shape[0] // ss.GROUPS_BLOCK) == 30
    for fold, want, name in ((False, plain, "word"), (True, folded, "word_folded")):
        first, count, group = want
        assert first.size == kat[name]["groups"]
        groups, wf, wc, wg = call(ss, d_manual, spans[:, 0], spans[:, 1], fold)
        assert groups == first.size == {False: 5153, True: 3974}[fold]
        wf.check(first, (name, "first"))
        wc.check(count, (name, "count"))
        wg.check(group, (name, "group"))
        got_f, got_c, got_g = wf.view[:groups].cpu().numpy(), wc.view[:groups].cpu().numpy(), wg.view[:spans.shape[0]].cpu().numpy()
        assert int(got_c.sum()) == spans.shape[0] and (got_g[got_f] == np.arange(groups)).all()
        # ... and the fixture's rows, key by key
        keys = [manual[spans[k, 0]:spans[k, 1]] for k in got_f.tolist()]
        table = [((k.lower() if fold else k), f, c) for k, f, c in zip(keys, got_f.tolist(), got_c.tolist())]
        assert G.digest(table) == kat[name]["sha256"]
        top = int(np.argmax(got_c))
        assert [table[top][0].decode(), table[top][1], table[top][2]] == kat[name]["top"]


def test_the_run_form_returns_the_same_through_one_call(ss, manual, d_manual, kat):
    with mk_lib(ss):
        for name in ("word", "word_folded", "digits", "nonspace"):
            c = kat[name]
            pat = ss.RunPattern(c["pattern"])
            begin, end, count = pat.groups(d_manual, ignore_case=c["folded"])
            b, e, n = begin.cpu().tolist(), end.cpu().tolist(), count.cpu().tolist()
            assert len(b) == c["groups"] and sum(n) == c["keys"], name
            fb, fe = pat.find_all(d_manual)
            want_f, want_c, _ = rule_groups(manual, fb.cpu().numpy(), fe.cpu().numpy(), c["folded"])
            assert b == fb.cpu().numpy()[want_f].tolist() and e == fe.cpu().numpy()[want_f].tolist() and n == want_c.tolist(), name
            keys = [manual[x:y].lower() if c["folded"] else manual[x:y] for x, y in zip(b, e)]
            assert G.digest(list(zip(keys, want_f.tolist(), n))) == c["sha256"], name
            # the sizing call, a capacity below the total and sentinels around the three arrays
            cap = c["groups"] - 3
            wb, we, wc = Window(cap), Window(cap), Window(cap)
            assert pat.groups_into(d_manual, wb.view, we.view, wc.view, cap, c["folded"]) == (c["groups"], c["keys"]), name
            wb.check(b[:cap], name)
            we.check(e[:cap], name)
            wc.check(n[:cap], name)
            assert pat.groups_into(d_manual, None, None, None, 0, c["folded"]) == (c["groups"], c["keys"]), name
            # the vocabulary is printed without a host copy
            text = ss.gather_ranges(d_manual, begin, end, b"\n").cpu().numpy().tobytes()
            assert text == b"".join(manual[x:y] + b"\n" for x, y in zip(b, e)), name
        assert ss.RunPattern(r"\w+").groups(d_manual[:0])[0].numel() == 0
    # a pattern of a build without the grouping refuses and names the build
    with ss.runs_build():
        with pytest.raises(ss.SlicesliceError, match=r"ss\.groups_build\(\)"):
            ss.RunPattern(r"\w+").groups(d_manual)


def test_group_lines_against_the_fixture(ss, manual, d_manual, kat):
    with mk_lib(ss):
        for name in ("lines", "lines_folded"):
            c = kat[name]
            spans = np.array(G.ranges(manual, None), dtype=np.int64)
            first, count, _ = rule_groups(manual, spans[:, 0], spans[:, 1], c["folded"])
            begin, end, number, cnt = (x.cpu().numpy() for x in ss.group_lines(d_manual, ignore_case=c["folded"]))
            assert begin.size == c["groups"] == first.size and int(cnt.sum()) == c["keys"] == spans.shape[0], name
            assert (begin == spans[first, 0]).all() and (end == spans[first, 1]).all() and (number == first + 1).all() and (cnt == count).all(), name
            keys = [manual[x:y].lower() if c["folded"] else manual[x:y] for x, y in zip(begin.tolist(), end.tolist())]
            assert G.digest(list(zip(keys, first.tolist(), cnt.tolist()))) == c["sha256"], name
        # another delimiter, a last line without one, empty lines, an empty view, a view that is one delimiter
        for text, delim, want in ((b"b;a;;b;;a;c", b";", [(0, 1, 1, 2), (2, 3, 2, 2), (4, 4, 3, 2), (10, 11, 7, 1)]),
                                  (b"x\nx\n", b"\n", [(0, 1, 1, 2)]), (b"\n", b"\n", [(0, 0, 1, 1)]), (b"", b"\n", []),
                                  (b"\n\n\nq", b"\n", [(0, 0, 1, 3), (3, 4, 4, 1)]), (b"Ab\naB\nab", b"\n", [(0, 2, 1, 1), (3, 5, 2, 1), (6, 8, 3, 1)])):
            d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda() if text else torch.empty(0, dtype=torch.uint8, device="cuda")
            got = list(zip(*(x.cpu().tolist() for x in ss.group_lines(d, delim))))
            assert got == want, (text, got)
        d = torch.from_numpy(np.frombuffer(b"Ab\naB\nab", dtype=np.uint8).copy()).cuda()
        assert list(zip(*(x.cpu().tolist() for x in ss.group_lines(d, ignore_case=True)))) == [(0, 2, 1, 3)]
        # a delimiter that is an upper-case letter still cuts lines where keys are folded
        d = torch.from_numpy(np.frombuffer(b"xAXAa", dtype=np.uint8).copy()).cuda()
        assert list(zip(*(x.cpu().tolist() for x in ss.group_lines(d, b"A", ignore_case=True)))) == [(0, 1, 1, 2), (4, 5, 3, 1)]


# ---- 2. block borders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_block_borders_with_keys_cycling_through_seven_values(ss, n):
    host = b"zero,one,two,three,four,five,six,"
    spans, at = [], 0
    for w in host.split(b",")[:7]:
        spans.append((at, at + len(w)))
        at += len(w) + 1
    arena = Arena(host)
    begin = [spans[(3 * k) % 7][0] for k in range(n)]
    end = [spans[(3 * k) % 7][1] for k in range(n)]
    first, count, group = check(ss, arena.view(0, len(host))[0], host, begin, end, what=n)
    assert first.size == min(n, 7) and int(count.sum()) == n


# ---- 3. one group, all distinct ----------------------------------------------------------------------------------------------------
def test_one_group_of_seventy_thousand(ss):
    n = 70000
    host = b"ab" * n
    arena = Arena(host)
    view = arena.view(0, len(host))[0]
    # the same range, n times; then n distinct ranges with the same bytes
    for begin in ([4] * n, list(range(0, 2 * n, 2))):
        first, count, group = check(ss, view, host, begin, [b + 2 for b in begin], what="one group")
        assert first.tolist() == [0] and count.tolist() == [n] and not group.any()


def test_all_distinct_three_byte_keys(ss):
    n = 70000
    host = b"".join(bytes([33 + k % 90, 33 + (k // 90) % 90, 33 + k // 8100]) for k in range(n))
    arena = Arena(host)
    begin = [3 * k for k in range(n)]
    first, count, group = check(ss, arena.view(0, len(host))[0], host, begin, [b + 3 for b in begin], what="distinct", weak=(False,))
    assert first.tolist() == list(range(n)) and (count == 1).all() and group.tolist() == list(range(n))


# ---- 4. lengths and alignment ------------------------------------------------------------------------------------------------------
def test_keys_of_every_length_at_every_misalignment(ss):
    lengths = list(range(0, 81)) + [127, 128, 129, 255, 256, 257, 4097]
    rng = np.random.default_rng(5)
    for mis in range(16):
        # every key twice, at two places of different alignment, and a third copy that differs in its last byte
        parts, begin, end, at = [], [], [], 0
        for copy in range(3):
            pad = bytes(rng.integers(1, 255, mis + 3 * copy, dtype=np.uint8))
            parts.append(pad)
            at += len(pad)
            for L in lengths:
                key = bytes((7 * L + 13 * j) % 251 + 1 for j in range(L))
                if copy == 2 and L:
                    key = key[:-1] + bytes([key[-1] ^ 0x40])
                parts.append(key)
                begin.append(at)
                end.append(at + L)
                at += L
        host = b"".join(parts)
        arena = Arena(host)
        first, count, group = check(ss, arena.view(0, len(host))[0], host, begin, end, what=("lengths", mis), weak=(False, True) if mis in (0, 5) else (False,))
        k = len(lengths)
        assert first.size == 2 * k - 1 and count[:k].tolist() == [3] + [2] * (k - 1) and (count[k:] == 1).all()


def test_prefixes_of_each_other_and_two_long_keys_that_differ_in_the_last_byte(ss):
    host = b"a" * 300
    arena = Arena(host)
    begin = [0] * 300 + [300 - L for L in range(1, 301)]
    end = list(range(1, 301)) + [300] * 300
    first, count, group = check(ss, arena.view(0, 300)[0], host, begin, end, what="prefixes")
    assert first.tolist() == list(range(300)) and (count == 2).all()
    # two keys of 1 MiB that differ in the last byte, plus a copy of the first; at three alignments
    MiB = 1 << 20
    rng = np.random.default_rng(9)
    key = rng.integers(0, 256, MiB, dtype=np.uint8)
    other = key.copy()
    other[-1] ^= 1
    host = np.concatenate((np.zeros(3, np.uint8), key, np.zeros(2, np.uint8), other, np.zeros(6, np.uint8), key))
    arena = Arena(host)
    begin = [3, 3 + MiB + 2, 3 + 2 * MiB + 8]
    first, count, group = check(ss, arena.view(0, host.size)[0], host, begin, [b + MiB for b in begin], what="1 MiB")
    assert first.tolist() == [0, 1] and count.tolist() == [2, 1] and group.tolist() == [0, 1, 0]


def test_empty_keys_and_overlapping_repeated_and_descending_ranges(ss):
    host = b"abcabcabcXabcabc"
    arena = Arena(b"##" + host + b"##")
    view = arena.view(2, len(host))[0]
    n = len(host)
    # empty keys at offset 0, at len and clamped from beyond the view; a descending range; an end beyond the view
    begin = [0, n, n + 5, 2 ** 63, 7, 0, 13, 2 ** 64 - 1]
    end = [0, n, n + 9, 2 ** 64 - 1, 3, 3, 2 ** 64 - 1, 2 ** 64 - 1]
    first, count, group = check(ss, view, host, begin, end, what="empty")
    assert first.tolist() == [0, 5] and count.tolist() == [6, 2]
    # every range of the view, in descending order: overlapping and repeated keys, equal bytes at different places
    pairs = [(b, e) for b in range(n, -1, -1) for e in range(n, b - 1, -1)] * 2
    first, count, group = check(ss, view, host, [p[0] for p in pairs], [p[1] for p in pairs], what="every range")
    assert first.size == len({host[b:e] for b, e in pairs})


def test_bytes_outside_the_view_play_no_part(ss):
    # equal keys at both ends of the view; the bytes just outside would make them differ, or - folded - equal to a third key
    for fold in (False, True):
        inner = b"Key" + b"-" * 21 + (b"kEY" if fold else b"Key")
        for left, right in ((b"Q", b"Z"), (b"\xff", b"\x00"), (b"K", b"y")):
            for mis in (0, 1, 3, 13, 15):
                arena = Arena(b"." * mis + left * 16 + inner + right * 16)
                view = arena.view(mis + 16, len(inner))[0]
                n = len(inner)
                begin, end = [0, n - 3, 0, n - 3, n - 2], [3, n, 3, n + 40, 2 ** 63]
                first, count, group = check(ss, view, inner, begin, end, fold, what=("outside", fold, left, mis))
                assert first.tolist() == [0, 4] and count.tolist() == [4, 1]


# ---- 5. the weak hash, determinism, capacity ---------------------------------------------------------------------------------------
def test_the_weak_hash_gives_identical_outputs(ss, d_manual, words):
    spans, plain, folded = words
    for fold, want in ((False, plain), (True, folded)):
        groups, wf, wc, wg = call(ss, d_manual, spans[:, 0], spans[:, 1], fold, weak=True)
        assert groups == want[0].size
        wf.check(want[0], "weak first")
        wc.check(want[1], "weak count")
        wg.check(want[2], "weak group")
    # 5,000 distinct keys of lengths 1 .. 4: one probe chain of 5,000 slots
    keys = [str(k).encode() for k in range(5000)]
    host = b",".join(keys)
    begin = np.cumsum([0] + [len(k) + 1 for k in keys[:-1]])
    end = begin + np.array([len(k) for k in keys])
    arena = Arena(host)
    first, count, group = check(ss, arena.view(0, len(host))[0], host, begin, end, what="5000 distinct")
    assert first.tolist() == list(range(5000))


def test_three_runs_give_equal_outputs(ss, d_manual, words):
    spans = words[0]
    b, e = dev(spans[:, 0]), dev(spans[:, 1])
    with mk_lib(ss):
        runs = [ss.group_ranges(d_manual, b, e, ignore_case=True, want_group=True) for _ in range(3)]
        lines = [ss.group_lines(d_manual) for _ in range(3)]
    for other in runs[1:] + lines[1:]:
        assert all(torch.equal(x, y) for x, y in zip(other, (runs if len(other) == 3 else lines)[0]))


def test_capacities_and_arrays_left_out(ss):
    host = b"".join(b"%d," % (k % 37) for k in range(300))
    begin = np.cumsum([0] + [len(b"%d," % (k % 37)) for k in range(299)])
    end = begin + np.array([len(b"%d" % (k % 37)) for k in range(300)])
    arena = Arena(host)
    view = arena.view(0, len(host))[0]
    first, count, group = rule_groups(host, begin, end)
    groups = first.size
    assert groups == 37
    for cap in (0, 1, groups - 1, groups, groups + 1):
        for want in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, True), (False, False, False),
                     (True, False, False)):
            got, wf, wc, wg = call(ss, view, begin, end, capacity=cap, want=want)
            assert got == groups, (cap, want)
            k = min(cap, groups)
            wf.check(first[:k] if want[0] else [], (cap, want, "first"))
            wc.check(count[:k] if want[1] else [], (cap, want, "count"))
            wg.check(group if want[2] else [], (cap, want, "group"))
    with mk_lib(ss):
        f, c = ss.group_ranges(view, begin, end, capacity=5)
        assert f.cpu().tolist() == first[:5].tolist() and c.cpu().tolist() == count[:5].tolist()
        f, c, g = ss.group_ranges(view, begin.tolist(), end.tolist(), want_group=True)
        assert f.cpu().tolist() == first.tolist() and c.cpu().tolist() == count.tolist() and g.cpu().tolist() == group.tolist()
        assert [x.numel() for x in ss.group_ranges(view, [], [], want_group=True)] == [0, 0, 0]


# ---- 6. NOCASE -------------------------------------------------------------------------------------------------------------------
def test_only_ascii_letters_fold(ss):
    # the bytes next to the letter ranges and their bit-7 twins: '@' 'A' 'Z' '[' '`' 'a' 'z' '{', each also with bit 7 set
    near = [0x40, 0x41, 0x5a, 0x5b, 0x60, 0x61, 0x7a, 0x7b]
    alphabet = bytes(near + [b | 0x80 for b in near])
    rng = np.random.default_rng(11)
    keys = [bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), int(L))) for L in rng.integers(1, 7, 4000)]
    keys += [bytes([b]) for b in alphabet] + [bytes([b]) * 5 for b in alphabet]
    host = b"".join(keys)
    end = np.cumsum([len(k) for k in keys])
    begin = end - np.array([len(k) for k in keys])
    arena = Arena(host)
    for fold in (False, True):
        first, count, group = check(ss, arena.view(0, len(host))[0], host, begin, end, fold, what=("nocase", fold), weak=(False,))
    single = {bytes([b]): int(group[4000 + k]) for k, b in enumerate(alphabet)}
    assert single[b"A"] == single[b"a"] and single[b"Z"] == single[b"z"] and len(set(single.values())) == 14
    assert len({single[bytes([b])] for b in (0x40, 0x60, 0x5b, 0x7b, 0xc1, 0xe1, 0xda, 0xfa)}) == 8


# ---- 7. the Python and the tool layer ----------------------------------------------------------------------------------------------
def test_most_common_ties_are_in_first_occurrence_order(ss, manual, d_manual):
    counter = collections.Counter(re.findall(rb"\w+", manual))
    with mk_lib(ss):
        pat = ss.RunPattern(r"\w+")
        for k in (1, 10, 500, 5153, 6000, None):
            begin, end, count = pat.most_common(d_manual, k)
            got = [(manual[b:e], c) for b, e, c in zip(begin.cpu().tolist(), end.cpu().tolist(), count.cpu().tolist())]
            assert got == counter.most_common(k), k
        folded = collections.Counter(w.lower() for w in re.findall(rb"\w+", manual))
        begin, end, count = pat.most_common(d_manual, 50, ignore_case=True)
        assert [(manual[b:e].lower(), c) for b, e, c in zip(begin.cpu().tolist(), end.cpu().tolist(), count.cpu().tolist())] == folded.most_common(50)
        d = torch.from_numpy(np.frombuffer(b"b a c a b c d", dtype=np.uint8).copy()).cuda()
        begin, end, count = pat.most_common(d, 3)
        assert (begin.cpu().tolist(), count.cpu().tolist()) == ([0, 2, 4], [2, 2, 2])


def test_more_groups_than_the_first_call_makes_room_for(ss):
    # 70,000 distinct tokens, one per line, each twice: the wrappers' first call has room for 65,536 rows and a second one follows
    n = 70000
    host = b"".join(b"%d\n" % k for k in range(n)) * 2
    d = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).cuda()
    want = [b"%d" % k for k in range(n)]
    with mk_lib(ss):
        begin, end, count = (x.cpu().tolist() for x in ss.RunPattern(r"[0-9]+").groups(d))
        assert [host[b:e] for b, e in zip(begin, end)] == want and count == [2] * n
        begin, end, number, count = (x.cpu().tolist() for x in ss.group_lines(d))
        assert [host[b:e] for b, e in zip(begin, end)] == want and count == [2] * n and number == list(range(1, n + 1))


def _tool(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out.stdout


def test_the_tool_prints_what_the_counter_holds(ss, manual):
    path = os.path.join(GOLDEN, "data", "i386.txt")
    counter = collections.Counter(re.findall(rb"\w+", manual))
    want = b"".join(b"%d\t%s\n" % (c, w) for w, c in counter.items())
    assert _tool("--runs", r"\w+", "--uniq-count", path) == want
    assert _tool("--runs", r"\w+", "--uniq-count", "--device-output", path) == want
    folded = collections.Counter(w.lower() for w in re.findall(rb"\w+", manual))
    got = _tool("--runs", r"\w+", "--uniq-count", "-i", "--top", "5", "--device-output", path).splitlines()
    assert [(int(l.split(b"\t")[0]), l.split(b"\t")[1].lower()) for l in got] == [(c, w) for w, c in folded.most_common(5)]
    lines = manual.split(b"\n")[:-1]
    assert _tool("--uniq", path) == b"".join(l + b"\n" for l in dict.fromkeys(lines))
    by_line = collections.Counter(lines)
    assert _tool("--lines-uniq-count", "--top", "3", "--device-output", path) == b"".join(b"%d\t%s\n" % (c, l) for l, c in by_line.most_common(3))


def test_a_capturing_stream_is_refused_and_the_results_are_left_alone(ss, d_manual):
    import ctypes
    with mk_lib(ss):
        L = ss.lib()
        b, e = dev([0, 4]), dev([3, 7])
        groups, other = ctypes.c_uint64(77), ctypes.c_uint64(78)
        w = Window(4)
        assert ss.group_ranges_into(d_manual, b, e, None, None) == 2 and ss.group_lines(d_manual[:100])[0].numel() > 0     # (first use outside the capture)
        pat = ss.RunPattern(r"\w+")
        probe = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            probe.fill_(7)                                                          # (something to capture: the refused calls add nothing)
            st = torch.cuda.current_stream().cuda_stream
            rc1 = L.ss_group_ranges_device(d_manual.data_ptr(), 100, b.data_ptr(), e.data_ptr(), 2, 0, st, w.view.data_ptr(), None, 4, None, ctypes.byref(groups))
            m1 = L.ss_last_error().decode()
            rc2 = L.ss_group_lines_device(d_manual.data_ptr(), 100, 10, 0, st, w.view.data_ptr(), None, None, None, 4, ctypes.byref(groups), ctypes.byref(other))
            m2 = L.ss_last_error().decode()
            rc3 = L.ss_group_runs_device(pat._h, d_manual.data_ptr(), 100, 0, st, w.view.data_ptr(), None, None, 4, ctypes.byref(groups), ctypes.byref(other))
            m3 = L.ss_last_error().decode()
        assert rc1 == rc2 == rc3 == ss.SS_ERR_ARGUMENT and all("cannot be captured" in m for m in (m1, m2, m3)), (m1, m2, m3)
        assert (groups.value, other.value) == (77, 78)
        w.check([], "a capturing stream writes nothing")
