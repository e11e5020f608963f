"""The sparse reference of tests/_set_sparse.py against the dense rules of the suite, on real arrays of a few KiB: the scene kinds
that tests/test_gpu_set_grids.py plants into 200 MB, built here at 64 and at 200 bytes per part with chunks of four parts.  For
every pattern below the spans and the lines worked out from the scene list alone must equal what rule_offsets / rule_lines of
tests/test_masked_cpu.py and tests/test_classes_cpu.py, rule_runs / rule_lines of tests/test_runs_cpu.py, and `rule` of
tests/test_gpu_setmatches.py (with tests/test_gpu_needleset.py's lines_with_any) give on the array.  The geometry the helper
restates is read from the kernels' headers, and the two GPU shapes are checked from their scene lists.  No GPU.

PATTERNS is also what tests/test_gpu_set_grids.py searches for."""
import os
import re

import numpy as np

import test_classes_cpu as C
import test_masked_cpu as M
import test_runs_cpu as R
from _set_sparse import (BORDERS_B, CHUNK, DELIM, END_A, FILLER, KINDS, LEN_B, LONG_B, LONG_LINE, NL, ROTATIONS, THREADS, WG, Kit, Parts,
                         border_scenes, buffer_scenes, delimiters, grid_scenes, shape_a, shape_b, sparse_gaps, sparse_lines, sparse_spans,
                         view_scenes, write_scenes)
from test_gpu_needleset import lines_with_any
from test_gpu_setmatches import distinct, rule as set_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
_WORDS = [w for w in open(os.path.join(ROOT, "tests", "golden", "data", "words.txt"), "rb").read().split() if w.isalpha()]
THREE = [w for w in _WORDS if 4 <= len(w) <= 5][50::400]                            # a sparse set: Base, link, swaps
_MID = [w for w in _WORDS if 4 <= len(w) <= 9]
FORTY = _MID[7::len(_MID) // 40][:40] + [b"instruction", b"instructions"]           # ... and a needle that is a prefix of another
WORD = C.sets_of(C.re_set(r"\w"))[0]
DIGIT = C.sets_of(C.re_set(r"[0-9]"))[0]
NOT_NL = C.sets_of(C.re_set(r"[^\n]"))[0]
ZERO = np.zeros(0, dtype=np.int64)


class Pattern:
    """one pattern of one library: its kit, the dense rule as `array -> (start, end, tag)` for the occurrence calls (`rule`) and
    for the line calls (`line_rule`: runs are cut at the delimiter), and whether its scenes fit into parts of 64 bytes"""
    def __init__(self, lib, name, kit, rule, line_rule=None, small=True, **how):
        self.lib, self.name, self.kit, self.rule, self.line_rule, self.small, self.how = lib, name, kit, rule, line_rule or rule, small, how
        assert not small or kit.reach <= 9

    def spans(self, scenes, length, cache=None, lines=False):
        if self.lib == "gaps":
            return sparse_gaps(scenes, length, DELIM, self.how["lo"], self.how["hi"])
        cache = {} if cache is None else cache
        return sparse_spans(scenes, length, self.kit.margin, self.line_rule if lines else self.rule, cache.setdefault(lines, {}))


def _fixed(n):
    return lambda s: (s, s + n, np.zeros(s.size, dtype=np.int64))


def masked(name, value, mask, hits, straddle):
    n = len(value)
    return Pattern("masked", name, Kit(name, hits, n, straddle), lambda a: _fixed(n)(M.rule_offsets(a, value, mask)), value=value, mask=mask)


def classes(name, text, item, n, hits, straddle, small):
    sets = np.stack([item] * n)
    return Pattern("classes", name, Kit(name, hits, n, straddle), lambda a: _fixed(n)(C.rule_offsets(a, sets)), small=small, text=text, sets=sets)


def runs(name, words, lo, hi, hits, straddle, bitmap=False):
    def rule(delimiter):
        def f(a):
            b, e = R.rule_runs(a, words, lo, hi, delimiter)
            return b, e, np.zeros(b.size, dtype=np.int64)
        return f
    look = max(lo, (hi or 0) + 1)
    return Pattern("runs", name, Kit(name, hits, look, straddle), rule(None), rule(DELIM), words=words, lo=lo, hi=hi, bitmap=bitmap)


def needles(name, words, word, small):
    lens = np.array([len(d) for d in distinct(words)], dtype=np.int64)

    def rule(a):
        _, offs, ranks = set_rule(a, words, False, word)
        return offs, offs + lens[ranks], ranks
    longest = max(words, key=len)
    return Pattern("sets", name, Kit(name, words, len(longest), [words[0], longest]), rule, small=small, needles=words, word=word)


_W = Kit(r"\w+", [b"abc", b"q", b"Zz_09"], 1, [b"abcd"])
PATTERNS = [
    masked("qzjx", b"qzjx", b"\xff" * 4, [b"qzjx"], [b"qzjx"]),
    # a wildcard that accepts the delimiter: the second straddler is an occurrence that no line holds
    masked("q??jx", b"q\x00jx", b"\xff\x00\xff\xff", [b"qzjx", b"q\x00jx", b"qqqjx"], [b"qAjx", b"q\njx"]),
    classes("[0-9]{3}", "[0-9]{3}", DIGIT, 3, [b"123", b"9075"], [b"4567"], True),
    classes(r"\w{8}", r"\w{8}", WORD, 8, [b"abcdefgh", b"ABCD_012x"], [b"abcdefgh", b"abcdefg"], False),
    runs(r"\w+", WORD, 1, None, _W.hits, _W.straddle),
    runs(r"\w{3,}", WORD, 3, None, [b"abc", b"wxyz1"], [b"abcd", b"ab"]),
    runs(r"[0-9]{2,4}", DIGIT, 2, 4, [b"12", b"1234", b"907"], [b"123", b"12345"]),
    runs(r"[0-9]{2,4} by the bitmap", DIGIT, 2, 4, [b"12", b"1234", b"907"], [b"123", b"12345"], bitmap=True),
    # the set holds the FILLER: the whole view is runs, cut only at the scenes' delimiters (the scenes are those of \w+)
    Pattern("gaps", r"[^\n]{80,}", _W, None, words=NOT_NL, lo=80, hi=None, bitmap=False),
    needles("3 needles", THREE, False, True),
    needles("3 needles, whole words", THREE, True, True),
    needles("42 needles", FORTY, False, False),
    needles("42 needles, whole words", FORTY, True, False),
]
_SMALL_GAPS = Pattern("gaps", r"[^\n]{7,30}", _W, None, words=NOT_NL, lo=7, hi=30, bitmap=False)


# ---- the dense rules, as the suite has them ------------------------------------------------------------------------------------------
def dense(p, host):
    """((start, end, tag), (begin, end, number) of the selected lines) of pattern p on a real array, by the rules of the suite"""
    how = p.how
    if p.lib == "masked":
        s = M.rule_offsets(host, how["value"], how["mask"])
        return (s, s + len(how["value"]), 0 * s), M.rule_lines(host, how["value"], how["mask"], DELIM)
    if p.lib == "classes":
        s = C.rule_offsets(host, how["sets"])
        return (s, s + len(how["sets"]), 0 * s), C.rule_lines(host, how["sets"], DELIM)
    if p.lib in ("runs", "gaps"):
        b, e = R.rule_runs(host, how["words"], how["lo"], how["hi"])
        return (b, e, 0 * b), R.rule_lines(host, how["words"], how["lo"], how["hi"], DELIM)
    counts, offs, ranks = set_rule(host, how["needles"], False, how["word"])
    assert counts.sum() == offs.size
    lens = np.array([len(d) for d in distinct(how["needles"])], dtype=np.int64)
    # the line rule on the array: the lines of the occurrences (no needle holds the delimiter)
    d = np.flatnonzero(host == DELIM)
    ends = np.append(d, host.size) if d.size == 0 or d[-1] != host.size - 1 else d
    begins = np.concatenate([[0], d + 1])[:ends.size]
    sel = np.unique(np.searchsorted(ends, offs, side="left"))
    if not how["word"]:
        assert (sel + 1).tolist() == lines_with_any(host.tobytes(), how["needles"], DELIM)
    return (offs, offs + lens[ranks], ranks), (begins[sel], ends[sel], sel + 1)


def every_line(host):
    d = np.flatnonzero(host == DELIM)
    ends = np.append(d, host.size) if d.size == 0 or d[-1] != host.size - 1 else d
    return np.concatenate([[0], d + 1])[:ends.size], ends


def agree(p, scenes, length, what):
    """spans, lines and the other lines of pattern p: the scene list against the array; returns (spans, lines)"""
    host = write_scenes(np.full(length, FILLER, dtype=np.uint8), scenes)
    want_spans, want_lines = dense(p, host)
    got = p.spans(scenes, length)
    for g, w, name in zip(got, want_spans, ("start", "end", "tag")):
        assert g.dtype == np.int64 and g.size == w.size and (g == w).all(), (what, p.name, name, g[:8], w[:8])
    lines = sparse_lines(scenes, length, p.spans(scenes, length, lines=True))
    for g, w, name in zip(lines, want_lines, ("begin", "end", "number")):
        assert g.dtype == np.int64 and g.size == w.size and (g == w).all(), (what, p.name, "lines", name, g[:8], w[:8])
    others = sparse_lines(scenes, length, p.spans(scenes, length, lines=True), inverted=True)
    begins, ends = every_line(host)
    rest = np.setdiff1d(np.arange(1, begins.size + 1), want_lines[2])
    assert (others[2] == rest).all() and (others[0] == begins[rest - 1]).all() and (others[1] == ends[rest - 1]).all(), (what, p.name, "inverted")
    return got, lines


SMALL_BORDERS = (4, 5, 8, 20, 36, 35, 1, 3, 21, 7)          # chunk borders, the last chunk's one part, borders inside a chunk
SMALL_LONG = (9, 17)                                        # opens in chunk 2, closes in chunk 4


def small_grid(part, mis):
    return Parts(36 * part + part // 2 + 3 - mis, part, mis, chunk=4, threads=8)


def holder(part, patterns):
    for p in patterns:
        seen = set()
        for mis in (0, 5):
            pt = small_grid(part, mis)
            assert (pt.parts, pt.chunks, pt.per) == (37, 10, 5) and pt.parts - 4 * (pt.chunks - 1) == 1 and pt.length < 8 * 1024
            cut = pt.border(22) + part // 3
            for rot in range(2 * ROTATIONS):
                notes = {}
                scenes = grid_scenes(pt, p.kit, rot, SMALL_BORDERS, SMALL_LONG, flush=(cut,), notes=notes)
                what = (part, mis, rot)
                spans, lines = agree(p, scenes, pt.length, what)
                seen |= {v for k, v in notes.items() if isinstance(k, int)} | {("g", notes["long line"])}
                # kind g: no delimiter in the middle chunk, one line across it; kind h: flush with the end; kind i: in most parts
                d = delimiters(scenes)
                assert not ((d >= pt.border(12)) & (d < pt.border(16))).any() and scenes[-1][0] + len(scenes[-1][1]) == pt.length
                assert notes["background"] >= 40, notes
                if p.lib != "gaps":
                    assert lines[1][-1] == pt.length and spans[0].size > 60, what
                    long = (lines[0] < pt.border(12)) & (lines[1] >= pt.border(16))
                    assert int(long.sum()) == (1 if rot % 3 < 2 else 0), what
                # a shorter view of the same bytes, cut out of the scene list
                lo = mis % 3
                agree(p, view_scenes(scenes, lo, cut), cut - lo, what + ("cut",))
        want = {(kind, sub) for kind in range(len(KINDS)) for sub in range(p.kit.variants(kind))} | {("g", v) for v in range(len(LONG_LINE))}
        assert seen == want, (p.name, sorted(want - seen, key=str))


def test_every_kind_and_rule_at_64_bytes_per_part():
    small = [p for p in PATTERNS if p.small and p.lib != "gaps"] + [_SMALL_GAPS]
    assert {p.lib for p in small} == {"masked", "classes", "runs", "gaps", "sets"} and len(small) == 10
    holder(64, small)


def test_every_kind_and_rule_at_200_bytes_per_part():
    holder(200, [p for p in PATTERNS if p.lib != "gaps"] + [_SMALL_GAPS, Pattern("gaps", "[^\\n]{80,}", PATTERNS[4].kit, None, words=NOT_NL, lo=80, hi=None)])


def test_corners_of_the_reference():
    p, q, g = PATTERNS[1], PATTERNS[10], _SMALL_GAPS
    for length, scenes in ((1000, []), (1000, [(0, NL)]), (1000, [(999, NL)]), (1000, [(0, b"qzjx")]), (1000, [(996, b"qzjx")]),
                           (1000, [(0, b"zjx" + NL), (997, NL + b"qz")]), (1000, [(10, b"q"), (11, b"\n"), (12, b"jx")]),
                           (1000, [(500, b"Base"), (504, b"link"), (508, b"k swaps")]), (4, [(0, b"Base")]), (3, [(0, b"Bas")]),
                           (1000, [(0, NL), (1, NL), (998, NL), (999, NL)]), (1000, [(100, b"kBase Base"), (400, NL + b" link")])):
        for pat in (p, q, g, PATTERNS[4], PATTERNS[6]):
            agree(pat, scenes, length, ("corner", scenes))


# ---- the geometry the helper restates -----------------------------------------------------------------------------------------------
def _constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text) or re.search(r"constexpr[^;]*[,\s]%s\s*=\s*([^;,]+)[;,]" % name, text)
    assert m, (header, name)
    return m.group(1).strip()


def test_the_restated_constants_are_the_headers():
    assert int(_constant("needleset_launch.hpp", "kSetU")) == 4 and int(_constant("needleset_launch.hpp", "kSetTiles")) == 8
    assert int(_constant("lines_launch.hpp", "kLineChunk")) == CHUNK == 256
    assert int(_constant("prefix_kernel.hpp", "kPrefixThreads")) == THREADS == 1024
    assert int(_constant("lines_kernels.hpp", "kCombineThreads")) == THREADS
    # kWavesPerBlock = kBlock / kWave (scan_filters.hpp): four waves of 64 lanes
    assert _constant("scan_filters.hpp", "kWavesPerBlock") == "kBlock / kWave"
    waves = int(_constant("scan_filters.hpp", "kBlock")) // int(_constant("scan_filters.hpp", "kWave"))
    assert waves == 4
    launch = " ".join(open(os.path.join(CSRC, "needleset_launch.hpp")).read().split())
    assert "kSetTileChunks = (uint64_t)kWavesPerBlock * kSetU * 64;" in launch and "kSetPartBytes = kSetTileChunks * 16 * kSetTiles;" in launch
    assert waves * 4 * 64 * 16 * 8 == WG == 131072
    # the three pieces of code every one of the five host files goes through past one part
    for host in ("ss_needleset.hip", "ss_masked.hip", "ss_classes.hip", "ss_runs.hip"):
        text = open(os.path.join(CSRC, host)).read()
        assert "launch_lines_chunks(" in text and "launch_lines_combine(" in text and "kLineChunk" in text, host
    for host in ("ss_setmatches.hip", "ss_masked.hip", "ss_classes.hip", "ss_runs.hip"):
        assert "launch_set_prefix(" in open(os.path.join(CSRC, host)).read(), host
    assert "prefix_kernel<uint64_t>" in open(os.path.join(CSRC, "ss_setmatches.hip")).read()


def test_the_two_gpu_shapes_place_their_scenes_where_intended():
    a0, a5, b = shape_a(0), shape_a(5), shape_b()
    assert (a0.parts, a0.chunks, a0.per) == (a5.parts, a5.chunks, a5.per) == (258, 2, 1) and a0.parts - CHUNK * (a0.chunks - 1) == 2
    assert (b.parts, b.chunks, b.per) == (1537, 7, 2) and b.parts - CHUNK * (b.chunks - 1) == 1
    assert b.parts - 768 * b.per == 1 and THREADS - 769 == 255              # a one-part last run, 255 idle threads
    assert 33.7e6 < a0.length < 33.9e6 and 201e6 < b.length < 202e6 and a5.length == a0.length - 5 and a5.border(256) == a0.border(256) - 5
    assert LONG_B[0] // CHUNK == 2 and LONG_B[1] // CHUNK == 4
    for p in (PATTERNS[1], PATTERNS[3], PATTERNS[6], PATTERNS[12]):
        kit = p.kit
        at = {256: set(), 257: set()}
        long = set()
        for rot in range(ROTATIONS):
            notes = {}
            scenes = buffer_scenes(kit, rot, notes=notes)
            have = set(scenes)
            for j, k in enumerate(BORDERS_B):
                kind, sub = notes[k]
                assert kind == (j + rot) % len(KINDS) and set(border_scenes(kind, j, b.border(k), kit)) <= have, (rot, k)
                near = [o for o, t in scenes if b.border(k) - kit.reach <= o and o + len(t) <= b.border(k) + kit.reach]
                assert len(near) == len(border_scenes(kind, j, b.border(k), kit)), (rot, k, near)        # and nothing else there
                if k in at:
                    at[k].add(kind)
            long.add(notes["long line"])
            d = delimiters(scenes)
            assert not ((d >= b.border(3 * CHUNK)) & (d < b.border(4 * CHUNK))).any()
            assert ((d >= b.border(2 * CHUNK)) & (d < b.border(3 * CHUNK))).any() and ((d >= b.border(4 * CHUNK)) & (d < b.border(5 * CHUNK))).any()
            opened, closed = b.border(LONG_B[0]) + WG // 2, b.border(LONG_B[1]) + WG // 2
            assert not ((d > opened) & (d < closed)).any() and opened in d and closed in d
            # kind h at both ends, each in the last part of its shape; a scene on the first byte
            assert scenes[-1][0] + len(scenes[-1][1]) == LEN_B and int(b.part_of(scenes[-1][0])) == 1536
            assert any(o + len(t) == END_A and t[:1] == NL for o, t in scenes) and int(a0.part_of(END_A - 1)) == 257 and scenes[0][0] == 0
            # kind i: 1 + (7 w mod 5) scenes in every part outside the long line, but for the few that a border scene displaces
            full = sum(1 + (7 * w) % 5 for w in range(b.parts) if not LONG_B[0] <= w <= LONG_B[1])
            assert full - 12 <= notes["background"] <= full and len(scenes) > 3500, (notes["background"], full)
            per_part = np.bincount(b.part_of([o for o, t in scenes if len(t) >= 3 and t[:1] == NL and t[-1:] == NL]), minlength=b.parts)
            assert (per_part[[300, 301, 302, 303, 304]] == [1 + (7 * w) % 5 for w in range(300, 305)]).all()
            # what shape A sees of it, at either misalignment: the same scenes up to its end
            for mis in (0, 5):
                cut = view_scenes(scenes, mis, END_A)
                assert cut[-1][0] + len(cut[-1][1]) == END_A - mis and len(cut) > 600
        assert at[256] == at[257] == set(range(len(KINDS))) and long == {0, 1, 2}, (at, long)
