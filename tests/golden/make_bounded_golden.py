#!/usr/bin/env python3
"""Regenerates tests/golden/bounded_kat.json, the known answers of the whole-word / whole-line calls
(include/sliceslice_hip_bounded.h).

    python tests/golden/make_bounded_golden.py

Pure Python over tests/golden/data/.  The rule, as the header states it: an occurrence at offset p of a needle of n bytes has the
neighbours hay[p - 1] (absent when p == 0) and hay[p + n] (absent when p + n == len).  WORD keeps it when each neighbour is absent,
no word byte ([0-9A-Za-z_]) or - in the line forms - the delimiter; LINE (line forms only) when each is absent or the delimiter.
A line matches when one of its occurrences is kept.  Ignoring case changes which bytes are equal and nothing else.

* ``index`` / ``words`` - every 13th word of data/words.txt (its index there, the word as latin-1).  Per word, against
  data/i386.txt with delimiter '\\n': ``word_count`` (whole-word occurrences), ``word_lines`` (lines with one), ``line_lines`` (lines
  equal to the word) and the same three ignoring case (``*_nocase``).
* ``table`` - the same six figures and the unbounded count for `the`, `descriptor` and `intel`, which README and DESIGN.md 5.10 quote.
* ``grep_checked`` - whether the three line counts of every word above were compared with ``LC_ALL=C grep -a -F -c`` with ``-w``,
  ``-x`` and ``-w -i`` (and ``-x -i``) when this file was written: done where a ``grep`` is on the machine, and this script refuses
  to write the file on a difference.  ``grep_version`` is the first line of ``grep --version`` then.  No test runs grep.
* ``cases`` - a hand-written table of small haystacks covering the rule's corners, with the expected offsets (occurrence form; null
  for LINE, which has none) and records (line form) written out by hand; this script refuses to write the file unless the rule
  reproduces them.  ``how`` is "w" or "x", with "i" behind it for ignoring case.
"""
import bisect
import json
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
WORD_BYTES = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")
STRIDE = 13


def occurrences(data, needle, nocase):
    """every offset of needle in data, overlapping, ascending (nocase: both sides through bytes.lower())"""
    h, n = (data.lower(), needle.lower()) if nocase else (data, needle)
    out, i = [], h.find(n)
    while i >= 0:
        out.append(i)
        i = h.find(n, i + 1)
    return out


def kept(data, p, n, line, delimiter):
    """the rule for the occurrence [p, p + n): the neighbours are read from the bytes AS THEY ARE"""
    for at in (p - 1, p + n):
        if at < 0 or at >= len(data):
            continue                                    # absent
        b = data[at]
        if delimiter is not None and b == delimiter:
            continue
        if line or b in WORD_BYTES:
            return False
    return True


def offsets_of(data, needle, nocase=False):
    """WORD, occurrence form"""
    return [p for p in occurrences(data, needle, nocase) if kept(data, p, len(needle), False, None)]


def lines_of(data, needle, delimiter, line, nocase=False):
    """[(begin, end, number)] of the lines of `data` (cut at the delimiter byte as it is) with a kept occurrence.  The needle a
    folding searcher holds is the folded one; a needle that holds the delimiter matches no line."""
    held = needle.lower() if nocase else needle
    if delimiter in held:
        return []
    ends = [i for i, b in enumerate(data) if b == delimiter]          # a line's end: its delimiter, or len for an open last line
    if not data.endswith(bytes([delimiter])) and data:
        ends.append(len(data))
    out, last = [], 0
    for p in occurrences(data, needle, nocase):
        if delimiter in data[p:p + len(needle)] or not kept(data, p, len(needle), line, delimiter):
            continue                                    # (ignoring case, a delimiter 'A' can sit where the folded bytes hold the needle's 'a')
        k = bisect.bisect_left(ends, p)                 # (it holds no delimiter: it lies inside line k)
        if k + 1 > last:
            last = k + 1
            out.append(((ends[k - 1] + 1) if k else 0, ends[k], k + 1))
    return out


# (what it shows, haystack, needle, delimiter, how, expected offsets or None, expected records) - haystack and needle as latin-1
CASES = [
    ("a word between blanks, and the same bytes inside 'other'", "the other the", "the", 10, "w", [0, 10], [(0, 13, 1)]),
    ("inside longer words it is no word", "other then these", "the", 10, "w", [], []),
    ("'_' and the digits are word bytes", "_the the_ 1the the2 the", "the", 10, "w", [20], [(0, 23, 1)]),
    ("'@' '[' '`' '{' next to the letters and '/' ':' next to the digits are no word bytes", "@ab[ `ab{ /ab: ", "ab", 10, "w",
     [1, 6, 11], [(0, 15, 1)]),
    ("bytes >= 0x80 are no word bytes: 0x80, and 0xC1 / 0xE1 whose low seven bits look like letters", "\x80ab\xc1 \xe1ab\xff", "ab", 10,
     "w", [1, 6], [(0, 9, 1)]),
    ("a haystack that is exactly the needle: both neighbours absent", "ab", "ab", 10, "w", [0], [(0, 2, 1)]),
    ("len == n + 1, a word byte behind", "abc", "ab", 10, "w", [], []),
    ("len == n + 1, a word byte in front", "cab", "ab", 10, "w", [], []),
    ("len == n + 1, a blank in front: the right neighbour is absent", " ab", "ab", 10, "w", [1], [(0, 3, 1)]),
    ("the test looks at the neighbours only, never at the needle's own bytes", "a.foo .foo", ".foo", 10, "w", [6], [(0, 10, 1)]),
    ("overlapping occurrences are tested one by one", "aa aaa a", "aa", 10, "w", [0], [(0, 8, 1)]),
    ("overlapping occurrences can both be kept", " - - ", " - ", 10, "w", [0, 2], [(0, 5, 1)]),
    ("a one-byte needle", "a a1 a", "a", 10, "w", [0, 5], [(0, 6, 1)]),
    ("needle longer than the haystack", "ab", "abc", 10, "w", [], []),
    ("a line matches when one occurrence is kept, also behind others that are not", "other the\nother\nthe", "the", 10, "w", [6, 16],
     [(0, 9, 1), (16, 19, 3)]),
    ("a delimiter that is a word byte still ends a word in the line forms, not in the occurrence forms", "theatheb the", "the", ord("a"),
     "w", [9], [(0, 3, 1), (4, 12, 2)]),
    ("a needle that holds the delimiter matches no line", "a b a b", "a b", ord(" "), "w", [0, 4], []),
    ("whole line: only lines equal to the needle, the open last line included", "the\nthe \n the\nthe", "the", 10, "x", None,
     [(0, 3, 1), (14, 17, 4)]),
    ("whole line: the last line with its delimiter", "ab\nthe\n", "the", 10, "x", None, [(3, 6, 2)]),
    ("whole line: empty lines match nothing", "\n\nthe\n\n", "the", 10, "x", None, [(2, 5, 3)]),
    ("whole line: blanks are not the delimiter", " the \nthe", "the", 10, "x", None, [(6, 9, 2)]),
    ("whole line, delimiter 0x00", "the\x00other\x00the", "the", 0, "x", None, [(0, 3, 1), (10, 13, 3)]),
    ("ignoring case: letters match in either case, the neighbour classes do not change", "The THE tHe oTHEr", "the", 10, "wi", [0, 4, 8],
     [(0, 17, 1)]),
    ("ignoring case the delimiter is not folded: 'A' ends a word, 'a' does not", "theAthea", "the", ord("A"), "wi", [], [(0, 3, 1)]),
    ("whole line ignoring case", "THE\nthe\nThe x", "the", 10, "xi", None, [(0, 3, 1), (4, 7, 2)]),
]

TABLE_WORDS = [b"the", b"descriptor", b"intel"]


def figures(data, w):
    return {"word_count": len(offsets_of(data, w)), "word_lines": len(lines_of(data, w, 10, False)),
            "line_lines": len(lines_of(data, w, 10, True)), "word_count_nocase": len(offsets_of(data, w, True)),
            "word_lines_nocase": len(lines_of(data, w, 10, False, True)), "line_lines_nocase": len(lines_of(data, w, 10, True, True))}


def grep_count(path, flags, w):
    p = subprocess.run(["grep", "-a", "-F", "-c"] + flags + ["-e", w, path], env=dict(os.environ, LC_ALL="C"), capture_output=True)
    assert p.returncode in (0, 1), (flags, w, p.stderr)
    return int(p.stdout)


def main():
    cases = []
    for what, hay, needle, delim, how, offs, recs in CASES:
        h, n = hay.encode("latin-1"), needle.encode("latin-1")
        nocase, line = how.endswith("i"), how.startswith("x")
        got_o = None if line else offsets_of(h, n, nocase)
        got_r = lines_of(h, n, delim, line, nocase)
        assert got_o == offs and got_r == recs, (what, got_o, offs, got_r, recs)
        cases.append({"what": what, "haystack": h.hex(), "needle": n.hex(), "delimiter": delim, "how": how, "offsets": offs,
                      "records": [list(r) for r in recs]})
    path = os.path.join(HERE, "data", "i386.txt")
    data = open(path, "rb").read()
    words = open(os.path.join(HERE, "data", "words.txt"), "rb").read().split(b"\n")
    if words[-1] == b"":
        words.pop()
    index = list(range(0, len(words), STRIDE))
    rows = [figures(data, words[k]) for k in index]
    table = {}
    for w in TABLE_WORDS:
        table[w.decode()] = dict(figures(data, w), count=len(occurrences(data, w, False)))
    grep = shutil.which("grep")
    version = None
    if grep:
        version = subprocess.run(["grep", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
        for w, f in list(zip((words[k] for k in index), rows)) + [(w, table[w.decode()]) for w in TABLE_WORDS]:
            if b"\n" in w or w == b"":
                continue
            got = (grep_count(path, ["-w"], w), grep_count(path, ["-x"], w), grep_count(path, ["-w", "-i"], w),
                   grep_count(path, ["-x", "-i"], w))
            want = (f["word_lines"], f["line_lines"], f["word_lines_nocase"], f["line_lines_nocase"])
            assert got == want, (w, got, want)
    out = {"stride": STRIDE, "index": index, "words": [words[k].decode("latin-1") for k in index], "table": table,
           "grep_checked": bool(grep), "grep_version": version, "cases": cases}
    for key in rows[0]:
        out[key] = [r[key] for r in rows]
    with open(os.path.join(HERE, "bounded_kat.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("bounded_kat.json:", len(index), "words,", sum(out["word_count"]), "whole-word occurrences,", sum(out["word_lines"]),
          "whole-word lines,", sum(out["line_lines"]), "whole lines, grep checked:", bool(grep), "-", len(cases), "cases")
    print(json.dumps(table))


if __name__ == "__main__":
    main()
