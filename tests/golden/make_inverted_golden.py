#!/usr/bin/env python3
"""Regenerates tests/golden/inverted_kat.json, the known answers of the inverted line calls (include/sliceslice_hip_inverted.h).

    python tests/golden/make_inverted_golden.py

Pure Python over tests/golden/data/.  The rule is the COMPLEMENT of make_lines_golden.py's and make_bounded_golden.py's: the lines of
the haystack are cut at the delimiter byte as it is, an unterminated last line is a line, an empty haystack has none; under ``how``
("" plain, "w" whole word, "x" whole line, each with "i" behind it for ignoring ASCII case) a line MATCHES when it holds an
occurrence that does not run over a delimiter and - "w" / "x" - is kept by make_bounded_golden.kept; the inverted call selects
exactly the lines that do not match.  A needle longer than the haystack or one that holds the delimiter matches no line, so every
line is selected; the empty needle ("" and "i" only) matches every line, so none is.

* ``index`` / ``words`` - every 113th word of data/words.txt (its index there, the word as latin-1): a few dozen.  Per word and
  ``how``, against data/i386.txt with delimiter '\\n': ``inverted[how]`` - the number of selected lines.  ``lines`` is the number of
  lines of the manual.
* ``table`` - the same six figures for `the`, `descriptor` and `intel`, which README and DESIGN.md 5.11 quote.
* ``grep_checked`` - whether every figure above was compared with ``LC_ALL=C grep -a -F -v -c`` (with ``-i``, ``-w``, ``-x`` as
  ``how`` says) when this file was written: done where a ``grep`` is on the machine (GNU grep 3.7 when this was last run), and this
  script refuses to write the file on a difference.  ``grep_version`` is the first line of ``grep --version`` then.  No test runs
  grep.
* ``cases`` - a hand-written table of small haystacks covering the rule's corners with the expected records (begin, end, number)
  written out by hand; this script refuses to write the file unless the rule reproduces them.
"""
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_bounded_golden import kept, occurrences      # noqa: E402  (the occurrence rule and the neighbour test, stated there)

STRIDE = 113
HOWS = ["", "i", "w", "wi", "x", "xi"]
TABLE_WORDS = [b"the", b"descriptor", b"intel"]


def all_lines(data, delimiter):
    """[(begin, end, number)] of every line: end is the line's delimiter, or len for an unterminated last line"""
    out, begin = [], 0
    for i, b in enumerate(data):
        if b == delimiter:
            out.append((begin, i, len(out) + 1))
            begin = i + 1
    if begin < len(data):
        out.append((begin, len(data), len(out) + 1))
    return out


def matches(data, line, needle, delimiter, how):
    """does the line (begin, end, number) of data match under `how`?  Neighbours are looked up in the whole haystack: a line's
    ends are delimiters or the haystack's ends."""
    nocase, bound = how.endswith("i"), how[:1] if how[:1] in ("w", "x") else ""
    held = needle.lower() if nocase else needle
    if delimiter in held:
        return False
    if not held:
        return True                                     # ("" and "i" only: the empty needle with a bound is refused)
    begin, end, _ = line
    for p in occurrences(data[begin:end], held, nocase):
        if not bound or kept(data, begin + p, len(held), bound == "x", delimiter):
            return True
    return False


def inverted_lines(data, needle, delimiter, how):
    return [l for l in all_lines(data, delimiter) if not matches(data, l, needle, delimiter, how)]


# (what it shows, haystack, needle, delimiter, how, expected records) - haystack and needle as latin-1
CASES = [
    ("the lines without the needle", "ab\ncd\nab cd\n", "ab", 10, "", [(3, 5, 2)]),
    ("an unterminated last line is a line", "ab\ncd", "ab", 10, "", [(3, 5, 2)]),
    ("an unterminated last line that matches is not selected", "cd\nab", "ab", 10, "", [(0, 2, 1)]),
    ("a match on the last line with its delimiter", "cd\nab\n", "ab", 10, "", [(0, 2, 1)]),
    ("empty lines never hold a needle", "\n\nab\n\n", "ab", 10, "", [(0, 0, 1), (1, 1, 2), (5, 5, 4)]),
    ("delimiters only", "\n\n\n", "a", 10, "", [(0, 0, 1), (1, 1, 2), (2, 2, 3)]),
    ("no delimiter and no match: one line", "abcabc", "cc", 10, "", [(0, 6, 1)]),
    ("no delimiter and a match: nothing", "abcabc", "ca", 10, "", []),
    ("a needle longer than the haystack matches no line: every line", "ab\nc", "abcde", 10, "", [(0, 2, 1), (3, 4, 2)]),
    ("a needle that holds the delimiter matches no line: every line", "a b a b", "a b", ord(" "), "",
     [(0, 1, 1), (2, 3, 2), (4, 5, 3), (6, 7, 4)]),
    ("the empty needle matches every line: none is selected", "ab\ncd", "", 10, "", []),
    ("an empty haystack has no line", "", "ab", 10, "", []),
    ("an occurrence across a delimiter is none", "ab\nab", "b\na", 10, "", [(0, 2, 1), (3, 5, 2)]),
    ("a delimiter that is a needle byte's other case is not folded", "xaBay", "ab", ord("B"), "i", [(0, 2, 1), (3, 5, 2)]),
    ("ignoring case", "AB\ncd\nAb x", "ab", 10, "i", [(3, 5, 2)]),
    ("case matters without it", "AB\ncd\nab x", "ab", 10, "", [(0, 2, 1), (3, 5, 2)]),
    ("whole word: a line whose occurrences all sit inside longer words is selected", "other\nthe other\nthen", "the", 10, "w",
     [(0, 5, 1), (16, 20, 3)]),
    ("whole word ignoring case; the delimiter 'A' ends a word, 'a' does not", "theAthea", "the", ord("A"), "wi", [(4, 8, 2)]),
    ("whole line: every line that is not the needle", "the\nthe \n the\nthe", "the", 10, "x", [(4, 8, 2), (9, 13, 3)]),
    ("whole line ignoring case", "THE\nthe\nThe x", "the", 10, "xi", [(8, 13, 3)]),
    ("whole line: empty lines are selected", "\n\nthe\n\n", "the", 10, "x", [(0, 0, 1), (1, 1, 2), (6, 6, 4)]),
]


def grep_count(path, how, w):
    flags = ["-" + f for f in how]
    p = subprocess.run(["grep", "-a", "-F", "-v", "-c"] + flags + ["-e", w, path], env=dict(os.environ, LC_ALL="C"), capture_output=True)
    assert p.returncode in (0, 1), (flags, w, p.stderr)
    return int(p.stdout)


def main():
    cases = []
    for what, hay, needle, delim, how, recs in CASES:
        h, n = hay.encode("latin-1"), needle.encode("latin-1")
        got = inverted_lines(h, n, delim, how)
        assert got == recs, (what, got, recs)
        merged = sorted(got + [l for l in all_lines(h, delim) if matches(h, l, n, delim, how)])
        assert merged == all_lines(h, delim), what
        cases.append({"what": what, "haystack": h.hex(), "needle": n.hex(), "delimiter": delim, "how": how, "records": [list(r) for r in recs]})
    path = os.path.join(HERE, "data", "i386.txt")
    data = open(path, "rb").read()
    words = open(os.path.join(HERE, "data", "words.txt"), "rb").read().split(b"\n")
    if words[-1] == b"":
        words.pop()
    index = list(range(0, len(words), STRIDE))
    lines = all_lines(data, 10)

    def figures(w):
        return {how: sum(1 for l in lines if not matches(data, l, w, 10, how)) for how in HOWS}
    rows = [figures(words[k]) for k in index]
    table = {w.decode(): figures(w) for w in TABLE_WORDS}
    grep = shutil.which("grep")
    version = None
    if grep:
        version = subprocess.run(["grep", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
        for w, f in list(zip((words[k] for k in index), rows)) + [(w, table[w.decode()]) for w in TABLE_WORDS]:
            if b"\n" in w or w == b"":
                continue
            for how in HOWS:
                got = grep_count(path, how, w)
                assert got == f[how], (w, how, got, f[how])
    out = {"stride": STRIDE, "index": index, "words": [words[k].decode("latin-1") for k in index], "lines": len(lines), "hows": HOWS,
           "inverted": {how: [r[how] for r in rows] for how in HOWS}, "table": table, "grep_checked": bool(grep), "grep_version": version,
           "cases": cases}
    with open(os.path.join(HERE, "inverted_kat.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("inverted_kat.json:", len(index), "words,", len(lines), "lines, grep checked:", bool(grep), version, "-", len(cases), "cases")
    print(json.dumps(table))


if __name__ == "__main__":
    main()
