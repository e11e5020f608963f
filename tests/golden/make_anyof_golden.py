#!/usr/bin/env python3
"""Regenerates tests/golden/anyof_kat.json, the known answers of the several-needle calls (include/sliceslice_hip_anyof.h).

    python tests/golden/make_anyof_golden.py

Every row is GNU grep's own output on data/i386.txt: ``LC_ALL=C grep -a -F -n -e A -e B ...`` (with ``-i``, ``-w``, ``-x``, ``-v``
as the row says; the context rows with ``-B before -A after``), and ``-c`` for the count.  This script needs a ``grep`` on the
machine and refuses to write the file unless the rule restated here in plain Python gives the same numbers for EVERY row:

    S_k = the numbers of the lines the non-inverted model selects for needle k (make_inverted_golden.matches), U their union,
    N the number of lines; the selected set is U, or {1 .. N} minus U with ``invert``; the context rows print what
    make_context_golden.context_rule prints for it.

``rows``: the five needle sets under "", "w", "i", "x", "wi", and inverted under "", "w", "i" - 40 rows.  Per row: ``needles``,
``how`` ("" plain, "w" whole word, "x" whole line, each with "i" behind it), ``invert``; ``selected``; the ``first`` and ``last``
20 numbers; ``sha256`` of all of them written one per line.  ``context_rows`` add ``before``, ``after``, ``printed``,
``separators`` and hold (number, kind) pairs and their checksum as tests/golden/context_kat.json does.  ``words_row``: data/words.txt
as a ``-f`` file (every word of it a needle), the count only.  No test runs this script.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_context_golden import checksum, context_rule, separators      # noqa: E402
from make_inverted_golden import all_lines, matches                     # noqa: E402  (the models' rule, stated there)

SETS = [["the", "descriptor", "intel"], ["segment", "segmentation"], ["a", "ab"], ["Intel", "386", "no-such-phrase-here"],
        ["protect", "protected", "protection", "mode"]]
FLAGS = [("", False), ("w", False), ("i", False), ("x", False), ("wi", False), ("", True), ("w", True), ("i", True)]
# (needles, how, invert, before, after): -B 1 -A 2; -C 2 with -v -w; before above N; a set that selects nothing; the row of the
# command-line tool's test
CONTEXT = [
    (SETS[0], "", False, 1, 2),
    (SETS[0], "w", True, 2, 2),
    (SETS[3], "x", False, 30000, 0),
    (["no-such-phrase-here", "nor-this-one"], "", False, 3, 3),
    (["the", "descriptor"], "w", False, 1, 1),
]


def grep_flags(how, invert):
    return ["-i"] * how.endswith("i") + ["-w"] * how.startswith("w") + ["-x"] * how.startswith("x") + ["-v"] * invert


def grep(path, needles, how, invert, extra):
    cmd = ["grep", "-a", "-F"] + extra + grep_flags(how, invert)
    for n in needles:
        cmd += ["-e", n]
    r = subprocess.run(cmd + [path], capture_output=True, env=dict(os.environ, LC_ALL="C"))
    assert r.returncode in (0, 1), r.stderr
    return r.stdout


def grep_pairs(out):
    pairs, seps = [], 0
    for line in out.split(b"\n")[:-1]:
        if line == b"--":
            seps += 1
            continue
        digits = 0
        while line[digits:digits + 1].isdigit():
            digits += 1
        assert digits and line[digits:digits + 1] in (b":", b"-"), line
        pairs.append((int(line[:digits]), 1 if line[digits:digits + 1] == b":" else 0))
    return pairs, seps


def numbers_checksum(numbers):
    return hashlib.sha256("".join("%d\n" % n for n in numbers).encode()).hexdigest()


def rule(data, lines, needles, how, invert):
    union = set()
    for needle in needles:
        union.update(l[2] for l in lines if matches(data, l, needle.encode(), 10, how))
    return [l[2] for l in lines if (l[2] in union) != invert]


def words_rule(data, words):
    """the number of lines that hold any of `words` (none of which holds a newline)"""
    starts = [0] + [k + 1 for k in range(len(data)) if data[k] == 10]
    import bisect
    hit = set()
    for w in words:
        at = data.find(w)
        while at >= 0:
            hit.add(bisect.bisect_right(starts, at))
            at = data.find(w, at + 1)
    return len(hit)


def main():
    if not shutil.which("grep"):
        raise SystemExit("make_anyof_golden.py: the rows are grep's output; there is no grep on this machine")
    path = os.path.join(HERE, "data", "i386.txt")
    data = open(path, "rb").read()
    lines = all_lines(data, 10)
    version = subprocess.run(["grep", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    rows, context_rows = [], []
    for needles in SETS:
        for how, invert in FLAGS:
            pairs, seps = grep_pairs(grep(path, needles, how, invert, ["-n"]))
            numbers = [p[0] for p in pairs]
            count = int(grep(path, needles, how, invert, ["-c"]))
            want = rule(data, lines, needles, how, invert)
            if numbers != want or count != len(want) or seps or not all(k for _, k in pairs):
                raise SystemExit("make_anyof_golden.py: grep and the rule differ for %r" % ((needles, how, invert),))
            rows.append({"needles": needles, "how": how, "invert": invert, "selected": count, "first": numbers[:20], "last": numbers[-20:],
                         "sha256": numbers_checksum(numbers)})
    for needles, how, invert, before, after in CONTEXT:
        pairs, seps = grep_pairs(grep(path, needles, how, invert, ["-n", "-B", str(before), "-A", str(after)]))
        want = context_rule(rule(data, lines, needles, how, invert), len(lines), before, after)
        if pairs != want or seps != separators(want):
            raise SystemExit("make_anyof_golden.py: grep and the rule differ for %r" % ((needles, how, invert, before, after),))
        context_rows.append({"needles": needles, "how": how, "invert": invert, "before": before, "after": after,
                             "selected": sum(k for _, k in pairs), "printed": len(pairs), "separators": seps,
                             "first": [list(p) for p in pairs[:20]], "last": [list(p) for p in pairs[-20:]], "sha256": checksum(pairs)})
    words_path = os.path.join(HERE, "data", "words.txt")
    words = [w for w in open(words_path, "rb").read().split(b"\n") if w]
    r = subprocess.run(["grep", "-a", "-F", "-c", "-f", words_path, path], capture_output=True, env=dict(os.environ, LC_ALL="C"))
    assert r.returncode in (0, 1), r.stderr
    if int(r.stdout) != words_rule(data, words):
        raise SystemExit("make_anyof_golden.py: grep and the rule differ for the word list")
    words_row = {"file": "data/words.txt", "needles": len(words), "how": "", "invert": False, "selected": int(r.stdout)}
    out = {"file": "data/i386.txt", "lines": len(lines), "grep_version": version, "grep_checked": True, "rows": rows,
           "context_rows": context_rows, "words_row": words_row}
    with open(os.path.join(HERE, "anyof_kat.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    for r in rows + context_rows:
        print(" ".join(r["needles"]), repr(r["how"]), r["invert"], r.get("before", ""), r.get("after", ""), r["selected"], r.get("printed", ""))
    print("words.txt:", words_row)


if __name__ == "__main__":
    main()
