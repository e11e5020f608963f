#!/usr/bin/env python3
"""Regenerates tests/golden/context_kat.json, the known answers of the context calls (include/sliceslice_hip_context.h).

    python tests/golden/make_context_golden.py

Every row is GNU grep's own output: ``LC_ALL=C grep -a -F -n -B before -A after`` (with ``-i``, ``-w``, ``-x``, ``-v`` as the row
says) on data/i386.txt, parsed into (number, kind) pairs - ``number:`` is a selected line (kind 1), ``number-`` a context line
(kind 0), ``--`` a separator.  This script needs a ``grep`` on the machine and refuses to write the file unless the rule restated
here in plain Python gives the same pairs and the same number of separators:

    S = the numbers of the lines the model selects (make_inverted_golden.matches, inverted or not), N = the number of lines;
    the output is every line in the union over s in S of [max(1, s - before), min(N, s + after)], once, ascending;
    a separator stands wherever two consecutive output numbers differ by more than 1.

Per row: ``needle``, ``how`` ("" plain, "w" whole word, "x" whole line, each with "i" behind it), ``invert``, ``before``,
``after``; ``selected`` (lines of kind 1), ``printed`` (all output lines), ``separators``; the ``first`` and ``last`` 20 pairs;
``sha256`` of the whole list written as ``number:kind`` lines.  No test runs this script; tests/test_gpu_context.py runs grep
once more, for the command-line tool.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_inverted_golden import all_lines, matches      # noqa: E402  (the models' rule, stated there)

# (needle, how, invert, before, after): the five rows the header's table quotes, then -x, -i -w, -v -i, -C 1 and 0 / 30,000 (> N)
ROWS = [
    (b"descriptor", "", False, 1, 2),
    (b"the", "w", False, 0, 3),
    (b"intel", "i", False, 5, 0),
    (b"the", "w", True, 2, 2),
    (b"no such phrase in the manual", "", False, 3, 3),
    (b"None", "x", False, 1, 1),
    (b"intel", "wi", False, 1, 1),
    (b"descriptor", "i", True, 0, 1),
    (b"the", "", False, 1, 1),
    (b"descriptor", "", False, 30000, 0),
    (b"descriptor", "", False, 0, 30000),
    (b"intel", "i", False, 30000, 30000),
    (b"Flags Affected", "xi", False, 0, 0),
]


def context_rule(selected, n_lines, before, after):
    """[(number, kind)] ascending"""
    sel = set(s for s in selected if 1 <= s <= n_lines)
    out = set()
    for s in sel:
        out.update(range(max(1, s - before), min(n_lines, s + after) + 1))
    return [(k, 1 if k in sel else 0) for k in sorted(out)]


def separators(pairs):
    return sum(1 for p, q in zip(pairs, pairs[1:]) if q[0] - p[0] > 1)


def checksum(pairs):
    return hashlib.sha256("".join("%d:%d\n" % p for p in pairs).encode()).hexdigest()


def grep_pairs(path, needle, how, invert, before, after):
    flags = ["-i"] * how.endswith("i") + ["-w"] * how.startswith("w") + ["-x"] * how.startswith("x") + ["-v"] * invert
    r = subprocess.run(["grep", "-a", "-F", "-n", "-B", str(before), "-A", str(after)] + flags + ["-e", needle.decode(), path],
                       capture_output=True, env=dict(os.environ, LC_ALL="C"))
    assert r.returncode in (0, 1), r.stderr
    pairs, seps = [], 0
    for line in r.stdout.split(b"\n")[:-1]:
        if line == b"--":
            seps += 1
            continue
        digits = 0
        while line[digits:digits + 1].isdigit():
            digits += 1
        assert digits and line[digits:digits + 1] in (b":", b"-"), line
        pairs.append((int(line[:digits]), 1 if line[digits:digits + 1] == b":" else 0))
    return pairs, seps


def main():
    if not shutil.which("grep"):
        raise SystemExit("make_context_golden.py: the rows are grep's output; there is no grep on this machine")
    path = os.path.join(HERE, "data", "i386.txt")
    data = open(path, "rb").read()
    lines = all_lines(data, 10)
    version = subprocess.run(["grep", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    rows = []
    for needle, how, invert, before, after in ROWS:
        pairs, seps = grep_pairs(path, needle, how, invert, before, after)
        selected = [l[2] for l in lines if matches(data, l, needle, 10, how) != invert]
        want = context_rule(selected, len(lines), before, after)
        if pairs != want or seps != separators(want):
            raise SystemExit("make_context_golden.py: grep and the rule differ for %r" % ((needle, how, invert, before, after),))
        rows.append({"needle": needle.decode(), "how": how, "invert": invert, "before": before, "after": after,
                     "selected": sum(k for _, k in pairs), "printed": len(pairs), "separators": seps,
                     "first": [list(p) for p in pairs[:20]], "last": [list(p) for p in pairs[-20:]], "sha256": checksum(pairs)})
    out = {"file": "data/i386.txt", "lines": len(lines), "grep_version": version, "grep_checked": True, "rows": rows}
    with open(os.path.join(HERE, "context_kat.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    for r in rows:
        print(r["needle"], r["how"], r["invert"], r["before"], r["after"], r["selected"], r["printed"], r["separators"])


if __name__ == "__main__":
    main()
