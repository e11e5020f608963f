#!/usr/bin/env python3
"""Regenerates tests/golden/output_kat.json, the known answers of the output calls (include/sliceslice_hip_output.h).

    python tests/golden/make_output_golden.py

The rows are those of context_kat.json (make_context_golden.ROWS) with line numbers, the empty needle with line numbers - every
line of the file - and one row without ``-n`` and with ``-A 1``.  Each row holds the length, the SHA-256 and the first and last
200 bytes (as latin-1 text) of what GNU grep writes to stdout.  The bytes are written from the rule restated here in plain Python:

    record i = (begin, end, number, kind) contributes, in this order:
      1. separators set, i > 0 and number[i] > number[i-1] + 1: ``--`` and the terminator;
      2. numbers set: the decimal digits of number[i], then ``:`` when kind[i] != 0 (or there are no kinds), else ``-``;
      3. the bytes [b, e) of the data, e = min(end, len), b = min(begin, e);
      4. the terminator, unless it is None (then the separator is ``--`` alone);
    the output is the concatenation; starts[i] is the offset where record i's contribution begins, starts[count] the length.

The records are make_context_golden.context_rule's lines; separators are set exactly when ``before`` or ``after`` is non-zero, as
in grep.  Where a GNU grep is on the machine the script compares every row with ``LC_ALL=C grep -a -F [-n] [-B before -A after]``
(the context options only where one is non-zero: grep -A 0 prints separators, plain grep does not) byte for byte, refuses to write the file on a difference and sets ``grep_checked`` (without LC_ALL=C grep's output differs on this
file).  No test runs this script.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_context_golden import ROWS as CONTEXT_ROWS, context_rule      # noqa: E402
from make_inverted_golden import all_lines, matches                     # noqa: E402

# (needle, how, invert, before, after, line_numbers)
ROWS = [r + (True,) for r in CONTEXT_ROWS] + [(b"", "", False, 0, 0, True), (b"descriptor", "", False, 0, 1, False)]
U64 = (1 << 64) - 1


def format_rule(data, begin, end, number=None, kind=None, terminator=10, numbers=False, separators=False):
    """(the output bytes, the count + 1 starts) of the rule above; numbers are taken modulo 2^64"""
    out, starts, tail = bytearray(), [], (b"" if terminator is None else bytes([terminator]))
    for i in range(len(begin)):
        starts.append(len(out))
        if separators and i > 0 and (int(number[i]) & U64) > (int(number[i - 1]) & U64) + 1:
            out += b"--" + tail
        if numbers:
            out += b"%d" % (int(number[i]) & U64) + (b":" if kind is None or kind[i] else b"-")
        e = min(int(end[i]) & U64, len(data))
        b = min(int(begin[i]) & U64, e)
        out += data[b:e] + tail
    starts.append(len(out))
    return bytes(out), starts


def row_records(data, lines, needle, how, invert, before, after):
    """(begin, end, number, kind) of the lines grep prints"""
    selected = [l[2] for l in lines if matches(data, l, needle, 10, how) != invert]
    pairs = context_rule(selected, len(lines), before, after)
    return ([lines[k - 1][0] for k, _ in pairs], [lines[k - 1][1] for k, _ in pairs], [k for k, _ in pairs], [kind for _, kind in pairs])


def row_output(data, lines, needle, how, invert, before, after, line_numbers):
    begin, end, number, kind = row_records(data, lines, needle, how, invert, before, after)
    return format_rule(data, begin, end, number, kind, 10, line_numbers, bool(before or after))[0]


def grep_output(path, needle, how, invert, before, after, line_numbers):
    flags = ["-i"] * how.endswith("i") + ["-w"] * how.startswith("w") + ["-x"] * how.startswith("x") + ["-v"] * invert + ["-n"] * line_numbers
    context = ["-B", str(before), "-A", str(after)] if before or after else []      # (an explicit -A 0 would turn the separators on)
    r = subprocess.run(["grep", "-a", "-F"] + context + flags + ["-e", needle.decode(), path],
                       capture_output=True, env=dict(os.environ, LC_ALL="C"))
    assert r.returncode in (0, 1), r.stderr
    return r.stdout


def main():
    path = os.path.join(HERE, "data", "i386.txt")
    data = open(path, "rb").read()
    lines = all_lines(data, 10)
    have_grep = bool(shutil.which("grep")) and "GNU grep" in subprocess.run(["grep", "--version"], capture_output=True, text=True).stdout
    version = subprocess.run(["grep", "--version"], capture_output=True, text=True).stdout.splitlines()[0] if have_grep else None
    rows = []
    for needle, how, invert, before, after, line_numbers in ROWS:
        text = row_output(data, lines, needle, how, invert, before, after, line_numbers)
        if have_grep and grep_output(path, needle, how, invert, before, after, line_numbers) != text:
            raise SystemExit("make_output_golden.py: grep and the rule differ for %r" % ((needle, how, invert, before, after, line_numbers),))
        rows.append({"needle": needle.decode(), "how": how, "invert": invert, "before": before, "after": after, "line_numbers": line_numbers,
                     "length": len(text), "sha256": hashlib.sha256(text).hexdigest(), "first": text[:200].decode("latin-1"),
                     "last": text[-200:].decode("latin-1")})
    out = {"file": "data/i386.txt", "lines": len(lines), "grep_version": version, "grep_checked": have_grep, "rows": rows}
    with open(os.path.join(HERE, "output_kat.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    for r in rows:
        print(repr(r["needle"]), r["how"], r["invert"], r["before"], r["after"], r["line_numbers"], r["length"], r["sha256"][:16])


if __name__ == "__main__":
    main()
