#!/usr/bin/env python3
"""Regenerates tests/golden/leftmost_kat.json, the known answers of the leftmost-longest calls
(include/sliceslice_hip_leftmost.h).

    python tests/golden/make_leftmost_golden.py

Six needle sets chosen for prefixes, infixes and self-overlap, each under the four combinations of ignore_case (grep -i) and
whole_word (grep -w), on data/i386.txt.  A row holds the count, the first and last eight (offset, needle index) pairs and the
SHA-256 of the whole list written as ``offset:index\\n`` lines.  Four replace rows - replacements empty, shorter than, as long as
and longer than their needles - hold the output's length and SHA-256.  The values come from the rule restated here as a byte-wise
loop:

    the occurrences of a needle are the offsets where its bytes stand (after the ASCII fold, with ignore_case); with whole_word
    only those with no word byte ([0-9A-Za-z_]) directly in front and behind; at each offset the longest occurring needle is the
    candidate; the first candidate is selected, and after a selected one at p of length L the next is the first candidate at or
    beyond p + L.

``rule_regex`` states it a second time as a ``re`` alternation sorted longest first (with the two word lookarounds for
whole_word); the script asserts both equal.  Where a GNU grep is on the machine it also compares every row with
``LC_ALL=C grep -a -o -b -F [-i] [-w] -e ...`` line for line, refuses to write the file on a difference and sets ``grep_checked``.
No test runs this script; tests import its rule.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = "data/i386.txt"
SETS = [
    [b"the", b"then", b"there", b"he", b"here"],
    [b"  ", b" "],
    [b"386", b"80386", b"8038", b"03"],
    [b"descriptor", b"script", b"descriptors", b"or"],
    [b"--", b"---", b"-"],
    [b"in", b"int", b"interrupt", b"interrupts", b"rupt"],
]
# (set index, ignore_case, whole_word, replacements parallel to the needles)
REPLACE_ROWS = [
    (0, False, False, [b"", b"", b"", b"", b""]),
    (2, False, False, [b"x", b"cpu", b"y", b"z"]),
    (0, True, True, [b"THE", b"THEN", b"THERE", b"HE", b"HERE"]),
    (3, True, False, [b"<<segment descriptor>>", b"[[a script]]", b"<<segment descriptors>>", b"or else"]),
]
_FOLD = bytes(b | 0x20 if 0x41 <= b <= 0x5A else b for b in range(256))
_WORD = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")


def rule(data, needles, ignore_case=False, whole_word=False):
    """[(offset, index of the needle as given)] of the leftmost-longest, non-overlapping selection: the byte-wise loop.  Of equal
    needles (after the fold) the smallest index is named."""
    data = bytes(data)
    text = data.translate(_FOLD) if ignore_case else data
    folded = [bytes(n).translate(_FOLD) if ignore_case else bytes(n) for n in needles]
    order = sorted(range(len(folded)), key=lambda k: (-len(folded[k]), k))        # longest first, then as given
    firsts = frozenset(n[:1] for n in folded)
    out, p, end = [], 0, len(text)
    while p < end:
        hit = None
        if text[p:p + 1] in firsts:
            for k in order:
                n = folded[k]
                if not n or not text.startswith(n, p):
                    continue
                if whole_word and ((p > 0 and data[p - 1] in _WORD) or (p + len(n) < end and data[p + len(n)] in _WORD)):
                    continue
                hit = k
                break
        if hit is None:
            p += 1
        else:
            out.append((p, hit))
            p += len(folded[hit])
    return out


def rule_regex(data, needles, ignore_case=False, whole_word=False):
    """The same as a ``re`` alternation sorted longest first."""
    order = sorted(range(len(needles)), key=lambda k: (-len(needles[k]), k))
    body = b"|".join(b"(" + re.escape(bytes(needles[k])) + b")" for k in order)
    if whole_word:
        body = b"(?<![0-9A-Za-z_])(?:" + body + b")(?![0-9A-Za-z_])"
    fold = (lambda b: bytes(b).translate(_FOLD)) if ignore_case else bytes
    first = {}
    for k, n in enumerate(needles):
        first.setdefault(fold(n), k)
    return [(m.start(), first[fold(needles[order[m.lastindex - 1]])]) for m in re.finditer(body, bytes(data), re.I if ignore_case else 0)]


def substitute(data, needles, replacements, ignore_case=False, whole_word=False):
    """The data with every selected occurrence replaced by the text of its needle."""
    out, at = bytearray(), 0
    for p, k in rule(data, needles, ignore_case, whole_word):
        out += data[at:p] + replacements[k]
        at = p + len(needles[k])
    return bytes(out + data[at:])


def list_hash(pairs):
    return hashlib.sha256(b"".join(b"%d:%d\n" % pk for pk in pairs)).hexdigest()


def grep_pairs(path, needles, ignore_case, whole_word):
    """What LC_ALL=C grep -a -o -b -F prints, as (offset, matched bytes)."""
    cmd = ["grep", "-a", "-o", "-b", "-F"] + (["-i"] if ignore_case else []) + (["-w"] if whole_word else [])
    for n in needles:
        cmd += ["-e", n.decode("latin-1")]
    out = subprocess.run(cmd + [path], capture_output=True, env=dict(os.environ, LC_ALL="C")).stdout
    return [(int(l.split(b":", 1)[0]), l.split(b":", 1)[1]) for l in out.split(b"\n") if l]


def main():
    data = open(os.path.join(HERE, FILE), "rb").read()
    grep = shutil.which("grep")
    version = subprocess.run([grep, "--version"], capture_output=True, text=True).stdout.splitlines()[0] if grep else ""
    checked = "GNU grep" in version
    rows = []
    for si, needles in enumerate(SETS):
        for ignore_case in (False, True):
            for whole_word in (False, True):
                pairs = rule(data, needles, ignore_case, whole_word)
                assert pairs == rule_regex(data, needles, ignore_case, whole_word), (si, ignore_case, whole_word)
                if checked:
                    got = grep_pairs(os.path.join(HERE, FILE), needles, ignore_case, whole_word)
                    want = [(p, data[p:p + len(needles[k])]) for p, k in pairs]
                    if got != want:
                        sys.exit("grep disagrees with the rule for set %d, -i %s, -w %s: %d against %d" % (si, ignore_case, whole_word, len(got), len(want)))
                rows.append({"set": si, "ignore_case": ignore_case, "whole_word": whole_word, "count": len(pairs),
                             "first": [list(x) for x in pairs[:8]], "last": [list(x) for x in pairs[-8:]], "sha256": list_hash(pairs)})
    replace = []
    for si, ignore_case, whole_word, reps in REPLACE_ROWS:
        text = substitute(data, SETS[si], reps, ignore_case, whole_word)
        replace.append({"set": si, "ignore_case": ignore_case, "whole_word": whole_word, "replacements": [r.decode("latin-1") for r in reps],
                        "length": len(text), "sha256": hashlib.sha256(text).hexdigest()})
    kat = {"file": FILE, "sets": [[n.decode("latin-1") for n in s] for s in SETS], "grep_checked": checked, "grep_version": version,
           "rows": rows, "replace": replace}
    with open(os.path.join(HERE, "leftmost_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")
    print("wrote %d rows and %d replace rows (grep checked: %s)" % (len(rows), len(replace), checked))


if __name__ == "__main__":
    main()
