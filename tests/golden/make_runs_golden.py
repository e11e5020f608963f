#!/usr/bin/env python3
"""Regenerates tests/golden/runs_kat.json, the known answers of the run calls (include/sliceslice_hip_runs.h).

    python tests/golden/make_runs_golden.py

An INDEPENDENT reference: a run pattern is ONE item C of the classes language and one quantifier, and the header states the
selection in ``re`` terms - ``(?<![C])[C]{min,max}(?![C])`` - so exactly that is handed to ``re`` (bytes, ``re.S``), over
data/i386.txt.  A case holds the count, the first and last runs as (begin, end) pairs, the SHA-256 of all begins followed by all ends
as little-endian 64-bit words, and the number of lines that hold a selected run: the text is ``split`` at the delimiter and every
piece searched on its own, which is the rule "the delimiter is never a member".  No test runs this script; tests import its
functions.
"""
import hashlib
import json
import os
import re
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = "data/i386.txt"
KEEP = 8
DELIMITER = 10
# (name, item, quantifier, ignore_case)
CASES = [
    ("words", r"\w", "+", False),
    ("numbers", r"[0-9]", "+", False),
    ("wc_w", r"\S", "+", False),
    ("three_digits_or_more", r"[0-9]", "{3,}", False),
    ("eight_word_bytes_or_more", r"\w", "{8,}", False),
    ("two_blanks_or_more", r" ", "{2,}", False),
    ("long_lines", r"[^\n]", "{80,}", False),
    ("exactly_three_digits", r"[0-9]", "{3}", False),
    ("two_to_five_capitals", r"[A-Z]", "{2,5}", False),
    ("words_nocase", r"\w", "+", True),
    ("numbers_nocase", r"[0-9]", "+", True),
    ("wc_w_nocase", r"\S", "+", True),
    ("three_digits_or_more_nocase", r"[0-9]", "{3,}", True),
    ("eight_word_bytes_or_more_nocase", r"\w", "{8,}", True),
    ("two_blanks_or_more_nocase", r" ", "{2,}", True),
    ("long_lines_nocase", r"[^\n]", "{80,}", True),
    ("exactly_three_digits_nocase", r"[0-9]", "{3}", True),
    ("two_to_five_capitals_nocase", r"[A-Z]", "{2,5}", True),
    ("hex_runs_nocase", r"[a-f0-9]", "{4,8}", True),
]


def to_regex(item, quantifier, ignore_case):
    c = item.encode("latin-1")
    return re.compile(b"(?<!" + c + b")" + c + quantifier.encode("latin-1") + b"(?!" + c + b")", re.S | (re.I if ignore_case else 0))


def runs_of(data, item, quantifier, ignore_case):
    """[(begin, end)] of the selected runs"""
    return [m.span() for m in to_regex(item, quantifier, ignore_case).finditer(data)]


def lines_of(data, item, quantifier, ignore_case, delimiter):
    rx = to_regex(item, quantifier, ignore_case)
    return sum(1 for piece in data.split(bytes([delimiter])) if rx.search(piece))


def list_hash(runs):
    return hashlib.sha256(b"".join(struct.pack("<Q", b) for b, _ in runs) + b"".join(struct.pack("<Q", e) for _, e in runs)).hexdigest()


def make(data):
    cases = []
    for name, item, quantifier, ignore_case in CASES:
        runs = runs_of(data, item, quantifier, ignore_case)
        cases.append({"name": name, "pattern": item + quantifier, "ignore_case": ignore_case, "delimiter": DELIMITER, "count": len(runs),
                      "lines": lines_of(data, item, quantifier, ignore_case, DELIMITER), "runs_sha256": list_hash(runs),
                      "first": [list(r) for r in runs[:KEEP]], "last": [list(r) for r in runs[-KEEP:]]})
    return {"file": FILE, "bytes": len(data),
            "lists": "runs_sha256 is the SHA-256 of all begins followed by all ends as little-endian 64-bit words; first and last hold "
                     "%d (begin, end) pairs each" % KEEP, "cases": cases}


def main():
    data = open(os.path.join(HERE, FILE), "rb").read()
    kat = make(data)
    with open(os.path.join(HERE, "runs_kat.json"), "w") as f:
        f.write("{\n")
        for key in ("file", "bytes", "lists"):
            f.write(" %s: %s,\n" % (json.dumps(key), json.dumps(kat[key])))
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in kat["cases"]) + "\n ]\n}\n")
    for c in kat["cases"]:
        print("%-34s %8d runs %8d lines" % (c["name"], c["count"], c["lines"]))


if __name__ == "__main__":
    main()
