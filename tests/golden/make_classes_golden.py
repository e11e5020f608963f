#!/usr/bin/env python3
"""Regenerates tests/golden/classes_kat.json, the known answers of the byte-class calls (include/sliceslice_hip_classes.h).

    python tests/golden/make_classes_golden.py

An INDEPENDENT reference: the pattern language is a strict subset of Python ``re`` byte patterns under ``re.S``, so every pattern is
handed to ``re`` as it stands, inside a lookahead with a group - ``(?=(...))`` - so that occurrences overlap and an occurrence that
would run past the end is no match.  It runs over data/i386.txt.  A case holds the count, the offsets (a list of more than 160 as
the SHA-256 of its little-endian 64-bit words with both ends, as masked_kat.json does) and the number of lines that hold an
occurrence wholly inside them: the text is ``split`` at the delimiter and every piece searched on its own.  No test runs this
script; tests import its functions.
"""
import hashlib
import json
import os
import re
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = "data/i386.txt"
KEEP = 160
# (name, pattern, ignore_case, delimiter)
CASES = [
    ("three_digits", r"[0-9]{3}", False, 10),
    ("four_digits", r"\d{4}", False, 10),
    ("hex_word", r"[0-9A-F]{4}H", False, 10),
    ("figure_number", r"[Ff]igure \d\d-\d", False, 10),
    ("clock", r"\d\d:\d\d", False, 10),
    ("not_printable", r"[^ -~\n]", False, 10),
    ("eight_word_bytes", r"\w{8}", False, 10),
    ("the_between_non_letters", r"[^a-z]the[^a-z]", False, 10),
    ("two_blanks", r"\s\s", False, 10),                                 # \s accepts the delimiter: such an occurrence is in no line
    ("three_vowels", r"[aeiou]{3}", False, 10),
    ("a_any_b", r"a.b", False, 10),
    ("a_any_b_nocase", r"a.b", True, 10),
    ("a_to_c_x", r"[a-c]x", False, 10),
    ("a_to_c_x_nocase", r"[a-c]x", True, 10),
    ("clock_space_delimited", r"\d\d:\d\d", False, 32),
]


def to_regex(pattern, ignore_case):
    return re.compile(b"(?=(" + pattern.encode("latin-1") + b"))", re.S | (re.I if ignore_case else 0))


def offsets_of(data, pattern, ignore_case):
    return [m.start() for m in to_regex(pattern, ignore_case).finditer(data)]


def lines_of(data, pattern, ignore_case, delimiter):
    """The number of lines that hold an occurrence wholly inside them (a last line without a delimiter counts as a line)."""
    rx = to_regex(pattern, ignore_case)
    return sum(1 for piece in data.split(bytes([delimiter])) if rx.search(piece))


def list_hash(offsets):
    return hashlib.sha256(b"".join(struct.pack("<Q", o) for o in offsets)).hexdigest()


def make(data):
    cases = []
    for name, pattern, ignore_case, delimiter in CASES:
        offsets = offsets_of(data, pattern, ignore_case)
        case = {"name": name, "pattern": pattern, "ignore_case": ignore_case, "delimiter": delimiter, "count": len(offsets),
                "lines": lines_of(data, pattern, ignore_case, delimiter)}
        if len(offsets) > KEEP:
            case.update(offsets_sha256=list_hash(offsets), first=offsets[:16], last=offsets[-16:])
        else:
            case["offsets"] = offsets
        cases.append(case)
    return {"file": FILE, "bytes": len(data),
            "lists": "a list of more than %d offsets is held as the SHA-256 of its offsets as little-endian 64-bit words, with its first "
                     "and last 16" % KEEP, "cases": cases}


def main():
    data = open(os.path.join(HERE, FILE), "rb").read()
    kat = make(data)
    with open(os.path.join(HERE, "classes_kat.json"), "w") as f:
        f.write("{\n")
        for key in ("file", "bytes", "lists"):
            f.write(" %s: %s,\n" % (json.dumps(key), json.dumps(kat[key])))
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in kat["cases"]) + "\n ]\n}\n")
    for c in kat["cases"]:
        print("%-26s %8d occurrences %8d lines" % (c["name"], c["count"], c["lines"]))


if __name__ == "__main__":
    main()
