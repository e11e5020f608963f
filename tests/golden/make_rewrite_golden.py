#!/usr/bin/env python3
"""Regenerates tests/golden/rewrite_kat.json, the known answers of the rewrite call (include/sliceslice_hip_rewrite.h).

    python tests/golden/make_rewrite_golden.py

An INDEPENDENT reference: the header states the output in ``re`` terms - ``re.sub(rb"(?<![C])[C]{min,max}(?![C])", replacement,
view)`` - so exactly that is handed to ``re`` (bytes, ``re.S``), over data/i386.txt.  With a delimiter the text is ``split`` at it,
every piece substituted on its own and the pieces joined by it again, which is the rule "the delimiter is never a member, and a
delimiter is always copied".  A case holds the number of selected runs, the output's length, its SHA-256 and its first and last 64
bytes as hex.  No test runs this script; tests import its functions.
"""
import hashlib
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = "data/i386.txt"
KEEP = 64
# (name, item, quantifier, text, delimiter or None)
CASES = [
    ("squeeze_blanks", r" ", "{2,}", b" ", None),
    ("numbers_to_N", r"[0-9]", "+", b"N", None),
    ("three_digits_to_num", r"[0-9]", "{3}", b"<num>", None),
    ("delete_space", r"\s", "+", b"", None),
    ("delete_short_words", r"\w", "{2,5}", b"", None),
    ("blank_long_lines", r"[^\n]", "{80,}", b"...", None),
    ("delete_words", r"\w", "+", b"", None),
    ("squeeze_space_per_line", r"\s", "+", b" ", 10),
]
SAME_OUTPUT = ("squeeze_space_per_line", "squeeze_blanks")


def to_regex(item, quantifier):
    c = item.encode("latin-1")
    return re.compile(b"(?<!" + c + b")" + c + quantifier.encode("latin-1") + b"(?!" + c + b")", re.S)


def sub(data, item, quantifier, text, delimiter=None):
    """(the output, the number of selected runs)"""
    rx = to_regex(item, quantifier)
    if delimiter is None:
        return rx.subn(lambda m: text, data)
    d = bytes([delimiter])
    pieces = [rx.subn(lambda m: text, piece) for piece in data.split(d)]
    return d.join(p for p, _ in pieces), sum(k for _, k in pieces)


def make(data):
    cases = []
    for name, item, quantifier, text, delimiter in CASES:
        out, count = sub(data, item, quantifier, text, delimiter)
        cases.append({"name": name, "pattern": item + quantifier, "text": text.decode("latin-1"), "delimiter": delimiter, "count": count,
                      "out_len": len(out), "sha256": hashlib.sha256(out).hexdigest(), "first": out[:KEEP].hex(), "last": out[-KEEP:].hex()})
    return {"file": FILE, "bytes": len(data),
            "outputs": "sha256 is the SHA-256 of the output; first and last hold its first and last %d bytes as hex; the output of %s is "
                       "the same bytes as that of %s: in the manual every run of white space of two bytes or more inside a line is "
                       "blanks" % ((KEEP,) + SAME_OUTPUT), "cases": cases}


def main():
    data = open(os.path.join(HERE, FILE), "rb").read()
    kat = make(data)
    with open(os.path.join(HERE, "rewrite_kat.json"), "w") as f:
        f.write("{\n")
        for key in ("file", "bytes", "outputs"):
            f.write(" %s: %s,\n" % (json.dumps(key), json.dumps(kat[key])))
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in kat["cases"]) + "\n ]\n}\n")
    for c in kat["cases"]:
        print("%-26s %8d runs %8d bytes" % (c["name"], c["count"], c["out_len"]))


if __name__ == "__main__":
    main()
