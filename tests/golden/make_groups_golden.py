"""Writes tests/golden/groups_kat.json: what plain Python - re.finditer, bytes.split, collections.Counter - says about the distinct
tokens and lines of tests/golden/data/i386.txt, for the grouping calls of include/sliceslice_hip_groups.h to be checked against.

    python tests/golden/make_groups_golden.py

A case is a list of keys in input order.  Recorded per case: the number of keys and of distinct keys, the most frequent key, the
first 40 and the last 5 rows (key, first, count) of the Counter filled in input order - `first` is the index of the key's first
occurrence in the list - and the SHA-256 over all rows."""
import collections
import hashlib
import json
import os
import re
import struct

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
FILE = "i386.txt"
HEAD, TAIL = 40, 5
# name, the pattern of the tokens (None: the lines), folded
CASES = [("word", rb"\w+", False), ("word_folded", rb"\w+", True), ("digits", rb"[0-9]+", False), ("nonspace", rb"\S+", False),
         ("lines", None, False), ("lines_folded", None, True)]


def fold(key):
    """bytes.lower() touches 'A'..'Z' alone, like the library's fold"""
    return key.lower()


def ranges(data, pattern, delimiter=b"\n"):
    """(begin, end) of every token of `pattern`, or of every line: empty lines are lines, the last one counts only if it has bytes"""
    if pattern is not None:
        return [m.span() for m in re.finditer(pattern, data)]
    out, at = [], 0
    pieces = data.split(delimiter)
    if pieces[-1] == b"":
        pieces.pop()
    for piece in pieces:
        out.append((at, at + len(piece)))
        at += len(piece) + 1
    return out


def rows(keys):
    """[(key, first, count)] of a Counter filled in input order"""
    first, count = {}, collections.Counter()
    for k, key in enumerate(keys):
        first.setdefault(key, k)
        count[key] += 1
    return [(key, first[key], count[key]) for key in count]


def digest(table):
    h = hashlib.sha256()
    for key, first, count in table:
        h.update(struct.pack("<qqq", len(key), first, count) + key)
    return h.hexdigest()


def make(data):
    cases = []
    for name, pattern, folded in CASES:
        spans = ranges(data, pattern)
        keys = [fold(data[b:e]) if folded else data[b:e] for b, e in spans]
        table = rows(keys)
        top = max(table, key=lambda r: (r[2], -r[1]))
        show = lambda r: [r[0].decode("latin-1"), r[1], r[2]]          # noqa: E731
        cases.append({"name": name, "pattern": pattern.decode() if pattern else None, "folded": folded, "keys": len(keys), "groups": len(table),
                      "top": show(top), "head": [show(r) for r in table[:HEAD]], "tail": [show(r) for r in table[-TAIL:]],
                      "sha256": digest(table)})
    return {"file": FILE, "bytes": len(data),
            "rows": "a row is (key, first, count): the key as latin-1 text, the index of its first occurrence in the list of keys and "
                    "its occurrences, in first-occurrence order; sha256 is over len(key), first, count as little-endian int64 and the "
                    "key's bytes, row after row", "cases": cases}


def main():
    data = open(os.path.join(HERE, FILE), "rb").read()
    kat = make(data)
    with open(os.path.join(os.path.dirname(HERE), "groups_kat.json"), "w") as f:
        f.write("{\n")
        for key in ("file", "bytes", "rows"):
            f.write(" %s: %s,\n" % (json.dumps(key), json.dumps(kat[key])))
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in kat["cases"]) + "\n ]\n}\n")
    for c in kat["cases"]:
        print("%-14s %8d keys %8d groups, top %r" % (c["name"], c["keys"], c["groups"], c["top"]))


if __name__ == "__main__":
    main()
