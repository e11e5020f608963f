#!/usr/bin/env python3
"""Regenerates tests/golden/fields_kat.json, the known answers of the field calls (include/sliceslice_hip_fields.h).

    python tests/golden/make_fields_golden.py

An INDEPENDENT reference, in plain Python over data/i386.txt: the view is ``split`` at the delimiter (a trailing empty piece is no
line), a line's fields are ``bytes.split`` (one separator) or ``re.split`` (a class) of it in EACH mode and the non-empty pieces of
``re.split`` over runs of the class in MERGE mode, and a walk over the pieces' lengths gives the offsets.  A case holds the number of
records, of selected lines and of lines, and the SHA-256 of the three arrays (begin, end, number as little-endian int64, one array
after the other) - not the arrays.  No test runs this script; tests import its functions.
"""
import hashlib
import json
import os
import re
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = "data/i386.txt"
EACH, MERGE = 0, 1
# (name, separator as a classes-language item, its members, mode, cut's range)
SELECTIONS = [
    ("blank_each_2", " ", b" ", EACH, "2"),
    ("space_merge_1", r"[ \t]", b" \t", MERGE, "1"),
    ("space_merge_2", r"[ \t]", b" \t", MERGE, "2"),
    ("space_merge_3_5", r"[ \t]", b" \t", MERGE, "3-5"),
    ("space_merge_7_", r"[ \t]", b" \t", MERGE, "7-"),
    ("dot_each_1_2", r"\.", b".", EACH, "1-2"),
]


def parse_range(text):
    """cut's single range -> (first, last), last 0: to the line's end"""
    lo, dash, hi = text.partition("-")
    first = int(lo) if lo else 1
    return first, (first if not dash else (int(hi) if hi else 0))


def line_fields(line, members, mode):
    """[(begin, end)] of the line's fields, relative to its first byte"""
    members = bytes(sorted(set(members)))
    if not members:
        return [(0, len(line))] if mode == EACH or line else []
    cls = b"[" + b"".join(re.escape(bytes([m])) for m in members) + b"]"
    out, at = [], 0
    if mode == EACH:
        for piece in (line.split(members) if len(members) == 1 else re.split(cls, line)):
            out.append((at, at + len(piece)))
            at += len(piece) + 1
    else:
        for k, piece in enumerate(re.split(b"(" + cls + b"+)", line)):      # field, separators, field, ...
            if k % 2 == 0 and piece:
                out.append((at, at + len(piece)))
            at += len(piece)
    return out


def records(data, members, mode, first, last, keep_short=False, delimiter=10):
    """(begin, end, number) lists and the number of lines"""
    members = bytes(m for m in set(members) if m != delimiter)
    lines = data.split(bytes([delimiter]))
    if lines[-1] == b"":
        lines.pop()
    begin, end, number, at = [], [], [], 0
    for k, line in enumerate(lines, 1):
        fields, stop = line_fields(line, members, mode), at + len(line)
        if len(fields) >= first:
            begin.append(at + fields[first - 1][0])
            end.append(at + fields[last - 1][1] if last and len(fields) >= last else stop)
            number.append(k)
        elif keep_short:
            begin.append(stop)
            end.append(stop)
            number.append(k)
        at = stop + 1
    return begin, end, number, len(lines)


def digest(begin, end, number):
    h = hashlib.sha256()
    for column in (begin, end, number):
        h.update(struct.pack("<%dq" % len(column), *column))
    return h.hexdigest()


def make(data):
    cases = []
    for name, item, members, mode, text in SELECTIONS:
        first, last = parse_range(text)
        selected = len(records(data, members, mode, first, last)[0])
        for keep in (False, True):
            b, e, n, lines = records(data, members, mode, first, last, keep)
            cases.append({"name": name + ("_keep_short" if keep else ""), "separator": item, "members": members.decode("latin-1"),
                          "mode": mode, "fields": text, "first": first, "last": last, "keep_short": keep, "records": len(b),
                          "selected": selected, "lines": lines, "bytes_selected": sum(y - x for x, y in zip(b, e)), "sha256": digest(b, e, n)})
    return {"file": FILE, "bytes": len(data),
            "records": "sha256 is the SHA-256 of begin, end and number as little-endian int64, one array after the other; with "
                       "keep_short there is one record per line", "cases": cases}


def main():
    data = open(os.path.join(HERE, FILE), "rb").read()
    kat = make(data)
    with open(os.path.join(HERE, "fields_kat.json"), "w") as f:
        f.write("{\n")
        for key in ("file", "bytes", "records"):
            f.write(" %s: %s,\n" % (json.dumps(key), json.dumps(kat[key])))
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in kat["cases"]) + "\n ]\n}\n")
    for c in kat["cases"]:
        print("%-28s %8d records %8d selected %8d lines" % (c["name"], c["records"], c["selected"], c["lines"]))


if __name__ == "__main__":
    main()
