#!/usr/bin/env python3
"""Regenerates tests/golden/masked_kat.json, the known answers of the masked-pattern calls (include/sliceslice_hip_masked.h).

    python tests/golden/make_masked_golden.py

An INDEPENDENT reference: every hex pattern is turned into a Python ``re`` bytes pattern - ``??`` becomes ``.`` (with ``re.S``), a
byte with a partial mask becomes a character class of the values it accepts, a full byte its escaped literal - inside a lookahead,
so that occurrences overlap.  It runs over data/i386.txt.  A case holds the count, the offsets (a list of more than 512 as the
SHA-256 of its little-endian 64-bit words with both ends, as disjoint_kat.json does) and the number of lines that hold an
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
KEEP = 512
# (name, hex pattern, delimiter)
CASES = [
    ("descriptor_gaps", "64 ?? 73 63 72 ?? ?? 74 6f 72", 10),           # d?scr??tor
    ("t_any_e", "74 ?? 65", 10),                                        # t?e
    ("three_digit_nibbles", "3? 3? 3?", 10),
    ("intel_any_case", None, 10),                                       # letter masks 0xDF (filled in below)
    ("dot_any_newline", "2e ?? 0a", 10),                                # the occurrence includes the delimiter: no line
    ("one_wildcard", "??", 10),                                         # every position; every line that is not empty
    ("two_wildcards", "?? ??", 10),
    ("low_nibble_only", "?0 ?d", 10),
    ("space_delimited", "74 ?? 65", 32),                                # the same pattern with ' ' as the delimiter
]


def parse_hex(text):
    """(value, mask) of a hex pattern: tokens of two characters, each a hex digit or '?'."""
    value, mask = bytearray(), bytearray()
    for token in text.split():
        assert len(token) == 2, token
        v = m = 0
        for ch in token:
            v, m = (v << 4) | (0 if ch == "?" else int(ch, 16)), (m << 4) | (0 if ch == "?" else 15)
        value.append(v)
        mask.append(m)
    return bytes(value), bytes(mask)


def letter_masks(word):
    return bytes(word), bytes(0xDF if chr(b).isalpha() else 0xFF for b in word)


def to_regex(value, mask):
    """The ``re`` bytes pattern of (value, mask), in a lookahead."""
    body = b""
    for v, m in zip(value, mask):
        if m == 0:
            body += b"."
        elif m == 0xFF:
            body += re.escape(bytes([v]))
        else:
            body += b"[" + b"".join(b"\\x%02x" % b for b in range(256) if b & m == v & m) + b"]"
    return re.compile(b"(?=" + body + b")", re.S)


def offsets_of(data, value, mask):
    n = len(value)
    return [m.start() for m in to_regex(value, mask).finditer(data) if m.start() + n <= len(data)]


def lines_of(data, value, mask, delimiter):
    """The number of lines that hold an occurrence wholly inside them (a last line without a delimiter counts as a line)."""
    rx, n = to_regex(value, mask), len(value)
    return sum(1 for piece in data.split(bytes([delimiter])) if any(m.start() + n <= len(piece) for m in rx.finditer(piece)))


def list_hash(offsets):
    return hashlib.sha256(b"".join(struct.pack("<Q", o) for o in offsets)).hexdigest()


def make(data):
    cases = []
    for name, text, delimiter in CASES:
        value, mask = letter_masks(b"intel") if text is None else parse_hex(text)
        offsets = offsets_of(data, value, mask)
        case = {"name": name, "value": value.hex(), "mask": mask.hex(), "delimiter": delimiter, "count": len(offsets),
                "lines": lines_of(data, value, mask, delimiter)}
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
    with open(os.path.join(HERE, "masked_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")
    for c in kat["cases"]:
        print("%-22s %8d occurrences %8d lines" % (c["name"], c["count"], c["lines"]))


if __name__ == "__main__":
    main()
