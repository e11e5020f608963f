#!/usr/bin/env python3
"""Regenerates tests/golden/lines_kat.json, the known answers of the matching-lines calls (include/sliceslice_hip_lines.h).

    python tests/golden/make_lines_golden.py

Pure Python over tests/golden/data/ - ``data.split(delimiter)`` and ``needle in line`` - with no other code involved.

* ``i386_lines`` / ``count_lines`` / ``total`` - the number of lines of data/i386.txt, and per word of data/words.txt (in file
  order) the number of lines that contain it; their sum.
* ``records`` - for about fifty chosen words the number of matching lines and the sha256 of their (begin, end, number) triples,
  packed as little-endian 64-bit integers in that order, line after line.
* ``cases`` - a hand-written table of small haystacks covering every rule of the header comment, with the expected records written
  out by hand; this script refuses to write the file unless the rule reproduces them.
"""
import hashlib
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))


def lines_of(data, needle, delimiter):
    """[(begin, end, number)] of the lines of `data` that contain `needle` - the rule of the header, restated naively."""
    pieces = data.split(bytes([delimiter]))
    if pieces[-1] == b"":
        pieces.pop()                    # nothing behind the last delimiter (or an empty haystack): no such line
    out, begin = [], 0
    for k, piece in enumerate(pieces):
        if needle in piece:
            out.append((begin, begin + len(piece), k + 1))
        begin += len(piece) + 1
    return out


def checksum(records):
    return hashlib.sha256(b"".join(struct.pack("<3Q", *r) for r in records)).hexdigest()


# (what it shows, haystack, needle, delimiter, expected records) - haystack and needle as latin-1 strings
CASES = [
    ("empty haystack", "", "a", 10, []),
    ("empty haystack, empty needle", "", "", 10, []),
    ("only delimiters: three empty lines, none holds a byte", "\n\n\n", "a", 10, []),
    ("only delimiters, empty needle: every empty line matches", "\n\n\n", "", 10, [(0, 0, 1), (1, 1, 2), (2, 2, 3)]),
    ("no trailing delimiter: the last line ends at len", "ab\ncab", "ab", 10, [(0, 2, 1), (3, 6, 2)]),
    ("trailing delimiter: no empty last line", "ab\ncab\n", "ab", 10, [(0, 2, 1), (3, 6, 2)]),
    ("empty needle counts the lines, the empty one included", "x\n\nyz", "", 10, [(0, 1, 1), (2, 2, 2), (3, 5, 3)]),
    ("a line counts once however many occurrences it holds", "aaaa\nba\naaa", "aa", 10, [(0, 4, 1), (8, 11, 3)]),
    ("an occurrence must lie wholly inside one line", "ab\ncd", "b\nc", 10, []),
    ("needle equal to the delimiter", "a\nb\n", "\n", 10, []),
    ("needle ending in the delimiter", "a\nb\n", "a\n", 10, []),
    ("line numbers count the lines in between", "no\nno\nyes\nno\nyes", "yes", 10, [(6, 9, 3), (13, 16, 5)]),
    ("delimiter 0x00 (grep -z)", "a\x00bb\x00a\x00", "a", 0, [(0, 1, 1), (5, 6, 3)]),
    ("delimiter 0x00: a newline is an ordinary byte", "a\nb\x00c", "a\nb", 0, [(0, 3, 1)]),
    ("delimiter 0xFF", "k\xffkk\xff\xffk", "kk", 255, [(2, 4, 2)]),
    ("delimiter 0xFF, empty needle", "k\xffkk\xff\xffk", "", 255, [(0, 1, 1), (2, 4, 2), (5, 5, 3), (6, 7, 4)]),
    ("needle longer than the haystack", "ab\n", "abcd", 10, []),
    ("needle as long as the haystack", "abcd", "abcd", 10, [(0, 4, 1)]),
    ("first byte is a delimiter", "\nab", "ab", 10, [(1, 3, 2)]),
    ("a one-byte needle", "xax\nxxx\na", "a", 10, [(0, 3, 1), (8, 9, 3)]),
    ("an ordinary letter as delimiter", "onetwothree", "w", ord("t"), [(4, 6, 2)]),
]

# words whose records are pinned: frequent, rare, absent, one byte, long, with blanks and punctuation
RECORD_WORDS = ["the", "e", "a", "A", "of", "is", "in", "instruction", "instructions", "segment", "descriptor", "privilege", "INTEL",
                "Intel", "386", "80386", "register", "registers", "memory", "operand", "operands", "flag", "flags", "page", "task",
                "interrupt", "exception", "protected", "mode", "real", "virtual", "address", "byte", "word", "doubleword", "stack",
                "pointer", "selector", "gate", "call", "jump", "return", "zero", "Zz", "xyzzy", " ", ".", "  ", "the ", " the ", "tion"]


def main():
    data = open(os.path.join(HERE, "data", "i386.txt"), "rb").read()
    words = open(os.path.join(HERE, "data", "words.txt"), "rb").read().split(b"\n")
    if words[-1] == b"":
        words.pop()
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    counts = [sum(1 for line in lines if w in line) for w in words]
    records = {}
    for w in RECORD_WORDS:
        r = lines_of(data, w.encode("latin-1"), 10)
        records[w] = {"lines": len(r), "sha256": checksum(r)}
    cases = []
    for what, hay, needle, delim, expected in CASES:
        got = lines_of(hay.encode("latin-1"), needle.encode("latin-1"), delim)
        assert got == expected, (what, got, expected)
        cases.append({"what": what, "haystack": hay.encode("latin-1").hex(), "needle": needle.encode("latin-1").hex(),
                      "delimiter": delim, "records": [list(r) for r in expected]})
    out = {"i386_lines": len(lines), "words": len(words), "total": sum(counts), "count_lines": counts, "records": records, "cases": cases}
    assert out["i386_lines"] == 20854 and out["words"] == 4585 and out["total"] == 410509, (out["i386_lines"], out["words"], out["total"])
    with open(os.path.join(HERE, "lines_kat.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("lines_kat.json:", out["i386_lines"], "lines,", out["words"], "words,", out["total"], "matching lines,", len(records), "record sets,",
          len(cases), "cases")


if __name__ == "__main__":
    main()
