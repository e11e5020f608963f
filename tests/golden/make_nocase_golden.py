#!/usr/bin/env python3
"""Regenerates tests/golden/nocase_kat.json, the known answers of the calls that ignore ASCII case (include/sliceslice_hip_nocase.h).

    python tests/golden/make_nocase_golden.py

Pure Python over tests/golden/data/: ``bytes.lower()`` on the haystack and on the needle, then the overlapping count and the
matching-lines rule of make_lines_golden.py - with the line cut made on the UNFOLDED bytes, because the delimiter is never folded.

* ``count`` / ``count_lines`` - per word of data/words.txt (in file order) the occurrences and the matching lines of data/i386.txt
  ignoring case; ``total_count`` / ``total_lines`` their sums; ``differ`` how many words get another presence or count than the
  case-sensitive search gives them.
* ``table`` - the figures quoted in DESIGN.md 5.9 for `descriptor`, `the` and `intel`, sensitive and ignoring case.
* ``records`` - for about fifty words the number of occurrences and of matching lines ignoring case and the sha256 of the offsets
  (little-endian 64-bit) and of the (begin, end, number) triples.
* ``cases`` - a hand-written table of small haystacks covering the fold's edges and the delimiter rule, with the expected offsets and
  records written out by hand; this script refuses to write the file unless the rule reproduces them.
"""
import hashlib
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))


def offsets_of(data, needle):
    """every i with data[i:i+len(needle)].lower() == needle.lower(), overlapping, ascending"""
    h, n = data.lower(), needle.lower()
    out, i = [], h.find(n)
    while i >= 0:
        out.append(i)
        i = h.find(n, i + 1)
    return out


def lines_of(data, needle, delimiter):
    """[(begin, end, number)] of the lines of `data` (cut at the delimiter byte AS IT IS) that contain `needle` ignoring case.  The
    needle a searcher holds is the folded one, and - as in the case-sensitive call - a needle that holds the delimiter matches no line."""
    pieces = data.split(bytes([delimiter]))
    if pieces[-1] == b"":
        pieces.pop()
    n = needle.lower()
    out, begin = [], 0
    for k, piece in enumerate(pieces):
        if delimiter not in n and n in piece.lower():
            out.append((begin, begin + len(piece), k + 1))
        begin += len(piece) + 1
    return out


def sha_offsets(offs):
    return hashlib.sha256(b"".join(struct.pack("<Q", o) for o in offs)).hexdigest()


def sha_records(records):
    return hashlib.sha256(b"".join(struct.pack("<3Q", *r) for r in records)).hexdigest()


# (what it shows, haystack, needle, delimiter, expected offsets, expected records) - haystack and needle as latin-1 strings
CASES = [
    ("letters match in either case", "abc ABC aBc", "abc", 10, [0, 4, 8], [(0, 11, 1)]),
    ("an upper-case needle is folded too", "abc ABC", "AbC", 10, [0, 4], [(0, 7, 1)]),
    ("overlapping occurrences in mixed case", "aAaA", "aa", 10, [0, 1, 2], [(0, 4, 1)]),
    ("'@' (0x40) is not '`' (0x60)", "@`", "`", 10, [1], [(0, 2, 1)]),
    ("'[' (0x5B) is not '{' (0x7B)", "[{", "{", 10, [1], [(0, 2, 1)]),
    ("'`' does not match '@' either", "`@", "@", 10, [1], [(0, 2, 1)]),
    ("'{' does not match '[' either", "{[", "[", 10, [1], [(0, 2, 1)]),
    ("bytes 0xC1 / 0xE1 look like 'A' / 'a' in seven bits and are neither", "\xc1\xe1aA", "a", 10, [2, 3], [(0, 4, 1)]),
    ("0xC1 does not match 0xE1", "\xc1\xe1", "\xe1", 10, [1], [(0, 2, 1)]),
    ("0xDA / 0xFA, the other end of the range", "\xda\xfazZ", "z", 10, [2, 3], [(0, 4, 1)]),
    ("digits and blanks compare exactly", "a1 A1 a! A\x11", "a1", 10, [0, 3], [(0, 11, 1)]),
    ("empty needle: len + 1 offsets, every line", "A\na", "", 10, [0, 1, 2, 3], [(0, 1, 1), (2, 3, 2)]),
    ("needle longer than the haystack", "Ab", "abc", 10, [], []),
    ("lines: a line counts once", "Ab aB\nxx\nAB", "ab", 10, [0, 3, 9], [(0, 5, 1), (9, 11, 3)]),
    ("the delimiter is not folded: 'A' cuts at 'A' only", "xaxAxa", "x", ord("A"), [0, 2, 4], [(0, 3, 1), (4, 6, 2)]),
    ("needle 'a' with delimiter 'A': the other case of the delimiter can match", "baAbbAa", "a", ord("A"), [1, 2, 5, 6],
     [(0, 2, 1), (6, 7, 3)]),
    ("needle 'A' with delimiter 'A': the searcher holds the folded 'a', which is not the delimiter", "baAbbAa", "A", ord("A"), [1, 2, 5, 6],
     [(0, 2, 1), (6, 7, 3)]),
    ("needle 'a' with delimiter 'a': a needle that holds the delimiter matches no line, whatever the lines hold", "bAabbaA", "a", ord("a"),
     [1, 2, 5, 6], []),
    ("needle 'A' with delimiter 'a': folded, it holds the delimiter", "bAabbaA", "A", ord("a"), [1, 2, 5, 6], []),
    ("delimiter 0x00", "Ab\x00aB\x00c", "AB", 0, [0, 3], [(0, 2, 1), (3, 5, 2)]),
    ("delimiter 0xFF", "Ab\xffc\xffaB", "ab", 255, [0, 5], [(0, 2, 1), (5, 7, 3)]),
    ("an occurrence must lie wholly inside one line", "A\nb", "a\nb", 10, [0], []),
]

RECORD_WORDS = ["the", "The", "THE", "e", "a", "A", "of", "is", "in", "instruction", "instructions", "segment", "descriptor", "Descriptor",
                "privilege", "INTEL", "Intel", "intel", "386", "80386", "register", "registers", "memory", "operand", "operands", "flag",
                "flags", "page", "task", "interrupt", "exception", "protected", "mode", "real", "virtual", "address", "byte", "word",
                "doubleword", "stack", "pointer", "selector", "gate", "call", "jump", "return", "zero", "Zz", "xyzzy", " ", ".", "the ",
                " the ", "tion", "TION"]


def main():
    cases = []
    for what, hay, needle, delim, offs, recs in CASES:
        h, n = hay.encode("latin-1"), needle.encode("latin-1")
        got_o, got_r = offsets_of(h, n), lines_of(h, n, delim)
        if n == b"":
            got_o = list(range(len(h) + 1))
        assert got_o == offs and got_r == recs, (what, got_o, offs, got_r, recs)
        cases.append({"what": what, "haystack": h.hex(), "needle": n.hex(), "delimiter": delim, "offsets": offs,
                      "records": [list(r) for r in recs]})
    data = open(os.path.join(HERE, "data", "i386.txt"), "rb").read()
    words = open(os.path.join(HERE, "data", "words.txt"), "rb").read().split(b"\n")
    if words[-1] == b"":
        words.pop()
    low = data.lower()
    low_lines = low.split(b"\n")
    if low_lines[-1] == b"":
        low_lines.pop()                 # ('\n' is no letter: the folded text's lines are the text's lines, folded)
    raw_lines = data.split(b"\n")[:len(low_lines)]

    def count(h, n):
        c, i = 0, h.find(n)
        while i >= 0:
            c, i = c + 1, h.find(n, i + 1)
        return c

    counts = [count(low, w.lower()) for w in words]
    line_counts = [sum(1 for l in low_lines if w.lower() in l) for w in words]
    differ = sum(1 for w, c in zip(words, counts) if c != count(data, w))
    table = {}
    for w in (b"descriptor", b"the", b"intel"):
        table[w.decode()] = {"count": count(data, w), "count_nocase": count(low, w),
                             "lines": sum(1 for l in raw_lines if w in l), "lines_nocase": sum(1 for l in low_lines if w in l)}
    records = {}
    for w in RECORD_WORDS:
        o, r = offsets_of(data, w.encode("latin-1")), lines_of(data, w.encode("latin-1"), 10)
        records[w] = {"count": len(o), "offsets_sha256": sha_offsets(o), "lines": len(r), "records_sha256": sha_records(r)}
    out = {"words": len(words), "total_count": sum(counts), "total_lines": sum(line_counts), "differ": differ, "count": counts,
           "count_lines": line_counts, "table": table, "records": records, "cases": cases}
    assert out["words"] == 4585 and differ == 2427, (out["words"], differ)
    assert table == {"descriptor": {"count": 355, "count_nocase": 480, "lines": 337, "lines_nocase": 458},
                     "the": {"count": 7398, "count_nocase": 9008, "lines": 4801, "lines_nocase": 5489},
                     "intel": {"count": 5, "count_nocase": 44, "lines": 3, "lines_nocase": 36}}, table
    with open(os.path.join(HERE, "nocase_kat.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("nocase_kat.json:", out["words"], "words,", out["total_count"], "occurrences,", out["total_lines"], "matching lines,", differ,
          "words differ,", len(records), "record sets,", len(cases), "cases")


if __name__ == "__main__":
    main()
