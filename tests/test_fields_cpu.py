"""CPU checks of the field calls (include/sliceslice_hip_fields.h): ss_fields_parse accepts and refuses what the language says and
names the column; `rule_fields`, the numpy restatement of THE RULE that the GPU tests import, against hand-written cases, against
the plain-Python reference of the fixture's generator on random data and against the fixture's rows; the nineteenth library stands on
the rewrite one, in a mapping of its own; the header, the ctypes table, the Rust module and the library's exports agree symbol by
symbol; the refusals that need no device."""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_fields_golden as G          # noqa: E402

FIELDS = ["ss_count_fields_device", "ss_fields_free", "ss_fields_info", "ss_fields_new", "ss_fields_parse", "ss_find_fields_device"]
EACH, MERGE, KEEP_SHORT = 0, 1, 1


def members_of(sep_set):
    """The byte values of a separator set given as bytes of members or as four 64-bit words."""
    if isinstance(sep_set, (bytes, bytearray)):
        return sorted(set(bytes(sep_set)))
    words = [int(w) for w in np.asarray(sep_set, dtype=np.uint64).reshape(4)]
    return [b for b in range(256) if (words[b >> 6] >> (b & 63)) & 1]


def words_of(members):
    words = [0, 0, 0, 0]
    for b in members:
        words[b >> 6] |= 1 << (b & 63)
    return np.array(words, dtype=np.uint64)


def rule_fields(hay, sep_set, mode, first, last, flags=0, delimiter=10):
    """THE RULE in numpy: (begin, end, number) int64 arrays, and the number of lines as a fourth value.  What the GPU tests compare
    with.  Events are counted with prefix sums over the whole view; a line's count is the difference at its two ends."""
    a = np.frombuffer(bytes(hay) if not isinstance(hay, np.ndarray) else hay.tobytes(), dtype=np.uint8)
    n = a.size
    empty = np.zeros(0, dtype=np.int64)
    if n == 0:
        return empty, empty, empty, 0
    table = np.zeros(256, dtype=bool)
    table[members_of(sep_set)] = True
    table[delimiter] = False                                    # the delimiter is never a separator
    isd, sep = a == delimiter, table[a]
    stop = np.flatnonzero(isd)                                  # where every line ends
    if not isd[-1]:
        stop = np.append(stop, n)
    start = np.concatenate(([0], stop[:-1] + 1))
    lines = stop.size
    line_of = np.cumsum(isd) - isd                              # a delimiter belongs to the line it closes
    begin, end = np.full(lines, -1, dtype=np.int64), stop.astype(np.int64).copy()

    def ordinals(mask):
        """positions of the set bytes, their lines and their 0-based ordinals inside their lines"""
        at = np.flatnonzero(mask)
        before = np.concatenate(([0], np.cumsum(mask)))         # before[i]: set bytes in [0, i)
        return at, line_of[at], before[at] - before[start[line_of[at]]], before[np.minimum(stop, n)] - before[start]

    if mode == EACH:
        at, line, k, count = ordinals(sep)
        fields = count + 1
        if first == 1:
            begin[:] = start
        else:
            hit = k == first - 2
            begin[line[hit]] = at[hit] + 1
        if last:
            hit = k == last - 1
            end[line[hit]] = at[hit]
    else:
        field = ~sep & ~isd
        opens = field & ~np.concatenate(([False], field[:-1]))
        closes = field & ~np.concatenate((field[1:], [False]))
        at, line, k, fields = ordinals(opens)
        hit = k == first - 1
        begin[line[hit]] = at[hit]
        if last:
            at, line, k, _ = ordinals(closes)
            hit = k == last - 1
            end[line[hit]] = at[hit] + 1
    selected = fields >= first
    assert ((begin >= 0) == selected).all()
    number = np.arange(1, lines + 1, dtype=np.int64)
    if flags & KEEP_SHORT:
        begin = np.where(selected, begin, stop)
        end = np.where(selected, end, stop)
        return begin.astype(np.int64), end.astype(np.int64), number, lines
    return begin[selected], end[selected], number[selected], lines


def cut_bytes(hay, sep_set, mode, first, last, flags=0, delimiter=10, terminator=b"\n"):
    """what FieldSelector.cut returns"""
    data = bytes(hay)
    b, e, _, _ = rule_fields(data, sep_set, mode, first, last, flags, delimiter)
    return b"".join(data[x:y] + terminator for x, y in zip(b.tolist(), e.tolist()))


def _records(hay, sep, mode, first, last, flags=0, delimiter=10):
    b, e, n, lines = rule_fields(hay, sep, mode, first, last, flags, delimiter)
    return list(zip(b.tolist(), e.tolist(), n.tolist())), lines


# ---- the language ------------------------------------------------------------------------------------------------------------------
def test_parse_accepts_the_language_and_refusals_name_the_column():
    with ss.fields_build():
        for text, want in (("1", (1, 1)), ("7", (7, 7)), ("2-", (2, 0)), ("3-5", (3, 5)), ("-4", (1, 4)), ("5-5", (5, 5)),
                           ("18446744073709551615", (2 ** 64 - 1, 2 ** 64 - 1)), ("1-18446744073709551615", (1, 2 ** 64 - 1)), ("007-010", (7, 10))):
            assert ss.parse_fields(text) == want == G.parse_range(text), text
        for text, column, said in (("", 1, "empty"), ("0", 1, "numbered from 1"), ("0-3", 1, "numbered from 1"), ("2-0", 3, "numbered from 1"),
                                   ("5-3", 3, "M < K"), ("a", 1, "K, K-, K-M or -M"), ("2x", 2, "K, K-, K-M or -M"), ("2-3-4", 4, "K, K-, K-M or -M"),
                                   ("-", 2, "without a number"), ("1,3", 2, "one call per range"), ("1-2,4", 4, "one call per range"),
                                   (",2", 1, "one call per range"), ("2-,5", 3, "one call per range"), ("18446744073709551616", 1, "64 bits"),
                                   ("1-99999999999999999999", 3, "64 bits"), (" 2", 1, "K, K-, K-M or -M"), ("2 ", 2, "K, K-, K-M or -M"),
                                   ("1\0002", 2, "NUL")):
            with pytest.raises(ss.SlicesliceError, match=r"ss_fields_parse: column %d: " % column) as e:
                ss.parse_fields(text)
            assert e.value.code == ss.SS_ERR_ARGUMENT and said in str(e.value), (text, str(e.value))
    with pytest.raises(ss.SlicesliceError, match=r"ss\.fields_build\(\)"):
        ss.parse_fields("1")


def test_parse_refusals_leave_the_results_alone():
    with ss.fields_build() as L:
        first, last = ctypes.c_uint64(77), ctypes.c_uint64(78)
        for text in (b"", b"0", b"3-2", b"1,2", b"x"):
            assert L.ss_fields_parse(text, ctypes.byref(first), ctypes.byref(last)) == ss.SS_ERR_ARGUMENT
            assert (first.value, last.value) == (77, 78), text
        assert L.ss_fields_parse(None, ctypes.byref(first), ctypes.byref(last)) == ss.SS_ERR_ARGUMENT
        assert L.ss_fields_parse(b"1", None, ctypes.byref(last)) == ss.SS_ERR_ARGUMENT and (first.value, last.value) == (77, 78)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_written_cases():
    # a,,c has three fields in EACH mode and two in MERGE mode
    assert _records(b"a,,c\n", b",", EACH, 1, 1) == ([(0, 1, 1)], 1)
    assert _records(b"a,,c\n", b",", EACH, 2, 2) == ([(2, 2, 1)], 1)
    assert _records(b"a,,c\n", b",", EACH, 3, 3) == ([(3, 4, 1)], 1)
    assert _records(b"a,,c\n", b",", EACH, 4, 4) == ([], 1)
    assert _records(b"a,,c\n", b",", EACH, 2, 0) == ([(2, 4, 1)], 1)
    assert _records(b"a,,c\n", b",", EACH, 1, 2) == ([(0, 2, 1)], 1)
    assert _records(b"a,,c\n", b",", EACH, 2, 9) == ([(2, 4, 1)], 1)
    assert _records(b"a,,c\n", b",", MERGE, 2, 2) == ([(3, 4, 1)], 1)
    assert _records(b"a,,c\n", b",", MERGE, 3, 3) == ([], 1)
    assert _records(b"a,,c\n", b",", MERGE, 1, 0) == ([(0, 4, 1)], 1)
    # an empty line: one empty field (EACH), no field (MERGE)
    assert _records(b"x\n\ny\n", b",", EACH, 1, 1) == ([(0, 1, 1), (2, 2, 2), (3, 4, 3)], 3)
    assert _records(b"x\n\ny\n", b",", EACH, 2, 2) == ([], 3)
    assert _records(b"x\n\ny\n", b",", MERGE, 1, 1) == ([(0, 1, 1), (3, 4, 3)], 3)
    assert _records(b"x\n\ny\n", b",", MERGE, 1, 1, KEEP_SHORT) == ([(0, 1, 1), (2, 2, 2), (3, 4, 3)], 3)
    assert _records(b"x\n\ny\n", b",", EACH, 2, 2, KEEP_SHORT) == ([(1, 1, 1), (2, 2, 2), (4, 4, 3)], 3)
    # leading and trailing separators
    assert _records(b"  a b  \n", b" ", EACH, 1, 1) == ([(0, 0, 1)], 1)
    assert _records(b"  a b  \n", b" ", EACH, 3, 3) == ([(2, 3, 1)], 1)
    assert _records(b"  a b  \n", b" ", EACH, 6, 6) == ([(7, 7, 1)], 1)
    assert _records(b"  a b  \n", b" ", EACH, 7, 7) == ([], 1)
    assert _records(b"  a b  \n", b" ", MERGE, 1, 1) == ([(2, 3, 1)], 1)
    assert _records(b"  a b  \n", b" ", MERGE, 2, 2) == ([(4, 5, 1)], 1)
    assert _records(b"  a b  \n", b" ", MERGE, 3, 3) == ([], 1)
    assert _records(b"  a b  \n", b" ", MERGE, 2, 5) == ([(4, 7, 1)], 1)         # trailing separators are kept when the fields run out
    assert _records(b"  a b  \n", b" ", MERGE, 1, 0) == ([(2, 7, 1)], 1)
    assert _records(b"   \n", b" ", MERGE, 1, 1) == ([], 1) and _records(b"   \n", b" ", EACH, 4, 4) == ([(3, 3, 1)], 1)
    assert _records(b"   \n", b" ", MERGE, 1, 1, KEEP_SHORT) == ([(3, 3, 1)], 1)
    # a last line without delimiter, an empty view, a view that is one delimiter
    assert _records(b"a b\nc d", b" ", EACH, 2, 2) == ([(2, 3, 1), (6, 7, 2)], 2)
    assert _records(b"a b\nc d", b" ", MERGE, 2, 0) == ([(2, 3, 1), (6, 7, 2)], 2)
    assert _records(b"a b\nc ", b" ", EACH, 2, 2) == ([(2, 3, 1), (6, 6, 2)], 2)
    assert _records(b"a b\nc ", b" ", MERGE, 2, 2) == ([(2, 3, 1)], 2)
    assert _records(b"a b\nc ", b" ", MERGE, 2, 2, KEEP_SHORT) == ([(2, 3, 1), (6, 6, 2)], 2)
    for mode in (EACH, MERGE):
        for flags in (0, KEEP_SHORT):
            assert _records(b"", b" ", mode, 1, 1, flags) == ([], 0)
    assert _records(b"\n", b" ", EACH, 1, 1) == ([(0, 0, 1)], 1) and _records(b"\n", b" ", MERGE, 1, 1) == ([], 1)
    assert _records(b"\n", b" ", MERGE, 1, 1, KEEP_SHORT) == ([(0, 0, 1)], 1) and _records(b"\n\n", b" ", EACH, 1, 0) == ([(0, 0, 1), (1, 1, 2)], 2)
    # the delimiter never separates, even where the set holds it; another delimiter
    assert _records(b"a b\nc d\n", b" \n", EACH, 2, 2) == _records(b"a b\nc d\n", b" ", EACH, 2, 2)
    assert _records(b"a b;c d", b" ", EACH, 2, 2, 0, ord(";")) == ([(2, 3, 1), (6, 7, 2)], 2)
    assert _records(b"a\nb c", words_of(b" "), EACH, 1, 0, 0, 0) == ([(0, 5, 1)], 1)
    assert cut_bytes(b"a,b,c\nd\ne,f\n", b",", EACH, 2, 2) == b"b\nf\n" and cut_bytes(b"a,b,c\nd\ne,f\n", b",", EACH, 2, 2, KEEP_SHORT) == b"b\n\nf\n"


def test_the_numpy_rule_agrees_with_the_plain_python_reference_on_random_data():
    rng = np.random.default_rng(23)
    for alphabet in (b"ab ,\n", b" \n", b"a ", b"ab\t ,.;\n\n", b",\n"):
        for size in (0, 1, 2, 17, 120):
            data = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size).tobytes() if size else b""
            for members in (b" ", b",", b" \t", b" ,\n", bytes(range(256))):
                for mode in (EACH, MERGE):
                    for first, last in ((1, 1), (1, 0), (2, 2), (2, 0), (2, 3), (3, 5), (5, 5)):
                        for flags in (0, KEEP_SHORT):
                            for delimiter in (10, ord("a")):
                                b, e, n, lines = G.records(data, members, mode, first, last, bool(flags), delimiter)
                                assert _records(data, members, mode, first, last, flags, delimiter) == (list(zip(b, e, n)), lines), \
                                    (data, members, mode, first, last, flags, delimiter)


def test_the_fixture_is_what_the_generator_gives_and_the_rule_reproduces_its_rows():
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    kat = json.load(open(os.path.join(GOLDEN, "fields_kat.json")))
    assert kat == json.loads(json.dumps(G.make(data)))
    assert os.path.getsize(os.path.join(GOLDEN, "fields_kat.json")) < 32768 and kat["bytes"] == len(data) == 857425
    assert [(c["separator"], c["mode"], c["fields"]) for c in kat["cases"] if not c["keep_short"]] == \
        [(" ", EACH, "2"), (r"[ \t]", MERGE, "1"), (r"[ \t]", MERGE, "2"), (r"[ \t]", MERGE, "3-5"), (r"[ \t]", MERGE, "7-"), (r"\.", EACH, "1-2")]
    assert len(kat["cases"]) == 12 and len({c["lines"] for c in kat["cases"]}) == 1
    for c in kat["cases"]:
        members = c["members"].encode("latin-1")
        b, e, n, lines = rule_fields(data, members, c["mode"], c["first"], c["last"], KEEP_SHORT if c["keep_short"] else 0)
        assert (b.size, lines, int((e - b).sum())) == (c["records"], c["lines"], c["bytes_selected"]), c["name"]
        assert c["records"] == (c["lines"] if c["keep_short"] else c["selected"]), c["name"]
        assert hashlib.sha256(b.astype("<i8").tobytes() + e.astype("<i8").tobytes() + n.astype("<i8").tobytes()).hexdigest() == c["sha256"], c["name"]
        assert (np.diff(b) > 0).all() and (e >= b).all() and (np.diff(n) > 0).all(), c["name"]


# ---- header, ctypes table, Rust block, build ---------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_fields.h")
    assert sorted(c) == sorted(ss.searcher.FIELDS_ABI) == FIELDS
    assert c["ss_fields_new"] == ("i32", ["ptr", "i32", "u64", "u64", "u32", "ptr"])
    assert c["ss_count_fields_device"] == ("i32", ["ptr", "ptr", "usize", "i32", "ptr", "ptr", "ptr"])
    assert c["ss_find_fields_device"] == ("i32", ["ptr", "ptr", "usize", "i32", "ptr", "ptr", "ptr", "ptr", "u64", "ptr"])
    # the find call's arguments behind the handle are the runs line call's, argument for argument
    runs = header_prototypes("sliceslice_hip_runs.h")
    assert c["ss_find_fields_device"] == runs["ss_find_lines_runs_device"]
    r = rust_prototypes("hip_fields.rs")
    assert r == c, (r, c)
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_fields.h")).read()
    rust = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_fields.rs")).read()
    for name, value, spelled in (("SS_FIELDS_EACH", 0, "c_int = 0"), ("SS_FIELDS_MERGE", 1, "c_int = 1"), ("SS_FIELDS_KEEP_SHORT", 1, "c_uint = 1")):
        assert re.search(r"#define %s\s+%du?\b" % (name, value), text) and getattr(ss, name) == value and "pub const %s: %s;" % (name, spelled) in rust
    assert re.search(r"#define SS_FIELDS_CARRY_CHUNK\s+256\b", text) and ss.FIELDS_CARRY_CHUNK == 256
    assert "pub const SS_FIELDS_CARRY_CHUNK: usize = 256;" in rust
    assert "constexpr int kFieldsCarryChunk = 256;" in open(os.path.join(CSRC, "fields_launch.hpp")).read()
    stats = re.search(r"typedef struct ss_fields_stats \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(re.findall(r"\b(\w+)[,;]", re.sub(r"/\*.*?\*/", "", stats))) == ss.searcher.FIELDS_STATS
    assert tuple(re.findall(r"pub (\w+): u64", rust.split("pub struct ss_fields_stats", 1)[1].split("}", 1)[0])) == ss.searcher.FIELDS_STATS
    for name, (res, args) in ss.searcher.FIELDS_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_fields.h":
            assert not set(c) & set(header_prototypes(h)), h
    assert '#include "sliceslice_hip_rewrite.h"' in text
    assert "hip_fields.rs" in open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "build.rs")).read()


def test_the_header_states_the_rule_the_refusals_and_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_fields.h")).read()
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).split())
    for said in ("THE RULE", "are sliceslice_hip_lines.h's", "The delimiter is never a separator, even where the set holds it",
                 "a non-empty class of byte values in the four-word layout of sliceslice_hip_classes.h", "every separator byte ends a field",
                 "a line with s separators has s + 1 fields", "an empty line has one empty field",
                 "maximal runs of bytes that are neither separator nor delimiter", "leading and trailing separators make no field",
                 "a line of separators only has 0 fields", "1 <= first", 'last == 0 means "to the line\'s end"', "otherwise first <= last",
                 "A line with n fields is selected when n >= first", "begin is the first byte of field `first`",
                 "If last != 0 and n >= last, end is the end of field `last`", "the position of its delimiter, or the view's end",
                 "TRAILING SEPARATORS ARE KEPT when the line runs out of fields", "begin == end == the line's end",
                 "exactly one record per line and record k is line k + 1", "Bytes outside [0, len) are absent",
                 "no load touches a 16-byte block that holds no byte of the view", "Records ascend", "make one call per range",
                 "naming the column (from 1) as ss_runs_parse does", "HOST ONLY", "THERE IS NO _async FORM", "*total is always the full record count",
                 "Capacity and NULL rules are ss_find_all_runs_device's", "Refused with SS_ERR_ARGUMENT and a message, nothing written",
                 "an unknown mode or flag", "first == 0", "last non-zero and below first", "an empty set", "a set that is only the delimiter",
                 "a handle made on another device", "a capturing stream", "a delimiter that is no byte", "one prefix sum and a ballot",
                 "a workgroup with a delimiter replaces the carry by its tail, one without adds its events", "it never reads the haystack",
                 "the view is read once", "No waiting between workgroups, no atomic", "80 bytes per workgroup", "the output depends on the input alone",
                 "Out of scope", "comma lists of ranges in one call", "quoted CSV fields", "multi-byte separators", "a replace form", "batched forms",
                 "an output delimiter other than the gather call's terminator"):
        assert said.lower() in flat.lower(), said


def test_the_nineteenth_library_stands_on_the_rewrite_one():
    b = _build()
    entry = b._lib("fields")
    assert entry["parent"] == "rewrite" and entry["sources"] == ["ss_fields.hip"]
    # a sixth mapping below the five that are pinned name by name, which are what they were
    assert list(b._FIELDS_LIBRARIES) == ["fields"] and b._FIELDS_LIBRARIES["fields"] is entry
    assert list(b._REWRITE_LIBRARIES) == ["rewrite"] and list(b._NEWEST_LIBRARIES) == ["runs"] and list(b._LATEST_LIBRARIES) == ["masked", "classes"]
    assert list(b._LATER_LIBRARIES) == ["output", "leftmost"] and "fields" not in b.LIBRARIES and len(b.LIBRARIES) == 12
    source = open(os.path.join(ROOT, "sliceslice-rs_amd", "_build.py")).read()
    assert source.index("_REWRITE_LIBRARIES = {") < source.index("_FIELDS_LIBRARIES = {") < source.index("def _lib(")
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_fields.so" == os.path.basename(b.fields_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_fields.json" == os.path.basename(b.fields_resources_path())
    assert callable(b.build_fields) and callable(b.fields_kernel_resources)
    assert "sliceslice-rs_amd/csrc/kernel_resources_fields.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("fields") == b._all_sources("rewrite") + ["ss_fields.hip"]
    assert b._all_sources("fields")[-3:] == ["ss_runs.hip", "ss_rewrite.hip", "ss_fields.hip"]
    for h in ("fields_kernels.hpp", "fields_launch.hpp", "fields_host.hpp", os.path.join("..", "..", "include", "sliceslice_hip_fields.h")):
        assert h in b._HEADERS, h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index('b.build_library("rewrite", force=True, verbose=True)') < \
        entry_point.index('b.build_library("fields", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["fields"][0] is ss.searcher.FIELDS_ABI and ss.searcher._FEATURES["fields"][1] == "ss_fields_new"
    product = ss.lib()
    assert not getattr(product, "has_fields")
    with ss.rewrite_build() as L:
        assert not L.has_fields and L.has_rewrite
    with ss.fields_build() as L:
        assert ss.lib() is L and L.has_fields and L.has_rewrite and L.has_runs and L.has_output and L.has_lines
        assert ss.searcher._feature_lib(L, "fields") is L
    assert ss.lib() is product


def test_the_headers_functions_are_the_librarys_exported_additions():
    b = _build()
    rewrite = _exported(b.build_rewrite())
    assert _exported(b.build_fields()) == sorted(rewrite + FIELDS)
    assert not set(FIELDS) & set(rewrite) and not set(FIELDS) & set(_exported(ss.build()))
    for name in list(b.LIBRARIES) + list(b._LATER_LIBRARIES) + list(b._LATEST_LIBRARIES) + list(b._NEWEST_LIBRARIES) + list(b._REWRITE_LIBRARIES):
        so = b.library_path_of(name)
        assert not os.path.exists(so) or not set(FIELDS) & set(_exported(so)), name


def test_the_new_kernels_use_no_private_segment_spill_no_vector_register_and_little_lds():
    rows = {r["name"]: r for r in _build().fields_kernel_resources() if r["tu"] == "ss_fields.hip"}
    names = sorted(rows)
    assert len(names) == 3 and sum("ss::fields_kernel" in n for n in names) == 2 and sum("ss::fields_carry_kernel" in n for n in names) == 1, names
    for name, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r.get("agprs", 0) == 0, (name, r)
        assert r["lds_bytes"] <= 16 * 1024 and r["vgprs"] <= 128, (name, r)
    kernels = open(os.path.join(CSRC, "fields_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in kernels.splitlines())
    host = open(os.path.join(CSRC, "ss_fields.hip")).read()
    for called in ("masked_load<U>(", "runs_members16(", "runs_select<U, true>(", "set_valid_bits(", "kSetU", "kSetTiles", "wave_exclusive_sum(",
                   "wave_sum(", "__builtin_amdgcn_ballot_w64("):
        assert called in code, called
    everything = code + "\n".join(l.split("//")[0] for l in host.splitlines())
    for banned in ("asm", "volatile", "__threadfence", "atomic", "hipMalloc"):      # no waiting between workgroups, no atomic
        assert banned not in everything, banned
    # the carry kernel does not read the haystack: it is handed no pointer to it
    carry = code.split("fields_carry_kernel(FieldsCarryArgs ca)", 1)[1]
    assert "hay" not in carry and "base[" not in carry
    launch = open(os.path.join(CSRC, "fields_launch.hpp")).read()
    assert "hay" not in launch.split("struct FieldsCarryArgs {", 1)[1].split("};", 1)[0]


def test_every_other_build_refuses_and_names_the_build():
    message = ss.searcher._FEATURES["fields"][2]
    assert "ss.fields_build()" in message and "libsliceslice_hip_fields.so" in message
    for context in (ss.rewrite_build, ss.runs_build):
        with context():
            with pytest.raises(ss.SlicesliceError, match=r"ss\.fields_build\(\)") as e:
                ss.FieldSelector(b",", 1)
            assert e.value.code == ss.SS_ERR_ARGUMENT
    with pytest.raises(ss.SlicesliceError, match=r"ss\.fields_build\(\)"):
        ss.FieldSelector(b",", 1)


def test_the_refusals_that_need_no_device_leave_the_results_alone():
    with ss.fields_build() as L:
        comma = words_of(b",")
        none = np.zeros(4, dtype=np.uint64)
        out = ctypes.c_void_p(0x77)
        for args, said in (((None, 0, 1, 1, 0), "NULL"), ((comma.ctypes.data, 2, 1, 1, 0), "mode"), ((comma.ctypes.data, -1, 1, 1, 0), "mode"),
                           ((comma.ctypes.data, 0, 1, 1, 2), "flag"), ((comma.ctypes.data, 0, 0, 1, 0), "first is 0"),
                           ((comma.ctypes.data, 1, 0, 0, 0), "first is 0"), ((comma.ctypes.data, 0, 3, 2, 0), "last is below first"),
                           ((none.ctypes.data, 0, 1, 1, 0), "the set is empty")):
            assert L.ss_fields_new(*args, ctypes.byref(out)) == ss.SS_ERR_ARGUMENT, said
            assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
            assert out.value == 0x77, said
        assert L.ss_fields_new(comma.ctypes.data, 0, 1, 1, 0, None) == ss.SS_ERR_ARGUMENT
        # the scan calls: refusals that come before the handle is looked at
        handle = ctypes.create_string_buffer(512)
        h = ctypes.cast(handle, ctypes.c_void_p)
        a, b = ctypes.c_uint64(77), ctypes.c_uint64(78)
        for args, said in (((None, None, 0, 10, None, ctypes.byref(a), ctypes.byref(b)), "fields is NULL"),
                           ((h, None, 0, 10, None, None, ctypes.byref(b)), "NULL"), ((h, None, 0, 10, None, ctypes.byref(a), None), "NULL"),
                           ((h, None, 5, 10, None, ctypes.byref(a), ctypes.byref(b)), "haystack is NULL"),
                           ((h, None, 0, 256, None, ctypes.byref(a), ctypes.byref(b)), "delimiter 256"),
                           ((h, None, 0, -1, None, ctypes.byref(a), ctypes.byref(b)), "delimiter -1")):
            assert L.ss_count_fields_device(*args) == ss.SS_ERR_ARGUMENT, said
            assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
            assert (a.value, b.value) == (77, 78), said
        for args, said in (((None, None, 0, 10, None, None, None, None, 0, ctypes.byref(a)), "fields is NULL"),
                           ((h, None, 0, 10, None, None, None, None, 0, None), "total is NULL"),
                           ((h, None, 0, 10, None, None, None, None, 4, ctypes.byref(a)), "all three arrays are NULL"),
                           ((h, None, 0, 300, None, None, None, None, 0, ctypes.byref(a)), "delimiter 300")):
            assert L.ss_find_fields_device(*args) == ss.SS_ERR_ARGUMENT, said
            assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
            assert a.value == 77, said
