"""CPU checks of the byte-class calls (include/sliceslice_hip_classes.h): the header, the ctypes table and the Rust module agree symbol
by symbol; the sixteenth library stands on the masked one and the product holds none of it; the new kernels use no private segment
and spill no vector register; ss_classes_parse accepts what Python's `re` accepts with the same meaning and refuses what the header
says, with the column; ss_classes_cover is the tightest pair; the two limits; the filter choice; classes_host.hpp in a program of
its own under ASan and UBSan; the numpy rule the GPU tests use agrees with `re`, and tests/golden/classes_kat.json is what its
generator produces now."""
import json
import os
import re
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_classes_golden as G         # noqa: E402

CLASSES = ["ss_classes_new", "ss_classes_free", "ss_classes_info", "ss_classes_parse", "ss_classes_cover", "ss_count_classes_device",
           "ss_count_classes_device_async", "ss_find_all_classes_device", "ss_count_lines_classes_device", "ss_find_lines_classes_device"]


def members(sets):
    """(n, 256) bool: byte b is bit b & 63 of word b >> 6 of every position's four words"""
    sets = np.ascontiguousarray(sets, dtype="<u8").reshape(-1, 4)
    return np.unpackbits(sets.view(np.uint8).reshape(-1, 32), axis=1, bitorder="little").astype(bool)


def sets_of(table):
    """the (n, 4) words of an (n, 256) bool table"""
    table = np.asarray(table, dtype=bool).reshape(-1, 256)
    return np.ascontiguousarray(np.packbits(table, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(-1, 4)


def rule_offsets(data, sets):
    """THE RULE in numpy: every p in [0, len - n] with hay[p + i] in set i for all i.  What the GPU tests compare with."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    table = members(sets)
    n = len(table)
    if n == 0 or data.size < n:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(data.size - n + 1, dtype=bool)
    for i in range(n):
        if not table[i].all():
            ok &= table[i][data[i:data.size - n + 1 + i]]
    return np.flatnonzero(ok).astype(np.int64)


def rule_lines(data, sets, delimiter):
    """(begin, end, number) of the lines that hold an occurrence wholly inside them, as sliceslice_hip_lines.h lays records out:
    end is the delimiter's index (len for an unterminated last line), number counts from 1."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n, offs = len(members(sets)), rule_offsets(data, sets)
    delims = np.flatnonzero(data == delimiter).astype(np.int64)
    ends = np.append(delims, data.size) if (delims.size == 0 or delims[-1] != data.size - 1) and data.size else delims
    begins = np.concatenate([[0], delims + 1])[:ends.size]
    line = np.searchsorted(ends, offs, side="left")                 # the line of the occurrence's first byte
    inside = offs + n <= ends[np.minimum(line, ends.size - 1)] if ends.size else np.zeros(0, dtype=bool)
    sel = np.unique(line[inside])
    return begins[sel], ends[sel], sel + 1


def re_set(item, ignore_case=False):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rx = re.compile(item.encode("latin-1"), re.S | (re.I if ignore_case else 0))
    return np.array([rx.fullmatch(bytes([b])) is not None for b in range(256)])


# ---- header, ctypes table, Rust block, build ---------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_classes.h")
    assert sorted(c) == sorted(ss.searcher.CLASSES_ABI) == sorted(CLASSES)
    masked = header_prototypes("sliceslice_hip_masked.h")
    for name in ("ss_count_%s_device", "ss_count_%s_device_async", "ss_find_all_%s_device", "ss_count_lines_%s_device", "ss_find_lines_%s_device"):
        assert c[name % "classes"] == masked[name % "masked"], name
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_classes.h")).read()
    flatc = " ".join(text.split())
    flatm = " ".join(open(os.path.join(ROOT, "include", "sliceslice_hip_masked.h")).read().split())
    for name in ("ss_count_%s_device(", "ss_count_%s_device_async(", "ss_find_all_%s_device(", "ss_count_lines_%s_device(", "ss_find_lines_%s_device("):
        # argument for argument, by name, after the first
        mine = re.search(re.escape(name % "classes") + r"const ss_classes \*pattern, ([^;]*);", flatc).group(1)
        model = re.search(re.escape(name % "masked") + r"const ss_masked \*pattern, ([^;]*);", flatm).group(1)
        assert mine == model, name
    assert c["ss_classes_new"] == ("i32", ["ptr", "usize", "ptr"]) and c["ss_classes_free"] == ("void", ["ptr"])
    assert c["ss_classes_info"] == ("i32", ["ptr", "i32", "ptr"])
    assert c["ss_classes_parse"] == ("i32", ["ptr", "i32", "ptr", "usize", "ptr"])
    assert c["ss_classes_cover"] == ("i32", ["ptr", "usize", "ptr", "ptr"])
    r = rust_prototypes("hip_classes.rs")
    assert r == c, (r, c)
    rust = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_classes.rs")).read()
    for name, value in (("MAX_LEN", 4096), ("MAX_INEXACT", 1024), ("MAX_DISTINCT", 64)):
        assert "pub const SS_CLASSES_%s: usize = %d;" % (name, value) in rust
        assert re.search(r"#define SS_CLASSES_%s\s+%d\b" % (name, value), text) and getattr(ss, "CLASSES_" + name) == value
    for name, (res, args) in ss.searcher.CLASSES_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_classes.h":
            assert not set(c) & set(header_prototypes(h)), h
    assert '#include "sliceslice_hip_masked.h"' in text
    # the stats are eight 64-bit words in the order of the Python names, and of the Rust struct
    body = re.search(r"typedef struct ss_classes_stats \{(.*?)\}", text, flags=re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]+);", body) for f in decl.split(",")]
    assert fields == list(ss.searcher.CLASSES_STATS) == ["n", "anchor", "distance", "single", "masked", "inexact", "distinct", "accepts_delimiter"]
    assert re.findall(r"pub (\w+): u64,", re.search(r"pub struct ss_classes_stats \{(.*?)\}", rust, flags=re.S).group(1)) == fields
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).split())
    for said in ("THE RULE", "1 <= n <= SS_CLASSES_MAX_LEN", "bit b & 63 of word b >> 6", "hay[p + i] in set i for all i < n",
                 "Occurrences overlap", "Bytes outside [0, len) are absent", "no load touches a 16-byte block that holds no byte of the view",
                 "64-bit", "`a.b` and `a[^x]b` do not match \"a\\nb\"", "sliceslice_hip_lines.h's, word for word",
                 "mask = ~(OR over members c of c ^ c0)", "SS_CLASSES_MAX_INEXACT (1,024)", "SS_CLASSES_MAX_DISTINCT (64)", "names the limit",
                 "strict subset of Python `re` byte patterns under re.DOTALL", "HOST ONLY", "offending column", "rarest set first",
                 "Refused with SS_ERR_ARGUMENT", "nothing written", "Out of scope", "variable length", "alternatives", "groups", "anchors",
                 "word / inverted / context / batched / replace forms", "sharper register filters", "DESIGN.md 5.20"):
        assert said.lower() in flat.lower(), said


def test_the_sixteenth_library_stands_on_the_masked_one():
    b = _build()
    entry = b._lib("classes")
    assert entry["parent"] == "masked" and entry["sources"] == ["ss_classes.hip"] and "classes" not in b.LIBRARIES
    assert list(b._LATEST_LIBRARIES) == ["masked", "classes"]
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_classes.so" == os.path.basename(b.classes_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_classes.json" == os.path.basename(b.classes_resources_path())
    assert "sliceslice-rs_amd/csrc/kernel_resources_classes.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("classes") == b._all_sources("masked") + ["ss_classes.hip"]
    for h in ("classes_host.hpp", "classes_kernels.hpp", "classes_launch.hpp", os.path.join("..", "..", "include", "sliceslice_hip_classes.h")):
        assert h in b._HEADERS, h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index('b.build_library("masked", force=True, verbose=True)') < \
        entry_point.index('b.build_library("classes", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["classes"][0] is ss.searcher.CLASSES_ABI and ss.searcher._FEATURES["classes"][1] == "ss_classes_new"
    product = ss.lib()
    assert not getattr(product, "has_classes")
    with ss.masked_build() as L:
        assert not L.has_classes
    with ss.classes_build() as L:
        assert ss.lib() is L and L.has_classes and L.has_masked and L.has_leftmost and L.has_lines and ss.searcher._feature_lib(L, "classes") is L
    assert ss.lib() is product
    masked = _exported(b.build_masked())
    assert _exported(b.build_classes()) == sorted(masked + CLASSES)
    assert not set(CLASSES) & set(masked) and not set(CLASSES) & set(_exported(ss.build()))
    # the kernels include the masked ones: neither edited nor copied
    kernels = open(os.path.join(CSRC, "classes_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in kernels.splitlines())
    assert '#include "masked_kernels.hpp"' in kernels and '#include "masked_launch.hpp"' in open(os.path.join(CSRC, "classes_launch.hpp")).read()
    for called in ("masked_load<U>(", "masked_filter<U>(", "masked_verify<true>(", "masked_verify<false>(", "masked_stage(", "line_capture<U>(",
                   "line_tile_done<U, false>("):
        assert called in code, called
    assert "asm" not in code and "__threadfence" not in code and "volatile" not in code and code.count("atomic") == 1
    host = open(os.path.join(CSRC, "classes_host.hpp")).read()
    assert "hip_runtime" not in host and "#include <hip" not in host and "__device__" not in host and "SS_API" not in host
    assert "ss_masked_choose_filter(" in host and "ByteCost" not in host


def test_the_product_and_the_masked_build_refuse_and_name_the_build():
    message = ss.searcher._FEATURES["classes"][2]
    assert "ss.classes_build()" in message and "libsliceslice_hip_classes.so" in message
    with ss.masked_build() as masked_library:
        pass
    for L in (ss.lib(), masked_library):
        assert not getattr(L, "has_classes", False)
    calls = (lambda: ss.ClassPattern(r"\d"), lambda: ss.ClassPattern.from_sets(np.ones((1, 4), dtype=np.uint64)),
             lambda: ss.ClassPattern.from_masked(b"a", b"\xdf"), lambda: ss.ClassPattern.from_bytes(b"x", True),
             lambda: ss.parse_classes("a"), lambda: ss.classes_cover(np.ones((1, 4), dtype=np.uint64)))
    for call in calls:
        with pytest.raises(ss.SlicesliceError, match=r"ss\.classes_build\(\)") as e:
            call()
        assert e.value.code == ss.SS_ERR_ARGUMENT
    with ss.masked_build():
        for call in calls:
            with pytest.raises(ss.SlicesliceError, match=r"ss\.classes_build\(\)") as e:
                call()


def test_the_new_kernels_use_no_private_segment_and_spill_no_vector_register():
    rows = {r["name"]: r for r in _build().classes_kernel_resources() if r["tu"] == "ss_classes.hip"}
    names = sorted(rows)
    assert len(names) == 4 and all("ss::classes_all_kernel" in n or "ss::classes_lines_kernel" in n for n in names), names
    for name, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r.get("agprs", 0) == 0, (name, r)
        assert r["lds_bytes"] <= 15 * 1024 + 2048, (name, r)       # covers, bitmaps, check list and the wave slots


# ---- ss_classes_parse --------------------------------------------------------------------------------------------------------------
ITEMS = [r"a", r"Z", r"_", r"0", r" ", r"-", r",", r":", r"#", "\xe9", r".", r"\d", r"\D", r"\w", r"\W", r"\s", r"\S", r"\n", r"\t", r"\r", r"\f",
         r"\v", r"\x00", r"\x41", r"\x7a", r"\xff", r"\xFf", r"\.", r"\\", r"\[", r"\]", r"\{", r"\}", r"\(", r"\)", r"\*", r"\+", r"\?", r"\|",
         r"\^", r"\$", r"\-", r"\_", r"\/", r"\"", r"\~", r"\!", r"\@", r"[0-9]", r"[0-9A-F]", r"[0-9a-fA-F]", r"[aeiou]", r"[Ff]", r"[^a]",
         r"[^a-z]", r"[^ -~\n]", r'[^"]', r"[a-c]", r"[-a]", r"[a-]", r"[^-]", r"[^-a]", r"[-]", r"[a\-z]", r"[\]]", r"[a\]]", r"[\[]", r"[\\]",
         r"[\^]", r"[a^]", r"[.]", r"[+*?.|()${}]", r"[\d]", r"[\D]", r"[^\d]", r"[\w-]", r"[\w.-]", r"[\s\d]", r"[^\W]", r"[^\s\w]", r"[\da-f]",
         r"[\x00-\x1f]", r"[\x80-\xff]", r"[\n-\r]", r"[ -\x2f]", r"[\--9]", r"[\x41-Z]", r"[a-a]", r"[a-zA-Z_]",r"[&]", r"[~|]", r"[a&]",
         r"[&-~]", r"[^\x00]", r"[^\x01-\xff]", "[\xe0-\xff]", r"[a-c-]", r"[\d-]", r"[{2}]", r"[,]"]


def test_every_accepted_item_means_what_re_means_by_it():
    with ss.classes_build():
        for item in ITEMS:
            for ignore_case in (False, True):
                got = ss.parse_classes(item, ignore_case)
                assert got.shape == (1, 4) and got.dtype == np.uint64, item
                assert (members(got)[0] == re_set(item, ignore_case)).all(), (item, ignore_case)
        # the header's own examples
        assert not members(ss.parse_classes(r"[^a]", True))[0][ord("A")] and members(ss.parse_classes(r"[^a]", False))[0][ord("A")]
        assert members(ss.parse_classes(r"[a-c]", True))[0][[ord(x) for x in "abcABC"]].all()
        assert members(ss.parse_classes(r"\D"))[0][10] and members(ss.parse_classes(r"\s"))[0][10] and members(ss.parse_classes(r"."))[0].all()
        # repetition, an empty text, str and bytes
        assert len(ss.parse_classes("")) == 0 and ss.parse_classes("").shape == (0, 4)
        assert len(ss.parse_classes(r"a{1}")) == 1 and len(ss.parse_classes(r"a{4096}")) == 4096 and len(ss.parse_classes(r"[0-9]{03}x{2}")) == 5
        assert len(ss.parse_classes(r"\d{4000}a{96}")) == 4096
        assert (ss.parse_classes(rb"[0-9A-F]{4}H") == ss.parse_classes(r"[0-9A-F][0-9A-F][0-9A-F][0-9A-F]H")).all()
        assert (ss.parse_classes(b"\xe9") == ss.parse_classes(r"\xe9")).all()


def test_whole_patterns_find_what_re_finds():
    manual = np.frombuffer(open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read(), dtype=np.uint8)
    rng = np.random.default_rng(5)
    two = rng.choice(np.frombuffer(b"ab", dtype=np.uint8), 20000)
    mixed = rng.choice(np.frombuffer(b"abAB\n-]x9", dtype=np.uint8), 20000)
    patterns = [c[1] for c in G.CASES] + [r"[ab]{3}", r"a[^a]a", r"[^b]{2}b", r"a.{3}b", r"\w\W", r"[a-]\]", r"[A-B]x", r"9\n[a-b]", r"\x61\x62{2}",
                                          r"[\x61-b]\S{2}-", r"[^\n]{5}\n"]
    with ss.classes_build():
        for pattern in patterns:
            for ignore_case in (False, True):
                sets = ss.parse_classes(pattern, ignore_case)
                for data in (manual, two, mixed):
                    with warnings.catch_warnings():
                        warnings.simplefilter("error")
                        want = G.offsets_of(data.tobytes(), pattern, ignore_case)
                    assert rule_offsets(data, sets).tolist() == want, (pattern, ignore_case)


REFUSED = [
    # (text, column)
    (r"\b", 2), (r"\A", 2), (r"\Z", 2), (r"\1", 2), (r"\0", 2), (r"\a", 2), (r"a\q", 3), ("ab\\", 3), (r"\x4", 3), (r"\x4g", 4), (r"\xg1", 3),
    (r"\x", 2), ("[a\\", 3), (r"[\b]", 3), (r"[\x4]", 5),
    (r"a|b", 2), (r"(a)", 1), (r"a)", 2), (r"a*", 2), (r"a+", 2), (r"a?", 2), (r"^a", 1), (r"a$", 2), (r"a]", 2), (r"a}", 2),
    (r"{2}", 1), (r"a{2}{3}", 5), (r"a{0}", 3), (r"a{4097}", 3), (r"a{99999999999999999999}", 3), (r"a{2,}", 4), (r"a{2,3}", 4), (r"a{,3}", 3),
    (r"a{}", 3), (r"a{2", 3), (r"a{x}", 3), (r"a{-1}", 3), (r"a{ 2}", 3),
    (r"[]", 2), (r"[^]", 3), (r"[]a]", 2), (r"[[]", 2), (r"[a[]", 3), (r"[[:alpha:]]", 2), (r"[a-[]", 4), (r"[a", 1), (r"x[^", 2), (r"[a-", 1),
    (r"[a--]", 4), (r"[--a]", 3), (r"[a&&b]", 4), (r"[~~]", 3), (r"[a||b]", 4), (r"[a--b]", 4),
    (r"[z-a]", 2), (r"[\xff-\x00]", 2), (r"[b-a]", 2), (r"[a-\d]", 4), (r"[\d-a]", 2), (r"[\w-\s]", 2), (r"[a-c-e]", 5), (r"[ab-]x[a-c-e]", 11),
    (r"[^\x00-\xff]", 1), (r"a[^\d\D]", 2), (r"[^\s\S]", 1), (r"[^\w\W]", 1),
    (r"a{4096}b", 8), (r"a{4000}b{97}", 9), (r"a{4096}{2}", 8),
]


def test_every_refusal_names_its_column():
    with ss.classes_build():
        for text, column in REFUSED:
            for ignore_case in (False, True):
                with pytest.raises(ss.SlicesliceError, match=r"ss_classes_parse: column %d\b" % column) as e:
                    ss.parse_classes(text, ignore_case)
                assert e.value.code == ss.SS_ERR_ARGUMENT, text
        with pytest.raises(ss.SlicesliceError, match=r"column 2\b") as e:
            ss.parse_classes(b"a\0b")
        assert e.value.code == ss.SS_ERR_ARGUMENT
        # a long text: 4,097 literals
        with pytest.raises(ss.SlicesliceError, match=r"column 4097\b.*4096 positions"):
            ss.parse_classes("a" * 4097)
        import ctypes
        L, n = ss.lib(), ctypes.c_size_t(77)
        assert L.ss_classes_parse(None, 0, None, 0, ctypes.byref(n)) == ss.SS_ERR_ARGUMENT
        assert L.ss_classes_parse(b"a", 0, None, 0, None) == ss.SS_ERR_ARGUMENT
        assert L.ss_classes_parse(b"a(", 0, None, 0, ctypes.byref(n)) == ss.SS_ERR_ARGUMENT and n.value == 77
        # the sets behind the capacity are not written
        out = np.full((3, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        assert L.ss_classes_parse(b"abc", 0, out.ctypes.data, 2, ctypes.byref(n)) == ss.SS_OK and n.value == 3
        assert (out[2] == 0x5A5A5A5A5A5A5A5A).all() and members(out[:2])[0][ord("a")] and members(out[:2])[1][ord("b")]


# ---- ss_classes_cover --------------------------------------------------------------------------------------------------------------
def test_the_cover_is_the_tightest_pair():
    rng = np.random.default_rng(6)
    with ss.classes_build():
        tables = []
        for trial in range(300):
            table = np.zeros(256, dtype=bool)
            base, spread = int(rng.integers(0, 256)), int(rng.integers(0, 256))
            picks = rng.integers(0, 256, int(rng.integers(1, 9))) if trial % 3 == 0 else base ^ (rng.integers(0, 256, int(rng.integers(1, 40))) & spread)
            table[picks] = True
            tables.append(table)
        value, mask = ss.classes_cover(sets_of(np.array(tables)))
        assert len(value) == len(mask) == 300
        b = np.arange(256)
        for table, v, m in zip(tables, value, mask):
            assert v & ~m & 0xFF == 0 and ((b[table] & m) == v).all()
            # brute force over all 65,536 pairs: none that accepts every member has more mask bits
            best = max(bin(mm).count("1") for mm in range(256) if len(set((b[table] & mm).tolist())) == 1)
            assert bin(m).count("1") == best, (v, m)
        cover = lambda text, ic=False: tuple(x.hex().upper() for x in ss.classes_cover(ss.parse_classes(text, ic)))      # noqa: E731
        assert cover("[0-9]") == ("30", "F0") and cover("[Ff]") == ("46", "DF") and cover(".") == ("00", "00") and cover("q") == ("71", "FF")
        # bit 3 differs between '0' and '8', so the formula of the header gives 80, not 88: 128 accepted values, as the header says
        assert cover("[0-9A-F]") == ("00", "80") and cover(r"\w") == ("00", "80") and cover("[aeiou]") == ("61", "E1") and cover('[^"]') == ("00", "00")
        assert cover("f", True) == ("46", "DF") and cover(r"\d\d:\d\d") == ("30303A3030", "F0F0FFF0F0")
        assert ss.classes_cover(np.zeros((0, 4), dtype=np.uint64)) == (b"", b"")
        with pytest.raises(ss.SlicesliceError, match="position 1 is empty") as e:
            ss.classes_cover(np.array([[1, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint64))
        assert e.value.code == ss.SS_ERR_ARGUMENT
        with pytest.raises(ValueError):
            ss.classes_cover(np.zeros((2, 3), dtype=np.uint64))


def _device_or_argument_error(make_it):
    """ss_classes_new plans on the host before it touches a device: a pattern within the limits is made where a GPU is, and fails
    with another code than SS_ERR_ARGUMENT where none is.  Returns the pattern or None."""
    try:
        return make_it()
    except ss.SlicesliceError as e:
        assert e.code != ss.SS_ERR_ARGUMENT, e
        return None


def test_the_two_limits_are_refused_by_name_and_their_edges_accepted():
    digit, letter = sets_of(re_set("[0-9]"))[0], sets_of(re_set("q"))[0]
    with ss.classes_build():
        for inexact in (1024, 1025):
            sets = np.tile(letter, (4096, 1))
            sets[np.arange(inexact) * 3 + 1] = digit
            if inexact == 1024:
                pat = _device_or_argument_error(lambda: ss.ClassPattern.from_sets(sets))
                if pat is not None:
                    info = pat.info()
                    assert (info["n"], info["single"], info["masked"], info["inexact"], info["distinct"]) == (4096, 3072, 0, 1024, 1)
            else:
                with pytest.raises(ss.SlicesliceError, match=r"more than 1024 .*SS_CLASSES_MAX_INEXACT") as e:
                    ss.ClassPattern.from_sets(sets)
                assert e.value.code == ss.SS_ERR_ARGUMENT
        for distinct in (64, 65):
            tables = np.zeros((4096, 256), dtype=bool)
            ids = np.arange(4096) % distinct
            tables[np.arange(4096), np.where(ids < 64, 4 * ids, 1)] = True
            tables[np.arange(1000), np.where(ids < 64, 4 * ids + 3, 2)[:1000]] = True      # {b, b + 3}: the cover accepts four values
            sets = sets_of(tables)
            if distinct == 64:
                pat = _device_or_argument_error(lambda: ss.ClassPattern.from_sets(sets))
                if pat is not None:
                    assert pat.info()["distinct"] == 64 and pat.info()["inexact"] == 1000
            else:
                with pytest.raises(ss.SlicesliceError, match=r"more than 64 distinct .*SS_CLASSES_MAX_DISTINCT") as e:
                    ss.ClassPattern.from_sets(sets)
                assert e.value.code == ss.SS_ERR_ARGUMENT
        for bad, said in ((np.zeros((0, 4), dtype=np.uint64), "SS_CLASSES_MAX_LEN"), (np.tile(letter, (4097, 1)), "SS_CLASSES_MAX_LEN"),
                          (np.array([letter, [0, 0, 0, 0]], dtype=np.uint64), "position 1 is empty")):
            with pytest.raises(ss.SlicesliceError, match=said) as e:
                ss.ClassPattern.from_sets(bad)
            assert e.value.code == ss.SS_ERR_ARGUMENT
        with pytest.raises(ss.SlicesliceError, match="SS_CLASSES_MAX_LEN") as e:
            ss.ClassPattern("")
        with pytest.raises(ValueError):
            ss.ClassPattern.from_masked(b"abc", b"\xff")


def test_the_filter_choice_is_the_masked_rule_on_the_covers_and_avoids_wild_positions():
    rng = np.random.default_rng(8)
    pool = [r".", r".", r"[^x]", r'[^"]', r"\D", r"[0-9]", r"\w", r"[Ff]", r"q", r"e", r"[0-9A-F]", r"\s"]
    with ss.classes_build():
        for trial in range(200):
            n = int(rng.integers(1, 40))
            items = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
            sets = ss.parse_classes("".join(items))
            value, mask = ss.classes_cover(sets)
            a, d = ss.masked_choose_filter(value, mask)
            live = [i for i in range(n) if mask[i]]
            if live:
                assert mask[a] != 0 and mask[a + d] != 0, items
            pat = _device_or_argument_error(lambda: ss.ClassPattern.from_sets(sets))
            if pat is not None:
                info = pat.info()
                assert (info["anchor"], info["distance"]) == (a, d), items
                assert info["single"] + info["masked"] + info["inexact"] == n


# ---- the host side in a program of its own -----------------------------------------------------------------------------------------
def test_the_parser_the_cover_and_the_plan_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/classes_host_check.cpp: parse_classes on every text up to length 4 over the alphabet a [ ] ^ - \\ d { 2 } . (no
    crash, the column inside the text, nothing written behind the capacity), class_cover against the definition, make_class_plan
    against a classification written out and at both limits.  A program of its own, compiled for the host and run as a child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "classes_host_check.cpp")
    exe = str(tmp_path / "classes_host_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 90000                     # (the sweep ran)


# ---- the rule and the fixture ------------------------------------------------------------------------------------------------------
def test_the_numpy_rule_agrees_with_re_and_the_fixture_is_what_the_generator_gives():
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    kat = json.load(open(os.path.join(GOLDEN, "classes_kat.json")))
    assert kat == json.loads(json.dumps(G.make(data)))
    assert os.path.getsize(os.path.join(GOLDEN, "classes_kat.json")) < 16384 and kat["bytes"] == len(data)
    by_name = {c["name"]: c for c in kat["cases"]}
    assert [c["name"] for c in kat["cases"]] == [c[0] for c in G.CASES]
    for needed in (r"[0-9]{3}", r"\d{4}", r"[0-9A-F]{4}H", r"[Ff]igure \d\d-\d", r"\d\d:\d\d", r"[^ -~\n]", r"\w{8}", r"[^a-z]the[^a-z]", r"\s\s",
                   r"[aeiou]{3}", r"a.b", r"[a-c]x"):
        assert any(c["pattern"] == needed and not c["ignore_case"] for c in kat["cases"]), needed
    assert sum(c["ignore_case"] for c in kat["cases"]) == 2
    # the values the issue names, for orientation
    for name, count, lines in (("three_digits", 3504, 1136), ("four_digits", 2068, 903), ("hex_word", 122, 115), ("clock", 90, 74),
                               ("not_printable", 53599, 3003), ("eight_word_bytes", 46025, 10063), ("the_between_non_letters", 6525, 4113),
                               ("two_blanks", 136511, 8152), ("three_vowels", 87, 70)):
        assert (by_name[name]["count"], by_name[name]["lines"]) == (count, lines), name
    assert [by_name[k]["count"] for k in ("figure_number", "a_any_b", "a_any_b_nocase", "a_to_c_x", "a_to_c_x_nocase")] == [28, 127, 154, 31, 760]
    arr = np.frombuffer(data, dtype=np.uint8)
    with ss.classes_build():
        for c in kat["cases"]:
            sets = ss.parse_classes(c["pattern"], c["ignore_case"])
            offs = rule_offsets(arr, sets)
            assert offs.size == c["count"], c["name"]
            if "offsets" in c:
                assert offs.tolist() == c["offsets"], c["name"]
            else:
                assert G.list_hash(offs.tolist()) == c["offsets_sha256"] and offs[:16].tolist() == c["first"] and offs[-16:].tolist() == c["last"], c["name"]
            assert rule_lines(arr, sets, c["delimiter"])[0].size == c["lines"], c["name"]
        # the rule's corners: a class that accepts the delimiter, the unterminated last line, an empty view
        for text in (r"a.b", r"a[^x]b"):
            s = ss.parse_classes(text)
            assert rule_offsets(b"a\nb", s).tolist() == [0] and rule_lines(b"a\nb", s, 10)[0].size == 0
            assert [x.tolist() for x in rule_lines(b"xx\nayb", s, 10)] == [[3], [6], [2]]
            assert [x.tolist() for x in rule_lines(b"ayb\n\naab\n", s, 10)] == [[0, 5], [3, 8], [1, 3]]
            assert rule_offsets(b"", s).size == 0 and rule_lines(b"", s, 10)[0].size == 0
