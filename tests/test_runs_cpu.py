"""CPU checks of the run calls (include/sliceslice_hip_runs.h): the header, the ctypes table and the Rust module agree symbol by
symbol; the seventeenth library stands on the classes one and no other build holds any of it; the new kernels use no private
segment, spill no vector register and little LDS; ss_runs_parse agrees with Python's `re` on what it accepts and refuses what the
header says, with the column; runs_swar.hpp and runs_host.hpp in a program of their own under ASan and UBSan; the numpy rule the GPU
tests use agrees with `re`'s look-around form, and tests/golden/runs_kat.json is what its generator produces now."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes
from test_classes_cpu import members, re_set, sets_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_runs_golden as G            # noqa: E402

RUNS = ["ss_runs_new", "ss_runs_free", "ss_runs_info", "ss_runs_parse", "ss_count_runs_device", "ss_count_runs_device_async",
        "ss_find_all_runs_device", "ss_count_lines_runs_device", "ss_find_lines_runs_device"]


def rule_runs(data, set_words, min_len=1, max_len=None, delimiter=None):
    """THE RULE in numpy: (begin, end) of the maximal runs of members whose length lies in [min_len, max_len]; with a delimiter that
    byte is never a member.  What the GPU tests compare with."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    table = members(np.asarray(set_words, dtype=np.uint64).reshape(1, 4))[0].copy()
    if delimiter is not None:
        table[delimiter] = False
    m = np.concatenate([[False], table[data], [False]]).astype(np.int8)
    d = np.diff(m)
    begin, end = np.flatnonzero(d == 1).astype(np.int64), np.flatnonzero(d == -1).astype(np.int64)
    length = end - begin
    keep = (length >= min_len) & ((length <= max_len) if max_len else True)
    return begin[keep], end[keep]


def rule_lines(data, set_words, min_len, max_len, delimiter):
    """(begin, end, number) of the lines that hold a selected run, as sliceslice_hip_lines.h lays records out."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    begin, _ = rule_runs(data, set_words, min_len, max_len, delimiter)
    delims = np.flatnonzero(data == delimiter).astype(np.int64)
    ends = np.append(delims, data.size) if (delims.size == 0 or delims[-1] != data.size - 1) and data.size else delims
    begins = np.concatenate([[0], delims + 1])[:ends.size]
    sel = np.unique(np.searchsorted(ends, begin, side="left"))
    return begins[sel], ends[sel], sel + 1


# ---- header, ctypes table, Rust block, build ---------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_runs.h")
    assert sorted(c) == sorted(ss.searcher.RUNS_ABI) == sorted(RUNS)
    masked = header_prototypes("sliceslice_hip_masked.h")
    for name in ("ss_count_%s_device", "ss_count_%s_device_async", "ss_count_lines_%s_device", "ss_find_lines_%s_device"):
        assert c[name % "runs"] == masked[name % "masked"], name
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_runs.h")).read()
    flatc = " ".join(text.split())
    flatm = " ".join(open(os.path.join(ROOT, "include", "sliceslice_hip_masked.h")).read().split())
    for name in ("ss_count_lines_%s_device(", "ss_find_lines_%s_device("):       # argument for argument, by name, after the first
        mine = re.search(re.escape(name % "runs") + r"const ss_runs \*runs, ([^;]*);", flatc).group(1)
        model = re.search(re.escape(name % "masked") + r"const ss_masked \*pattern, ([^;]*);", flatm).group(1)
        assert mine == model, name
    assert c["ss_runs_new"] == ("i32", ["ptr", "u64", "u64", "u32", "ptr"]) and c["ss_runs_free"] == ("void", ["ptr"])
    assert c["ss_runs_info"] == ("i32", ["ptr", "i32", "ptr"]) and c["ss_runs_parse"] == ("i32", ["ptr", "i32", "ptr", "ptr", "ptr"])
    assert c["ss_find_all_runs_device"] == ("i32", ["ptr", "ptr", "usize", "ptr", "ptr", "ptr", "u64", "ptr"])
    r = rust_prototypes("hip_runs.rs")
    assert r == c, (r, c)
    rust = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_runs.rs")).read()
    assert "pub const SS_RUNS_MAX_LEN: u64 = 4096;" in rust and "pub const SS_RUNS_MAX_RANGES: usize = 4;" in rust
    assert "pub const SS_RUNS_BITMAP: c_uint = 1;" in rust
    assert re.search(r"#define SS_RUNS_MAX_LEN\s+4096\b", text) and re.search(r"#define SS_RUNS_MAX_RANGES\s+4\b", text)
    assert re.search(r"#define SS_RUNS_BITMAP\s+1u\b", text)
    assert (ss.RUNS_MAX_LEN, ss.RUNS_MAX_RANGES, ss.SS_RUNS_BITMAP) == (4096, 4, 1)
    for name, (res, args) in ss.searcher.RUNS_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_runs.h":
            assert not set(c) & set(header_prototypes(h)), h
    assert '#include "sliceslice_hip_classes.h"' in text
    assert "hip_runs.rs" in open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "build.rs")).read()
    # the stats are six 64-bit words in the order of the Python names, and of the Rust struct
    body = re.search(r"typedef struct ss_runs_stats \{(.*?)\}", text, flags=re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]+);", body) for f in decl.split(",")]
    assert fields == list(ss.searcher.RUNS_STATS) == ["min_len", "max_len", "members", "ranges", "path", "accepts_delimiter"]
    assert re.findall(r"pub (\w+): u64,", re.search(r"pub struct ss_runs_stats \{(.*?)\}", rust, flags=re.S).group(1)) == fields
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).split())
    for said in ("THE RULE", "a non-empty set of byte values", "bit b & 63 of word b >> 6", "The full set is allowed",
                 "a maximal interval [begin, end) of the view whose bytes are all in the set", "begin == 0 or hay[begin-1] is not in the set",
                 "end == len or hay[end] is not in the set", "Bytes outside [0, len) are absent",
                 "no load touches a 16-byte block that holds no byte of the view", "min_len <= end - begin", "max_len == 0 (no maximum)",
                 "1 <= min_len <= SS_RUNS_MAX_LEN (4,096)", "min_len <= max_len <= SS_RUNS_MAX_LEN", "A run that is too long is not selected",
                 "a run is never chopped into pieces", "(?<![C])[C]{min,max}(?![C])", 're.finditer(rb"[C]{min,}")',
                 '"overlapping" and "disjoint" mean the same thing here', "the delimiter is never a member in the line calls",
                 "a run is cut at every delimiter", "A line matches when it holds a selected run", "sliceslice_hip_lines.h's",
                 "A set that is only the delimiter matches no line and is not refused", "64-bit", "exactly ONE item",
                 "`+`, `{k}`, `{k,}`, `{k,m}`", "which would match the empty string", "a missing quantifier", "anything behind the quantifier",
                 "k or m above 4,096", "m < k", "HOST ONLY", "SS_RUNS_BITMAP forces the bitmap path", "needs no scratch memory",
                 "can be captured into a hipGraph", "Either array may be NULL", "*total is always the full count", "ss_find_all_masked_device's",
                 "argument for argument, with `runs` first", "Refused with SS_ERR_ARGUMENT", "nothing written", "an unknown flag",
                 "a handle made on another device", "SS_RUNS_MAX_RANGES (4)", "exact for all 256 values", "no byte is read twice",
                 "max(min_len, max_len + 1)", "linear in the view", "is read a second time, one lane per run", "the only atomic",
                 "32 bytes per workgroup", "The output depends on the input alone", "Out of scope", "more than one item", "`*` and `?`",
                 "chopping long runs", "word / inverted / context / batched / replace forms", "counting member bytes or the longest run"):
        assert said.lower() in flat.lower(), said


def test_the_seventeenth_library_stands_on_the_classes_one():
    b = _build()
    entry = b._lib("runs")
    assert entry["parent"] == "classes" and entry["sources"] == ["ss_runs.hip"]
    # a fourth mapping below the three that are pinned name by name, which are what they were
    assert list(b._NEWEST_LIBRARIES) == ["runs"] and b._NEWEST_LIBRARIES["runs"] is entry
    assert list(b._LATEST_LIBRARIES) == ["masked", "classes"] and list(b._LATER_LIBRARIES) == ["output", "leftmost"]
    assert "runs" not in b.LIBRARIES and len(b.LIBRARIES) == 12
    source = open(os.path.join(ROOT, "sliceslice-rs_amd", "_build.py")).read()
    assert source.index("_LATER_LIBRARIES = {") < source.index("_LATEST_LIBRARIES = {") < source.index("_NEWEST_LIBRARIES = {")
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_runs.so" == os.path.basename(b.runs_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_runs.json" == os.path.basename(b.runs_resources_path())
    assert callable(b.build_runs) and callable(b.runs_kernel_resources)
    assert "sliceslice-rs_amd/csrc/kernel_resources_runs.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("runs") == b._all_sources("classes") + ["ss_runs.hip"]
    for h in ("runs_host.hpp", "runs_swar.hpp", "runs_kernels.hpp", "runs_launch.hpp", os.path.join("..", "..", "include", "sliceslice_hip_runs.h")):
        assert h in b._HEADERS, h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index('b.build_library("classes", force=True, verbose=True)') < \
        entry_point.index('b.build_library("runs", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["runs"][0] is ss.searcher.RUNS_ABI and ss.searcher._FEATURES["runs"][1] == "ss_runs_new"
    product = ss.lib()
    assert not getattr(product, "has_runs")
    with ss.classes_build() as L:
        assert not L.has_runs
    with ss.runs_build() as L:
        assert ss.lib() is L and L.has_runs and L.has_classes and L.has_masked and L.has_lines and ss.searcher._feature_lib(L, "runs") is L
    assert ss.lib() is product
    classes = _exported(b.build_classes())
    assert _exported(b.build_runs()) == sorted(classes + RUNS)
    assert not set(RUNS) & set(classes) and not set(RUNS) & set(_exported(ss.build()))
    # the kernels include the masked ones: neither edited nor copied
    kernels = open(os.path.join(CSRC, "runs_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in kernels.splitlines())
    assert '#include "masked_kernels.hpp"' in kernels and '#include "masked_launch.hpp"' in open(os.path.join(CSRC, "runs_launch.hpp")).read()
    for called in ("masked_load<U>(", "set_valid_bits(", "kSetU", "kSetTiles", "line_capture<U>(", "line_tile_done<U, false>(", "wave_exclusive_sum(",
                   "runs_in_range4(", "from_next_lane_or(", "__builtin_amdgcn_readlane("):
        assert called in code, called
    assert "masked_filter" not in code and "masked_verify" not in code
    host = open(os.path.join(CSRC, "ss_runs.hip")).read()
    everything = code + "\n".join(l.split("//")[0] for l in host.splitlines())
    assert "asm" not in everything and "__threadfence" not in everything and "volatile" not in everything and everything.count("atomic") == 1
    assert "launch_set_prefix(" in host and "hipMalloc" not in host
    # the range test is plain C++ that the host can include
    swar = open(os.path.join(CSRC, "runs_swar.hpp")).read()
    assert "hip_runtime" not in swar and "#include <hip" not in swar and "__host__ __device__" in swar and "#if defined(__HIPCC__)" in swar
    parser = open(os.path.join(CSRC, "runs_host.hpp")).read()
    assert "detail::escape(" in parser and "detail::bracket(" in parser and "hip_runtime" not in parser and "__device__" not in parser


def test_every_other_build_refuses_and_names_the_build():
    message = ss.searcher._FEATURES["runs"][2]
    assert "ss.runs_build()" in message and "libsliceslice_hip_runs.so" in message
    calls = (lambda: ss.RunPattern(r"\w+"), lambda: ss.RunPattern.from_set(np.ones(4, dtype=np.uint64)), lambda: ss.parse_runs("a+"))
    for call in calls:
        with pytest.raises(ss.SlicesliceError, match=r"ss\.runs_build\(\)") as e:
            call()
        assert e.value.code == ss.SS_ERR_ARGUMENT
    with ss.classes_build():
        for call in calls:
            with pytest.raises(ss.SlicesliceError, match=r"ss\.runs_build\(\).*|.*libsliceslice_hip_runs\.so") as e:
                call()
            assert e.value.code == ss.SS_ERR_ARGUMENT


def test_the_new_kernels_use_no_private_segment_spill_nothing_and_little_lds():
    rows = {r["name"]: r for r in _build().runs_kernel_resources() if r["tu"] == "ss_runs.hip"}
    names = sorted(rows)
    assert len(names) == 4 and all("ss::runs_all_kernel" in n or "ss::runs_lines_kernel" in n for n in names), names
    for name, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r.get("agprs", 0) == 0, (name, r)
        assert r["lds_bytes"] <= 16 * 1024, (name, r)


# ---- ss_runs_parse -------------------------------------------------------------------------------------------------------------------
ITEMS = [r"a", r"Z", r" ", r"-", "\xe9", r".", r"\d", r"\D", r"\w", r"\W", r"\s", r"\S", r"\n", r"\x00", r"\xff", r"\.", r"\+", r"\*", r"\{",
         r"[0-9]", r"[0-9A-F]", r"[0-9a-fA-F]", r"[A-Z]", r"[^\n]", r"[^a]", r"[a-c]", r"[+*?{}]", r"[\w-]", r"[^\s\w]", r"[\x80-\xff]", r"[,]"]
QUANTIFIERS = [("+", 1, None), ("{1}", 1, 1), ("{3}", 3, 3), ("{3,}", 3, None), ("{2,5}", 2, 5), ("{4096}", 4096, 4096), ("{1,4096}", 1, 4096),
               ("{4096,}", 4096, None), ("{7,7}", 7, 7), ("{080,}", 80, None)]


def test_every_accepted_form_means_what_re_means_by_it():
    with ss.runs_build():
        for item in ITEMS:
            for ignore_case in (False, True):
                for quantifier, lo, hi in QUANTIFIERS:
                    words, got_lo, got_hi = ss.parse_runs(item + quantifier, ignore_case)
                    assert words.shape == (4,) and words.dtype == np.uint64 and (got_lo, got_hi) == (lo, hi), (item, quantifier)
                    assert (members(words.reshape(1, 4))[0] == re_set(item, ignore_case)).all(), (item, ignore_case)
        assert (ss.parse_runs(rb"\w+")[0] == ss.parse_runs(r"\w+")[0]).all()
        assert not members(ss.parse_runs(r"[^a]+", True)[0].reshape(1, 4))[0][ord("A")]
        assert members(ss.parse_runs(r".+")[0].reshape(1, 4))[0].all()


REFUSED = [
    # (text, column)
    ("", 1), ("a", 1), (r"\w", 2), (r"[0-9]", 5), ("a*", 2), ("a?", 2), (r"\w*", 3), ("a{0}", 3), ("a{0,}", 3), ("a{0,5}", 3), ("a{,5}", 3),
    ("a+b", 3), ("a++", 3), ("a+?", 3), ("a{2}{3}", 5), ("ab+", 2), (r"\d\d+", 3), ("a{4097}", 3), ("a{2,4097}", 5), ("a{4097,}", 3),
    ("a{99999999999999999999,}", 3), ("a{5,2}", 5), ("a{}", 3), ("a{2", 3), ("a{2,", 4), ("a{2,x}", 5), ("a{x}", 3), ("a{2,3", 5), ("a{ 2}", 3),
    ("+", 1), ("*", 1), ("{2}", 1), ("(a)+", 1), ("^a+", 1), ("a|b", 2), ("[a", 1), ("[]+", 2), (r"\q+", 2), ("[z-a]+", 2), (r"\w+$", 4),
    ("a{3,5}x", 7), (r"[^\x00-\xff]+", 1), (r"\x4+", 4),
]


def test_every_refusal_names_its_column_and_writes_nothing():
    import ctypes
    with ss.runs_build():
        for text, column in REFUSED:
            for ignore_case in (False, True):
                with pytest.raises(ss.SlicesliceError, match=r"ss_runs_parse: column %d\b" % column) as e:
                    ss.parse_runs(text, ignore_case)
                assert e.value.code == ss.SS_ERR_ARGUMENT, text
        with pytest.raises(ss.SlicesliceError, match=r"column 2\b") as e:
            ss.parse_runs(b"a\0+")
        for text, said in (("a*", "empty string"), ("a{,3}", "empty string"), ("a{0,3}", "empty string"), ("a", "not followed"),
                           ("a+b", "behind the quantifier"), ("a{5000}", "4096"), ("a{3,2}", "m < k")):
            with pytest.raises(ss.SlicesliceError, match=said):
                ss.parse_runs(text)
        L = ss.lib()
        words = np.full(4, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        lo, hi = ctypes.c_uint64(77), ctypes.c_uint64(77)
        assert L.ss_runs_parse(b"a*", 0, words.ctypes.data, ctypes.byref(lo), ctypes.byref(hi)) == ss.SS_ERR_ARGUMENT
        assert L.ss_runs_parse(None, 0, words.ctypes.data, ctypes.byref(lo), ctypes.byref(hi)) == ss.SS_ERR_ARGUMENT
        assert L.ss_runs_parse(b"a+", 0, None, ctypes.byref(lo), ctypes.byref(hi)) == ss.SS_ERR_ARGUMENT
        assert L.ss_runs_parse(b"a+", 0, words.ctypes.data, None, ctypes.byref(hi)) == ss.SS_ERR_ARGUMENT
        assert L.ss_runs_parse(b"a+", 0, words.ctypes.data, ctypes.byref(lo), None) == ss.SS_ERR_ARGUMENT
        assert (words == 0x5A5A5A5A5A5A5A5A).all() and lo.value == 77 and hi.value == 77
        # ss_runs_new refuses on the host, before it asks for a device
        h = ctypes.c_void_p(1234)
        one = np.array([1, 0, 0, 0], dtype=np.uint64)
        for args in ((None, 1, 0, 0), (np.zeros(4, dtype=np.uint64).ctypes.data, 1, 0, 0), (one.ctypes.data, 0, 0, 0), (one.ctypes.data, 4097, 0, 0),
                     (one.ctypes.data, 1, 4097, 0), (one.ctypes.data, 5, 4, 0), (one.ctypes.data, 1, 0, 2), (one.ctypes.data, 1, 0, 0x80000000)):
            assert L.ss_runs_new(*args, ctypes.byref(h)) == ss.SS_ERR_ARGUMENT and L.ss_last_error(), args
        assert L.ss_runs_new(one.ctypes.data, 1, 0, 0, None) == ss.SS_ERR_ARGUMENT
        assert h.value == 1234
        L.ss_runs_free(None)


# ---- the host side in a program of its own -----------------------------------------------------------------------------------------
def test_the_range_test_the_ranges_and_the_parser_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/runs_host_check.cpp: the SWAR range test against the plain comparison for every (lo, hi) and every byte value in
    every lane, the split into maximal ranges, the parser on its refusals.  A program of its own, compiled for the host and run as a
    child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "runs_host_check.cpp")
    exe = str(tmp_path / "runs_host_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 32896 * 256 * 12           # (the sweep ran: every (lo, hi), value, lane and fill)


# ---- the rule and the fixture ------------------------------------------------------------------------------------------------------
def test_the_numpy_rule_agrees_with_re_on_random_data():
    rng = np.random.default_rng(11)
    items = [(r"[ab]", b"ab"), (r"\w", None), (r"[^\n]", None), (r"a", b"a"), (r".", None), (r"[a\n]", b"a\n")]
    for item, _ in items:
        words = sets_of(re_set(item))[0]
        for alphabet in (b"ab", b"aab\n", b"ab_ \n\xe9"):
            data = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), 3000).tobytes()
            for quantifier, lo, hi in (("+", 1, None), ("{1}", 1, 1), ("{2,}", 2, None), ("{3}", 3, 3), ("{2,4}", 2, 4), ("{7,}", 7, None)):
                want = G.runs_of(data, item, quantifier, False)
                begin, end = rule_runs(data, words, lo, hi)
                assert list(zip(begin.tolist(), end.tolist())) == [tuple(r) for r in want], (item, quantifier)
                if hi is None:                                      # with no maximum: exactly what finditer of [C]{min,} yields
                    plain = [m.span() for m in re.finditer(item.encode() + b"{%d,}" % lo, data, re.S)]
                    assert plain == [tuple(r) for r in want]
                for delimiter in (10, ord("a")):
                    lines = rule_lines(data, words, lo, hi, delimiter)
                    assert lines[0].size == G.lines_of(data, item, quantifier, False, delimiter), (item, quantifier, delimiter)
    # corners: the empty view, one run that is the whole view, a set that is only the delimiter
    full = np.full(4, ~np.uint64(0))
    assert rule_runs(b"", full)[0].size == 0 and [x.tolist() for x in rule_runs(b"abc", full)] == [[0], [3]]
    assert rule_lines(b"\n\n", sets_of(re_set(r"\n"))[0], 1, None, 10)[0].size == 0
    assert [x.tolist() for x in rule_lines(b"ab\n\ncd", full, 2, None, 10)] == [[0, 4], [2, 6], [1, 3]]


def test_the_fixture_is_what_the_generator_gives_and_holds_the_issues_numbers():
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    kat = json.load(open(os.path.join(GOLDEN, "runs_kat.json")))
    assert kat == json.loads(json.dumps(G.make(data)))
    assert os.path.getsize(os.path.join(GOLDEN, "runs_kat.json")) < 32768 and kat["bytes"] == len(data) == 857425
    by_name = {c["name"]: c for c in kat["cases"]}
    assert [c["name"] for c in kat["cases"]] == [c[0] for c in G.CASES]
    for name, count in (("words", 119587), ("numbers", 13677), ("wc_w", 119666), ("three_digits_or_more", 1436), ("eight_word_bytes_or_more", 18784),
                        ("two_blanks_or_more", 18778), ("long_lines", 163), ("exactly_three_digits", 363), ("two_to_five_capitals", 14021)):
        assert by_name[name]["count"] == count and by_name[name + "_nocase"]["pattern"] == by_name[name]["pattern"], name
    assert by_name["three_digits_or_more"]["lines"] == 1136 and by_name["wc_w"]["count"] == len(data.split())
    arr = np.frombuffer(data, dtype=np.uint8)
    with ss.runs_build():
        for c in kat["cases"]:
            words, lo, hi = ss.parse_runs(c["pattern"], c["ignore_case"])
            begin, end = rule_runs(arr, words, lo, hi)
            runs = list(zip(begin.tolist(), end.tolist()))
            assert len(runs) == c["count"] and G.list_hash(runs) == c["runs_sha256"], c["name"]
            assert [list(r) for r in runs[:G.KEEP]] == c["first"] and [list(r) for r in runs[-G.KEEP:]] == c["last"], c["name"]
            assert rule_lines(arr, words, lo, hi, c["delimiter"])[0].size == c["lines"], c["name"]
        # the cross-check against the classes library's fixture: sum of max(0, L - 7) over the \w+ runs == the \w{8} occurrences
        begin, end = rule_runs(arr, ss.parse_runs(r"\w+")[0])
    classes = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "classes_kat.json")))["cases"]}
    assert int(np.maximum(0, end - begin - 7).sum()) == classes["eight_word_bytes"]["count"] == 46025
