"""CPU checks of the output calls (include/sliceslice_hip_output.h): the header, the ctypes table and the Rust module agree symbol by
symbol; libsliceslice_hip_output.so exports the disjoint library's list plus three functions; the build table is what it was and the
thirteenth library stands below it; the new kernels use no private segment, no spill and no AGPR and every row of the disjoint
record reappears unchanged; the arithmetic of csrc/output_host.hpp passes a sweep against snprintf and the rule written out as a loop
in a stand-alone host program built with ASan and UBSan; tests/golden/output_kat.json is what the rule restated in Python gives; the
new Python calls are refused outside output_build(); tools/grep_hip.py documents --device-output."""
import hashlib
import inspect
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
OUTPUT = ["ss_format_lines_device", "ss_gather_ranges_device", "ss_grep_lines_device"]
KERNELS = ["ss::output_sizes_kernel", "ss::output_starts_kernel", "ss::output_copy_kernel"]


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_output.h")
    assert sorted(c) == sorted(ss.searcher.OUTPUT_ABI) == sorted(OUTPUT)
    assert c["ss_format_lines_device"] == ("i32", ["ptr", "ptr", "usize", "ptr", "ptr", "ptr", "ptr", "u64", "i32", "u32", "ptr", "ptr", "u64", "ptr", "ptr"])
    assert c["ss_gather_ranges_device"] == ("i32", ["ptr", "ptr", "usize", "ptr", "ptr", "u64", "i32", "ptr", "ptr", "u64", "ptr", "ptr"])
    # ss_find_lines_context_device's list up to `after`, then the flags, the stream, the buffer and the three results
    assert c["ss_grep_lines_device"] == ("i32", ["ptr", "ptr", "usize", "i32", "u32", "u64", "u64", "u32", "ptr", "ptr", "u64", "ptr", "ptr", "ptr"])
    assert c["ss_grep_lines_device"][1][:7] == header_prototypes("sliceslice_hip_context.h")["ss_find_lines_context_device"][1][:7]
    r, rust = rust_prototypes("hip_output.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_output.rs")).read()
    assert r == c, (r, c)
    for const in ("pub const SS_OUTPUT_BLOCK: u64 = 4096;", "pub const SS_OUTPUT_CHUNK: u64 = 16384;", "pub const SS_OUTPUT_NUMBER: c_uint = 1;",
                  "pub const SS_OUTPUT_SEPARATOR: c_uint = 2;"):
        assert const in rust, const
    for name, (res, args) in ss.searcher.OUTPUT_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_output.h":
            assert not set(c) & set(header_prototypes(h)), h
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_output.h")).read()
    assert '#include "sliceslice_hip_disjoint.h"' in text and "typedef struct" not in text
    assert re.search(r"#define SS_OUTPUT_BLOCK\s+4096u", text) and ss.OUTPUT_BLOCK == ss.searcher.OUTPUT_BLOCK == 4096
    assert re.search(r"#define SS_OUTPUT_CHUNK\s+16384u", text) and ss.OUTPUT_CHUNK == ss.searcher.OUTPUT_CHUNK == 16384
    assert re.search(r"#define SS_OUTPUT_NUMBER\s+1u", text) and re.search(r"#define SS_OUTPUT_SEPARATOR\s+2u", text)
    assert (ss.SS_OUTPUT_NUMBER, ss.SS_OUTPUT_SEPARATOR) == (1, 2)


def test_the_header_states_the_rule_and_the_refusals():
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_output.h")).read()
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).lower().split())
    for topic in ("Rule:", "contributes, in this order", "with SS_OUTPUT_SEPARATOR, and i > 0, and number[i] > number[i-1] + 1",
                  "the two bytes `--` and the terminator", "with SS_OUTPUT_NUMBER: the decimal digits of number[i]", "no leading zeros",
                  "1 to 20 digits", "0 prints `0`", "followed by `:` when kind[i] != 0 or d_kind is NULL, else by `-`",
                  "e = min(end[i], len) and b = min(begin[i], e)", "Nothing outside the view is ever copied, whatever the records say",
                  "the terminator byte, when `terminator` is 0..255", "-1 means none, and then the separator is `--` alone",
                  "the concatenation over i = 0 .. count-1", "Records may overlap, repeat or descend", "a descending pair gets no separator",
                  "without wrapping", "d_starts[i] is the output offset where record i's contribution begins, separator included",
                  "d_starts[count] equals *out_len", "Everything is 64-bit", "names the device and its scratch only",
                  "*out_len is always set", "written whenever it is non-NULL", "If out_capacity < *out_len, nothing is written to d_out and the call returns SS_OK",
                  "ss_replace_device", "nothing is written at *out_len or beyond", "d_out may have any alignment", "count == 0 gives 0 with no launch",
                  "Waits for the stream", "the same launches with flags == 0 and no numbers", "grep -o", "sed -n 'Np'",
                  "25 bytes per printed line", "returned inside the call", "terminator = delimiter", "SS_CONTEXT_INVERT included",
                  "passed through", "still reports *out_len, *lines and *selected", "Refused with SS_ERR_ARGUMENT", "nothing written",
                  "unknown flag bits", "a terminator outside -1..255", "NULL d_number", "NULL d_begin / d_end", "a NULL out_len",
                  "count >= 2^48", "intersects the haystack's range", "a capturing stream", "SS_ERR_NOMEM or SS_ERR_HIP",
                  "16 bytes per block", "one workgroup per SS_OUTPUT_CHUNK bytes", "16-byte aligned address at or below d_out",
                  "ONE 16-byte store", "stored exactly once", "no load touches a 16-byte block that holds no byte of the view",
                  "no workgroup waits for another", "no global atomic", "depends on the input alone", "DESIGN.md 5.17", "Out of scope",
                  "libsliceslice_hip_output.so"):
        assert topic.lower() in flat, topic
    # the neighbours point here and keep the words that the earlier tests look for
    for name, kept in (("sliceslice_hip_context.h", "the library returns no separators, the caller derives them"),
                       ("sliceslice_hip_anyof.h", "regular expressions; multi-byte terminators"),
                       ("sliceslice_hip_needleset.h", "an occurrence (non-line) form for sets")):
        old = open(os.path.join(ROOT, "include", name)).read()
        assert kept in " ".join(re.sub(r"^ \*", "", old, flags=re.M).split()) and "sliceslice_hip_output.h" in old, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.17" in design and "sliceslice_hip_output.h" in design.split("5.17", 1)[1]


# ---- the build ----------------------------------------------------------------------------------------------------------------------
def test_the_table_is_what_it_was_and_the_thirteenth_library_stands_below_it():
    b = _build()
    assert list(b.LIBRARIES) == ["service", "matches", "matches_batched", "lines", "nocase", "bounded", "inverted", "context", "anyof", "needleset",
                                 "setmatches", "disjoint"]
    entry = b._lib("output")
    assert entry["parent"] == "disjoint" and entry["sources"] == ["ss_output.hip"] and "output" not in b.LIBRARIES
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_output.so" == os.path.basename(b.output_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_output.json" == os.path.basename(b.output_resources_path())
    assert "sliceslice-rs_amd/csrc/kernel_resources_output.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("output") == b._all_sources("disjoint") + ["ss_output.hip"] and b.library_path_of("output") == entry["so"]
    assert callable(b.build_output) and callable(b.output_kernel_resources)
    with pytest.raises(KeyError):
        b._lib("no such library")
    for h in ("output_kernels.hpp", "output_launch.hpp", "output_host.hpp", os.path.join("..", "..", "include", "sliceslice_hip_output.h")):
        assert h in b._HEADERS and os.path.exists(os.path.join(CSRC, h)), h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index("for name in b.LIBRARIES:") < entry_point.index('b.build_library("output", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["output"][0] is ss.searcher.OUTPUT_ABI and ss.searcher._FEATURES["output"][1] == "ss_format_lines_device"
    product = ss.lib()
    assert not getattr(product, "has_output")
    with ss.output_build() as L:
        assert ss.lib() is L and L.has_output and L.has_disjoint and L.has_context and ss.searcher._feature_lib(L, "output") is L
    assert ss.lib() is product
    with ss.disjoint_build() as L:
        assert not L.has_output
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "libsliceslice_hip_output.so" in readme and "thirteenth" in readme
    assert "hip_output.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hip_output.rs" in open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "build.rs")).read()


def test_the_output_library_exports_the_disjoint_list_plus_three():
    b = _build()
    disjoint = _exported(b.build_disjoint())
    assert _exported(b.build_output()) == sorted(disjoint + OUTPUT)
    assert not set(OUTPUT) & set(disjoint) and not set(OUTPUT) & set(_exported(ss.build()))


def test_the_new_kernels_use_no_private_segment_and_every_other_row_is_what_it_was():
    b = _build()
    rows = b.output_kernel_resources()
    own = [r for r in rows if r["tu"] == "ss_output.hip"]
    names = sorted(r["name"].split("(")[0] for r in own)
    assert names == sorted(KERNELS + ["void ss::prefix_kernel<unsigned long>"]), names
    for r in own:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["agprs"] == 0, r
        assert r["lds_bytes"] <= 48 * 1024, r
    copy = [r for r in own if "output_copy_kernel" in r["name"]][0]
    assert copy["vgprs"] <= 128 and copy["waves_per_simd"] >= 4 and copy["lds_bytes"] <= 20 * 1024, copy
    disjoint = b.disjoint_kernel_resources()
    assert [r for r in rows if r["tu"] != "ss_output.hip"] == disjoint and len(rows) == len(disjoint) + 4
    assert not [r for r in disjoint if "output" in r["name"] or "output" in r["tu"]]
    text = open(os.path.join(CSRC, "output_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    # no waiting between workgroups, no atomic of any kind, no inline assembly; one 16-byte load and one 16-byte store per unit
    assert "asm" not in code and "__threadfence" not in code and "atomic" not in code and "volatile" not in code
    assert "*reinterpret_cast<uint4 *>(a.out_base + u)" in code and "out_u32x4_unaligned" in code and "SS_OUTPUT_CHUNK" in code
    host = open(os.path.join(CSRC, "ss_output.hip")).read()
    for used in ("take_scratch(", "ScratchLease", "prefix_kernel<uint64_t>", "stream_is_capturing(", "hipFree(", "ss_find_lines_context_device(",
                 "total * 25"):
        assert used in host, used
    assert "SS_API" not in open(os.path.join(CSRC, "output_host.hpp")).read()


# ---- the host arithmetic --------------------------------------------------------------------------------------------------------------
def test_digits_sizes_clamps_and_separators_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/output_host_check.cpp: out_digits / out_digit / out_write_decimal against snprintf at every power of ten +- 1 and
    at 2^64 - 1, the size, clamp and separator arithmetic against the rule written out as a loop over all small cases.  A program
    of its own, compiled for the host and run as a child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "output_host_check.cpp")
    exe = str(tmp_path / "output_host_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 1000000                 # (the sweep ran)
    header = open(os.path.join(CSRC, "output_host.hpp")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header and "__device__" not in header
    assert '#define SS_OUTPUT_FN __host__ __device__ __forceinline__' in open(os.path.join(CSRC, "output_kernels.hpp")).read()


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_restated_rule_gives():
    sys.path.insert(0, GOLDEN)
    try:
        import make_output_golden as m
    finally:
        sys.path.remove(GOLDEN)
    kat = json.load(open(os.path.join(GOLDEN, "output_kat.json")))
    data = open(os.path.join(GOLDEN, kat["file"]), "rb").read()
    lines = m.all_lines(data, 10)
    assert kat["lines"] == len(lines) == 20854 and kat["grep_checked"] and "3.7" in kat["grep_version"]
    context = json.load(open(os.path.join(GOLDEN, "context_kat.json")))["rows"]
    assert [(r["needle"], r["how"], r["invert"], r["before"], r["after"]) for r in kat["rows"][:len(context)]] == \
        [(r["needle"], r["how"], r["invert"], r["before"], r["after"]) for r in context]
    assert all(r["line_numbers"] for r in kat["rows"][:len(context)]) and len(kat["rows"]) == len(context) + 2 == len(m.ROWS)
    assert (kat["rows"][-2]["needle"], kat["rows"][-2]["line_numbers"]) == ("", True)
    assert (kat["rows"][-1]["line_numbers"], kat["rows"][-1]["before"], kat["rows"][-1]["after"]) == (False, 0, 1)
    assert kat["rows"][0]["needle"] == "descriptor" and kat["rows"][0]["length"] == 56185
    for row, (needle, how, invert, before, after, line_numbers) in zip(kat["rows"], m.ROWS):
        begin, end, number, kind = m.row_records(data, lines, needle, how, invert, before, after)
        text, starts = m.format_rule(data, begin, end, number, kind, 10, line_numbers, bool(before or after))
        assert len(text) == row["length"] == starts[-1] and hashlib.sha256(text).hexdigest() == row["sha256"], row["needle"]
        assert text[:200].decode("latin-1") == row["first"] and text[-200:].decode("latin-1") == row["last"], row["needle"]
        printed = [r for r in context if (r["needle"], r["how"], r["invert"], r["before"], r["after"]) == (needle.decode(), how, invert, before, after)]
        if printed:                                             # (the lines and the separators that the context fixture counted)
            assert len(begin) == printed[0]["printed"] and text.count(b"\n--\n") + text.startswith(b"--\n") == printed[0]["separators"] * bool(before or after)
    every = kat["rows"][-2]
    assert every["length"] == len(data) + sum(len("%d:" % k) for k in range(1, len(lines) + 1))
    # the rule's corners, by hand
    assert m.format_rule(b"abcdef", [1, 9, 4, 0], [3, 12, 2, 99], [7, 8, 10, 9], [1, 0, 1, 0], 10, True, True) == \
        (b"7:bc\n8-\n--\n10:\n9-abcdef\n", [0, 5, 8, 15, 24])
    assert m.format_rule(b"abcdef", [1, 4], [3, 6], [1, 5], None, None, False, True) == (b"bc--ef", [0, 2, 6])
    assert m.format_rule(b"abc", [0], [3], [2 ** 64 - 1], [0], 0, True, False) == (b"18446744073709551615-abc\x00", [0, 25])
    assert os.path.getsize(os.path.join(GOLDEN, "output_kat.json")) < 16384


# ---- Python and the command-line tool -------------------------------------------------------------------------------------------------
def test_the_new_calls_and_where_they_are_refused():
    assert str(inspect.signature(ss.format_lines)) == \
        "(haystack, begin, end, number=None, kind=None, delimiter=b'\\n', line_numbers=None, separators=False, stream=None)"
    assert str(inspect.signature(ss.format_lines_into)) == \
        "(haystack, begin, end, d_out, number=None, kind=None, delimiter=b'\\n', line_numbers=None, separators=False, d_starts=None, stream=None)"
    assert str(inspect.signature(ss.gather_ranges)) == "(haystack, begin, end, terminator=None, return_starts=False, stream=None)"
    grep = "(self, haystack, before=0, after=0, delimiter=b'\\n', line_numbers=False, stream=None, ignore_case=False, whole_word=False, " \
           "whole_line=False, invert=False)"
    assert str(inspect.signature(ss.DynamicHipSearcher.grep)) == grep == str(inspect.signature(ss.MemchrHipSearcher.grep))
    assert str(inspect.signature(ss.grep_anyof)) == "(searchers, " + grep[len("(self, "):]
    assert str(inspect.signature(ss.NeedleSet.grep)) == \
        "(self, haystack, before=0, after=0, delimiter=b'\\n', line_numbers=False, whole_word=False, whole_line=False, invert=False, stream=None)"
    # ... and the calls they are composed of are what they were
    assert str(inspect.signature(ss.DynamicHipSearcher.find_lines_context)) == \
        "(self, haystack, before=0, after=0, delimiter=b'\\n', capacity=None, stream=None, ignore_case=False, whole_word=False, whole_line=False, invert=False)"
    assert ss.output_build is ss.searcher.output_build and "stdout" in ss.output_build.__doc__
    assert not getattr(ss.lib(), "has_output", False)
    message = ss.searcher._FEATURES["output"][2]
    for name in ("format_lines", "format_lines_into", "gather_ranges", "grep", "grep_anyof", "NeedleSet.grep"):
        assert "output_build" in message and name in message, name
    for fn in (ss.DynamicHipSearcher.grep, ss.NeedleSet.grep):
        assert '_feature_lib(self._L, "output")' in inspect.getsource(fn)
    assert "ss_grep_lines_device" in inspect.getsource(ss.DynamicHipSearcher.grep)
    for fn in (ss.grep_anyof, ss.NeedleSet.grep):                # composed in Python: no C entry of their own
        assert "_format(" in inspect.getsource(fn) and "find_lines" in inspect.getsource(fn)
    # refused by the product library before anything touches a device
    s = ss.DynamicHipSearcher.__new__(ss.DynamicHipSearcher)
    s._L, s._h = ss.lib(), None
    needles = ss.NeedleSet.__new__(ss.NeedleSet)
    needles._L, needles._h = ss.lib(), None
    for call in (lambda: s.grep((0, 0)), lambda: needles.grep((0, 0)), lambda: ss.grep_anyof([s], (0, 0)), lambda: ss.grep_anyof([], (0, 0)),
                 lambda: ss.format_lines((0, 0), [1], [2]), lambda: ss.format_lines_into((0, 0), [1], [2], None),
                 lambda: ss.gather_ranges((0, 0), [1], [2])):
        with pytest.raises(ss.SlicesliceError, match=r"ss\.output_build\(\)") as e:
            call()
        assert e.value.code == ss.SS_ERR_ARGUMENT


def test_grep_hip_device_output_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    tool = os.path.join(ROOT, "tools", "grep_hip.py")

    def grep(*args):
        return subprocess.run([sys.executable, tool] + list(args), capture_output=True, text=True, timeout=300)

    # refused before any library is loaded: --device-output writes what --lines prints
    for args in (("--device-output", "a", words), ("--device-output", "--count-lines", "a", words), ("--device-output", "--lines", "a"),
                 ("--device-output", "--lines", "--count", "a", words), ("--device-output", "--one-pass", "--lines", "a", words)):
        usage = grep(*args)
        assert usage.returncode != 0 and "--device-output --lines" in usage.stderr and "Traceback" not in usage.stderr, (args, usage)
    both = grep("--device-output", "--lines", "-w", "-x", "a", words)
    assert both.returncode != 0 and "exclude each other" in both.stderr
    empty = grep("--device-output", "--lines", "-w", "", words)
    assert empty.returncode != 0 and "empty needle" in empty.stderr
    doc = open(tool).read()
    for said in ("--device-output", "ss_grep_lines_device", "ss_format_lines_device", "libsliceslice_hip_output.so", "ON THE DEVICE", "one copy",
                 "without it nothing changes"):
        assert said in doc, said
    for rel in ("sliceslice-rs_amd/bindings/rust/hip_output.rs", "include/sliceslice_hip_output.h", "tests/native/output_host_check.cpp",
                "tests/test_gpu_output.py", "tests/golden/make_output_golden.py", "tools/fuzz_output.py", "tools/output_bench.py"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
