"""CPU checks of the context calls (include/sliceslice_hip_context.h): the header, the ctypes table and the Rust module agree symbol
by symbol; libsliceslice_hip_context.so exports the six earlier headers plus two functions while every other library exports what
it did; the new kernels meet their resource bar and every row of the
other records is what it was; tools/grep_hip.py documents and refuses what the issue lists; the rule restated here on numpy arrays
reproduces tests/golden/context_kat.json (GNU grep's output); the range arithmetic of csrc/context_ranges.hpp passes an exhaustive
sweep in a stand-alone host program built with ASan and UBSan; the methods are refused outside context_build()."""
import hashlib
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes
from test_bounded_cpu import BOUNDED, LINES, NOCASE, _grep
from test_inverted_cpu import INVERTED, all_lines, inverted_lines_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTEXT = ["ss_lines_around_device", "ss_find_lines_context_device"]
U64_MAX = (1 << 64) - 1


# ---- the rule on numpy arrays ---------------------------------------------------------------------------------------------------
def context_rule(selected, n_lines, before, after):
    """(numbers, kinds): the lines in the union over the valid s of `selected` (1 <= s <= n_lines) of
    [max(1, s - before), min(n_lines, s + after)], once and ascending, and 1 where the line is one of them.  before / after are Python
    integers of any size: an amount of n_lines or more reaches the end of the view, which is what saturating arithmetic gives."""
    sel = np.asarray([int(s) for s in np.asarray(selected).reshape(-1).tolist() if 1 <= int(s) <= n_lines], dtype=np.int64)
    if sel.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8)
    b, a = min(int(before), n_lines), min(int(after), n_lines)
    edge = np.zeros(n_lines + 2, dtype=np.int64)
    np.add.at(edge, np.maximum(1, sel - b), 1)
    np.add.at(edge, np.minimum(n_lines, sel + a) + 1, -1)
    numbers = np.flatnonzero(np.cumsum(edge)[:n_lines + 1] > 0).astype(np.int64)
    chosen = np.zeros(n_lines + 1, dtype=np.uint8)
    chosen[sel] = 1
    return numbers, chosen[numbers]


def separators(numbers):
    return int((np.diff(numbers) > 1).sum())


def checksum(numbers, kinds):
    return hashlib.sha256("".join("%d:%d\n" % p for p in zip(numbers.tolist(), kinds.tolist())).encode()).hexdigest()


def selected_numbers(data, needle, delimiter, how, invert):
    """the numbers of the lines the model call selects (test_inverted_cpu's rule, or its complement)"""
    not_matching = [l[2] for l in inverted_lines_rule(data, needle, delimiter, how)]
    if invert:
        return not_matching
    gone = set(not_matching)
    return [l[2] for l in all_lines(data, delimiter) if l[2] not in gone]


def test_the_rule_on_small_cases():
    assert context_rule([3], 5, 1, 1)[0].tolist() == [2, 3, 4] and context_rule([3], 5, 1, 1)[1].tolist() == [0, 1, 0]
    assert context_rule([1, 5], 5, 9, 0)[0].tolist() == [1, 2, 3, 4, 5] and context_rule([1, 5], 5, 9, 0)[1].tolist() == [1, 0, 0, 0, 1]
    assert context_rule([0, 6], 5, U64_MAX, U64_MAX)[0].size == 0 and context_rule([], 5, 1, 1)[0].size == 0
    assert context_rule([2], 9, U64_MAX, 0)[0].tolist() == [1, 2] and context_rule([2], 4, 0, U64_MAX)[0].tolist() == [2, 3, 4]
    assert separators(np.array([1, 2, 4, 5, 9])) == 2 and separators(np.array([7])) == 0


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_context.h")
    assert sorted(c) == sorted(ss.searcher.CONTEXT_ABI) == sorted(CONTEXT)
    # (searcher, haystack, len, delimiter, ...) as in the line calls; the outputs are the line calls' three arrays plus the kinds
    find_lines = header_prototypes("sliceslice_hip_lines.h")["ss_find_lines_device"][1]
    assert c["ss_lines_around_device"][1] == find_lines[:4] + ["ptr", "u64", "u64", "u64"] + find_lines[4:8] + ["ptr"] + find_lines[8:]
    assert c["ss_find_lines_context_device"][1] == find_lines[:4] + ["u32", "u64", "u64"] + find_lines[4:8] + ["ptr"] + find_lines[8:] + ["ptr"]
    r, rust = rust_prototypes("hip_context.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_context.rs")).read()
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.CONTEXT_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h",
              "sliceslice_hip_nocase.h"):
        assert not set(c) & set(header_prototypes(h)), h
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_context.h")).read()
    assert '#include "sliceslice_hip_inverted.h"' in text and "#define SS_BOUND" not in text
    assert re.search(r"#define SS_CONTEXT_INVERT 8u\b", text) and ss.SS_CONTEXT_INVERT == 8 and "SS_CONTEXT_INVERT: c_uint = 8;" in rust
    part = int(re.search(r"#define SS_CONTEXT_PART_BYTES (\d+)u\b", text).group(1))
    assert part == ss.CONTEXT_PART_BYTES == ss.searcher.CONTEXT_PART_BYTES and part % 4096 == 0 and ("SS_CONTEXT_PART_BYTES: usize = %d;" % part) in rust
    assert ss.searcher.SS_CONTEXT_INVERT & (ss.searcher.SS_BOUND_WORD | ss.searcher.SS_BOUND_LINE | ss.searcher.SS_BOUND_NOCASE) == 0
    for topic in ("Rule:", "Out of scope", "STRICTLY ASCENDING", "breach", "saturate", "2^64 - 1", "separator", "kind", "capacity",
                  "count only", "no global atomic", "never per line", "misaligned view", "capturable",
                  "libsliceslice_hip_context.so", "SS_ERR_NOMEM", "-m", "multi-byte terminators", "regular expressions",
                  "batched, plan, sharded, service"):
        assert topic.lower() in text.lower(), topic
    # the earlier headers point here and keep the words that tests/test_inverted_cpu.py looks for
    for h in ("sliceslice_hip_inverted.h", "sliceslice_hip_bounded.h"):
        old = open(os.path.join(ROOT, "include", h)).read()
        scope = old[old.index("Out of scope"):]
        assert "sliceslice_hip_context.h" in scope and "context lines" in scope and "-m" in scope, h


def test_the_context_library_exports_six_headers_plus_two_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    batched = list(header_prototypes("sliceslice_hip_matches_batched.h"))
    service = list(header_prototypes("sliceslice_hip_service.h"))
    assert _exported(b.build_context()) == sorted(product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT)
    assert _exported(b.build_inverted()) == sorted(product + matches + LINES + NOCASE + BOUNDED + INVERTED)
    assert _exported(b.build_bounded()) == sorted(product + matches + LINES + NOCASE + BOUNDED)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_service()) == sorted(product + service)
    assert _exported(b.build_matches()) == sorted(product + matches)
    assert _exported(b.build_matches_batched()) == sorted(product + matches + batched)
    assert _exported(b.build_lines()) == sorted(product + matches + LINES)
    assert _exported(b.build_nocase()) == sorted(product + matches + LINES + NOCASE)
    assert os.path.basename(b.context_library_path()) == "libsliceslice_hip_context.so"


def test_the_context_kernels_meet_their_bar_and_every_other_row_is_what_it_was():
    b = _build()
    rows = b.context_kernel_resources()
    own = [r for r in rows if r["tu"] == "ss_context.hip"]
    names = sorted(r["name"].split("(")[0] for r in own)
    assert names == ["ss::context_census_kernel", "ss::context_fill_kernel", "ss::context_ranges_kernel", "ss::context_select_kernel",
                     "void ss::prefix_kernel<unsigned long>"], names
    for r in own:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128, r
    census = [r for r in own if "context_census_kernel" in r["name"]][0]
    assert census.get("lds_bytes", 0) <= 1024, census
    # every row of the inverted library's record reappears unchanged, and no other record names a context kernel
    inverted = b.inverted_kernel_resources()
    assert [r for r in rows if r["tu"] != "ss_context.hip"] == inverted and len(rows) == len(inverted) + 5
    product = json.load(open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "kernel_resources.json")))
    for other in (product, b.matches_kernel_resources(), b.matches_batched_kernel_resources(), b.lines_kernel_resources(),
                  b.nocase_kernel_resources(), b.bounded_kernel_resources(), inverted):
        assert not [r for r in other if "context" in r["name"] or "context" in r["tu"]]


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_the_rule_reproduces_the_fixture():
    kat = json.load(open(os.path.join(GOLDEN, "context_kat.json")))
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    assert kat["grep_checked"] is True and "3.7" in kat["grep_version"] and kat["lines"] == len(all_lines(data, 10)) == 20854
    assert os.path.getsize(os.path.join(GOLDEN, "context_kat.json")) < os.path.getsize(os.path.join(GOLDEN, "nocase_kat.json"))
    # the table of the issue, README and DESIGN.md 5.12
    quoted = {("descriptor", "", False, 1, 2): (337, 1026, 174), ("the", "w", False, 0, 3): (4416, 9270, 927),
              ("intel", "i", False, 5, 0): (36, 178, 22), ("the", "w", True, 2, 2): (16438, 20600, 140),
              ("no such phrase in the manual", "", False, 3, 3): (0, 0, 0)}
    seen = {(r["needle"], r["how"], r["invert"], r["before"], r["after"]): (r["selected"], r["printed"], r["separators"]) for r in kat["rows"]}
    for key, figures in quoted.items():
        assert seen[key] == figures, key
    hows = {(r["how"], r["invert"]) for r in kat["rows"]}
    assert {("x", False), ("wi", False), ("i", True), ("w", True), ("", False), ("i", False)} <= hows
    assert any(r["before"] == r["after"] == 1 for r in kat["rows"])
    assert any(r["before"] == 0 and r["after"] > kat["lines"] for r in kat["rows"]) and any(r["after"] == 0 and r["before"] > kat["lines"] for r in kat["rows"])
    for r in kat["rows"]:
        sel = selected_numbers(data, r["needle"].encode(), 10, r["how"], r["invert"])
        numbers, kinds = context_rule(sel, kat["lines"], r["before"], r["after"])
        what = (r["needle"], r["how"], r["invert"], r["before"], r["after"])
        assert (len(sel), numbers.size, separators(numbers)) == (r["selected"], r["printed"], r["separators"]), what
        assert int(kinds.sum()) == r["selected"] and numbers[kinds == 1].tolist() == sel, what
        pairs = [list(p) for p in zip(numbers.tolist(), kinds.tolist())]
        assert pairs[:20] == r["first"] and pairs[-20:] == r["last"] and checksum(numbers, kinds) == r["sha256"], what


# ---- the range arithmetic, on the host ----------------------------------------------------------------------------------------
def test_the_range_arithmetic_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/context_ranges_check.cpp: N <= 6, every subset, b and a in {0, 1, 2, 5, 2^64 - 1}, against a brute-force union;
    entries 0 and above N; saturation; neighbours out of order.  A program of its own, compiled for the host and run as a child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "context_ranges_check.cpp")
    exe = str(tmp_path / "context_ranges_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 50000                  # (the sweep ran)
    header = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "context_ranges.hpp")).read()
    assert "__host__ __device__" in header and "hip_runtime" not in header
    assert '#include "context_ranges.hpp"' in open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "context_kernels.hpp")).read()


# ---- Python and the command-line tool -----------------------------------------------------------------------------------------
def test_the_methods_are_refused_outside_the_context_library():
    class Fake:
        _L = ss.lib()
        _h = None
    calls = (("find_lines_context", (b"abc",)), ("find_lines_context_into", (b"abc", None, None, None, None, 0)),
             ("lines_around", (b"abc", [1])), ("lines_around_into", (b"abc", [1], None, None, None, None, 0)))
    for build in (None, ss.lines_build, ss.bounded_build, ss.inverted_build):
        if build is not None:
            with build():
                Fake._L = ss.lib()
        for meth, args in calls:
            for kw in ({}, dict(before=2), dict(after=1, before=1)):
                with pytest.raises(ss.SlicesliceError, match="context_build") as e:
                    getattr(ss.DynamicHipSearcher, meth)(Fake(), *args, **kw)
                assert e.value.code == ss.SS_ERR_ARGUMENT
    # the signatures the issue gives, on both classes
    want = {"find_lines_context": "(self, haystack, before=0, after=0, delimiter=b'\\n', capacity=None, stream=None, ignore_case=False, "
                                  "whole_word=False, whole_line=False, invert=False)",
            "find_lines_context_into": "(self, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b'\\n', "
                                       "stream=None, ignore_case=False, whole_word=False, whole_line=False, invert=False)",
            "lines_around": "(self, haystack, numbers, before=0, after=0, delimiter=b'\\n', capacity=None, stream=None)",
            "lines_around_into": "(self, haystack, numbers, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b'\\n', "
                                 "stream=None)"}
    for meth, sig in want.items():
        for cls in (ss.DynamicHipSearcher, ss.MemchrHipSearcher):
            assert str(inspect.signature(getattr(cls, meth))) == sig, (cls, meth)
    assert str(inspect.signature(ss.lines_around)) == want["lines_around"].replace("(self, ", "(")
    assert "grep -A" in ss.context_build.__doc__ and not getattr(ss.lib(), "has_context", False)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="2\\^64 - 1"):
            ss.searcher._context_amount(bad, "before")


def test_grep_hip_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    usage = _grep()
    assert usage.returncode != 0 and "-A NUM" in usage.stderr and "--before-context" in usage.stderr and "--context" in usage.stderr
    assert "--invert-match" in usage.stderr and "--word-regexp" in usage.stderr and "--line-regexp" in usage.stderr
    for flag in (("-A", "2"), ("-B", "2"), ("-C", "2"), ("--context=2",), ("-A2",), ("--after-context", "2")):
        for out in ("--count", "--offsets", "--count-lines"):
            refused = _grep(*flag, out, "a", words)
            assert refused.returncode != 0 and "--lines" in refused.stderr and "context" in refused.stderr.lower(), (flag, out, refused)
        alone = _grep(*flag, "a", words)
        assert alone.returncode != 0 and "--lines" in alone.stderr, (flag, alone)
        both = _grep(*flag, "--lines", "--count-lines", "a", words)
        assert both.returncode != 0 and "--lines" in both.stderr
    several = _grep("-C", "1", "--count", "-e", "a", "-e", "b", words)
    assert several.returncode != 0 and "-C" in several.stderr and "-e" in several.stderr
    for bad in ("x", "-1", "1.5", "", "0x10"):
        refused = _grep("-C", bad, "--lines", "a", words)
        assert refused.returncode != 0 and "non-negative integer" in refused.stderr, (bad, refused)
    assert _grep("--context=two", "--lines", "a", words).returncode != 0
    exclusive = _grep("-C", "1", "-w", "-x", "--lines", "a", words)
    assert exclusive.returncode != 0 and "-w" in exclusive.stderr and "-x" in exclusive.stderr
    empty = _grep("-C", "1", "-x", "--lines", "", words)
    assert empty.returncode != 0 and "empty" in empty.stderr
    doc = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert "number-line" in doc and "LC_ALL=C grep -F -n" in doc and "find_lines_context" in doc
    for rel in ("tools/fuzz_context.py", "tools/context_bench.py", "tests/golden/make_context_golden.py", "profiles/context/README.md",
                "sliceslice-rs_amd/bindings/rust/hip_context.rs", "include/sliceslice_hip_context.h", "tests/native/context_ranges_check.cpp"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    assert "5.12" in open(os.path.join(ROOT, "DESIGN.md")).read() and "sliceslice_hip_context.h" in open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "libsliceslice_hip_context.so" in open(os.path.join(ROOT, "README.md")).read()
    assert "hip_context.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
