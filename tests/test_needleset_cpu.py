"""CPU checks of the needle-set calls (include/sliceslice_hip_needleset.h): the header, the ctypes table and the Rust module agree
symbol by symbol; libsliceslice_hip_needleset.so exports the anyof library's list plus five functions while every other library
exports what it did; the six set kernels meet their resource bar and every
row of the anyof record reappears unchanged; the tables and the lookup of csrc/needleset_tables.hpp pass a sweep against a
brute-force memcmp loop in a stand-alone host program built with ASan and UBSan; the set is refused outside needleset_build();
tools/grep_hip.py documents --one-pass and refuses what it should."""
import inspect
import json
import os
import re
import shutil
import subprocess

import pytest

import sliceslice_rs_amd as ss
from test_anyof_cpu import ANYOF
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes
from test_bounded_cpu import BOUNDED, LINES, NOCASE, _grep
from test_context_cpu import CONTEXT
from test_inverted_cpu import INVERTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEEDLESET = ["ss_needle_set_new", "ss_needle_set_free", "ss_needle_set_info", "ss_count_lines_set_device", "ss_find_lines_set_device"]


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_needleset.h")
    assert sorted(c) == sorted(ss.searcher.NEEDLESET_ABI) == sorted(NEEDLESET)
    # the line calls are the anyof calls with the set in the place of (searchers, needles)
    anyof = header_prototypes("sliceslice_hip_anyof.h")
    assert c["ss_find_lines_set_device"][1] == ["ptr"] + anyof["ss_find_lines_anyof_device"][1][2:]
    assert c["ss_count_lines_set_device"][1] == ["ptr"] + anyof["ss_count_lines_anyof_device"][1][2:]
    assert c["ss_needle_set_new"] == ("i32", ["ptr", "ptr", "u32", "u32", "ptr"]) and c["ss_needle_set_free"] == ("void", ["ptr"])
    assert c["ss_needle_set_info"] == ("i32", ["ptr", "ptr"])
    r, rust = rust_prototypes("hip_needleset.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_needleset.rs")).read()
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.NEEDLESET_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h",
              "sliceslice_hip_nocase.h"):
        assert not set(c) & set(header_prototypes(h)), h
    assert not set(c) & (set(header_prototypes("sliceslice_hip_context.h")) | set(BOUNDED) | set(INVERTED) | set(anyof))
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_needleset.h")).read()
    assert '#include "sliceslice_hip_anyof.h"' in text and "#define SS_BOUND" not in text and "#define SS_CONTEXT" not in text
    assert "#define SS_ANYOF" not in text and int(re.search(r"#define SS_SET_NOCASE\s+(\d+)u\b", text).group(1)) == ss.SS_SET_NOCASE == 1
    assert "SS_SET_NOCASE: c_uint = 1;" in rust
    # the stats: eight 64-bit words under the same names in the header, the Python tuple and the Rust struct
    fields = re.findall(r"uint64_t\s+([a-z_]+);", re.search(r"typedef struct ss_needle_set_stats \{(.*?)\}", text, flags=re.S).group(1))
    assert tuple(fields) == ss.searcher.NEEDLESET_STATS and len(fields) == 8
    assert re.findall(r"pub ([a-z_]+): u64,", re.search(r"pub struct ss_needle_set_stats \{(.*?)\}", rust, flags=re.S).group(1)) == fields
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).lower().split())
    for topic in ("Rule:", "sliceslice_hip_anyof.h has the rule", "value for value and array for array", "Out of scope", "SS_SET_NOCASE",
                  "never folded", "SS_BOUND_NOCASE is accepted only when it equals the set's fold", "count == 0", "SS_ANYOF_MAX_NEEDLES",
                  "2^32 bytes", "capturing stream", "another device", "no async form", "ONE scan", "one LDS load", "masked dword compare",
                  "known to match", "No global atomic", "deterministic", "temporary buffer", "returned on every way out", "SS_ERR_NOMEM",
                  "empty needle", "libsliceslice_hip_needleset.so", "-m", "-o", "a `how` per needle", "regular expressions",
                  "multi-byte terminators", "occurrence (non-line) form", "batched, plan, sharded, service", "prefix of another", "DESIGN.md 5.14"):
        assert topic.lower() in flat, topic
    # the earlier headers point here and keep the words that the earlier tests look for
    for h in ("sliceslice_hip_anyof.h", "sliceslice_hip_context.h", "sliceslice_hip_inverted.h", "sliceslice_hip_bounded.h"):
        old = open(os.path.join(ROOT, "include", h)).read()
        scope = old[old.index("Out of scope"):]
        assert "sliceslice_hip_needleset.h" in scope and "-m" in scope, h
        assert h == "sliceslice_hip_anyof.h" or ("sliceslice_hip_anyof.h" in scope and "several needles" in scope), h


def test_the_needleset_library_exports_the_anyof_list_plus_five_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    anyof = product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT + ANYOF
    assert _exported(b.build_needleset()) == sorted(anyof + NEEDLESET)
    assert _exported(b.build_anyof()) == sorted(anyof)
    assert _exported(b.build_context()) == sorted(product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_lines()) == sorted(product + matches + LINES)
    assert os.path.basename(b.needleset_library_path()) == "libsliceslice_hip_needleset.so"


def test_the_set_kernels_meet_their_bar_and_every_other_row_is_what_it_was():
    b = _build()
    rows = b.needleset_kernel_resources()
    own = [r for r in rows if r["tu"] == "ss_needleset.hip"]
    names = sorted(r["name"].split("(")[0] for r in own)
    assert names == sorted("void ss::set_scan_kernel<%d, %s>" % (mode, fold) for mode in (0, 1, 2) for fold in ("false", "true")), names
    for r in own:
        # no scratch memory, no spilled vector register, four waves per SIMD, the two bitmaps in at most 32 KiB of LDS
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["agprs"] == 0, r
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128 and 16384 <= r["lds_bytes"] <= 32768, r
    # every row of the anyof library's record reappears unchanged, and no other record names a set kernel
    anyof = b.anyof_kernel_resources()
    assert [r for r in rows if r["tu"] != "ss_needleset.hip"] == anyof and len(rows) == len(anyof) + 6
    product = json.load(open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "kernel_resources.json")))
    for other in (product, b.matches_kernel_resources(), b.lines_kernel_resources(), b.nocase_kernel_resources(), b.bounded_kernel_resources(),
                  b.inverted_kernel_resources(), b.context_kernel_resources(), anyof):
        assert not [r for r in other if "set_scan" in r["name"] or "needleset" in r["tu"]]
    kernels = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "needleset_kernels.hpp")).read()
    assert "atomic" not in kernels.lower().replace("no global atomic", "")                       # no atomic of any kind
    for called in ("line_capture<U>(", "line_tile_done<U, MODE == kSetEmitInv>(", "load_chunk<true>(", '#include "needleset_launch.hpp"'):
        assert called in kernels, called
    for rewritten in ("line_wave_summary(", "line_wave_emit(", "line_piece("):
        assert "__forceinline__ " + rewritten not in kernels and " " + rewritten.rstrip("(") + "<" not in kernels.replace("line_tile_done<", "")
    host = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "ss_needleset.hip")).read()
    for launched in ("launch_lines_chunks(", "launch_lines_combine(", "launch_lines_total_inverted(", "ss_lines_around_device("):
        assert launched in host, launched


# ---- the tables, on the host --------------------------------------------------------------------------------------------------------
def test_the_tables_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/needleset_tables_check.cpp: sets over alphabets of 2 - 3 bytes with needles of 0 - 7 bytes, with and without the
    fold, and sets of 300 needles that share one two-byte key with lengths up to 2,000, on small haystacks, position by position
    against a brute-force memcmp loop under every `how`.  A program of its own, compiled for the host and run as a child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "needleset_tables_check.cpp")
    exe = str(tmp_path / "needleset_tables_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 1000000                 # (the sweep ran)
    header = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "needleset_tables.hpp")).read()
    assert "__host__ __device__" in header and "hip_runtime" not in header and "#include <hip" not in header
    assert '#include "needleset_tables.hpp"' in open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "needleset_launch.hpp")).read()
    kernels = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "needleset_kernels.hpp")).read()
    assert "set_match_at(" in kernels and "set_walk(" in kernels                  # the same lookup text runs on the device


# ---- Python and the command-line tool -------------------------------------------------------------------------------------------------
def test_the_set_is_refused_outside_the_needleset_library():
    for build in (None, ss.lines_build, ss.context_build, ss.anyof_build):
        with pytest.raises(ss.SlicesliceError, match="needleset_build") as e:
            if build is None:
                ss.NeedleSet([b"abc"])
            else:
                with build():
                    ss.NeedleSet([b"abc"], ignore_case=True)
        assert e.value.code == ss.SS_ERR_ARGUMENT
    want = {"__init__": "(self, needles, ignore_case=False)",
            "count_lines": "(self, haystack, delimiter=b'\\n', whole_word=False, whole_line=False, invert=False, stream=None)",
            "find_lines": "(self, haystack, before=0, after=0, delimiter=b'\\n', whole_word=False, whole_line=False, invert=False, "
                          "capacity=None, stream=None)",
            "find_lines_into": "(self, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b'\\n', "
                               "whole_word=False, whole_line=False, invert=False, stream=None)",
            "info": "(self)", "close": "(self)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(ss.NeedleSet, name))) == sig, name
    assert ss.NeedleSet is ss.searcher.NeedleSet and "grep -f FILE" in ss.needleset_build.__doc__ and not getattr(ss.lib(), "has_needleset", False)


def test_grep_hip_one_pass_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    # --one-pass goes with -e / -f and a line output only, and refuses before any library is loaded
    for args in (("--one-pass", "abc", words, "--count-lines"), ("--one-pass", "--count", "-e", "a", "-e", "b", words),
                 ("--one-pass", "-e", "a", words), ("--one-pass", "abc", words)):
        refused = _grep(*args)
        assert refused.returncode != 0 and "--one-pass" in refused.stderr and "-e / -f" in refused.stderr, (args, refused)
    for out in ("--count-lines", "--lines"):
        both = _grep("--one-pass", "-w", "-x", out, "-e", "a", "-e", "b", words)
        assert both.returncode != 0 and "-w" in both.stderr and "-x" in both.stderr
        empty = _grep("--one-pass", "-x", out, "-e", "a", "-e", "", words)
        assert empty.returncode != 0 and "empty" in empty.stderr
        usage = _grep("--one-pass", out, "-e", "a", "-e", "b")
        assert usage.returncode != 0 and "--count-lines | --lines" in usage.stderr and "-f <patterns file>" in usage.stderr
    refused = _grep("--one-pass", "-C", "2", "--count-lines", "-e", "a", "-e", "b", words)
    assert refused.returncode != 0 and "--lines" in refused.stderr and "context" in refused.stderr.lower()
    doc = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert "--one-pass" in doc and "ss_count_lines_set_device" in doc and "libsliceslice_hip_needleset.so" in doc and "byte for byte" in doc
    for rel in ("tools/fuzz_needleset.py", "tools/needleset_bench.py", "profiles/needleset/README.md",
                "sliceslice-rs_amd/bindings/rust/hip_needleset.rs", "include/sliceslice_hip_needleset.h", "tests/native/needleset_tables_check.cpp",
                "tests/test_gpu_needleset.py", "tests/test_gpu_zz_needleset_timing.py"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    assert "5.14" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "libsliceslice_hip_needleset.so" in open(os.path.join(ROOT, "README.md")).read()
    assert "hip_needleset.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
