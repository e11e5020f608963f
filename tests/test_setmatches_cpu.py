"""CPU checks of the occurrence calls of a needle set (include/sliceslice_hip_setmatches.h): the header, the ctypes table and the
Rust module agree symbol by symbol; libsliceslice_hip_setmatches.so exports the needleset library's list plus four functions while
every other library exports what it did; the set's struct is shared through one internal header; the four occurrence kernels meet
their resource bar and every row of the needleset record reappears unchanged; needle identity in csrc/needleset_tables.hpp - the
ranks, the slots and set_each_at - passes a sweep against a brute-force memcmp loop in a stand-alone host program built with ASan
and UBSan; the new methods of ss.NeedleSet are refused outside setmatches_build(); tools/grep_hip.py documents --frequencies and
refuses what it should."""
import inspect
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
from test_needleset_cpu import NEEDLESET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
SETMATCHES = ["ss_needle_set_ranks", "ss_count_set_device", "ss_count_set_device_async", "ss_find_all_set_device"]


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_setmatches.h")
    assert sorted(c) == sorted(ss.searcher.SETMATCHES_ABI) == sorted(SETMATCHES)
    # (set, haystack, len, how, stream, ...): the count calls end in two pointers, find in two pointers, the capacity and the total
    assert c["ss_needle_set_ranks"] == ("i32", ["ptr", "ptr"])
    assert c["ss_count_set_device"] == c["ss_count_set_device_async"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "ptr", "ptr"])
    assert c["ss_find_all_set_device"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "ptr", "ptr", "u64", "ptr"])
    r, rust = rust_prototypes("hip_setmatches.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_setmatches.rs")).read()
    assert r == c, (r, c)
    assert "use crate::hip_needleset::{ss_needle_set, NeedleSet};" in rust and "pub fn as_raw" in \
        open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_needleset.rs")).read()
    for name, (res, args) in ss.searcher.SETMATCHES_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h",
              "sliceslice_hip_nocase.h"):
        assert not set(c) & set(header_prototypes(h)), h
    assert not set(c) & (set(header_prototypes("sliceslice_hip_needleset.h")) | set(BOUNDED) | set(INVERTED) | set(CONTEXT) | set(ANYOF))
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_setmatches.h")).read()
    assert '#include "sliceslice_hip_needleset.h"' in text and "#define SS_BOUND" not in text and "#define SS_SET" not in text
    assert "typedef struct" not in text                         # the set's type is the needleset header's


def test_the_header_states_the_rule_and_the_refusals():
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_setmatches.h")).read()
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).lower().split())
    for topic in ("Rank:", "sorted, deduplicated order", "compare as unsigned", "a proper prefix sorts before the longer needle",
                  "share a rank", "ranks ascend with their lengths", "Rule:", "what ss_count_device returns",
                  "ss_count_nocase_device / ss_count_bounded_device", "Occurrences overlap", "A needle longer than `len` gives 0",
                  "outside [0, len) are absent", "No delimiter exists", "sum of the counts", "ordered by offset, then by rank",
                  "Nothing is written at index `capacity` or beyond", "may each be NULL", "capacity == 0 means the total only",
                  "`distinct` entries, overwritten; may be NULL", "either may be NULL, not both", "0 or SS_BOUND_WORD",
                  "SS_BOUND_NOCASE is accepted only when it equals the set's fold", "Refused with SS_ERR_ARGUMENT",
                  "nothing written", "SS_BOUND_LINE, SS_CONTEXT_INVERT and unknown bits", "holds the empty needle",
                  "NULL haystack with len > 0", "another device", "a capturing stream, for the two calls that wait",
                  "can be captured into a hipGraph", "needs no scratch beyond them", "per-call free list", "return it on every way out",
                  "4,096 bins", "one 64-bit device-scope add per occurrence", "deterministic", "no sort", "DESIGN.md 5.15",
                  "Out of scope", "leftmost-longest", "batched, plan, sharded, service", "libsliceslice_hip_setmatches.so"):
        assert topic.lower() in flat, topic
    # the neighbours point here and keep the words that the earlier tests look for
    old = open(os.path.join(ROOT, "include", "sliceslice_hip_needleset.h")).read()
    scope = old[old.index("Out of scope"):]
    assert "occurrence (non-line) form" in scope and "sliceslice_hip_setmatches.h" in scope


def test_the_setmatches_library_exports_the_needleset_list_plus_four_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    needleset = product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT + ANYOF + NEEDLESET
    assert _exported(b.build_setmatches()) == sorted(needleset + SETMATCHES)
    assert _exported(b.build_needleset()) == sorted(needleset)
    assert _exported(b.build_anyof()) == sorted(product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT + ANYOF)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_matches()) == sorted(product + matches)
    assert os.path.basename(b.setmatches_library_path()) == "libsliceslice_hip_setmatches.so"


def test_the_sets_struct_is_shared_by_the_two_translation_units_through_one_internal_header():
    host = open(os.path.join(CSRC, "needleset_host.hpp")).read()
    assert "struct ss_needle_set {" in host
    for tu in ("ss_needleset.hip", "ss_setmatches.hip"):
        text = open(os.path.join(CSRC, tu)).read()
        assert '#include "needleset_host.hpp"' in text and "struct ss_needle_set {" not in text, tu


def test_the_occurrence_kernels_meet_their_bar_and_every_other_row_is_what_it_was():
    b = _build()
    rows = b.setmatches_kernel_resources()
    own = [r for r in rows if r["tu"] == "ss_setmatches.hip"]
    kernels = [r for r in own if "set_all_kernel" in r["name"]]
    names = sorted(r["name"].split("(")[0] for r in kernels)
    assert names == sorted("void ss::set_all_kernel<%d, %s>" % (mode, fold) for mode in (0, 1) for fold in ("false", "true")), names
    assert sorted(r["name"].split("(")[0] for r in own if r not in kernels) == ["void ss::prefix_kernel<unsigned long>"]
    for r in own:
        # no scratch memory, no spilled vector register, no AGPR, four waves per SIMD, bitmaps plus bins in at most 40 KiB of LDS
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["agprs"] == 0, r
        assert r["waves_per_simd"] >= 4 and r["lds_bytes"] <= 40960, r
    for r in kernels:
        assert r["lds_bytes"] >= 16384, r                        # (the two bitmaps are staged)
    # every row of the needleset library's record reappears unchanged, and no other record names an occurrence kernel
    needleset = b.needleset_kernel_resources()
    assert [r for r in rows if r["tu"] != "ss_setmatches.hip"] == needleset and len(rows) == len(needleset) + 5
    for other in (needleset, b.anyof_kernel_resources(), b.matches_kernel_resources()):
        assert not [r for r in other if "set_all" in r["name"] or "setmatches" in r["tu"]]
    text = open(os.path.join(CSRC, "setmatches_kernels.hpp")).read()
    for called in ('#include "needleset_kernels.hpp"', "set_valid_bits(", "set_lookup16(", "set_lookup16_b1(", "load_chunk<true>(", "set_each_at(",
                   "from_next_lane_or(", "__HIP_MEMORY_SCOPE_AGENT", "wave_exclusive_sum("):
        assert called in text, called
    assert "asm" not in text and "set_line_known" not in text and "line_tile_done" not in text
    host = open(os.path.join(CSRC, "ss_setmatches.hip")).read()
    for used in ("take_scratch(", "ScratchLease", "prefix_kernel<uint64_t>", "stream_is_capturing(", "hipMemsetAsync("):
        assert used in host, used


# ---- needle identity, on the host ---------------------------------------------------------------------------------------------------
def test_ranks_slots_and_set_each_at_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/setmatches_tables_check.cpp: rank_of, the ranks of the entries and of the short needles, the slots and
    set_each_at, position by position against a brute-force memcmp loop.  A program of its own, compiled for the host and run as a
    child; the needleset program still builds with -Wall -Werror from the same header."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "setmatches_tables_check.cpp")
    exe = str(tmp_path / "setmatches_tables_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 1000000                 # (the sweep ran)
    header = open(os.path.join(CSRC, "needleset_tables.hpp")).read()
    assert "__host__ __device__" in header and "hip_runtime" not in header and "#include <hip" not in header
    assert "SS_SET_HD void set_each_at(" in header and "kSetNoDelim" in header and "struct SetRanks" in header
    # additive: the entry and the view are what they were
    assert re.search(r"struct SetEntry \{\s*uint32_t off, len;[^}]*uint32_t word, mask;[^}]*\};", header)
    view = re.search(r"struct SetView \{(.*?)\};", header, flags=re.S).group(1)
    assert re.findall(r"\*?(\w+);", view) == ["b1", "bp", "bucket", "entry", "blob", "fold", "has1"]
    assert '#include "needleset_tables.hpp"' in open(os.path.join(CSRC, "needleset_host.hpp")).read()


# ---- Python and the command-line tool -------------------------------------------------------------------------------------------------
def test_the_new_methods_and_where_they_are_refused():
    want = {"ranks": "(self)",
            "count": "(self, haystack, whole_word=False, stream=None)",
            "count_total": "(self, haystack, whole_word=False, stream=None)",
            "count_async": "(self, haystack, d_counts, d_total, whole_word=False, stream=None)",
            "find_all": "(self, haystack, whole_word=False, capacity=None, stream=None)",
            "find_all_into": "(self, haystack, d_offsets, d_ranks, capacity, whole_word=False, stream=None)",
            # ... and the existing ones are what they were
            "__init__": "(self, needles, ignore_case=False)", "info": "(self)", "close": "(self)",
            "count_lines": "(self, haystack, delimiter=b'\\n', whole_word=False, whole_line=False, invert=False, stream=None)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(ss.NeedleSet, name))) == sig, name
    assert ss.setmatches_build is ss.searcher.setmatches_build and "word-frequency table" in ss.setmatches_build.__doc__
    assert not getattr(ss.lib(), "has_setmatches", False)
    for name in ("ranks", "count", "count_total", "count_async", "find_all", "find_all_into"):
        assert "setmatches_build" in ss.searcher._FEATURES["setmatches"][2] and name in ss.searcher._FEATURES["setmatches"][2], name
        assert '_feature_lib(self._L, "setmatches")' in inspect.getsource(getattr(ss.NeedleSet, name)), name


def test_grep_hip_frequencies_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    # refused before any library is loaded
    for args, word in ((("--frequencies", "-x", "-e", "a", words), "-x"), (("--frequencies", "-v", "-e", "a", words), "-v"),
                       (("--frequencies", "-A", "1", "-e", "a", words), "-A"), (("--frequencies", "-C2", "-e", "a", words), "-C"),
                       (("--frequencies", "--line-regexp", "-e", "a", words), "-x")):
        refused = _grep(*args)
        assert refused.returncode != 0 and word in refused.stderr and "occurrences" in refused.stderr, (args, refused)
    empty = _grep("--frequencies", "-e", "a", "-e", "", words)
    assert empty.returncode != 0 and "empty" in empty.stderr
    for args in (("--frequencies", words), ("--frequencies", "-e", "a"), ("--frequencies", "-e", "a", words, "extra"),
                 ("--frequencies", "--count", "-e", "a", words)):
        usage = _grep(*args)
        assert usage.returncode != 0 and "--frequencies [-i] [-w] (-e <pattern>)... [-f <patterns file>] <file>" in usage.stderr, (args, usage)
    # --one-pass --count stays refused
    refused = _grep("--one-pass", "--count", "-e", "a", "-e", "b", words)
    assert refused.returncode != 0 and "--one-pass" in refused.stderr
    doc = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert "--frequencies" in doc and "ss_count_set_device" in doc and "libsliceslice_hip_setmatches.so" in doc
    assert "byte for byte what --count -e ... prints" in doc
    for rel in ("sliceslice-rs_amd/bindings/rust/hip_setmatches.rs", "include/sliceslice_hip_setmatches.h",
                "tests/native/setmatches_tables_check.cpp", "tests/test_gpu_setmatches.py"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    assert "5.15" in open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "libsliceslice_hip_setmatches.so" in readme and "eleven" in readme
    assert "hip_setmatches.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
