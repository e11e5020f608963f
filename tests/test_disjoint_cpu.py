"""CPU checks of the non-overlapping calls (include/sliceslice_hip_disjoint.h): the header, the ctypes table and the Rust module agree
symbol by symbol; libsliceslice_hip_disjoint.so exports the setmatches library's list plus four functions while every other library
exports what it did; the new kernels use no private segment and every row
of the setmatches record reappears unchanged; the border function and the greedy walk of csrc/disjoint_host.hpp pass a sweep
against brute force in a stand-alone host program built with ASan and UBSan; tests/golden/disjoint_kat.json is what bytes.count and
re.finditer give; the new Python methods are refused outside disjoint_build(); tools/grep_hip.py documents -o and --replace and
refuses what it should."""
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
from test_anyof_cpu import ANYOF
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes
from test_bounded_cpu import BOUNDED, LINES, NOCASE, _grep
from test_context_cpu import CONTEXT
from test_inverted_cpu import INVERTED
from test_needleset_cpu import NEEDLESET
from test_setmatches_cpu import SETMATCHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
DISJOINT = ["ss_select_disjoint_device", "ss_count_disjoint_device", "ss_find_all_disjoint_device", "ss_replace_device"]
KERNELS = ["ss::disjoint_block_kernel", "ss::disjoint_chain_kernel", "ss::disjoint_emit_kernel", "ss::replace_kernel"]


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_disjoint.h")
    assert sorted(c) == sorted(ss.searcher.DISJOINT_ABI) == sorted(DISJOINT)
    assert c["ss_select_disjoint_device"] == ("i32", ["ptr", "ptr", "u64", "u64", "ptr", "ptr", "u64", "ptr"])
    # the models' argument lists: (searcher, haystack, len, how, stream, ...)
    assert c["ss_count_disjoint_device"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "ptr"])
    assert c["ss_find_all_disjoint_device"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "ptr", "u64", "ptr"])
    assert c["ss_replace_device"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "usize", "ptr", "ptr", "u64", "ptr", "ptr"])
    r, rust = rust_prototypes("hip_disjoint.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_disjoint.rs")).read()
    assert r == c, (r, c)
    assert "pub const SS_DISJOINT_BLOCK: u64 = 4096;" in rust
    for name, (res, args) in ss.searcher.DISJOINT_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h",
              "sliceslice_hip_nocase.h"):
        assert not set(c) & set(header_prototypes(h)), h
    assert not set(c) & (set(header_prototypes("sliceslice_hip_setmatches.h")) | set(header_prototypes("sliceslice_hip_needleset.h")) | set(BOUNDED) | set(INVERTED) | set(CONTEXT) | set(ANYOF))
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_disjoint.h")).read()
    assert '#include "sliceslice_hip_setmatches.h"' in text and "#define SS_BOUND" not in text and "typedef struct" not in text
    assert re.search(r"#define SS_DISJOINT_BLOCK\s+4096u", text) and ss.DISJOINT_BLOCK == ss.searcher.DISJOINT_BLOCK == 4096


def test_the_header_states_the_rule_and_the_refusals():
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_disjoint.h")).read()
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).lower().split())
    for topic in ("Rule:", "those that the model call for `how` keeps", "ss_find_all_device", "ss_find_all_nocase_device",
                  "ss_find_all_bounded_device", "The first occurrence is selected", "the first occurrence at or beyond p + n",
                  "The bounds test comes before the selection", "neither is selected nor blocks a later one", "GNU grep -o -b -w -F",
                  "4, 8, 11, 15", "re.finditer", "outside [0, len) are absent", "Everything is 64-bit", "Empty needle:",
                  "the model's len + 1 offsets", "the replace call refuses it", "names the device and scratch only", "strictly ascending",
                  "the caller's contract", "n >= 1 is any 64-bit length", "Nothing is written at index `capacity` or beyond",
                  "capacity == 0 or a NULL d_selected means count only", "count == 0 gives 0 with no launch",
                  "nothing faults and nothing is written outside the first min(total, capacity) entries", "unspecified",
                  "takes one length", "leftmost-longest", "Waits for the stream", "`replacement` is host memory", "replacement_len may be 0",
                  "*out_len = len + count * (replacement_len - n)", "If out_capacity < *out_len, nothing is written and the call returns SS_OK",
                  "bytes.replace(needle, replacement)", "nothing is written at *out_len or beyond", "Refused with SS_ERR_ARGUMENT",
                  "nothing written", "SS_BOUND_LINE, SS_CONTEXT_INVERT and unknown bits", "the empty needle with any `how` bit",
                  "a capturing stream", "d_selected == d_offsets", "an overflow of *out_len", "intersects the haystack's range",
                  "longest proper border", "the call IS the model call", "no temporary memory", "8 bytes per overlapping occurrence",
                  "ss_find_lines_context_device", "SS_ERR_NOMEM or SS_ERR_HIP", "returned inside the call", "run head", "at most j + n",
                  "No workgroup waits for another", "no global atomic", "deterministic", "exactly once", "DESIGN.md 5.16", "Out of scope",
                  "libsliceslice_hip_disjoint.so"):
        assert topic.lower() in flat, topic
    # the neighbours point here and keep the words that the earlier tests look for
    for name, kept in (("sliceslice_hip_matches.h", "keep an offset when it is at least n past the last one kept"),
                       ("sliceslice_hip_setmatches.h", "leftmost-longest / non-overlapping selection")):
        old = open(os.path.join(ROOT, "include", name)).read()
        assert kept in " ".join(re.sub(r"^ \*", "", old, flags=re.M).split()) and "sliceslice_hip_disjoint.h" in old, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.16" in design and "sliceslice_hip_disjoint.h" in design.split("5.16", 1)[1]


def test_the_disjoint_library_exports_the_setmatches_list_plus_four_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    setmatches = product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT + ANYOF + NEEDLESET + SETMATCHES
    assert _exported(b.build_disjoint()) == sorted(setmatches + DISJOINT)
    assert _exported(b.build_setmatches()) == sorted(setmatches)
    assert _exported(b.build_needleset()) == sorted(product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT + ANYOF + NEEDLESET)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_matches()) == sorted(product + matches)
    assert os.path.basename(b.disjoint_library_path()) == "libsliceslice_hip_disjoint.so"


def test_the_new_kernels_use_no_private_segment_and_every_other_row_is_what_it_was():
    b = _build()
    rows = b.disjoint_kernel_resources()
    own = [r for r in rows if r["tu"] == "ss_disjoint.hip"]
    names = sorted(r["name"].split("(")[0] for r in own)
    assert names == sorted(KERNELS + ["void ss::prefix_kernel<unsigned long>"]), names
    for r in own:
        # no scratch memory, no spilled register, no AGPR; the offsets of a block (32 KiB) and three 16-bit words per entry in LDS
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["agprs"] == 0, r
        assert r["lds_bytes"] <= 58 * 1024, r
    for r in own:
        if "block_kernel" in r["name"] or "emit_kernel" in r["name"]:
            assert r["lds_bytes"] >= 32768 and r["waves_per_simd"] >= 4, r         # (one workgroup of 1,024 lanes is four waves per SIMD)
    setmatches = b.setmatches_kernel_resources()
    assert [r for r in rows if r["tu"] != "ss_disjoint.hip"] == setmatches and len(rows) == len(setmatches) + 5
    for other in (setmatches, b.needleset_kernel_resources(), b.matches_kernel_resources()):
        assert not [r for r in other if "disjoint" in r["name"] or "replace_kernel" in r["name"] or "disjoint" in r["tu"]]
    text = open(os.path.join(CSRC, "disjoint_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    # no waiting between workgroups, no global atomic: the one atomic is the LDS minimum of the first head; loads of 16 bytes per lane
    assert "asm" not in code and "while (atomic" not in code and "__threadfence" not in code and "volatile" not in code
    assert code.count("atomic") == 1 and "atomicMin(s_head" in code and "__syncthreads_or(" in code
    assert "const uint4 v = *reinterpret_cast<const uint4 *>(a.base + q0)" in code and "SS_CONTEXT_PART_BYTES" in code
    host = open(os.path.join(CSRC, "ss_disjoint.hip")).read()
    for used in ("take_scratch(", "ScratchLease", "prefix_kernel<uint64_t>", "stream_is_capturing(", "longest_proper_border(", "hipFree(",
                 "ss_find_all_bounded_device(", "ss_find_all_nocase_device(", "ss_find_all_device(", "replaced_length("):
        assert used in host, used
    assert "SS_API" not in open(os.path.join(CSRC, "disjoint_host.hpp")).read()


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------
def test_the_border_and_the_greedy_walk_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/disjoint_host_check.cpp: longest_proper_border against the quadratic definition for every needle over {a, b} up
    to length 10, select_disjoint_host against the obvious loop for every offset subset of a 14-byte window.  A program of its own,
    compiled for the host and run as a child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "disjoint_host_check.cpp")
    exe = str(tmp_path / "disjoint_host_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 1000000                 # (the sweep ran)
    header = open(os.path.join(CSRC, "disjoint_host.hpp")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header and "__device__" not in header


def holds(case, offsets):
    """the fixture's list is `offsets`: given in full, or - a long list - by its SHA-256 as little-endian 64-bit words and its ends"""
    offsets = [int(o) for o in offsets]
    if "offsets" in case:
        return offsets == case["offsets"]
    digest = hashlib.sha256(np.asarray(offsets, dtype="<u8").tobytes()).hexdigest()
    return digest == case["offsets_sha256"] and offsets[:16] == case["first"] and offsets[-16:] == case["last"] and len(offsets) == case["count"]


def test_the_fixture_is_what_python_counts():
    kat = json.load(open(os.path.join(GOLDEN, "disjoint_kat.json")))
    data = open(os.path.join(GOLDEN, kat["file"]), "rb").read()
    assert kat["bytes"] == len(data) == 857425 and "3.7" in kat["grep"]
    by_name = {c["name"]: c for c in kat["cases"]}
    assert sorted(by_name) == ["blank_line", "dashes", "ee", "intel_i", "the", "the_w", "two_spaces", "zeros"]
    table = {"two_spaces": (b"  ", 125181, 68060), "blank_line": (b"\n\n", 5177, 4479), "zeros": (b"000", 298, 185), "dashes": (b"--", 31, 29)}
    for name, (needle, overlapping, count) in table.items():
        case = by_name[name]
        assert (case["needle"].encode(), case["overlapping"], case["count"]) == (needle, overlapping, count), name
    word = rb"[0-9A-Za-z_]"
    for case in kat["cases"]:
        needle, flags = case["needle"].encode(), case["flags"]
        hay = data.lower() if "-i" in flags else data
        pat = re.escape(needle)
        if "-w" in flags:
            pat = rb"(?<!" + word + rb")" + pat + rb"(?!" + word + rb")"
        else:
            assert case["count"] == hay.count(needle), case["name"]
            assert case["overlapping"] == len(re.findall(rb"(?=" + re.escape(needle) + rb")", hay)), case["name"]
        want = [m.start() for m in re.finditer(pat, hay)]
        assert holds(case, want) and case["count"] == len(want), case["name"]
        assert not holds(case, want[:-1] + [want[-1] + 1]) and ("offsets" in case) == (case["count"] <= 512), case["name"]
    assert os.path.getsize(os.path.join(GOLDEN, "disjoint_kat.json")) < 16384


# ---- Python and the command-line tool -------------------------------------------------------------------------------------------------
def test_the_new_methods_and_where_they_are_refused():
    want = {"count_disjoint": "(self, haystack, stream=None, ignore_case=False, whole_word=False)",
            "find_all_disjoint": "(self, haystack, capacity=None, stream=None, ignore_case=False, whole_word=False)",
            "find_all_disjoint_into": "(self, haystack, d_offsets, stream=None, ignore_case=False, whole_word=False)",
            "replace": "(self, haystack, replacement, stream=None, ignore_case=False, whole_word=False)",
            # ... and the existing ones are what they were
            "count": "(self, haystack, stream=None, ignore_case=False, whole_word=False)",
            "find_all": "(self, haystack, capacity=None, stream=None, ignore_case=False, whole_word=False)",
            "find_all_into": "(self, haystack, d_offsets, stream=None, ignore_case=False, whole_word=False)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(ss.DynamicHipSearcher, name))) == sig, name
    assert str(inspect.signature(ss.select_disjoint)) == "(offsets, n, capacity=None, stream=None)"
    assert str(inspect.signature(ss.select_disjoint_into)) == "(offsets, n, d_out, stream=None)"
    assert ss.disjoint_build is ss.searcher.disjoint_build and "bytes.replace" in ss.disjoint_build.__doc__
    assert not getattr(ss.lib(), "has_disjoint", False)
    message = ss.searcher._FEATURES["disjoint"][2]
    for name in ("count_disjoint", "find_all_disjoint", "find_all_disjoint_into", "replace"):
        assert "disjoint_build" in message and name in message, name
        assert '_feature_lib(self._L, "disjoint")' in inspect.getsource(getattr(ss.DynamicHipSearcher, name)), name
    for fn in (ss.select_disjoint, ss.select_disjoint_into):
        assert fn.__name__ in message and '_feature_lib(lib(), "disjoint")' in inspect.getsource(fn)
    # refused by the product library before anything touches a device: a searcher that belongs to the product (no handle is made:
    # the refusal comes before the handle is looked at)
    s = ss.DynamicHipSearcher.__new__(ss.DynamicHipSearcher)
    s._L, s._h = ss.lib(), None
    for call in (lambda: s.count_disjoint((0, 0)), lambda: s.find_all_disjoint((0, 0)), lambda: s.replace((0, 0), b"x"),
                 lambda: ss.select_disjoint([1, 2], 2), lambda: ss.select_disjoint_into([1, 2], 2, None)):
        with pytest.raises(ss.SlicesliceError, match=r"ss\.disjoint_build\(\)") as e:
            call()
        assert e.value.code == ss.SS_ERR_ARGUMENT


def test_grep_hip_only_matching_and_replace_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    # refused before any library is loaded: -o and --replace know no lines
    for args, word in ((("-o", "--count", "-x", "a", words), "-x"), (("-o", "--count", "-v", "a", words), "-v"),
                       (("-o", "--offsets", "-A", "1", "a", words), "-A"), (("--only-matching", "--lines", "a", words), "--lines"),
                       (("--replace", "b", "-x", "a", words), "-x"), (("--replace", "b", "-v", "a", words), "-v"),
                       (("--replace", "b", "-C2", "a", words), "-C"), (("--replace", "b", "--count", "a", words), "--count"),
                       (("-o", "--frequencies", "-e", "a", words), "--frequencies")):
        refused = _grep(*args)
        assert refused.returncode != 0 and word in refused.stderr and "non-overlapping" in refused.stderr, (args, refused)
    for args in (("-o", "a", words), ("-o", "--count", "a"), ("--replace", "b", "a"), ("--replace",)):
        usage = _grep(*args)
        assert usage.returncode != 0 and "-o (--count | --offsets) [-i] [-w] <needle> <file>" in usage.stderr and \
            "--replace <text> [-i] [-w] <needle> <file>" in usage.stderr, (args, usage)
    empty = _grep("--replace", "b", "", words)
    assert empty.returncode != 0 and "empty" in empty.stderr
    doc = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    for said in ("--only-matching", "--replace", "ss_find_all_disjoint_device", "ss_replace_device", "libsliceslice_hip_disjoint.so",
                 "byte for byte what grep -o -b -F prints"):
        assert said in doc, said
    for rel in ("sliceslice-rs_amd/bindings/rust/hip_disjoint.rs", "include/sliceslice_hip_disjoint.h", "tests/native/disjoint_host_check.cpp",
                "tests/test_gpu_disjoint.py", "tools/fuzz_disjoint.py", "tools/disjoint_bench.py"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "libsliceslice_hip_disjoint.so" in readme and "twelve" in readme
    assert "hip_disjoint.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hip_disjoint.rs" in open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "build.rs")).read()
