"""CPU checks of the leftmost-longest calls (include/sliceslice_hip_leftmost.h): the header, the ctypes table and the Rust module agree
symbol by symbol; libsliceslice_hip_leftmost.so exports the output library's list plus five functions; both build tables are what
they were and the fourteenth library stands beside the thirteenth; the new kernels use no private segment, no spill, no AGPR and at
most 48 KiB of LDS, and every row of the output record reappears unchanged; the arithmetic of csrc/leftmost_host.hpp passes a sweep
against brute force in a stand-alone host program built with ASan and UBSan; tests/golden/leftmost_kat.json is what the rule
restated in Python gives; the new Python calls are refused outside leftmost_build()."""
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
LEFTMOST = ["ss_select_leftmost_device", "ss_count_leftmost_set_device", "ss_find_all_leftmost_set_device", "ss_replace_set_device",
            "ss_needle_set_lengths"]
KERNELS = ["ss::leftmost_longest_kernel", "ss::leftmost_longest_final_kernel", "ss::leftmost_block_kernel", "ss::leftmost_chain_kernel",
           "ss::leftmost_emit_kernel", "ss::leftmost_deltas_kernel", "ss::leftmost_starts_kernel", "ss::leftmost_copy_kernel"]


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_leftmost.h")
    assert sorted(c) == sorted(ss.searcher.LEFTMOST_ABI) == sorted(LEFTMOST)
    assert c["ss_select_leftmost_device"] == ("i32", ["ptr", "ptr", "ptr", "u64", "ptr", "ptr", "ptr", "u64", "ptr"])
    assert c["ss_count_leftmost_set_device"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "ptr"])
    # the set's own find call, argument for argument
    assert c["ss_find_all_leftmost_set_device"] == header_prototypes("sliceslice_hip_setmatches.h")["ss_find_all_set_device"]
    assert c["ss_replace_set_device"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "ptr", "u32", "ptr", "ptr", "u64", "ptr", "ptr"])
    assert c["ss_needle_set_lengths"] == ("i32", ["ptr", "ptr"])
    r, rust = rust_prototypes("hip_leftmost.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_leftmost.rs")).read()
    assert r == c, (r, c)
    assert "pub const SS_LEFTMOST_BLOCK: u64 = 4096;" in rust
    for name, (res, args) in ss.searcher.LEFTMOST_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_leftmost.h":
            assert not set(c) & set(header_prototypes(h)), h
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_leftmost.h")).read()
    assert '#include "sliceslice_hip_output.h"' in text and "typedef struct" not in text
    assert re.search(r"#define SS_LEFTMOST_BLOCK\s+4096u", text) and ss.LEFTMOST_BLOCK == ss.searcher.LEFTMOST_BLOCK == 4096


def test_the_header_states_the_rule_and_the_refusals():
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_leftmost.h")).read()
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).lower().split())
    for topic in ("Rule:", "those ss_find_all_set_device lists for the same set and `how`", "0 or SS_BOUND_WORD",
                  "SS_BOUND_NOCASE is accepted only when it equals the set's fold", "the one with the greatest rank is the candidate",
                  "ranks ascend with length there", "The first candidate is selected",
                  "the next selected one is the first candidate at or beyond p + L", "The word test comes before the selection",
                  "neither is selected nor blocks", "a shorter needle at the same offset that is a whole word then is the candidate",
                  "Bytes outside [0, len) are absent", "Everything is 64-bit", "A set that holds the empty needle is refused",
                  "`set` names the device and its scratch only", "ascend and may repeat", "each >= 1", "ascend within a run of equal offsets",
                  "the caller's contract", "Either array may be NULL", "capacity == 0 means count only",
                  "Nothing is written at index `capacity` or beyond", "count == 0 gives 0 with no launch", "nothing faults",
                  "A zero length lies in device memory and is NOT detected", "Waits for the stream",
                  "belongs to needle k as given to ss_needle_set_new", "must equal the set's `needles` stat",
                  "Needles that share a rank must carry equal replacements", "computed with overflow checks",
                  "If out_capacity < *out_len, nothing is written and the call returns SS_OK", "nothing is written at *out_len or beyond",
                  "d_out may have any alignment and must not intersect the haystack", "`distinct` entries, host memory",
                  "Refused with SS_ERR_ARGUMENT", "nothing written", "SS_BOUND_LINE, SS_CONTEXT_INVERT and unknown bits",
                  "a set made on another device", "a capturing stream", "d_selected == d_offsets", "count >= 2^48",
                  "a NULL replacement with a length", "intersects the haystack's range", "an overflow of *out_len", "SS_ERR_NOMEM or SS_ERR_HIP",
                  "temporary memory is returned on every way out", "12 bytes per pair", "another 8 bytes per entry", "10.8 GB",
                  "per-rank table uploaded once per call", "SS_LEFTMOST_BLOCK entries staged in LDS", "pointer doubling",
                  "one-workgroup chain pass", "16-byte aligned address at or below d_out", "ONE 16-byte store", "stored exactly once",
                  "no load touches a 16-byte block that holds no byte of the view or of the (padded) replacement blob",
                  "no workgroup waits for another", "no global atomic", "depends on the input alone", "DESIGN.md 5.18", "Out of scope",
                  "a scan that emits only the longest pair per offset", "a host-side proof that a set cannot overlap itself",
                  "libsliceslice_hip_leftmost.so"):
        assert topic.lower() in flat, topic
    # the neighbours point here and keep the words that the earlier tests look for
    for name, kept in (("sliceslice_hip_setmatches.h", "leftmost-longest / non-overlapping selection (it follows on the host from the ordered pairs)"),
                       ("sliceslice_hip_disjoint.h", "Out of scope: leftmost-longest selection over a needle set's pairs")):
        old = open(os.path.join(ROOT, "include", name)).read()
        assert kept in " ".join(re.sub(r"^ \*", "", old, flags=re.M).split()) and "sliceslice_hip_leftmost.h" in old, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.18" in design and "sliceslice_hip_leftmost.h" in design.split("5.18", 1)[1]
    section = design.split("### 5.18", 1)[1].split("\n## ", 1)[0]
    for said in ("inside the staging", "sufficient form", "5,000", "48 KiB"):      # the choices the issue asks to be written down
        assert said in section, said


# ---- the build ----------------------------------------------------------------------------------------------------------------------
def test_both_tables_are_what_they_were_and_the_fourteenth_library_stands_beside_the_thirteenth():
    b = _build()
    assert list(b.LIBRARIES) == ["service", "matches", "matches_batched", "lines", "nocase", "bounded", "inverted", "context", "anyof", "needleset",
                                 "setmatches", "disjoint"]
    assert list(b._LATER_LIBRARIES) == ["output", "leftmost"]
    assert b._lib("output")["parent"] == "disjoint" and b._lib("output")["sources"] == ["ss_output.hip"]
    entry = b._lib("leftmost")
    assert entry["parent"] == "output" and entry["sources"] == ["ss_leftmost.hip"] and "leftmost" not in b.LIBRARIES
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_leftmost.so" == os.path.basename(b.leftmost_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_leftmost.json" == os.path.basename(b.leftmost_resources_path())
    assert "sliceslice-rs_amd/csrc/kernel_resources_leftmost.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("leftmost") == b._all_sources("output") + ["ss_leftmost.hip"] and b.library_path_of("leftmost") == entry["so"]
    assert callable(b.build_leftmost) and callable(b.leftmost_kernel_resources)
    for h in ("leftmost_kernels.hpp", "leftmost_launch.hpp", "leftmost_host.hpp", os.path.join("..", "..", "include", "sliceslice_hip_leftmost.h")):
        assert h in b._HEADERS and os.path.exists(os.path.join(CSRC, h)), h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index('b.build_library("output", force=True, verbose=True)') < \
        entry_point.index('b.build_library("leftmost", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["leftmost"][0] is ss.searcher.LEFTMOST_ABI and ss.searcher._FEATURES["leftmost"][1] == "ss_select_leftmost_device"
    product = ss.lib()
    assert not getattr(product, "has_leftmost")
    with ss.leftmost_build() as L:
        assert ss.lib() is L and L.has_leftmost and L.has_output and L.has_disjoint and L.has_setmatches and ss.searcher._feature_lib(L, "leftmost") is L
    assert ss.lib() is product
    with ss.output_build() as L:
        assert not L.has_leftmost
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "libsliceslice_hip_leftmost.so" in readme and "fourteenth" in readme and "thirteenth" in readme and "twelve" in readme
    assert "hip_leftmost.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hip_leftmost.rs" in open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "build.rs")).read()


def test_the_leftmost_library_exports_the_output_list_plus_five():
    b = _build()
    output = _exported(b.build_output())
    assert _exported(b.build_leftmost()) == sorted(output + LEFTMOST)
    assert not set(LEFTMOST) & set(output) and not set(LEFTMOST) & set(_exported(ss.build()))


def test_the_new_kernels_use_no_private_segment_and_every_other_row_is_what_it_was():
    b = _build()
    rows = b.leftmost_kernel_resources()
    own = [r for r in rows if r["tu"] == "ss_leftmost.hip"]
    names = sorted(r["name"].split("(")[0] for r in own)
    assert names == sorted(KERNELS + ["void ss::prefix_kernel<unsigned long>"]), names
    for r in own:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["agprs"] == 0, r
        assert r["lds_bytes"] <= 48 * 1024, r
    copy = [r for r in own if "leftmost_copy_kernel" in r["name"]][0]
    assert copy["vgprs"] <= 128 and copy["waves_per_simd"] >= 4 and copy["lds_bytes"] <= 1024, copy
    for name in ("leftmost_block_kernel", "leftmost_emit_kernel"):              # the staging fills the limit and no more
        assert [r for r in own if name in r["name"]][0]["lds_bytes"] == 48 * 1024, name
    output = b.output_kernel_resources()
    assert [r for r in rows if r["tu"] != "ss_leftmost.hip"] == output and len(rows) == len(output) + 9
    assert not [r for r in output if "leftmost" in r["name"] or "leftmost" in r["tu"]]
    text = open(os.path.join(CSRC, "leftmost_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    # no waiting between workgroups, no global atomic (the one atomic is the LDS minimum of the first head), no inline assembly
    assert "asm" not in code and "__threadfence" not in code and "volatile" not in code
    assert code.count("atomic") == 1 and "atomicMin(s_head, first)" in code
    assert "*reinterpret_cast<uint4 *>(a.out_base + u)" in code and "lm_u32x4_unaligned" in code and "SS_OUTPUT_CHUNK" in code
    assert '#include "prefix_kernel.hpp"' in text and "disjoint_kernels.hpp" not in code
    host = open(os.path.join(CSRC, "ss_leftmost.hip")).read()
    for used in ("take_scratch(", "ScratchLease", "prefix_kernel<uint64_t>", "stream_is_capturing(", "hipFree(", "ss_count_set_device(",
                 "ss_find_all_set_device(", "taken * 12", "kLeftmostBlobPad"):
        assert used in host, used
    assert "SS_API" not in open(os.path.join(CSRC, "leftmost_host.hpp")).read()


# ---- the host arithmetic --------------------------------------------------------------------------------------------------------------
def test_the_selection_the_rank_table_the_length_and_the_starts_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/leftmost_host_check.cpp: select_leftmost_host against a byte-wise walk for every text over {a, b} up to length 10
    and three needle sets, at every capacity; rank_replacements with equal and conflicting duplicates; replaced_set_length at the
    edges of 64 bits; replaced_starts_host against a loop that writes the substituted text.  A program of its own, compiled for the
    host and run as a child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "leftmost_host_check.cpp")
    exe = str(tmp_path / "leftmost_host_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 500000                  # (the sweep ran)
    header = open(os.path.join(CSRC, "leftmost_host.hpp")).read()
    assert "hip_runtime" not in header and "#include <hip" not in header and "__device__" not in header


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_restated_rule_gives():
    sys.path.insert(0, GOLDEN)
    try:
        import make_leftmost_golden as m
    finally:
        sys.path.remove(GOLDEN)
    kat = json.load(open(os.path.join(GOLDEN, "leftmost_kat.json")))
    data = open(os.path.join(GOLDEN, kat["file"]), "rb").read()
    assert kat["grep_checked"] and "3.7" in kat["grep_version"]
    assert [[n.encode("latin-1") for n in s] for s in kat["sets"]] == m.SETS and len(m.SETS) >= 6
    assert m.SETS[0] == [b"the", b"then", b"there", b"he", b"here"] and m.SETS[1] == [b"  ", b" "] and m.SETS[2] == [b"386", b"80386", b"8038", b"03"]
    assert len(kat["rows"]) == 4 * len(m.SETS)
    assert [(r["set"], r["ignore_case"], r["whole_word"]) for r in kat["rows"]] == \
        [(s, i, w) for s in range(len(m.SETS)) for i in (False, True) for w in (False, True)]
    for row in kat["rows"]:
        needles = m.SETS[row["set"]]
        pairs = m.rule(data, needles, row["ignore_case"], row["whole_word"])
        assert len(pairs) == row["count"] and m.list_hash(pairs) == row["sha256"], row
        assert [list(x) for x in pairs[:8]] == row["first"] and [list(x) for x in pairs[-8:]] == row["last"], row
    rows = {(r["set"], r["ignore_case"], r["whole_word"]): r["count"] for r in kat["rows"]}
    # the counts that three statements of the rule agreed on before the library was written
    assert [rows[0, i, w] for i, w in ((False, False), (True, False), (False, True), (True, True))] == [9424, 9726, 6623, 8134]
    assert (rows[1, False, False], rows[1, False, True], rows[2, False, False], rows[2, False, True]) == (167263, 67929, 519, 492)
    assert m.rule_regex(data[:60000], m.SETS[0], True, True) == m.rule(data[:60000], m.SETS[0], True, True)
    assert len(kat["replace"]) == 4 == len(m.REPLACE_ROWS)
    kinds = set()
    for row, (si, ignore_case, whole_word, reps) in zip(kat["replace"], m.REPLACE_ROWS):
        text = m.substitute(data, m.SETS[si], reps, ignore_case, whole_word)
        assert (row["set"], row["ignore_case"], row["whole_word"]) == (si, ignore_case, whole_word)
        assert len(text) == row["length"] and hashlib.sha256(text).hexdigest() == row["sha256"], row
        for n, r in zip(m.SETS[si], reps):
            kinds.add("empty" if not r else "shorter" if len(r) < len(n) else "equal" if len(r) == len(n) else "longer")
    assert kinds == {"empty", "shorter", "equal", "longer"}
    # the rule's corners, by hand
    assert m.rule(b"then there here", m.SETS[0]) == [(0, 1), (5, 2), (11, 4)]
    assert m.rule(b"aaaaa", [b"aa", b"a"]) == [(0, 0), (2, 0), (4, 1)]
    assert m.rule(b"int inter", [b"in", b"int", b"inter"], whole_word=True) == [(0, 1), (4, 2)]
    assert m.rule(b"inter-", [b"in", b"int", b"inter-x", b"inter"], whole_word=True) == [(0, 3)]
    assert m.rule(b"The THE", [b"the", b"THE"], ignore_case=True) == [(0, 0), (4, 0)]
    assert m.substitute(b"then there", m.SETS[0], [b"1", b"22", b"", b"4", b"5"]) == b"22 "
    assert os.path.getsize(os.path.join(GOLDEN, "leftmost_kat.json")) < 32768


# ---- Python -----------------------------------------------------------------------------------------------------------------------
def test_the_new_calls_and_where_they_are_refused():
    assert str(inspect.signature(ss.NeedleSet.count_leftmost)) == "(self, haystack, whole_word=False, stream=None)"
    assert str(inspect.signature(ss.NeedleSet.find_all_leftmost)) == "(self, haystack, whole_word=False, capacity=None, stream=None)"
    assert str(inspect.signature(ss.NeedleSet.find_all_leftmost_into)) == "(self, haystack, d_offsets, d_ranks, capacity, whole_word=False, stream=None)"
    assert str(inspect.signature(ss.NeedleSet.replace)) == "(self, haystack, replacements, whole_word=False, stream=None)"
    assert str(inspect.signature(ss.NeedleSet.lengths)) == "(self)"
    assert str(inspect.signature(ss.select_leftmost)) == "(offsets, lengths, capacity=None, stream=None)"
    assert str(inspect.signature(ss.select_leftmost_into)) == "(offsets, lengths, d_selected, d_which, capacity=None, stream=None)"
    # ... and the calls they stand beside are what they were
    assert str(inspect.signature(ss.NeedleSet.find_all)) == "(self, haystack, whole_word=False, capacity=None, stream=None)"
    assert str(inspect.signature(ss.DynamicHipSearcher.replace)) == "(self, haystack, replacement, stream=None, ignore_case=False, whole_word=False)"
    assert ss.leftmost_build is ss.searcher.leftmost_build and "grep -o -F -f FILE" in ss.leftmost_build.__doc__
    assert not getattr(ss.lib(), "has_leftmost", False)
    message = ss.searcher._FEATURES["leftmost"][2]
    for name in ("count_leftmost", "find_all_leftmost", "find_all_leftmost_into", "replace", "lengths", "select_leftmost", "select_leftmost_into"):
        assert "ss.leftmost_build()" in message and name in message, name
    for fn in (ss.NeedleSet.count_leftmost, ss.NeedleSet.find_all_leftmost_into, ss.NeedleSet.replace, ss.NeedleSet.lengths):
        assert '_feature_lib(self._L, "leftmost")' in inspect.getsource(fn)
    # refused by the product library - and by the output library - before anything touches a device
    with ss.output_build() as output_library:
        pass
    assert output_library is not ss.lib() and not output_library.has_leftmost
    for L in (ss.lib(), output_library):
        needles = ss.NeedleSet.__new__(ss.NeedleSet)
        needles._L, needles._h, needles._count = L, None, 1
        for call in (lambda: needles.count_leftmost((0, 0)), lambda: needles.find_all_leftmost((0, 0)),
                     lambda: needles.find_all_leftmost_into((0, 0), None, None, 0), lambda: needles.replace((0, 0), [b"x"]),
                     lambda: needles.lengths(), lambda: ss.select_leftmost([1], [1]), lambda: ss.select_leftmost_into([1], [1], None, None)):
            with pytest.raises(ss.SlicesliceError, match=r"ss\.leftmost_build\(\)") as e:
                call()
            assert e.value.code == ss.SS_ERR_ARGUMENT
    for rel in ("sliceslice-rs_amd/bindings/rust/hip_leftmost.rs", "include/sliceslice_hip_leftmost.h", "tests/native/leftmost_host_check.cpp",
                "tests/test_gpu_leftmost.py", "tests/golden/make_leftmost_golden.py", "tests/golden/leftmost_kat.json",
                "tests/test_gpu_zz_leftmost_timing.py", "tools/fuzz_leftmost.py", "tools/leftmost_bench.py", "profiles/leftmost/README.md",
                "profiles/leftmost/timing_test_spread.jsonl", "profiles/leftmost/leftmost_bench_1gib.jsonl"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel


def test_grep_hip_set_forms_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    tool = os.path.join(ROOT, "tools", "grep_hip.py")

    def grep(*args):
        return subprocess.run([sys.executable, tool] + list(args), capture_output=True, text=True, timeout=300)

    # refused before any library is loaded: the selection knows no lines
    for args, word in ((("-o", "--count", "-x", "-e", "a", words), "-x"), (("-o", "--count", "-v", "-e", "a", words), "-v"),
                       (("-o", "--offsets", "-A", "1", "-e", "a", words), "-A"), (("-o", "--lines", "-e", "a", words), "--lines"),
                       (("-o", "--count", "--one-pass", "-e", "a", words), "--one-pass"), (("--replace-map", words, "-x", words), "-x"),
                       (("--replace-map", words, "--count", words), "--count"), (("--replace-map", words, "-e", "a", words), "-e / -f"),
                       (("--replace-map", words, "--replace", "b", "a", words), "--replace")):
        refused = grep(*args)
        assert refused.returncode != 0 and word in refused.stderr and "leftmost-longest" in refused.stderr and "Traceback" not in refused.stderr, (args, refused)
    for args in (("-o", "-e", "a", words), ("-o", "--count", "-e", "a"), ("-o", "--count", "--offsets", "-e", "a", words), ("--replace-map",),
                 ("--replace-map", words)):
        usage = grep(*args)
        assert usage.returncode != 0 and "-o (--count | --offsets) [-i] [-w] (-e <needle>)... [-f <needles file>] <file>" in usage.stderr and \
            "--replace-map <map file> [-i] [-w] <file>" in usage.stderr, (args, usage)
    empty = grep("-o", "--count", "-e", "", "-e", "a", words)
    assert empty.returncode != 0 and "empty needle" in empty.stderr
    no_tab = grep("--replace-map", words, words)
    assert no_tab.returncode != 0 and "one TAB" in no_tab.stderr
    doc = open(tool).read()
    for said in ("--replace-map", "LEFTMOST-LONGEST", "ss_find_all_leftmost_set_device", "ss_replace_set_device", "libsliceslice_hip_leftmost.so",
                 "needle<TAB>text", "byte for byte what LC_ALL=C grep -o -b -F prints"):
        assert said in doc, said


def test_the_recorded_fuzz_run_found_no_mismatch_and_the_timing_bounds_are_the_recorded_runs():
    fuzz = json.load(open(os.path.join(ROOT, "profiles", "leftmost", "fuzz_leftmost_seed1_45s.json")))
    assert (fuzz["fuzz"], fuzz["seed"], fuzz["seconds"], fuzz["mismatches"]) == ("leftmost", 1, 45.0, 0) and fuzz["calls"] > 10000
    assert set(fuzz["by_how"]) == {"--", "-w", "i-", "iw"}
    rows = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "leftmost", "timing_test_spread.jsonl"))]
    assert rows[-1] == {"runs": 10, "all_green": True}
    by = {r["quantity"]: r for r in rows if "quantity" in r}
    a, b = by["host_route_over_count_leftmost"], by["set_replace_over_searcher_replace"]
    assert a["samples"] == b["samples"] == 10
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    text = open(os.path.join(ROOT, "tests", "test_gpu_zz_leftmost_timing.py")).read()
    floor = float(re.search(r"^FLOOR_HOST_ROUTE_OVER_COUNT_LEFTMOST = ([0-9.]+)", text, flags=re.M).group(1))
    ceiling = float(re.search(r"^CEILING_SET_REPLACE_OVER_SEARCHER_REPLACE = ([0-9.]+)", text, flags=re.M).group(1))
    # the floor: the lowest ratio less the spread, rounded down, never below 1; the ceiling: the highest plus the spread
    assert floor == max(1, int(a["min"] - (a["max"] - a["min"]))) and abs(ceiling - (b["max"] + (b["max"] - b["min"]))) < 5e-4
    bench = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "leftmost", "leftmost_bench_1gib.jsonl"))]
    assert [r["needles"] for r in bench if r["row"] == "set"] == ["1", "3", "16", "words"] and len([r for r in bench if r["row"] == "dense"]) == 2
    assert bench[3]["count"] == 4585 and bench[3]["pairs"] > 8e8 and bench[0]["bytes"] == 1 << 30
