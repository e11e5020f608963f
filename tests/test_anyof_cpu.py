"""CPU checks of the several-needle calls (include/sliceslice_hip_anyof.h): the header, the ctypes table and the Rust module agree
symbol by symbol; libsliceslice_hip_anyof.so exports the context library's list plus three functions while every other library
exports what it did; the two new kernels meet their resource bar and every
row of the context record reappears unchanged; the union rule restated here on numpy arrays reproduces tests/golden/anyof_kat.json
(GNU grep's output); the index arithmetic of csrc/anyof_segments.hpp passes an exhaustive sweep in a stand-alone host program built
with ASan and UBSan; the functions are refused outside anyof_build(); tools/grep_hip.py documents and refuses what it should."""
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
from test_context_cpu import CONTEXT, checksum, context_rule, selected_numbers, separators
from test_inverted_cpu import INVERTED, all_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ANYOF = ["ss_union_numbers_device", "ss_count_lines_anyof_device", "ss_find_lines_anyof_device"]


# ---- the rule on numpy arrays ---------------------------------------------------------------------------------------------------
def anyof_rule(data, needles, delimiter, how, invert):
    """the numbers of the lines that match any needle under `how` (the union of the single-needle rules), or with `invert` of the
    lines that match none"""
    union = set()
    for needle in needles:
        union.update(selected_numbers(data, needle, delimiter, how, False))
    return [l[2] for l in all_lines(data, delimiter) if (l[2] in union) != invert]


def test_the_rule_on_small_cases():
    data = b"ab\nabc\n\nxbc\nAB"
    assert anyof_rule(data, [b"ab", b"bc"], 10, "", False) == [1, 2, 4] and anyof_rule(data, [b"ab", b"bc"], 10, "", True) == [3, 5]
    assert anyof_rule(data, [b"ab", b"abc"], 10, "", False) == anyof_rule(data, [b"abc", b"ab", b"ab"], 10, "", False) == [1, 2]
    assert anyof_rule(data, [b"ab", b"xbc"], 10, "x", False) == [1, 4] and anyof_rule(data, [b"ab"], 10, "i", False) == [1, 2, 5]
    assert anyof_rule(data, [b"zz", b""], 10, "", False) == [1, 2, 3, 4, 5] and anyof_rule(data, [b"zz"], 10, "w", True) == [1, 2, 3, 4, 5]


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_anyof.h")
    assert sorted(c) == sorted(ss.searcher.ANYOF_ABI) == sorted(ANYOF)
    # the find call is the context call with (searchers, needles) in the searcher's place; the count call is its head and `lines`
    context = header_prototypes("sliceslice_hip_context.h")["ss_find_lines_context_device"][1]
    assert c["ss_find_lines_anyof_device"][1] == ["ptr", "u32"] + context[1:]
    assert c["ss_count_lines_anyof_device"][1] == ["ptr", "u32"] + context[1:5] + ["ptr", "ptr"]
    assert c["ss_union_numbers_device"][1] == ["ptr", "ptr", "ptr", "u32", "u64", "i32", "ptr", "ptr", "u64", "ptr"]
    r, rust = rust_prototypes("hip_anyof.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_anyof.rs")).read()
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.ANYOF_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h",
              "sliceslice_hip_nocase.h"):
        assert not set(c) & set(header_prototypes(h)), h
    assert not set(c) & (set(header_prototypes("sliceslice_hip_context.h")) | set(BOUNDED) | set(INVERTED))
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_anyof.h")).read()
    assert '#include "sliceslice_hip_context.h"' in text and "#define SS_BOUND" not in text and "#define SS_CONTEXT" not in text
    most = int(re.search(r"#define SS_ANYOF_MAX_NEEDLES\s+(\d+)u\b", text).group(1))
    segment = int(re.search(r"#define SS_ANYOF_SEGMENT_LINES\s+(\d+)u\b", text).group(1))
    assert most == ss.ANYOF_MAX_NEEDLES == ss.searcher.ANYOF_MAX_NEEDLES == 65536 and ("SS_ANYOF_MAX_NEEDLES: u32 = %d;" % most) in rust
    assert segment == ss.ANYOF_SEGMENT_LINES == ss.searcher.ANYOF_SEGMENT_LINES == 65536 and ("SS_ANYOF_SEGMENT_LINES: u64 = %d;" % segment) in rust
    for topic in ("Rule:", "Out of scope", "STRICTLY ASCENDING", "breach", "complement", "capacity", "count only", "no global atomic",
                  "never per line", "deterministic", "capturable", "libsliceslice_hip_anyof.so", "SS_ERR_NOMEM", "K times", "census",
                  "reads the numbers twice", "never touches the haystack", "single pass over the haystack", "-m", "-o with several needles",
                  "regular expressions", "multi-byte terminators", "batched, plan, sharded, service", "prefix of another", "2^31 - 1"):
        assert topic.lower() in " ".join(re.sub(r"^ \*", "", text, flags=re.M).lower().split()), topic
    # the earlier headers point here and keep the words that the earlier tests look for
    for h in ("sliceslice_hip_context.h", "sliceslice_hip_inverted.h", "sliceslice_hip_bounded.h"):
        old = open(os.path.join(ROOT, "include", h)).read()
        scope = old[old.index("Out of scope"):]
        assert "sliceslice_hip_anyof.h" in scope and "several needles" in scope and "-m" in scope, h


def test_the_anyof_library_exports_the_context_list_plus_three_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    batched = list(header_prototypes("sliceslice_hip_matches_batched.h"))
    service = list(header_prototypes("sliceslice_hip_service.h"))
    context = product + matches + LINES + NOCASE + BOUNDED + INVERTED + CONTEXT
    assert _exported(b.build_anyof()) == sorted(context + ANYOF)
    assert _exported(b.build_context()) == sorted(context)
    assert _exported(b.build_inverted()) == sorted(product + matches + LINES + NOCASE + BOUNDED + INVERTED)
    assert _exported(b.build_bounded()) == sorted(product + matches + LINES + NOCASE + BOUNDED)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_service()) == sorted(product + service)
    assert _exported(b.build_matches()) == sorted(product + matches)
    assert _exported(b.build_matches_batched()) == sorted(product + matches + batched)
    assert _exported(b.build_lines()) == sorted(product + matches + LINES)
    assert _exported(b.build_nocase()) == sorted(product + matches + LINES + NOCASE)
    assert os.path.basename(b.anyof_library_path()) == "libsliceslice_hip_anyof.so"


def test_the_union_kernels_meet_their_bar_and_every_other_row_is_what_it_was():
    b = _build()
    rows = b.anyof_kernel_resources()
    own = [r for r in rows if r["tu"] == "ss_anyof.hip"]
    names = sorted(r["name"].split("(")[0] for r in own)
    assert names == ["ss::anyof_count_kernel", "ss::anyof_emit_kernel", "void ss::prefix_kernel<unsigned long>"], names
    for r in own:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128 and r.get("lds_bytes", 0) <= 16384, r
    for r in own:
        if "anyof" in r["name"]:
            assert r["lds_bytes"] >= 8192, r                      # (the bitmap is in LDS)
    # every row of the context library's record reappears unchanged, and no other record names a union kernel
    context = b.context_kernel_resources()
    assert [r for r in rows if r["tu"] != "ss_anyof.hip"] == context and len(rows) == len(context) + 3
    product = json.load(open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "kernel_resources.json")))
    for other in (product, b.matches_kernel_resources(), b.lines_kernel_resources(), b.nocase_kernel_resources(), b.bounded_kernel_resources(),
                  b.inverted_kernel_resources(), context):
        assert not [r for r in other if "anyof" in r["name"] or "anyof" in r["tu"]]
    kernels = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "anyof_kernels.hpp")).read()
    assert "atomicOr(&s_bits" in kernels and "atomicAdd" not in kernels and "atomicOr(&aa" not in kernels        # LDS atomics only


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_the_rule_reproduces_the_fixture():
    kat = json.load(open(os.path.join(GOLDEN, "anyof_kat.json")))
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    assert kat["grep_checked"] is True and "3.7" in kat["grep_version"] and kat["lines"] == len(all_lines(data, 10)) == 20854
    assert os.path.getsize(os.path.join(GOLDEN, "anyof_kat.json")) < os.path.getsize(os.path.join(GOLDEN, "nocase_kat.json"))
    # five needle sets under eight flag combinations; the table of the issue, README and DESIGN.md 5.13
    sets = {tuple(r["needles"]) for r in kat["rows"]}
    assert sets == {("the", "descriptor", "intel"), ("segment", "segmentation"), ("a", "ab"), ("Intel", "386", "no-such-phrase-here"),
                    ("protect", "protected", "protection", "mode")} and len(kat["rows"]) == 40
    flags = {("", False), ("w", False), ("i", False), ("x", False), ("wi", False), ("", True), ("w", True), ("i", True)}
    seen = {(tuple(r["needles"]), r["how"], r["invert"]): r["selected"] for r in kat["rows"]}
    assert set(seen) == {(s, h, v) for s in sets for h, v in flags}
    the = ("the", "descriptor", "intel")
    quoted = {(the, "", False): 4962, (the, "w", False): 4558, (the, "i", False): 5766, (the, "wi", False): 5115, (the, "", True): 15892,
              (the, "w", True): 16296, (("segment", "segmentation"), "x", False): 1, (("Intel", "386", "no-such-phrase-here"), "x", False): 4,
              (("a", "ab"), "w", False): 1706}
    for key, figure in quoted.items():
        assert seen[key] == figure, key
    assert len(selected_numbers(data, b"the", 10, "", False)) == 4801
    for r in kat["rows"]:
        what = (r["needles"], r["how"], r["invert"])
        sel = anyof_rule(data, [n.encode() for n in r["needles"]], 10, r["how"], r["invert"])
        assert len(sel) == r["selected"] and sel[:20] == r["first"] and sel[-20:] == r["last"], what
        assert hashlib.sha256("".join("%d\n" % n for n in sel).encode()).hexdigest() == r["sha256"], what
    rows = kat["context_rows"]
    assert len(rows) >= 4 and any((r["before"], r["after"]) == (1, 2) for r in rows) and any(r["before"] > kat["lines"] for r in rows)
    assert any(r["before"] == r["after"] == 2 and r["invert"] and r["how"] == "w" for r in rows) and any(r["selected"] == r["printed"] == 0 for r in rows)
    for r in rows:
        what = (r["needles"], r["how"], r["invert"], r["before"], r["after"])
        sel = anyof_rule(data, [n.encode() for n in r["needles"]], 10, r["how"], r["invert"])
        numbers, kinds = context_rule(sel, kat["lines"], r["before"], r["after"])
        assert (len(sel), numbers.size, separators(numbers)) == (r["selected"], r["printed"], r["separators"]), what
        pairs = [list(p) for p in zip(numbers.tolist(), kinds.tolist())]
        assert pairs[:20] == r["first"] and pairs[-20:] == r["last"] and checksum(numbers, kinds) == r["sha256"], what
    # the project's word list as a -f file: the count of the lines that hold any of its words
    row = kat["words_row"]
    words = [w for w in open(os.path.join(GOLDEN, row["file"]), "rb").read().split(b"\n") if w]
    assert len(words) == row["needles"] == 4585 and row["how"] == "" and row["invert"] is False
    starts = np.concatenate(([0], np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10) + 1))
    hit = np.zeros(starts.size + 1, dtype=bool)
    for w in set(words):
        at, found = data.find(w), []
        while at >= 0:
            found.append(at)
            at = data.find(w, at + 1)
        hit[np.searchsorted(starts, np.asarray(found, dtype=np.int64), side="right")] = True
    assert int(hit.sum()) == row["selected"]


# ---- the index arithmetic, on the host ------------------------------------------------------------------------------------------
def test_the_segment_arithmetic_in_a_host_program_under_asan_and_ubsan(tmp_path):
    """tests/native/anyof_segments_check.cpp: segments of 4 numbers, N <= 10, every subset over 1 to 3 lists with duplicates, with
    and without complement, every capacity, against a brute-force union; the real segment size at its borders; lists out of order.
    A program of its own, compiled for the host and run as a child."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++")
    src = os.path.join(ROOT, "tests", "native", "anyof_segments_check.cpp")
    exe = str(tmp_path / "anyof_segments_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 failures" in ran.stdout and "runtime error" not in ran.stderr, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert int(ran.stdout.split()[-4]) > 1000000                 # (the sweep ran)
    header = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "anyof_segments.hpp")).read()
    assert "__host__ __device__" in header and "hip_runtime" not in header
    assert '#include "anyof_segments.hpp"' in open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "anyof_kernels.hpp")).read()


# ---- Python and the command-line tool -----------------------------------------------------------------------------------------
def test_the_functions_are_refused_outside_the_anyof_library():
    class Fake:
        _L = ss.lib()
        _h = None
    calls = ((ss.count_lines_anyof, ([Fake()], b"abc")), (ss.find_lines_anyof, ([Fake(), Fake()], b"abc")),
             (ss.find_lines_anyof_into, ([Fake()], b"abc", None, None, None, None, 0)), (ss.union_numbers, ([[1, 2]], 5)),
             (ss.union_numbers_into, ([[1, 2]], 5, None, 0)), (ss.count_lines_anyof, ([], b"abc")))
    for build in (None, ss.lines_build, ss.inverted_build, ss.context_build):
        for fn, args in calls:
            for kw in ({}, dict(stream=None)):
                with pytest.raises(ss.SlicesliceError, match="anyof_build") as e:
                    if build is None:
                        fn(*args, **kw)
                    else:
                        with build():
                            Fake._L = ss.lib()
                            fn(*args, **kw)
                assert e.value.code == ss.SS_ERR_ARGUMENT
    flags = "ignore_case=False, whole_word=False, whole_line=False, invert=False)"
    want = {"count_lines_anyof": "(searchers, haystack, delimiter=b'\\n', stream=None, " + flags,
            "find_lines_anyof": "(searchers, haystack, before=0, after=0, delimiter=b'\\n', capacity=None, stream=None, " + flags,
            "find_lines_anyof_into": "(searchers, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b'\\n', "
                                     "stream=None, " + flags,
            "union_numbers": "(lists, limit, complement=False, capacity=None, stream=None)",
            "union_numbers_into": "(lists, limit, d_out, capacity, complement=False, stream=None)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(ss, name))) == sig and getattr(ss, name) is getattr(ss.searcher, name), name
    assert "grep -e" in ss.anyof_build.__doc__ and not getattr(ss.lib(), "has_anyof", False)


def test_grep_hip_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    # what the earlier tests pin stays: several patterns with --count refuse -i, -w, -v and context, naming the flag and -e
    for flag in (("-w",), ("-v",), ("-C", "1"), ("-i",), ("-x",)):
        refused = _grep(*flag, "--count", "-e", "a", "-e", "b", words)
        assert refused.returncode != 0 and flag[0] in refused.stderr and "-e" in refused.stderr, (flag, refused)
    alone = _grep("-i", "-e", "a", "-e", "b", words)
    assert alone.returncode != 0 and "-i" in alone.stderr and "-e" in alone.stderr
    # the line outputs with -e / -f: what they refuse before any library is loaded
    for out in ("--count-lines", "--lines"):
        both = _grep("-w", "-x", out, "-e", "a", "-e", "b", words)
        assert both.returncode != 0 and "-w" in both.stderr and "-x" in both.stderr
        empty = _grep("-x", out, "-e", "a", "-e", "", words)
        assert empty.returncode != 0 and "empty" in empty.stderr
        usage = _grep(out, "-e", "a", "-e", "b")
        assert usage.returncode != 0 and "--count-lines | --lines" in usage.stderr and "-f <patterns file>" in usage.stderr
    two = _grep("--count-lines", "--lines", "-e", "a", words)
    assert two.returncode != 0 and "--count-lines | --lines" in two.stderr
    for flag in (("-A", "2"), ("-C2",), ("--context=2",)):
        refused = _grep(*flag, "--count-lines", "-e", "a", "-e", "b", words)
        assert refused.returncode != 0 and "--lines" in refused.stderr and "context" in refused.stderr.lower(), (flag, refused)
    bad = _grep("-C", "x", "--lines", "-e", "a", words)
    assert bad.returncode != 0 and "non-negative integer" in bad.stderr
    doc = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert "ss_count_lines_anyof_device" in doc and "LC_ALL=C grep -F -c" in doc and "grep -f FILE" in doc and "libsliceslice_hip_anyof.so" in doc
    for rel in ("tools/fuzz_anyof.py", "tools/anyof_bench.py", "tests/golden/make_anyof_golden.py", "profiles/anyof/README.md",
                "sliceslice-rs_amd/bindings/rust/hip_anyof.rs", "include/sliceslice_hip_anyof.h", "tests/native/anyof_segments_check.cpp"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    assert "5.13" in open(os.path.join(ROOT, "DESIGN.md")).read() and "sliceslice_hip_anyof.h" in open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "libsliceslice_hip_anyof.so" in open(os.path.join(ROOT, "README.md")).read()
    assert "hip_anyof.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
