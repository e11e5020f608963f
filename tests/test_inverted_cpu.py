"""CPU checks of the inverted line calls (include/sliceslice_hip_inverted.h): the header, the ctypes table and the Rust module
agree symbol by symbol and are the line calls' argument lists with `unsigned how` behind the delimiter;
libsliceslice_hip_inverted.so exports exactly the six headers while every other library exports what it did; the 36 inverted emit kernels meet the scan kernels' bar, sit in their two translation units and
in no other library's record, and the bounded library's record reappears unchanged; the rule restated here reproduces
tests/golden/inverted_kat.json; the methods are refused outside inverted_build(); tools/grep_hip.py refuses what has no
complement."""
import inspect
import json
import os
import re

import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes
from test_bounded_cpu import BOUNDED, LINES, NOCASE, _grep, bounded_lines_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INVERTED = ["ss_count_lines_inverted_device", "ss_count_lines_inverted_device_async", "ss_find_lines_inverted_device"]
HOWS = ["", "i", "w", "wi", "x", "xi"]


# ---- the rule, restated line by line ------------------------------------------------------------------------------------------
def all_lines(data, delimiter):
    pieces = data.split(bytes([delimiter]))
    if pieces[-1] == b"":
        pieces.pop()
    out, begin = [], 0
    for k, piece in enumerate(pieces):
        out.append((begin, begin + len(piece), k + 1))
        begin += len(piece) + 1
    return out


def inverted_lines_rule(data, needle, delimiter, how):
    """[(begin, end, number)] of the lines that do NOT match under `how`: every line minus test_bounded_cpu's rule ("w", "x") or
    minus the lines that hold the needle ("": a piece between delimiters holds no delimiter, so `in` is the whole rule)"""
    nocase = how.endswith("i")
    n = needle.lower() if nocase else needle
    if how[:1] in ("w", "x"):
        hit = {r[2] for r in bounded_lines_rule(data, n, delimiter, how[0] == "x", nocase)}
    elif delimiter in n:
        hit = set()
    else:
        hit = {k for b, e, k in all_lines(data, delimiter) if n in (data[b:e].lower() if nocase else data[b:e])}
    return [l for l in all_lines(data, delimiter) if l[2] not in hit]


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_inverted.h")
    assert sorted(c) == sorted(ss.searcher.INVERTED_ABI) == sorted(INVERTED)
    # the argument lists of the models with `how` behind the delimiter - exactly the bounded line calls'
    l, b = header_prototypes("sliceslice_hip_lines.h"), header_prototypes("sliceslice_hip_bounded.h")
    for model in LINES:
        res, args = l[model]
        assert c[model.replace("_device", "_inverted_device")] == (res, args[:4] + ["u32"] + args[4:]) == b[model.replace("_device", "_bounded_device")], model
    r, rust = rust_prototypes("hip_inverted.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_inverted.rs")).read()
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.INVERTED_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h",
              "sliceslice_hip_nocase.h"):
        assert not set(c) & set(header_prototypes(h)), h
    assert not set(c) & set(b)
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_inverted.h")).read()
    assert '#include "sliceslice_hip_bounded.h"' in text and "#define SS_BOUND" not in text            # the existing bits and no new ones
    assert "hip_bounded::{SS_BOUND_LINE, SS_BOUND_NOCASE, SS_BOUND_WORD}" in rust and "pub const" not in rust
    for topic in ("Rule:", "Out of scope", "no inverted OCCURRENCE form", "unterminated last line", "empty haystack", "EVERY line",
                  "empty needle", "context lines", "-m", "multi-byte terminators", "regular expressions", "batched, plan, sharded, service",
                  "libsliceslice_hip_inverted.so", "capacity"):
        assert topic.lower() in text.lower(), topic
    # -v left the bounded header's out-of-scope list and DESIGN.md 5.10's
    bounded = open(os.path.join(ROOT, "include", "sliceslice_hip_bounded.h")).read()
    scope = bounded[bounded.index("Out of scope"):]
    assert "-v and" not in scope and "sliceslice_hip_inverted.h" in scope


def test_the_inverted_library_exports_six_headers_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    batched = list(header_prototypes("sliceslice_hip_matches_batched.h"))
    service = list(header_prototypes("sliceslice_hip_service.h"))
    assert _exported(b.build_inverted()) == sorted(product + matches + LINES + NOCASE + BOUNDED + INVERTED)
    assert _exported(b.build_bounded()) == sorted(product + matches + LINES + NOCASE + BOUNDED)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_service()) == sorted(product + service)
    assert _exported(b.build_matches()) == sorted(product + matches)
    assert _exported(b.build_matches_batched()) == sorted(product + matches + batched)
    assert _exported(b.build_lines()) == sorted(product + matches + LINES)
    assert _exported(b.build_nocase()) == sorted(product + matches + LINES + NOCASE)
    assert os.path.basename(b.inverted_library_path()) == "libsliceslice_hip_inverted.so"


def test_the_inverted_kernels_meet_the_scan_kernels_bar():
    b = _build()
    rows = b.inverted_kernel_resources()
    units = {"scan_inst_inverted.hip": {}, "scan_inst_inverted_nocase.hip": {}}
    small = []
    for r in rows:
        if "inverted" not in r["name"]:
            assert r["tu"] not in units, r
            continue
        assert r["tu"] in units, r
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
        m = re.match(r"void ss::lines_emit_inverted_kernel<(\d), (\d), (true|false), (true|false), (true|false)>", r["name"])
        if not m:
            small.append(r["name"].split("(")[0])
            assert r["tu"] == "scan_inst_inverted.hip" and r["vgprs"] <= 64 and r.get("lds_bytes", 0) <= 4096, r
            continue
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128, r
        assert r.get("lds_bytes", 0) <= 1024, r
        fold = m.group(4) == "true"
        assert r["tu"] == ("scan_inst_inverted_nocase.hip" if fold else "scan_inst_inverted.hip"), r
        units[r["tu"]][m.groups()[:3] + (m.group(5),)] = r
    want = sorted(k + (bound,) for k in [(str(q), m, "false") for q in range(4) for m in ("0", "2")] + [("0", "0", "true")]
                  for bound in ("false", "true"))
    for tu, found in units.items():
        assert sorted(found) == want and len(found) == 18, tu
    assert sorted(small) == ["ss::lines_plain_inverted_kernel", "ss::lines_total_inverted_kernel"]
    # emit only: below the twin that also sums up (lines_scan_bounded[_nocase]_kernel of the same choice) in registers and LDS
    twins = {}
    for r in rows:
        m = re.match(r"void ss::lines_scan_bounded(_nocase)?_kernel<(\d), (\d), (true|false)>", r["name"])
        if m:
            twins[(m.group(1) is not None,) + m.groups()[1:]] = r
    for tu, found in units.items():
        for key, r in found.items():
            if key[3] == "true":
                twin = twins[(tu.endswith("_nocase.hip"),) + key[:3]]
                assert r["vgprs"] <= twin["vgprs"] and r["lds_bytes"] < twin["lds_bytes"], (r, twin)
    # every row of the bounded library's record reappears unchanged, and no other record names an inverted kernel
    bounded = b.bounded_kernel_resources()
    assert [r for r in rows if "inverted" not in r["name"]] == bounded and len(rows) == len(bounded) + 36 + 2
    product = json.load(open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "kernel_resources.json")))
    for other in (product, b.matches_kernel_resources(), b.matches_batched_kernel_resources(), b.lines_kernel_resources(),
                  b.nocase_kernel_resources(), bounded):
        assert not [r for r in other if "inverted" in r["name"] or "inverted" in r["tu"]]


def test_the_rule_reproduces_the_fixture():
    kat = json.load(open(os.path.join(GOLDEN, "inverted_kat.json")))
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    words = open(os.path.join(GOLDEN, "data", "words.txt"), "rb").read().split(b"\n")
    assert kat["grep_checked"] is True and "3.7" in kat["grep_version"] and kat["hows"] == HOWS
    assert kat["index"] == list(range(0, 4585, kat["stride"])) and 24 <= len(kat["index"]) <= 60
    assert [words[k].decode("latin-1") for k in kat["index"]] == kat["words"]
    assert kat["lines"] == len(all_lines(data, 10)) == 20854
    for how in HOWS:
        assert len(kat["inverted"][how]) == len(kat["index"]), how
    for j in range(0, len(kat["index"]), 5):
        w = words[kat["index"][j]]
        for how in HOWS:
            assert len(inverted_lines_rule(data, w, 10, how)) == kat["inverted"][how][j], (w, how)
    # the figures the issue, README and DESIGN.md 5.11 quote
    assert kat["table"] == {"the": {"": 16053, "i": 15365, "w": 16438, "wi": 15984, "x": 20854, "xi": 20854},
                            "descriptor": {"": 20517, "i": 20396, "w": 20577, "wi": 20473, "x": 20854, "xi": 20854},
                            "intel": {"": 20851, "i": 20818, "w": 20853, "wi": 20820, "x": 20854, "xi": 20854}}
    for w, t in kat["table"].items():
        assert {how: len(inverted_lines_rule(data, w.encode(), 10, how)) for how in HOWS} == t, w
    # the complement, against the fixtures of the models
    bounded = json.load(open(os.path.join(GOLDEN, "bounded_kat.json")))["table"]
    for w, t in kat["table"].items():
        assert t["w"] + bounded[w]["word_lines"] == t["x"] + bounded[w]["line_lines"] == t["wi"] + bounded[w]["word_lines_nocase"] == kat["lines"]
    whats = " ".join(c["what"] for c in kat["cases"])
    for topic in ("unterminated last line", "longer than the haystack", "holds the delimiter", "empty needle", "empty haystack", "delimiters only",
                  "no delimiter", "across a delimiter", "not folded", "ignoring case", "whole word", "whole line", "empty lines"):
        assert topic in whats, topic
    assert {c["how"] for c in kat["cases"]} == set(HOWS)
    for c in kat["cases"]:
        h, n = bytes.fromhex(c["haystack"]), bytes.fromhex(c["needle"])
        if len(n) == 0:
            assert c["records"] == [] and c["how"] in ("", "i")
            continue
        assert inverted_lines_rule(h, n, c["delimiter"], c["how"]) == [tuple(r) for r in c["records"]], c["what"]


def test_the_methods_are_refused_outside_the_inverted_library():
    class Fake:
        _L = ss.lib()
        _h = None
    calls = (("count_lines_inverted", (b"abc",)), ("count_lines_inverted_async", (None, None)), ("find_lines_inverted", (b"abc",)),
             ("find_lines_inverted_into", (b"abc", None, None, None, 0)))
    for build in (None, ss.matches_build, ss.lines_build, ss.nocase_build, ss.bounded_build):
        if build is not None:
            with build():
                Fake._L = ss.lib()
        for meth, args in calls:
            for kw in ({}, dict(ignore_case=True), dict(whole_word=True), dict(whole_line=True, ignore_case=True)):
                with pytest.raises(ss.SlicesliceError, match="inverted_build") as e:
                    getattr(ss.DynamicHipSearcher, meth)(Fake(), *args, **kw)
                assert e.value.code == ss.SS_ERR_ARGUMENT
    # the signatures are the models', keyword for keyword, on both classes; there is no inverted occurrence method
    for meth, _ in calls:
        model = meth.replace("_inverted", "")
        for cls in (ss.DynamicHipSearcher, ss.MemchrHipSearcher):
            assert str(inspect.signature(getattr(cls, meth))) == str(inspect.signature(getattr(cls, model))), (cls, meth)
    for cls in (ss.DynamicHipSearcher, ss.MemchrHipSearcher):
        assert not [m for m in dir(cls) if "inverted" in m and "lines" not in m]
    assert "no inverted" in ss.inverted_build.__doc__ and not getattr(ss.lib(), "has_inverted", False)


def test_grep_hip_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    usage = _grep()
    assert usage.returncode != 0 and "--invert-match" in usage.stderr and "--word-regexp" in usage.stderr
    for out in ("--count", "--offsets"):
        refused = _grep("-v", out, "a", words)
        assert refused.returncode != 0 and "-v" in refused.stderr and "--count-lines" in refused.stderr and "complement" in refused.stderr, (out, refused)
    alone = _grep("-v", "a", words)
    assert alone.returncode != 0 and "--count-lines" in alone.stderr
    several = _grep("-v", "--count", "-e", "a", "-e", "b", words)
    assert several.returncode != 0 and "-v" in several.stderr and "-e" in several.stderr
    both = _grep("-v", "-w", "-x", "--count-lines", "a", words)
    assert both.returncode != 0 and "-w" in both.stderr and "-x" in both.stderr
    empty = _grep("-v", "-x", "--lines", "", words)
    assert empty.returncode != 0 and "empty" in empty.stderr
    doc = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert "occurrences have no complement" in doc
    for rel in ("tools/fuzz_inverted.py", "tools/inverted_bench.py", "tests/golden/make_inverted_golden.py", "profiles/inverted/README.md",
                "sliceslice-rs_amd/bindings/rust/hip_inverted.rs", "include/sliceslice_hip_inverted.h"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    assert "5.11" in open(os.path.join(ROOT, "DESIGN.md")).read() and "sliceslice_hip_inverted.h" in open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "libsliceslice_hip_inverted.so" in open(os.path.join(ROOT, "README.md")).read()
    assert "hip_inverted.rs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
