"""CPU checks of the whole-word / whole-line calls (include/sliceslice_hip_bounded.h): the header, the ctypes table and the Rust
module agree symbol by symbol and are the models' argument lists with `unsigned how` inserted; libsliceslice_hip_bounded.so exports
exactly the five headers while the product and the five earlier libraries export what they did; the 36 bounded kernels
meet the scan kernels' bar, sit in their two translation units and in no other library's record, and the nocase library's record
reappears unchanged; the rule restated here reproduces tests/golden/bounded_kat.json; the keywords are refused outside
bounded_build(); tools/grep_hip.py refuses what the library refuses."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LINES = ["ss_count_lines_device", "ss_count_lines_device_async", "ss_find_lines_device"]
NOCASE = ["ss_searcher_new_nocase", "ss_count_nocase_device", "ss_count_nocase_device_async", "ss_find_all_nocase_device",
          "ss_count_lines_nocase_device", "ss_count_lines_nocase_device_async", "ss_find_lines_nocase_device"]
BOUNDED = ["ss_count_bounded_device", "ss_count_bounded_device_async", "ss_find_all_bounded_device", "ss_count_lines_bounded_device",
           "ss_count_lines_bounded_device_async", "ss_find_lines_bounded_device"]
WORD_BYTES = frozenset(b"0123456789_" + bytes(range(0x41, 0x5B)) + bytes(range(0x61, 0x7B)))


# ---- the rule, restated line by line (tests/test_gpu_bounded.py restates it once more, on numpy arrays) -------------------------
def _kept_in(piece, j, n, line, first, last):
    """the occurrence [j, j + n) of a piece that holds no delimiter: `first` / `last` say that the piece's ends are the view's ends
    or delimiters (always, in the line forms), so that a neighbour beyond them qualifies"""
    for at, edge in ((j - 1, first), (j + n, last)):
        if at < 0 or at >= len(piece):
            if not edge:
                return False
            continue
        if line or piece[at] in WORD_BYTES:
            return False
    return True


def bounded_offsets_rule(data, needle, nocase=False):
    """WORD in the occurrence forms: ascending offsets of the occurrences both of whose neighbours are absent or no word bytes"""
    h, n = (data.lower(), needle.lower()) if nocase else (data, needle)
    out, i = [], h.find(n) if n else -1
    while i >= 0:
        if _kept_in(data, i, len(n), False, True, True):
            out.append(i)
        i = h.find(n, i + 1)
    return out


def bounded_lines_rule(data, needle, delimiter, line, nocase=False):
    """[(begin, end, number)] of the lines - cut at the delimiter byte as it is - that hold a kept occurrence (WORD: neighbours
    beyond the line's ends or no word bytes; LINE: beyond the line's ends).  A needle that holds the delimiter matches no line."""
    n = needle.lower() if nocase else needle
    pieces = data.split(bytes([delimiter]))
    if pieces[-1] == b"":
        pieces.pop()
    out, begin = [], 0
    for k, piece in enumerate(pieces):
        p = piece.lower() if nocase else piece          # (a piece holds no delimiter, so the fold cannot make one look like a needle byte)
        j = p.find(n) if n and delimiter not in n else -1
        while j >= 0:
            if _kept_in(piece, j, len(n), line, True, True):
                out.append((begin, begin + len(piece), k + 1))
                break
            j = p.find(n, j + 1)
        begin += len(piece) + 1
    return out


# ---- header, ctypes table, Rust block -------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_bounded.h")
    assert sorted(c) == sorted(ss.searcher.BOUNDED_ABI) == sorted(BOUNDED)
    # the argument lists of the models with `how` in front of the stream
    m, l = header_prototypes("sliceslice_hip_matches.h"), header_prototypes("sliceslice_hip_lines.h")
    for model, protos, at in (("ss_count_device", m, 3), ("ss_count_device_async", m, 3), ("ss_find_all_device", m, 3),
                              ("ss_count_lines_device", l, 4), ("ss_count_lines_device_async", l, 4), ("ss_find_lines_device", l, 4)):
        res, args = protos[model]
        assert c[model.replace("_device", "_bounded_device")] == (res, args[:at] + ["u32"] + args[at:]), model
    r, rust = rust_prototypes("hip_bounded.rs"), open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_bounded.rs")).read()
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.BOUNDED_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h",
              "sliceslice_hip_nocase.h"):
        assert not set(c) & set(header_prototypes(h)), h
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_bounded.h")).read()
    assert '#include "sliceslice_hip_nocase.h"' in text
    for name, value in (("SS_BOUND_WORD", 1), ("SS_BOUND_LINE", 2), ("SS_BOUND_NOCASE", 4)):
        assert re.search(r"#define %s\s+%du\b" % (name, value), text), name
        assert re.search(r"pub const %s: c_uint = %d;" % (name, value), rust), name
        assert getattr(ss.searcher, name) == value
    for topic in ("Rule:", "Out of scope", "never folded", "absent", "0x80", "empty needle", "neighbours only", "libsliceslice_hip_bounded.so"):
        assert topic.lower() in text.lower(), topic


def test_the_bounded_library_exports_five_headers_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    batched = list(header_prototypes("sliceslice_hip_matches_batched.h"))
    service = list(header_prototypes("sliceslice_hip_service.h"))
    assert _exported(b.build_bounded()) == sorted(product + matches + LINES + NOCASE + BOUNDED)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_service()) == sorted(product + service)
    assert _exported(b.build_matches()) == sorted(product + matches)
    assert _exported(b.build_matches_batched()) == sorted(product + matches + batched)
    assert _exported(b.build_lines()) == sorted(product + matches + LINES)
    assert _exported(b.build_nocase()) == sorted(product + matches + LINES + NOCASE)
    assert os.path.basename(b.bounded_library_path()) == "libsliceslice_hip_bounded.so"


def test_the_bounded_kernels_meet_the_scan_kernels_bar():
    b = _build()
    rows = b.bounded_kernel_resources()
    units = {"scan_inst_bounded.hip": {"all": {}, "lines": {}}, "scan_inst_bounded_nocase.hip": {"all": {}, "lines": {}}}
    for r in rows:
        if "bounded" not in r["name"]:
            assert r["tu"] not in units, r
            continue
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128, r
        assert r.get("lds_bytes", 0) <= 1024, r
        m = re.match(r"void ss::scan_all_bounded_kernel<(\d), (\d), (true|false), (true|false)>", r["name"])
        if m:
            fold, key, kind = m.group(4) == "true", m.groups()[:3], "all"
        else:
            m = re.match(r"void ss::lines_scan_bounded(_nocase)?_kernel<(\d), (\d), (true|false)>", r["name"])
            assert m, r["name"]
            fold, key, kind = m.group(1) is not None, m.groups()[1:], "lines"
        assert r["tu"] == ("scan_inst_bounded_nocase.hip" if fold else "scan_inst_bounded.hip"), r
        units[r["tu"]][kind][key] = r
    want = sorted([(str(q), m, "false") for q in range(4) for m in ("0", "2")] + [("0", "0", "true")])
    for tu, found in units.items():
        assert sorted(found["all"]) == want and sorted(found["lines"]) == want, tu
        assert len([r for r in rows if r["tu"] == tu]) == 18, tu
    # every row of the nocase library's record reappears unchanged, and no other record names a bounded kernel
    nocase = b.nocase_kernel_resources()
    assert [r for r in rows if "bounded" not in r["name"]] == nocase and len(rows) == len(nocase) + 36
    product = json.load(open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "kernel_resources.json")))
    for other in (product, b.matches_kernel_resources(), b.matches_batched_kernel_resources(), b.lines_kernel_resources(), nocase):
        assert not [r for r in other if "bounded" in r["name"]]


def test_is_word_byte_is_the_c_locale_class():
    assert {b for b in range(256) if ss.is_word_byte(b)} == set(WORD_BYTES) and len(WORD_BYTES) == 63
    for b in b"@[`{/:\x80\xc1\xe1\xff \n\x00":
        assert not ss.is_word_byte(b), b
    # closed under the fold: a letter and its other case are in the same class
    assert all(ss.is_word_byte(b) == ss.is_word_byte(ss.fold_ascii(bytes([b]))[0]) for b in range(256))
    # ... and the kernels' test (bounded_kernels.hpp), restated on Python integers
    src = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "bounded_kernels.hpp")).read()
    body = src[src.index("bool is_word_byte(uint32_t b)"):]
    assert "((b | 0x20u) - 'a') < 26u || (b - '0') < 10u || b == '_'" in body[:body.index("}")]
    u32 = 0xFFFFFFFF
    for b in range(256):
        assert ((((b | 0x20) - 0x61) & u32) < 26 or ((b - 0x30) & u32) < 10 or b == 0x5F) == ss.is_word_byte(b), b


def test_the_rule_reproduces_the_fixture():
    kat = json.load(open(os.path.join(GOLDEN, "bounded_kat.json")))
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    words = open(os.path.join(GOLDEN, "data", "words.txt"), "rb").read().split(b"\n")
    assert kat["grep_checked"] is True and kat["grep_version"]
    assert kat["index"] == list(range(0, 4585, kat["stride"])) and 300 <= len(kat["index"]) <= 500
    assert [words[k].decode("latin-1") for k in kat["index"]] == kat["words"]
    for key in ("word_count", "word_lines", "line_lines", "word_count_nocase", "word_lines_nocase", "line_lines_nocase"):
        assert len(kat[key]) == len(kat["index"]), key

    def figures(w):
        return {"word_count": len(bounded_offsets_rule(data, w)), "word_lines": len(bounded_lines_rule(data, w, 10, False)),
                "line_lines": len(bounded_lines_rule(data, w, 10, True)), "word_count_nocase": len(bounded_offsets_rule(data, w, True)),
                "word_lines_nocase": len(bounded_lines_rule(data, w, 10, False, True)),
                "line_lines_nocase": len(bounded_lines_rule(data, w, 10, True, True))}
    for j in range(0, len(kat["index"]), 7):
        got = figures(words[kat["index"][j]])
        assert got == {key: kat[key][j] for key in got}, kat["words"][j]
    # the figures README and DESIGN.md 5.10 quote
    assert kat["table"]["the"] == {"count": 7398, "word_count": 6524, "word_lines": 4416, "line_lines": 0, "word_count_nocase": 7755,
                                   "word_lines_nocase": 4870, "line_lines_nocase": 0}
    for w, t in kat["table"].items():
        assert dict(figures(w.encode()), count=t["count"]) == t, w
    assert sum(kat["line_lines"]) > 0 and sum(kat["word_count"]) > sum(kat["word_lines"]) > 0
    whats = " ".join(c["what"] for c in kat["cases"])
    for topic in ("'@'", "'_'", "0x80", "0xC1", "exactly the needle", "len == n + 1", "neighbours only", "overlapping", "one-byte",
                  "also behind others", "still ends a word", "holds the delimiter", "open last line", "empty lines", "0x00",
                  "not folded", "whole line ignoring case"):
        assert topic in whats, topic
    for c in kat["cases"]:
        h, n = bytes.fromhex(c["haystack"]), bytes.fromhex(c["needle"])
        nocase, line = c["how"].endswith("i"), c["how"].startswith("x")
        assert (c["offsets"] is None) == line, c["what"]
        if not line:
            assert bounded_offsets_rule(h, n, nocase) == c["offsets"], c["what"]
        assert bounded_lines_rule(h, n, c["delimiter"], line, nocase) == [tuple(r) for r in c["records"]], c["what"]


def test_the_keywords_are_refused_outside_the_bounded_library():
    class Fake:
        _L = ss.lib()
        _h = None
    calls = (("count", (b"abc",)), ("count_async", (None, None)), ("find_all", (b"abc",)), ("find_all_into", (b"abc", None)),
             ("count_lines", (b"abc",)), ("count_lines_async", (None, None)), ("find_lines", (b"abc",)),
             ("find_lines_into", (b"abc", None, None, None, 0)))
    line_methods = ("count_lines", "count_lines_async", "find_lines", "find_lines_into")
    for build in (None, ss.matches_build, ss.lines_build, ss.nocase_build):
        if build is not None:
            with build():
                Fake._L = ss.lib()
        for meth, args in calls:
            for kw in (dict(whole_word=True), dict(whole_word=True, ignore_case=True)) + \
                      ((dict(whole_line=True), dict(whole_line=True, ignore_case=True)) if meth in line_methods else ()):
                with pytest.raises(ss.SlicesliceError, match="bounded_build") as e:
                    getattr(ss.DynamicHipSearcher, meth)(Fake(), *args, **kw)
                assert e.value.code == ss.SS_ERR_ARGUMENT
    for meth, _ in calls:
        names = list(inspect.signature(getattr(ss.DynamicHipSearcher, meth)).parameters)
        tail = ["ignore_case", "whole_word"] + (["whole_line"] if meth in line_methods else [])
        assert names[-len(tail):] == tail, (meth, names)                 # behind ignore_case: positional calls mean what they did
        for k in tail:
            assert inspect.signature(getattr(ss.DynamicHipSearcher, meth)).parameters[k].default is False, (meth, k)
        assert ("whole_line" in names) == (meth in line_methods), meth
    for meth in ("count", "find_all", "count_lines", "count_lines_async", "find_lines", "find_lines_into"):
        names = list(inspect.signature(getattr(ss.MemchrHipSearcher, meth)).parameters)
        assert "whole_word" in names and ("whole_line" in names) == (meth in line_methods), meth
    assert not getattr(ss.lib(), "has_bounded", False)


def _grep(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grep_hip.py")] + list(args), capture_output=True, text=True)


def test_grep_hip_argument_errors_and_documents():
    words = os.path.join(GOLDEN, "data", "words.txt")
    usage = _grep()
    assert usage.returncode != 0 and "--word-regexp" in usage.stderr and "--line-regexp" in usage.stderr
    both = _grep("-w", "-x", "--count-lines", "a", words)
    assert both.returncode != 0 and "-w" in both.stderr and "-x" in both.stderr
    for out in ("--count", "--offsets"):
        refused = _grep("-x", out, "a", words)
        assert refused.returncode != 0 and "-x" in refused.stderr and "--count-lines" in refused.stderr, (out, refused)
    alone = _grep("-w", "a", words)
    assert alone.returncode != 0 and "--count" in alone.stderr
    empty = _grep("-w", "--count", "", words)
    assert empty.returncode != 0 and "empty" in empty.stderr
    several = _grep("-w", "--count", "-e", "a", "-e", "b", words)
    assert several.returncode != 0 and "-w" in several.stderr and "-e" in several.stderr
    for rel in ("tools/fuzz_bounded.py", "tools/bounded_bench.py", "tests/golden/make_bounded_golden.py", "profiles/bounded/README.md",
                "sliceslice-rs_amd/bindings/rust/hip_bounded.rs", "include/sliceslice_hip_bounded.h"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    assert "5.10" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "libsliceslice_hip_bounded.so" in open(os.path.join(ROOT, "README.md")).read()
