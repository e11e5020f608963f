"""CPU checks of the calls that ignore ASCII case (include/sliceslice_hip_nocase.h): the header, the ctypes table and the Rust module
agree symbol by symbol; libsliceslice_hip_nocase.so exports exactly the four headers while the other libraries export what they did;
the folding kernels meet the scan kernels' bar and live in no other library; the Python methods refuse outside nocase_build();
fold_ascii is bytes.lower(); the rule restated here reproduces tests/golden/nocase_kat.json."""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys

import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class as norm, exported as _exported, header_prototypes, rust_prototypes
from test_lines_cpu import lines_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LINES = ["ss_count_lines_device", "ss_count_lines_device_async", "ss_find_lines_device"]
NOCASE = ["ss_searcher_new_nocase", "ss_count_nocase_device", "ss_count_nocase_device_async", "ss_find_all_nocase_device",
          "ss_count_lines_nocase_device", "ss_count_lines_nocase_device_async", "ss_find_lines_nocase_device"]


def count_rule(data, needle):
    """overlapping occurrences of needle in data, case-sensitive"""
    c, i = 0, data.find(needle)
    while i >= 0:
        c, i = c + 1, data.find(needle, i + 1)
    return c


def offsets_nocase(data, needle):
    h, n = data.lower(), needle.lower()
    if not n:
        return list(range(len(h) + 1))
    out, i = [], h.find(n)
    while i >= 0:
        out.append(i)
        i = h.find(n, i + 1)
    return out


def lines_nocase(data, needle, delimiter):
    """lines_rule ignoring case.  The cut is made on the bytes as they are: a delimiter that is a letter is replaced by a byte that
    bytes.lower() leaves alone and that occurs in neither side before the fold."""
    if delimiter in needle.lower():         # (the searcher's needle is the folded one)
        return []
    if 0x41 <= delimiter <= 0x5A or 0x61 <= delimiter <= 0x7A:
        spare = next(b for b in range(0x80, 0x100) if b not in data and b not in needle)
        data, delimiter = data.replace(bytes([delimiter]), bytes([spare])), spare
    return lines_rule(data.lower(), needle.lower(), delimiter)


def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_nocase.h")
    assert sorted(c) == sorted(ss.searcher.NOCASE_ABI) == sorted(NOCASE)
    # the argument lists of the models
    m, l, p = header_prototypes("sliceslice_hip_matches.h"), header_prototypes("sliceslice_hip_lines.h"), header_prototypes()
    assert c["ss_searcher_new_nocase"] == p["ss_searcher_new"]
    for model, protos in (("ss_count_device", m), ("ss_count_device_async", m), ("ss_find_all_device", m), ("ss_count_lines_device", l),
                          ("ss_count_lines_device_async", l), ("ss_find_lines_device", l)):
        assert c[model.replace("_device", "_nocase_device")] == protos[model], model
    r = rust_prototypes("hip_nocase.rs")
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.NOCASE_ABI.items():
        got = (norm(res), [norm(a) for a in args])
        want = c[name]
        assert [a.replace("usize", "u64") for a in got[1]] == [a.replace("usize", "u64") for a in want[1]] and got[0] == want[0], name
    for h in ("sliceslice_hip.h", "sliceslice_hip_matches.h", "sliceslice_hip_matches_batched.h", "sliceslice_hip_lines.h"):
        assert not set(c) & set(header_prototypes(h)), h
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_nocase.h")).read()
    assert '#include "sliceslice_hip_lines.h"' in text
    for topic in ("Out of scope", "never folded", "ss_searcher_new_nocase", "0xC1"):
        assert topic.lower() in text.lower(), topic


def test_the_nocase_library_exports_four_headers_and_the_others_what_they_did():
    b = _build()
    product = list(header_prototypes())
    matches = list(header_prototypes("sliceslice_hip_matches.h"))
    batched = list(header_prototypes("sliceslice_hip_matches_batched.h"))
    assert _exported(b.build_nocase()) == sorted(product + matches + LINES + NOCASE)
    assert _exported(ss.build()) == sorted(product)
    assert _exported(b.build_matches()) == sorted(product + matches)
    assert _exported(b.build_matches_batched()) == sorted(product + matches + batched)
    assert _exported(b.build_lines()) == sorted(product + matches + LINES)
    assert os.path.basename(b.nocase_library_path()) == "libsliceslice_hip_nocase.so"


def test_the_folding_kernels_meet_the_scan_kernels_bar():
    b = _build()
    rows = b.nocase_kernel_resources()
    assert len([r for r in rows if re.match(r"void ss::scan_kernel<", r["name"])]) == 22         # the product's objects, unchanged
    assert len([r for r in rows if re.match(r"void ss::scan_all_kernel<", r["name"])]) == 9      # ... the matches library's
    assert len([r for r in rows if re.match(r"void ss::lines_scan_kernel<", r["name"])]) == 9    # ... and the lines library's
    found = {"scan_all_nocase_kernel": {}, "lines_scan_nocase_kernel": {}}
    for r in rows:
        if "nocase" not in r["name"]:
            continue
        assert r["tu"] == "scan_inst_nocase.hip", r
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128, r
        assert r.get("lds_bytes", 0) <= 1024, r
        m = re.match(r"void ss::(scan_all_nocase_kernel|lines_scan_nocase_kernel)<(\d), (\d), (true|false)>", r["name"])
        assert m, r["name"]
        found[m.group(1)][m.groups()[1:]] = r
    want = sorted([(str(q), m, "false") for q in range(4) for m in ("0", "2")] + [("0", "0", "true")])
    assert sorted(found["scan_all_nocase_kernel"]) == want and sorted(found["lines_scan_nocase_kernel"]) == want
    # that translation unit holds nothing else, and the folding kernels are in no other library's record
    assert len([r for r in rows if r["tu"] == "scan_inst_nocase.hip"]) == 18
    product = json.load(open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "kernel_resources.json")))
    assert len(product) == 37
    for other in (b.matches_kernel_resources(), b.matches_batched_kernel_resources(), b.lines_kernel_resources(), product):
        assert not [r for r in other if "nocase" in r["name"]]
    # the library is the lines library plus that unit
    assert sorted(r["kernel"] for r in rows if "nocase" not in r["name"]) == sorted(r["kernel"] for r in b.lines_kernel_resources())


def test_methods_refuse_outside_the_nocase_library():
    class Fake:
        _L = ss.lib()
        _h = None
    calls = (("count", (b"abc",)), ("count_async", (None, None)), ("find_all", (b"abc",)), ("find_all_into", (b"abc", None)),
             ("count_lines", (b"abc",)), ("count_lines_async", (None, None)), ("find_lines", (b"abc",)),
             ("find_lines_into", (b"abc", None, None, None, 0)))
    for build in (None, ss.matches_build, ss.lines_build):
        if build is not None:
            with build():
                Fake._L = ss.lib()
        for meth, args in calls:
            with pytest.raises(ss.SlicesliceError, match="nocase_build"):
                getattr(ss.DynamicHipSearcher, meth)(Fake(), *args, ignore_case=True)
        with pytest.raises(ss.SlicesliceError, match="nocase_build"):
            with (build() if build is not None else _Nothing()):
                ss.DynamicHipSearcher.new_nocase(b"Abc")
    import inspect
    for meth, _ in calls:
        assert inspect.signature(getattr(ss.DynamicHipSearcher, meth)).parameters["ignore_case"].default is False, meth
    for meth in ("count", "find_all", "count_lines", "count_lines_async", "find_lines", "find_lines_into"):
        assert inspect.signature(getattr(ss.MemchrHipSearcher, meth)).parameters["ignore_case"].default is False, meth
    with ss.nocase_build() as L:
        assert L.has_nocase and L.has_lines and L.has_matches and not L.has_matches_batched
    assert not getattr(ss.lib(), "has_nocase", False)


class _Nothing:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def test_fold_ascii_is_bytes_lower():
    every = bytes(range(256))
    assert ss.fold_ascii(every) == every.lower()
    assert [b for b in range(256) if ss.fold_ascii(bytes([b])) != bytes([b])] == list(range(0x41, 0x5B))
    assert ss.fold_ascii(b"@AZ[`az{\xc1\xda\xe1\xfa") == b"@az[`az{\xc1\xda\xe1\xfa"
    assert ss.fold_ascii(bytearray(b"MiXed")) == b"mixed" and ss.fold_ascii(b"") == b""


def test_the_word_fold_of_the_kernels_on_every_byte_in_every_lane():
    """fold_ascii4 of csrc/scan_filters.hpp, restated on Python integers with the constants read from the source."""
    src = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "scan_filters.hpp")).read()
    body = src[src.index("uint32_t fold_ascii4(uint32_t x)"):]
    body = body[:body.index("}")]
    consts = [int(c, 16) for c in re.findall(r"0x([0-9a-f]{8})u", body)]
    assert consts == [0x7f7f7f7f, 0x3f3f3f3f, 0x25252525, 0x80808080] and "m >> 2" in body, consts

    def fold4(x):
        h = x & consts[0]
        m = ((h + consts[1]) & ~(h + consts[2]) & ~x & consts[3]) & 0xFFFFFFFF
        return x | (m >> 2)

    for lane in range(4):
        for b in range(256):
            for fill in (0x00, 0x41, 0x5A, 0x7F, 0xFF, 0x5B, 0x40):
                raw = bytearray([fill] * 4)
                raw[lane] = b
                assert struct.pack("<I", fold4(struct.unpack("<I", raw)[0])) == bytes(raw).lower(), (lane, b, fill)
    import random
    rnd = random.Random(9)
    for _ in range(20000):
        raw = bytes(rnd.getrandbits(8) for _ in range(4))
        assert struct.pack("<I", fold4(struct.unpack("<I", raw)[0])) == raw.lower(), raw


def test_the_rule_reproduces_the_fixture():
    kat = json.load(open(os.path.join(GOLDEN, "nocase_kat.json")))
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    words = open(os.path.join(GOLDEN, "data", "words.txt"), "rb").read().split()
    low = data.lower()
    assert len(words) == kat["words"] == len(kat["count"]) == len(kat["count_lines"]) == 4585
    assert sum(kat["count"]) == kat["total_count"] and sum(kat["count_lines"]) == kat["total_lines"]
    assert kat["differ"] == 2427
    lines = low.split(b"\n")[:-1]
    for k in list(range(0, len(words), 97)) + [words.index(b"the"), words.index(b"Intel")]:
        assert count_rule(low, words[k].lower()) == kat["count"][k], words[k]
        assert sum(1 for l in lines if words[k].lower() in l) == kat["count_lines"][k], words[k]
    # the figures quoted in DESIGN.md 5.9
    assert kat["table"] == {"descriptor": {"count": 355, "count_nocase": 480, "lines": 337, "lines_nocase": 458},
                            "the": {"count": 7398, "count_nocase": 9008, "lines": 4801, "lines_nocase": 5489},
                            "intel": {"count": 5, "count_nocase": 44, "lines": 3, "lines_nocase": 36}}
    for w, t in kat["table"].items():
        n = w.encode()
        assert (count_rule(data, n), count_rule(low, n)) == (t["count"], t["count_nocase"]), w
        assert (len(lines_rule(data, n, 10)), len(lines_nocase(data, n, 10))) == (t["lines"], t["lines_nocase"]), w
    assert kat["count"][words.index(b"the")] == 9008 and kat["count_lines"][words.index(b"the")] == 5489
    assert len(kat["records"]) >= 50
    for w, want in kat["records"].items():
        n = w.encode("latin-1")
        o, r = offsets_nocase(data, n), lines_nocase(data, n, 10)
        assert (len(o), len(r)) == (want["count"], want["lines"]), w
        assert hashlib.sha256(b"".join(struct.pack("<Q", x) for x in o)).hexdigest() == want["offsets_sha256"], w
        assert hashlib.sha256(b"".join(struct.pack("<3Q", *t) for t in r)).hexdigest() == want["records_sha256"], w
    whats = " ".join(c["what"] for c in kat["cases"])
    for topic in ("'@'", "'['", "'`'", "'{'", "0xC1", "0xDA", "empty needle", "not folded", "other case of the delimiter",
                  "holds the delimiter", "0x00", "0xFF", "overlapping"):
        assert topic in whats, topic
    for c in kat["cases"]:
        h, n = bytes.fromhex(c["haystack"]), bytes.fromhex(c["needle"])
        assert offsets_nocase(h, n) == c["offsets"], c["what"]
        assert lines_nocase(h, n, c["delimiter"]) == [tuple(r) for r in c["records"]], c["what"]


def test_tools_and_documents_know_the_calls():
    grep = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert '"-i"' in grep and "--ignore-case" in grep
    for rel in ("tools/fuzz_nocase.py", "tools/nocase_bench.py", "tests/golden/make_nocase_golden.py",
                "sliceslice-rs_amd/bindings/rust/hip_nocase.rs", "include/sliceslice_hip_nocase.h"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel
    tool = os.path.join(ROOT, "tools", "grep_hip.py")
    usage = subprocess.run([sys.executable, tool], capture_output=True, text=True)
    assert usage.returncode != 0 and "--ignore-case" in usage.stderr
    alone = subprocess.run([sys.executable, tool, "-i", "a", os.path.join(GOLDEN, "data", "words.txt")], capture_output=True, text=True)
    assert alone.returncode != 0 and "--count" in alone.stderr
    # several patterns go through the batched library, which has no folding form
    refused = subprocess.run([sys.executable, tool, "-i", "-e", "a", "-e", "b", os.path.join(GOLDEN, "data", "words.txt")],
                             capture_output=True, text=True)
    assert refused.returncode != 0 and "-i" in refused.stderr and "-e" in refused.stderr, refused
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.9" in design and "libsliceslice_hip_nocase.so" in open(os.path.join(ROOT, "README.md")).read()
