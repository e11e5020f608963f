"""CPU checks of the masked-pattern calls (include/sliceslice_hip_masked.h): the header, the ctypes table and the Rust module agree
symbol by symbol; the fifteenth library stands on the leftmost one and the product holds none of it; the new kernels use no private
segment and spill no vector register; ss_masked_parse_hex accepts and refuses what the header says, with the column;
ss_masked_choose_filter keeps its promises; the numpy rule the GPU tests use agrees with `re` on the fixture's cases, and
tests/golden/masked_kat.json is what its generator produces now."""
import json
import os
import re
import sys

import numpy as np
import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_masked_golden as G          # noqa: E402

MASKED = ["ss_masked_new", "ss_masked_free", "ss_masked_info", "ss_masked_parse_hex", "ss_masked_choose_filter", "ss_count_masked_device",
          "ss_count_masked_device_async", "ss_find_all_masked_device", "ss_count_lines_masked_device", "ss_find_lines_masked_device"]


def rule_offsets(data, value, mask):
    """THE RULE in numpy: every p in [0, len - n] with (hay[p + i] & mask[i]) == value[i] for all i.  What the GPU tests compare with."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n = len(value)
    if n == 0 or data.size < n:
        return np.zeros(0, dtype=np.int64)
    ok = np.ones(data.size - n + 1, dtype=bool)
    for i, (v, m) in enumerate(zip(value, mask)):
        if m:
            ok &= (data[i:data.size - n + 1 + i] & m) == (v & m)
    return np.flatnonzero(ok).astype(np.int64)


def rule_lines(data, value, mask, delimiter):
    """(begin, end, number) of the lines that hold an occurrence wholly inside them, as sliceslice_hip_lines.h lays records out:
    end is the delimiter's index (len for an unterminated last line), number counts from 1."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n, offs = len(value), rule_offsets(data, value, mask)
    delims = np.flatnonzero(data == delimiter).astype(np.int64)
    ends = np.append(delims, data.size) if (delims.size == 0 or delims[-1] != data.size - 1) and data.size else delims
    begins = np.concatenate([[0], delims + 1])[:ends.size]
    line = np.searchsorted(ends, offs, side="left")                 # the line of the occurrence's first byte
    inside = offs + n <= ends[np.minimum(line, ends.size - 1)] if ends.size else np.zeros(0, dtype=bool)
    sel = np.unique(line[inside])
    return begins[sel], ends[sel], sel + 1


# ---- header, ctypes table, Rust block, build ---------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_masked.h")
    assert sorted(c) == sorted(ss.searcher.MASKED_ABI) == sorted(MASKED)
    matches, lines = header_prototypes("sliceslice_hip_matches.h"), header_prototypes("sliceslice_hip_lines.h")
    # the argument lists of the model calls, argument for argument
    assert c["ss_count_masked_device"] == matches["ss_count_device"] and c["ss_count_masked_device_async"] == matches["ss_count_device_async"]
    assert c["ss_find_all_masked_device"] == matches["ss_find_all_device"]
    assert c["ss_count_lines_masked_device"] == lines["ss_count_lines_device"] and c["ss_find_lines_masked_device"] == lines["ss_find_lines_device"]
    assert c["ss_masked_new"] == ("i32", ["ptr", "ptr", "usize", "ptr"]) and c["ss_masked_free"] == ("void", ["ptr"])
    assert c["ss_masked_parse_hex"] == ("i32", ["ptr", "ptr", "ptr", "usize", "ptr"])
    assert c["ss_masked_choose_filter"] == ("i32", ["ptr", "ptr", "usize", "ptr", "ptr", "ptr"])
    r = rust_prototypes("hip_masked.rs")
    assert r == c, (r, c)
    rust = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_masked.rs")).read()
    assert "pub const SS_MASKED_MAX_LEN: usize = 4096;" in rust
    for name, (res, args) in ss.searcher.MASKED_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_masked.h":
            assert not set(c) & set(header_prototypes(h)), h
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_masked.h")).read()
    assert '#include "sliceslice_hip_leftmost.h"' in text
    assert re.search(r"#define SS_MASKED_MAX_LEN\s+4096", text) and ss.MASKED_MAX_LEN == 4096
    # the stats are eight 64-bit words in the order of the Python names
    body = re.search(r"typedef struct ss_masked_stats \{(.*?)\}", text, flags=re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]+);", body) for f in decl.split(",")]
    assert fields == list(ss.searcher.MASKED_STATS)
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).split())
    for said in ("THE RULE", "(hay[p + i] & mask[i]) == value[i]", "1 <= n <= SS_MASKED_MAX_LEN", "`value` is stored as value & mask",
                 "Occurrences overlap", "Bytes outside [0, len) are absent", "no load touches a 16-byte block that holds no byte of the view",
                 "64-bit", "len - n + 1", "`61 ?? 62` does not match \"a\\nb\"", "sliceslice_hip_lines.h's, word for word",
                 "A NULL mask means all 0xFF", "HOST ONLY", "offending column", "never chosen while any other exists",
                 "Refused with SS_ERR_ARGUMENT", "nothing written", "Out of scope", "variable-length jumps", "alternatives", "replace",
                 "regular expressions", "DESIGN.md 5.19"):
        assert said.lower() in flat.lower(), said


def test_the_fifteenth_library_stands_on_the_leftmost_one():
    b = _build()
    entry = b._lib("masked")
    assert entry["parent"] == "leftmost" and entry["sources"] == ["ss_masked.hip"] and "masked" not in b.LIBRARIES
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_masked.so" == os.path.basename(b.masked_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_masked.json" == os.path.basename(b.masked_resources_path())
    assert "sliceslice-rs_amd/csrc/kernel_resources_masked.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("masked") == b._all_sources("leftmost") + ["ss_masked.hip"]
    for h in ("masked_kernels.hpp", "masked_launch.hpp", os.path.join("..", "..", "include", "sliceslice_hip_masked.h")):
        assert h in b._HEADERS, h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index('b.build_library("leftmost", force=True, verbose=True)') < \
        entry_point.index('b.build_library("masked", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["masked"][0] is ss.searcher.MASKED_ABI and ss.searcher._FEATURES["masked"][1] == "ss_masked_new"
    product = ss.lib()
    assert not getattr(product, "has_masked")
    with ss.leftmost_build() as L:
        assert not L.has_masked
    with ss.masked_build() as L:
        assert ss.lib() is L and L.has_masked and L.has_leftmost and L.has_output and L.has_lines and ss.searcher._feature_lib(L, "masked") is L
    assert ss.lib() is product
    leftmost = _exported(b.build_leftmost())
    assert _exported(b.build_masked()) == sorted(leftmost + MASKED)
    assert not set(MASKED) & set(leftmost) and not set(MASKED) & set(_exported(ss.build()))


def test_the_product_refuses_and_names_the_build():
    message = ss.searcher._FEATURES["masked"][2]
    assert "ss.masked_build()" in message and "libsliceslice_hip_masked.so" in message
    assert not getattr(ss.lib(), "has_masked", False)
    for call in (lambda: ss.MaskedPattern(b"abc"), lambda: ss.MaskedPattern.from_hex("41 ??"), lambda: ss.MaskedPattern.from_bytes(b"x", True),
                 lambda: ss.parse_hex("41"), lambda: ss.masked_choose_filter(b"ab")):
        with pytest.raises(ss.SlicesliceError, match=r"ss\.masked_build\(\)") as e:
            call()
        assert e.value.code == ss.SS_ERR_ARGUMENT


def test_the_new_kernels_use_no_private_segment_and_spill_no_vector_register():
    rows = {r["name"]: r for r in _build().masked_kernel_resources() if r["tu"] == "ss_masked.hip"}
    names = sorted(rows)
    assert len(names) == 4 and all("ss::masked_all_kernel" in n or "ss::masked_lines_kernel" in n for n in names), names
    for name, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r.get("agprs", 0) == 0, (name, r)
        assert r["lds_bytes"] <= 8192 + 2048, (name, r)            # value / mask for 4,096 bytes and the wave slots


# ---- ss_masked_parse_hex -----------------------------------------------------------------------------------------------------------
def test_parse_hex_accepts_and_refuses_what_the_header_says():
    with ss.masked_build():
        assert ss.parse_hex("48 8b ?? 4?") == (bytes([0x48, 0x8B, 0x00, 0x40]), bytes([0xFF, 0xFF, 0x00, 0xF0]))
        assert ss.parse_hex("?F") == (b"\x0f", b"\x0f") and ss.parse_hex("??") == (b"\x00", b"\x00")
        assert ss.parse_hex("488B") == ss.parse_hex("48 8b") == ss.parse_hex("  48\t8B  ") == (b"\x48\x8b", b"\xff\xff")
        assert ss.parse_hex("aAbB") == (b"\xaa\xbb", b"\xff\xff")
        assert ss.parse_hex("") == (b"", b"") and ss.parse_hex("   ") == (b"", b"")
        for text in ("48 8b ?? 4?", "3? 3? 3?", "?0 ?d", "ff" * 300):
            assert ss.parse_hex(text) == G.parse_hex(" ".join(re.findall("..", text.replace(" ", "")))), text
        for text, column in (("48 8", 5), ("4 8", 2), ("48 xz", 4), ("48 8g", 5), ("[4-6]", 1), ("48|49", 3), ("4?,", 3), ("48 ?", 5), ("48\n49", 3)):
            with pytest.raises(ss.SlicesliceError, match=r"column %d\b" % column) as e:
                ss.parse_hex(text)
            assert e.value.code == ss.SS_ERR_ARGUMENT, text


# ---- ss_masked_choose_filter -------------------------------------------------------------------------------------------------------
def test_choose_filter_keeps_its_promises():
    rng = np.random.default_rng(7)
    with ss.masked_build():
        choose = ss.masked_choose_filter
        # never a 0x00 mask beside a non-zero one, d <= 16, both positions inside, deterministic
        for trial in range(300):
            n = int(rng.integers(1, 70))
            value = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            mask = bytes(int(rng.choice([0x00, 0x00, 0xFF, 0xF0, 0x0F, 0xDF, 0x01])) for _ in range(n))
            hist = rng.integers(0, 1 << 20, 256).astype(np.uint64) if trial % 3 == 0 else None
            a, d = choose(value, mask, hist)
            assert (a, d) == choose(value, mask, hist) and 0 <= d <= 16 and a + d < n, (value, mask)
            live = [i for i in range(n) if mask[i]]
            if live:
                assert mask[a] != 0 and mask[a + d] != 0, (value, mask, a, d)
                pair = any(0 < j - i <= 16 for i in live for j in live)
                assert (d != 0) == pair, (value, mask, a, d)
            else:
                assert (a, d) == (0, 0)
        # only one position has a mask, or the two are more than 16 apart
        assert choose(b"\0" * 9 + b"q" + b"\0" * 9, b"\0" * 9 + b"\xff" + b"\0" * 9) == (9, 0)
        value, mask = bytearray(40), bytearray(40)
        value[2], mask[2], value[19], mask[19] = ord("q"), 0xFF, ord("e"), 0xFF
        assert choose(bytes(value), bytes(mask)) == (2, 0)          # 17 apart: the cheaper one alone (q before e)
        value[18], mask[18] = ord("e"), 0xFF
        assert choose(bytes(value), bytes(mask)) == (2, 16)
        # z before e, and a full byte before a nibble of the same letter
        assert choose(b"eeze") == (0, 2) and choose(b"ezee") == (0, 1) and choose(b"zeee") == (0, 1)
        assert choose(b"eeeeez", None)[0] + choose(b"eeeeez", None)[1] == 5
        assert choose(b"zzz", b"\xf0\xff\xf0") in ((0, 1), (1, 1))
        # a NULL mask is all 0xFF
        assert choose(b"descriptor") == choose(b"descriptor", b"\xff" * 10)
        # the caller's histogram decides where it is given: 'z' made common, 'e' rare
        hist = np.full(256, 1000, dtype=np.uint64)
        hist[ord("z")], hist[ord("e")] = 10 ** 9, 1
        a, d = choose(b"zqqe", None, hist)
        assert a + d == 3 and a != 0
        for bad in (b"", b"x" * 4097):
            with pytest.raises(ss.SlicesliceError) as e:
                choose(bad)
            assert e.value.code == ss.SS_ERR_ARGUMENT


# ---- the rule and the fixture ------------------------------------------------------------------------------------------------------
def test_the_numpy_rule_agrees_with_re_and_the_fixture_is_what_the_generator_gives():
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    kat = json.load(open(os.path.join(GOLDEN, "masked_kat.json")))
    assert kat == json.loads(json.dumps(G.make(data)))
    assert os.path.getsize(os.path.join(GOLDEN, "masked_kat.json")) < 16384 and kat["bytes"] == len(data)
    by_name = {c["name"]: c for c in kat["cases"]}
    assert [c["name"] for c in kat["cases"]] == [c[0] for c in G.CASES]
    # the values the issue names, for orientation
    assert (by_name["descriptor_gaps"]["count"], by_name["descriptor_gaps"]["lines"]) == (355, 337)
    assert (by_name["t_any_e"]["count"], by_name["t_any_e"]["lines"]) == (7894, 5013)
    assert by_name["three_digit_nibbles"]["count"] == 3951 and by_name["intel_any_case"]["count"] == 44
    assert (by_name["dot_any_newline"]["count"], by_name["dot_any_newline"]["lines"]) == (1610, 0)
    assert by_name["one_wildcard"]["count"] == 857425
    arr = np.frombuffer(data, dtype=np.uint8)
    for c in kat["cases"]:
        value, mask = bytes.fromhex(c["value"]), bytes.fromhex(c["mask"])
        offs = rule_offsets(arr, value, mask)
        assert offs.size == c["count"], c["name"]
        if "offsets" in c:
            assert offs.tolist() == c["offsets"], c["name"]
        else:
            assert G.list_hash(offs.tolist()) == c["offsets_sha256"] and offs[:16].tolist() == c["first"] and offs[-16:].tolist() == c["last"], c["name"]
        begin, end, number = rule_lines(arr, value, mask, c["delimiter"])
        assert begin.size == c["lines"], c["name"]
    # the rule's corners: a wildcard that accepts the delimiter, the unterminated last line, an empty view
    v, m = G.parse_hex("61 ?? 62")
    assert rule_offsets(b"a\nb", v, m).tolist() == [0] and rule_lines(b"a\nb", v, m, 10)[0].size == 0
    assert [x.tolist() for x in rule_lines(b"xx\naxb", v, m, 10)] == [[3], [6], [2]]
    assert [x.tolist() for x in rule_lines(b"axb\n\naab\n", v, m, 10)] == [[0, 5], [3, 8], [1, 3]]
    assert rule_offsets(b"", v, m).size == 0 and rule_lines(b"", v, m, 10)[0].size == 0
