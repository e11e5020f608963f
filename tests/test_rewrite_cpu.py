"""CPU checks of the rewrite call (include/sliceslice_hip_rewrite.h): the header, the ctypes table and the Rust module agree symbol
by symbol; the eighteenth library stands on the runs one, in a mapping of its own, and no other build holds the call; the new
kernels use no private segment, spill no vector register and little LDS, and their source calls the run kernels' parts; the
refusals that need no device; the numpy rule the GPU tests use agrees with `re.sub`; tests/golden/rewrite_kat.json is what its
generator produces now; the per-workgroup offset identity against a direct count."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class, exported as _exported, header_prototypes, rust_prototypes
from test_classes_cpu import re_set, sets_of
from test_runs_cpu import QUANTIFIERS, RUNS, rule_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_rewrite_golden as G         # noqa: E402

REWRITE = ["ss_replace_runs_device"]


def rule_replace(data, set_words, text, min_len=1, max_len=None, delimiter=None):
    """THE RULE in numpy: (the output bytes, the number of selected runs).  What the GPU tests compare with."""
    data = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
    begin, end = rule_runs(data, set_words, min_len, max_len, delimiter)
    pieces, at = [], 0
    for b, e in zip(begin.tolist(), end.tolist()):
        pieces.append(data[at:b])
        pieces.append(bytes(text))
        at = e
    pieces.append(data[at:])
    return b"".join(pieces), int(begin.size)


# ---- header, ctypes table, Rust block, build ---------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_rewrite.h")
    assert sorted(c) == sorted(ss.searcher.REWRITE_ABI) == REWRITE
    assert c["ss_replace_runs_device"] == ("i32", ["ptr", "ptr", "usize", "i32", "ptr", "usize", "ptr", "ptr", "u64", "ptr", "ptr"])
    # the contract mirrors ss_replace_device: the same arguments behind the delimiter, by name
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_rewrite.h")).read()
    flat = " ".join(text.split())
    model = " ".join(open(os.path.join(ROOT, "include", "sliceslice_hip_disjoint.h")).read().split())
    mine = re.search(r"ss_replace_runs_device\(const ss_runs \*runs, const void \*d_haystack, size_t len, int delimiter, ([^;]*);", flat).group(1)
    theirs = re.search(r"ss_replace_device\(const ss_searcher \*s, const void \*d_haystack, size_t len, unsigned how, ([^;]*);", model).group(1)
    assert mine == theirs
    r = rust_prototypes("hip_rewrite.rs")
    assert r == c, (r, c)
    rust = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_rewrite.rs")).read()
    assert "pub const SS_REWRITE_MAX_TEXT: usize = 4096;" in rust and "use crate::hip_runs::ss_runs;" in rust
    assert re.search(r"#define SS_REWRITE_MAX_TEXT\s+4096\b", text) and ss.SS_REWRITE_MAX_TEXT == 4096
    for name, (res, args) in ss.searcher.REWRITE_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_rewrite.h":
            assert not set(c) & set(header_prototypes(h)), h
    assert '#include "sliceslice_hip_runs.h"' in text
    assert "hip_rewrite.rs" in open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "build.rs")).read()


def test_the_header_states_the_rule_the_refusals_and_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_rewrite.h")).read()
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).split())
    for said in ("THE RULE", "its Class, Run and Selected are that header's, word for word", "-1 (none) or a byte 0 .. 255",
                 "that byte is never a member in this call, even where the set holds it", "a run is cut at every delimiter",
                 "a delimiter is always copied", "the line calls' rule", r"`s/\s+/ /g` behave as sed does, line by line",
                 "the view with every selected run replaced by the `replacement_len` bytes of `replacement`",
                 "everything else is copied in order: non-members, and runs too short or too long to be selected",
                 "A replacement is not rescanned", "the number of selected runs", "what ss_count_runs_device returns",
                 "the count of the pattern with that byte taken out of its set",
                 "len - (sum of the selected runs' lengths) + count * replacement_len, in 64 bits",
                 're.sub(rb"(?<![C])[C]{min,max}(?![C])", replacement, view)', 're.sub(rb"[C]{min,}", replacement, view)',
                 "replacement_len == 0 deletes", "Bytes outside [0, len) are absent",
                 "no load touches a 16-byte block that holds no byte of the view", "HOST memory",
                 "*out_len and *count are always set on SS_OK", "If out_capacity < *out_len nothing is written and the call returns SS_OK",
                 "a NULL d_out with capacity 0 is the sizing call, ONE pass", "every byte of d_out[0, *out_len) is written exactly once",
                 "nothing at *out_len or beyond", "The call waits for the stream", "len == 0 gives 0, 0 with no launch",
                 "Refused with SS_ERR_ARGUMENT and a message, nothing written", "a NULL handle or result pointers",
                 "a NULL haystack with len > 0", "a delimiter outside -1 .. 255", "a set that is only the delimiter (nothing can match)",
                 "a NULL replacement with replacement_len > 0", "replacement_len > SS_REWRITE_MAX_TEXT", "a NULL d_out with out_capacity > 0",
                 "a d_out range that intersects the haystack's range", "an overflow of *out_len", "a capturing stream",
                 "a handle made on another device", "three 64-bit words, taken mod 2^64", "S = sum(e + 1) - sum(b)",
                 "open = rank_b - rank_e", "PS + open * P", "P - (PS + open * P) + rank_b * replacement_len", "prefix-XOR",
                 "keep = valid & ~inside", "ONE 16-byte store", "copied by the whole wave, one begin at a time",
                 "No waiting between workgroups, no atomic", "48 bytes per workgroup plus a constant, never per run",
                 "the output depends on the input alone", "Out of scope", "an async / capturable form", "back-references", "per-run texts",
                 "more than one item", "anchors", "batched forms", "a plain byte translate (`tr a-z A-Z`)"):
        assert said.lower() in flat.lower(), said


def test_the_eighteenth_library_stands_on_the_runs_one():
    b = _build()
    entry = b._lib("rewrite")
    assert entry["parent"] == "runs" and entry["sources"] == ["ss_rewrite.hip"]
    # a fifth mapping below the four that are pinned name by name, which are what they were
    assert list(b._REWRITE_LIBRARIES) == ["rewrite"] and b._REWRITE_LIBRARIES["rewrite"] is entry
    assert list(b._NEWEST_LIBRARIES) == ["runs"] and list(b._LATEST_LIBRARIES) == ["masked", "classes"]
    assert list(b._LATER_LIBRARIES) == ["output", "leftmost"] and "rewrite" not in b.LIBRARIES and len(b.LIBRARIES) == 12
    source = open(os.path.join(ROOT, "sliceslice-rs_amd", "_build.py")).read()
    assert source.index("_NEWEST_LIBRARIES = {") < source.index("_REWRITE_LIBRARIES = {") < source.index("def _lib(")
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_rewrite.so" == os.path.basename(b.rewrite_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_rewrite.json" == os.path.basename(b.rewrite_resources_path())
    assert callable(b.build_rewrite) and callable(b.rewrite_kernel_resources)
    assert "sliceslice-rs_amd/csrc/kernel_resources_rewrite.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("rewrite") == b._all_sources("runs") + ["ss_rewrite.hip"]
    for h in ("runs_handle.hpp", "rewrite_kernels.hpp", "rewrite_launch.hpp", os.path.join("..", "..", "include", "sliceslice_hip_rewrite.h")):
        assert h in b._HEADERS, h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index('b.build_library("runs", force=True, verbose=True)') < \
        entry_point.index('b.build_library("rewrite", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["rewrite"][0] is ss.searcher.REWRITE_ABI and ss.searcher._FEATURES["rewrite"][1] == "ss_replace_runs_device"
    product = ss.lib()
    assert not getattr(product, "has_rewrite")
    with ss.runs_build() as L:
        assert not L.has_rewrite and L.has_runs
    with ss.rewrite_build() as L:
        assert ss.lib() is L and L.has_rewrite and L.has_runs and L.has_classes and L.has_lines and ss.searcher._feature_lib(L, "rewrite") is L
    assert ss.lib() is product
    runs = _exported(b.build_runs())
    assert _exported(b.build_rewrite()) == sorted(runs + REWRITE) and set(RUNS) <= set(runs)
    assert not set(REWRITE) & set(runs) and not set(REWRITE) & set(_exported(ss.build()))
    for name in list(b.LIBRARIES) + list(b._LATER_LIBRARIES) + list(b._LATEST_LIBRARIES) + list(b._NEWEST_LIBRARIES):
        so = b.library_path_of(name)
        assert not os.path.exists(so) or not set(REWRITE) & set(_exported(so)), name


def test_the_handle_is_shared_and_the_kernels_call_the_run_kernels_parts():
    kernels = open(os.path.join(CSRC, "rewrite_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in kernels.splitlines())
    assert '#include "runs_kernels.hpp"' in kernels and '#include "runs_launch.hpp"' in open(os.path.join(CSRC, "rewrite_launch.hpp")).read()
    for called in ("masked_load<U>(", "runs_masks<U>(", "runs_select<U, true>(", "set_valid_bits(", "kSetU", "kSetTiles", "kSetPartBytes",
                   "wave_exclusive_sum(", "wave_sum(", "aligned(1)"):
        assert called in code, called
    assert "runs_members16" not in code and "runs_in_range4" not in code and "load_chunk" not in code       # called, not copied
    host = open(os.path.join(CSRC, "ss_rewrite.hip")).read()
    everything = code + "\n".join(l.split("//")[0] for l in host.splitlines())
    for banned in ("asm", "volatile", "__threadfence", "atomic", "hipMalloc"):
        assert banned not in everything, banned
    assert host.count("launch_set_prefix(") == 3 and "take_scratch(" in host and '#include "runs_handle.hpp"' in host
    # the handle and runs_args moved, whole, into the header both translation units include
    handle = open(os.path.join(CSRC, "runs_handle.hpp")).read()
    runs = open(os.path.join(CSRC, "ss_runs.hip")).read()
    assert "struct ss_runs {" in handle and "inline int runs_args(" in handle and '#include "runs_handle.hpp"' in runs
    assert "struct ss_runs {" not in runs and "int runs_args(" not in runs and "struct ss_runs {" not in host


def test_the_new_kernels_use_no_private_segment_spill_nothing_and_little_lds():
    rows = {r["name"]: r for r in _build().rewrite_kernel_resources() if r["tu"] == "ss_rewrite.hip"}
    names = sorted(rows)
    assert len(names) == 2 and all("ss::runs_replace_kernel" in n for n in names), names
    for name, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r.get("agprs", 0) == 0, (name, r)
        assert r["lds_bytes"] <= 16 * 1024, (name, r)


def test_every_other_build_refuses_and_names_the_build():
    message = ss.searcher._FEATURES["rewrite"][2]
    assert "ss.rewrite_build()" in message and "libsliceslice_hip_rewrite.so" in message

    class Elsewhere(ss.RunPattern):                 # a pattern of a build without the call; no handle, so nothing is freed
        def __init__(self, L):
            self._h, self._L, self.min_len, self.max_len = None, L, 1, None

    with ss.runs_build() as L:
        other = Elsewhere(L)
    for call in (lambda p: p.replace(b"abc", b"x"), lambda p: p.replace_into(b"abc", b"x", None), lambda p: p.delete(b"abc")):
        for pattern in (other, Elsewhere(ss.lib())):
            with pytest.raises(ss.SlicesliceError, match=r"ss\.rewrite_build\(\)") as e:
                call(pattern)
            assert e.value.code == ss.SS_ERR_ARGUMENT


def test_the_refusals_that_need_no_device_leave_the_results_alone():
    with ss.rewrite_build() as L:
        handle = ctypes.create_string_buffer(512)               # never read: every refusal below comes before the handle is looked at
        h = ctypes.cast(handle, ctypes.c_void_p)
        text = ctypes.create_string_buffer(b"x" * 5000)
        out_len, count = ctypes.c_uint64(77), ctypes.c_uint64(78)
        ol, c = ctypes.byref(out_len), ctypes.byref(count)
        for args, said in (((None, None, 0, -1, text, 1, None, None, 0, ol, c), "runs is NULL"),
                           ((h, None, 0, -1, text, 1, None, None, 0, None, c), "NULL"),
                           ((h, None, 0, -1, text, 1, None, None, 0, ol, None), "NULL"),
                           ((h, None, 0, -2, text, 1, None, None, 0, ol, c), "delimiter -2"),
                           ((h, None, 0, 256, text, 1, None, None, 0, ol, c), "delimiter 256"),
                           ((h, None, 0, -1, text, 4097, None, None, 0, ol, c), "SS_REWRITE_MAX_TEXT"),
                           ((h, None, 0, -1, None, 1, None, None, 0, ol, c), "replacement is NULL"),
                           ((h, None, 0, -1, text, 1, None, None, 5, ol, c), "d_out is NULL")):
            assert L.ss_replace_runs_device(*args) == ss.SS_ERR_ARGUMENT, said
            assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
            assert (out_len.value, count.value) == (77, 78), said


# ---- the rule and the fixture ------------------------------------------------------------------------------------------------------
def test_the_numpy_rule_agrees_with_re_sub_on_random_data():
    rng = np.random.default_rng(12)
    for item in (r"[ab]", r"\w", r"[^\n]", r"a", r".", r"[a\n]"):
        words = sets_of(re_set(item))[0]
        for alphabet in (b"ab", b"aab\n", b"ab_ \n\xe9"):
            data = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), 1500).tobytes()
            for quantifier, lo, hi in QUANTIFIERS:
                for text in (b"", b"N", b"<a_b>"):
                    assert rule_replace(data, words, text, lo, hi) == G.sub(data, item, quantifier, text), (item, quantifier, text)
                    if hi is None:                          # with no maximum: exactly re.sub of [C]{min,}
                        assert rule_replace(data, words, text, lo, hi)[0] == re.sub(item.encode() + b"{%d,}" % lo, lambda m: text, data, flags=re.S)
                    for delimiter in (10, ord("a")):        # \n, and a member of most of the sets
                        assert rule_replace(data, words, text, lo, hi, delimiter) == G.sub(data, item, quantifier, text, delimiter), \
                            (item, quantifier, text, delimiter)
    full = np.full(4, ~np.uint64(0))
    assert rule_replace(b"", full, b"x") == (b"", 0) and rule_replace(b"abc", full, b"x") == (b"x", 1)
    assert rule_replace(b"ab\n\ncd", full, b"-", 2, None, 10) == (b"-\n\n-", 2) and rule_replace(b"abc", full, b"") == (b"", 1)


def test_the_fixture_is_what_the_generator_gives_and_holds_the_issues_numbers():
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    kat = json.load(open(os.path.join(GOLDEN, "rewrite_kat.json")))
    assert kat == json.loads(json.dumps(G.make(data)))
    assert os.path.getsize(os.path.join(GOLDEN, "rewrite_kat.json")) < 32768 and kat["bytes"] == len(data) == 857425
    rows = [(c["pattern"], c["text"], c["delimiter"], c["count"], c["out_len"]) for c in kat["cases"]]
    assert rows == [(" {2,}", " ", None, 18778, 732244), ("[0-9]+", "N", None, 13677, 848426), ("[0-9]{3}", "<num>", None, 363, 858151),
                    (r"\s+", "", None, 119666, 601248), (r"\w{2,5}", "", None, 73067, 626760), (r"[^\n]{80,}", "...", None, 163, 834351),
                    (r"\w+", "", None, 119587, 336932), (r"\s+", " ", 10, 110142, 732244)]
    by_name = {c["name"]: c for c in kat["cases"]}
    assert by_name[G.SAME_OUTPUT[0]]["sha256"] == by_name[G.SAME_OUTPUT[1]]["sha256"] and "the same bytes" in kat["outputs"]
    import hashlib
    with ss.runs_build():
        for c in kat["cases"]:
            words, lo, hi = ss.parse_runs(c["pattern"])
            out, count = rule_replace(data, words, c["text"].encode("latin-1"), lo, hi, c["delimiter"])
            assert (count, len(out), hashlib.sha256(out).hexdigest()) == (c["count"], c["out_len"], c["sha256"]), c["name"]
            assert out[:G.KEEP].hex() == c["first"] and out[-G.KEEP:].hex() == c["last"], c["name"]


def test_the_per_workgroup_offset_identity_against_a_direct_count():
    """P - (PS + open * P) + rank_b * t is the number of output bytes in front of view position P, for parts of 37 bytes, with every
    sum taken mod 2^64 as the kernels take them."""
    rng = np.random.default_rng(13)
    part, mask = 37, (1 << 64) - 1
    for trial in range(200):
        n = int(rng.integers(1, 400))
        inside = np.zeros(n + 1, dtype=bool)
        begins, ends, at = [], [], int(rng.integers(0, 5))
        while at < n:
            length = int(rng.choice([1, 2, 3, 36, 37, 38, 80, 200]))
            b, e = at, min(n, at + length)
            begins.append(b)
            ends.append(e - 1)                              # the run's last byte: where the kernels see its end
            inside[b:e] = True
            at = e + int(rng.integers(1, 50))
        begins, ends = np.array(begins, dtype=np.int64), np.array(ends, dtype=np.int64)
        for t in (0, 1, 5, 4096):
            rank_b = rank_e = ps = 0
            for P in range(0, n, part):
                open_ = (rank_b - rank_e) & mask
                assert open_ in (0, 1) and open_ == int(P > 0 and inside[P - 1] and inside[P] and not (begins == P).any())
                got = (P - (ps + open_ * P) + rank_b * t) & mask
                want = int((~inside[:P]).sum()) + int((begins < P).sum()) * t
                assert got == want, (trial, P, t)
                mine_b, mine_e = begins[(begins >= P) & (begins < P + part)], ends[(ends >= P) & (ends < P + part)]
                rank_b, rank_e = rank_b + mine_b.size, rank_e + mine_e.size
                ps = (ps + int((mine_e + 1).sum()) - int(mine_b.sum())) & mask
            assert rank_b == rank_e and ps == int(inside.sum())
