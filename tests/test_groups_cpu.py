"""CPU checks of the grouping calls (include/sliceslice_hip_groups.h): `rule_groups`, the restatement of THE RULE that the GPU tests
import, against hand-written cases and against the fixture tests/golden/groups_kat.json; the twentieth library stands on the fields
one, in a mapping of its own; the header, the ctypes table, the Rust module and the library's exports agree symbol by symbol; the
kernels' resources; the refusals that need no device; ss_groups_scratch_bytes against the header's formula."""
import ctypes
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
CSRC = os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_groups_golden as G          # noqa: E402

GROUPS = ["ss_group_lines_device", "ss_group_ranges_device", "ss_group_runs_device", "ss_groups_scratch_bytes"]
NOCASE, WEAK_HASH = 1, 2
MAX_RANGES = 2 ** 32 - 2


def rule_groups(view, begin, end, fold=False):
    """THE RULE in Python: (first, count, group) int64 arrays.  The key of range k is view[b:e] with e = min(end, len) and
    b = min(begin, e) - the clamp of the gather call - folded where asked; groups are numbered in order of their first member."""
    data = bytes(view) if not isinstance(view, np.ndarray) else view.tobytes()
    n = len(data)
    index, first, count, group = {}, [], [], []
    for k, (b, e) in enumerate(zip(np.asarray(begin, dtype=np.uint64).tolist(), np.asarray(end, dtype=np.uint64).tolist())):
        e = min(e, n)
        b = min(b, e)
        key = data[b:e].lower() if fold else data[b:e]
        j = index.setdefault(key, len(first))
        if j == len(first):
            first.append(k)
            count.append(0)
        count[j] += 1
        group.append(j)
    return np.array(first, dtype=np.int64), np.array(count, dtype=np.int64), np.array(group, dtype=np.int64)


def table_size(n):
    """the slots of the table of a call over n ranges, as the header says"""
    if n == 0:
        return 0
    t = 2
    while t < 2 * n and t < 2 ** 32:
        t *= 2
    return t


def scratch_bytes(n):
    """the header's formula"""
    return 32 + 12 * n + 8 * table_size(n) + 12 * ((n + 4095) // 4096)


def _rows(view, ranges, fold=False):
    f, c, g = rule_groups(view, [r[0] for r in ranges], [r[1] for r in ranges], fold)
    return f.tolist(), c.tolist(), g.tolist()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_written_cases():
    view = b"the cat The cat"
    words = [(0, 3), (4, 7), (8, 11), (12, 15)]
    assert _rows(view, words) == ([0, 1, 2], [1, 2, 1], [0, 1, 2, 1])
    assert _rows(view, words, True) == ([0, 1], [2, 2], [0, 1, 0, 1])
    # no ranges, one range, the same range twice, equal bytes at different places
    assert _rows(view, []) == ([], [], [])
    assert _rows(view, [(4, 7)]) == ([0], [1], [0])
    assert _rows(view, [(4, 7), (4, 7), (12, 15)]) == ([0], [3], [0, 0, 0])
    # descending order of the ranges: groups are numbered by their first member in the LIST
    assert _rows(view, words[::-1]) == ([0, 1, 3], [2, 1, 1], [0, 1, 0, 2])
    # overlapping ranges; keys that are prefixes of each other are different keys
    assert _rows(b"aaaa", [(0, 1), (0, 2), (1, 3), (2, 4), (0, 4), (3, 4)]) == ([0, 1, 4], [2, 3, 1], [0, 1, 1, 1, 2, 0])
    # all empty keys are one group: empty at 0, at len, beyond the view, and a descending range
    assert _rows(b"abc", [(0, 0), (3, 3), (7, 9), (2, 1), (1, 2), (9, 2)]) == ([0, 4], [5, 1], [0, 0, 0, 0, 1, 0])
    # the clamp: an end beyond the view is the view's end
    assert _rows(b"abcab", [(3, 99), (0, 2), (3, 5)]) == ([0], [3], [0, 0, 0])
    # only 'A' .. 'Z' fold: '@' and '`', '[' and '{' stay apart, and so do bytes with bit 7
    view = b"@`[{\xc1\xe1Aa"
    assert _rows(view, [(k, k + 1) for k in range(8)], True) == ([0, 1, 2, 3, 4, 5, 6], [1, 1, 1, 1, 1, 1, 2], [0, 1, 2, 3, 4, 5, 6, 6])
    assert _rows(view, [(k, k + 1) for k in range(8)], False)[0] == list(range(8))


def test_the_fixture_is_what_the_generator_gives_and_the_rule_reproduces_its_rows():
    data = open(os.path.join(GOLDEN, "data", "i386.txt"), "rb").read()
    kat = json.load(open(os.path.join(GOLDEN, "groups_kat.json")))
    assert kat == json.loads(json.dumps(G.make(data)))
    assert os.path.getsize(os.path.join(GOLDEN, "groups_kat.json")) < 32768 and kat["bytes"] == len(data) == 857425
    assert [(c["name"], c["pattern"], c["folded"]) for c in kat["cases"]] == \
        [("word", r"\w+", False), ("word_folded", r"\w+", True), ("digits", "[0-9]+", False), ("nonspace", r"\S+", False),
         ("lines", None, False), ("lines_folded", None, True)]
    by = {c["name"]: c for c in kat["cases"]}
    assert (by["word"]["keys"], by["word"]["groups"], by["word_folded"]["groups"]) == (119587, 5153, 3974)
    assert by["word"]["top"] == ["the", 13, 6524] and (by["lines"]["keys"], by["lines"]["groups"]) == (20854, 12616)
    for c in kat["cases"]:
        spans = G.ranges(data, c["pattern"].encode() if c["pattern"] else None)
        first, count, group = rule_groups(data, [s[0] for s in spans], [s[1] for s in spans], c["folded"])
        assert (len(spans), first.size) == (c["keys"], c["groups"]), c["name"]
        assert int(count.sum()) == c["keys"] and (group[first] == np.arange(first.size)).all() and (np.diff(first) > 0).all(), c["name"]
        keys = [data[spans[k][0]:spans[k][1]] for k in first.tolist()]
        if c["folded"]:
            keys = [k.lower() for k in keys]
        table = list(zip(keys, first.tolist(), count.tolist()))
        assert G.digest(table) == c["sha256"], c["name"]
        show = [[k.decode("latin-1"), f, n] for k, f, n in table]
        assert show[:40] == c["head"] and show[-5:] == c["tail"] and c["top"] in show, c["name"]


# ---- header, ctypes table, Rust block, build ---------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_groups.h")
    assert sorted(c) == sorted(ss.searcher.GROUPS_ABI) == GROUPS
    assert c["ss_group_ranges_device"] == ("i32", ["ptr", "usize", "ptr", "ptr", "u64", "u32", "ptr", "ptr", "ptr", "u64", "ptr", "ptr"])
    assert c["ss_group_runs_device"] == ("i32", ["ptr", "ptr", "usize", "u32", "ptr", "ptr", "ptr", "ptr", "u64", "ptr", "ptr"])
    assert c["ss_group_lines_device"] == ("i32", ["ptr", "usize", "i32", "u32", "ptr", "ptr", "ptr", "ptr", "ptr", "u64", "ptr", "ptr"])
    assert c["ss_groups_scratch_bytes"] == ("i32", ["u64", "ptr"])
    r = rust_prototypes("hip_groups.rs")
    assert r == c, (r, c)
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_groups.h")).read()
    rust = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip_groups.rs")).read()
    for name, value, spelled in (("SS_GROUPS_NOCASE", 1, "c_uint = 1"), ("SS_GROUPS_WEAK_HASH", 2, "c_uint = 2")):
        assert re.search(r"#define %s\s+%du\b" % (name, value), text) and getattr(ss, name) == value and "pub const %s: %s;" % (name, spelled) in rust
    assert re.search(r"#define SS_GROUPS_MAX_RANGES\s+0xfffffffeull\b", text) and ss.GROUPS_MAX_RANGES == 0xfffffffe == MAX_RANGES
    assert "pub const SS_GROUPS_MAX_RANGES: u64 = 0xfffffffe;" in rust
    assert re.search(r"#define SS_GROUPS_BLOCK\s+4096\b", text) and ss.GROUPS_BLOCK == 4096 and "pub const SS_GROUPS_BLOCK: usize = 4096;" in rust
    assert re.search(r"#define SS_GROUPS_LDS_BYTES\s+24576\b", text) and ss.GROUPS_LDS_BYTES == 24576 and "pub const SS_GROUPS_LDS_BYTES: usize = 24576;" in rust
    assert re.search(r"#define SS_GROUPS_LANE_MAX\s+128\b", text) and ss.GROUPS_LANE_MAX == 128 and "pub const SS_GROUPS_LANE_MAX: usize = 128;" in rust
    launch = open(os.path.join(CSRC, "groups_launch.hpp")).read()
    assert "constexpr int kGroupsBlock = 4096;" in launch and "constexpr int kGroupsLaneMax = 128;" in launch
    assert "constexpr uint32_t kGroupsEmpty = 0xffffffffu;" in launch and "constexpr int kGroupsLdsBits = 11;" in launch
    for name, (res, args) in ss.searcher.GROUPS_ABI.items():
        assert (ctypes_class(res), [ctypes_class(a) for a in args]) == (c[name][0], [a.replace("usize", "u64") for a in c[name][1]]), name
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "sliceslice_hip_groups.h":
            assert not set(c) & set(header_prototypes(h)), h
    assert '#include "sliceslice_hip_fields.h"' in text
    assert "hip_groups.rs" in open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "build.rs")).read()
    for name in ("groups_build", "group_ranges", "group_ranges_into", "group_lines", "groups_scratch_bytes"):
        assert callable(getattr(ss, name)), name
    assert callable(ss.RunPattern.groups) and callable(ss.RunPattern.most_common)


def test_the_header_states_the_rule_the_refusals_and_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "include", "sliceslice_hip_groups.h")).read()
    flat = " ".join(re.sub(r"^ \*", "", text, flags=re.M).split())
    for said in ("THE RULE", "the key of range k is the bytes hay[begin[k], end[k])", "two 64-bit device arrays", "they may overlap, repeat and descend",
                 "clamped to the view exactly as ss_gather_ranges_device", "With SS_GROUPS_NOCASE every key byte goes through the ASCII fold",
                 "before it is hashed or compared", "the haystack is not copied", "the same length and the same bytes",
                 "All empty keys are equal to each other", "the classes of equal keys", "in order of its FIRST member, the smallest k",
                 "the order of a Python dict or Counter filled in input order", "first[j] is that k", "count[j] is the number of members",
                 "group[k] is the j of range k", "a function of the input alone", "bit-identical from run to run",
                 "n <= SS_GROUPS_MAX_RANGES (2^32 - 2)", "slots and indices are 32-bit inside",
                 "no load touches a 16-byte block that holds no byte of the view", "d_group, if given, holds all n entries",
                 "*groups is always the full number", "n == 0 is allowed and gives 0 groups", "Waits for the stream",
                 "the FIRST token of group j", "prints the vocabulary without a host copy", "empty lines are included",
                 "the last line counts only if it has bytes", "the number of the first line of group j", "SS_FIELDS_KEEP_SHORT",
                 "HOST ONLY", "32 + 12 n + 8 T + 12 B bytes", "the smallest power of two >= 2 n", "8 bytes of hash and 4 bytes of slot number per range",
                 "4 bytes of slot and 4 bytes of counter per slot", "28 to 44 bytes per range", "16 bytes per range more", "FOR TESTS",
                 "the hash is replaced by length & 3", "one of four probe chains", "The results are the same with and without it",
                 "Refused with SS_ERR_ARGUMENT and a message, nothing written and the results left alone", "NULL result pointers",
                 "NULL arrays with n > 0", "a NULL haystack with len > 0", "an unknown flag", "the message names the limit",
                 "a delimiter that is no byte", "a handle made on another device", "a capturing stream", "no sort and no list of candidate pairs",
                 "no key is hashed twice", "the whole wave on one key above that", "open addressing with linear probing",
                 "stored hashes first, bytes only when they agree", "an atomic min", "no lane ever waits for another",
                 "slots never become empty again", "a ballot loop over equal slots", "a workgroup-private LDS table keyed by slot",
                 "SS_GROUPS_LDS_BYTES = 24,576 bytes", "flushed with one add per entry", "never more than 2^32", "THE POOL KEEPS WHAT IT TOOK",
                 "never frees one", "a last pass writes group[k]",
                 "Out of scope", "sorting the groups by key bytes", "grouping by a field of each line", "an async or capturable form",
                 "batched forms", "multi-GPU", "folding beyond ASCII", "more than 2^32 - 2 ranges"):
        assert said.lower() in flat.lower(), said
    kernels = open(os.path.join(CSRC, "groups_kernels.hpp")).read()
    assert "WHY THE LOOP CANNOT HANG" in kernels and "WHY 128" in kernels and "NOBODY HAS MEASURED" in kernels


def test_the_twentieth_library_stands_on_the_fields_one():
    b = _build()
    entry = b._lib("groups")
    assert entry["parent"] == "fields" and entry["sources"] == ["ss_groups.hip"]
    # a seventh mapping below the six that are pinned name by name, which are what they were
    assert list(b._GROUPS_LIBRARIES) == ["groups"] and b._GROUPS_LIBRARIES["groups"] is entry
    assert list(b._FIELDS_LIBRARIES) == ["fields"] and list(b._REWRITE_LIBRARIES) == ["rewrite"] and list(b._NEWEST_LIBRARIES) == ["runs"]
    assert list(b._LATEST_LIBRARIES) == ["masked", "classes"] and list(b._LATER_LIBRARIES) == ["output", "leftmost"]
    assert "groups" not in b.LIBRARIES and len(b.LIBRARIES) == 12
    for name, parent, sources in (("fields", "rewrite", ["ss_fields.hip"]), ("rewrite", "runs", ["ss_rewrite.hip"]), ("runs", "classes", ["ss_runs.hip"]),
                                  ("classes", "masked", ["ss_classes.hip"]), ("masked", "leftmost", ["ss_masked.hip"]),
                                  ("leftmost", "output", ["ss_leftmost.hip"]), ("output", "disjoint", ["ss_output.hip"])):
        assert (b._lib(name)["parent"], b._lib(name)["sources"]) == (parent, sources), name
    source = open(os.path.join(ROOT, "sliceslice-rs_amd", "_build.py")).read()
    assert source.index("_FIELDS_LIBRARIES = {") < source.index("_GROUPS_LIBRARIES = {") < source.index("def _lib(")
    assert os.path.basename(entry["so"]) == "libsliceslice_hip_groups.so" == os.path.basename(b.groups_library_path())
    assert os.path.basename(entry["resources"]) == "kernel_resources_groups.json" == os.path.basename(b.groups_resources_path())
    assert callable(b.build_groups) and callable(b.groups_kernel_resources)
    assert "sliceslice-rs_amd/csrc/kernel_resources_groups.json" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert b._all_sources("groups") == b._all_sources("fields") + ["ss_groups.hip"]
    assert b._all_sources("groups")[-3:] == ["ss_rewrite.hip", "ss_fields.hip", "ss_groups.hip"]
    for h in ("groups_kernels.hpp", "groups_launch.hpp", "groups_host.hpp", os.path.join("..", "..", "include", "sliceslice_hip_groups.h")):
        assert h in b._HEADERS, h
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry_point.index('b.build_library("fields", force=True, verbose=True)') < \
        entry_point.index('b.build_library("groups", force=True, verbose=True)') < entry_point.index("b.build_tuning(")
    assert ss.searcher._FEATURES["groups"][0] is ss.searcher.GROUPS_ABI and ss.searcher._FEATURES["groups"][1] == "ss_group_ranges_device"
    product = ss.lib()
    assert not getattr(product, "has_groups")
    with ss.fields_build() as L:
        assert not L.has_groups and L.has_fields
    with ss.groups_build() as L:
        assert ss.lib() is L and L.has_groups and L.has_fields and L.has_rewrite and L.has_runs and L.has_output and L.has_lines
        assert ss.searcher._feature_lib(L, "groups") is L
    assert ss.lib() is product


def test_the_headers_functions_are_the_librarys_exported_additions():
    b = _build()
    fields = _exported(b.build_fields())
    assert _exported(b.build_groups()) == sorted(fields + GROUPS)
    assert not set(GROUPS) & set(fields) and not set(GROUPS) & set(_exported(ss.build()))
    for name in (list(b.LIBRARIES) + list(b._LATER_LIBRARIES) + list(b._LATEST_LIBRARIES) + list(b._NEWEST_LIBRARIES) + list(b._REWRITE_LIBRARIES) +
                 list(b._FIELDS_LIBRARIES)):
        so = b.library_path_of(name)
        assert not os.path.exists(so) or not set(GROUPS) & set(_exported(so)), name


def test_the_new_kernels_use_no_private_segment_no_spill_and_little_lds():
    rows = {r["name"]: r for r in _build().groups_kernel_resources() if r["tu"] == "ss_groups.hip"}
    names = sorted(rows)
    assert len(names) == 8, names
    for kernel, copies in (("ss::groups_hash_kernel<", 2), ("ss::groups_insert_kernel<", 2), ("ss::groups_count_kernel(", 1),
                           ("ss::groups_rank_kernel<", 2), ("ss::groups_number_kernel(", 1)):
        assert sum(kernel in n for n in names) == copies, (kernel, names)
    for name, r in rows.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r.get("agprs", 0) == 0, (name, r)
        # the LDS count table is in: 2,048 entries of an 8-byte key and a 4-byte count in the count kernel, SS_GROUPS_LDS_BYTES;
        # everywhere else the only LDS is the four wave sums of the rank kernel
        assert r["lds_bytes"] == (ss.GROUPS_LDS_BYTES if "groups_count_kernel" in name else 16 if "groups_rank_kernel" in name else 0), (name, r)
        assert ss.GROUPS_LDS_BYTES == 2048 * 12 == 24576 and r["vgprs"] <= 128, (name, r)
    kernels = open(os.path.join(CSRC, "groups_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in kernels.splitlines())
    host = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "ss_groups.hip")).read().splitlines())
    for called in ("__hip_atomic_load(&a.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)", "__hip_atomic_compare_exchange_strong(",
                   "__hip_atomic_fetch_min(", "__hip_atomic_fetch_add(", "__builtin_amdgcn_ballot_w64(", "out_clamp(", "fold_ascii4("):
        assert called in code, called
    assert "launch_prefix(" in host and "take_scratch(" in host and "stream_is_capturing(" in host
    for banned in ("asm", "volatile", "__threadfence", "hipMalloc", "sort"):      # plain C++ atomics, leased scratch, no sort
        assert banned not in code + host, banned


def test_no_slot_number_is_the_empty_marker():
    """With 2^32 slots every 32-bit value is a slot number, the largest included, so no kernel may read a slot number as "none".  The
    marker kGroupsEmpty is a value of a table ENTRY, a member's index, and the largest index, SS_GROUPS_MAX_RANGES - 1, lies below it."""
    assert table_size(2 ** 30) == 2 ** 31 and table_size(2 ** 30 + 1) == 2 ** 32 == table_size(MAX_RANGES)
    largest_slot, empty = table_size(MAX_RANGES) - 1, 0xffffffff
    assert largest_slot == empty                          # ... which is why the marker cannot be a slot number
    assert MAX_RANGES - 1 < empty                         # the largest member index is no marker
    kernels = open(os.path.join(CSRC, "groups_kernels.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in kernels.splitlines())
    # the marker appears only where a table entry is read or swapped: in the insert kernel, against `v` and `seen`
    uses = [l.strip() for l in code.splitlines() if "kGroupsEmpty" in l]
    assert uses == ["uint32_t v = kGroupsEmpty;", "if (v == kGroupsEmpty) {", "uint32_t seen = kGroupsEmpty;"], uses
    for name in ("mine", "slots[r]", "a.slot[k]", "ls", " s "):
        assert not re.search(r"%s\s*[!=]=\s*kGroupsEmpty|kGroupsEmpty\s*[!=]=\s*%s" % (re.escape(name), re.escape(name)), code), name
    assert "uint32_t mine = 0;" in code and "A SLOT NUMBER IS NEVER A MARKER" in kernels
    # the LDS table of the count kernel marks an occupied entry by a bit ABOVE the slot number, not by a slot value
    assert "const unsigned long long key = (1ull << 32) | ls;" in code and "__shared__ unsigned long long s_key[kGroupsLdsSlots];" in code


def test_every_other_build_refuses_and_names_the_build():
    message = ss.searcher._FEATURES["groups"][2]
    assert "ss.groups_build()" in message and "libsliceslice_hip_groups.so" in message
    for context in (ss.fields_build, ss.runs_build):
        with context():
            for call in (lambda: ss.group_ranges(b"abc", [0], [1]), lambda: ss.group_lines(b"abc"), lambda: ss.groups_scratch_bytes(1)):
                with pytest.raises(ss.SlicesliceError, match=r"ss\.groups_build\(\)") as e:
                    call()
                assert e.value.code == ss.SS_ERR_ARGUMENT
    with pytest.raises(ss.SlicesliceError, match=r"ss\.groups_build\(\)"):
        ss.groups_scratch_bytes(1)


def test_the_refusals_that_need_no_device_leave_the_results_alone():
    with ss.groups_build() as L:
        a, b = ctypes.c_uint64(77), ctypes.c_uint64(78)
        ra, rb = ctypes.byref(a), ctypes.byref(b)
        some = ctypes.c_void_p(0x1000)                      # never read: every call below is refused before it looks at memory
        for args, said in (((None, 0, None, None, 0, 0, None, None, None, 0, None, None), "groups is NULL"),
                           ((None, 0, None, some, 3, 0, None, None, None, 0, None, ra), "d_begin or d_end is NULL and n is 3"),
                           ((None, 0, some, None, 3, 0, None, None, None, 0, None, ra), "d_begin or d_end is NULL and n is 3"),
                           ((None, 0, some, some, MAX_RANGES + 1, 0, None, None, None, 0, None, ra), "SS_GROUPS_MAX_RANGES = 4294967294"),
                           ((None, 0, some, some, 2 ** 63, 0, None, None, None, 0, None, ra), "2^32 - 2"),
                           ((None, 5, some, some, 3, 0, None, None, None, 0, None, ra), "haystack is NULL"),
                           ((None, 0, some, some, 3, 4, None, None, None, 0, None, ra), "unknown flag"),
                           ((None, 0, None, None, 0, 8, None, None, None, 0, None, ra), "unknown flag")):
            assert L.ss_group_ranges_device(*args) == ss.SS_ERR_ARGUMENT, said
            assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
            assert (a.value, b.value) == (77, 78), said
        handle = ctypes.create_string_buffer(512)
        h = ctypes.cast(handle, ctypes.c_void_p)
        for args, said in (((h, None, 0, 0, None, None, None, None, 0, None, rb), "groups or tokens is NULL"),
                           ((h, None, 0, 0, None, None, None, None, 0, ra, None), "groups or tokens is NULL"),
                           ((None, None, 0, 0, None, None, None, None, 0, ra, rb), "runs is NULL"),
                           ((h, None, 5, 0, None, None, None, None, 0, ra, rb), "haystack is NULL"),
                           ((h, None, 0, 4, None, None, None, None, 0, ra, rb), "unknown flag")):
            assert L.ss_group_runs_device(*args) == ss.SS_ERR_ARGUMENT, said
            assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
            assert (a.value, b.value) == (77, 78), said
        for args, said in (((None, 0, 10, 0, None, None, None, None, None, 0, None, rb), "groups or lines is NULL"),
                           ((None, 0, 10, 0, None, None, None, None, None, 0, ra, None), "groups or lines is NULL"),
                           ((None, 0, 256, 0, None, None, None, None, None, 0, ra, rb), "delimiter 256"),
                           ((None, 0, -1, 0, None, None, None, None, None, 0, ra, rb), "delimiter -1"),
                           ((None, 5, 10, 0, None, None, None, None, None, 0, ra, rb), "haystack is NULL"),
                           ((None, 0, 10, 16, None, None, None, None, None, 0, ra, rb), "unknown flag")):
            assert L.ss_group_lines_device(*args) == ss.SS_ERR_ARGUMENT, said
            assert said in L.ss_last_error().decode(), (said, L.ss_last_error())
            assert (a.value, b.value) == (77, 78), said


def test_scratch_bytes_is_the_headers_formula():
    assert [table_size(n) for n in (0, 1, 2, 3, 4096, 4097, 2 ** 31, 2 ** 31 + 1, MAX_RANGES)] == \
        [0, 2, 4, 8, 8192, 16384, 2 ** 32, 2 ** 32, 2 ** 32]
    with ss.groups_build() as L:
        for n in (0, 1, 2, 3, 4095, 4096, 4097, 119587, 2 ** 31, MAX_RANGES):
            assert ss.groups_scratch_bytes(n) == scratch_bytes(n), n
            assert not 1 <= n <= 2 ** 31 or 28 * n <= scratch_bytes(n) - 32 - 12 * ((n + 4095) // 4096) <= 44 * n, n
        assert ss.groups_scratch_bytes(0) == 32 and ss.groups_scratch_bytes(1) == 32 + 12 + 16 + 12
        assert ss.groups_scratch_bytes(4096) == 32 + 12 * 4096 + 8 * 8192 + 12
        out = ctypes.c_uint64(77)
        for n in (MAX_RANGES + 1, 2 ** 32, 2 ** 64 - 1):
            assert L.ss_groups_scratch_bytes(n, ctypes.byref(out)) == ss.SS_ERR_ARGUMENT and out.value == 77
            assert "SS_GROUPS_MAX_RANGES = 4294967294" in L.ss_last_error().decode()
            with pytest.raises(ss.SlicesliceError, match="2\\^32 - 2"):
                ss.groups_scratch_bytes(n)
        assert L.ss_groups_scratch_bytes(1, None) == ss.SS_ERR_ARGUMENT
