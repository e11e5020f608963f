"""CPU checks of the batched every-occurrence calls (include/sliceslice_hip_matches_batched.h): the header, the ctypes table and the
Rust module agree symbol by symbol; libsliceslice_hip_matches_batched.so exports exactly the three headers' functions while the
product and the matches library export none of the new two; the shared objects are the same objects (their kernels' rows in the
new library's resource record equal the other records' rows); the new kernels meet the scan kernels' bar; Python refuses outside
matches_batched_build()."""
import json
import os
import re

import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class as norm, exported as _exported, header_prototypes, rust_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "sliceslice_hip_matches_batched.h"


def test_header_ctypes_and_rust_agree():
    c = header_prototypes(HEADER)
    assert sorted(c) == sorted(ss.searcher.MATCHES_BATCHED_ABI) == ["ss_count_batched", "ss_find_all_batched"]
    assert c["ss_count_batched"] == ("i32", ["ptr"] * 6 + ["usize", "ptr", "ptr"])
    assert c["ss_find_all_batched"] == ("i32", ["ptr"] * 6 + ["usize", "ptr", "ptr", "ptr", "ptr", "u64", "ptr"])
    r = rust_prototypes("hip_matches_batched.rs")
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.MATCHES_BATCHED_ABI.items():
        got = (norm(res), [norm(a) for a in args])
        want = c[name]
        assert [a.replace("usize", "u64") for a in got[1]] == [a.replace("usize", "u64") for a in want[1]] and got[0] == want[0], name
    # the ranges go in exactly as in ss_search_batched (which has a `position` in front of `count`)
    sb = header_prototypes()["ss_search_batched"]
    assert c["ss_count_batched"][1][:6] == sb[1][:6] and sb[1][7] == "usize"
    # none of it is in the other headers
    assert not set(c) & (set(header_prototypes()) | set(header_prototypes("sliceslice_hip_matches.h")))


def test_the_new_library_exports_three_headers_and_the_others_none_of_the_new_two():
    b = _build()
    new = list(ss.searcher.MATCHES_BATCHED_ABI)
    assert not any(n in _exported(ss.build()) for n in new)
    assert not any(n in _exported(b.build_matches()) for n in new)
    both = sorted(list(header_prototypes()) + list(header_prototypes("sliceslice_hip_matches.h")) + list(header_prototypes(HEADER)))
    assert _exported(b.build_matches_batched()) == both


def test_the_shared_objects_are_the_same_objects():
    """The rows of the product's and the matches library's kernels inside kernel_resources_matches_batched.json equal the rows of
    kernel_resources.json / kernel_resources_matches.json built from the same tree."""
    b = _build()
    rows = b.matches_batched_kernel_resources()
    product = b.kernel_resources()
    matches = b.matches_kernel_resources()
    own = [r for r in rows if r["tu"] in ("ss_matches_batched.hip", "scan_inst_all_batched.hip")]
    shared = [r for r in rows if r not in own]
    assert shared == matches and matches[:len(product)] == product and len(product) == 37
    assert own and all(r["tu"] == "scan_inst_all_batched.hip" for r in own)


def test_the_new_kernels_meet_the_bar():
    rows = [r for r in _build().matches_batched_kernel_resources() if r["tu"] == "scan_inst_all_batched.hip"]
    scans = {}
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r             # every kernel of the unit, helpers included
        m = re.match(r"void ss::scan_all_batched_kernel<(true|false)>", r["name"])
        if not m:
            continue
        scans[m.group(1)] = r
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128, r
        assert r.get("lds_bytes", 0) <= 1024 + 4 * 2048, r                               # 1 KiB + the four waves' needle slices
    assert sorted(scans) == ["false", "true"]                                            # count passes, emit pass
    # spilled scalar registers (written at kernel entry, read back on tiles with candidates): what the build records today
    assert scans["false"]["sgpr_spills"] <= 45 and scans["true"]["sgpr_spills"] <= 58, (scans["false"]["sgpr_spills"], scans["true"]["sgpr_spills"])
    # the unit holds the kernels it defines and nothing else: batch_cold_kernel, which it launches too, lives in ss_batched.hip
    names = sorted(re.sub(r"^void ", "", r["name"]).split("(")[0] for r in rows)
    assert names == sorted(["ss::batch_all_plan_kernel", "ss::prefix_kernel<unsigned long>", "ss::batch_rows_kernel",
                            "ss::scan_all_batched_kernel<true>", "ss::scan_all_batched_kernel<false>"]), names


def test_python_refuses_outside_the_new_build():
    assert not getattr(ss.lib(), "has_matches_batched", False)
    for fn in (ss.count_batched, ss.find_all_batched):
        with pytest.raises(ss.SlicesliceError, match="matches_batched_build"):
            fn(None, None, None, None)
    with ss.matches_build():
        with pytest.raises(ss.SlicesliceError, match="matches_batched_build"):
            ss.count_batched(None, None, None, None)


def test_tools_know_the_batched_forms():
    """(what grep_hip.py prints for several patterns is checked on the GPU: tests/test_gpu_matches_batched.py)"""
    grep = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert "count_batched" in grep and '"-f"' in grep
    assert "--batched" in open(os.path.join(ROOT, "tools", "matches_bench.py")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "fuzz_matches_batched.py"))
