"""CPU checks of every-occurrence search (include/sliceslice_hip_matches.h): the header, the ctypes table and the Rust module agree
symbol by symbol; libsliceslice_hip_matches.so exports exactly the product header plus the matches header while the product library
exports none of it; the library's kernels meet the scan kernels' bar; the Python methods refuse outside matches_build()."""
import json
import os
import re

import pytest

import sliceslice_rs_amd as ss
from test_bindings_cpu import build_module as _build, ctypes_class as norm, exported as _exported, header_prototypes, rust_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_ctypes_and_rust_agree():
    c = header_prototypes("sliceslice_hip_matches.h")
    assert sorted(c) == sorted(ss.searcher.MATCHES_ABI) == ["ss_count_device", "ss_count_device_async", "ss_find_all_device"]
    assert c["ss_find_all_device"] == ("i32", ["ptr", "ptr", "usize", "ptr", "ptr", "u64", "ptr"])
    assert c["ss_count_device"] == ("i32", ["ptr", "ptr", "usize", "ptr", "ptr"])
    r = rust_prototypes("hip_matches.rs")
    assert r == c, (r, c)
    for name, (res, args) in ss.searcher.MATCHES_ABI.items():
        got = (norm(res), [norm(a) for a in args])
        want = c[name]
        assert [a.replace("usize", "u64") for a in got[1]] == [a.replace("usize", "u64") for a in want[1]] and got[0] == want[0], name
    # none of it is in the product's header
    assert not set(c) & set(header_prototypes())


def test_the_matches_library_exports_both_headers_and_the_product_neither():
    b = _build()
    product = _exported(ss.build())
    assert not any(n in product for n in ss.searcher.MATCHES_ABI)
    matches = _exported(b.build_matches())
    assert matches == sorted(list(header_prototypes()) + list(header_prototypes("sliceslice_hip_matches.h")))


def test_the_matches_kernels_meet_the_scan_kernels_bar():
    rows = _build().matches_kernel_resources()
    product = json.load(open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "kernel_resources.json")))
    assert len([r for r in rows if re.match(r"void ss::scan_kernel<", r["name"])]) == 22         # the product's objects, unchanged
    alls = {}
    for r in rows:
        m = re.match(r"void ss::scan_all_kernel<(\d), (\d), (true|false)>", r["name"])
        if not m:
            continue
        alls[m.groups()] = r
        assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128, r
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
        assert r.get("lds_bytes", 0) <= 1024, r
        # spilled scalar registers (written once at kernel entry, read back on tiles with candidates): what the build records today
        ceiling = 0 if m.group(3) == "true" else (48 if m.group(2) == "2" else 88)
        assert r["sgpr_spills"] <= ceiling, (r["name"], r["sgpr_spills"])
    # one kernel per (Q, MODE, one-byte) combination find() has: 4 Q x MODE 0, 4 Q x MODE 2, one-byte
    assert sorted(alls) == sorted([(str(q), m, "false") for q in range(4) for m in ("0", "2")] + [("0", "0", "true")])
    assert len(product) == 37


def test_methods_refuse_outside_the_matches_library():
    class Fake:
        _L = ss.lib()
        _h = None
    for meth, args in (("count", (b"abc",)), ("find_all", (b"abc",))):
        with pytest.raises(ss.SlicesliceError, match="matches_build"):
            getattr(ss.DynamicHipSearcher, meth)(Fake(), *args)


def test_tools_know_the_new_flags():
    grep = open(os.path.join(ROOT, "tools", "grep_hip.py")).read()
    assert "--count" in grep and "--offsets" in grep
    assert os.path.exists(os.path.join(ROOT, "tools", "matches_bench.py"))
