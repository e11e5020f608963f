"""CPU-only checks of the bindings around the C ABI and of bench.py's launch contract.

* the Rust `extern "C"` block (sliceslice-rs_amd/bindings/rust/hip.rs - source only, there is no rustc in this
  image) is compared mechanically with include/sliceslice_hip.h: same names, same arity, same pointer /
  integer widths per argument and for the return value;
* the ctypes table of the Python mirror gets the same treatment;
* `python bench.py --gpus N` never prints a line it cannot back with N ranks on N devices."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

import sliceslice_rs_amd as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strip_c_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _c_class(t):
    """pointer / integer width class of a C type as spelled in the header."""
    t = t.strip()
    if "*" in t or "[" in t:
        return "ptr"
    t = re.sub(r"\bconst\b", "", t).strip()
    return {"int": "i32", "unsigned": "u32", "size_t": "usize", "uint64_t": "u64", "uint32_t": "u32", "float": "f32", "double": "f64",
            "void": "void"}[t]


def header_prototypes(header="sliceslice_hip.h"):
    text = _strip_c_comments(open(os.path.join(ROOT, "include", header)).read())
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    text = re.sub(r"\bSS_API\b", "", text)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret.startswith("typedef"):
            continue
        arglist = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                arr = "[" in a
                a = re.sub(r"\[.*?\]", "", a)
                mm = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a.strip())      # type + parameter name
                typ = mm.group(1).strip()
                arglist.append("ptr" if arr else _c_class(typ))
        protos[name] = (_c_class(ret), arglist)
    return protos


def _rust_class(t):
    t = t.strip()
    if t.startswith("*"):
        return "ptr"
    return {"c_int": "i32", "c_uint": "u32", "usize": "usize", "u64": "u64", "u32": "u32", "c_float": "f32", "f64": "f64"}[t]


def rust_prototypes(source="hip.rs"):
    text = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", source)).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', text, flags=re.S).group(1)
    block = re.sub(r"//[^\n]*", "", block)
    protos = {}
    for m in re.finditer(r"fn\s+(ss_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        name, args, ret = m.group(1), m.group(2).strip(), (m.group(3) or "").strip()
        arglist = [_rust_class(a.split(":", 1)[1]) for a in args.split(",") if a.strip()] if args else []
        protos[name] = ("void" if not ret else _rust_class(ret), arglist)
    return protos


def build_module():
    return sys.modules["sliceslice_rs_amd._build"]


def exported(path):
    """names of the functions a shared library exports"""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)


def ctypes_class(t):
    """pointer / integer width class of an entry of a ctypes table, as header_prototypes spells it.  c_size_t and c_uint64 are one
    ctypes type on this ABI (and c_uint32 is c_uint), so both come out as "u64": callers compare after usize -> u64."""
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents") or isinstance(t, type(ctypes.POINTER(ctypes.c_int))):
        return "ptr"
    return {ctypes.c_int: "i32", ctypes.c_uint: "u32", ctypes.c_size_t: "usize", ctypes.c_uint64: "u64", ctypes.c_float: "f32",
            ctypes.c_double: "f64"}[t]


def test_header_parser_sees_every_symbol():
    protos = header_prototypes()
    assert sorted(protos) == sorted(ss.searcher.ABI)                 # the same set tests/test_host_logic.py checks in the .so
    assert len(protos) <= 50 and not any(n.startswith("ss_debug_") for n in protos)       # the reference-facing surface stays small
    tuning = header_prototypes("sliceslice_hip_tuning.h")
    assert sorted(tuning) == sorted(list(ss.searcher.TOOLS_ABI) + list(ss.searcher.HOOKS_ABI))
    # the resident search service is declared apart (a library of its own: libsliceslice_hip_service.so)
    service = header_prototypes("sliceslice_hip_service.h")
    assert sorted(service) == sorted(ss.searcher.SERVICE_ABI) and not any(n.startswith("ss_service_") for n in protos)
    assert protos["ss_searcher_new"] == ("i32", ["ptr", "usize", "ptr"])
    assert protos["ss_find_sharded"] == ("i32", ["ptr", "ptr", "usize", "u64", "ptr", "ptr", "ptr"])
    assert protos["ss_searcher_free"] == ("void", ["ptr"])
    assert protos["ss_last_error"] == ("ptr", [])


def test_rust_extern_block_matches_the_header():
    c, r = header_prototypes(), rust_prototypes()
    assert sorted(r) == sorted(c), (sorted(set(c) - set(r)), sorted(set(r) - set(c)))
    for name in c:
        assert r[name] == c[name], (name, r[name], c[name])
    # ... and the service's module against the service's header
    cs, rs = header_prototypes("sliceslice_hip_service.h"), rust_prototypes("hip_service.rs")
    assert sorted(rs) == sorted(cs) == sorted(ss.searcher.SERVICE_ABI)
    for name in cs:
        assert rs[name] == cs[name], (name, rs[name], cs[name])
    text = open(os.path.join(ROOT, "sliceslice-rs_amd", "bindings", "rust", "hip.rs")).read()
    # constants the Rust side restates
    hdr = open(os.path.join(ROOT, "include", "sliceslice_hip.h")).read()
    for cname, cval in re.findall(r"^\s*(SS_(?:OK|ERR_[A-Z_]+))\s*=\s*(\d+)", hdr, flags=re.M):
        assert re.search(r"pub const %s: c_int = %s;" % (cname, cval), text), cname
    assert "pub const SS_UNIQUE_ID_BYTES: usize = 128;" in text and "#define SS_UNIQUE_ID_BYTES 128" in hdr
    # `new` must not degrade to with_position(len - 1): the caller of `new` did not choose a position
    new_body = text.split("pub fn new(needle: N) -> Self {", 1)[1].split("}", 1)[0]
    assert "ss_searcher_new(" in new_body and "with_position" not in new_body
    # the copy shown in INTEGRATION.md is this file's extern block, not an older one
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "bindings/rust/hip.rs" in integ and "ss_search_sharded_all" in integ


def test_ctypes_table_matches_the_header():
    c, cls = header_prototypes(), ctypes_class
    c.update(header_prototypes("sliceslice_hip_tuning.h"))
    c.update(header_prototypes("sliceslice_hip_service.h"))
    tables = dict(ss.searcher.ABI, **ss.searcher.TOOLS_ABI, **ss.searcher.HOOKS_ABI, **ss.searcher.SERVICE_ABI)
    for name, (res, args) in tables.items():
        got = (cls(res), [cls(a) for a in args])
        want = c[name]
        # size_t and uint64_t are the same width on this ABI; the table may spell either
        norm = lambda p: (p[0].replace("usize", "u64"), [a.replace("usize", "u64") for a in p[1]])   # noqa: E731
        assert norm(got) == norm(want), (name, got, want)


# What the one table holds: name -> (parent, the sources it adds, the internal headers it is known to need, the symbol has_<name>
# keys on where that is pinned).  Every library's own header, include/sliceslice_hip_<name>.h, is expected besides.
EXPECTED_LIBRARIES = {
    "service": (None, ["ss_service.hip"], [], None),
    "matches": (None, ["ss_matches.hip", "scan_inst_all.hip"], [], None),
    "matches_batched": ("matches", ["ss_matches_batched.hip", "scan_inst_all_batched.hip"], [], None),
    "lines": ("matches", ["ss_lines.hip", "scan_inst_lines.hip"], [], None),
    "nocase": ("lines", ["ss_nocase.hip", "scan_inst_nocase.hip"], [], None),
    "bounded": ("nocase", ["ss_bounded.hip", "scan_inst_bounded.hip", "scan_inst_bounded_nocase.hip"], [], None),
    "inverted": ("bounded", ["ss_inverted.hip", "scan_inst_inverted.hip", "scan_inst_inverted_nocase.hip"],
                 ["inverted_kernels.hpp", "inverted_small_kernels.hpp", "inverted_launch.hpp", "bounded_how.hpp"], None),
    "context": ("inverted", ["ss_context.hip"], ["context_kernels.hpp", "context_launch.hpp", "context_ranges.hpp"], None),
    "anyof": ("context", ["ss_anyof.hip"], ["anyof_kernels.hpp", "anyof_launch.hpp", "anyof_segments.hpp"], "ss_union_numbers_device"),
    "needleset": ("anyof", ["ss_needleset.hip"], ["needleset_kernels.hpp", "needleset_launch.hpp", "needleset_tables.hpp"], "ss_needle_set_new"),
    "setmatches": ("needleset", ["ss_setmatches.hip"],
                   ["setmatches_kernels.hpp", "setmatches_launch.hpp", "needleset_host.hpp", "needleset_tables.hpp"], "ss_count_set_device"),
    "disjoint": ("setmatches", ["ss_disjoint.hip"], ["disjoint_kernels.hpp", "disjoint_launch.hpp", "disjoint_host.hpp"], "ss_count_disjoint_device"),
}
DELETED_TABLES = ["MORE_LIBRARIES", "YET_MORE_LIBRARIES", "ONE_MORE_LIBRARY", "NEXT_LIBRARY", "SET_LIBRARY", "OCCURRENCE_LIBRARY", "DISJOINT_LIBRARY"]


def test_every_library_of_the_table_has_its_header_table_context_flag_and_guard():
    """_build.LIBRARIES is the one place a library is entered: everything else about it goes by its name."""
    b = build_module()
    libraries, csrc = b.LIBRARIES, os.path.join(ROOT, "sliceslice-rs_amd", "csrc")
    assert list(libraries) == list(EXPECTED_LIBRARIES)
    with pytest.raises(KeyError):
        b._lib("no such library")
    # a change to any internal header or C header rebuilds the objects: the list is the tree's
    on_disk = [f for f in os.listdir(csrc) if f.endswith(".hpp")] + \
        [os.path.join("..", "..", "include", f) for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")]
    assert sorted(b._HEADERS) == sorted(on_disk) and len(on_disk) >= 57
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    product = ss.lib()
    for name, entry in libraries.items():
        parent, sources, headers, symbol = EXPECTED_LIBRARIES[name]
        assert entry["parent"] is None or entry["parent"] in list(libraries)[:list(libraries).index(name)], name
        assert entry["parent"] == parent and entry["sources"] == sources and b._lib(name) is entry, name
        assert all(os.path.exists(os.path.join(csrc, s)) for s in entry["sources"]), name
        assert b.library_path_of(name) == entry["so"] == getattr(b, name + "_library_path")(), name
        assert os.path.basename(entry["so"]) == "libsliceslice_hip_%s.so" % name
        if name == "service":
            assert entry["resources"] is None and not hasattr(b, "service_resources_path") and not hasattr(b, "service_kernel_resources")
        else:
            assert os.path.basename(entry["resources"]) == "kernel_resources_%s.json" % name == os.path.basename(getattr(b, name + "_resources_path")())
            assert "sliceslice-rs_amd/csrc/" + os.path.basename(entry["resources"]) in ignored, name
        assert b._all_sources(name) == b._all_sources(parent) + sources, name
        header = "sliceslice_hip_%s.h" % name
        for h in headers + [os.path.join("..", "..", "include", header)]:
            assert h in b._HEADERS and os.path.exists(os.path.join(csrc, h)), h
        table = getattr(ss.searcher, name.upper() + "_ABI")
        assert sorted(table) == sorted(header_prototypes(header)), name
        assert ss.searcher._FEATURES[name][0] is table and ss.searcher._FEATURES[name][1] in table, name
        assert symbol is None or ss.searcher._FEATURES[name][1] == symbol, name
        context = getattr(ss, name + "_build")
        assert not getattr(product, "has_" + name), name
        with pytest.raises(ss.SlicesliceError, match=r"ss\.%s_build\(\)" % name) as e:
            ss.searcher._feature_lib(product, name)
        assert e.value.code == ss.SS_ERR_ARGUMENT
        with context() as L:
            assert ss.lib() is L and getattr(L, "has_" + name) and ss.searcher._feature_lib(L, name) is L, name
            held, up = set(), name
            while up is not None:                       # a library holds what it stands on, and nothing else of the table
                held.add(up)
                up = libraries[up]["parent"]
            assert {n for n in libraries if getattr(L, "has_" + n)} == held, name
            with ss.service_build() as inner:           # blocks nest and restore
                assert ss.lib() is inner
            assert ss.lib() is L
        assert ss.lib() is product


def test_the_one_table_is_what_the_entry_point_builds_and_the_documents_describe():
    entry_point = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    # the whole table (the colon: no slice of it), in its pinned order, before the tuning build - and no library by hand
    assert entry_point.index("for name in b.LIBRARIES:") < entry_point.index("b.build_library(name, force=True, verbose=True)") < entry_point.index("b.build_tuning(")
    assert not [name for name in EXPECTED_LIBRARIES if "b.build_%s(" % name in entry_point]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    paragraph = [p for p in design.split("\n\n") if "opt-in libraries" in p and "entered ONCE" in p]
    assert len(paragraph) == 1 and "`LIBRARIES`" in paragraph[0]
    assert all(re.search(r"\b%s\b" % name, paragraph[0]) for name in EXPECTED_LIBRARIES)
    # the seven tables that stood next to it are gone from the code and from the two documents (this file names them to say so)
    texts = [os.path.join(ROOT, "README.md"), os.path.join(ROOT, "DESIGN.md")]
    for folder, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if not d.startswith(".")]
        texts += [os.path.join(folder, f) for f in files if f.endswith(".py")]
    for path in texts:
        if os.path.abspath(path) != os.path.abspath(__file__):
            text = open(path, errors="replace").read()
            assert not [t for t in DELETED_TABLES if t in text], path


def _bench(args, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        if not env_extra or k not in env_extra:
            env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300,
                          env=env, cwd=ROOT)


def test_bench_refuses_to_mislabel_a_run():
    """No GPU here: `--gpus 2` must exit non-zero with NOTHING on stdout (the driver parses stdout), and say why.
    The same for a launcher whose WORLD_SIZE disagrees with --gpus, and for N = 1 without a device."""
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("two GPUs visible: the refusal branch is covered by tests/test_gpu_sharded.py")
    out = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert out.returncode != 0 and out.stdout.strip() == ""
    assert "--gpus 2 but only" in out.stderr and "refusing" in out.stderr
    out = _bench(["--gpus", "4", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert out.returncode != 0 and out.stdout.strip() == ""
    assert "WORLD_SIZE=2 but --gpus 4" in out.stderr
    out = _bench(["--steps", "0", "--warmup", "0"])
    assert out.returncode != 0 and out.stdout.strip() == "" and "--steps must be >= 1" in out.stderr
    if not torch.cuda.is_available():
        out = _bench(["--steps", "1", "--warmup", "0"])
        assert out.returncode != 0 and out.stdout.strip() == "" and "no CPU path" in out.stderr


def test_bench_loads_the_built_libraries_from_a_tree_it_cannot_write():
    """bench.py may run as a user who cannot write the checkout another user built: the build lock in csrc/ then raises
    PermissionError before anything is checked, and bench.py loads the libraries build() made instead of failing."""
    code = ("import importlib.util, sys\n"
            "sys.path.insert(0, %r)\n"
            "import sliceslice_rs_amd\n"
            "from oracle import oracle as O\n"
            "def refuse(self):\n"
            "    raise PermissionError(13, 'Permission denied', self._path)\n"
            "sys.modules['sliceslice_rs_amd._build']._Lock.__enter__ = refuse\n"
            "spec = importlib.util.spec_from_file_location('bench_under_test', %r)\n"
            "bench = importlib.util.module_from_spec(spec)\n"
            "spec.loader.exec_module(bench)\n"
            "ss = bench.load_libraries()\n"
            "assert (ss.fill_random_host(4096, 7) == O.fill_random(4096, 7)).all()\n"
            "assert ss.choose_filter_triple(b'privilege level') == ss.choose_filter_triple(b'privilege level', None)\n"
            "print('loaded')\n") % (ROOT, os.path.join(ROOT, "bench.py"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip() == "loaded", out.stdout[-2000:] + out.stderr[-3000:]
    assert "loading the libraries build() made as they are" in out.stderr


def test_filter_pair_choice_properties():
    """ss_choose_filter_triple (pure host code): a pair inside the needle, at most 15 apart, the reference's own
    pair (0, n-1) whenever nothing in the needle is rarer, rare bytes when there are some."""
    import random
    rng = random.Random(1)
    for _ in range(2000):
        n = rng.choice([2, 3, 5, 16, 17, 40, 200, 1500, 3000])
        alpha = rng.choice([bytes(range(256)), b"etaoin shrdlu", b"ab", b"the quick brown fox jumps over the lazy dog.,;!"])
        nd = bytes(rng.choice(alpha) for _ in range(n))
        a, b = ss.choose_filter_pair(nd)
        assert 0 <= a < b < n and b - a <= 15, (nd[:20], a, b)
        assert b < 1024
    assert ss.choose_filter_pair(b"") == (0, 0) and ss.choose_filter_pair(b"x") == (0, 0)
    assert ss.choose_filter_triple(b"ab") == (0, 1, 1)                        # no third byte: the second one once more
    assert ss.choose_filter_triple(b"abc") == (0, 1, 2)
    assert ss.choose_filter_triple(bytes(range(200, 216))) == (0, 15, 14)    # nothing to choose between: the reference's pair + one
    assert ss.choose_filter_triple(b" the quick brown fox ") == (5, 19, 9)   # 'q', 'x', 'k' instead of ' ' and ' '
    assert ss.choose_filter_triple(b"a" * 15 + b"b") == (0, 15, 14)
    assert 1 in ss.choose_filter_triple(b"ab" + b"a" * 14)                   # 'b' is in the filter wherever it sits
    assert ss.choose_filter_triple(b"privilege level zero!")[1] == 20        # '!'
    a, b, c = ss.choose_filter_triple(b"e" * 2000 + b"\x07\x08")            # only the first 1024 bytes are looked at
    assert max(b, c) < 1024
    rng = random.Random(2)
    for _ in range(2000):
        n = rng.choice([3, 4, 16, 17, 100, 2000])
        nd = bytes(rng.choice(b"etaoinshr dlu,.XQ\x00\xfe") for _ in range(n))
        a, b, c = ss.choose_filter_triple(nd)
        assert a < b < n and a < c < n and b != c and b - a <= 15 and c - a <= 15, (nd[:24], a, b, c)
        assert ss.choose_filter_pair(nd) == (a, b)


def test_filter_choice_for_a_callers_position():
    """ss_choose_filter_for_position (pure host code): the caller's byte is always tested; up to 15 bytes from needle[0] the
    partner is the reference's needle[0], further away a byte at most 15 in front of `position`, and a third byte within 15
    of the partner whenever the needle has one to offer."""
    import random
    with ss.tuning_build():                                          # a hooks-build entry point (sliceslice_hip_tuning.h)
        _filter_choice_for_a_callers_position(random.Random(3))
    with pytest.raises(ss.SlicesliceError):                          # ... which the product library does not have
        ss.choose_filter_for_position(b"abc", 1)


def _filter_choice_for_a_callers_position(rng):
    for _ in range(3000):
        n = rng.choice([1, 2, 3, 16, 17, 18, 40, 200, 1100, 3000])
        nd = bytes(rng.choice(b"etaoinshr dlu,.XQ\x00\xfe") for _ in range(n))
        p = rng.choice([0, n - 1, n // 2, rng.randrange(n)])
        a, b, c = ss.choose_filter_for_position(nd, p)
        assert b == p and ss.choose_position(nd) == n - 1
        if p < 16:
            others = [k for k in range(1, min(16, n)) if k != p]                 # what needle[1..15] has to offer as a third byte
            assert a == 0 and (c in others if others and n >= 3 else c == b), (n, p, a, b, c)
        else:
            assert p - 15 <= a < p and a < c <= min(a + 15, n - 1) and c != p, (n, p, a, b, c)
    assert ss.choose_filter_for_position(b" the quick brown fox ", 20) == (5, 20, 19)      # 'q' ... ' ' + 'x'
    assert ss.choose_filter_for_position(b" the quick brown fox ", 7) == (0, 7, 5)
    assert ss.choose_filter_for_position(b"", 5) == (0, 0, 0)                             # N0: any position (x86.rs:470)
    assert ss.choose_filter_for_position(b"x", 0) == (0, 0, 0)
    for nd, p in ((b"x", 1), (b"foo", 3), (b"a" * 40, 40)):                               # x86.rs:300, 473
        with pytest.raises(ss.PositionError):
            ss.choose_filter_for_position(nd, p)


def test_histogram_driven_filter_choice():
    """ss_choose_filter_triple with a histogram: the same chooser with log2(count + 1) of the byte counts as the cost."""
    import numpy as np
    text = open(os.path.join(ROOT, "tests", "golden", "data", "i386.txt"), "rb").read()
    hist = np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256).astype(np.uint64)
    for nd in (b" the quick brown fox ", b"segment descriptor table entries are", b"privilege level zero!", b"ab", b"abc"):
        a, b, c = ss.choose_filter_triple(nd, hist)
        n = len(nd)
        assert 0 <= a < b < n and a < c < n and b - a <= 15 and c - a <= 15 and (c != b or n == 2), (nd, a, b, c)
        # no other triple anchored at the same first byte is rarer under the histogram
        lg = lambda x: np.log2(float(hist[x]) + 1.0)                                       # noqa: E731
        cost = lg(nd[b]) + lg(nd[c])
        others = sorted(lg(nd[k]) for k in range(a + 1, min(n, a + 16)))
        assert n == 2 or cost <= others[0] + others[1] + 0.3, (nd, a, b, c)              # 1/8-bit fixed point in the library
    # a corpus the static ranking is wrong about: all 'a' - the one 'e' must be in the filter
    ha = np.zeros(256, dtype=np.uint64)
    ha[ord("a")] = 10 ** 9
    assert 40 in ss.choose_filter_triple(b"a" * 40 + b"e", ha)
    assert 40 not in ss.choose_filter_triple(b"a" * 40 + b"e")          # the static guess ranks 'e' as the commonest letter
    assert ss.choose_filter_triple(b"xyz", None) == ss.choose_filter_triple(b"xyz")


def test_bench_line_fields_of_the_committed_round2_capture():
    """Shape of the round-2 bench line (committed under profiles/r02 once captured on the GPU box)."""
    path = os.path.join(ROOT, "profiles", "r02", "bench64g.json")
    if not os.path.exists(path):
        import pytest
        pytest.skip("no round-2 capture committed yet")
    d = json.loads(open(path).read())
    assert d["n_gpus"] == 1 and d["config"]["ranks"] == 1 and d["config"]["filter_bytes"] == [0, 15, 13]
    assert d["roofline"]["traffic_source"].startswith("stored ratio")
    assert set(d["configs"]) >= {"1", "3", "5", "latency_us"}
    assert [r["needle_len"] for r in d["configs"]["3"]["rows"]] == [1, 2, 4, 8, 16, 32, 128]
    c = d["cpu_baseline"]
    assert c["cores"] == c["threads_used"] and c["host_physical_cores"] >= 1


def test_rccl_enum_values_the_library_hard_codes():
    """librccl is dlopen()ed, so ss_comm.hip restates four enum values of rccl.h instead of including it; they
    must agree with the header of the ROCm this image ships."""
    hdr = "/opt/rocm/include/rccl/rccl.h"
    if not os.path.exists(hdr):
        import pytest
        pytest.skip("no rccl.h in this image")
    text = open(hdr).read()
    src = open(os.path.join(ROOT, "sliceslice-rs_amd", "csrc", "ss_comm.hip")).read()
    fake = open(os.path.join(ROOT, "tests", "native", "fake_rccl.c")).read()
    for name, const in (("ncclInt32", "kNcclInt32"), ("ncclUint64", "kNcclUint64"), ("ncclMax", "kNcclMax"), ("ncclMin", "kNcclMin")):
        want = int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))
        got = int(re.search(r"constexpr int %s = (\d+);" % const, src).group(1))
        assert got == want, (name, got, want)
        # the shared-memory stand-in of the multi-rank tests restates them too
        assert int(re.search(r"\bk%s = (\d+)" % name[4:], fake).group(1)) == want, name
    assert "#define SS_UNIQUE_ID_BYTES 128" in open(os.path.join(ROOT, "include", "sliceslice_hip.h")).read()
    assert re.search(r"#define NCCL_UNIQUE_ID_BYTES 128", text)


# Ceilings on spilled scalar registers per kernel family - spill SLOTS as the compiler reports them.  What a slot costs depends on
# where it is written: the single-stream kernels write 28 of theirs once, at kernel entry (loop invariants that the candidate path's
# register needs would otherwise push out of the hot loop), and read them back only at the end of a tile that HAD candidates; the hot
# path (load, filter, ballot, next tile) touches none (DESIGN.md section 4.6 has the lane map).  Round 3 doubled the numbers unnoticed
# (26 -> 53 on the headline kernel, 91 -> 184/245 on the batched ones, which inlined one whole scan_tiles per filter window) because
# nothing looked; a build that goes 25 % over what is recorded here fails.  Lower the numbers when a kernel improves.
SGPR_SPILL_CEILINGS = {
    "scan_kernel, single stream (MODE 0), search": 53,
    "scan_kernel, single stream (MODE 0), find": 51,
    "scan_kernel, cross-lane (MODE 2)": 17,
    "scan_kernel, one-byte needles": 0,
    "scan_batched_plan_kernel": 65,
    "service_kernel": 88,
}


def _family(name):
    m = re.match(r"void ss::scan_kernel<(\d), (\d), (true|false), (\d), (\d), (true|false), (true|false)>", name)
    if m:
        q, mode, one_byte, u, nt, find, l8 = m.groups()
        if one_byte == "true":
            return "scan_kernel, one-byte needles"
        if mode in ("2", "3"):
            return "scan_kernel, cross-lane (MODE 2)"
        return "scan_kernel, single stream (MODE 0), " + ("find" if find == "true" else "search")
    for fam in ("scan_batched_plan_kernel", "service_kernel"):
        if fam in name:
            return fam
    return None


def test_kernels_the_library_launches_by_default_keep_four_waves_per_simd():
    """build() records what the register allocator did with every kernel (csrc/kernel_resources.json).  The product library
    holds exactly what the constructors and ss_searcher_set_filter3 can select - 22 scan kernels (scan_launch.hpp::kernel_built),
    37 kernels in all (round 6: minus the service and publish kernels, plus the plan kernels' single-workgroup instantiations); the tuning residue (U = 8, plain loads, two-byte 8-byte phases) lives in the tuning build, and the
    two-stream kernels of rounds 1-3 (MODE 1) are gone.  Every one of them keeps >= 4 waves per SIMD, without scratch and without
    spilled vector registers - which side of a register-count step a kernel lands on has moved with unrelated edits before (at
    three waves the scan runs at 6.3 TB/s) - and within its family's ceiling of spilled scalar registers."""
    build = sys.modules["sliceslice_rs_amd._build"]
    rows = build.kernel_resources()
    names = [r["name"] for r in rows]
    assert len(rows) <= 37, len(rows)
    assert any("scan_batched_plan_kernel<4, false, false, false>" in n for n in names) and any("scan_pairs_kernel" in n for n in names)
    # the plan-run forms: with the run machinery (problems scanned by several workgroups) and without (every problem one workgroup);
    # a run is ONE launch - no publish kernel, and no service kernel in the product
    assert any("scan_batched_plan_kernel<4, false, true, true>" in n for n in names) and any("scan_batched_plan_kernel<4, false, true, false>" in n for n in names)
    assert not any("publish_kernel" in n or "service_kernel" in n for n in names)
    scans = set()
    for r in rows:
        m = re.match(r"void ss::scan_kernel<(\d), (\d), (true|false), (\d), (\d), (true|false), (true|false)>", r["name"])
        if m:
            q, mode, one_byte, u, nt, find, l8 = m.groups()
            scans.add(m.groups())
            assert u == "4" and nt == "1" and mode in ("0", "2", "3"), r["name"]
            assert not (mode == "3" and find == "true"), r["name"]        # the pair-alone kernels exist for search only
            if one_byte == "true":
                assert (l8 == "true") == (find == "false"), r["name"]
            else:
                assert l8 == "false", r["name"]
            assert r.get("lds_bytes", 0) <= 1024, r         # static LDS: the completion word's workgroup flag (occupancy_pad leaves 1 KiB)
        if m or "scan_batched" in r["name"]:
            assert r["waves_per_simd"] >= 4 and r["vgprs"] <= 128, r
            assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
        fam = _family(r["name"])
        if fam is not None:
            assert r["sgpr_spills"] <= SGPR_SPILL_CEILINGS[fam] * 1.25, (fam, r["name"], r["sgpr_spills"])
    assert len(scans) == 22, sorted(scans)
    # The newest tracked copy under profiles/ describes kernels that still meet the same bars (a compiler point release or an
    # unrelated header edit may move a register or a spill: the ceilings above are the contract, not equality with a record).
    import glob
    tracked = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]", "kernel_resources.json")))
    if tracked:
        have = {r["name"] for r in rows}
        for r in json.load(open(tracked[-1])):
            fam = _family(r["name"])
            if r["name"] in have and fam is not None:
                assert r["sgpr_spills"] <= SGPR_SPILL_CEILINGS[fam] * 1.25 and r["waves_per_simd"] >= 4, (tracked[-1], r)
