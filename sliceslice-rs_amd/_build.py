"""Builds csrc/ into the in-tree C-ABI libraries with hipcc for gfx950 (cross-compiles without a GPU).

    libsliceslice_hip.so          the product: include/sliceslice_hip.h and nothing else (-fvisibility=hidden)
    libsliceslice_hip_<name>.so   the opt-in libraries of LIBRARIES below (service, matches, matches_batched, lines, nocase, bounded,
                                  inverted, context, anyof, needleset, setmatches, disjoint) and of the mappings under it (output,
                                  leftmost, masked, classes, runs, rewrite, fields, groups): the
                                  objects of the library's parent (the product's, where it has none) plus its own sources, which
                                  define include/sliceslice_hip_<name>.h - a process uses ONE library: the product or one of these
    libsliceslice_hip_tools.so    benchmark helpers (synthetic haystack generator, read ceiling, self-test): ss_tools.hip
    libsliceslice_hip_tuning.so   the product's sources with -DSS_TUNING_VARIANTS -DSS_TEST_HOOKS: every kernel variant,
                                  ss_searcher_set_variant / _set_grid, fault injection (tools/, the variant and hook tests)
    libsliceslice_hip_asan.so / _tsan.so   the host code under sanitizers (with the test hooks), device code untouched
    tests/native/libfake_rccl.so  the shared-memory RCCL stand-in of the multi-rank tests (test infrastructure)

Every translation unit is compiled in parallel.  Concurrency: every rank of a `torch.distributed.run` job may call build() at
once on a fresh clone.  Each build runs under an exclusive fcntl lock, objects and libraries are written to temporary names and
os.replace()d into place, so no process can ever CDLL a half-written file, and the up-to-date check compares the library with
its objects (a failed link leaves an old .so behind newer .o files)."""
import fcntl
import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_ROOT = os.path.dirname(_HERE)
_SO = os.path.join(_CSRC, "libsliceslice_hip.so")
_TOOLS_SO = os.path.join(_CSRC, "libsliceslice_hip_tools.so")
# host-side translation units (ss_internal.hpp lists what each holds) ...
_HOST_SOURCES = ["ss_core.hip", "ss_scan.hip", "ss_census.hip", "ss_host.hip", "ss_batched.hip", "ss_comm.hip"]
# ... and the scan kernel family, one explicit-instantiation unit per (U, load flavour, search / find).  The product holds what
# the constructors and ss_searcher_set_filter3 can select (scan_launch.hpp::kernel_built): U = 4, non-temporal loads.
_KERNEL_SOURCES = ["scan_inst_u4_nt1.hip", "scan_inst_find_nt1.hip"]
_SOURCES = _HOST_SOURCES + _KERNEL_SOURCES


def _library(name, parent, sources, resources=True):
    return {"parent": parent, "sources": sources, "so": os.path.join(_CSRC, "libsliceslice_hip_%s.so" % name),
            "resources": os.path.join(_CSRC, "kernel_resources_%s.json" % name) if resources else None}


# The opt-in libraries, none of them in the product, each entered ONCE and here: name -> its parent (None: the product; a parent stands
# before its children), the sources it adds to its parent's, its .so and the record of its kernels' registers.  The name is also that
# of its header (include/sliceslice_hip_<name>.h), of its table and context manager in searcher.py (<NAME>_ABI, <name>_build), of its
# lock file (.build_<name>.lock) and of the build_<name> / <name>_library_path / ... functions defined from this table further down.
LIBRARIES = {
    "service": _library("service", None, ["ss_service.hip"], resources=False),       # (also in the hooks builds)
    "matches": _library("matches", None, ["ss_matches.hip", "scan_inst_all.hip"]),
    "matches_batched": _library("matches_batched", "matches", ["ss_matches_batched.hip", "scan_inst_all_batched.hip"]),
    "lines": _library("lines", "matches", ["ss_lines.hip", "scan_inst_lines.hip"]),
    "nocase": _library("nocase", "lines", ["ss_nocase.hip", "scan_inst_nocase.hip"]),
    "bounded": _library("bounded", "nocase", ["ss_bounded.hip", "scan_inst_bounded.hip", "scan_inst_bounded_nocase.hip"]),
    "inverted": _library("inverted", "bounded", ["ss_inverted.hip", "scan_inst_inverted.hip", "scan_inst_inverted_nocase.hip"]),
    "context": _library("context", "inverted", ["ss_context.hip"]),
    "anyof": _library("anyof", "context", ["ss_anyof.hip"]),
    "needleset": _library("needleset", "anyof", ["ss_needleset.hip"]),
    "setmatches": _library("setmatches", "needleset", ["ss_setmatches.hip"]),
    "disjoint": _library("disjoint", "setmatches", ["ss_disjoint.hip"]),
}
# The thirteenth, in a mapping of its own until the table's pinned list of names moves: grep's output written on the device
# (include/sliceslice_hip_output.h).  Everything below looks in both mappings.
_LATER_LIBRARIES = {"output": _library("output", "disjoint", ["ss_output.hip"])}
# ... and the fourteenth beside it: leftmost-longest selection over a needle set's pairs and the set replace
# (include/sliceslice_hip_leftmost.h).
_LATER_LIBRARIES["leftmost"] = _library("leftmost", "output", ["ss_leftmost.hip"])
# ... and the fifteenth, in a third mapping because the two above are pinned name by name: byte patterns with wildcards and per-byte
# masks (include/sliceslice_hip_masked.h).
_LATEST_LIBRARIES = {"masked": _library("masked", "leftmost", ["ss_masked.hip"])}
# ... and the sixteenth below it: fixed-length patterns of byte classes (include/sliceslice_hip_classes.h).
_LATEST_LIBRARIES["classes"] = _library("classes", "masked", ["ss_classes.hip"])
# ... and the seventeenth, in a fourth mapping because the names of the third are pinned too: the maximal runs of one byte class
# (include/sliceslice_hip_runs.h).
_NEWEST_LIBRARIES = {"runs": _library("runs", "classes", ["ss_runs.hip"])}
# ... and the eighteenth, in a fifth mapping for the same reason: the selected runs replaced or deleted on the device
# (include/sliceslice_hip_rewrite.h).
_REWRITE_LIBRARIES = {"rewrite": _library("rewrite", "runs", ["ss_rewrite.hip"])}
# ... and the nineteenth, in a sixth mapping for the same reason: fields first .. last of every line located on the device
# (include/sliceslice_hip_fields.h).
_FIELDS_LIBRARIES = {"fields": _library("fields", "rewrite", ["ss_fields.hip"])}
# ... and the twentieth, in a seventh mapping for the same reason: equal tokens or lines grouped and counted on the device
# (include/sliceslice_hip_groups.h).
_GROUPS_LIBRARIES = {"groups": _library("groups", "fields", ["ss_groups.hip"])}
_SERVICE_SOURCES = LIBRARIES["service"]["sources"]
# The tuning build adds every variant ss_searcher_set_variant can name: plain loads, U = 8.
_TUNING_SOURCES = _SOURCES + _SERVICE_SOURCES + ["scan_inst_u4_nt0.hip", "scan_inst_find_nt0.hip", "scan_inst_u8_nt0.hip", "scan_inst_u8_nt1.hip"]
# What every object is older than when it is stale: each csrc/*.hpp and each C header include/*.h (the include/*.hpp C++ wrappers are
# compiled into nothing here), relative to csrc/.  Read from the tree, so that a new header cannot be forgotten.
_HEADERS = sorted(f for f in os.listdir(_CSRC) if f.endswith(".hpp")) + \
    sorted(os.path.join("..", "..", "include", f) for f in os.listdir(os.path.join(_ROOT, "include")) if f.endswith(".h"))
_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-fvisibility=hidden"]
_HOOK_FLAGS = ["-DSS_TEST_HOOKS=1"]
# Host-side sanitizer builds (the reference's guard on its unsafe code is its ASAN CI job,
# .github/workflows/check.yml:42-58): ASan + UBSan / TSan on the HOST code of the same sources, device code untouched.
_SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-omit-frame-pointer", "-g", "-O1"]
_TSAN_FLAGS = ["-fsanitize=thread", "-fno-gpu-sanitize", "-fno-omit-frame-pointer", "-g", "-O1"]
_NATIVE_BENCH_SRC = os.path.join(_ROOT, "tools", "native_bench.cpp")
_NATIVE_BENCH = os.path.join(_ROOT, "tools", "native_bench")
_FAKE_RCCL_SRC = os.path.join(_ROOT, "tests", "native", "fake_rccl.c")
_FAKE_RCCL = os.path.join(_ROOT, "tests", "native", "libfake_rccl.so")


def library_path():
    return _SO


def tools_library_path():
    return _TOOLS_SO


def native_bench_path():
    return _NATIVE_BENCH


def fake_rccl_path():
    return _FAKE_RCCL


def _mtime(rel):
    return os.path.getmtime(os.path.join(_CSRC, rel))


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: the HIP library cannot be built (and there is no CPU fallback)")
    return hipcc


class _Lock:
    def __init__(self, name):
        self._path = os.path.join(_CSRC, name)

    def __enter__(self):
        self._fh = open(self._path, "w")
        fcntl.flock(self._fh, fcntl.LOCK_EX)
        return self

    def __exit__(self, *a):
        fcntl.flock(self._fh, fcntl.LOCK_UN)
        self._fh.close()
        return False


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _build_variant(so, obj_suffix, extra_flags, link_flags, force, verbose, sources, own=None, record_resources=False,
                   resources=None):
    """Compiles `sources` (those in `own` - default: all - with `extra_flags` into <name><obj_suffix>; the others are taken as the
    regular build's <name>.o) and links them into `so`.  record_resources: every kernel's registers of the library go to
    `resources` (default csrc/kernel_resources.json)."""
    resources = resources or _RESOURCES
    own = sources if own is None else own
    newest_header = max(_mtime(h) for h in _HEADERS)
    objs = [os.path.join(_CSRC, s[:-4] + (obj_suffix if s in own else ".o")) for s in sources]
    todo = []
    for src, obj in zip(sources, objs):
        if src not in own:
            continue
        stale = record_resources and not os.path.exists(obj + ".res")            # objects from before the resource record
        if force or stale or not os.path.exists(obj) or os.path.getmtime(obj) < max(_mtime(src), newest_header):
            todo.append((src, obj))
    if (not todo and os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(o) for o in objs) and
            (not record_resources or os.path.exists(resources))):
        return so
    hipcc = _hipcc()
    tag = ".tmp%d" % os.getpid()

    def compile_one(job):
        src, obj = job
        cmd = [hipcc] + _FLAGS + extra_flags + ["-c", os.path.join(_CSRC, src), "-o", obj + tag]
        if not record_resources:
            _run(cmd, verbose)
        else:
            # the regular build also records what the register allocator did with every kernel (see _resources)
            if verbose:
                print(" ".join(cmd), flush=True)
            p = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], stderr=subprocess.PIPE, text=True)
            rows = _resources(p.stderr, src)
            if p.returncode != 0:
                sys.stderr.write(p.stderr)
                raise subprocess.CalledProcessError(p.returncode, cmd)
            with open(obj + ".res" + tag, "w") as f:
                json.dump(rows, f)
            os.replace(obj + ".res" + tag, obj + ".res")
        os.replace(obj + tag, obj)

    if todo:
        with ThreadPoolExecutor(max_workers=min(len(todo), os.cpu_count() or 1) or 1) as pool:
            list(pool.map(compile_one, todo))
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-Bsymbolic-functions", "-o", so + tag] + link_flags + objs +
         ["-ldl", "-pthread"], verbose)
    os.replace(so + tag, so)
    if record_resources:
        rows = []
        for o in objs:
            if os.path.exists(o + ".res"):
                rows += json.load(open(o + ".res"))
        with open(resources + tag, "w") as f:
            json.dump(rows, f, indent=0)
        os.replace(resources + tag, resources)
    return so


_RESOURCES = os.path.join(_CSRC, "kernel_resources.json")
_RES_KEYS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
             "Occupancy [waves/SIMD]": "waves_per_simd", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
             "LDS Size [bytes/block]": "lds_bytes"}


def _resources(remarks, tu):
    """-Rpass-analysis=kernel-resource-usage remarks -> one row per kernel.  Kept next to the library
    (csrc/kernel_resources.json, `kernel_resources()`): the scan kernels are fast at four waves per SIMD (<= 128 VGPRs) and
    14 % slower at three, and which side of 128 the allocator lands on moves with unrelated edits; scalar-register spills
    (v_writelane traffic in front of every short-lived workgroup's first load) doubled unnoticed in round 3."""
    rows, cur = [], None
    for line in remarks.splitlines():
        m = re.search(r"remark: (?:\s*)([A-Za-z \[\]/]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"kernel": val, "tu": tu}
            rows.append(cur)
        elif cur is not None and key in _RES_KEYS:
            cur[_RES_KEYS[key]] = int(val)
    if rows:
        names = subprocess.run(["c++filt"] + [r["kernel"] for r in rows], capture_output=True, text=True)
        if names.returncode == 0:
            for r, n in zip(rows, names.stdout.splitlines()):
                r["name"] = n
    return rows


def kernel_resources():
    """Rows of csrc/kernel_resources.json (written by build()): kernel, name, vgprs, waves_per_simd, spills, ...  Product library
    only (the tools library's kernels are in csrc/ss_tools.o.res)."""
    build()
    return json.load(open(_RESOURCES))


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> csrc/libsliceslice_hip.so (+ libsliceslice_hip_tools.so).  Returns the product's path."""
    with _Lock(".build.lock"):
        so = _build_variant(_SO, ".o", [], [], force, verbose, _SOURCES, record_resources=True)
    build_tools(force=force, verbose=verbose)
    return so


def _lib(name):
    """The entry of library `name` (KeyError: there is none)."""
    for table in (LIBRARIES, _GROUPS_LIBRARIES, _FIELDS_LIBRARIES, _REWRITE_LIBRARIES, _NEWEST_LIBRARIES, _LATEST_LIBRARIES):
        if name in table:
            return table[name]
    return _LATER_LIBRARIES[name]


def _all_sources(name):
    """The sources of library `name` and of every library it stands on, the product's first (None: the product's alone)."""
    return _SOURCES if name is None else _all_sources(_lib(name)["parent"]) + _lib(name)["sources"]


def build_library(name, force=False, verbose=False):
    """`name` is a key of LIBRARIES, the one table.  The objects of its parent (built first; they and their resource records are shared)
    + its own sources -> csrc/libsliceslice_hip_<name>.so.  The kernels of the whole library are recorded in csrc/kernel_resources_<name>.json (the
    service has no kernels of interest and no record)."""
    lib = _lib(name)
    if lib["parent"] is None:
        build(verbose=verbose)
    else:
        build_library(lib["parent"], verbose=verbose)
    with _Lock(".build_%s.lock" % name):
        return _build_variant(lib["so"], ".o", [], [], force, verbose, _all_sources(name), own=lib["sources"],
                              record_resources=lib["resources"] is not None, resources=lib["resources"])


def library_path_of(name):
    return _lib(name)["so"]


def library_kernel_resources(name):
    """Rows of csrc/kernel_resources_<name>.json (written by build_library(name)): the kernels of the library's parents and its own."""
    build_library(name)
    return json.load(open(_lib(name)["resources"]))


def _wrappers(name):
    """build_<name>, <name>_library_path and - where the library has a resource record - <name>_resources_path and
    <name>_kernel_resources: the names tests, tools and documents call, by those names."""
    def build_it(force=False, verbose=False): return build_library(name, force, verbose)                             # noqa: E704
    named = {"build_" + name: build_it, name + "_library_path": lambda: library_path_of(name)}
    if _lib(name)["resources"] is not None:
        named.update({name + "_resources_path": lambda: _lib(name)["resources"], name + "_kernel_resources": lambda: library_kernel_resources(name)})
    for public, function in named.items():
        function.__name__ = function.__qualname__ = public
    return named


for _name in (list(LIBRARIES) + list(_LATER_LIBRARIES) + list(_LATEST_LIBRARIES) + list(_NEWEST_LIBRARIES) + list(_REWRITE_LIBRARIES) +
              list(_FIELDS_LIBRARIES) + list(_GROUPS_LIBRARIES)):
    globals().update(_wrappers(_name))


def build_tools(force=False, verbose=False):
    """csrc/ss_tools.hip -> csrc/libsliceslice_hip_tools.so: the benchmark helpers of include/sliceslice_hip_tuning.h, group 1."""
    with _Lock(".build_toolslib.lock"):
        return _build_variant(_TOOLS_SO, ".o", [], [], force, verbose, ["ss_tools.hip"])


def build_sanitized(force=False, verbose=False):
    """The host logic with ASan + UBSan and the test hooks -> csrc/libsliceslice_hip_asan.so (test builds only:
    load it with SLICESLICE_HIP_LIB=<path> and the ASan runtime preloaded; see tests/test_gpu_native.py)."""
    so = os.path.join(_CSRC, "libsliceslice_hip_asan.so")
    build(verbose=verbose)                                  # the kernel-instantiation objects are shared with the regular build
    with _Lock(".build_asan.lock"):
        return _build_variant(so, ".asan.o", _SAN_FLAGS + _HOOK_FLAGS, ["-fsanitize=address,undefined", "-shared-libsan"], force, verbose,
                              _SOURCES + _SERVICE_SOURCES, own=_HOST_SOURCES + _SERVICE_SOURCES)


def build_tsan(force=False, verbose=False):
    """ThreadSanitizer build of the host code (with the test hooks) -> csrc/libsliceslice_hip_tsan.so (tests/test_gpu_native.py)."""
    so = os.path.join(_CSRC, "libsliceslice_hip_tsan.so")
    build(verbose=verbose)
    with _Lock(".build_tsan.lock"):
        return _build_variant(so, ".tsan.o", _TSAN_FLAGS + _HOOK_FLAGS, ["-fsanitize=thread", "-shared-libsan"], force, verbose,
                              _SOURCES + _SERVICE_SOURCES, own=_HOST_SOURCES + _SERVICE_SOURCES)


def tsan_runtime():
    out = subprocess.check_output([_hipcc(), "-print-file-name=libclang_rt.tsan-x86_64.so"], text=True).strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def asan_runtime():
    """Path of the clang ASan runtime that build_sanitized() links against (to LD_PRELOAD into python)."""
    out = subprocess.check_output([_hipcc(), "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def build_native_bench(force=False, verbose=False):
    """tools/native_bench.cpp -> tools/native_bench: the measurements that must not have Python or torch in the
    loop (per-call latencies, the config-1 per-needle loop, the multi-rank overheads), linked against the in-tree libraries."""
    build(verbose=verbose)
    so = build_service(verbose=verbose)         # (a superset of the product: the tool also times the resident service)
    with _Lock(".build_tools.lock"):
        if (not force and os.path.exists(_NATIVE_BENCH) and
                os.path.getmtime(_NATIVE_BENCH) >= max(os.path.getmtime(_NATIVE_BENCH_SRC), os.path.getmtime(so), os.path.getmtime(_TOOLS_SO))):
            return _NATIVE_BENCH
        tmp = _NATIVE_BENCH + ".tmp%d" % os.getpid()
        _run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(_ROOT, "include"), _NATIVE_BENCH_SRC, "-o", tmp,
              "-L", _CSRC, "-lsliceslice_hip_service", "-lsliceslice_hip_tools", "-Wl,-rpath,$ORIGIN/../sliceslice-rs_amd/csrc",
              "-Wl,-rpath,/opt/rocm/lib", "-pthread"], verbose)
        os.replace(tmp, _NATIVE_BENCH)
        return _NATIVE_BENCH


def build_fake_rccl(force=False, verbose=False):
    """tests/native/fake_rccl.c -> tests/native/libfake_rccl.so: the shared-memory stand-in that lets the native collective code
    run with several ranks on ONE GPU (real RCCL refuses that).  Test infrastructure; handed to the library with
    SLICESLICE_RCCL_LIB=<path>."""
    with _Lock(".build_fake_rccl.lock"):
        if not force and os.path.exists(_FAKE_RCCL) and os.path.getmtime(_FAKE_RCCL) >= os.path.getmtime(_FAKE_RCCL_SRC):
            return _FAKE_RCCL
        tmp = _FAKE_RCCL + ".tmp%d" % os.getpid()
        _run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-I/opt/rocm/include", _FAKE_RCCL_SRC, "-o", tmp,
              "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-pthread", "-Wl,-rpath,/opt/rocm/lib"], verbose)
        os.replace(tmp, _FAKE_RCCL)
        return _FAKE_RCCL


def tuning_library_path():
    return os.path.join(_CSRC, "libsliceslice_hip_tuning.so")


def build_tuning(force=False, verbose=False):
    """Every kernel variant ss_searcher_set_variant can name plus the test hooks (-DSS_TUNING_VARIANTS -DSS_TEST_HOOKS, with the plain-load
    and U = 8 translation units) -> csrc/libsliceslice_hip_tuning.so.  Not the product: tools/ and the variant / hook tests load it
    with SLICESLICE_HIP_LIB=<path>."""
    so = tuning_library_path()
    with _Lock(".build_tuning.lock"):
        return _build_variant(so, ".tuning.o", ["-DSS_TUNING_VARIANTS=1"] + _HOOK_FLAGS, [], force, verbose, _TUNING_SOURCES)


def build_ab(name, defines, force=False, verbose=False):
    """A/B builds of the SAME sources with extra -D flags -> csrc/libsliceslice_hip_<name>.so (tuning only; load
    with SLICESLICE_HIP_LIB=<path>, see tools/ab_compare.py)."""
    so = os.path.join(_CSRC, "libsliceslice_hip_%s.so" % name)
    with _Lock(".build_ab_%s.lock" % name):
        return _build_variant(so, ".%s.o" % name, ["-D" + d for d in defines] + _HOOK_FLAGS, [], force, verbose, _SOURCES + _SERVICE_SOURCES)
