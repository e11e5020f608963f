"""The one-process-per-GPU path on real hardware, with as many ranks as the box has GPUs (1 on the
test box): torch.distributed (RCCL) and native RCCL (ss_comm_*) transports of the found flag."""
import os
import subprocess
import sys

import pytest

from conftest import timing_log

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("build", ["product", "hooks"])
def test_sharded_search_both_transports(build):
    """Real RCCL, as many ranks as the box has GPUs.  Against the hooks build the worker also injects a failure into the last
    rank's scan (ss_debug_fail_next_scans): that rank its own error, the others SS_ERR_PEER, nobody left in the collective."""
    import torch
    import sliceslice_rs_amd  # noqa: F401
    n = max(1, min(torch.cuda.device_count(), 8))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    if build == "hooks":
        env["SLICESLICE_HIP_LIB"] = sys.modules["sliceslice_rs_amd._build"].build_tuning()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", "29533" if build == "product" else "29534", os.path.join(ROOT, "tests", "_sharded_gpu_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "sharded gpu worker ok" in out.stdout


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_kernels_with_several_ranks_on_one_gpu(world):
    """world_size 2 and 3 with the REAL shard kernels: the ranks share cuda:0 and the flag all-reduce runs
    over gloo (RCCL refuses two ranks on one GPU).  Matches are planted across every shard boundary."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", SS_TEST_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(29540 + world), os.path.join(ROOT, "tests", "_sharded_gpu_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "sharded gpu worker ok" in out.stdout


def test_single_process_multi_gpu_entry():
    """ss_comm_init_all / ss_search_sharded_all / ss_find_sharded_all: every visible GPU (1 on the test box, 8 on a
    node) driven from THIS process, ncclCommInitAll + one grouped all-reduce per search.  Matches are planted at
    0, at the very end and across every shard edge; both combine modes (RCCL all-reduce, host OR) must agree."""
    import numpy as np
    import torch
    import sliceslice_rs_amd as ss
    G = max(1, min(torch.cuda.device_count(), 8))
    needle = bytes(range(200, 216))
    total = (48 << 20) + 12345
    node = ss.NodeSearcher(needle, devices=list(range(G)))
    ranges = [node.shard_range(total, g) for g in range(G)]
    S = -(-total // G)
    shards = []
    for g, (b, e) in enumerate(ranges):
        assert b == g * S and e == min(total, b + S + 15)
        t = torch.empty(e - b, dtype=torch.uint8, device="cuda:%d" % g)
        with torch.cuda.device(g):
            ss.fill_random_device(t, 0x5EED0001, b)
            torch.cuda.synchronize()
        shards.append(t)
    begins = [b for b, _ in ranges]
    pn = np.frombuffer(needle, dtype=np.uint8)
    cur = torch.cuda.current_device()
    for mode in (ss.NodeSearcher.COMBINE_RCCL, ss.NodeSearcher.COMBINE_HOST):
        node.set_combine(mode)
        assert node.search_in(shards) is False and node.find(shards, begins) is None
        spots = [0, total - 16, total // 2] + [r * S - k for r in range(1, G) for k in (1, 8, 15)] + [r * S for r in range(1, G)]
        for at in spots:
            saved = []
            for g, (b, e) in enumerate(ranges):
                lo, hi = max(at, b), min(at + 16, e)
                if lo < hi:                                  # shard g holds (part of) the planted bytes
                    saved.append((g, lo - b, hi - b, shards[g][lo - b:hi - b].clone()))
                    shards[g][lo - b:hi - b] = torch.from_numpy(pn[lo - at:hi - at].copy()).to(shards[g].device)
            for g in range(G):
                torch.cuda.synchronize(g)
            assert node.search_in(shards) is True, (mode, at)
            assert node.find(shards, begins) == at, (mode, at)
            for g, lo, hi, old in saved:
                shards[g][lo:hi] = old
            for g in range(G):
                torch.cuda.synchronize(g)
            assert node.search_in(shards) is False, (mode, at)
        assert torch.cuda.current_device() == cur            # the caller's current device is restored
    # the empty needle, and shards shorter than the needle
    empty = ss.NodeSearcher(b"", devices=list(range(G)))
    assert empty.search_in(shards) is True and empty.find(shards, begins) == 0
    tiny = [s[:5] for s in shards]
    assert node.search_in(tiny) is False and node.find(tiny, begins) is None
    node.close()
    empty.close()
    # epoch wrap of the set's flags (the hook that moves the epoch lives in hooks builds)
    with ss.tuning_build():
        node = ss.NodeSearcher(needle, devices=list(range(G)))
    node.set_epoch(2**31 - 3)
    for mode in (ss.NodeSearcher.COMBINE_RCCL, ss.NodeSearcher.COMBINE_HOST):
        node.set_combine(mode)
        for it in range(4):
            assert node.search_in(shards) is False
            shards[-1][-16:] = torch.from_numpy(pn.copy()).to(shards[-1].device)
            torch.cuda.synchronize(G - 1)
            assert node.search_in(shards) is True
            with torch.cuda.device(G - 1):
                ss.fill_random_device(shards[-1], 0x5EED0001, begins[-1])
                torch.cuda.synchronize()
    node.close()


def _run_bench(args, env_extra, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus N` must never print an n_gpus-1 line under an N-GPU label."""
    import torch
    n = torch.cuda.device_count() + 1
    out = _run_bench(["--gpus", str(n), "--steps", "2", "--warmup", "1"], {})
    assert out.returncode != 0
    assert out.stdout.strip() == "", out.stdout
    assert "only %d HIP device(s) visible" % (n - 1) in out.stderr


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it starts 2 ranks itself.  On a one-GPU box the two
    ranks share cuda:0 and the flag travels over gloo (SS_BENCH_SHARE_GPU / SS_BENCH_BACKEND); on a multi-GPU
    box it is the real thing: native RCCL, one rank per device."""
    import json
    import torch
    multi = torch.cuda.device_count() >= 2
    extra = {} if multi else {"SS_BENCH_SHARE_GPU": "1", "SS_BENCH_BACKEND": "gloo"}
    out = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--haystack-gib", "0.5", "--no-ceiling"], extra)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and d["config"]["launcher"] == "self"
    assert d["config"]["ranks_share_one_gpu"] is (not multi)
    if multi:
        assert d["config"]["rccl_ranks"] == 2 and d["config"]["transport"] == "rccl"
    assert d["config"]["haystack_bytes"] == 1 << 29 and d["config"]["shard_bytes"] == (1 << 28) + 15
    assert d["value"] > 0 and "cpu_baseline" not in d


def test_bench_native_rccl_path_with_one_rank():
    """The N > 1 code path of bench.py (ShardedSearcher over the native RCCL transport: ss_comm_init_rank,
    ss_search_sharded, ncclCommCount) with the only rank count a one-GPU box allows."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SS_BENCH_FORCE_DIST="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--haystack-gib", "2", "--no-cpu-baseline", "--no-configs", "--no-ceiling"],
                         capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["transport"] == "rccl" and d["config"]["rccl_ranks"] == 1
    assert d["config"]["transport_note"] is None and d["config"]["launcher"] == "external"
    assert d["roofline"]["achieved"] > 3000 and abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / 8000.0) < 1e-3


def _line(out):
    import json
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


QUICK = ["--no-cpu-baseline", "--no-configs", "--no-ceiling", "--no-traffic"]


@pytest.mark.timing
def test_bench_short_timed_region_runs_on_settled_clocks():
    """at 8 GPUs a step is ~1.2 ms, so 5 warm-up + 20 timed steps are shorter than the clocks' ramp after an
    idle gap; bench.py therefore spins search_in for >= 100 ms first.  On an 8 GiB haystack (one rank's shard at 8 GPUs) 20 timed
    steps must report what 200 report.  Noise model (profiles/r05/timing_test_spread.jsonl, 10 runs): short / long = 0.984-1.002,
    median 0.999 (two PROCESSES: their placement alone moves a rate by 1-2 %); the bar is 2 %, and a pair that is off is measured again
    (three pairs at most)."""
    pairs = []
    for attempt in range(3):                              # (two processes: their placement alone moves a rate by 1-2 % on one box -
        short = _line(_run_bench(["--haystack-gib", "8", "--steps", "20", "--warmup", "5"] + QUICK, {}))       # profiles/r04/README.md -
        long_ = _line(_run_bench(["--haystack-gib", "8", "--steps", "200", "--warmup", "5"] + QUICK, {}))      # so a pair that is off is
        assert short["config"]["prewarm_ms"] >= 100 and short["config"]["prewarm_steps"] >= 8                  # measured again)
        pairs.append((short["value"], long_["value"]))
        timing_log("bench_short_vs_long", short_over_long=round(short["value"] / long_["value"], 4))
        if abs(short["value"] / long_["value"] - 1) < 0.02:
            break
    else:
        raise AssertionError("20 timed steps never came within 2 %% of 200: %r" % (pairs,))
    assert short["roofline"]["kernel_ms"] <= short["roofline"]["kernel_ms_avg"] * 1.02        # the median is the reported statistic
    assert short["roofline"]["kernel_launches"] == 20


def test_bench_single_process_mode_and_the_fallback_to_it():
    """`--single-process --gpus G` (every visible G): one process, ncclCommInitAll, grouped all-reduce.  And the automatic fallback:
    when the ranks' bootstrap fails (SS_BENCH_FAIL_DIST_INIT=1 makes it) rank 0 runs that form and says so."""
    import torch
    for G in range(1, torch.cuda.device_count() + 1):
        d = _line(_run_bench(["--single-process", "--gpus", str(G), "--haystack-gib", "2", "--steps", "5", "--warmup", "2"] + QUICK, {}))
        assert d["n_gpus"] == G and d["config"]["launcher"] == "single-process" and d["config"]["ranks"] == G
        assert d["config"]["transport"].startswith("rccl") and d["config"]["transport_note"] is None
        assert d["config"]["haystack_bytes"] == 2 << 30 and d["value"] > 1000
    env = {"SS_BENCH_FORCE_DIST": "1", "SS_BENCH_FAIL_DIST_INIT": "1", "WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0",
           "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29578"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--haystack-gib", "2", "--steps", "5", "--warmup", "2"] + QUICK,
                         capture_output=True, text=True, timeout=900, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env), cwd=ROOT)
    d = _line(out)
    assert d["config"]["launcher"] == "single-process" and "bootstrap failed" in d["config"]["transport_note"]
    assert d["n_gpus"] == 1 and d["value"] > 1000


def test_live_bench_line_contract_and_measured_traffic():
    """The line of a --full run (smaller haystack, same code path): every contract field, the roofline block's arithmetic, and
    roofline.traffic MEASURED in the run (a child `rocprofv3 --pmc FETCH_SIZE` pass) rather than a stored ratio."""
    d = _line(_run_bench(["--full", "--haystack-gib", "4", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-configs"], {}, timeout=1200))
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str),
                     ("data", str), ("config", dict), ("roofline", dict)):
        assert key in d and isinstance(d[key], typ), key
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / r["kernel_ms"] / 1e6) < 1.0
    assert r["traffic_source"].startswith("measured in this run"), r.get("traffic_note") or r["traffic_source"]
    assert 0.99 <= r["traffic_per_algorithmic_byte"] <= 1.05, r["traffic_per_algorithmic_byte"]
    assert abs(r["traffic"] - r["traffic_per_algorithmic_byte"] * r["algorithmic_bytes_per_launch"]) < 1e-3 * r["traffic"]


def test_plain_bench_run_times_the_headline_only_and_dumps_its_answers(tmp_path):
    """Without --full the run sets up, warms up, times --steps steps and prints the line: no read ceiling, other configs, CPU baseline
    or live traffic pass.  --dump-outputs DIR holds what search_in returned in the last timed step (the needle is absent) and its
    answers to the seeded planted cases: true where the needle went in whole, false for the near misses."""
    import importlib.util
    import numpy as np
    import sliceslice_rs_amd as ss
    d = _line(_run_bench(["--haystack-gib", "2", "--steps", "7", "--warmup", "1", "--dump-outputs", str(tmp_path)], {}))
    assert d["steps"] == 7 and d["roofline"]["kernel_launches"] == 7 and d["ms_per_step"] > 0 and d["value"] > 1000
    assert not {"cpu_baseline", "configs", "configs_summary"} & set(d) and "read_ceiling_gbps" not in d["roofline"]
    assert d["roofline"]["traffic_source"].startswith("stored ratio")
    found, planted = np.load(tmp_path / "found.npy"), np.load(tmp_path / "planted.npy")
    assert found.dtype == planted.dtype == np.float32 and found.tolist() == [0.0]
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    want = [float(c[2]) for c in bench.planted_cases(bench.absent_needle(ss, 16), d["config"]["haystack_bytes"])]
    assert planted.tolist() == want and 0.0 in want and 1.0 in want, (planted.tolist(), want)


# ---- the NATIVE collective code with more than one rank, on one GPU ----------------------------------------------------------
# Real RCCL refuses two ranks on one device, so on a one-GPU box ss_search_sharded / ss_find_sharded / the RCCL branch of
# ss_search_sharded_all had only ever executed with nranks == 1 - and the first real multi-rank run is the driver's, unattended.
# tests/native/fake_rccl.c implements the nine nccl* symbols the library resolves over POSIX shared memory; the library loads it
# instead of librccl when SLICESLICE_RCCL_LIB names it.  Every worker below is a process of its own (the variable is read once).

def _fake_env(extra=None):
    build = sys.modules.get("sliceslice_rs_amd._build")
    if build is None:
        import sliceslice_rs_amd  # noqa: F401
        build = sys.modules["sliceslice_rs_amd._build"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SLICESLICE_RCCL_LIB=build.build_fake_rccl(), FAKE_RCCL_TIMEOUT_S="240")
    env.update(extra or {})
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return env, build


def _run_ranks(world, loops, env, tmp_path, timeout=1500):
    worker = os.path.join(ROOT, "tests", "_native_ranks_worker.py")
    id_file = str(tmp_path / ("uid_%d_%d" % (world, loops)))
    procs = [subprocess.Popen([sys.executable, worker, "rank", str(r), str(world), id_file, str(loops)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise AssertionError("a rank hung (rank outputs so far: %r)" % (outs,))
    for r, (p, (out, err)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("rank %d of %d ok" % (r, world)) in out, "rank %d: %s %s" % (r, out[-1500:], err[-3000:])
    return [o for o, _ in outs]


@pytest.mark.parametrize("world", [2, 3, 8])
def test_native_collectives_with_several_ranks_on_one_gpu(world, tmp_path):
    """ss_comm_init_rank / ss_search_sharded / ss_find_sharded from 2, 3 and 8 PROCESSES sharing cuda:0, the product library on
    the native transport: absent; a match in every rank's shard, at both ends, straddling every boundary by 1 .. n-1 bytes; two
    matches (leftmost wins); shards shorter than the needle; 10,000 back-to-back searches (epochs, the every-256th stream wait, the
    answer word behind the all-reduce) with the needle turning up on one rank now and then."""
    env, _ = _fake_env()
    outs = _run_ranks(world, 10000 if world <= 3 else 4000, env, tmp_path)
    assert "0 injected failures" in outs[0]


@pytest.mark.parametrize("world", [2, 8])
def test_native_collectives_survive_a_failing_rank(world, tmp_path):
    """The same against the hooks build, plus: ss_debug_fail_next_scans on the last rank -> that rank returns its own error, every
    other rank SS_ERR_PEER, nobody is left in the all-reduce, the next search finds all ranks in step; and the 2^31 epoch wrap
    of the communicator's flag pair crossed by all ranks together."""
    env, build = _fake_env()
    env["SLICESLICE_HIP_LIB"] = build.build_tuning()
    outs = _run_ranks(world, 300, env, tmp_path)
    assert all("3 injected failures" in o for o in outs)


def test_a_collective_slower_than_the_spin_budget_still_gives_the_answer(tmp_path):
    """a sharded search whose bounded spin on the answer words runs out - a first ncclAllReduce that connects
    lazily, a rank that arrives late - must collect the words behind the drain, not read a buffer nobody wrote.  The stand-in's every
    third all-reduce sleeps 3 ms (the budget for these shards is ~0.5 ms): the single-process set of three devices and two
    processes of the pair form, hooks build, every answer as without the delay - and the late path WAS taken (ss_debug_late_answers)."""
    import re
    env, build = _fake_env({"FAKE_RCCL_SLOW_US": "3000", "FAKE_RCCL_SLOW_EVERY": "3"})
    env["SLICESLICE_HIP_LIB"] = build.build_tuning()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_native_ranks_worker.py"), "set", "3"], capture_output=True,
                         text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0 and "set of 3 ok" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
    assert int(re.search(r"(\d+) late answers", out.stdout).group(1)) >= 100, out.stdout[-300:]
    outs = _run_ranks(2, 600, env, tmp_path)
    assert all(int(re.search(r"(\d+) late answers", o).group(1)) >= 3 for o in outs), outs


@pytest.mark.parametrize("G", [3, 8])
def test_single_process_set_with_the_grouped_all_reduce_on_one_gpu(G):
    """ss_comm_init_all / ss_search_sharded_all / ss_find_sharded_all with G = 3 and 8 shards on one GPU: ncclCommInitAll, the G
    all-reduces inside one ncclGroupStart/End, the read-back from device 0 - against the host combine, with matches at 0, at the
    end and across every shard edge, 600 back-to-back searches per mode."""
    env, _ = _fake_env()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_native_ranks_worker.py"), "set", str(G)], capture_output=True,
                         text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0 and ("set of %d ok" % G) in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
    env, build = _fake_env()
    env["SLICESLICE_HIP_LIB"] = build.build_tuning()                            # once more with the epoch wrap (a hook)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_native_ranks_worker.py"), "set", str(G)], capture_output=True,
                         text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0 and ("set of %d ok" % G) in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.timing
def test_cross_device_early_exit_of_the_single_process_search():
    """A match on ONE device ends the other devices' scans too (tests/_native_ranks_worker.py relay_main): three shards of 3 GiB
    on one GPU, the needle at the start of shard 0 - with the host's relay the call returns in well under 0.6 of the time it
    takes with SLICESLICE_CROSS_EXIT=0.  Noise model (profiles/r05/timing_test_spread.jsonl, 10 runs): 0.109-0.113 ms with the relay,
    1.01-1.18 ms without - a ratio of 0.09-0.11 against the bar of 0.6."""
    env, build = _fake_env()
    env["SLICESLICE_HIP_LIB"] = build.build_tuning()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_native_ranks_worker.py"), "relay"], capture_output=True,
                         text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0 and "relay ok" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
    timing_log("cross_device_relay", line=[l for l in out.stdout.splitlines() if l.startswith("relay ok")][-1])


def test_bench_with_eight_ranks_on_the_native_transport():
    """`python bench.py --gpus 8` end to end the way the driver launches it - bench.py starts the ranks itself - with all eight on
    cuda:0: torch.distributed (gloo) for the bootstrap only, the searches through ss_comm_init_rank / ss_search_sharded over the
    stand-in.  The line must say 8 ranks, the native transport, and that the ranks shared one GPU (its GB/s mean nothing)."""
    import json
    env, _ = _fake_env({"SS_BENCH_SHARE_GPU": "1", "SS_BENCH_BACKEND": "gloo"})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "20", "--warmup", "5",
                          "--haystack-gib", "2", "--no-ceiling", "--full"], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["config"]["ranks"] == 8 and d["config"]["rccl_ranks"] == 8
    assert d["config"]["transport"].startswith("rccl") and d["config"]["transport_note"] is None
    assert d["config"]["ranks_share_one_gpu"] is True
    # the line names the collective library its communicator is made of - here the stand-in, by path and by the
    # version only it reports (a real run shows torch's or the system's librccl and RCCL's own version, e.g. 22606)
    assert d["config"]["librccl_path"].endswith("libfake_rccl.so") and d["config"]["librccl_version"] == 1, d["config"]
    assert d["config"]["librccl_env"] == env["SLICESLICE_RCCL_LIB"]
    assert d["config"]["haystack_bytes"] == 2 << 30 and d["config"]["shard_bytes"] == (2 << 30) // 8 + 15
    assert d["value"] > 0 and d["roofline"]["kernel_launches"] == 20
    # the N > 1 line explains itself.  Both forms ran - one rank per GPU (launched by bench.py itself) and all
    # "GPUs" from one process - the better one is the line, the other sits under config.other_form with its own figures ...
    other = d["config"]["other_form"]
    assert {d["config"]["launcher"], other["launcher"]} == {"self", "single-process"}, (d["config"]["launcher"], other)
    assert other["value"] > 0 and other["value"] <= d["value"] and other["rccl_ranks"] == 8      # (ncclCommCount of every communicator)
    # ... every rank's (device's) kernel times are there, and a step is split into the slowest rank's kernel and the rest
    for form in (d["roofline"]["per_rank"], other["per_rank"]):
        assert [r["rank"] for r in form] == list(range(8))
        assert all(0 < r["kernel_ms_min"] <= r["kernel_ms_median"] <= r["kernel_ms_max"] and r["launches"] == 20 for r in form)
    for sb, ms in ((d["step_breakdown"], d["ms_per_step"]), (other["step_breakdown"], other["ms_per_step"])):
        assert abs(sb["kernel_ms_slowest_rank"] + sb["outside_kernel_ms"] - ms) < 2e-3 and sb["kernel_ms_slowest_rank"] > 0
    multi, single = (d, other) if d["config"]["launcher"] == "self" else (other, d)
    mb = multi["step_breakdown"]
    assert mb["small_shard_sharded_call_us"] > mb["small_shard_plain_call_us"] > 0
    assert abs(mb["collective_only_us"] - (mb["small_shard_sharded_call_us"] - mb["small_shard_plain_call_us"])) < 0.2
    iss = single["step_breakdown"]["issue_us"]
    assert iss["all"] > 0 and iss["scans"] > 0 and single["step_breakdown"]["small_shard_call_us"] > 0
    # ... and the line says which workgroups-per-CU setting the timed launches ran with (a 256 MiB shard: census territory)
    for form in (d["config"]["workgroups_per_cu_timed"], other["workgroups_per_cu_timed"]):
        assert set(form) <= {"4", "6"} and sum(form.values()) == 20
