"""bench.py's control flow for N > 1 (sharded stepping, one all-to-all per tick, convergence section,
the JSON contract) driven on CPU: two gloo ranks, CPU tensors and — injected by THIS test, bench.py itself
never touches it outside its cpu_baseline leg — the oracle library behind the same C ABI.  It guards the
driver's multi-GPU run, which cannot be rehearsed here (one GPU per gpurun call)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q, extra=()):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch

    import bench
    from tests._oracle import load_oracle

    try:
        args = bench.parse_args(["--gpus", str(world), "--steps", "20", "--warmup", "10", "--nodes-per-gpu", "2048",
                                 "--view-slots", "64", "--ring", "32", "--no-cpu-baseline", "--allow-drops", "--full", *extra])
        out = bench.run(args, lib=load_oracle(), dev=torch.device("cpu"), backend="gloo")
        q.put((rank, json.dumps(out) if out is not None else "null"))
    except BaseException as e:  # noqa: BLE001
        q.put((rank, "ERR " + repr(e)))
        raise


@pytest.mark.parametrize("world", [1, 2])
def test_bench_control_flow(world):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    from tests._scenario import free_port
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    res = dict(q.get(timeout=5) for _ in procs)
    assert not any(str(v).startswith("ERR") for v in res.values()), res
    out = json.loads(res[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "rounds_to_99"):
        assert key in out, key
    assert out["n_gpus"] == world and out["steps"] == 20 and out["scaling"] == "weak" and out["vs_baseline"] is None
    assert out["value"] > 0 and out["config"]["workload"].startswith(f"{2048 * world} nodes")
    r99 = out["rounds_to_99"]
    assert 32 <= r99["n"] <= 64 and 1 <= r99["median"] <= 60 and r99["p90"] >= r99["median"] and sum(r99["histogram"].values()) == r99["n"]
    assert r99["window_ticks"][0] == 320 + 400, "the convergence window starts at a fixed tick, whatever --steps / --warmup are"
    assert set(out["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    if world > 1:
        assert all(res[r] == "null" for r in range(1, world))
    # the ONE line the driver parses: short enough that an 8 KB tail holds all of it (round 5's 21 KB line lost its head)
    sys.path.insert(0, ROOT)
    import bench
    line = bench.compact(out)
    txt = json.dumps(line)
    assert len(txt) < bench.LINE_LIMIT < 6000, len(txt)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "rounds_to_99", "detail_file"):
        assert key in line, key
    assert set(line["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"} and len(line["config"]["workload"]) <= 300
    assert line["value"] == pytest.approx(out["value"], rel=1e-4)


def test_bench_control_flow_random_fanout_on_two_ranks():
    # (r4, r5) the N > 1 line on memberlist's kRandomNodes: ShardedSim's all-to-all of the packed slabs, the JSON's exchange section
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    from tests._scenario import free_port
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, ("--fanout-model", "krandomnodes"))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    res = dict(q.get(timeout=5) for _ in procs)
    assert not any(str(v).startswith("ERR") for v in res.values()), res
    out = json.loads(res[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["fanout_model"] == "krandomnodes"
    assert out["exchange"]["collective"].startswith("equal-split all-to-all of packed slabs") and out["exchange"]["chunks"] == 2
    x = out["exchange"]
    # what leaves a rank: (V - 1) / V of its slabs; the slabs are the packets (64-byte cells) plus a few per cent (12 sigma of room,
    # a count byte per target, headers) — not the O(N) per shard of round 4's all-gather
    assert x["bytes_arriving_per_gpu_per_tick"] == x["bytes_leaving_gpu_per_tick"] == x["bytes_per_gpu_per_tick"] // 2
    assert x["bytes_per_gpu_per_tick"] < 1.4 * x["packet_bytes_per_gpu_per_tick"]   # (2 048 nodes per rank: 12 sigma is 9 % here; the oracle's slab carries 8 index bytes per packet)
    assert 1 <= out["rounds_to_99"]["median"] <= 60


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with WORLD_SIZE unset starts and supervises its ranks itself.  The
    rehearsal script runs bench.main() unchanged — argument parsing, self_launch, the watchdog — with run() handed the
    oracle library, CPU tensors and gloo (this test's doing: bench.py has no such switch)."""
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "tests", "_bench_cpu_rehearsal.py"), "--gpus", "2", "--steps", "10", "--warmup", "5",
           "--preroll", "40", "--nodes-per-gpu", "2048", "--view-slots", "64", "--ring", "32", "--no-cpu-baseline", "--no-convergence",
           "--allow-drops", "--backend", "gloo", "--full"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and "error" not in out
    assert out["distributed"]["world_size"] == 2 and out["distributed"]["backend"] == "gloo"
    # (r5) at every N the headline is the reference's kRandomNodes (one exchange of packed slabs per round), the bijection — its
    # all-to-all issued chunk-wise — next to it: the 1 -> 8 GPU series is ONE model
    assert out["config"]["fanout_model"] == "krandomnodes" and out["exchange"]["chunks"] == 2
    assert out["fanout_models"]["bijection"]["exchange"]["chunks"] == 2 and out["fanout_models"]["bijection"]["value"] > 0


def test_bench_reports_a_dead_rank_instead_of_hanging():
    """A rank that dies (here: an impossible --chunks) takes the run down with an "error" line, after one retry."""
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "tests", "_bench_cpu_rehearsal.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--preroll", "8", "--nodes-per-gpu", "2048", "--view-slots", "64", "--ring", "32", "--no-cpu-baseline", "--no-convergence",
           "--allow-drops", "--backend", "gloo", "--fanout", "9"]   # fan-out 9 does not exist: sim_create fails on every rank
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and "error" in json.loads(lines[0]) and json.loads(lines[0])["value"] is None


def test_bench_plain_run_is_the_headline_and_dumps_what_it_computed(tmp_path, monkeypatch):
    """Without --full a run measures the headline model alone; --dump-outputs writes the state of the headline cluster right
    after its last timed tick, the same in a plain and a --full run, and that state is what the workload rolled to that tick
    gives (digest)."""
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from serf_amd import _ffi
    from tests._oracle import load_oracle

    lib = load_oracle()
    common = ["--gpus", "1", "--steps", "12", "--warmup", "4", "--preroll", "40", "--nodes-per-gpu", "2048", "--view-slots", "64",
              "--ring", "32", "--allow-drops"]
    plain = bench.parse_args(common + ["--dump-outputs", str(tmp_path / "plain")])
    out = bench.run(plain, lib=lib, dev=torch.device("cpu"), backend="gloo")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == 12 and out["value"] > 0 and out["ms_per_step"] > 0 and out["config"]["fanout_model"] == "krandomnodes"
    assert list(out["fanout_models"]) == ["krandomnodes"] and out["rounds_to_99"] is None
    for key in ("long_window", "cpu_baseline", "parity", "second_load"):
        assert key not in out, key
    full = bench.parse_args(common + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    out_full = bench.run(full, lib=lib, dev=torch.device("cpu"), backend="gloo")
    assert set(out_full["fanout_models"]) == {"krandomnodes", "bijection"} and out_full["rounds_to_99"]["n"] > 0

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == ["cluster_stats.npy", "digest.npy", "members.npy", "queue.npy", "rows.npy"]
    assert sorted(os.listdir(tmp_path / "full")) == names
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.dtype == np.float64 and a.size > 0, name
        assert np.array_equal(a, b), f"{name}: a plain and a --full run dumped different outputs"
        total += a.nbytes
    assert total <= 64 << 20
    cs = np.load(tmp_path / "plain" / "cluster_stats.npy")
    assert cs[-1] == 40 + 4 + 12, "the dump is taken right after the last timed tick"

    kw, ops = bench.workload(plain, 2048, "krandomnodes")
    sim = _ffi.Sim(lib, _ffi.make_config(2048, **kw))
    for o in ops:
        sim.inject(*o)
    sim.step(40 + 4 + 12)
    want = [[x >> 32, x & 0xFFFFFFFF] for x in sim.digest()]
    rows = sim.dump(_ffi.ARR_ROWS)
    sim.close()
    assert np.load(tmp_path / "plain" / "digest.npy").tolist() == want
    got = np.load(tmp_path / "plain" / "rows.npy")
    assert got.shape == (2048, 36) and len(rows) == 2048   # (2 048 nodes: the sample is all of them, in order)
    assert got[:, 0].tolist() == (rows["clock"] >> np.uint64(32)).tolist() and got[:, 1].tolist() == (rows["clock"] & np.uint64(0xFFFFFFFF)).tolist()
    assert got[:, 10].tolist() == rows["flags"].tolist() and got[:, 20:].tolist() == rows["susp"].tolist()


def test_cpu_baseline_leaves_out_the_parity_ticks_it_cannot_reach_in_its_budget():
    """bench.py --full on a long timed region: the oracle cannot follow the GPU to the end of it in its CPU budget.  What it
    cannot reach is reported as not compared (digest None, a reason) instead of ending the run; what it reaches is compared."""
    sys.path.insert(0, ROOT)
    import bench
    from serf_amd import _ffi
    from tests._oracle import load_oracle

    args = bench.parse_args(["--steps", "12", "--warmup", "4", "--preroll", "40", "--nodes-per-gpu", "2048", "--view-slots", "64",
                             "--ring", "32"])
    args.cpu_thread_curve = False
    res, dig, why = bench.cpu_baseline(args, "krandomnodes", [44, 56], seconds_budget=120.0)
    assert res["value"] > 0 and dig[44] is not None and dig[56] is not None and why is None
    kw, ops = bench.workload(args, 2048, "krandomnodes")
    sim = _ffi.Sim(load_oracle(), _ffi.make_config(2048, **kw))
    for o in ops:
        sim.inject(*o)
    sim.step(44)
    assert tuple(dig[44]) == sim.digest()
    sim.step(12)
    assert tuple(dig[56]) == sim.digest()
    sim.close()

    far = 10 ** 7   # (hours of oracle time: never begun)
    res, dig2, why = bench.cpu_baseline(args, "krandomnodes", [44, far], seconds_budget=20.0)
    assert res["value"] > 0 and dig2[44] == dig[44] and dig2[far] is None and "not rolled" in why
    res, dig3, why = bench.cpu_baseline(args, "krandomnodes", [far, far + 12], seconds_budget=0.5)
    assert res is None and dig3 == {far: None, far + 12: None} and "not rolled" in why
