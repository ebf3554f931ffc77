"""bench.py --gpus N launches N ranks: the parent starts
torch.distributed.run as a child before any GPU call, every rank checks WORLD_SIZE == N, the
rollouts are sharded in contiguous ranges, and one all-reduce(MIN) of the 8-byte key picks the
global winner. --stub-cpu runs that skeleton on CPU ranks over gloo with a stub in place of the
kernel (the GPU run uses the same functions with RCCL and the HIP kernel)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def run_bench(*argv, env=None, timeout=240):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                          timeout=timeout, env=e, cwd=ROOT)


@pytest.mark.parametrize("world,total", [(2, 1000), (3, 1001)])
def test_gpus_n_spawns_n_ranks_with_distinct_shards(world, total):
    r = run_bench("--gpus", str(world), "--stub-cpu", "--steps", "3", "--warmup", "1", "--total-rollouts",
                  str(total))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout  # rank 0 prints one JSON line
    out = json.loads(line[0])
    assert out["n_gpus"] == world and out["scaling"] == "strong"
    # between the two clock reads only the best-key all-reduce (bench.timed_window; VERDICT r05 item 3:
    # no barrier inside the window, the slowest rank is the MAX all-reduce of elapsed afterwards)
    assert out["collectives_in_timed_window"] == 1
    shards = sorted(out["stub_shards"])
    assert [s[0] for s in shards] == list(range(world))
    assert len({s[3] for s in shards}) == world  # one process per rank
    pos = 0
    for _, id0, count, _ in shards:  # contiguous, disjoint, covering [0, total)
        assert id0 == pos and count > 0
        pos += count
    assert pos == total
    # the global winner: the stub's per-cycle COT over ALL rollouts, ties to the lowest id
    from hslabs_amd import dist as hdist
    from hslabs_amd import synth

    p = synth.gen_params(total, "hexapod")
    work = torch.from_numpy(p["period"] * p["step_height"] * (3 / 20))
    sel = hdist.select_cot(work, torch.from_numpy(p["step_length"]), 22.0, 20, 3).numpy()
    want = int(np.nanargmin(sel.astype(np.float32)))
    assert out["best_rollout"]["id"] == want
    assert abs(p["step_length"][want]) >= 1e-3


def test_default_layout_is_configs3_over_ranks():
    import bench

    a = bench.parse(["--gpus", "8"])
    lay = [bench.job_layout(a, 8, r) for r in range(8)]
    assert all(l["cfg"] == "configs[3]" and l["B"] == 32768 and l["scaling"] == "strong" for l in lay)
    assert [l["id0"] for l in lay] == [32768 * r for r in range(8)]
    one = bench.job_layout(bench.parse([]), 1, 0)
    assert one["cfg"] == "configs[1]" and one["B"] == 4096
    weak = bench.job_layout(bench.parse(["--gpus", "2", "--rollouts", "4096"]), 2, 1)
    assert weak["scaling"] == "weak" and weak["id0"] == 4096 and weak["B"] == 4096


def test_world_size_mismatch_is_an_error():
    r = run_bench("--gpus", "2", "--stub-cpu", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_committed_pmc_summary_is_keyed_to_the_driver_workload():
    """bench.py attaches the committed PMC traffic (profiles/pmc_traffic.json: one summary per workload)
    only to the workload key it was taken on and only for the library hash it records: configs[1] (the
    driver's run, bench.py --gpus 1 --steps 20 --warmup 5), configs[2] and configs[4]."""
    sys.path.insert(0, ROOT)
    import bench

    j = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["workloads"]
    # bench.py's traffic keys, with each workload's algorithmic bytes per bench step
    for key, alg in (("hexapod B=4096 H=1", 1_572_864), ("spider B=16384 H=32 fp32", None),
                     ("mixed B=4096 H=1 fp64", None)):
        e = j[key]
        assert e["workload"] == key and len(e["lib_sha256"]) == 16
        if alg:
            assert e["hbm_bytes_per_step"] > alg  # >= the algorithmic bytes
        got, why = bench.pmc_for(key, e["lib_sha256"])
        assert got is not None and got["hbm_bytes_per_step"] == e["hbm_bytes_per_step"], why
        assert bench.pmc_for(key, "0" * 16)[0] is None  # another library: refused
    assert bench.pmc_for("hexapod B=1 H=1", j["hexapod B=4096 H=1"]["lib_sha256"])[0] is None  # no summary


def test_every_bench_mode_times_through_timed_window():
    """the control loop, solve_forces and the simulation all time through bench.timed_window (clock, job,
    synchronize, clock), which issues no collective of its own; the stub's count above covers it"""
    import inspect

    sys.path.insert(0, ROOT)
    import bench

    src = inspect.getsource(bench)
    assert src.count("timed_window(") == 5  # the definition, the stub, main, main_forces, main_sim
    assert src.count("time.perf_counter() - t0") == 3  # the three CPU-baseline loops only
    calls = []
    el = bench.timed_window(lambda: calls.append("job"), lambda: calls.append("sync"))
    assert calls == ["job", "sync"] and el >= 0


def test_full_and_dump_outputs_are_off_by_default():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_last_step_rows_of_a_packed_output_buffer():
    """hs_run_calls packs [B][K * H][d] from the buffer's start, whatever rows the buffer was allocated with"""
    import bench

    B, K, H, d, alloc = 5, 3, 2, 4, 8
    buf = torch.full((B, alloc, d), -1.0, dtype=torch.float64)
    packed = torch.arange(B * K * H * d, dtype=torch.float64).view(B, K * H, d)
    buf.view(-1)[:packed.numel()] = packed.view(-1)
    assert torch.equal(bench.last_step_rows(buf, B, K * H, H), packed[:, (K - 1) * H:])
    flags = torch.arange(B * alloc, dtype=torch.int32).view(B, alloc)
    assert torch.equal(bench.last_step_rows(flags, B, K * H, H), flags.view(-1)[:B * K * H].view(B, K * H)[:, -H:])


def test_dump_outputs_formats_and_seeded_sample(tmp_path, monkeypatch):
    import bench

    g = torch.Generator().manual_seed(1)
    arrays = {"tau": torch.randn(100, 2, 3, generator=g), "cf": torch.randn(100, 2, 6, generator=g).double(),
              "flags": torch.arange(200, dtype=torch.int32).view(100, 2), "best_key": torch.tensor([0.5, 7.0]),
              "none": None}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = {f: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert set(got) == {"tau.npy", "cf.npy", "flags.npy", "best_key.npy"}
    assert got["tau.npy"].dtype == np.float32 and got["cf.npy"].dtype == np.float64
    assert got["flags.npy"].dtype == np.float64 and np.array_equal(got["flags.npy"], arrays["flags"].numpy())
    assert np.array_equal(got["tau.npy"], arrays["tau"].numpy())
    # over the budget: the same seeded rollouts of every per-rollout array, the same in a second run
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, rank=1, world=2)
    s1 = {f: np.load(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")}
    s2 = {f: np.load(tmp_path / "s2" / f) for f in os.listdir(tmp_path / "s2")}
    assert set(s1) == {n + ".rank1.npy" for n in ("tau", "cf", "flags", "best_key", "rollout_rows")}
    assert sum(a.nbytes for a in s1.values()) <= 4000
    rows = s1["rollout_rows.rank1.npy"].astype(int)
    assert 1 <= len(rows) < 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(s1["cf.rank1.npy"], arrays["cf"].numpy()[rows])
    assert np.array_equal(s1["best_key.rank1.npy"], arrays["best_key"].numpy())
    assert all(np.array_equal(s1[f], s2[f]) for f in s1)
