"""bench.py on the GPU: a plain run prints the headline line only, --full adds the untimed checks
(and, unless --no-cpu, the CPU baseline), and --dump-outputs writes what the timed job computed in
its last step: the same numbers a caller of hs_run_calls gets for that step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import MODELS, ROOT

pytestmark = pytest.mark.gpu

B, K, W = 300, 3, 5  # more than one block, no multiple of the wavefront's 8 rollouts; warmup rows > timed rows
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("best_rollout", "nan_steps", "cpu_baseline")


@pytest.fixture(scope="module")
def gpu(product):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return product


@pytest.fixture(scope="module")
def direct(gpu):
    """the K fused steps of the bench's batch through the package, run once for both cases"""
    import torch

    from hslabs_amd import dist as hdist
    from hslabs_amd import synth

    model = gpu.KinematicModel(os.path.join(MODELS, "hexapod.xml"))
    b = gpu.DeviceBatch(model, synth.gen_params(B, "hexapod"), n_t=20, k0=0, horizon=K,
                        outputs=("tau", "cf", "work_cot", "flags"))
    b.work_cot.zero_()
    b.reset_best()
    b.key_steps = K
    b.run_calls(K, call_horizon=1, best=True, accumulate=True)
    torch.cuda.synchronize()
    cot, rid = hdist.decode(b.best_key ^ hdist._FLIP)
    return {"best_key": np.array([cot, rid], np.float64),
            "tau": b.tau[:, K - 1:].cpu().numpy(), "cf": b.cf[:, K - 1:].cpu().numpy(),
            "flags": b.flags[:, K - 1:].cpu().numpy().astype(np.float64), "work_cot": b.work_cot.cpu().numpy()}


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_bench_line_and_dumped_outputs(direct, tmp_path, full):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--rollouts", str(B), "--dump-outputs", str(tmp_path)] + (["--full", "--no-cpu"] if full else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE)
    assert out["steps"] == K and out["unit"] == "steps/s" and out["dtype"] == "f64" and out["higher_is_better"]
    # value = rollouts x steps / elapsed, ms_per_step = elapsed / steps, rounded to 1e-4 ms in the line
    assert out["ms_per_step"] > 0 and abs(out["ms_per_step"] - B * 1e3 / out["value"]) <= 1e-4
    if full:
        assert out["nan_steps"] == 0 and out["cpu_baseline"] is None
        assert 0 <= out["best_rollout"]["id"] < B
    else:
        assert not any(k in out for k in FULL_ONLY)
    got = {os.path.splitext(f)[0]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"tau", "cf", "flags", "work_cot", "best_key"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for name, want in direct.items():
        assert got[name].shape == want.shape, name
        assert np.array_equal(got[name], want, equal_nan=True), name  # the same kernels on the same inputs
    assert 0 <= got["best_key"][1] < B and np.isfinite(got["best_key"][0])
