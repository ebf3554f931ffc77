"""What the closed-loop simulation's GPU test files share (test_gpu_sim*.py, test_gpu_cpc.py): the fixtures,
the model dictionaries, the batch makers, the readers of a batch's tables and outputs, the moved batches of
the dynamics and CPC tests, and the body bound every one of them holds. Not a test module: the test files
import from it by name (the fixtures included)."""
import os

import numpy as np
import pytest

from conftest import MODELS, PGS_CONFIG
from test_sim_dynamics import CASES, MOVE_STEPS, TSI0

BODY_TOL = 1e-10   # body state and torso against the oracle (measured ~1e-13 after 100 steps)
NEVER = 10 ** 6    # a check_from no run reaches: the trial kernel without its fall check


@pytest.fixture(scope="module")
def gpu(product):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return product


@pytest.fixture(scope="module")
def hmodels(gpu):
    return {n: gpu.KinematicModel(os.path.join(MODELS, f"{n}.xml")) for n in ("hexapod", "spider", "myant")}


@pytest.fixture(scope="module")
def models(gpu):
    """name -> (model, its pgs setup) of tests/test_sim_dynamics.py's CASES"""
    return {name: (gpu.KinematicModel(os.path.join(MODELS, f"{name}.xml")), gpu.read_pgs_config(PGS_CONFIG, pid))
            for name, pid in CASES.items()}


def tables(sb):
    """the controller tables q, dq, tau on the host, as float64 whatever the batch's precision"""
    return [t.cpu().numpy().astype(np.float64) for t in (sb.tables.q, sb.tables.dq, sb.tables.tau)]


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def make_batch(gpu, model, name, B, period=3.0, **kw):
    """B rollouts of synth.gen_sim_params"""
    from hslabs_amd import synth

    return gpu.SimBatch(model, synth.gen_sim_params(B, name, period=period), **kw)


def batch(gpu, model, p, B, **kw):
    """B rollouts of the pgs setup p, at rest at trajectory sample TSI0"""
    return gpu.SimBatch(model, [p] * B, tsi0=TSI0, **kw)


def new_batch(gpu, models, name, dtype=None, n=len(MOVE_STEPS)):
    m, p = models[name]
    return gpu.SimBatch(m, [p] * n, tsi0=TSI0, dtype=dtype)


def moved(gpu, models, name, dtype=None):
    """A batch whose rollout i has taken MOVE_STEPS[i] position-control steps, the tracker pushed before
    every one of them (float64), and the last torques of each rollout. Returns (batch, tau0, history)
    with history = the bodies before each of the 25 steps [25][B][n][13]."""
    import torch

    B = len(MOVE_STEPS)
    sb = new_batch(gpu, models, name, dtype)
    f64 = sb.dtype == torch.float64
    nmj = sb.model.nmj

    def snap(tau):
        return sb.body.clone(), sb.seed.clone(), sb.tsi.clone(), sb.ders.clone(), tau

    snaps, hist = {0: snap(torch.zeros((B, nmj), dtype=sb.dtype, device=sb.device))}, []
    for i in range(max(MOVE_STEPS)):
        hist.append(sb.body.clone())
        if f64:
            sb.track_push()
        o = sb.step(1, outputs=("tau_cmd",))
        if i + 1 in MOVE_STEPS:
            snaps[i + 1] = snap(o["tau_cmd"][:, -1].clone())
    tau0 = torch.empty((B, nmj), dtype=sb.dtype, device=sb.device)
    for i, n in enumerate(MOVE_STEPS):
        body, seed, tsi, ders, tau = snaps[n]
        sb.body[i], sb.seed[i], sb.tsi[i], sb.ders[i], tau0[i] = body[i], seed[i], tsi[i], ders[i], tau[i]
    sb.last_tau = tau0
    torch.cuda.synchronize()
    return sb, tau0, torch.stack(hist)


@pytest.fixture(scope="module")
def moved64(gpu, models):
    """name -> (batch, tau0, history); read only: tests copy what they advance"""
    return {name: moved(gpu, models, name) for name in CASES}


def copy_state(dst, src):
    dst.body.copy_(src.body)
    dst.seed.copy_(src.seed)
    dst.tsi.copy_(src.tsi)
    dst.ders.copy_(src.ders)
    dst.last_tau = None if src.last_tau is None else src.last_tau.clone()
    return dst
