"""What the limb-lane kernel's GPU test files share (test_gpu_limb*.py): the fixtures, the library's run-time
switches, its counters, and the runners of a fused batch, a mixed plan and forces mode. Not a test module: the
test files import from it by name (the `gpu` and `hmodels` fixtures included)."""
import contextlib
import os

import numpy as np
import pytest

from conftest import MODELS

OUTS = ("tau", "cf", "flags", "work_cot")
# the library's switches per mapping (the tile runs: every launch length takes the tile mapping)
TILE = dict(HS_LIMB="1", HS_LIMB_TILE="1", HS_LIMB_TILE_MIN="1")
PACKED = dict(HS_LIMB="1", HS_LIMB_TILE="0")
ROLLOUT = dict(HS_LIMB="0")


@pytest.fixture(scope="module")
def gpu(product):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return product


@pytest.fixture(scope="module")
def hmodels(gpu):
    return {n: gpu.KinematicModel(os.path.join(MODELS, f"{n}.xml")) for n in ("hexapod", "spider", "myant")}


@contextlib.contextmanager
def env(**switches):
    """the library's run-time switches (read from the environment on every call) set or, at None, removed for
    the block, then put back as the caller had them"""
    old = {k: os.environ.get(k) for k in switches}
    for k, v in switches.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def product_route(**switches):
    """the switches of the product's route: every HS_LIMB* switch (HS_LIMB_TILE* among them) out of the
    environment, `switches` set"""
    return {**{k: None for k in os.environ if k.startswith("HS_LIMB")}, **switches}


@contextlib.contextmanager
def counted(gpu, switches):
    """`switches` for the block; the dict it yields gets how far the block moved the library's counters: limb,
    tile, planned and looped launches and deferred steps"""
    api = gpu.api
    read = dict(limb_launches=api.limb_launches, tile_launches=api.limb_tile_launches,
                plan_launches=api.limb_tile_plan_launches, loop_launches=api.limb_tile_loop_launches,
                deferred=api.limb_deferred)
    c = {}
    with env(**switches):
        c0 = {k: f() for k, f in read.items()}
        yield c
        c.update({k: f() - c0[k] for k, f in read.items()})


def fused_calls(gpu, make, switches, K, Hc=1, nan_fill=False):
    """K fused calls of Hc steps (hs_run_calls / hs_run_mixed_calls) with the best key on the batch make()
    builds under `switches`, its tau and cf NaN first where nan_fill: the outputs on the host, the raw key and
    the counters"""
    import torch

    with counted(gpu, switches) as c:
        b = make()
        if nan_fill:
            for k in ("tau", "cf"):
                getattr(b, k).fill_(float("nan"))
        b.key_steps = K * Hc
        b.work_cot.zero_()
        b.reset_best()
        b.run_calls(K, call_horizon=Hc, best=True, accumulate=True)
        torch.cuda.synchronize()
        out = {k: getattr(b, k).cpu().numpy() for k in OUTS}
        out["best_key"] = int(b.best_key.item())
    out.update(c)
    return out


def run(gpu, model, params, switches, K, Hc=1, k0=0, n_t=20, dtype=None, **more):
    """fused_calls on a DeviceBatch of one model, `more` switches on top of `switches`"""
    return fused_calls(gpu, lambda: gpu.DeviceBatch(model, params, n_t=n_t, k0=k0, horizon=K * Hc, outputs=OUTS, dtype=dtype),
                       dict(switches, **more), K, Hc)


def run_mixed(gpu, models, idx, params, switches, K, Hc=1, dtype=None):
    """fused_calls on a MixedBatch (synth.gen_mixed's params and idx) whose tau and cf start as NaN"""
    return fused_calls(gpu, lambda: gpu.MixedBatch(models, idx, params, n_t=20, k0=0, horizon=K * Hc, outputs=OUTS, dtype=dtype),
                       switches, K, Hc, nan_fill=True)


def forces_tau(gpu, model, params, K, Hc=1):
    """forces mode's input: the control run's torques of K calls of Hc steps, perturbed per step and joint"""
    import torch

    ctl = gpu.DeviceBatch(model, params, n_t=20, k0=0, horizon=K * Hc, outputs=("tau",))
    ctl.run_calls(K, call_horizon=Hc)
    i = torch.arange(K * Hc, device=ctl.tau.device)[None, :, None]
    j = torch.arange(model.nmj, device=ctl.tau.device)[None, None, :]
    return ctl.tau + 0.2 * torch.sin(0.7 * i + 1.3 * j)


def run_forces(gpu, model, params, tau, switches, K, Hc=1):
    """solve_forces (hs_run_forces_calls) on `tau` under `switches`: cf (NaN first), flags and the counters"""
    import torch

    with counted(gpu, switches) as c:
        fb = gpu.DeviceBatch(model, params, n_t=20, k0=0, horizon=K * Hc, outputs=("cf", "flags"))
        fb.cf.fill_(float("nan"))
        fb.forces_launcher(tau, K, call_horizon=Hc)()
        torch.cuda.synchronize()
        out = dict(cf=fb.cf.cpu().numpy(), flags=fb.flags.cpu().numpy())
    out.update(c)
    return out


def same(a, b, what, outs=OUTS, deferred=False):
    """the outputs bitwise, the best key where the runs have one, and (deferred) as many deferred steps"""
    for k in outs:
        assert np.array_equal(a[k], b[k], equal_nan=True), \
            f"{what}: {k} differs on {int((a[k] != b[k]).sum())} entries (max {np.nanmax(np.abs(a[k].astype(float) - b[k].astype(float))):.3e})"
    if "best_key" in a:
        assert a["best_key"] == b["best_key"], what
    if deferred:
        assert a["deferred"] == b["deferred"], f"{what}: {a['deferred']} steps deferred against {b['deferred']}"
