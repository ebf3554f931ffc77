"""The tile mapping's planned slot sequence (hslabs_amd/csrc/hs_limb_tile.h limb_tile_plan, read by
hs_limb_kernel's TILE instantiations from a kernel argument) against the parity order and the packed mapping.

The sequence decides which steps share a wavefront and so where a stencil row's FK is computed, never its
value: tau, cf, flags, work_cot and the best key are BITWISE the same four ways -- the default (the planner's
sequence where it saves FK passes), the planner's sequence forced (HS_LIMB_TILE_PLAN=2: also where it saves
nothing, as on myant, whose four limbs leave room for every request in the first pass), the parity order
(HS_LIMB_TILE_PLAN=0) and the packed mapping (HS_LIMB_TILE=0). hs_limb_tile_plan_launches counts the launches
on the planner's sequence: every tile launch of the forced run, none of the parity and packed runs. All tile runs set HS_LIMB_TILE_MIN=1, so every launch
length takes the tile mapping. The shapes are test_gpu_limb_tile.py's, at lengths where the planner's sequence
differs from the parity order (K = 40: four full chains' tiles and a tail tile of four segments)."""
import contextlib
import os

import numpy as np
import pytest

from conftest import MODELS

pytestmark = pytest.mark.gpu

OUTS = ("tau", "cf", "flags", "work_cot")
TILE = dict(HS_LIMB="1", HS_LIMB_TILE="1", HS_LIMB_TILE_MIN="1")
# the four runs: the library's switches (None: not in the environment)
MODES = {
    "default": dict(TILE, HS_LIMB_TILE_PLAN=None),
    "forced": dict(TILE, HS_LIMB_TILE_PLAN="2"),
    "parity": dict(TILE, HS_LIMB_TILE_PLAN="0"),
    "packed": dict(HS_LIMB="1", HS_LIMB_TILE="0", HS_LIMB_TILE_PLAN=None),
}


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


@contextlib.contextmanager
def counted(gpu, mode):
    """the switches of `mode` for the block; the dict it yields gets the block's tile launches, planned
    launches and deferred steps"""
    c = {}
    with env(**MODES[mode]):
        t0, p0, d0 = gpu.api.limb_tile_launches(), gpu.api.limb_tile_plan_launches(), gpu.api.limb_deferred()
        yield c
        c["tile_launches"] = gpu.api.limb_tile_launches() - t0
        c["plan_launches"] = gpu.api.limb_tile_plan_launches() - p0
        c["deferred"] = gpu.api.limb_deferred() - d0


def run(gpu, model, params, mode, K=40, Hc=1, k0=0, dtype=None):
    """K fused calls of Hc steps under `mode`: the outputs, the key and the counters"""
    import torch

    with counted(gpu, mode) as c:
        b = gpu.DeviceBatch(model, params, n_t=20, k0=k0, horizon=K * Hc, outputs=OUTS, dtype=dtype)
        b.key_steps = K * Hc
        b.work_cot.zero_()
        b.reset_best()
        b.run_calls(K, call_horizon=Hc, best=True, accumulate=True)
        torch.cuda.synchronize()
        out = {k: getattr(b, k).cpu().numpy() for k in OUTS}
        out["best_key"] = int(b.best_key.item())
    out.update(c)
    return out


def same(a, b, what, outs=OUTS):
    for k in outs:
        assert np.array_equal(a[k], b[k], equal_nan=True), \
            f"{what}: {k} differs on {int((a[k] != b[k]).sum())} entries (max {np.nanmax(np.abs(a[k].astype(float) - b[k].astype(float))):.3e})"
    if "best_key" in a:
        assert a["best_key"] == b["best_key"], what


def check_counters(r, what, default_planned=None):
    """the planner's sequence ran on every tile launch of the forced run and on none of the parity and packed
    runs; on `default_planned` launches of the default run where the case knows the number"""
    assert r["forced"]["tile_launches"] > 0 and r["forced"]["plan_launches"] == r["forced"]["tile_launches"], what
    assert r["default"]["tile_launches"] == r["parity"]["tile_launches"] == r["forced"]["tile_launches"], what
    assert r["parity"]["plan_launches"] == 0, what
    assert r["packed"]["tile_launches"] == 0 and r["packed"]["plan_launches"] == 0, what
    assert 0 <= r["default"]["plan_launches"] <= r["default"]["tile_launches"], what
    if default_planned is not None:
        assert r["default"]["plan_launches"] == default_planned, what


def four_ways(gpu, model, params, what, default_planned=None, **kw):
    r = {mode: run(gpu, model, params, mode, **kw) for mode in MODES}
    check_counters(r, what, default_planned)
    for mode in ("default", "forced", "parity"):
        same(r[mode], r["packed"], f"{what}: {mode} / packed")
    return r


@pytest.mark.parametrize("k0", [0, 13])
def test_full_tiles_and_a_four_segment_tail(gpu, hmodels, k0):
    """K = 40 on a hexapod: four chains of 10, a tile for the first 8 of each and the four 2-step remainders
    in the last tile (8 requests, one further pass where the parity order takes three); from k0 = 13 the
    period wraps inside the launch's first chains"""
    from hslabs_amd import synth

    p = synth.gen_params(3, "hexapod", id0=77)
    r = four_ways(gpu, hmodels["hexapod"], p, f"hexapod B=3 K=40 k0={k0}", default_planned=1, k0=k0)
    assert np.isfinite(r["default"]["tau"]).all()


def test_partial_last_tile_and_partial_batch(gpu, hmodels):
    """K = 23: the last tile idles one slot; B = 9: the second batch wavefront has one rollout"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=4321)
    four_ways(gpu, hmodels["hexapod"], p, "hexapod B=9 K=23", K=23)


@pytest.mark.parametrize("name,B,Hc,K", [("hexapod", 5, 5, 4), ("spider", 4, 32, 2)])
def test_calls_of_more_than_one_step(gpu, hmodels, name, B, Hc, K):
    """rows that advance within a call and jump between calls; configs[2]'s call shape"""
    from hslabs_amd import synth

    p = synth.gen_params(B, name, id0=31)
    four_ways(gpu, hmodels[name], p, f"{name} B={B} H={Hc} K={K}", K=K, Hc=Hc)


def test_turning_gaits(gpu, hmodels):
    """the chain bodies pushed to the lanes of the plan's neighbours"""
    from hslabs_amd import synth

    p = synth.gen_params(17, "spider", id0=5, curved=True)
    four_ways(gpu, hmodels["spider"], p, "spider curved B=17 K=40")


def test_myant_deferred_steps(gpu, hmodels):
    """ids 4717 .. 4727 (test_gpu_limb_tile.py's window with a deferring rollout): the same number of deferred
    steps under every sequence"""
    from hslabs_amd import synth

    p = synth.gen_params(11, "myant", id0=4717)
    r = four_ways(gpu, hmodels["myant"], p, "myant B=11 K=40", default_planned=0)
    n = {mode: r[mode]["deferred"] for mode in MODES}
    print(f"myant: deferred steps {n}")
    assert n["packed"] > 0 and len(set(n.values())) == 1


def test_mixed_plan(gpu, hmodels):
    """myant + hexapod wavefronts on one sequence, planned for the launch's six limb lanes"""
    import torch
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(24)
    ms = [hmodels[n] for n in synth.MIXED_MODELS]

    def go(mode):
        with counted(gpu, mode) as c:
            mb = gpu.MixedBatch(ms, idx, params, n_t=20, k0=0, horizon=40, outputs=OUTS)
            for k in ("tau", "cf"):
                getattr(mb, k).fill_(float("nan"))
            mb.key_steps = 40
            mb.work_cot.zero_()
            mb.reset_best()
            mb.run_calls(40, call_horizon=1, best=True, accumulate=True)
            torch.cuda.synchronize()
            out = {k: getattr(mb, k).cpu().numpy() for k in OUTS}
            out["best_key"] = int(mb.best_key.item())
        out.update(c)
        return out

    r = {mode: go(mode) for mode in MODES}
    check_counters(r, "mixed", default_planned=1)
    for mode in ("default", "forced", "parity"):
        same(r[mode], r["packed"], f"mixed: {mode} / packed")
    assert np.isfinite(r["default"]["tau"]).all() and np.isfinite(r["default"]["cf"]).all()


def test_second_chunk(gpu, hmodels):
    """K = 300: launches of 256 and of 44 steps, the second planned from first step 256"""
    from hslabs_amd import synth

    p = synth.gen_params(2, "hexapod", id0=77)
    r = four_ways(gpu, hmodels["hexapod"], p, "hexapod B=2 K=300", default_planned=2, K=300)
    assert r["forced"]["tile_launches"] == 2


def test_forces_mode(gpu, hmodels):
    """solve_forces: contact forces and flags bitwise under every sequence"""
    import torch
    from hslabs_amd import synth

    m, B, K = hmodels["hexapod"], 9, 40
    p = synth.gen_params(B, "hexapod", id0=11)
    ctl = gpu.DeviceBatch(m, p, n_t=20, k0=0, horizon=K, outputs=("tau",))
    ctl.run_calls(K, call_horizon=1)
    i = torch.arange(K, device=ctl.tau.device)[None, :, None]
    j = torch.arange(m.nmj, device=ctl.tau.device)[None, None, :]
    tau = ctl.tau + 0.2 * torch.sin(0.7 * i + 1.3 * j)

    def go(mode):
        with counted(gpu, mode) as c:
            fb = gpu.DeviceBatch(m, p, n_t=20, k0=0, horizon=K, outputs=("cf", "flags"))
            fb.cf.fill_(float("nan"))
            fb.forces_launcher(tau, K, call_horizon=1)()
            torch.cuda.synchronize()
            out = dict(cf=fb.cf.cpu().numpy(), flags=fb.flags.cpu().numpy())
        out.update(c)
        return out

    r = {mode: go(mode) for mode in MODES}
    check_counters(r, "forces", default_planned=1)
    assert np.isfinite(r["packed"]["cf"]).all()
    for mode in ("default", "forced", "parity"):
        same(r[mode], r["packed"], f"forces: {mode} / packed", outs=("cf", "flags"))


def test_fp32(gpu, hmodels):
    """the single-precision build on the planner's sequence (forced, whatever it saves at this length),
    configs[2]'s call shape, against the packed run: test_gpu_limb_tile.py's test_fp32 bound (1e-3 relative)
    and the same flags"""
    import torch
    from hslabs_amd import synth

    p = synth.gen_params(16, "spider", id0=5)
    t = run(gpu, hmodels["spider"], p, "forced", K=2, Hc=32, dtype=torch.float32)
    pk = run(gpu, hmodels["spider"], p, "packed", K=2, Hc=32, dtype=torch.float32)
    assert t["tile_launches"] > 0 and t["plan_launches"] == t["tile_launches"]
    assert pk["tile_launches"] == 0 and pk["plan_launches"] == 0
    for k in ("tau", "cf", "work_cot"):
        assert np.isfinite(t[k])[np.isfinite(pk[k])].all(), k
    assert np.array_equal(t["flags"], pk["flags"])
    for k in ("tau", "cf"):
        ok = np.isfinite(t[k]) & np.isfinite(pk[k])
        err = np.abs(t[k].astype(np.float64) - pk[k]) / np.maximum(1.0, np.abs(pk[k].astype(np.float64)))
        print(f"fp32 planned tile against packed: max relative {k} difference {err[ok].max():.3e}")
        assert err[ok].max() < 1e-3
