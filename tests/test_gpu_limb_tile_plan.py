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
import numpy as np
import pytest

import limb_gpu_kit as kit
from limb_gpu_kit import TILE, forces_tau, gpu, hmodels, same  # noqa: F401

pytestmark = pytest.mark.gpu

# the four runs: the library's switches (None: not in the environment)
MODES = {
    "default": dict(TILE, HS_LIMB_TILE_PLAN=None),
    "forced": dict(TILE, HS_LIMB_TILE_PLAN="2"),
    "parity": dict(TILE, HS_LIMB_TILE_PLAN="0"),
    "packed": dict(HS_LIMB="1", HS_LIMB_TILE="0", HS_LIMB_TILE_PLAN=None),
}


def run(gpu, model, params, mode, K=40, **kw):
    """K fused calls of Hc steps under MODES[mode]: the outputs, the key and the counters"""
    return kit.run(gpu, model, params, MODES[mode], K, **kw)


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
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(24)
    ms = [hmodels[n] for n in synth.MIXED_MODELS]

    def go(mode):
        return kit.run_mixed(gpu, ms, idx, params, MODES[mode], 40)

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
    from hslabs_amd import synth

    m, B, K = hmodels["hexapod"], 9, 40
    p = synth.gen_params(B, "hexapod", id0=11)
    tau = forces_tau(gpu, m, p, K)

    def go(mode):
        return kit.run_forces(gpu, m, p, tau, MODES[mode], K)

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
