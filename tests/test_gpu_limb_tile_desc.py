"""The tile descriptor on the GPU (hslabs_amd/csrc/hs_limb_tile.h: limb_tile_desc, built by launch_limb; read by
limb_step and limb_tile_kd in hs_limb.h in place of their per-lane row arithmetic, neighbour tests, ballots and bit
scans).

The descriptor says where a value is computed, never the value: tau, cf, flags, work_cot and the best key of the
tile route are BITWISE those of the packed mapping (HS_LIMB_TILE=0), and the same number of steps is deferred
(limb_deferred). The shapes are the smallest that reach each branch: full tiles plus a remainder tile with a further
FK pass, a start inside the gait period, idle slots, calls of H > 1, a turning gait (the chain body through
ds_permute, in the pass the descriptor's requests say), four limbs with tier-2 deferrals (E0 = 8), a mixed
plan (4- and 6-limb wavefronts under one descriptor), two launches, the parity order and the forced chain order through the same descriptor, 1, 3
and 5 tiles per wavefront, forces mode, and the fp32 build (not bitwise: test_gpu_limb_tile.py's bound)."""
import functools

import numpy as np
import pytest

import limb_gpu_kit as kit
from limb_gpu_kit import PACKED, TILE, forces_tau, gpu, hmodels  # noqa: F401

pytestmark = pytest.mark.gpu

run = functools.partial(kit.run, K=40)  # K fused calls of Hc steps under `mode`: the outputs, the key and the counters
same = functools.partial(kit.same, deferred=True)  # and the same number of deferred steps


def tile_vs_packed(gpu, model, params, what, modes=(TILE,), **kw):
    """every tile mode against one packed run"""
    packed = run(gpu, model, params, PACKED, **kw)
    assert packed["tile_launches"] == 0, what
    runs = []
    for mode in modes:
        t = run(gpu, model, params, mode, **kw)
        assert t["tile_launches"] > 0, what
        same(t, packed, f"{what} {sorted(set(mode.items()) - set(TILE.items()))}: tile / packed")
        runs.append(t)
    return runs, packed


def test_full_tiles_and_a_remainder_tile(gpu, hmodels):
    """hexapod, B = 11 (the second batch wavefront has three rollouts), 40 steps from k0 = 0: the planner's four
    full tiles (2 requests each) and one remainder tile with 8 requests, one further pass"""
    from hslabs_amd import synth

    p = synth.gen_params(11, "hexapod", id0=4321)
    (t,), _ = tile_vs_packed(gpu, hmodels["hexapod"], p, "hexapod B=11 K=40")
    assert t["plan_launches"] == t["tile_launches"] == 1
    assert np.isfinite(t["tau"]).all()


def test_a_start_inside_the_period(gpu, hmodels):
    """hexapod, B = 11, 64 steps from k0 = 13: the rows wrap at other places than the tiles end"""
    from hslabs_amd import synth

    p = synth.gen_params(11, "hexapod", id0=4321)
    tile_vs_packed(gpu, hmodels["hexapod"], p, "hexapod B=11 K=64 k0=13", K=64, k0=13)


@pytest.mark.parametrize("K", [13, 21])
def test_idle_slots(gpu, hmodels, K):
    """a last tile with 3 idle slots: they carry the tile's first row, are no share target and no request"""
    from hslabs_amd import synth

    p = synth.gen_params(3, "hexapod", id0=77)
    tile_vs_packed(gpu, hmodels["hexapod"], p, f"hexapod B=3 K={K}", K=K, k0=13)


def test_calls_of_four_steps(gpu, hmodels):
    """H = 4: the rows advance within a call and jump between calls (limb_tile_row's two terms)"""
    from hslabs_amd import synth

    p = synth.gen_params(5, "hexapod", id0=31)
    tile_vs_packed(gpu, hmodels["hexapod"], p, "hexapod B=5 H=4 K=10", K=10, Hc=4)


def test_a_turning_hexapod(gpu, hmodels):
    """the chain bodies through ds_permute in the pass their request is served, the torso record's rows"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=5, curved=True)
    tile_vs_packed(gpu, hmodels["hexapod"], p, "hexapod curved B=9 K=40")


def test_myant_defers_the_same_steps(gpu, hmodels):
    """four limbs (E0 = 8: every request on the idle lanes of pass 0), B = 9 of test_gpu_limb_tile.py's window
    with a deferring rollout (ids 4717 .. 4727, tier 2): same() compares the deferred counts"""
    from hslabs_amd import synth

    p9 = synth.gen_params(9, "myant", id0=4717)
    tile_vs_packed(gpu, hmodels["myant"], p9, "myant B=9")
    p = synth.gen_params(11, "myant", id0=4717)
    (t,), pk = tile_vs_packed(gpu, hmodels["myant"], p, "myant B=11 (the deferring window)")
    print(f"myant: {t['deferred']} steps deferred (tile), {pk['deferred']} (packed)")
    assert t["deferred"] > 0


def test_mixed_plan(gpu, hmodels):
    """myant + hexapod through MixedBatch: 4- and 6-limb wavefronts read one descriptor, E0 and the pass of a
    request from the wavefront's own model"""
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(24)
    ms = [hmodels[n] for n in synth.MIXED_MODELS]

    def go(mode):
        return kit.run_mixed(gpu, ms, idx, params, mode, 40)

    t, pk = go(TILE), go(PACKED)
    assert t["tile_launches"] > 0 and pk["tile_launches"] == 0
    same(t, pk, "mixed: tile / packed")
    assert np.isfinite(t["tau"]).all() and np.isfinite(t["cf"]).all()


def test_two_launches(gpu, hmodels):
    """300 steps: launches of 256 steps (all 32 tiles of a descriptor) and of 44 from step 256"""
    from hslabs_amd import synth

    p = synth.gen_params(2, "hexapod", id0=77)
    (t,), _ = tile_vs_packed(gpu, hmodels["hexapod"], p, "hexapod B=2 K=300", K=300)
    assert t["tile_launches"] == 2


def test_every_sequence_and_every_loop_length(gpu, hmodels):
    """the parity order (HS_LIMB_TILE_PLAN=0) and the forced chain order (=2) through the same descriptor, and
    1, 3 and 5 tiles per wavefront: hexapod, B = 11, 64 steps from k0 = 13, one packed run for all"""
    from hslabs_amd import synth

    p = synth.gen_params(11, "hexapod", id0=4321)
    modes = [dict(TILE, HS_LIMB_TILE_PLAN="0"), dict(TILE, HS_LIMB_TILE_PLAN="2")]
    modes += [dict(TILE, HS_LIMB_TILE_LOOP=str(tl)) for tl in (1, 3, 5)]
    runs, _ = tile_vs_packed(gpu, hmodels["hexapod"], p, "hexapod B=11 K=64 k0=13", modes=modes, K=64, k0=13)
    assert runs[0]["plan_launches"] == 0  # the counter counts the planner's sequence only
    assert runs[1]["plan_launches"] == 1
    # the forced chain order on four limbs, where the planner itself keeps the parity order
    p4 = synth.gen_params(9, "myant", id0=4717)
    tile_vs_packed(gpu, hmodels["myant"], p4, "myant B=9 chain order", modes=[dict(TILE, HS_LIMB_TILE_PLAN="2")])


def test_forces_mode(gpu, hmodels):
    """solve_forces through the descriptor against the packed mapping: contact forces and flags bitwise"""
    from hslabs_amd import synth

    m, B, K = hmodels["hexapod"], 9, 40
    p = synth.gen_params(B, "hexapod", id0=11)
    tau = forces_tau(gpu, m, p, K)

    def go(mode):
        return kit.run_forces(gpu, m, p, tau, mode, K)

    t, pk = go(TILE), go(PACKED)
    assert t["tile_launches"] > 0 and pk["tile_launches"] == 0
    assert np.isfinite(pk["cf"]).all()
    same(t, pk, "forces: tile / packed", outs=("cf", "flags"))


def test_fp32(gpu, hmodels):
    """the single-precision TILE instantiations take the descriptor too (reached through HS_LIMB_TILE_MIN): the
    same flags, torques within test_gpu_limb_tile.py's fp32 bound of the packed run (1e-3 relative; not bitwise)"""
    import torch
    from hslabs_amd import synth

    p = synth.gen_params(16, "spider", id0=5)
    t = run(gpu, hmodels["spider"], p, TILE, K=2, Hc=32, dtype=torch.float32)
    pk = run(gpu, hmodels["spider"], p, PACKED, K=2, Hc=32, dtype=torch.float32)
    assert t["tile_launches"] > 0 and pk["tile_launches"] == 0
    assert np.array_equal(t["flags"], pk["flags"])
    ok = np.isfinite(pk["tau"])
    assert np.isfinite(t["tau"])[ok].all()
    err = np.abs(t["tau"].astype(np.float64) - pk["tau"]) / np.maximum(1.0, np.abs(pk["tau"].astype(np.float64)))
    print(f"fp32 tile against packed: max relative torque difference {err[ok].max():.3e}")
    assert err[ok].max() < 1e-3
