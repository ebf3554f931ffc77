"""The tile loop's wavefront constants in LDS (hslabs_amd/csrc/hs_limb.h: LimbLaneK, the model's per-lane
constants formed by the head's lanes; LimbRolloutK, the rollout's sample times and straight-gait frames copied
by the head; the tile's slots by one scalar load; the joint rates' loads in one batch with the wrap as selects).

Staging says where a value is read from, never the value: tau, cf, flags, work_cot and the best key of the looped
tile route are BITWISE those of the packed mapping (HS_LIMB_TILE=0) and of hs_rollout_kernel's fused step
(HS_LIMB=0), the same number of steps is deferred as by the packed mapping (limb_deferred), and the looped
launches are counted. Every case runs HS_LIMB_TILE_LOOP = 1, 2 and 5: the same kernel with one, two and all
five tiles behind one head (hs_limb_tile_loop_launches counts a launch whose wavefronts run more than one tile,
so it rises with the runs at 2 and 5; the run at 1 is pinned by its tile launches)."""
import functools

import numpy as np
import pytest

from conftest import transformed
import limb_gpu_kit as kit
from limb_gpu_kit import PACKED, ROLLOUT, TILE, gpu, hmodels  # noqa: F401

pytestmark = pytest.mark.gpu

TLS = (1, 2, 5)
run = functools.partial(kit.run, K=40)  # K fused calls of Hc steps under `mode`: the outputs, the key and the counters
same = functools.partial(kit.same, deferred=True)  # and, unless deferred=False, the same number of deferred steps


def loop(tl, **more):
    return dict(TILE, HS_LIMB_TILE_LOOP=str(tl), **more)


def check(go, what, more=None):
    """go(mode) under the looped tile route at every TL against the packed mapping and hs_rollout_kernel"""
    more = more or {}
    packed, rollout = go(dict(PACKED, **more)), go(dict(ROLLOUT, **more))
    assert packed["tile_launches"] == 0 and rollout["tile_launches"] == 0, what
    same(packed, rollout, f"{what}: packed / HS_LIMB=0", deferred=False)
    runs = {}
    for tl in TLS:
        r = runs[tl] = go(loop(tl, **more))
        assert r["tile_launches"] > 0, f"{what} TL={tl}"
        if tl > 1:
            assert r["loop_launches"] == r["tile_launches"], f"{what} TL={tl}: the looped launches were not counted"
        same(r, packed, f"{what}: TL={tl} / packed")
        same(r, rollout, f"{what}: TL={tl} / HS_LIMB=0", deferred=False)
    assert sum(r["loop_launches"] for r in runs.values()) > 0, what
    return runs, packed


def check_batch(gpu, model, params, what, more=None, **kw):
    return check(lambda mode: run(gpu, model, params, mode, **kw), what, more)


def test_straight(gpu, hmodels):
    """hexapod, B = 9 (the second batch wavefront holds one live rollout), K = 40: the frames and the chain
    bodies from the staged KinFrames, five tiles behind one head at TL = 5"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=4321)
    runs, _ = check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 K=40")
    assert np.isfinite(runs[5]["tau"]).all()


def test_curved(gpu, hmodels):
    """turning gaits: the torso record's rows stay in global memory, the lane constants and the sample times
    come from LDS"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=5, curved=True)
    check_batch(gpu, hmodels["hexapod"], p, "hexapod curved B=9 K=40")


def test_transformed_record(gpu, hmodels):
    """transformed records beside plain ones: straight and record-driven wavefronts in one launch"""
    from hslabs_amd import synth

    p, on = transformed(synth.gen_params(9, "hexapod", id0=900), np.random.default_rng(17), tilt=0.05)
    assert on.any() and not on.all()
    check_batch(gpu, hmodels["hexapod"], p, "hexapod transformed B=9 K=40")


def test_idle_slots_in_a_looped_tile(gpu, hmodels):
    """K = 44 with HS_LIMB_TILE_MIN=40: six tiles, the last with four idle slots, whose groups select the
    tile's first step from the scalar slots"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=77)
    check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 K=44", more=dict(HS_LIMB_TILE_MIN="40"), K=44)


def test_rows_wrap(gpu, hmodels):
    """calls of H = 4 steps from k0 = 13: the rows advance within a call, jump between calls and wrap with the
    period inside tiles"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=31)
    check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 H=4 K=10 k0=13", K=10, Hc=4, k0=13)


def test_last_rows_of_the_staged_times(gpu, hmodels):
    """n_t = 56, a whole period of K = 56 steps from k0 = 13: the call's table is the period's 56 samples and
    the stencil's four more, so the steps read the staged t_tab up to row 59 of HS_KTAB = 64"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=4321)
    check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 K=56 n_t=56", K=56, k0=13, n_t=56)


def test_myant_defers_inside_a_chunk(gpu, hmodels):
    """four limbs, ids 4719 .. 4727 (the end of test_gpu_limb_tile.py's window, which holds its deferring
    rollout: tier-2 deferrals in tiles that are not the chunk's last): the lane block of a four-limb model, and
    the same steps deferred"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "myant", id0=4719)
    runs, packed = check_batch(gpu, hmodels["myant"], p, "myant B=9 K=40")
    print(f"myant: {packed['deferred']} steps deferred (packed), {runs[5]['deferred']} (TL=5)")
    assert packed["deferred"] > 0


def test_mixed_plan(gpu, hmodels):
    """myant + hexapod, B = 16: wavefronts of one launch carry different lane blocks"""
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(16)
    assert set(idx.tolist()) == {0, 1}
    ms = [hmodels[n] for n in synth.MIXED_MODELS]

    def go(mode):
        return kit.run_mixed(gpu, ms, idx, params, mode, 40)

    runs, _ = check(go, "mixed B=16 K=40")
    assert np.isfinite(runs[5]["tau"]).all() and np.isfinite(runs[5]["cf"]).all()


def test_two_launches_restage(gpu, hmodels):
    """K = 300 on one batch: a launch of 256 steps and one of 44 from step 256, the second launch's heads stage
    again after the first's"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=77)
    runs, _ = check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 K=300", K=300)
    assert all(r["tile_launches"] == 2 for r in runs.values())
