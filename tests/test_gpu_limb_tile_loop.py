"""The tile loop of the limb-lane kernel's tile mapping (hslabs_amd/csrc/hs_limb.h: hs_limb_kernel's head runs
limb_step for each tile of the wavefront's chunk; launch_map::limb_tile_loop, hs_limb_tile.h's chunk
arithmetic) against a tile per wavefront and against the packed mapping.

How many tiles a wavefront runs decides which wavefront computes a step, never its value: tau, cf, flags,
work_cot and the best key are BITWISE those of HS_LIMB_TILE_LOOP=1 (a tile per wavefront, the launch before
the loop existed) and of the packed mapping (HS_LIMB_TILE=0), at TL = 2, 3 and 5 tiles per wavefront. The
shapes are the smallest that reach each way the loop can go wrong: uneven chunks, a chunk holding every tile,
TL above the tile count, idle slots in a tile that is looped into, a deferred step in a tile that is not the
chunk's last (it must end its group's tile, not the wavefront), turning gaits, calls of H > 1, a mixed plan,
two launches; forces mode, which does not loop, under the switch. All tile runs set HS_LIMB_TILE_MIN=1, so every launch length takes the tile
mapping. hs_limb_tile_loop_launches counts the launches whose wavefronts ran more than one tile."""
import functools

import numpy as np
import pytest

from conftest import transformed
import limb_gpu_kit as kit
from limb_gpu_kit import OUTS, PACKED, TILE, forces_tau, gpu, hmodels, same  # noqa: F401

pytestmark = pytest.mark.gpu

TLS = (2, 3, 5)
run = functools.partial(kit.run, K=40)  # K fused calls of Hc steps under `mode`: the outputs, the key and the counters


def loop(tl):
    return dict(TILE, HS_LIMB_TILE_LOOP=str(tl))


def check(runs, one, packed, what, outs=OUTS):
    """runs[tl] (tl > 1) against a tile per wavefront and against the packed mapping; the counter reports the
    looped launches and only them"""
    assert one["tile_launches"] > 0 and one["loop_launches"] == 0, what
    assert packed["tile_launches"] == 0 and packed["loop_launches"] == 0, what
    for tl, r in runs.items():
        assert r["tile_launches"] == one["tile_launches"] and r["loop_launches"] == r["tile_launches"], f"{what} TL={tl}"
        same(r, one, f"{what}: TL={tl} / TL=1", outs)
        same(r, packed, f"{what}: TL={tl} / packed", outs)


def all_ways(gpu, model, params, what, tls=TLS, **kw):
    one = run(gpu, model, params, loop(1), **kw)
    packed = run(gpu, model, params, PACKED, **kw)
    runs = {tl: run(gpu, model, params, loop(tl), **kw) for tl in tls}
    check(runs, one, packed, what)
    return runs, one, packed


def test_uneven_chunks_and_a_partial_batch(gpu, hmodels):
    """hexapod, B = 13 (the second batch wavefront has five rollouts), K = 40 from k0 = 13: five tiles in
    chunks of 2 + 2 + 1 and 3 + 2 and all five in one wavefront; the period wraps inside tiles"""
    from hslabs_amd import synth

    p = synth.gen_params(13, "hexapod", id0=4321)
    _, one, _ = all_ways(gpu, hmodels["hexapod"], p, "hexapod B=13 K=40 k0=13", k0=13)
    assert np.isfinite(one["tau"]).all()


def test_idle_slots_in_a_looped_tile(gpu, hmodels):
    """hexapod, B = 3, K = 44: six tiles, the last with four idle slots, run after other tiles by the same
    wavefront at every TL"""
    from hslabs_amd import synth

    p = synth.gen_params(3, "hexapod", id0=77)
    all_ways(gpu, hmodels["hexapod"], p, "hexapod B=3 K=44", K=44)


def test_more_tiles_per_wavefront_than_tiles(gpu, hmodels):
    """K = 9 at TL = 5: two tiles, the second with one live slot, in a chunk cut short by the tile count"""
    from hslabs_amd import synth

    p = synth.gen_params(3, "hexapod", id0=77)
    all_ways(gpu, hmodels["hexapod"], p, "hexapod B=3 K=9", tls=(5,), K=9, k0=13)


@pytest.mark.parametrize("barrier", ["1", "0"])
def test_a_deferred_step_ends_its_tile_only(gpu, hmodels, barrier):
    """test_gpu_limb_tile.py's transformed records (tilted: steps the closed form declines): the groups that
    defer leave their tile, the wavefront goes on to the next one. The same steps are deferred at every TL,
    with the fixup's grid barrier and without"""
    from hslabs_amd import synth

    rng = np.random.default_rng(17)
    p, _ = transformed(synth.gen_params(64, "hexapod", id0=900, curved=True), rng, tilt=0.05)
    m, what = hmodels["hexapod"], f"transformed hexapod, HS_FIX_BARRIER={barrier}"
    one = run(gpu, m, p, loop(1), HS_FIX_BARRIER=barrier)
    assert one["deferred"] > 0, what  # (first: the comparison below cannot pass with nothing deferred)
    packed = run(gpu, m, p, PACKED, HS_FIX_BARRIER=barrier)
    runs = {tl: run(gpu, m, p, loop(tl), HS_FIX_BARRIER=barrier) for tl in TLS}
    print(f"transformed: deferred steps TL=1 {one['deferred']}, packed {packed['deferred']}, "
          + ", ".join(f"TL={tl} {r['deferred']}" for tl, r in runs.items()))
    check(runs, one, packed, what)
    assert packed["deferred"] == one["deferred"]
    for tl, r in runs.items():
        assert r["deferred"] == one["deferred"], f"{what} TL={tl}"


def test_myant_deferred_steps(gpu, hmodels):
    """four limbs, ids 4717 .. 4727 (test_gpu_limb_tile.py's window with a deferring rollout, tier 2): the same
    number of deferred steps at every TL"""
    from hslabs_amd import synth

    p = synth.gen_params(11, "myant", id0=4717)
    m = hmodels["myant"]
    one = run(gpu, m, p, loop(1))
    assert one["deferred"] > 0
    packed = run(gpu, m, p, PACKED)
    runs = {tl: run(gpu, m, p, loop(tl)) for tl in TLS}
    check(runs, one, packed, "myant B=11 K=40")
    assert all(r["deferred"] == one["deferred"] for r in runs.values()) and packed["deferred"] == one["deferred"]


@pytest.mark.parametrize("name,B", [("hexapod", 9), ("spider", 17)])
def test_turning_gaits(gpu, hmodels, name, B):
    """the torso record's rows and the chain bodies through the exchange, tile after tile"""
    from hslabs_amd import synth

    p = synth.gen_params(B, name, id0=5, curved=True)
    all_ways(gpu, hmodels[name], p, f"{name} curved B={B} K=40")


def test_calls_of_more_than_one_step(gpu, hmodels):
    """Hc = 5, K = 8: the rows advance within a call and jump between calls"""
    from hslabs_amd import synth

    p = synth.gen_params(5, "hexapod", id0=31)
    all_ways(gpu, hmodels["hexapod"], p, "hexapod B=5 H=5 K=8", K=8, Hc=5)


def test_mixed_plan(gpu, hmodels):
    """myant + hexapod through MixedBatch: the wavefront's model and its rollout from the plan's tables, read
    once for the chunk"""
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(24)
    ms = [hmodels[n] for n in synth.MIXED_MODELS]

    def go(mode):
        return kit.run_mixed(gpu, ms, idx, params, mode, 40)

    one, packed = go(loop(1)), go(PACKED)
    check({tl: go(loop(tl)) for tl in TLS}, one, packed, "mixed")
    assert np.isfinite(one["tau"]).all() and np.isfinite(one["cf"]).all()


def test_forces_mode(gpu, hmodels):
    """solve_forces: contact forces and flags bitwise whatever HS_LIMB_TILE_LOOP says. Forces mode keeps a tile
    per wavefront (its kernel instantiations have no tile loop: with it they spill registers), so the switch
    must change neither its grid nor its outputs, and the counter reports no looped launch"""
    from hslabs_amd import synth

    m, B, K = hmodels["hexapod"], 9, 40
    p = synth.gen_params(B, "hexapod", id0=11)
    tau = forces_tau(gpu, m, p, K)

    def go(mode):
        return kit.run_forces(gpu, m, p, tau, mode, K)

    one, packed = go(loop(1)), go(PACKED)
    assert np.isfinite(packed["cf"]).all()
    assert one["tile_launches"] > 0 and packed["tile_launches"] == 0
    for tl in TLS:
        r = go(loop(tl))
        assert r["tile_launches"] == one["tile_launches"] and r["loop_launches"] == 0, tl
        same(r, one, f"forces: TL={tl} / TL=1", outs=("cf", "flags"))
        same(r, packed, f"forces: TL={tl} / packed", outs=("cf", "flags"))


def test_two_launches(gpu, hmodels):
    """K = 300: launches of 256 steps (32 tiles) and of 44 (six tiles, first step 256), both looped"""
    from hslabs_amd import synth

    p = synth.gen_params(2, "hexapod", id0=77)
    runs, one, _ = all_ways(gpu, hmodels["hexapod"], p, "hexapod B=2 K=300", K=300)
    assert one["tile_launches"] == 2 and all(r["loop_launches"] == 2 for r in runs.values())


def test_switch_values(gpu, hmodels):
    """HS_LIMB_TILE_LOOP=1 and values that are no positive number run a tile per wavefront (no looped launch:
    the rule's answer at this batch, far below the resident wavefronts); a packed launch counts as none"""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(3, "hexapod", id0=77)
    for v in ("1", "", "abc", "0", "-3", "2x"):
        r = run(gpu, m, p, loop(v))
        assert r["tile_launches"] == 1 and r["loop_launches"] == 0, v
    assert run(gpu, m, p, dict(PACKED, HS_LIMB_TILE_LOOP="5"))["loop_launches"] == 0
    assert run(gpu, m, p, loop(4))["loop_launches"] == 1
    one_tile = run(gpu, m, p, loop(4), K=8)  # a launch of one tile: no wavefront runs more than one
    assert one_tile["tile_launches"] == 1 and one_tile["loop_launches"] == 0


def test_fp32_keeps_a_tile_per_wavefront(gpu, hmodels):
    """the single-precision TILE instantiations have no tile loop: under the switch the launch, its outputs
    (bitwise: the same kernel on the same grid) and the counter are those of a tile per wavefront"""
    import torch
    from hslabs_amd import synth

    p = synth.gen_params(16, "spider", id0=5)
    one = run(gpu, hmodels["spider"], p, loop(1), K=2, Hc=32, dtype=torch.float32)
    r = run(gpu, hmodels["spider"], p, loop(5), K=2, Hc=32, dtype=torch.float32)
    assert one["tile_launches"] > 0 and r["tile_launches"] == one["tile_launches"]
    assert one["loop_launches"] == 0 and r["loop_launches"] == 0
    same(r, one, "fp32 spider: TL=5 / TL=1")
