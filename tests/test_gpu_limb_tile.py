"""The limb-lane kernel's tile mapping (hslabs_amd/csrc/hs_limb.h TILE, hs_limb_tile.h) against its packed
mapping and against hs_rollout_kernel.

A tile-mapped wavefront runs eight steps of one rollout, two steps apart, and every group takes its
stencil's outer rows from its neighbours' centre FK (or from a request when no neighbour holds the row).
Sharing decides where a value is computed, never the value: tau, cf, flags, work_cot and the best key are
BITWISE those of the packed mapping (HS_LIMB_TILE=0) and, in fp64, of hs_rollout_kernel (HS_LIMB=0). The
shapes are the smallest that reach each way the mapping can go wrong: a partial batch, breaks of the slot
sequence (period wrap, parity switch), half-empty tiles, calls of H > 1, turning gaits (the chain bodies
through the exchange), four-limb models (every request in the first pass), deferred steps, a mixed plan,
two launch chunks, forces mode, fp32. The tile runs set HS_LIMB_TILE_MIN=1 so that every launch length
takes the tile mapping whatever the routing rule is; test_routing_rule checks the rule itself with the
switch unset.
"""
import functools
import os

import numpy as np
import pytest

from conftest import transformed
import limb_gpu_kit as kit
from limb_gpu_kit import PACKED, ROLLOUT, TILE, forces_tau, gpu, hmodels, run_forces, run_mixed, same  # noqa: F401

pytestmark = pytest.mark.gpu

run = functools.partial(kit.run, K=20)  # K fused calls of Hc steps on the mapping `mode`: the outputs, the key, the counters


def three_ways(gpu, model, params, what, **kw):
    """tile against packed and against hs_rollout_kernel, bitwise; the tile mapping ran in the tile run only"""
    t = run(gpu, model, params, TILE, **kw)
    p = run(gpu, model, params, PACKED, **kw)
    r = run(gpu, model, params, ROLLOUT, **kw)
    assert t["tile_launches"] > 0 and p["tile_launches"] == 0 and r["tile_launches"] == 0, what
    same(t, p, f"{what}: tile / packed")
    same(t, r, f"{what}: tile / hs_rollout_kernel")
    return t, p


def test_partial_batch_and_breaks(gpu, hmodels):
    """B = 9: the second batch wavefront has one rollout; K = 20 from k0 = 0: the period wrap, the parity
    switch and a half-empty last tile"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=4321)
    t, _ = three_ways(gpu, hmodels["hexapod"], p, "hexapod B=9 K=20")
    assert np.isfinite(t["tau"]).all()


@pytest.mark.parametrize("K", [1, 2, 7, 8, 9, 16, 17, 23])
def test_tile_and_wrap_edges(gpu, hmodels, K):
    """one step, one tile exactly, one over, two tiles, and wraps of k0 = 13 inside a tile"""
    from hslabs_amd import synth

    p = synth.gen_params(3, "hexapod", id0=77)
    three_ways(gpu, hmodels["hexapod"], p, f"hexapod B=3 k0=13 K={K}", K=K, k0=13)


@pytest.mark.parametrize("name,B,Hc,K", [("hexapod", 5, 5, 4), ("spider", 4, 32, 2)])
def test_calls_of_more_than_one_step(gpu, hmodels, name, B, Hc, K):
    """an odd horizon flips the step parity between calls; configs[2]'s call shape"""
    from hslabs_amd import synth

    p = synth.gen_params(B, name, id0=31)
    three_ways(gpu, hmodels[name], p, f"{name} B={B} H={Hc} K={K}", K=K, Hc=Hc)


def test_turning_gaits(gpu, hmodels):
    """the torso record's rows and the chain bodies through the exchange"""
    from hslabs_amd import synth

    p = synth.gen_params(17, "spider", id0=5, curved=True)
    three_ways(gpu, hmodels["spider"], p, "spider curved B=17")


def test_myant(gpu, hmodels):
    """four limbs: every request fits the first pass; one- and two-contact steps (fast_solve_lanes' closed
    forms) and steps the kernel defers (tier 2: a rollout whose legs stay straight), the same number on
    both mappings. The 11 rollouts are ids 4717 .. 4727 of the synthetic myant gaits: the window of
    tests/test_gpu_limb.py's B = 1024, id0 = 4321 batch (8 of 20,480 steps deferred) that holds a deferring
    rollout (4 of its 220 steps); most windows of that batch, its first 11 rollouts among them, defer none."""
    from hslabs_amd import synth

    p = synth.gen_params(11, "myant", id0=4717)
    t, pk = three_ways(gpu, hmodels["myant"], p, "myant B=11")
    print(f"myant: {t['deferred']} steps deferred (tile), {pk['deferred']} (packed)")
    assert t["deferred"] > 0 and t["deferred"] == pk["deferred"]


@pytest.mark.parametrize("barrier", ["1", "0"])
def test_transformed_records(gpu, hmodels, barrier):
    """tilted records: steps the closed form declines, their fix items' (step, slot) from per-group steps,
    with the fixup's grid barrier and without"""
    from hslabs_amd import synth

    rng = np.random.default_rng(17)
    p, _ = transformed(synth.gen_params(64, "hexapod", id0=900, curved=True), rng, tilt=0.05)
    t, pk = three_ways(gpu, hmodels["hexapod"], p, f"transformed hexapod, HS_FIX_BARRIER={barrier}",
                       HS_FIX_BARRIER=barrier)
    print(f"transformed: {t['deferred']} steps deferred (tile), {pk['deferred']} (packed)")
    assert t["deferred"] > 0 and t["deferred"] == pk["deferred"]


def test_mixed_plan(gpu, hmodels):
    """myant + hexapod through MixedBatch: the wavefront's model and its rollout from the plan's tables"""
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(24)
    ms = [hmodels[n] for n in synth.MIXED_MODELS]

    def go(mode):
        return run_mixed(gpu, ms, idx, params, mode, 20)

    t, p, r = go(TILE), go(PACKED), go(ROLLOUT)
    assert t["tile_launches"] > 0 and p["tile_launches"] == 0 and r["tile_launches"] == 0
    same(t, p, "mixed: tile / packed")
    same(t, r, "mixed: tile / hs_rollout_kernel")
    assert np.isfinite(t["tau"]).all() and np.isfinite(t["cf"]).all()


def test_two_launch_chunks(gpu, hmodels):
    """K = 300: launches of 256 + 44 steps, the second with a first step other than 0"""
    from hslabs_amd import synth

    p = synth.gen_params(2, "hexapod", id0=77)
    t, _ = three_ways(gpu, hmodels["hexapod"], p, "hexapod B=2 K=300", K=300)
    assert t["tile_launches"] == 2


def test_forces_mode(gpu, hmodels):
    """solve_forces through the tile mapping against the packed one: contact forces and flags bitwise"""
    from hslabs_amd import synth

    m, B, K = hmodels["hexapod"], 9, 20
    p = synth.gen_params(B, "hexapod", id0=11)
    tau = forces_tau(gpu, m, p, K)

    def go(mode):
        r = run_forces(gpu, m, p, tau, mode, K)
        return r["cf"], r["flags"], r["tile_launches"]

    ct, ft, nt = go(TILE)
    cp, fp_, np_ = go(PACKED)
    assert nt > 0 and np_ == 0
    assert np.array_equal(ft, fp_), f"flags differ on {int((ft != fp_).sum())} steps"
    assert np.isfinite(ct).all()
    assert np.array_equal(ct, cp), f"forces differ on {int((ct != cp).sum())} entries"


def test_fp32(gpu, hmodels):
    """the single-precision build, configs[2]'s call shape: finite wherever the packed run is, the same
    flags, torques and contact forces within the fp32 build's bound of the packed run
    (tests/test_gpu_limb.py's: 1e-3 relative)"""
    import torch
    from hslabs_amd import synth

    p = synth.gen_params(16, "spider", id0=5)
    t = run(gpu, hmodels["spider"], p, TILE, K=2, Hc=32, dtype=torch.float32)
    pk = run(gpu, hmodels["spider"], p, PACKED, K=2, Hc=32, dtype=torch.float32)
    assert t["tile_launches"] > 0 and pk["tile_launches"] == 0
    for k in ("tau", "cf", "work_cot"):
        assert np.isfinite(t[k])[np.isfinite(pk[k])].all(), k
    ok = np.isfinite(t["tau"]) & np.isfinite(pk["tau"])
    err = np.abs(t["tau"].astype(np.float64) - pk["tau"]) / np.maximum(1.0, np.abs(pk["tau"].astype(np.float64)))
    print(f"fp32 tile against packed: max relative torque difference {err[ok].max():.3e}, "
          f"flags differ on {int((t['flags'] != pk['flags']).sum())} steps")
    assert np.array_equal(t["flags"], pk["flags"])
    assert err[ok].max() < 1e-3
    okc = np.isfinite(t["cf"]) & np.isfinite(pk["cf"])
    errc = np.abs(t["cf"].astype(np.float64) - pk["cf"]) / np.maximum(1.0, np.abs(pk["cf"].astype(np.float64)))
    print(f"fp32 tile against packed: max relative contact force difference {errc[okc].max():.3e}")
    assert errc[okc].max() < 1e-3


def test_routing_rule(gpu, hmodels):
    """the committed rule, with no HS_LIMB_TILE_MIN in the environment: fp64 launches of at least 40 steps
    whose tiles idle at most 1 slot in 32 take the tile mapping, every other launch the packed one
    (hs_limb_tile_launches counts which ran); a value of HS_LIMB_TILE_MIN that is no positive number is
    ignored"""
    import torch
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(3, "hexapod", id0=77)
    old = os.environ.pop("HS_LIMB_TILE_MIN", None)
    try:
        def tiles(K, dtype=None, **sw):
            return run(gpu, m, p, dict(HS_LIMB="1", **sw), K=K, dtype=dtype)["tile_launches"]

        assert tiles(20) == 0       # the driver shape: three tiles, the last half empty
        assert tiles(16) == 0 and tiles(39) == 0  # below the threshold
        assert tiles(40) == 1
        assert tiles(200) == 1
        assert tiles(44) == 0       # 4 idle slots of 48
        assert tiles(250) == 1      # 6 idle slots of 256: within 1 in 32
        assert tiles(300) == 1      # chunks of 256 (tile) + 44 (packed)
        assert tiles(200, dtype=torch.float32) == 0
        assert tiles(200, HS_LIMB_TILE="0") == 0
        assert tiles(20, HS_LIMB_TILE_MIN="1") == 1
        for junk in ("", "abc", "0", "-3", "8x"):
            assert tiles(20, HS_LIMB_TILE_MIN=junk) == 0 and tiles(200, HS_LIMB_TILE_MIN=junk) == 1, junk
    finally:
        if old is not None:
            os.environ["HS_LIMB_TILE_MIN"] = old
