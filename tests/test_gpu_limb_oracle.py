"""The step kernels the benchmark times, on the routes the product takes, against the CPU oracle.

1. The single-precision limb-lane kernel (hs_limb_kernel<float>, hslabs_amd/csrc/hs_limb.h): route() in
   hs_capi.cpp sends every eligible fp32 fused call of hs_run_calls / hs_run_mixed_calls to it (bench.py
   --fp32, configs[2]). tests/test_gpu_limb.py holds it to hs_rollout_kernel<float> only, and the two are
   not bitwise, so nothing follows from that kernel's oracle tests. Here every step of it is
   compared with the fp64 oracle's tree mode: finiteness, contact sets, flags, torques, contact forces,
   work, COT and the best key, with no routing switch in the environment.
2. The tile mapping (hs_limb_kernel<..., TILE>), which an fp64 fused launch of at least 40 steps takes by
   the committed rule (bench.py --steps 200): 40 steps on the default route against the oracle's fast and
   tree modes at the fp64 bounds of tests/test_gpu_parity.py. Steps 20 .. 39 are past one gait period: the
   oracle's own handling of H > n_t.

The fp32 reference is the fp64 oracle's tree mode on the steps the ABI gives the calls (include/hslabs.h,
hs_run_calls: call c solves steps k0_c .. k0_c + H - 1, k0_c = (k0 + c H) mod n_t): oracle.batch per call,
calls that follow each other without a wrap in one run (call_segments). Where no call wraps that is
oracle.batch(k0, K H). Where one does, it is not for a turning gait: the oracle's run of K H steps goes on
past the period, and a turning gait's samples past n_t are not the first period's (every spider gait of
synth.gen_params turns, curvature -0.15). Straight gaits repeat, and for them the test asserts that the two
references are one.

What may be left out of an fp32 comparison, and why (the bounds are the project's: FP32_TOL = 1e-3 relative
per step, tests/test_gpu.py; median 1e-5, tests/test_gpu_parity.py):
  * contact band: a step whose contact set (|cf| > 0 per foot) differs from the oracle's, but only where
    the oracle's own decision z < rcap + 1e-4 is marginal: some foot within BAND = 1e-5 m of the threshold
    (a tenth of the contact band, about 300 float ulps of the largest foot coordinate, 0.28 m). Any other
    mismatch fails. The oracle alone puts at most 1 % of a batch's steps in the band (asserted), so no more
    can be left out. Measured on the CPU: 0.49 % of the spider and hexapod batches (minimum margin
    1.55e-6 m), 0.10 % of myant's (7.6e-6 m), 0.59 % / 0.18 % of the mixed batch's hexapod / myant
    rollouts, none of cases d, f and the online case.
  * near rank: compare()'s rule. A step flagged HS_FLAG_NEAR_RANK on either side is compared wherever the
    oracle's tree and ortho answers agree within the fp64 parity bounds and excluded only where they
    disagree. Measured on the CPU: they disagree on 0 steps of every batch here except the tilted records'
    (case f: 41 of 4060 steps, 1.0 %; cap 2 %, tests/test_gpu_rec_transform.py's for tilted hexapods).
"""
import numpy as np
import pytest

from conftest import record_to_oracle_gait, transformed
from limb_gpu_kit import OUTS, counted, fused_calls, gpu, hmodels, product_route  # noqa: F401
from test_gpu_parity import (FP32_TOL, TAU_ABS, check_fast_every_step, check_flags, compare, near, npy,
                             reference_agreement, threads)

pytestmark = pytest.mark.gpu

N_T = 20
BAND = 1e-5     # m: the oracle's contact decision counts as marginal within this of rcap + 1e-4
MAX_BAND = 0.01  # the oracle's own in-band share of a batch's steps


def fused(gpu, make, K, Hc, nan_fill=False):
    """K fused calls of Hc steps (hs_run_calls / hs_run_mixed_calls) with the best key on the batch make()
    builds, on the product's route (no HS_LIMB* switch in the environment): the outputs on the host, the raw
    key, and how far the launch counters moved"""
    return fused_calls(gpu, make, product_route(), K, Hc, nan_fill)


def contact_sets(cf, nf):
    """tests/test_gpu.py's: the feet that carry a force"""
    return np.abs(cf.reshape(*cf.shape[:-1], nf, 3)).max(axis=-1) > 0


def call_segments(k0, K, Hc):
    """The steps K fused calls of Hc solve, by the ABI (include/hslabs.h, hs_run_calls): call c solves steps
    k0_c .. k0_c + Hc - 1 with k0_c = (k0 + c Hc) mod n_t. -> [(first step, steps)], calls that follow each
    other without a wrap joined: (0, 20) for 20 calls of 1 from 0; (0, 32), (12, 32) for configs[2]'s two
    calls of 32."""
    segs = []
    for c in range(K):
        kc = (k0 + c * Hc) % N_T
        if segs and segs[-1][0] + segs[-1][1] == kc:
            segs[-1] = (segs[-1][0], segs[-1][1] + Hc)
        else:
            segs.append((kc, Hc))
    return segs


def oracle_calls(oracle_mod, omodel, gaits, segs, basis):
    """the oracle on the calls' steps: oracle.batch per segment, rows in the calls' order, work and COT summed
    as accumulate sums them"""
    rs = [oracle_mod.batch(omodel, gaits, N_T, k, h, basis=basis, n_threads=threads()) for k, h in segs]
    out = {k: np.concatenate([r[k] for r in rs], axis=1) for k in ("tau", "cf", "flags")}
    out["work"], out["cot"] = sum(r["work"] for r in rs), sum(r["cot"] for r in rs)
    return out


def step_index(segs):
    """the gait step (k0_c + h) of every output row"""
    return np.concatenate([np.arange(k, k + h) for k, h in segs])


def band_share(oracle_mod, omodel, gaits, rcap, ksteps):
    """the share of the batch's [B][H] steps on which the oracle's own contact decision is marginal"""
    uniq, inv = np.unique(ksteps, return_inverse=True)
    m = np.array([[np.abs(oracle_mod.dynrec_dump(omodel, g, N_T, int(k))["fpos"][:, 2] - (rcap + 1e-4)).min()
                   for k in uniq] for g in gaits])
    return (m[:, inv] < BAND).mean()


def against_oracle(what, g, oracle_mod, omodel, gaits, rcap, segs, max_excluded=0.0, min_work=0.9, work=True):
    """The fp32 batch g (tau, cf, flags, work_cot, the counters) against the fp64 oracle's tree mode on the
    calls' steps (segs: call_segments): checks 1 to 6 of this module. Returns the oracle's result."""
    r = oracle_calls(oracle_mod, omodel, gaits, segs, oracle_mod.BASIS_TREE)
    ksteps = step_index(segs)
    tau, cf = g["tau"].astype(np.float64), g["cf"].astype(np.float64)
    flags = g["flags"].astype(np.uint32)
    B, H = flags.shape
    nf = r["cf"].shape[-1] // 3
    assert tau.shape == r["tau"].shape and cf.shape == r["cf"].shape
    if len(segs) > 1:
        # The calls wrapped. The oracle's one run of H steps from the first k0 goes on past the period instead
        # (t keeps growing): the same torques for a straight gait, which repeats with the period (held to the
        # fp64 bound here, so for those the two references are one), but not for a turning one, whose samples
        # past n_t are not those of the first period (measured on the CPU: up to 0.17 relative on case a's
        # steps 32 .. 63, where the fp64 kernel is within 4e-14 of the per-call oracle).
        u = oracle_mod.batch(omodel, gaits, N_T, segs[0][0], H, basis=oracle_mod.BASIS_TREE, n_threads=threads())
        du = np.abs(u["tau"] - r["tau"]).max(axis=(1, 2))
        straight = np.array([gt.curvature == 0 and gt.rec_transform is None for gt in gaits])
        print(f"{what}: the oracle's unwrapped run of {H} steps against its per-call runs {segs}: max |dtau| "
              f"{du[straight].max() if straight.any() else 0:.2e} over {int(straight.sum())} straight gaits, "
              f"{du[~straight].max() if (~straight).any() else 0:.2e} over {int((~straight).sum())} turning ones")
        assert (du[straight] < TAU_ABS).all()
    # 1. finite wherever the oracle is: no finiteness mask below
    assert np.isfinite(tau[np.isfinite(r["tau"])]).all(), f"{what}: non-finite torques"
    assert np.isfinite(cf[np.isfinite(r["cf"])]).all(), f"{what}: non-finite contact forces"
    wc = g["work_cot"].astype(np.float64)
    assert np.isfinite(wc[np.isfinite(r["cot"])]).all(), f"{what}: non-finite work / COT"
    # 2. contact sets: a mismatch is left out only where the oracle's own decision is marginal
    share = band_share(oracle_mod, omodel, gaits, rcap, ksteps)
    assert share <= MAX_BAND, f"{what}: the oracle alone has {100 * share:.2f} % of the steps in the contact band"
    differ = (contact_sets(cf, nf) != contact_sets(r["cf"], nf)).any(axis=-1)
    left = np.zeros((B, H), bool)
    for b, s in zip(*np.nonzero(differ)):
        fz = oracle_mod.dynrec_dump(omodel, gaits[b], N_T, int(ksteps[s]))["fpos"][:, 2]
        margin = np.abs(fz - (rcap + 1e-4)).min()
        assert margin < BAND, (f"{what}: contact set of rollout {b} step {s} differs from the oracle's with every foot "
                               f"at least {margin:.3e} m from the threshold")
        left[b, s] = True
    assert left.mean() <= MAX_BAND
    # 3. near rank: compare()'s rule
    flagged = near(flags, r["flags"]) & ~left
    agree, h0 = np.zeros((B, H), bool), 0
    for k, h in segs:
        rows = slice(h0, h0 + h)
        agree[:, rows], _ = reference_agreement(oracle_mod, omodel, gaits, {"tau": r["tau"][:, rows], "cf": r["cf"][:, rows]},
                                                flagged[:, rows], oracle_mod.BASIS_TREE, N_T, k)
        h0 += h
    excl = flagged & ~agree
    cmp = ~left & ~excl
    print(f"{what}: {int(cmp.sum())} of {cmp.size} steps compared, {int(left.sum())} left out (contact band; the "
          f"oracle alone has {100 * share:.3f} % in it), {int(flagged.sum())} flagged HS_FLAG_NEAR_RANK of which "
          f"{int(excl.sum())} excluded (tree and ortho disagree); limb_launches +{g['limb_launches']}, limb_tile_launches "
          f"+{g['tile_launches']}, limb_deferred +{g['deferred']}")
    assert excl.mean() <= max_excluded, f"{what}: {100 * excl.mean():.3f} % excluded (limit {100 * max_excluded} %)"
    # 4. flags
    check_flags(flags, r["flags"], what, ~cmp)
    # 5. torques and contact forces
    et = np.abs(tau - r["tau"]).max(axis=-1) / np.maximum(1, np.abs(r["tau"]).max(axis=-1))
    ec = np.abs(cf - r["cf"]).max(axis=-1) / np.maximum(1, np.abs(r["cf"]).max(axis=-1))
    print(f"{what}: tau error max {et[cmp].max():.3e} median {np.median(et[cmp]):.3e}, cf error max {ec[cmp].max():.3e} "
          f"(relative to max(1, the step's largest))")
    assert et[cmp].max() < FP32_TOL, f"{what}: {int((et[cmp] >= FP32_TOL).sum())} steps' torques over {FP32_TOL} (max {et[cmp].max():.3e})"
    assert ec[cmp].max() < FP32_TOL, f"{what}: {int((ec[cmp] >= FP32_TOL).sum())} steps' contact forces over {FP32_TOL} (max {ec[cmp].max():.3e})"
    assert np.median(et[cmp]) < 1e-5
    # 6. work and COT of every rollout compared whole
    if work:
        whole = cmp.all(axis=1) & np.isfinite(r["cot"])
        assert whole.sum() >= max(1, int(np.ceil(min_work * B))), f"{what}: work compared on only {int(whole.sum())} of {B} rollouts"
        ew = np.abs(wc[whole, 0] - r["work"][whole]) / np.maximum(np.abs(r["work"][whole]), 1e-30)
        print(f"{what}: work compared on {int(whole.sum())} of {B} rollouts, max relative error {ew.max():.3e}")
        np.testing.assert_allclose(wc[whole, 0], r["work"][whole], rtol=1e-3, atol=1e-6)
        np.testing.assert_allclose(wc[whole, 1], r["cot"][whole], rtol=1e-3, atol=1e-6)
    return r


def best_is_oracle_argmin(what, gpu, g, r, K, Hc):
    """7. the key names the oracle's argmin of |COT| over the rollouts with a finite COT (on these batches the
    oracle's best and second best differ by 10 % and 13 %, measured on the CPU, so the id is unambiguous); its
    float32 COT is the oracle's within 1e-3 relative. The key's COT is one cycle's, hs_best_key_cot: the
    accumulated COT times n_t / steps."""
    cot, rid = gpu.api.decode_best_key(g["best_key"])
    ac = np.where(np.isfinite(r["cot"]), np.abs(r["cot"]), np.inf)
    best = int(np.argmin(ac))
    second = np.partition(ac, 1)[1]
    print(f"{what}: key ({cot:.6f}, {rid}); oracle's best {best} with {ac[best] * N_T / (K * Hc):.6f}, second best "
          f"{100 * (second / ac[best] - 1):.1f} % above")
    assert second > 1.01 * ac[best]
    assert rid == best
    assert abs(cot - ac[best] * N_T / (K * Hc)) < 1e-3 * ac[best] * N_T / (K * Hc)


# id: (model, curved, id0, tilt of the record transforms or None, B, K, Hc, k0, excluded cap, min_work, best key)
CASES = {
    "a-spider-configs2-shape": ("spider", False, 5, None, 203, 2, 32, 0, 0.0, 0.9, True),
    "b-hexapod-curved": ("hexapod", True, 5, None, 203, 20, 1, 0, 0.0, 0.9, True),
    "c-myant": ("myant", False, 5, None, 203, 20, 1, 0, 0.0, 0.9, False),
    "d-spider-partial-wavefront": ("spider", True, 5, None, 5, 7, 3, 5, 0.0, 0.9, False),
    "e-hexapod-records-flat": ("hexapod", True, 900, 0.0, 203, 20, 1, 0, 0.0, 0.9, False),
    "f-hexapod-records-tilted": ("hexapod", True, 900, 0.05, 203, 20, 1, 0, 0.02, 0.8, False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_limb_kernel_matches_fp64_oracle(gpu, hmodels, oracle_mod, omodels, case):
    """a: configs[2]'s call shape (64 steps are 3.2 periods, the second call solves steps 12 .. 43; the last
    wavefront holds 3 rollouts). b: turning gaits, six limbs. c: 0 to 4 contacts, the oracle's full-rank,
    unreach, no-contact and near-rank flags, the one- and two-contact closed forms on limb lanes. d: fewer
    rollouts than a wavefront's eight, calls of H > 1, a k0 offset and the wrap. e: record transforms (yaw,
    translation, lift) mixed with plain gaits in one wavefront, no-contact steps. f: tilted records, the
    ill-posed steps the closed form declines: the fp32 fixup launch fed by the limb kernel must have run."""
    import torch
    from hslabs_amd import synth

    name, curved, id0, tilt, B, K, Hc, k0, max_excluded, min_work, best = CASES[case]
    p = synth.gen_params(B, name, id0=id0, curved=curved)
    if tilt is not None:
        p, _ = transformed(p, np.random.default_rng(17), tilt=tilt)
    g = fused(gpu, lambda: gpu.DeviceBatch(hmodels[name], p, n_t=N_T, k0=k0, horizon=K * Hc, outputs=OUTS,
                                           dtype=torch.float32), K, Hc)
    assert g["limb_launches"] > 0 and g["tile_launches"] == 0, "the fp32 route is the packed limb-lane kernel"
    if case.startswith("f"):
        assert g["deferred"] > 0, "the tilted records must defer steps to the fixup launch"
    gaits = [record_to_oracle_gait(oracle_mod, r) for r in p]
    r = against_oracle(case, g, oracle_mod, omodels[name], gaits, hmodels[name].rcap, call_segments(k0, K, Hc),
                       max_excluded, min_work)
    if best:
        best_is_oracle_argmin(case, gpu, g, r, K, Hc)


def test_fp32_limb_kernel_mixed_plan_matches_fp64_oracle(gpu, hmodels, oracle_mod, omodels):
    """g: the fp32 mixed plan (myant + hexapod interleaved, one launch), configs[2]'s call shape, each model's
    rollouts against the oracle separately; the rows past myant's joints and feet written 0 (the buffers
    start as NaN)"""
    import torch
    from hslabs_amd import synth

    B, K, Hc = 203, 2, 32
    params, idx = synth.gen_mixed(B)
    ms = [hmodels[n] for n in synth.MIXED_MODELS]
    g = fused(gpu, lambda: gpu.MixedBatch(ms, idx, params, n_t=N_T, k0=0, horizon=K * Hc, outputs=OUTS,
                                          dtype=torch.float32), K, Hc, nan_fill=True)
    assert g["limb_launches"] > 0 and g["tile_launches"] == 0
    for k, name in enumerate(synth.MIXED_MODELS):
        sel = np.nonzero(idx == k)[0]
        m = hmodels[name]
        assert (g["tau"][sel][:, :, m.nmj:] == 0).all() and (g["cf"][sel][:, :, 3 * m.nfeet:] == 0).all()
        gm = dict(g, tau=g["tau"][sel][:, :, :m.nmj], cf=g["cf"][sel][:, :, :3 * m.nfeet], flags=g["flags"][sel],
                  work_cot=g["work_cot"][sel])
        gaits = [record_to_oracle_gait(oracle_mod, params[i]) for i in sel]
        against_oracle(f"g-mixed {name}", gm, oracle_mod, omodels[name], gaits, m.rcap, call_segments(0, K, Hc))


def test_fp32_limb_kernel_online_matches_fp64_oracle(gpu, hmodels, oracle_mod, omodels):
    """the fp32 online shape (HS_LIMB_ONLINE=1: hs_run_steps, a limb-lane launch per call and its fixup): three
    calls of horizon 4 from k0 = 0; the batch holds the last call's rows, steps 8 .. 11 (checks 1 to 5; on the
    CPU the oracle's tree and ortho modes disagree on none of these 148 steps)"""
    import torch
    from hslabs_amd import synth

    name, B, Hc, K = "myant", 37, 4, 3
    p = synth.gen_params(B, name, id0=31, curved=True)
    with counted(gpu, product_route(HS_LIMB_ONLINE="1")) as c:
        b = gpu.DeviceBatch(hmodels[name], p, n_t=N_T, k0=0, horizon=Hc, outputs=OUTS, dtype=torch.float32)
        b.work_cot.zero_()
        b.run_steps(K, best=False, accumulate=False)
        torch.cuda.synchronize()
        g = {k: npy(getattr(b, k)) for k in OUTS}
    g.update(c)
    assert g["limb_launches"] == K and g["tile_launches"] == 0
    gaits = [record_to_oracle_gait(oracle_mod, r) for r in p]
    against_oracle("online myant", g, oracle_mod, omodels[name], gaits, hmodels[name].rcap, [((K - 1) * Hc, Hc)],
                   work=False)


@pytest.mark.parametrize("name", ["hexapod", "myant"])
def test_default_route_tile_launch_matches_oracle(gpu, hmodels, oracle_mod, omodels, name):
    """fp64, 40 fused steps from k0 = 0, no switch set: the routing rule takes the tile mapping (5 full
    tiles). Every step against the oracle's fast mode with no exclusion and against its tree mode at the fp64
    bounds with none excluded (on the CPU the tree and ortho modes disagree on 0 of these 440 steps), work and
    COT included. myant is the four-limb case, every request in the first pass. Steps 20 .. 39 repeat the
    gait's period against the oracle's own H > n_t."""
    from hslabs_amd import synth

    B, K = 11, 40
    p = synth.gen_params(B, name, id0=5)
    g = fused(gpu, lambda: gpu.DeviceBatch(hmodels[name], p, n_t=N_T, k0=0, horizon=K, outputs=OUTS), K, 1)
    print(f"{name}: limb_launches +{g['limb_launches']}, limb_tile_launches +{g['tile_launches']}, limb_deferred +{g['deferred']}")
    assert g["tile_launches"] > 0, "a 40-step fp64 launch takes the tile mapping by the committed rule"
    gaits = [record_to_oracle_gait(oracle_mod, r) for r in p]
    f = oracle_mod.batch(omodels[name], gaits, N_T, 0, K, basis=oracle_mod.BASIS_FAST, n_threads=threads())
    check_fast_every_step(f"tile {name}", g, f)
    r = oracle_mod.batch(omodels[name], gaits, N_T, 0, K, basis=oracle_mod.BASIS_TREE, n_threads=threads())
    compare(f"tile {name} vs tree", g, r, oracle_mod, omodels[name], gaits, oracle_mod.BASIS_TREE, max_excluded=0.0,
            min_work=1.0)
