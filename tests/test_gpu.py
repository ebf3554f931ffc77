"""GPU parity (MI355X): the HIP path through the C ABI against the oracle, the
committed golden vectors, and size-independent properties at BASELINE sizes.

Tolerances (fp64): per-joint motor torque |GPU - oracle| < 1e-9 N*m on the
reference setups (north_star asks < 1e-6; observed ~1e-12, the residue of
device vs glibc transcendental ULPs amplified by the 1/(4 dt^2) stencil),
contact forces < 1e-8, COT relative < 1e-9. Steps flagged HS_FLAG_NEAR_RANK
on either side (a rank or routing decision within rounding of its threshold) are
compared wherever the oracle's two reference-faithful bases agree, and excluded (counted) only where
they do not (test_gpu_parity.compare).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, MODELS, PGS_CONFIG, PGS_IDS, golden_params, record_to_oracle_gait, to_oracle_gait
from test_gpu_parity import as_batch, check_fast_every_step, check_flags, compare, near

pytestmark = pytest.mark.gpu

TAU_TOL = 1e-9
CF_TOL = 1e-8
FP32_TOL = 1e-3  # stated single-precision bound: |tau_f32 - tau_f64| <= 1e-3 max(1, |tau|) per step


@pytest.fixture(scope="module")
def gpu(product):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return product


@pytest.fixture(scope="module")
def hmodels(gpu):
    return {n: gpu.KinematicModel(os.path.join(MODELS, f"{n}.xml")) for n in ("hexapod", "spider", "myant")}


def wrapdiff(a, b):
    d = a - b
    return np.abs((d + np.pi) % (2 * np.pi) - np.pi)


@pytest.mark.parametrize("sid", PGS_IDS)
def test_pgs_setups_match_oracle(gpu, hmodels, oracle_mod, omodels, sid):
    p = gpu.read_pgs_config(PGS_CONFIG, sid)
    name = p.fname.replace(".xml", "")
    g = gpu.run_host(hmodels[name], [p], n_t=20, k0=0, horizon=20)
    og = to_oracle_gait(oracle_mod, p)
    for basis in (oracle_mod.BASIS_FAST, oracle_mod.BASIS_TREE, oracle_mod.BASIS_ORTHO):
        r = oracle_mod.rollout(omodels[name], og, 20, basis=basis)
        excl = compare(f"pgs {sid} vs basis {basis}", g, as_batch(r), oracle_mod, omodels[name], [og], basis,
                       min_work=1.0)
        k = ~excl[0]
        assert np.abs(g["tau"][0][k] - r["tau"][k]).max() < TAU_TOL * max(1, np.abs(r["tau"]).max())
        assert np.abs(g["x"][0][k] - r["x"][k]).max() < CF_TOL * max(1, np.abs(r["x"]).max())
    assert not near(g["flags"][0]).any()  # the kernel's own decisions on the shipped setups
    assert wrapdiff(g["q"][0], r["q"][2:22]).max() < 1e-12


@pytest.mark.parametrize("path", sorted(__import__("glob").glob(os.path.join(GOLDEN, "pgs_*.npz"))),
                         ids=lambda p: os.path.basename(p))
def test_golden_vectors(gpu, hmodels, path):
    z = np.load(path)
    p = gpu.read_pgs_config(PGS_CONFIG, int(z["sid"]))
    g = gpu.run_host(hmodels[str(z["xml"]).replace(".xml", "")], [p], n_t=int(z["n_t"]), horizon=int(z["n_t"]))
    assert np.abs(g["tau"][0] - z["tau"]).max() < TAU_TOL * max(1, np.abs(z["tau"]).max())
    assert np.abs(g["cf"][0] - z["cf"]).max() < CF_TOL * max(1, np.abs(z["cf"]).max())
    assert g["work_cot"][0, 1] == pytest.approx(float(z["cot"]), rel=1e-9)


def test_golden_synthetic_batch(gpu, hmodels):
    z = np.load(os.path.join(GOLDEN, "synth_hexapod16.npz"))
    params = golden_params(z["params"])
    g = gpu.run_host(hmodels["hexapod"], params, n_t=20, horizon=20)
    scale = np.maximum(1, np.abs(z["tau"]).max(axis=(1, 2)))
    assert (np.abs(g["tau"] - z["tau"]).max(axis=(1, 2)) < 1e-6 * scale).all()  # north_star bound
    np.testing.assert_allclose(g["work_cot"][:, 1], z["cot"], rtol=1e-8)


@pytest.mark.parametrize("name,curved", [("hexapod", False), ("hexapod", True), ("spider", False),
                                         ("spider", True), ("myant", False)])
def test_synthetic_batches_match_oracle(gpu, hmodels, oracle_mod, omodels, name, curved):
    from hslabs_amd import synth

    B = 96
    params = synth.gen_params(B, name, id0=12345, curved=curved)
    g = gpu.run_host(hmodels[name], params, n_t=20, horizon=20)
    gaits = [record_to_oracle_gait(oracle_mod, r) for r in params]
    f = oracle_mod.batch(omodels[name], gaits, 20, 0, 20, basis=oracle_mod.BASIS_FAST, n_threads=8)
    check_fast_every_step(f"{name} curved={curved}", g, f)
    r = oracle_mod.batch(omodels[name], gaits, 20, 0, 20, basis=oracle_mod.BASIS_TREE, n_threads=8)
    compare(f"{name} curved={curved} vs tree", g, r, oracle_mod, omodels[name], gaits, oracle_mod.BASIS_TREE,
            min_work=0.95)


def test_window_decomposition_is_bitwise_stable(gpu, hmodels):
    """Steps are independent given their 5-sample window: solving k0..k0+H-1 in any split
    gives the same bits as the full cycle."""
    from hslabs_amd import synth

    params = synth.gen_params(32, "hexapod", id0=99)
    full = gpu.run_host(hmodels["hexapod"], params, n_t=20, k0=0, horizon=20)
    for k0, H in [(0, 1), (7, 3), (19, 1), (5, 15)]:
        part = gpu.run_host(hmodels["hexapod"], params, n_t=20, k0=k0, horizon=H)
        assert np.array_equal(part["tau"], full["tau"][:, k0:k0 + H])
        assert np.array_equal(part["cf"], full["cf"][:, k0:k0 + H])


def test_accumulate_matches_full_cycle_work(gpu, hmodels):
    import torch

    from hslabs_amd import synth

    params = synth.gen_params(64, "hexapod", id0=7)
    full = gpu.run_host(hmodels["hexapod"], params, n_t=20, k0=0, horizon=20, want=("work_cot",))
    b = gpu.DeviceBatch(hmodels["hexapod"], params, n_t=20, k0=0, horizon=1)
    b.work_cot.zero_()
    for k in range(20):
        b.k0 = k
        b.run(accumulate=True)
    torch.cuda.synchronize()
    wc = b.work_cot.cpu().numpy()
    assert np.array_equal(wc[:, 0], full["work_cot"][:, 0])  # same summation order -> same bits
    assert np.array_equal(wc[:, 1], full["work_cot"][:, 1])


def test_run_steps_matches_launch_loop(gpu, hmodels):
    """hs_run_steps (native launch loop, k0 wrapping the cycle) == the same launches one by one;
    an odd batch leaves the last wavefront's second half idle."""
    import torch

    from hslabs_amd import synth

    params = synth.gen_params(257, "hexapod", id0=3)
    m = hmodels["hexapod"]
    a = gpu.DeviceBatch(m, params, n_t=20, horizon=1)
    b = gpu.DeviceBatch(m, params, n_t=20, horizon=1)
    a.work_cot.zero_()
    b.work_cot.zero_()
    for s in range(27):
        a.k0 = s % 20
        a.run(best=False, accumulate=True)
    b.k0 = 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(54)]
    b.run_steps(27, best=False, accumulate=True, events=ev)
    torch.cuda.synchronize()
    assert torch.equal(a.work_cot, b.work_cot)
    assert torch.equal(a.tau, b.tau) and torch.equal(a.cf, b.cf) and torch.equal(a.flags, b.flags)
    assert all(ev[2 * i].elapsed_time(ev[2 * i + 1]) > 0 for i in range(27))


def test_setup_cache_is_per_call_and_per_stream(gpu, hmodels):
    """The gait setup stored by a call's first launch (and loaded by its later ones) never
    reaches another call: interleaved calls with other gait parameters, on one stream and on
    two streams, give the bits of independent runs."""
    import torch

    from hslabs_amd import synth

    m = hmodels["hexapod"]
    pa, pb = synth.gen_params(96, "hexapod", id0=11), synth.gen_params(96, "hexapod", id0=12, curved=True)
    ref_a = gpu.run_host(m, pa, n_t=20, k0=3, horizon=4)
    ref_b = gpu.run_host(m, pb, n_t=20, k0=3, horizon=4)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for sa, sb in [(s1, s1), (s1, s2)]:
        a = gpu.DeviceBatch(m, pa, n_t=20, k0=3, horizon=2)
        b = gpu.DeviceBatch(m, pb, n_t=20, k0=3, horizon=2)
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(2):  # a, b, a, b: each call's second launch loads that call's setup
            a.run(stream=sa, best=False)
            b.run(stream=sb, best=False)
            sa.synchronize()
            sb.synchronize()
            ta.append(a.tau.cpu().numpy().copy())
            tb.append(b.tau.cpu().numpy().copy())
            a.k0, b.k0 = 5, 5
        assert np.array_equal(np.concatenate(ta, axis=1), ref_a["tau"])
        assert np.array_equal(np.concatenate(tb, axis=1), ref_b["tau"])


def test_device_batch_best_key(gpu, hmodels):
    import torch

    from hslabs_amd import dist as hdist
    from hslabs_amd import synth

    params = synth.gen_params(512, "hexapod", id0=4096)
    b = gpu.DeviceBatch(hmodels["hexapod"], params, n_t=20, k0=0, horizon=20, rollout_id_base=4096)
    b.reset_best()
    b.run(best=True)
    torch.cuda.synchronize()
    L = torch.from_numpy(params["step_length"].copy()).to(b.work_cot.device)
    sel = hdist.select_cot(b.work_cot[:, 0], L, hmodels["hexapod"].total_mass, 20, 20)
    c_kernel, id_kernel = gpu.decode_best_key(int(b.best_key.item()) & 0xFFFFFFFFFFFFFFFF)
    c_torch, id_torch = hdist.decode(hdist.best_key(sel, 4096))
    cot = sel.cpu().numpy().astype(np.float32)
    ref = int(np.nanargmin(cot))
    assert id_kernel == id_torch == 4096 + ref
    assert c_kernel == c_torch == cot[ref]
    # one cycle (key_steps = n_t): the selection COT is |reference COT|
    wc = b.work_cot.cpu().numpy()
    ok = np.abs(params["step_length"]) >= 1e-3
    np.testing.assert_array_equal(sel.cpu().numpy()[ok], np.abs(wc[ok, 1]))


def test_full_size_properties(gpu, hmodels):
    """BASELINE configs[1] size (B = 4096, H = 1) over a whole cycle: no NaN, torso
    actuation eliminated wherever >= 3 feet are down, contact forces balance the
    total momentum rate + weight (sum over feet = sum_i f_i - torso force)."""
    import torch

    from hslabs_amd import synth

    m = hmodels["hexapod"]
    params = synth.gen_params(4096, "hexapod")
    b = gpu.DeviceBatch(m, params, n_t=20, k0=0, horizon=1, outputs=("tau", "cf", "x", "flags", "work_cot"))
    n = m.n_parts
    for k in (0, 7, 13):
        b.k0 = k
        b.run(best=False)
        torch.cuda.synchronize()
        flags = b.flags.cpu().numpy()[:, 0]
        x = b.x.cpu().numpy()[:, 0]
        cf = b.cf.cpu().numpy()[:, 0].reshape(-1, 6, 3)
        assert not (flags & 8).any(), "NaN flagged"
        assert np.isfinite(b.tau.cpu().numpy()).all()
        ndown = (np.abs(cf).max(axis=2) > 0).sum(axis=1)
        good = (ndown >= 3) & ((flags & 0x7) == 0) & ((flags & 256) == 0)
        assert good.mean() > 0.5
        torso = np.concatenate([x[:, :3], x[:, 3 * n:3 * n + 3]], axis=1)
        scale = np.maximum(1, np.abs(cf).max(axis=(1, 2)))
        assert (np.abs(torso[good]).max(axis=1) < 1e-9 * scale[good]).all()


def test_straight_leg_steps_use_augmented_closed_form(gpu, hmodels, oracle_mod, omodels):
    """IK-clamped steps (singular D_c) go through the kernel's augmented-system tier, not the
    Eigen-style path, and match the oracle's fast and tree modes."""
    from hslabs_amd import synth
    from test_oracle import DEGENERATE_MYANT

    arr = synth.gen_params(4096, "myant")[list(DEGENERATE_MYANT)]
    g = gpu.run_host(hmodels["myant"], arr, n_t=20, horizon=20)
    assert not (g["flags"] & 64).any()
    assert ((g["flags"] & 16) != 0).sum() >= 10
    gaits = [record_to_oracle_gait(oracle_mod, r) for r in arr]
    f = oracle_mod.batch(omodels["myant"], gaits, 20, 0, 20, basis=oracle_mod.BASIS_FAST, n_threads=8)
    check_fast_every_step("straight legs", g, f)
    r = oracle_mod.batch(omodels["myant"], gaits, 20, 0, 20, basis=oracle_mod.BASIS_TREE, n_threads=8)
    compare("straight legs vs tree", g, r, oracle_mod, omodels["myant"], gaits, oracle_mod.BASIS_TREE, min_work=1.0)


def test_edge_cases(gpu, hmodels):
    from hslabs_amd import PgsConfigParams

    m = hmodels["hexapod"]
    # torso lifted far above reach: legs clamp straight (ignore_reach), no foot touches the ground
    up = PgsConfigParams(torso_pos=(0, 0, 1.5), step_duration=1, period=3, step_length=0.2, step_height=0.05)
    r = gpu.run_host(m, [up], n_t=20, horizon=4)
    assert (r["flags"] & 16).all()   # HS_FLAG_UNREACH
    assert (r["flags"] & 32).all()   # HS_FLAG_NO_CONTACT: k = 0
    assert (r["cf"] == 0).all()
    # without ignore_reach the reference would exit(1); here the step is flagged instead
    r2 = gpu.run_host(m, [up], n_t=20, horizon=2, ignore_reach=False)
    assert (r2["flags"] & 16).all()
    # single rollout, long horizon (several cycles), k0 > n_t
    base = gpu.read_pgs_config(PGS_CONFIG, 8)
    r3 = gpu.run_host(m, [base], n_t=20, k0=25, horizon=40)
    r4 = gpu.run_host(m, [base], n_t=20, k0=5, horizon=1)
    assert np.abs(r3["tau"][0, 0] - r4["tau"][0, 0]).max() < 1e-9  # periodic in time (one cycle later)
    # large batch (config 4 shard size) completes
    from hslabs_amd import synth

    big = gpu.run_host(m, synth.gen_params(32768, "hexapod"), n_t=20, horizon=1, want=("tau", "flags"))
    assert np.isfinite(big["tau"]).all()


@pytest.mark.parametrize("horizon", [1, 20])
def test_mixed_batch_matches_single_model_runs(gpu, hmodels, horizon):
    """BASELINE configs[4]: myant + hexapod interleaved in one launch == each model's own
    launch, bit for bit (same arithmetic; the LDS layout is sized to the larger model);
    output rows padded to the larger model's dimensions with zeros."""
    import torch

    from hslabs_amd import synth

    params, idx = synth.gen_mixed(301, id0=5)
    ms = [hmodels[n] for n in synth.MIXED_MODELS]
    mb = gpu.MixedBatch(ms, idx, params, n_t=20, horizon=horizon, outputs=("tau", "cf", "q", "x", "flags", "work_cot"))
    assert (mb.dims.nmj, mb.dims.nfeet, mb.dims.config_dim, mb.dims.n_parts) == (18, 6, 24, 22)
    mb.work_cot.zero_()
    mb.k0 = 3
    mb.run(best=False, accumulate=True)
    torch.cuda.synchronize()
    for k, m in enumerate(ms):
        sel = np.nonzero(idx == k)[0]
        sb = gpu.DeviceBatch(m, params[sel], n_t=20, k0=3, horizon=horizon,
                             outputs=("tau", "cf", "q", "x", "flags", "work_cot"))
        sb.work_cot.zero_()
        sb.run(best=False, accumulate=True)
        torch.cuda.synchronize()
        t = torch.from_numpy(sel).to(mb.tau.device)
        assert torch.equal(mb.tau[t][:, :, :m.nmj], sb.tau)
        assert torch.equal(mb.cf[t][:, :, :3 * m.nfeet], sb.cf)
        assert torch.equal(mb.q[t][:, :, :m.config_dim], sb.q)
        assert torch.equal(mb.x[t][:, :, :6 * m.n_parts], sb.x)
        assert torch.equal(mb.flags[t], sb.flags) and torch.equal(mb.work_cot[t], sb.work_cot)
        assert (mb.tau[t][:, :, m.nmj:] == 0).all() and (mb.cf[t][:, :, 3 * m.nfeet:] == 0).all()
        assert (mb.x[t][:, :, 6 * m.n_parts:] == 0).all()


def test_mixed_batch_matches_oracle(gpu, hmodels, oracle_mod, omodels):
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(24, id0=1000)
    mb = gpu.MixedBatch([hmodels[n] for n in synth.MIXED_MODELS], idx, params, n_t=20, horizon=20)
    mb.run(best=False)
    import torch

    torch.cuda.synchronize()
    tau = mb.tau.cpu().numpy()
    for b in range(24):
        name = synth.MIXED_MODELS[idx[b]]
        r = oracle_mod.rollout(omodels[name], record_to_oracle_gait(oracle_mod, params[b]), 20,
                               basis=oracle_mod.BASIS_FAST)
        nmj = hmodels[name].nmj
        assert np.abs(tau[b, :, :nmj] - r["tau"]).max() < 1e-6 * max(1, np.abs(r["tau"]).max())


@pytest.mark.parametrize("name", ["hexapod", "spider", "myant"])
def test_forces_given_torques_match_oracle(gpu, hmodels, oracle_mod, omodels, name):
    """hs_run_forces (solve_forces, ftsolver.cpp:331-378): the kernel's reduced weighted least
    squares equals the oracle's dense Householder LS, for torques inconsistent with the motion, on
    every step neither side flags HS_FLAG_NEAR_RANK. No step of these inputs is rank deficient: the
    steps that drop a force component (the basic solution, HS_FLAG_GENERAL | HS_FLAG_DEPENDENT) are
    test_forces_lifted_torso_matches_oracle's, and the fp32 build's tests/test_gpu_forces_f32_oracle.py's."""
    import torch

    from hslabs_amd import synth

    m = hmodels[name]
    params = synth.gen_params(12, name, id0=4321)
    full = gpu.DeviceBatch(m, params, n_t=20, horizon=20, outputs=("tau", "cf"))
    full.run(best=False)
    tau = full.tau + 0.25 * torch.cos(torch.arange(20, device=full.tau.device)[None, :, None]
                                      + torch.arange(m.nmj, device=full.tau.device)[None, None, :])
    fb = gpu.DeviceBatch(m, params, n_t=20, horizon=20, outputs=("cf", "flags"))
    fb.run_forces(tau)
    torch.cuda.synchronize()
    cf, flags, tz = fb.cf.cpu().numpy(), fb.flags.cpu().numpy(), tau.cpu().numpy()
    fo = oracle_mod.forces_batch(omodels[name], [record_to_oracle_gait(oracle_mod, r) for r in params], tz, 20,
                                 n_threads=8)
    skip = near(flags, fo["flags"])
    check_flags(flags, fo["flags"], f"{name} forces", skip)
    assert np.array_equal((flags & 64)[~skip], (fo["flags"] & 64)[~skip])
    scale = np.maximum(1.0, np.abs(fo["cf"]).max(axis=-1))
    err = np.abs(cf - fo["cf"]).max(axis=-1)
    assert (err[~skip] < 1e-9 * scale[~skip]).all(), f"{name} forces: max rel {(err / scale)[~skip].max():.3e}"


@pytest.mark.parametrize("name", ["hexapod", "spider", "myant"])
def test_forces_dense_path_matches_limb_blocks(gpu, hmodels, oracle_mod, omodels, name):
    """solve_forces' two routes: the 6 x 6 system after the limbs' block elimination (HS_SOLVE_AUTO,
    where every foot's block B_f is well conditioned) and the dense normal equations over the feet
    (the route of a near-singular B_f; every step with HS_SOLVE_REFERENCE) give the same forces, and
    the dense route matches the oracle's Householder least squares."""
    import torch

    from hslabs_amd import synth

    m = hmodels[name]
    params = synth.gen_params(64, name, id0=555)
    full = gpu.DeviceBatch(m, params, n_t=20, horizon=20, outputs=("tau",))
    full.run(best=False)
    tau = full.tau + 0.3 * torch.sin(torch.arange(20, device=full.tau.device)[None, :, None] * 0.7
                                     + torch.arange(m.nmj, device=full.tau.device)[None, None, :])
    out = {}
    for mode in (gpu.capi.HS_SOLVE_AUTO, gpu.capi.HS_SOLVE_REFERENCE):
        fb = gpu.DeviceBatch(m, params, n_t=20, horizon=20, outputs=("cf", "flags"))
        fb.solve_mode = mode
        fb.run_forces(tau)
        torch.cuda.synchronize()
        out[mode] = (fb.cf.cpu().numpy(), fb.flags.cpu().numpy())
    (ca, fa), (cd, fd) = out[gpu.capi.HS_SOLVE_AUTO], out[gpu.capi.HS_SOLVE_REFERENCE]
    nr = ~np.uint32(256)  # the 6 x 6 route takes no rank decision, so only the dense one can be near one
    assert np.array_equal(fa & nr, fd & nr)
    scale = np.maximum(1, np.abs(cd).max(axis=-1))
    skip = near(fd)
    assert (np.abs(ca - cd).max(axis=-1)[~skip] < 1e-9 * scale[~skip]).all()
    tz = tau.cpu().numpy()
    fo = oracle_mod.forces_batch(omodels[name], [record_to_oracle_gait(oracle_mod, r) for r in params], tz, 20,
                                 n_threads=8)
    skip = near(fd, fo["flags"])
    err = np.abs(cd - fo["cf"]).max(axis=-1) / np.maximum(1.0, np.abs(fo["cf"]).max(axis=-1))
    assert (err[~skip] < 1e-9).all()


@pytest.mark.parametrize("name,B,n_calls,ch", [("hexapod", 12, 1, 20), ("hexapod", 97, 7, 3), ("myant", 300, 300, 1)])
def test_forces_calls_bitwise_equal_run_forces(gpu, hmodels, name, B, n_calls, ch):
    """hs_run_forces_calls (the fused form) writes exactly what n_calls calls of hs_run_forces
    write (call horizon ch, k0 marching by ch through the cycle, hs_run_steps semantics): one call
    of 20 steps, an odd batch (idle half-wavefront), and S = 300 > the launch's step chunk at small
    B (two step launches)."""
    import torch

    from hslabs_amd import synth

    m = hmodels[name]
    S, k0 = n_calls * ch, 3
    params = synth.gen_params(B, name, id0=97 + B)
    full = gpu.DeviceBatch(m, params, n_t=20, k0=k0, horizon=S, outputs=("tau",))
    full.run(best=False)
    tau = full.tau + 0.1 * torch.sin(torch.arange(S, device=full.tau.device)[None, :, None]
                                     + torch.arange(m.nmj, device=full.tau.device)[None, None, :])
    fz = gpu.DeviceBatch(m, params, n_t=20, k0=k0, horizon=S, outputs=("cf", "q", "flags"))
    fz.run_forces_calls(tau, n_calls, call_horizon=ch)
    ref = gpu.DeviceBatch(m, params, n_t=20, k0=k0, horizon=ch, outputs=("cf", "q", "flags"))
    cf, q, fl = [], [], []
    for i in range(n_calls):
        ref.k0 = (k0 + i * ch) % 20
        ref.run_forces(tau[:, i * ch:(i + 1) * ch])
        cf.append(ref.cf.clone())
        q.append(ref.q.clone())
        fl.append(ref.flags.clone())
    torch.cuda.synchronize()
    assert torch.equal(fz.cf, torch.cat(cf, dim=1))
    assert torch.equal(fz.q, torch.cat(q, dim=1))
    assert torch.equal(fz.flags, torch.cat(fl, dim=1))
    assert torch.isfinite(fz.cf).all()


def test_forces_bench_shape_matches_oracle(gpu, hmodels, oracle_mod, omodels):
    """solve_forces at the bench's shape (bench.py --forces: hexapod B = 4096, K = 20 fused calls of
    horizon 1, hs_run_forces_calls), with the control loop's torques perturbed so the forces are not
    just its own contact forces, against the oracle's least squares on EVERY step neither side flags
    HS_FLAG_NEAR_RANK: forces within 1e-9 * max(1, |f|), flags identical. The recorded runs of this shape
    hold no rank-deficient step (the count is printed); those are test_forces_lifted_torso_matches_oracle's."""
    import torch

    from hslabs_amd import synth

    m = hmodels["hexapod"]
    B, K = 4096, 20
    from test_gpu_parity import threads

    params = synth.gen_params(B, "hexapod")
    ctl = gpu.DeviceBatch(m, params, n_t=20, k0=0, horizon=K, outputs=("tau",))
    ctl.run_calls(K, call_horizon=1)
    i = torch.arange(K, device=ctl.tau.device)[None, :, None]
    j = torch.arange(m.nmj, device=ctl.tau.device)[None, None, :]
    bb = torch.arange(B, device=ctl.tau.device)[:, None, None]
    tau = ctl.tau + 0.2 * torch.sin(0.7 * i + 1.3 * j + 0.01 * bb)
    fb = gpu.DeviceBatch(m, params, n_t=20, k0=0, horizon=K, outputs=("cf", "flags"))
    fb.forces_launcher(tau, K)()
    torch.cuda.synchronize()
    cf, flags = fb.cf.cpu().numpy(), fb.flags.cpu().numpy().astype(np.uint32)
    fo = oracle_mod.forces_batch(omodels["hexapod"], [record_to_oracle_gait(oracle_mod, r) for r in params],
                                 tau.cpu().numpy(), 20, n_threads=threads())
    skip = near(flags, fo["flags"])
    print(f"forces bench shape: {int(skip.sum())} of {skip.size} steps flagged HS_FLAG_NEAR_RANK, "
          f"{int(((flags & 64) != 0).sum())} rank-deficient (basic solution)")
    check_flags(flags, fo["flags"], "forces bench shape", skip)
    assert np.array_equal((flags & 64)[~skip], (fo["flags"] & 64)[~skip])
    assert np.isfinite(cf).all()
    err = np.abs(cf - fo["cf"]).max(axis=-1) / np.maximum(1.0, np.abs(fo["cf"]).max(axis=-1))
    assert (err[~skip] < 1e-9).all(), f"forces bench shape: {(err[~skip] >= 1e-9).sum()} steps over 1e-9"


def lifted_torso_run(gpu, hmodels, oracle_mod, omodels, name):
    """the lifted-torso batch of `name` (forces_gpu_kit.lifted_batch) in fp64 through hs_run_forces and
    hs_run_forces_calls, bit for bit the same, and the fp64 oracle on it: (gaits, tau, lifted rows, kernel, oracle)"""
    import torch

    from forces_gpu_kit import kernel_forces, lifted_batch

    O, om = oracle_mod, omodels[name]
    params, gaits, tau, rows = lifted_batch(O, om, name)
    fo = O.forces_batch(om, gaits, tau, 20)
    a = kernel_forces(gpu, hmodels[name], params, tau, torch.float64)
    n0 = gpu.api.limb_launches()
    b = kernel_forces(gpu, hmodels[name], params, tau, torch.float64, calls=True)
    assert gpu.api.limb_launches() > n0  # the limb-lane kernel and its forces fixup launch
    assert np.array_equal(a["cf"], b["cf"]) and np.array_equal(a["flags"], b["flags"])
    return gaits, tau, rows, a, fo


@pytest.mark.parametrize("name", ["hexapod", "myant"])
def test_forces_lifted_torso_flags_and_drops(gpu, hmodels, oracle_mod, omodels, name):
    """solve_forces' rank-deficient and singular-block steps in fp64: the lifted-torso cases (test_oracle.
    LIFTED_CASES) interleaved with ordinary rollouts, through hs_run_forces and hs_run_forces_calls (the
    limb-lane kernel, which defers these steps to its forces fixup launch), bit for bit the same. Where
    neither side flags HS_FLAG_NEAR_RANK: equal flags (GENERAL | DEPENDENT included) and the same components
    exactly 0; the hexapod has at least 12 such clean-drop steps (flag 592), myant 1.2 (every B_f singular,
    full rank: the dense route without a drop) all 20. Where a side flags NEAR_RANK the dropped sets may differ
    and the solution is not unique: the kernel's forces are finite, DEPENDENT is set exactly where a component
    is exactly 0, and gamma (test_forces_oracle_f32: the least squares' gradient over the kernel's own kept
    columns) is at most 10 x the oracle's largest on those steps -- a rounding residual of another
    factorisation, not a like-for-like quantity. The forces themselves: test_forces_lifted_torso_matches_oracle."""
    from test_forces_oracle_f32 import CLEAN_DROP, dependent_where_zero, dropped_set, gammas

    O, om = oracle_mod, omodels[name]
    gaits, tau, rows, a, fo = lifted_torso_run(gpu, hmodels, O, omodels, name)
    assert np.isfinite(a["cf"]).all() and not (a["flags"] & 8).any()
    skip = near(a["flags"], fo["flags"])
    k = ~skip
    assert np.array_equal(a["flags"][k], fo["flags"][k])
    assert np.array_equal(dropped_set(a["cf"])[k], dropped_set(fo["cf"])[k])
    assert dependent_where_zero(a["cf"], a["flags"])
    n_drop = int(((fo["flags"] == CLEAN_DROP) & k).sum())
    print(f"{name} lifted fp64: {int(k.sum())} of {k.size} steps compared, {n_drop} clean drops (flag 592), "
          f"{int(skip.sum())} flagged HS_FLAG_NEAR_RANK")
    if name == "hexapod":
        assert n_drop >= 12
    else:
        assert k[rows].all() and (fo["flags"][rows] == 16).all()
    if skip.any():
        steps = [np.nonzero(skip[r])[0] for r in range(len(gaits))]
        g_k = np.concatenate([gammas(O, om, gaits[r], tau[r], a["cf"][r], steps[r]) for r in range(len(gaits))])
        g_o = np.concatenate([gammas(O, om, gaits[r], tau[r], fo["cf"][r], steps[r]) for r in range(len(gaits))])
        same = (dropped_set(a["cf"]) == dropped_set(fo["cf"])).all(axis=-1)
        print(f"{name} lifted fp64, the {int(skip.sum())} near-rank steps: gamma kernel {g_k.max():.2e}, oracle "
              f"{g_o.max():.2e} ({g_k.max() / g_o.max():.2f} x); dropped sets equal on {int((same & skip).sum())}")
        assert g_k.max() <= 10 * g_o.max()


@pytest.mark.parametrize("name", ["hexapod", "myant"])
def test_forces_lifted_torso_matches_oracle(gpu, hmodels, oracle_mod, omodels, name):
    """The forces of the lifted-torso batches in fp64, on every step neither side flags HS_FLAG_NEAR_RANK, within
    1e-9 max(1, max |f|) of the oracle's (the project's fp64 bound), the clean-drop steps and myant 1.2 included.
    Measured on MI355X (profiles/forces_f32_oracle.txt): the 16 clean drops within 1.9e-13, myant's lifted steps
    within 1.9e-14, the ordinary rollouts within 2.8e-15, and 3.6e-10 on the worst of 4 steps of the hexapod lifted
    to 1.0 that keep all 18 columns with the smallest squared pivot 5.8e-10 .. 7.5e-10 of the largest reduced
    diagonal (over 4 x the 1e-10 guard, so not flagged; cond(N) 4.4e10 .. 6.3e10, forces of 1.5 .. 3.8 kN). Those 4
    steps were at 1.4e-7 .. 2.7e-6 before the dense route's corrected-semi-normal-equations step: the normal
    equations alone lose cond(N) eps, the oracle's Householder QR sqrt(cond(N)) eps."""
    from test_forces_oracle_f32 import CLEAN_DROP, spread

    gaits, tau, rows, a, fo = lifted_torso_run(gpu, hmodels, oracle_mod, omodels, name)
    k = ~near(a["flags"], fo["flags"])
    err = spread(a["cf"], fo["cf"])
    lifted = np.zeros_like(k)
    lifted[rows] = True
    for what, sel in (("clean drops (592)", k & (fo["flags"] == CLEAN_DROP)), ("lifted, no drop", k & lifted & ((fo["flags"] & 512) == 0)),
                      ("ordinary rollouts", k & ~lifted)):
        if sel.any():
            print(f"{name} lifted fp64, {what}: {int(sel.sum())} steps, max rel {err[sel].max():.2e}, "
                  f"{int((err[sel] >= 1e-9).sum())} at or over 1e-9")
    assert (err[k] < 1e-9).all(), f"{name} lifted: {int((err[k] >= 1e-9).sum())} steps over 1e-9, max rel {err[k].max():.3e}"


def test_forces_calls_fp32(gpu, hmodels):
    """The single-precision build of solve_forces: the fused form is bitwise the per-call form, and
    both stay near the fp64 forces where the least squares is well posed (no HS_FLAG_GENERAL)."""
    import torch

    from hslabs_amd import synth

    m = hmodels["hexapod"]
    params = synth.gen_params(256, "hexapod", id0=2024)
    full = gpu.DeviceBatch(m, params, n_t=20, k0=0, horizon=20, outputs=("tau",))
    full.run_calls(20)
    ref = gpu.DeviceBatch(m, params, n_t=20, k0=0, horizon=20, outputs=("cf", "flags"))
    ref.run_forces(full.tau)
    f32a = gpu.DeviceBatch(m, params, n_t=20, k0=0, horizon=20, outputs=("cf", "flags"), dtype=torch.float32)
    f32a.run_forces(full.tau)
    f32b = gpu.DeviceBatch(m, params, n_t=20, k0=0, horizon=20, outputs=("cf", "flags"), dtype=torch.float32)
    f32b.run_forces_calls(full.tau, 20)
    torch.cuda.synchronize()
    assert torch.equal(f32a.cf, f32b.cf) and torch.equal(f32a.flags, f32b.flags)
    c64, c32 = ref.cf.cpu().numpy(), f32b.cf.double().cpu().numpy()
    ok = ((ref.flags.cpu().numpy() & 72) == 0) & ((f32b.flags.cpu().numpy() & 72) == 0)  # GENERAL | NAN
    assert ok.mean() > 0.9
    err = np.abs(c32 - c64).max(axis=-1) / np.maximum(1, np.abs(c64).max(axis=-1))
    assert np.isfinite(c32[ok]).all() and np.median(err[ok]) < 1e-3


PD_CASES = [(0, 1), (7, 1), (19, 1), (18, 3)]  # (k0, H); H = 3 at k0 = 18 wraps tsi within the call


def pd_run(gpu, m, params, k0, H, rng, dtype):
    """hs_run_pd on random measurements [B][H][nmj] of `dtype`: the batch, (q, dq) on the host, (cmd, q0, dq0)"""
    import torch

    b = gpu.DeviceBatch(m, params, n_t=20, k0=k0, horizon=H, outputs=("tau",), dtype=dtype)
    q = torch.from_numpy(rng.uniform(-np.pi, np.pi, (len(params), H, m.nmj))).to(dtype).cuda()
    dq = torch.from_numpy(rng.uniform(-3, 3, (len(params), H, m.nmj))).to(dtype).cuda()
    out = b.run_pd(q, dq, k=100.0, targets=True)
    torch.cuda.synchronize()
    assert all(o.dtype == dtype for o in out)
    plain = gpu.DeviceBatch(m, params, n_t=20, k0=k0, horizon=1, outputs=("tau",), dtype=dtype)
    for h in range(H):  # the step's feedforward was written too: a plain run()'s torques of the cycle's step
        plain.k0 = (k0 + h) % 20
        plain.run(best=False)
        torch.cuda.synchronize()
        assert torch.equal(b.tau[:, h], plain.tau[:, 0]), (k0, h)
    return (q.double().cpu().numpy(), dq.double().cpu().numpy()), [o.double().cpu().numpy() for o in out]


def test_position_control_matches_oracle(gpu, hmodels, oracle_mod, omodels):
    """hs_run_pd (player.cpp:388-432) against the oracle's control law on all three models, over the cycle
    incl. the wrap of tsi into [2, n_t + 1] (k0 = tsi - 2), between calls and within one (H = 3)."""
    import torch

    from hslabs_amd import synth

    for name in ("hexapod", "spider", "myant"):
        m = hmodels[name]
        params = synth.gen_params(16, name, id0=777)
        rng = np.random.default_rng(5)
        for k0, H in PD_CASES:
            (q, dq), (cmd, q0, dq0) = pd_run(gpu, m, params, k0, H, rng, torch.float64)
            for i in (0, 5, 15):
                og = record_to_oracle_gait(oracle_mod, params[i])
                for h in range(H):
                    ref, rq0, rdq0 = oracle_mod.pd_torques(omodels[name], og, k0 + h + 2, q[i, h], dq[i, h], k=100.0)
                    assert np.abs(q0[i, h] - rq0).max() < 1e-12
                    assert np.abs(dq0[i, h] - rdq0).max() < 1e-9 * max(1, np.abs(rdq0).max())
                    assert np.abs(cmd[i, h] - ref).max() < 1e-9 * max(1, np.abs(ref).max())


@pytest.mark.parametrize("name", ["hexapod", "spider", "myant"])
def test_position_control_fp32(gpu, hmodels, oracle_mod, omodels, name):
    """hs_run_pd with HS_PREC_F32 (float q_meas, dq_meas and outputs) against the fp64 oracle's control law at
    the float-rounded measurements: tau_cmd, q_target and dq_target within FP32_TOL, each relative to
    max(1, |ref|) of the step (FP32_TOL's own definition). Measured on MI355X, tau_cmd / q_target / dq_target:
    hexapod 7.4e-7 / 1.3e-6 / 3.8e-6, spider 5.4e-7 / 4.4e-7 / 5.0e-6, myant 5.1e-6 / 2.9e-6 / 3.8e-5."""
    import torch

    from hslabs_amd import synth

    m = hmodels[name]
    params = synth.gen_params(16, name, id0=777)
    rng = np.random.default_rng(5)
    worst = np.zeros(3)
    for k0, H in PD_CASES:
        (q, dq), out = pd_run(gpu, m, params, k0, H, rng, torch.float32)
        for i in range(16):
            og = record_to_oracle_gait(oracle_mod, params[i])
            for h in range(H):
                ref = oracle_mod.pd_torques(omodels[name], og, k0 + h + 2, q[i, h], dq[i, h], k=100.0)
                worst = np.maximum(worst, [np.abs(o[i, h] - r).max() / max(1, np.abs(r).max()) for o, r in zip(out, ref)])
    print(f"{name} position control fp32 vs the fp64 oracle: tau_cmd {worst[0]:.2e} q_target {worst[1]:.2e} "
          f"dq_target {worst[2]:.2e}")
    assert worst[0] < FP32_TOL
    assert worst[1] < FP32_TOL
    assert worst[2] < FP32_TOL


@pytest.mark.parametrize("sid", [8, 9, 24])
def test_complete_traj_matches_oracle(gpu, hmodels, oracle_mod, omodels, sid, tmp_path):
    """periodic::get_complete_traj (periodic.cpp:406-426) / record_per_traj's traj.txt:
    rows tsi = 0 .. n_t-1 (tsi < 2 read at tsi + n_t) of (q, compute_vel_traj rates, torques)."""
    p = gpu.read_pgs_config(PGS_CONFIG, sid)
    name = p.fname.replace(".xml", "")
    m = hmodels[name]
    rec = gpu.complete_traj(m, [p], 20)[0]
    r = oracle_mod.rollout(omodels[name], to_oracle_gait(oracle_mod, p), 20, basis=oracle_mod.BASIS_FAST)
    cfg, nmj, dt = m.config_dim, m.nmj, p.period / 20
    for tsi in range(20):
        i = tsi + 20 if tsi < 2 else tsi
        d = r["q"][i + 1] - r["q"][i - 1]
        d = np.where(d > np.pi, d - 2 * np.pi, np.where(d < -np.pi, d + 2 * np.pi, d))
        assert wrapdiff(rec[tsi, :cfg], r["q"][i]).max() < 1e-12
        assert np.abs(rec[tsi, cfg:2 * cfg] - d / (2 * dt)).max() < 1e-9
        assert np.abs(rec[tsi, 2 * cfg:] - r["tau"][i - 2]).max() < TAU_TOL * max(1, np.abs(r["tau"]).max())
    path = str(tmp_path / "traj.txt")
    out = gpu.ModelPlayer(m).record_per_traj(p, 20, path)
    rows = open(path).read().splitlines()
    assert len(rows) == 20 and len(rows[0].split()) == 2 * cfg + nmj
    np.testing.assert_allclose(np.loadtxt(path), out, rtol=1e-5, atol=1e-5)  # 6 significant digits


def contact_sets(cf, nf):
    return np.abs(cf.reshape(*cf.shape[:-1], nf, 3)).max(axis=-1) > 0


@pytest.mark.parametrize("name", ["hexapod", "spider", "myant"])
def test_fp32_matches_fp64(gpu, hmodels, name):
    """HS_PREC_F32 (BASELINE configs[2] precision) against the fp64 kernel (== oracle to 1e-12)
    on synthetic straight and curved gaits: within FP32_TOL wherever both precisions chose the
    same contact set; a contact decision (foot height within rounding of rcap + 1e-4) may flip
    on a handful of steps."""
    import torch

    from hslabs_amd import synth

    m = hmodels[name]
    for curved in (False, True):
        p = synth.gen_params(512, name, id0=2024, curved=curved)
        out = {}
        for dt in (torch.float64, torch.float32):
            b = gpu.DeviceBatch(m, p, n_t=20, horizon=20, outputs=("tau", "cf", "flags", "work_cot"), dtype=dt)
            b.run(best=False)
            torch.cuda.synchronize()
            assert b.tau.dtype == dt
            out[dt] = (b.tau.double().cpu().numpy(), b.cf.double().cpu().numpy(), b.flags.cpu().numpy())
        t64, c64, f64 = out[torch.float64]
        t32, c32, f32 = out[torch.float32]
        same = (contact_sets(c64, m.nfeet) == contact_sets(c32, m.nfeet)).all(axis=-1)
        assert same.mean() > 0.995
        err = np.abs(t32 - t64).max(axis=-1) / np.maximum(1, np.abs(t64).max(axis=-1))
        assert err[same].max() < FP32_TOL
        assert not (f32 & 8).any() and np.isfinite(t32).all()


def test_fp32_configs2_size(gpu, hmodels):
    """BASELINE configs[2]: spider, 16384 rollouts x horizon 32, fp32 -- finite, no NaN or
    general-path steps, and the first rollouts agree with fp64 within FP32_TOL."""
    import torch

    from hslabs_amd import synth

    m = hmodels["spider"]
    p = synth.gen_params(16384, "spider")
    b = gpu.DeviceBatch(m, p, n_t=20, horizon=32, outputs=("tau", "cf", "flags", "work_cot"),
                        dtype=torch.float32)
    b.work_cot.zero_()
    b.run_steps(2, best=False, accumulate=True)  # 64 steps, k0 marching through the cycle
    torch.cuda.synchronize()
    flags = b.flags.cpu().numpy()
    assert not (flags & (8 | 64)).any()
    assert torch.isfinite(b.tau).all() and torch.isfinite(b.work_cot).all()
    ref = gpu.DeviceBatch(m, p[:64], n_t=20, k0=12, horizon=32, outputs=("tau", "cf"))
    ref.run(best=False)
    torch.cuda.synchronize()
    t64, c64 = ref.tau.cpu().numpy(), ref.cf.cpu().numpy()
    t32, c32 = b.tau[:64].double().cpu().numpy(), b.cf[:64].double().cpu().numpy()  # 2nd call: k0 = 32 % 20
    same = (contact_sets(c64, m.nfeet) == contact_sets(c32, m.nfeet)).all(axis=-1)
    err = np.abs(t32 - t64).max(axis=-1) / np.maximum(1, np.abs(t64).max(axis=-1))
    assert same.mean() > 0.99 and err[same].max() < FP32_TOL


def test_forces_round_trip(gpu, hmodels):
    """modelplayer::test_dynamics (playerexperim.cpp:95-121) on the GPU at configs[1] size:
    forces recovered from the kernel's own torques equal its contact forces where >= 3 feet
    are down (torso actuation zero)."""
    import torch

    from hslabs_amd import synth

    m = hmodels["hexapod"]
    params = synth.gen_params(4096, "hexapod")
    b = gpu.DeviceBatch(m, params, n_t=20, k0=5, horizon=1, outputs=("tau", "cf"))
    b.run(best=False)
    f = gpu.DeviceBatch(m, params, n_t=20, k0=5, horizon=1, outputs=("cf", "flags"))
    f.run_forces(b.tau)
    torch.cuda.synchronize()
    cf, cf2 = b.cf.cpu().numpy()[:, 0], f.cf.cpu().numpy()[:, 0]
    nc = (np.abs(cf.reshape(-1, 6, 3)).max(axis=2) > 0).sum(axis=1)
    sel = nc >= 3
    assert sel.mean() > 0.5
    scale = np.maximum(1, np.abs(cf).max(axis=1))
    assert (np.abs(cf2 - cf).max(axis=1)[sel] < 1e-9 * scale[sel]).all()
