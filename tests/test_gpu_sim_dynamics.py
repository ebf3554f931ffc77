"""GPU checks of "dynamics from simulation" (hs_sim_config, hs_sim_track_push, hs_sim_probe,
hs_sim_regress_B, hs_sim_estimate_B) against the library's own sequential path
(open-loop hs_sim_trial steps, one probe after another), the oracle driven one step at a time
(tests/test_sim_dynamics.py: oracle_probes), the NumPy tracker and numpy.linalg.lstsq.

Shapes: B = 3 rollouts -- at rest at trajectory sample 2, and after 13 and 25 position-control steps,
which have a tracker history and other contact sets -- of the hexapod (pgs id 8) and myant (pgs id 9).
Bounds are those of tests/test_gpu_sim.py and tests/test_gpu_sim_trial.py: bodies 1e-10 (BODY_TOL),
hinge angles 1e-9; the configuration round trip has tests/test_gpu_config.py's 1e-12.
"""
import numpy as np
import pytest

from sim_gpu_kit import (BODY_TOL, NEVER, copy_state, gpu, models, moved, moved64, new_batch)  # noqa: F401
from test_sim_dynamics import CASES, MOVE_STEPS, TSI0, lstsq_Bt, np_probe_accel, np_track_push, oracle_probes

pytestmark = pytest.mark.gpu

Q_TOL = 1e-9
CFG_TOL = 1e-12
B = len(MOVE_STEPS)


def sequential_probes(seq, tau):
    """The reference's loop with existing kernels: for every probe j, one open-loop hs_sim_trial step of
    seq's state with tau[:, j] in the table row, the state put back and the seed carried. Advances
    seq.seed only. Returns body_out [B][m][n][13] and n_contacts [B][m]."""
    import torch

    body0, tsi0 = seq.body.clone(), seq.tsi.clone()
    rows = [seq.table_row(int(t)) for t in tsi0.cpu()]
    keep = seq.tables.tau.clone()
    bodies, ncs = [], []
    for j in range(tau.shape[1]):
        for b, r in enumerate(rows):
            seq.tables.tau[b, r] = tau[b, j]
        o = seq.trial(1, open_loop=True, check_from=NEVER, n_contacts=True)
        bodies.append(seq.body.clone())
        ncs.append(o["n_contacts"][:, 0].clone())
        seq.body.copy_(body0)
        seq.tsi.copy_(tsi0)
    seq.tables.tau.copy_(keep)
    assert (seq.state == -1).all()
    return torch.stack(bodies, 1), torch.stack(ncs, 1)


def dtau_for(gpu, sb, m, seed=0):
    import torch
    from hslabs_amd import synth

    return torch.as_tensor(synth.gen_torque_perturbations(sb.B, m, sb.model.nmj, seed=seed), dtype=sb.dtype,
                           device=sb.device)


# ---- 6. the configuration round trip
@pytest.mark.parametrize("name", sorted(CASES))
def test_config_round_trip(gpu, models, name):
    import torch

    sb = new_batch(gpu, models, name, n=1)
    m = sb.model
    rng = np.random.default_rng(11)
    c = np.empty((64, m.config_dim))
    c[:, :3] = rng.uniform(-1, 1, (64, 3))
    c[:, 3] = rng.uniform(-3, 3, 64)
    c[:, 4] = rng.uniform(-1.2, 1.2, 64)  # the singular angle of euler_angles_from_affine
    c[:, 5] = rng.uniform(-3, 3, 64)
    c[:, 6:] = rng.uniform(-2.5, 2.5, (64, m.nmj))
    ct = torch.as_tensor(c, device=sb.device)
    body = torch.empty((64, m.n_parts, 13), dtype=torch.float64, device=sb.device)
    st = torch.cuda.current_stream(sb.device).cuda_stream
    gpu.capi.check(gpu.capi.load().hs_sim_reset(m.handle, 64, ct.data_ptr(), m.config_dim, body.data_ptr(), 0, st))
    back = sb.config(body=body)
    err = (back - ct).abs().max().item()
    body[:, :, 3:7] *= -1  # the same rotations
    err_neg = (sb.config(body=body) - ct).abs().max().item()
    print(f"{name}: config(reset(c)) - c: {err:.3e}, quaternions negated {err_neg:.3e}")
    assert err < CFG_TOL and err_neg < CFG_TOL


@pytest.mark.parametrize("name", sorted(CASES))
def test_config_motor_part_is_the_oracles_hinge_angles(moved64, oracle_mod, omodels, name):
    sb = moved64[name][0]
    cfg, body = sb.config().cpu().numpy(), sb.body.cpu().numpy()
    for b in range(B):
        q, _ = oracle_mod.sim_hinges(omodels[name], body[b])
        assert np.abs(cfg[b, 6:] - q).max() < Q_TOL, (name, b)
    assert np.abs(cfg[:, :3] - body[:, 0, :3]).max() < 1.0  # the torso frame sits near its body


# ---- 7. the tracker
def test_track_push_is_the_numpy_restatement(gpu, models, moved64):
    hist = moved64["hexapod"][2]
    sb = new_batch(gpu, models, "hexapod")
    ders = np.zeros((B, 3, sb.model.config_dim))
    for i in range(5):
        c = sb.config(body=hist[10 + i].contiguous())
        sb.track_push(c)
        np_track_push(ders, c.cpu().numpy(), sb.params.dt)
        assert np.array_equal(sb.ders.cpu().numpy(), ders), i
    assert np.abs(ders[:, 2]).max() > 0


# ---- 8. probes against the sequential path of existing kernels
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_probes_match_sequential_trial_steps(gpu, models, moved64, name, prec):
    import torch

    if prec == "f64":
        src, tau0, _ = moved64[name]
        sb = copy_state(new_batch(gpu, models, name), src)
    else:
        sb, tau0, _ = moved(gpu, models, name, torch.float32)
    seq = copy_state(new_batch(gpu, models, name, sb.dtype), sb)
    m = 5
    dtau = dtau_for(gpu, sb, m, seed=1)
    body_before, seed_before = sb.body.clone(), sb.seed.clone()
    out = sb.probe(dtau, tau0=tau0, body_out=True, n_contacts=True)
    tau = tau0[:, None, :] + dtau
    ref_body, ref_nc = sequential_probes(seq, tau)
    torch.cuda.synchronize()
    assert torch.equal(sb.body, body_before)
    assert torch.equal(out["tau_out"], tau)
    assert torch.equal(out["n_contacts"], ref_nc)
    assert torch.equal(sb.seed, seq.seed) and not torch.equal(sb.seed, seed_before)
    dev = (out["body_out"] - ref_body).abs().max().item()
    print(f"{name} {prec}: body_out against sequential trial steps: max deviation {dev:.3e}")
    assert torch.equal(out["body_out"], ref_body)
    assert torch.equal(out["config_out"], sb.config(body=out["body_out"]))
    # m = 1 is the first of the five
    keep = sb.seed.clone()
    sb.seed.copy_(seed_before)
    one = sb.probe(dtau[:, :1].contiguous(), tau0=tau0, body_out=True)
    assert torch.equal(one["body_out"][:, 0], out["body_out"][:, 0])
    assert torch.equal(one["config_out"][:, 0], out["config_out"][:, 0])
    sb.seed.copy_(keep)
    # probes of one rollout differ, and tau0 = None reads the batch's last torques
    assert not torch.equal(out["body_out"][:, 0], out["body_out"][:, 1])
    seq.last_tau = tau0
    a, b =sb.probe(dtau, tau0=tau0), seq.probe(dtau)
    assert torch.equal(a["config_out"], b["config_out"]) and torch.equal(sb.seed, seq.seed)


# ---- 9. probes against the oracle
@pytest.fixture(scope="module")
def probe_case(gpu, models, moved64, oracle_mod, omodels):
    """name -> the m = config_dim + 20 probes of the three states on the GPU and on the oracle"""
    import torch

    res = {}
    for name in CASES:
        src, tau0, _ = moved64[name]
        sb = copy_state(new_batch(gpu, models, name), src)
        m = sb.model.config_dim + 20
        dtau = dtau_for(gpu, sb, m, seed=2)
        out = sb.probe(dtau, tau0=tau0, body_out=True, n_contacts=True)
        torch.cuda.synchronize()
        tau = (tau0[:, None, :] + dtau).cpu().numpy()
        body, seed = src.body.cpu().numpy(), src.seed.cpu().numpy().astype(np.uint32)
        ref = [oracle_probes(oracle_mod, omodels[name], body[b], int(seed[b]), tau[b]) for b in range(B)]
        res[name] = dict(sb=sb, src=src, m=m, out={k: v.cpu().numpy() for k, v in out.items()}, ref=ref, tau=tau,
                         out_dev=out)
    return res


@pytest.mark.parametrize("name", sorted(CASES))
def test_probes_match_oracle(probe_case, oracle_mod, omodels, name):
    c = probe_case[name]
    o, seed = c["out"], c["sb"].seed.cpu().numpy().astype(np.uint32)
    for b in range(B):
        bodies, ncs, seeds = c["ref"][b]
        dev = np.abs(o["body_out"][b] - bodies).max()
        print(f"{name} rollout {b}: {c['m']} probes, contacts {ncs[0]}, body_out max deviation {dev:.3e}")
        assert dev < BODY_TOL
        assert np.array_equal(o["n_contacts"][b], ncs)
        assert int(seed[b]) == seeds[-1]
        for j in range(c["m"]):
            q, _ = oracle_mod.sim_hinges(omodels[name], bodies[j])
            assert np.abs(o["config_out"][b, j, 6:] - q).max() < Q_TOL, (b, j)


# ---- 10. the regression
@pytest.fixture(scope="module")
def regress_case(probe_case):
    """name -> T, U (NumPy U from the GPU's config_out and the batch's tracker)"""
    res = {}
    for name, c in probe_case.items():
        ders = c["src"].ders.cpu().numpy()
        res[name] = (c["sb"], c["out"]["tau_out"], np_probe_accel(ders, c["out"]["config_out"], c["sb"].params.dt))
    return res


def check_regression(sb, T, U, what):
    nmj = sb.model.nmj
    r = sb.regress_B(T, U)
    Bt, rank = r["Bt"].cpu().numpy(), r["rank"].cpu().numpy()
    for b in range(B):
        ref, A = lstsq_Bt(T[b], U[b])
        assert np.linalg.matrix_rank(A) == nmj + 1
        dev, scale = np.abs(Bt[b] - ref).max(), np.abs(ref).max()
        print(f"{what} rollout {b}: m = {T.shape[1]}, max |Bt - lstsq| = {dev:.3e}, max |Bt| = {scale:.3e}")
        assert dev <= 1e-9 * scale, (what, b)
    assert (rank == nmj + 1).all()
    return Bt


@pytest.mark.parametrize("name", sorted(CASES))
def test_regression_matches_lstsq(regress_case, name):
    sb, T, U = regress_case[name]
    check_regression(sb, T, U, name)
    n = sb.model.nmj + 1
    check_regression(sb, T[:, :n].copy(), U[:, :n].copy(), f"{name} square")


def test_regression_rank_deficient_and_unity(regress_case):
    sb, T, U = regress_case["hexapod"]
    nmj, cfg = sb.model.nmj, sb.model.config_dim
    k = 3
    T = T.copy()
    T[:, :, k] = 0.25  # c * the ones column with |c| < 1: the ones column is the larger and is picked first
    r = sb.regress_B(T, U)
    Bt, rank = r["Bt"].cpu().numpy(), r["rank"].cpu().numpy()
    assert (rank == nmj).all(), rank
    assert (Bt[:, k] == 0).all()
    others = [i for i in range(nmj) if i != k]
    for b in range(B):
        ref, _ = lstsq_Bt(T[b][:, others], U[b])
        dev = np.abs(Bt[b][others] - ref).max()
        print(f"rank-deficient rollout {b}: max deviation {dev:.3e} of {np.abs(ref).max():.3e}")
        assert dev <= 1e-9 * np.abs(ref).max()
    r = sb.regress_B(T[:, :0], U[:, :0])  # m = 0: set_Bt_unity
    unity = np.zeros((nmj, cfg))
    unity[np.arange(nmj), cfg - nmj + np.arange(nmj)] = 1
    assert np.array_equal(r["Bt"].cpu().numpy(), np.broadcast_to(unity, (B, nmj, cfg)))
    assert (r["rank"].cpu().numpy() == 0).all()
    seed = sb.seed.clone()
    e0 = sb.estimate_B(m=0)  # the same through the estimate: the tracker is pushed, nothing is probed
    assert np.array_equal(e0["Bt"].cpu().numpy(), np.broadcast_to(unity, (B, nmj, cfg)))
    assert tuple(e0["T"].shape) == (B, 0, nmj) and (sb.seed == seed).all()
    assert (sb.ders[:, 0] == sb.config()).all()


# ---- 11. end to end
@pytest.mark.parametrize("name", sorted(CASES))
def test_estimate_B_is_the_composition(gpu, models, moved64, oracle_mod, omodels, name):
    """hs_sim_estimate_B on the moving states against its parts, and against the CPU: oracle probes,
    hs_sim_config of their bodies, the NumPy tracker, lstsq. The bound follows from the project's own
    configuration bound: an error of 1e-9 in a configuration is 1e-9 / dt^2 in an acceleration, and
    the least-squares map amplifies a perturbation of U's columns (norm <= sqrt(m) per entry bound)
    by at most ||pinv([T | 1])||_2.
    Measured on MI355X: max |Bt - Bt_ref| 1.7e-11 for both models (the resting rollout; 7e-15 on the
    moving ones) against bounds of 8.9e-5 (hexapod) and 9.3e-5 (myant) or more."""
    import torch

    src, tau0, _ = moved64[name]
    a = copy_state(new_batch(gpu, models, name), src)
    b = copy_state(new_batch(gpu, models, name), src)
    m, dt = a.model.config_dim + 20, a.params.dt
    dtau = dtau_for(gpu, a, m, seed=4)
    est = a.estimate_B(dtau=dtau)  # tau0: the batch's last torques
    c0 = b.config()
    b.track_push(c0)
    pr = b.probe(dtau, tau0=tau0)
    U = np_probe_accel(b.ders.cpu().numpy(), pr["config_out"].cpu().numpy(), dt)
    rg = b.regress_B(pr["tau_out"], U)
    torch.cuda.synchronize()
    ders_ref = np_track_push(src.ders.cpu().numpy(), c0.cpu().numpy(), dt)
    assert np.array_equal(a.ders.cpu().numpy(), ders_ref) and torch.equal(a.ders, b.ders)
    assert torch.equal(est["T"], pr["tau_out"]) and torch.equal(est["T"], tau0[:, None, :] + dtau)
    assert np.array_equal(est["U"].cpu().numpy(), U)
    assert torch.equal(a.seed, b.seed) and torch.equal(a.body, src.body) and torch.equal(a.tsi, src.tsi)
    assert torch.equal(est["Bt"], rg["Bt"]) and torch.equal(est["rank"], rg["rank"])  # the same kernel
    assert (est["rank"] == a.model.nmj + 1).all()
    # against the CPU
    body, seed = src.body.cpu().numpy(), src.seed.cpu().numpy().astype(np.uint32)
    T = est["T"].cpu().numpy()
    Bt = est["Bt"].cpu().numpy()
    worst, worst_bound = 0.0, np.inf
    for r in range(B):
        bodies, _, _ = oracle_probes(oracle_mod, omodels[name], body[r], int(seed[r]), T[r])
        cfg_ref = a.config(body=torch.as_tensor(bodies, device=a.device)).cpu().numpy()
        U_ref = np_probe_accel(ders_ref[r:r + 1], cfg_ref[None], dt)[0]
        Bt_ref, A = lstsq_Bt(T[r], U_ref)
        bound = (1e-9 / dt ** 2) * np.linalg.norm(np.linalg.pinv(A), 2) * np.sqrt(m)
        dev = np.abs(Bt[r] - Bt_ref).max()
        print(f"{name} rollout {r}: max |Bt - Bt_ref| = {dev:.3e}, bound {bound:.3e}, max |Bt| {np.abs(Bt_ref).max():.3e}")
        assert dev <= bound, (name, r)
        worst, worst_bound = max(worst, dev), min(worst_bound, bound)
    print(f"{name}: worst {worst:.3e}, smallest bound {worst_bound:.3e}")


# ---- 12. a simulation loop
def test_estimate_then_step_loop(gpu, models):
    """10 x (estimate_B; step): the reference's simulate_ode with dynamics_from_simulation_flag. The
    estimate moves only the dRand stream and the tracker."""
    import torch

    sb = new_batch(gpu, models, "hexapod")       # the feature
    seq = new_batch(gpu, models, "hexapod")      # the reference-order loop from existing kernels
    plain = new_batch(gpu, models, "hexapod")    # step(1) alone, seeds set by hand
    m = sb.model.config_dim + 20
    nmj, cfg = sb.model.nmj, sb.model.config_dim
    tau0 = torch.zeros((B, nmj), dtype=torch.float64, device=sb.device)
    for it in range(10):
        dtau = dtau_for(gpu, sb, m, seed=100 + it)
        est = sb.estimate_B(dtau=dtau)
        assert torch.equal(est["T"], tau0[:, None, :] + dtau), it
        sequential_probes(seq, tau0[:, None, :] + dtau)
        assert torch.equal(sb.seed, seq.seed), it
        plain.seed.copy_(sb.seed)
        o = sb.step(1, outputs=("tau_cmd",))
        tau0 = o["tau_cmd"][:, -1].clone()
        seq.step(1)
        plain.step(1)
        assert torch.equal(sb.seed, seq.seed) and torch.equal(sb.seed, plain.seed), it
        assert torch.equal(sb.body, plain.body) and torch.equal(sb.body, seq.body), it
        rec = sb.traj_record()
        assert tuple(rec.shape) == (B, 2 * cfg + nmj)
        assert torch.equal(rec, torch.cat([sb.ders[:, 0], sb.ders[:, 1], tau0], 1)), it
    torch.cuda.synchronize()
    assert (sb.tsi == TSI0 + 10).all()
    assert (est["rank"] == nmj + 1).all()
    assert sb.ders[:, 2].abs().max() > 0
