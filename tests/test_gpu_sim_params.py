"""GPU parity of the simulation kernel (hs_sim_kernel.h: hs_sim_step, and the TRIAL and PROBE instantiations
hs_sim_trial and hs_sim_probe) with the oracle under every parameter set of tests/test_sim_params.py:
each field of hs_sim_params away from its default, on the scenarios of that file (stand, land, sunk).

Both sides read the GPU's controller tables and start from bitwise the same state: the scenario is
written into the batch's body array and read back. Bounds are those of tests/test_gpu_sim.py, unchanged:
contact counts, tsi and the dRand seed equal, body and torso 1e-10, tau_cmd 1e-9 relative to
max(1, |tau|), q_meas 1e-9, normal force 1e-8 relative; tests/test_sim_params.py measures what a
rounding-sized perturbation does over the same steps (1.1e-13 at most).

What these tests found: sor_pair bounded a contact's normal row above by mu (the friction rows' bound;
the oracle and ODE leave the normal row in [0, inf)). With the default mu = inf nothing showed; under
mu = 0.5 the hexapod's contact counts left the oracle's at the third step. Fixed there.

Measured on MI355X (library 1edc3706), maxima over the rollouts of each case; no run was shortened:
  a. 12 steps, B = 4 (2 stand, 2 land), hexapod / myant, spider for mu=0.5, iterations=9, mixed:
       body 1.0e-13 (dt=0.005, hexapod; every other set 4.5e-14 .. 8.4e-14; iterations=0 1.9e-15),
       tau_cmd 7.7e-13 relative (dt=0.005, myant), q_meas 1.8e-15, torso 4.4e-16,
       normal_force 1.6e-12 relative (gravity=0, myant); contact counts 0 .. 6 seen; seeds equal.
     sunk, 3 steps (22 / 17 / 18 contacts): body 4.0e-14, normal_force 2.1e-16 relative.
  c. kicks under gravity = 0: tau_cmd 1.2e-12, q_meas 8.9e-16, torso 1.1e-16, body 5.8e-14.
  d. probes: body_out 4.4e-16 (0 with iterations=0), contact counts and seeds equal.
  e. fp32: d_same 1.1e-7 (iterations=0) .. 6.6e-5 (iterations=1, myant) against d_other 1.2e-2 .. 1.4;
     the smallest d_other / d_same asked for is 1.1e3 (iterations=33, myant). Not asked (d_other <= 1e-2):
     cfm=1e-5 on both models, iterations=33 on the hexapod.
"""
import os

import numpy as np
import pytest

from conftest import MODELS
from sim_gpu_kit import BODY_TOL, NEVER, gpu, hmodels, host, tables  # noqa: F401
from test_sim_dynamics import oracle_probes
from test_sim_params import (F32_D_OTHER, F32_ROLLOUTS, KICK_DV, KICK_EVERY, KICK_PHASE, PARAM_SETS,
                             STAND_ONLY, STEPS, SUNK_SETS, TSI0, oracle_kicked, scenario, scenario_of, set_n_t,
                             torso_distance)

pytestmark = pytest.mark.gpu

B_STEP = 4
SPIDER_SETS = ("mu=0.5", "iterations=9", "mixed")
STEP_CASES = [(p, m) for p in PARAM_SETS for m in ("hexapod", "myant")] + [(p, "spider") for p in SPIDER_SETS]
SUNK_CASES = [(p, m) for p in SUNK_SETS for m in ("hexapod", "myant")] + [("mu=0.5", "spider"), ("mixed", "spider")]


def set_batch(gpu, hmodels, name, B, pname, **kw):
    """B rollouts of synth.gen_sim_params under PARAM_SETS[pname] (None: the defaults)"""
    from hslabs_amd import synth

    sb = gpu.SimBatch(hmodels[name], synth.gen_sim_params(B, name), **dict(PARAM_SETS[pname] if pname else {}, **kw))
    assert sb.n_t == (set_n_t(pname) if pname else 300) and sb.table_row(TSI0) == 0
    return sb


def half_and_half(pname, B):
    """the first half of a batch stands, the second lands (a set that is stand only: all of it)"""
    return ["stand"] * B if pname in STAND_ONLY else ["stand"] * (B // 2) + ["land"] * (B - B // 2)


def start(sb, whiches):
    """write scenario whiches[b] into rollout b and read the state back: the bits both sides start from
    (as float64, whatever the batch's precision)"""
    import torch

    body = sb.body.cpu().numpy()
    for b, which in enumerate(whiches):
        body[b] = scenario(body[b], which)
    sb.body.copy_(torch.as_tensor(body, device=sb.device))
    torch.cuda.synchronize()
    return sb.body.cpu().numpy().astype(np.float64)


def oracle_params(O, pname, **kw):
    return O.SimParams(**dict(PARAM_SETS[pname] if pname else {}, **kw))


def compare_steps(O, om, P, sb, o, body0, steps, body_bound):
    """the assertions of tests/test_gpu_sim.py::test_steps_match_oracle on every rollout of sb after `steps`
    steps from body0; body_bound(r) gives the bound of the final body state. Returns the maximum deviations
    and the contact counts seen."""
    qt, dqt, tt = tables(sb)
    body, seed, tsi = sb.body.cpu().numpy(), sb.seed.cpu().numpy().astype(np.uint32), sb.tsi.cpu().numpy()
    dev = dict(body=0.0, tau_cmd=0.0, q_meas=0.0, torso=0.0, normal_force=0.0)
    seen = set()
    for b in range(sb.B):
        r = O.sim_run(om, P, sb.n_t, qt[b], dqt[b], tt[b], body0[b], 0, TSI0, steps)
        d = {k: float(np.abs(r[k] - (body[b] if k == "body" else o[k][b])).max()) for k in dev}
        d["normal_force"] /= max(1, r["normal_force"].max())
        d["tau_cmd"] /= max(1, np.abs(r["tau_cmd"]).max())
        for k in dev:
            dev[k] = max(dev[k], d[k])
        seen |= set(r["n_contacts"].tolist())
        assert (r["n_contacts"] == o["n_contacts"][b]).all(), (b, r["n_contacts"], o["n_contacts"][b])
        assert d["body"] < body_bound(r), (b, d)
        assert d["tau_cmd"] < 1e-9, (b, d)
        assert d["q_meas"] < 1e-9, (b, d)
        assert d["torso"] < BODY_TOL, (b, d)
        assert d["normal_force"] < 1e-8, (b, d)
        assert int(tsi[b]) == r["tsi"] == TSI0 + steps
        assert int(seed[b]) == r["seed"], (b, int(seed[b]), r["seed"])
    return dev, seen


def show(what, dev, seen):
    print(f"{what}: max deviation body {dev['body']:.2e} tau_cmd {dev['tau_cmd']:.2e} (rel) q_meas "
          f"{dev['q_meas']:.2e} torso {dev['torso']:.2e} normal_force {dev['normal_force']:.2e} (rel); "
          f"contact counts {sorted(seen)}")


# ---- a. hs_sim_step against the oracle, per set
@pytest.mark.parametrize("pname,name", STEP_CASES)
def test_steps_match_oracle(gpu, hmodels, oracle_mod, omodels, pname, name):
    import torch

    sb = set_batch(gpu, hmodels, name, B_STEP, pname)
    body0 = start(sb, half_and_half(pname, B_STEP))
    o = host(sb.step(STEPS))
    torch.cuda.synchronize()
    dev, seen = compare_steps(oracle_mod, omodels[name], oracle_params(oracle_mod, pname), sb, o, body0, STEPS,
                              lambda r: BODY_TOL)
    show(f"{name} {pname}, {STEPS} steps", dev, seen)
    if PARAM_SETS[pname].get("iterations") == 0:
        assert (sb.seed == 0).all()  # no sweep, no draw


def collision_parts(name):
    import xml.etree.ElementTree as ET

    bodies = ET.parse(os.path.join(MODELS, f"{name}.xml")).getroot().iter("body")
    return sum(1 for bd in bodies if bd.find("geom") is not None and bd.find("geom").get("type") in ("capsule", "sphere"))


@pytest.mark.parametrize("pname,name", SUNK_CASES)
def test_sunk_matches_oracle(gpu, hmodels, oracle_mod, omodels, pname, name):
    """the maximum row count under finite friction: every contact's two friction rows clamp"""
    import torch

    sb = set_batch(gpu, hmodels, name, 2, pname)
    body0 = start(sb, ["sunk"] * 2)
    o = host(sb.step(3))
    torch.cuda.synchronize()
    assert o["n_contacts"][:, 0].max() == collision_parts(name)
    dev, seen = compare_steps(oracle_mod, omodels[name], oracle_params(oracle_mod, pname), sb, o, body0, 3,
                              lambda r: 1e-9 * max(1.0, np.abs(r["body"]).max()))
    show(f"{name} {pname}, sunk, 3 steps", dev, seen)


# ---- b. launch split
@pytest.mark.parametrize("pname", ["mixed", "iterations=7"])
def test_launch_split_is_bitwise(gpu, hmodels, pname):
    import torch

    a, b = (set_batch(gpu, hmodels, "hexapod", B_STEP, pname) for _ in range(2))
    ba, bb = start(a, half_and_half(pname, B_STEP)), start(b, half_and_half(pname, B_STEP))
    assert np.array_equal(ba, bb)
    oa = a.step(STEPS)
    parts = [b.step(STEPS // 3) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(a.body, b.body) and torch.equal(a.seed, b.seed) and torch.equal(a.tsi, b.tsi)
    assert torch.equal(oa["tau_cmd"], torch.cat([p["tau_cmd"] for p in parts], dim=1))
    assert (a.tsi == TSI0 + STEPS).all() and (a.seed != 0).all()


# ---- c. the TRIAL instantiation
@pytest.mark.parametrize("name", ["hexapod", "myant"])
@pytest.mark.parametrize("pname", ["mixed", "mu=0.05"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_trial_with_extras_off_is_sim_step(gpu, hmodels, name, pname, prec):
    import torch

    dtype = torch.float64 if prec == "f64" else torch.float32
    a, b = (set_batch(gpu, hmodels, name, B_STEP, pname, dtype=dtype) for _ in range(2))
    ba, bb = start(a, half_and_half(pname, B_STEP)), start(b, half_and_half(pname, B_STEP))
    assert np.array_equal(ba, bb)
    oa = a.step(STEPS)
    ob = b.trial(STEPS, check_from=NEVER)
    torch.cuda.synchronize()
    assert torch.equal(a.body, b.body) and torch.equal(a.seed, b.seed) and torch.equal(a.tsi, b.tsi)
    for k, v in oa.items():
        assert torch.equal(v, ob[k]), k
    assert (b.state == gpu.capi.HS_TRIAL_RUNNING).all()
    assert torch.isfinite(a.body).all() and (oa["n_contacts"] > 0).any()


def test_kicks_without_gravity_match_oracle(gpu, hmodels, oracle_mod, omodels):
    """the kick's force in v/h + M^-1 f and in the velocity update with no gravity term on top of it, against
    the kick emulation of tests/test_sim_trial.py (dv added to the root body's lvel before the kicked step;
    one rounding apart), at the bounds of tests/test_gpu_sim_trial.py"""
    import torch

    pname, name = "gravity=0", "hexapod"
    B = len(KICK_DV)
    sb = set_batch(gpu, hmodels, name, B, pname)
    body0 = start(sb, half_and_half(pname, B))
    dv = np.array(KICK_DV)
    o = host(sb.trial(STEPS, kick_dv=dv, kick_every=KICK_EVERY, kick_phase=KICK_PHASE, check_from=NEVER))
    torch.cuda.synchronize()
    qt, dqt, tt = tables(sb)
    body, seed = sb.body.cpu().numpy(), sb.seed.cpu().numpy().astype(np.uint32)
    P = oracle_params(oracle_mod, pname)
    for b in range(B):
        r = oracle_kicked(oracle_mod, omodels[name], P, sb.n_t, qt[b], dqt[b], tt[b], body0[b], STEPS, dv[b])
        d = {k: np.abs(r[k] - o[k][b]).max() for k in ("tau_cmd", "q_meas", "torso")}
        db = np.abs(r["body"] - body[b]).max()
        print(f"kick {KICK_DV[b]}: max deviation tau_cmd {d['tau_cmd']:.2e} q_meas {d['q_meas']:.2e} torso "
              f"{d['torso']:.2e} body {db:.2e}; contact counts {sorted(set(r['n_contacts'].tolist()))}")
        assert d["tau_cmd"] < 1e-9 * max(1, np.abs(r["tau_cmd"]).max()), b
        assert d["q_meas"] < 1e-9, b
        assert d["torso"] < BODY_TOL, b
        assert db < BODY_TOL, b
        assert (r["n_contacts"] == o["n_contacts"][b]).all() and int(seed[b]) == r["seed"], b
    assert (o["state"] == gpu.capi.HS_TRIAL_RUNNING).all()


# ---- d. the PROBE instantiation
@pytest.mark.parametrize("name", ["hexapod", "myant"])
@pytest.mark.parametrize("pname", ["iterations=0", "iterations=7", "iterations=9", "iterations=33", "mu=0.5"])
def test_probes_match_oracle(gpu, hmodels, oracle_mod, omodels, pname, name):
    """m = 5 probes from a state six position-control steps in (the landing rollouts have touched down), from
    seeds of the test's own: the only check of the probe's dRand jump-ahead at a reshuffle count other than
    the defaults' 3"""
    import torch
    from hslabs_amd import synth

    m = 5
    sb = set_batch(gpu, hmodels, name, B_STEP, pname)
    start(sb, half_and_half(pname, B_STEP))
    tau0 = sb.step(6, outputs=("tau_cmd",))["tau_cmd"][:, -1].clone()
    seed0 = np.array([1, 0x9E3779B9, 123456789, 0xFFFFFFFF][:B_STEP], dtype=np.uint32)
    sb.seed.copy_(torch.as_tensor(seed0.view(np.int32), device=sb.device))
    body0 = sb.body.cpu().numpy()
    dtau = torch.as_tensor(synth.gen_torque_perturbations(B_STEP, m, sb.model.nmj, seed=1), device=sb.device)
    out = host(sb.probe(dtau, tau0=tau0, body_out=True, n_contacts=True))
    torch.cuda.synchronize()
    assert np.array_equal(sb.body.cpu().numpy(), body0)  # a probe does not advance the state
    tau = (tau0[:, None, :] + dtau).cpu().numpy()
    assert np.array_equal(out["tau_out"], tau)
    seed = sb.seed.cpu().numpy().view(np.uint32)
    P = oracle_params(oracle_mod, pname, k=1e-300)
    worst, seen = 0.0, set()
    for b in range(B_STEP):
        bodies, ncs, seeds = oracle_probes(oracle_mod, omodels[name], body0[b], int(seed0[b]), tau[b], params=P)
        worst = max(worst, float(np.abs(out["body_out"][b] - bodies).max()))
        seen |= set(ncs.tolist())
        assert np.abs(out["body_out"][b] - bodies).max() < BODY_TOL, b
        assert np.array_equal(out["n_contacts"][b], ncs), b
        assert int(seed[b]) == seeds[-1], (b, int(seed[b]), seeds)
        assert (seeds[-1] == int(seed0[b])) == (P.iterations == 0)
    print(f"{name} {pname}: {m} probes, body_out max deviation {worst:.2e}; contact counts {sorted(seen)}")


# ---- e. fp32, discriminating only
@pytest.fixture(scope="module")
def f32_defaults(gpu, hmodels, oracle_mod, omodels):
    """model -> the oracle's final bodies under the defaults, on land, from a default fp32 batch's tables and
    state (computed once, read only)"""
    import torch

    res = {}
    for name in ("hexapod", "myant"):
        sb = set_batch(gpu, hmodels, name, F32_ROLLOUTS, None, dtype=torch.float32)
        body0 = start(sb, ["land"] * F32_ROLLOUTS)
        qt, dqt, tt = tables(sb)
        P = oracle_mod.SimParams()
        res[name] = np.array([oracle_mod.sim_run(omodels[name], P, sb.n_t, qt[b], dqt[b], tt[b], body0[b], 0, TSI0,
                                                 STEPS)["body"] for b in range(F32_ROLLOUTS)])
    return res


@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_f32_follows_its_own_parameters(gpu, hmodels, oracle_mod, omodels, f32_defaults, pname):
    """Floats cannot follow the double trajectory bit for bit, so this asks that the fp32 kernel sits clearly
    nearer the oracle's answer under its own parameters (d_same: final torso state, the largest deviation of
    8 rollouts on land) than the defaults' answer lies from it (d_other): d_same < d_other / 4 wherever
    d_other > 1e-2 (tests/test_sim_params.py names the sets; at least 12). A condition, not a tolerance."""
    import torch

    for name in ("hexapod", "myant"):
        sb = set_batch(gpu, hmodels, name, F32_ROLLOUTS, pname, dtype=torch.float32)
        assert sb.body.dtype == torch.float32
        body0 = start(sb, ["land"] * F32_ROLLOUTS)
        sb.step(STEPS, outputs=())
        torch.cuda.synchronize()
        assert torch.isfinite(sb.body).all(), name
        qt, dqt, tt = tables(sb)
        P = oracle_params(oracle_mod, pname)
        ref = np.array([oracle_mod.sim_run(omodels[name], P, sb.n_t, qt[b], dqt[b], tt[b], body0[b], 0, TSI0,
                                           STEPS)["body"] for b in range(F32_ROLLOUTS)])
        d_same = torso_distance(sb.body.cpu().numpy(), ref)
        d_other = torso_distance(ref, f32_defaults[name])
        asked = d_other > F32_D_OTHER
        print(f"{name} {pname} fp32: d_same {d_same:.3e}, d_other {d_other:.3e}"
              f"{'' if asked else '  (not asked: d_other <= 1e-2)'}")
        if asked:
            assert d_same < d_other / 4, (name, d_same, d_other)
        assert (sb.tsi == TSI0 + STEPS).all()


# ---- f. the 3-waves/SIMD fp32 build
def test_f32_occupancy_builds_agree_under_mixed(gpu, hmodels):
    """tests/test_gpu_sim.py::test_f32_occupancy_builds_agree under `mixed`, landing: a 16384-spider fp32
    batch runs the 3-waves/SIMD build, a small one the default build; the same rollouts come out bit for bit"""
    import torch
    from hslabs_amd import synth

    params = synth.gen_sim_params(16384, "spider")
    big = gpu.SimBatch(hmodels["spider"], params, dtype=torch.float32, **PARAM_SETS["mixed"])
    big.body.copy_(scenario(big.body, "land"))
    big.step(8, outputs=())
    idx = [0, 5000, 16383]
    small = gpu.SimBatch(hmodels["spider"], params[idx], dtype=torch.float32, **PARAM_SETS["mixed"])
    small.body.copy_(scenario(small.body, "land"))
    o = small.step(8, outputs=("n_contacts",))
    torch.cuda.synchronize()
    assert torch.isfinite(small.body).all() and (o["n_contacts"] > 0).any()
    for k, i in enumerate(idx):
        assert torch.equal(small.body[k], big.body[i])
        assert small.seed[k].item() == big.seed[i].item()
