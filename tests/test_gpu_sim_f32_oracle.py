"""The fp32 simulation kernels (hs_sim_kernel<..., float, 1|3, TRIAL, PROBE> through hs_sim_step, hs_sim_trial
and hs_sim_probe with HS_PREC_F32) against the oracle, one step at a time, bounded by the oracle's own
single-precision build (oracle/hs_oracle_f32.cpp; tests/test_sim_oracle_f32.py makes it trustworthy and
holds the helpers).

Shape. The teacher is the fp64 oracle's free run over one gait period (300 steps, pgs 8 / 9 / 24, n_t = 300)
from the GPU's float reset state with the GPU's float tables. Rollout k of a float SimBatch of B = 300 is set
to teacher state k (body rounded to float, that step's seed, tsi = 2 + k), and ONE one-step launch takes all
300 single steps. Both builds of the oracle take the same steps on the CPU from the same bits.

Bound (sim_gpu_kit.hold_to_oracles). A step is decided when every part has |d| > 1e-5 at its start (d: the
fp64 oracle's contact depths). For each quantity, spread = the largest |f32 oracle - f64 oracle| over the
decided steps, relative to max(1, |f64 value|), computed in the test from the same states; on decided steps
|kernel - f64 oracle| <= 4 x spread: the kernel keeps the oracle's operation order except for FMAs in the
SOR sweeps and the device atan2, so its error is another draw of the same rounding process. n_contacts and
the seed are the fp64 oracle's on decided steps; on undecided ones n_contacts may differ by at most the
number of parts with |d| <= 1e-5, and the quantities are compared where it agrees. At most 10 % of a model's
steps may be undecided (asserted).

The open-loop k of the single-precision oracle is K_OPEN_F32 (1e-300 is 0 in float, which switches the
oracle's torques off); the open-loop test asserts that all three sides apply the table row bit for bit.

Measured on MI355X (profiles/sim_f32_oracle.txt holds every printed line), kernel vs f64 oracle as a multiple
of the spread, the largest over the decided states; undecided states 20 / 3 / 21 of 300 (hexapod / myant / spider):
  1. step      hexapod  body 0.45 tau_cmd 0.66 q_meas 0.64 torso 0.77 normal_force 1.05  (spread 4.4e-5 6.7e-5 6.7e-7 8.1e-8 3.8e-4)
               myant         0.39         0.51        0.44       0.76              1.16  (spread 4.6e-5 8.5e-5 9.3e-7 9.5e-8 1.3e-3)
               spider        0.76         0.85        0.74       0.93              3.41  (spread 2.4e-5 6.2e-5 4.8e-7 6.4e-8 3.6e-4)
               myant's state 0 (the reset state, 2 parts with |d| <= 1e-5) is taken with another contact count.
  2. sets      mixed 1.04, iterations=7 1.07, iterations=33 1.04 (normal_force, the largest; body 0.56 .. 0.69)
  3. 3 waves   bit for bit
  4. trial     open loop: tau_cmd equal, normal_force 1.06, torso 0.90; torque limit 4.1654 (clips 455 torques in 186
               states): normal_force 1.07; kick: torso 0.77 over all, 0.77 over the kicked rollouts; fall check: as the oracle
  5. probes    body_out hexapod 0.38, myant 0.23; contact counts and seeds equal wherever the count is decided
The factor 4 is not used up anywhere; the normal force is the quantity nearest to it, on shallow contacts, where
d's rounding is a per cent of d: the spider's 3.41 is one step (150: two contacts 4.5e-5 and 5.7e-5 deep carrying
2.46, kernel 2.4590, f64 2.4560, f32 oracle 2.4551; every other spider step stays under 0.7 x), myant's largest
(step 297) one contact 2.3e-5 deep, and the two oracle builds differ most on the same steps.
"""
import os

import numpy as np
import pytest

from conftest import PGS_CONFIG
from sim_gpu_kit import NEVER, gpu, hmodels, hold_to_oracles, one_step_results, set_states, tables0  # noqa: F401
from test_sim_dynamics import oracle_probes
from test_sim_oracle_f32 import (F32_CASES, K_OPEN_F32, MARGIN, N_T, QUANTITIES, STEPS, TSI0, contact_depths, f32,
                                 near_zero, omodels32, single_steps, teacher_states)  # noqa: F401
from test_sim_params import PARAM_SETS
from test_sim_trial import RUNNING, oracle_trial

pytestmark = pytest.mark.gpu

B_BIG = 16384                  # a spider batch the launcher gives the 3-waves/SIMD build
STEP_SETS = ("mixed", "iterations=7", "iterations=33")
PROBE_STATES = (0, 13, 25)     # tests/test_sim_dynamics.py MOVE_STEPS
PROBE_M = 5
LIMIT_CLEAR = 1e-4             # no |tau| within this (relative) of the torque limit
HC_CLEAR = 1e-4                # the fall check is compared on states at least this far from hc
KICK_EVERY, KICK_PHASE = 7, 3
STEP_Q = QUANTITIES
TRIAL_Q = QUANTITIES


def float_batch(gpu, hmodels, name, B, **kw):
    import torch

    p = gpu.read_pgs_config(PGS_CONFIG, F32_CASES[name])
    sb = gpu.SimBatch(hmodels[name], [p] * B, tsi0=TSI0, dtype=torch.float32, **kw)
    assert sb.n_t == N_T and sb.table_row(TSI0) == 0
    return sb


@pytest.fixture(scope="module")
def teachers(gpu, hmodels, oracle_mod, omodels):
    """name -> (tables, teacher states, near); computed on first use, read only"""
    cache = {}

    def get(name):
        if name not in cache:
            O = oracle_mod
            sb = float_batch(gpu, hmodels, name, 2)
            tabs = tables0(sb)
            assert all(np.array_equal(t[0].cpu().numpy(), t[1].cpu().numpy()) for t in
                       (sb.tables.q, sb.tables.dq, sb.tables.tau))
            body0 = sb.body[0].cpu().numpy().astype(np.float64)
            states = teacher_states(O, omodels[name], O.SimParams(), tabs, body0, STEPS)
            cache[name] = (tabs, states, near_zero(contact_depths(O, omodels[name], states[0])))
        return cache[name]

    return get


@pytest.fixture(scope="module")
def step_runs(gpu, hmodels, oracle_mod, omodels, omodels32, teachers):
    """(name, parameter set or None) -> the one-step launch of hs_sim_step over the 300 teacher states and both
    oracle builds' steps from them; computed on first use, read only"""
    import torch

    cache = {}

    def get(name, pname=None):
        if (name, pname) not in cache:
            O = oracle_mod
            tabs, states, near = teachers(name)
            over = PARAM_SETS[pname] if pname else {}
            sb = float_batch(gpu, hmodels, name, STEPS, **over)
            assert all(np.array_equal(a, b) for a, b in zip(tabs, tables0(sb)))
            set_states(sb, states)
            o = sb.step(1)
            torch.cuda.synchronize()
            kern = one_step_results(sb, o)
            assert (kern["tsi"] == states[2] + 1).all()
            P = O.SimParams(**over)
            cache[(name, pname)] = dict(kern=kern, near=near,
                                        r64=single_steps(O, omodels[name], P, tabs, states),
                                        r32=single_steps(O, omodels32[name], P, tabs, states))
        return cache[(name, pname)]

    return get


# ---- 1. hs_sim_step, the defaults
@pytest.mark.parametrize("name", sorted(F32_CASES))
def test_step_is_held_to_the_oracles(step_runs, name):
    r = step_runs(name)
    hold_to_oracles(f"{name} step", r["kern"], r["r64"], r["r32"], r["near"], STEP_Q)
    assert r["r64"]["n_contacts"].min() < r["r64"]["n_contacts"].max()


# ---- 2. hs_sim_step under other parameters: the per-step bound where test_gpu_sim_params.py section e only discriminates
@pytest.mark.parametrize("pname", STEP_SETS)
def test_step_under_parameter_sets(step_runs, pname):
    r = step_runs("hexapod", pname)
    hold_to_oracles(f"hexapod {pname} step", r["kern"], r["r64"], r["r32"], r["near"], STEP_Q)
    d = step_runs("hexapod")["r64"]
    assert not np.array_equal(d["body"], r["r64"]["body"])  # the set is felt
    if "iterations" in PARAM_SETS[pname]:
        assert not np.array_equal(d["seed"], r["r64"]["seed"])  # another number of reshuffles


# ---- 3. the 3-waves/SIMD build
def test_three_waves_build_is_bitwise_the_default_build(gpu, hmodels, teachers, step_runs):
    """the 300 teacher states as the first rollouts of a 16384-spider batch (the rest: copies of state 0), which
    the launcher gives the 3-waves/SIMD build: they come out bit for bit as from the default build in test 1"""
    import torch

    _, states, _ = teachers("spider")
    ref = step_runs("spider")["kern"]
    sb = float_batch(gpu, hmodels, "spider", B_BIG)
    set_states(sb, states)
    o = sb.step(1)
    torch.cuda.synchronize()
    big = one_step_results(sb, o, STEPS)
    for k in STEP_Q + ("n_contacts", "seed", "tsi"):
        assert np.array_equal(big[k], ref[k]), k
    assert torch.equal(sb.body[STEPS:], sb.body[STEPS:STEPS + 1].expand(B_BIG - STEPS, -1, -1))
    assert torch.equal(sb.body[STEPS], sb.body[0])


# ---- 4. hs_sim_trial
def trial_steps(O, om, tabs, states, single, **kw):
    """one oracle_trial step of the build that owns om from every teacher state; kw may hold per-state lists"""
    qt, dqt, tt = tabs
    out = {k: [] for k in QUANTITIES + ("n_contacts", "seed", "state")}
    extra = dict(k_open=K_OPEN_F32, real=np.float32) if single else {}
    for i, (b, s, t) in enumerate(zip(*states[:3])):
        args = {k: (v[i] if isinstance(v, (list, np.ndarray)) else v) for k, v in kw.items()}
        r = oracle_trial(O, om, N_T, qt, dqt, tt, b, int(t), 1, seed0=int(s), **extra, **args)
        for k in ("tau_cmd", "q_meas", "torso", "normal_force", "n_contacts"):
            out[k].append(r[k][0] if len(r[k]) else np.full(r[k].shape[1:], np.nan))
        out["body"].append(r["body"])
        out["seed"].append(r["seed"])
        out["state"].append(r["state"])
    res = {k: np.array(v) for k, v in out.items()}
    res["seed"] = res["seed"].astype(np.uint32)
    return res


def trial_launch(gpu, hmodels, states, **kw):
    import torch

    sb = float_batch(gpu, hmodels, "hexapod", STEPS)
    set_states(sb, states)
    o = sb.trial(1, **kw)
    torch.cuda.synchronize()
    return sb, o


def test_trial_open_loop(gpu, hmodels, oracle_mod, omodels, omodels32, teachers):
    """open loop: every rollout applies its own table row (tsi = 2 + k: 300 different rows)"""
    O = oracle_mod
    tabs, states, near = teachers("hexapod")
    sb, o = trial_launch(gpu, hmodels, states, open_loop=True, check_from=NEVER)
    kern = one_step_results(sb, o)
    r64 = trial_steps(O, omodels["hexapod"], tabs, states, False, open_loop=True, check_from=NEVER)
    r32 = trial_steps(O, omodels32["hexapod"], tabs, states, True, open_loop=True, check_from=NEVER)
    rows = (states[2] % N_T + N_T - 2) % N_T
    for r in (kern, r64, r32):  # the torque is the table row, bit for bit: K_OPEN_F32 has not switched it off
        assert np.array_equal(r["tau_cmd"], tabs[2][rows])
    assert (o["state"].cpu().numpy() == RUNNING).all()
    hold_to_oracles("hexapod trial open loop", kern, r64, r32, near, TRIAL_Q)


def clear_limit(tau):
    """a torque limit from the teacher's |tau_cmd| [K][nmj]: the middle of the widest relative gap between
    neighbouring values in the upper half of the largest torques per state, so that it clips at most states"""
    peak = np.sort(np.abs(tau).max(axis=1))
    cand = np.sort(np.abs(tau).ravel())
    cand = cand[(cand >= peak[len(peak) // 4]) & (cand <= peak[len(peak) // 2])]
    gap = cand[1:] / cand[:-1]
    i = int(np.argmax(gap))
    return float(np.sqrt(cand[i] * cand[i + 1]))


def test_trial_torque_limit(gpu, hmodels, oracle_mod, omodels, omodels32, teachers, step_runs):
    """one step under a torque limit that clips: chosen from the fp64 oracle's PD torques at the teacher states,
    clear of every one of them by LIMIT_CLEAR, so that all three sides clip the same joints"""
    O = oracle_mod
    tabs, states, near = teachers("hexapod")
    free = step_runs("hexapod")
    lim = clear_limit(free["r64"]["tau_cmd"])
    for r in (free["r64"], free["r32"], free["kern"]):
        rel = np.abs(np.abs(r["tau_cmd"]) / lim - 1)
        assert rel.min() > LIMIT_CLEAR, (lim, rel.min())
    clipped = np.abs(free["r64"]["tau_cmd"]) > lim
    assert clipped.any(axis=1).mean() >= 0.5 and not clipped.all(axis=1).any()
    print(f"torque limit {lim!r}: clips {int(clipped.sum())} torques of {clipped.size} in "
          f"{int(clipped.any(axis=1).sum())} of {len(clipped)} states")
    sb, o = trial_launch(gpu, hmodels, states, torque_limit=lim, check_from=NEVER)
    kern = one_step_results(sb, o)
    r64 = trial_steps(O, omodels["hexapod"], tabs, states, False, limit=lim, check_from=NEVER)
    r32 = trial_steps(O, omodels32["hexapod"], tabs, states, True, limit=lim, check_from=NEVER)
    for r in (kern, r64, r32):
        assert np.array_equal(np.abs(r["tau_cmd"]) > lim * (1 - LIMIT_CLEAR / 2), clipped)  # the same joints clip
        assert np.abs(r["tau_cmd"]).max() <= lim * (1 + 1e-6)
    assert not np.array_equal(kern["body"], free["kern"]["body"])
    hold_to_oracles("hexapod trial torque limit", kern, r64, r32, near, TRIAL_Q)


def test_trial_kick(gpu, hmodels, oracle_mod, omodels, omodels32, teachers, step_runs):
    """the step at which a kick acts: the rollouts with tsi % KICK_EVERY == KICK_PHASE are kicked, each by its own
    dv, the others take the plain step"""
    O = oracle_mod
    tabs, states, near = teachers("hexapod")
    rng = np.random.default_rng(11)
    dv = f32(rng.uniform(-1.0, 1.0, (STEPS, 3)))
    kicked = states[2] % KICK_EVERY == KICK_PHASE
    assert 30 < kicked.sum() < 60 and (near[kicked] == 0).sum() > 30
    sb, o = trial_launch(gpu, hmodels, states, kick_dv=dv, kick_every=KICK_EVERY, kick_phase=KICK_PHASE,
                         check_from=NEVER)
    kern = one_step_results(sb, o)
    kw = dict(dv=list(dv), kick_every=KICK_EVERY, kick_phase=KICK_PHASE, check_from=NEVER)
    r64 = trial_steps(O, omodels["hexapod"], tabs, states, False, **kw)
    r32 = trial_steps(O, omodels32["hexapod"], tabs, states, True, **kw)
    free = step_runs("hexapod")
    same = np.array([np.array_equal(a, b) for a, b in zip(kern["body"], free["kern"]["body"])])
    assert np.array_equal(same, ~kicked)  # a kick moves the step, and only where it acts
    assert np.array_equal(r64["body"][~kicked], free["r64"]["body"][~kicked])
    hold_to_oracles("hexapod trial kick", kern, r64, r32, near, TRIAL_Q)
    sel = {k: v[kicked] for k, v in kern.items()}
    hold_to_oracles("hexapod trial kick, the kicked rollouts", sel, {k: v[kicked] for k, v in r64.items()},
                    {k: v[kicked] for k, v in r32.items()}, near[kicked], TRIAL_Q, cap=False)


def test_trial_fall_check(gpu, hmodels, oracle_mod, omodels, teachers, step_runs):
    """the fall check at hc = the median torso height of the teacher states: a state at least HC_CLEAR away from
    hc freezes or steps as on the oracle; a frozen rollout keeps its state, a stepping one takes test 1's step"""
    O = oracle_mod
    tabs, states, near = teachers("hexapod")
    z = states[0][:, 0, 2]
    hc = float(np.float32(np.median(z)))
    clear = np.abs(z - hc) >= HC_CLEAR
    assert clear.mean() > 0.9 and 30 < (z[clear] < hc).sum() < STEPS - 30
    sb, o = trial_launch(gpu, hmodels, states, hc=hc, check_from=0)
    kern = one_step_results(sb, o)
    state, fall_z = o["state"].cpu().numpy(), o["fall_z"].cpu().numpy()
    r64 = trial_steps(O, omodels["hexapod"], tabs, states, False, hc=hc, check_from=0)
    assert np.array_equal(state[clear], r64["state"][clear])
    fell = state != RUNNING
    assert np.array_equal(fell[clear], (z < hc)[clear])
    assert np.array_equal(state[fell], states[2][fell]) and np.array_equal(fall_z[fell], z[fell].astype(np.float32))
    assert np.array_equal(kern["body"][fell], states[0][fell]) and np.array_equal(kern["seed"][fell], states[1][fell])
    assert np.array_equal(kern["tsi"][fell], states[2][fell]) and np.isnan(fall_z[~fell]).all()
    assert np.isnan(kern["torso"][fell]).all() and (kern["n_contacts"][fell] == -1).all()
    free = step_runs("hexapod")["kern"]
    for k in TRIAL_Q + ("n_contacts", "seed", "tsi"):
        assert np.array_equal(kern[k][~fell], free[k][~fell]), k


# ---- 5. hs_sim_probe
@pytest.mark.parametrize("name", ["hexapod", "myant"])
def test_probes_are_held_to_the_oracles(gpu, hmodels, oracle_mod, omodels, omodels32, teachers, name):
    """m = 5 probes from teacher states 0, 13 and 25: body_out, n_contacts and the seed after the probes against
    oracle_probes on both builds; tau_out is tau0 + dtau in float, bit for bit"""
    import torch
    from hslabs_amd import synth

    O = oracle_mod
    _, states, near = teachers(name)
    idx = list(PROBE_STATES)
    st = tuple(s[idx] for s in states)
    assert (near[idx[1:]] == 0).all()  # the two moving states are decided; the reset state is what it is
    nmj = hmodels[name].nmj
    sb = float_batch(gpu, hmodels, name, len(idx))
    set_states(sb, st)
    tau0 = st[3].astype(np.float32)
    dtau = synth.gen_torque_perturbations(len(idx), PROBE_M, nmj, seed=1).astype(np.float32)
    out = sb.probe(torch.as_tensor(dtau), tau0=torch.as_tensor(tau0), body_out=True, n_contacts=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(sb.body.cpu().numpy().astype(np.float64), st[0])  # a probe does not advance the state
    tau = tau0[:, None, :] + dtau
    assert tau.dtype == np.float32 and np.array_equal(out["tau_out"], tau)
    seed = sb.seed.cpu().numpy().view(np.uint32)
    kern, r64, r32 = ({k: [] for k in ("body", "n_contacts", "seed")} for _ in range(3))
    for b in range(len(idx)):
        for r, om, k in ((r64, omodels[name], 1e-300), (r32, omodels32[name], K_OPEN_F32)):
            bodies, ncs, seeds = oracle_probes(O, om, st[0][b], int(st[1][b]), tau[b].astype(np.float64),
                                               params=O.SimParams(k=k))
            r["body"] += list(bodies)
            r["n_contacts"] += list(ncs)
            r["seed"] += [seeds[-1]] * PROBE_M  # the chain's end: each probe's draws are the same affine map
        kern["body"] += list(out["body_out"][b].astype(np.float64))
        kern["n_contacts"] += list(out["n_contacts"][b])
        kern["seed"] += [int(seed[b])] * PROBE_M
    kern, r64, r32 = ({k: np.array(v) for k, v in r.items()} for r in (kern, r64, r32))
    assert (r64["seed"] != np.repeat(st[1], PROBE_M)).all()
    hold_to_oracles(f"{name} probes", kern, r64, r32, np.repeat(near[idx], PROBE_M), ("body",), cap=False)
