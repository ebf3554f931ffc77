"""GPU parity of the batched fall test (hs_sim_trial: the TRIAL instantiations of hs_sim_kernel)
against the oracle driven one step at a time (tests/test_sim_trial.py: oracle_trial).

Common set-up: hexapod, pgs id 8, n_t = 300, at rest at trajectory sample 2 (table row 0),
tsi0 = 2, seed 0. Both sides read the GPU's controller tables and start from the GPU's reset
state, as tests/test_gpu_sim.py does. Per-step bounds are that file's: tau_cmd 1e-9 relative to
max(1, |tau|), q_meas 1e-9, torso 1e-10 (BODY_TOL); it measures 1e-13, which leaves four orders
for the one-rounding difference of the kick emulation.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import MODELS, PGS_CONFIG
from sim_gpu_kit import BODY_TOL, batch, gpu, host  # noqa: F401
from test_sim_trial import (HC, KICK_D, KICK_EVERY, KICK_PHASE, KICK_STEPS, LIMIT_STEPS, LIMITS, N_T, RUNNING,
                            SURVIVED, TSI0, assert_kick_margins, assert_limit_margins, kick_traces, limit_traces,
                            oracle_trial)

pytestmark = pytest.mark.gpu

KICK_ARGS = dict(kick_every=KICK_EVERY, kick_phase=KICK_PHASE, hc=HC, check_from=0, check_until=-1)


@pytest.fixture(scope="module")
def hexapod(gpu):
    return gpu.KinematicModel(os.path.join(MODELS, "hexapod.xml"))


@pytest.fixture(scope="module")
def pgs8(gpu):
    return gpu.read_pgs_config(PGS_CONFIG, 8)


def kick_dv(ds=KICK_D):
    dv = np.zeros((len(ds), 3))
    dv[:, 1] = ds
    return dv


@pytest.fixture(scope="module")
def setup(gpu, hexapod, pgs8, oracle_mod, omodels):
    """the tables and the reset state both sides use"""
    sb = batch(gpu, hexapod, pgs8, 1)
    qt, dqt, tt = (t[0].cpu().numpy() for t in (sb.tables.q, sb.tables.dq, sb.tables.tau))
    assert sb.n_t == N_T and sb.table_row(TSI0) == 0
    return oracle_mod, omodels["hexapod"], qt, dqt, tt, sb.body[0].cpu().numpy()


@pytest.fixture(scope="module")
def kick_ref(setup):
    """case 2 on the oracle (computed once, read only)"""
    tr = kick_traces(*setup)
    assert_kick_margins(tr)
    return tr


@pytest.fixture(scope="module")
def kick_gpu(gpu, hexapod, pgs8):
    """case 2 on the GPU in one launch (computed once, read only)"""
    import torch

    sb = batch(gpu, hexapod, pgs8, len(KICK_D))
    out = sb.trial(KICK_STEPS, kick_dv=kick_dv(), **KICK_ARGS)
    torch.cuda.synchronize()
    return sb, out


# ---- 1. extras off is today's path
@pytest.mark.parametrize("name,pgs_id", [("hexapod", 8), ("spider", 24), ("myant", 9)])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_extras_off_is_sim_step(gpu, name, pgs_id, prec):
    import torch

    m = gpu.KinematicModel(os.path.join(MODELS, f"{name}.xml"))
    p = gpu.read_pgs_config(PGS_CONFIG, pgs_id)
    dtype = torch.float64 if prec == "f64" else torch.float32
    a, b = batch(gpu, m, p, 3, dtype=dtype), batch(gpu, m, p, 3, dtype=dtype)
    oa = a.step(40)
    ob = b.trial(40, check_from=10 ** 6)
    torch.cuda.synchronize()
    assert torch.equal(a.body, b.body) and torch.equal(a.seed, b.seed) and torch.equal(a.tsi, b.tsi)
    for k, v in oa.items():
        assert torch.equal(v, ob[k]), k
    assert (b.state == RUNNING).all()
    assert b.trial_summary() == dict(running=3, survived=0, fallen=0, min_fall_tsi=-1, sum_fall_tsi=0)


# ---- 2. kicks and falls against the oracle
def test_kicks_and_falls_match_oracle(kick_ref, kick_gpu):
    sb, out = kick_gpu
    o = host(out)
    tsi, body = sb.tsi.cpu().numpy(), sb.body.cpu().numpy()
    for b, (d, r) in enumerate(zip(KICK_D, kick_ref)):
        print(f"d={d}: state gpu {o['state'][b]} oracle {r['state']}, fall_z gpu {o['fall_z'][b]!r} oracle "
              f"{r['fall_z']!r}, min |z - hc| {np.abs(r['heights'] - HC).min():.3e}")
    for b, (d, r) in enumerate(zip(KICK_D, kick_ref)):
        assert o["state"][b] == r["state"], d
        n = len(r["torso"])  # steps taken
        if r["state"] == RUNNING:
            assert n == KICK_STEPS and tsi[b] == TSI0 + KICK_STEPS and np.isnan(o["fall_z"][b])
        else:
            assert tsi[b] == r["state"] == TSI0 + n
            assert abs(o["fall_z"][b] - r["fall_z"]) < BODY_TOL
            assert o["fall_z"][b] < HC
            # rows after the fall are untouched
            for k in ("tau_cmd", "q_meas", "torso", "normal_force"):
                assert np.isnan(o[k][b, n:]).all() and not np.isnan(o[k][b, :n]).any(), (d, k)
            assert (o["n_contacts"][b, n:] == -1).all() and (o["n_contacts"][b, :n] >= 0).all()
            assert abs(body[b, 0, 2] - r["fall_z"]) < BODY_TOL
        # per-step bounds up to 40 steps after the kick
        m = min(n, KICK_PHASE - TSI0 + 1 + 40)
        dev = {k: np.abs(r[k][:m] - o[k][b, :m]).max(axis=tuple(range(1, r[k].ndim))) for k in
               ("tau_cmd", "q_meas", "torso")}
        print(f"d={d}: max dev over {m} steps tau {dev['tau_cmd'].max():.2e} q {dev['q_meas'].max():.2e} "
              f"torso {dev['torso'].max():.2e}")
        assert dev["tau_cmd"].max() < 1e-9 * max(1, np.abs(r["tau_cmd"][:m]).max()), d
        assert dev["q_meas"].max() < 1e-9, d
        assert dev["torso"].max() < BODY_TOL, d
    st = o["state"]
    fell = st[st >= 0]
    assert sb.trial_summary() == dict(running=int((st == RUNNING).sum()), survived=int((st == SURVIVED).sum()),
                                      fallen=len(fell), min_fall_tsi=int(fell.min()), sum_fall_tsi=int(fell.sum()))


# ---- 3. launch splitting
def bits(t):
    """a floating-point tensor as integers: unwritten rows are the same NaN on both sides"""
    import torch

    if not t.is_floating_point():
        return t
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def split_equals_single(gpu, model, p, single, dv, dtype=None, **args):
    import torch

    sa, oa = single
    kw = {} if dtype is None else dict(dtype=dtype)
    sb = batch(gpu, model, p, dv.shape[0], **kw)
    names = ("tau_cmd", "q_meas", "torso", "n_contacts", "normal_force")
    parts = [sb.trial(KICK_STEPS // 3, kick_dv=dv, **args) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(sa.body, sb.body) and torch.equal(sa.seed, sb.seed) and torch.equal(sa.tsi, sb.tsi)
    assert torch.equal(sa.state, sb.state)
    assert torch.equal(bits(sa.fall_z), bits(sb.fall_z))
    for k in names:
        assert torch.equal(bits(oa[k]), bits(torch.cat([q[k] for q in parts], dim=1))), k


def test_launch_split_is_bitwise(gpu, hexapod, pgs8, kick_gpu):
    """3 launches of 50 steps: d = 100 enters the second launch frozen, d = 40, 60, 80 the third"""
    split_equals_single(gpu, hexapod, pgs8, kick_gpu, kick_dv(), **KICK_ARGS)


# ---- 4. the window
def test_check_window(gpu, hexapod, pgs8, setup, kick_ref):
    import torch

    # with check_from later than a rollout's crossing step the fall is recorded at check_from, as the
    # reference would (it checks the height, not the crossing): d = 60, 80, 100 cross before tsi 70
    late = 70
    ref = kick_traces(*setup, check_from=late)
    sb = batch(gpu, hexapod, pgs8, len(KICK_D))
    sb.trial(KICK_STEPS, kick_dv=kick_dv(), torso=True, **dict(KICK_ARGS, check_from=late))
    torch.cuda.synchronize()
    st, tsi = sb.state.cpu().numpy(), sb.tsi.cpu().numpy()
    for b, (d, r, r0) in enumerate(zip(KICK_D, ref, kick_ref)):
        assert np.abs(r["heights"][late - TSI0:] - HC).min() >= 1e-6, d  # the margin condition, on this trace
        assert st[b] == r["state"], d
        if r0["state"] == RUNNING:
            assert st[b] == RUNNING and tsi[b] == TSI0 + KICK_STEPS
        else:
            assert st[b] == max(r0["state"], late) == tsi[b], d
    assert (st == late).sum() == 3

    # with check_until = 60 whoever has not fallen by tsi 60 survives, frozen at tsi 61
    sb = batch(gpu, hexapod, pgs8, len(KICK_D))
    sb.trial(KICK_STEPS, kick_dv=kick_dv(), torso=True, **dict(KICK_ARGS, check_until=60))
    torch.cuda.synchronize()
    st, tsi = sb.state.cpu().numpy(), sb.tsi.cpu().numpy()
    for b, (d, r0) in enumerate(zip(KICK_D, kick_ref)):
        if 0 <= r0["state"] <= 60:
            assert st[b] == r0["state"] == tsi[b], d
        else:
            assert st[b] == SURVIVED and tsi[b] == 61, d
    assert (st == SURVIVED).sum() == 5 and (st >= 0).sum() == 3
    assert sb.trial_summary()["survived"] == 5


# ---- 5. torque limit
def test_torque_limit(gpu, hexapod, pgs8, setup):
    """limits 2.0 and 0.5, 130 steps, hc = 0.7. torque_limit is one value per launch
    (hs_sim_trial_args), so the two rollouts are two launches of B = 1."""
    import torch

    ref = limit_traces(*setup)
    assert_limit_margins(ref)
    free = setup[0].sim_run(setup[1], setup[0].SimParams(), N_T, *setup[2:5], setup[5], 0, TSI0, LIMIT_STEPS)
    assert np.abs(free["tau_cmd"]).max() > 2.0  # the limits clip (6.8 unclipped)
    o = {}
    for lim in LIMITS:  # the limit is one value per launch
        sb = batch(gpu, hexapod, pgs8, 1)
        out = host(sb.trial(LIMIT_STEPS, torque_limit=lim, hc=HC))
        out["tsi"] = sb.tsi.cpu().numpy()
        o[lim] = out
    torch.cuda.synchronize()
    for lim, r in zip(LIMITS, ref):
        g = o[lim]
        n = len(r["tau_cmd"])
        assert g["state"][0] == r["state"], lim
        assert g["tsi"][0] == TSI0 + n
        assert np.abs(g["tau_cmd"][0, :n]).max() <= lim
        assert np.abs(g["tau_cmd"][0, :n]).max() == lim  # ... and the clip is active
        m = min(n, 60)
        dt, dq = np.abs(r["tau_cmd"][:m] - g["tau_cmd"][0, :m]).max(), np.abs(r["q_meas"][:m] - g["q_meas"][0, :m]).max()
        print(f"limit {lim}: state {g['state'][0]}, max dev over {m} steps tau {dt:.2e} q {dq:.2e}")
        assert dt < 1e-9 * max(1, np.abs(r["tau_cmd"][:m]).max())
        assert dq < 1e-9


# ---- 6. open loop
def test_open_loop(gpu, hexapod, pgs8, setup):
    import torch

    O, om, qt, dqt, tt, body0 = setup
    sb = batch(gpu, hexapod, pgs8, 1)
    assert sb.params.k == 100
    out = host(sb.trial(60, open_loop=True, check_from=10 ** 6))
    torch.cuda.synchronize()
    rows = [(tsi % N_T + N_T - 2) % N_T for tsi in range(TSI0, TSI0 + 60)]
    assert np.array_equal(out["tau_cmd"][0], tt[rows])
    r = oracle_trial(O, om, N_T, qt, dqt, tt, body0, TSI0, 60, open_loop=True, check_from=10 ** 6)
    assert np.abs(r["q_meas"] - out["q_meas"][0]).max() < 1e-9
    assert np.abs(r["torso"] - out["torso"][0]).max() < BODY_TOL
    assert np.abs(r["body"] - sb.body[0].cpu().numpy()).max() < BODY_TOL


# ---- 7. fp32
def test_f32_falls_and_split(gpu, hexapod, pgs8, kick_ref):
    import torch

    ds = (0.0, 10.0, 40.0, 60.0, 80.0, 100.0)  # the wide margins: minima >= 0.788, falls before step 80
    sb = batch(gpu, hexapod, pgs8, len(ds), dtype=torch.float32)
    out = sb.trial(KICK_STEPS, kick_dv=kick_dv(ds), **KICK_ARGS)
    torch.cuda.synchronize()
    st = sb.state.cpu().numpy()
    want = np.array([kick_ref[KICK_D.index(d)]["state"] for d in ds])
    print("fp32 fall tsi", dict(zip(ds, st.tolist())), "fp64", dict(zip(ds, want.tolist())))
    assert ((st >= 0) == (want >= 0)).all()
    assert (st[want < 0] == RUNNING).all()
    assert out["tau_cmd"].dtype == torch.float32 and sb.fall_z.dtype == torch.float32
    split_equals_single(gpu, hexapod, pgs8, (sb, out), kick_dv(ds), dtype=torch.float32, **KICK_ARGS)


# ---- 8. bad arguments fail loudly
def trial_args(sb, gpu, dv=None):
    from hslabs_amd import capi

    t = capi.SimTrialArgsC()
    a = t.sim
    a.n_rollouts, a.n_steps, a.n_t = sb.B, 1, sb.n_t
    a.params = sb.params
    a.body, a.seed, a.tsi = sb.body.data_ptr(), sb.seed.data_ptr(), sb.tsi.data_ptr()
    a.q_tab, a.dq_tab, a.tau_tab = sb.tables.q.data_ptr(), sb.tables.dq.data_ptr(), sb.tables.tau.data_ptr()
    t.state = sb._state.data_ptr()
    if dv is not None:
        t.kick_dv = dv.data_ptr()
    return t


@pytest.fixture(scope="module")
def bad(gpu, hexapod, pgs8):
    import torch

    sb = batch(gpu, hexapod, pgs8, 2)
    sb._state = torch.full((2,), RUNNING, dtype=torch.int32, device=sb.device)
    dv = torch.zeros((2, 3), dtype=torch.float64, device=sb.device)
    torch.cuda.synchronize()
    return sb, dv, sb.body.clone()


def rejected(gpu, hexapod, bad, t, word):
    import torch

    from hslabs_amd import capi

    sb, _, body0 = bad
    L = capi.load()
    assert L.hs_sim_trial(hexapod.handle, ctypes.byref(t)) == -1  # HS_E_ARG
    assert word.encode() in L.hs_last_error(), L.hs_last_error()
    torch.cuda.synchronize()
    assert torch.equal(sb.body, body0) and (sb.tsi == TSI0).all() and (sb._state == RUNNING).all()  # nothing ran


def test_rejects_null_state(gpu, hexapod, bad):
    t = trial_args(bad[0], gpu)
    t.state = None
    rejected(gpu, hexapod, bad, t, "state")


@pytest.mark.parametrize("phase", [-1, 5, 9])
def test_rejects_kick_phase_outside_period(gpu, hexapod, bad, phase):
    t = trial_args(bad[0], gpu, bad[1])
    t.kick_every, t.kick_phase = 5, phase
    rejected(gpu, hexapod, bad, t, "kick_phase")


def test_rejects_kicks_without_dv(gpu, hexapod, bad):
    t = trial_args(bad[0], gpu)
    t.kick_every, t.kick_phase = 5, 0
    rejected(gpu, hexapod, bad, t, "kick_dv")


def test_rejects_negative_torque_limit(gpu, hexapod, bad):
    t = trial_args(bad[0], gpu)
    t.torque_limit = -1.0
    rejected(gpu, hexapod, bad, t, "torque_limit")


def test_rejects_what_sim_step_rejects(gpu, hexapod, bad):
    t = trial_args(bad[0], gpu)
    t.sim.q_tab = None
    rejected(gpu, hexapod, bad, t, "tables")
    t = trial_args(bad[0], gpu)
    t.sim.params.mu = 0.0
    rejected(gpu, hexapod, bad, t, "mu")
    t = trial_args(bad[0], gpu)
    t.sim.body = None
    rejected(gpu, hexapod, bad, t, "body")
    t = trial_args(bad[0], gpu)
    t.sim.params.k = 0.0
    t.sim.tau_tab = None
    t.open_loop = 1
    rejected(gpu, hexapod, bad, t, "open_loop")


# ---- 9. the handle
def test_handle_runs_the_trial(gpu, hexapod, pgs8, kick_ref):
    """hs_sim_create + hs_sim_set_trial + hs_sim_advance, B = 2: case 2's d = 0 and d = 40"""
    from hslabs_amd import capi
    from hslabs_amd.api import params_array

    L = capi.load()
    arr = params_array([pgs8, pgs8])
    h = ctypes.c_void_p()
    gp = arr.ctypes.data_as(ctypes.POINTER(capi.GaitParamsC))
    capi.check(L.hs_sim_create(hexapod.handle, gp, 2, None, TSI0 * 0.01, ctypes.byref(h)), "hs_sim_create")
    try:
        st = np.zeros(2, np.int32)
        assert L.hs_sim_get_trial_state(h, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1
        dv = np.ascontiguousarray(kick_dv((0.0, 40.0)))
        capi.check(L.hs_sim_set_trial(h, 0, 0.0, KICK_EVERY, KICK_PHASE, dv.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                      HC, 0, -1), "hs_sim_set_trial")
        torso = np.full((2, 50, 3), np.nan)
        for _ in range(3):
            capi.check(L.hs_sim_advance(h, 50, None, None, torso.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None,
                                        None), "hs_sim_advance")
        tsi = np.zeros(2, np.int32)
        capi.check(L.hs_sim_get_trial_state(h, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "get_trial_state")
        capi.check(L.hs_sim_get_state(h, None, tsi.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "get_state")
    finally:
        L.hs_sim_free(h)
    r0, r40 = kick_ref[KICK_D.index(0.0)], kick_ref[KICK_D.index(40.0)]
    assert st.tolist() == [r0["state"], r40["state"]] == [RUNNING, 74]
    assert tsi.tolist() == [TSI0 + KICK_STEPS, 74]
    assert (torso[1] == 0).all()  # d = 40 entered the third call frozen: its rows stay as the handle cleared them
