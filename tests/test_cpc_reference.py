"""Configuration path control (hs_cpc_torques / hs_cpc_target_points / hs_sim_cpc_step: cpccontroller, cpc.cpp,
as modelplayer::set_cpc_torques drives it, player.cpp:465-481) off the GPU: `cpc_reference`, the NumPy
restatement of the controller the GPU tests compare with (solves by numpy.linalg.solve), the seeded fixture
builder, the conditions the fixtures must meet so that the GPU comparison may demand equal choices, the known
answers, the ctypes mirrors, the exports and the argument checks. tests/test_gpu_cpc.py imports these.

Every choice of the controller is a comparison of rounded values: which losses are the n_cand smallest and in
which order, which candidate has the best score in a pass of the gain loop, whether that candidate's torque norm
exceeds tauc, whether the state is within tp_dist of the chosen target point. `cpc_reference` returns the
relative margin of each; where all exceed MARGIN the GPU must choose alike.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT

DIMS = {"hexapod": (24, 18), "myant": (18, 12)}   # config_dim, nmj
DEFAULTS = dict(w=10., sg=1., n_cand=10, k0=200., kc=10., tauc=20., loss_cc=10., tp_dist=0.5, goal_t0s=1,
                tpdist_switch=1, mask=(0, 1, 5))  # player.cpp:453, 458; cpc.cpp:40-42, 188, 490
FLAG_NONFINITE, FLAG_NOSCORE, FLAG_RANK = 1, 2, 4
MARGIN = 1e-6
DT = 0.01
SEED = 7
SHAPES = ((70, 10), (10, 10), (70, 1), (130, 4))  # (n_tp, n_cand): two lane passes with a partial second, every
#                                                   point a candidate, a single candidate, three passes
TAUCS = (1e9, 20., 1e-3)
NOISE = ((0., 0.), (1e-3, 1e-3), (1e-2, 1e-2), (5e-2, 5e-2), (0.2, 0.2), (0.05, 0.5))  # (q, dq) of the six states


def rel(a, b):
    """relative distance of two compared values; inf where one is not finite (it sorts last, no tie)"""
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf
    d = max(abs(a), abs(b))
    return abs(a - b) / d if d > 0 else 0.0


def apply_mask(x, cfg, mask):
    x = np.array(x, dtype=np.float64)
    for i in mask:
        x[..., i] = 0
        x[..., cfg + i] = 0
    return x


def cpc_reference(Bt, q, dq, tp, low_tpdist=1, **kw):
    """cpccontroller::get_motor_torques for one rollout, in the reference's order. Bt [nmj][cfg], q / dq [cfg]
    (unmasked), tp [n_tp][2 cfg + nmj] (masked). Returns tau, last_tpi, low_tpdist, flags, loss, cand_tpi,
    cand_t0s, passes, i_best and `margin`, the smallest relative margin of its choices (with `margins`, each)."""
    P = dict(DEFAULTS, **kw)
    nmj, cfg = Bt.shape
    psi, nc, n_tp = cfg - nmj, int(P["n_cand"]), tp.shape[0]
    assert n_tp >= nc >= 1
    flags, margins = 0, {}
    # set_current_state + apply_mask, on a copy
    st = apply_mask(np.concatenate([q, dq]), cfg, P["mask"])
    q0, dq0 = st[:cfg], st[cfg:]
    # compute_b
    Bt_chi = Bt[:, psi:]
    b = np.vstack([-np.eye(psi), np.linalg.solve(Bt_chi, Bt[:, :psi])])
    bbt = b @ b.T
    # compute_prox_loss_over_tps
    qd, dqd, taud = tp[:, :cfg], tp[:, cfg:2 * cfg], tp[:, 2 * cfg:]
    with np.errstate(all="ignore"):
        btil = dqd @ bbt.T
        del_q = qd - q0
        denom = btil @ dq0
        t0 = (btil * del_q).sum(1) / denom
        s = (btil * dqd).sum(1) / denom
        c0 = (del_q - dqd * t0[:, None] / s[:, None]) @ b
        c1 = (dqd / s[:, None] - dq0) @ b
        loss = (P["w"] * t0) ** 2 + (s - P["sg"]) ** 2 + P["loss_cc"] * ((c0 * c0).sum(1) + (c1 * c1).sum(1))
    if not np.isfinite(loss).all():
        flags |= FLAG_NONFINITE
    # candidates: ascending loss, ties and non-finite losses by index
    key = np.where(np.isfinite(loss), loss, np.inf)
    order = np.lexsort((np.arange(n_tp), key))
    cand = order[:nc]
    margins["loss order"] = min([rel(key[order[i]], key[order[i + 1]]) for i in range(min(nc, n_tp - 1))] or [np.inf])
    t0c, sc, lc = t0[cand], s[cand].copy(), loss[cand]
    if P["goal_t0s"] and (not P["tpdist_switch"] or low_tpdist):
        sc[:] = P["sg"]
    # the gain loop over cost2
    B_chi = Bt_chi.T
    chi0, dchi0 = q0[psi:], dq0[psi:]
    chid, dchid = qd[cand][:, psi:], dqd[cand][:, psi:]
    k, passes = P["k0"], 0
    margins["score"], margins["tauc"] = np.inf, np.inf
    while True:
        with np.errstate(all="ignore"):
            Kd = k * (chi0 - chid + dchid * t0c[:, None] / sc[:, None]) + 2 * np.sqrt(k) * (dchi0 - dchid / sc[:, None])
            taus = taud[cand] - np.linalg.solve(B_chi, Kd.T).T
            norms = np.sqrt((taus * taus).sum(1))
            score = norms / (norms.sum() / nc) + lc / (lc.sum() / nc)
        i_best, score_min = -1, 1e10
        for i in range(nc):
            if score[i] < score_min:
                i_best, score_min = i, score[i]
        if i_best < 0:
            flags |= FLAG_NOSCORE
            i_best = 0
        elif nc > 1:
            margins["score"] = min(margins["score"], min(rel(score[i_best], score[i]) for i in range(nc) if i != i_best))
        k /= 2
        passes += 1
        margins["tauc"] = min(margins["tauc"], rel(norms[i_best], P["tauc"]))
        if not (k > P["kc"] and norms[i_best] > P["tauc"]):
            break
    # last_cand, tp_dist_check, clip_norm
    tpi = int(cand[i_best])
    dist = np.sqrt(((st - tp[tpi, :2 * cfg]) ** 2).sum())
    margins["tp_dist"] = rel(dist, P["tp_dist"])
    tau = taus[i_best].copy()
    if norms[i_best] > P["tauc"]:
        tau *= P["tauc"] / norms[i_best]
    return dict(tau=tau, last_tpi=tpi, low_tpdist=int(dist < P["tp_dist"]), flags=flags, loss=loss,
                cand_tpi=cand.astype(np.int32), cand_t0s=np.stack([t0c, sc], 1), passes=passes, i_best=i_best,
                margins=margins, margin=min(margins.values()), b=b, Bt_chi=Bt_chi)


# ---- the fixtures
def make_fixture(name, n_tp, seed=SEED):
    """Six rollouts of model `name` over n_tp target points: tp [n_tp][2 cfg + nmj] on a closed two-harmonic
    path q(theta) with its analytic rate at dt = DT per point, random torque rows, masked; Bt [6][nmj][cfg] =
    [0.3 N | 2 I + 0.1 N] (cond(B_chi) about 1.7); states [6][2][cfg] on the NOISE ladder around the points `at`."""
    cfg, nmj = DIMS[name]
    rng = np.random.default_rng([seed, cfg, n_tp])
    th = 2 * np.pi * np.arange(n_tp) / n_tp
    om = 2 * np.pi / (n_tp * DT)
    a0 = rng.uniform(-0.5, 0.5, cfg)
    A = rng.uniform(-0.3, 0.3, (4, cfg))
    A[2:] *= 0.4
    q = a0 + np.outer(np.cos(th), A[0]) + np.outer(np.sin(th), A[1]) + np.outer(np.cos(2 * th), A[2]) + \
        np.outer(np.sin(2 * th), A[3])
    dq = om * (-np.outer(np.sin(th), A[0]) + np.outer(np.cos(th), A[1]) - 2 * np.outer(np.sin(2 * th), A[2]) +
               2 * np.outer(np.cos(2 * th), A[3]))
    tau = rng.uniform(-1, 1, (n_tp, nmj))
    tp = np.concatenate([apply_mask(np.concatenate([q, dq], 1), cfg, DEFAULTS["mask"]), tau], 1)
    n = len(NOISE)
    Bt = np.concatenate([0.3 * rng.standard_normal((n, nmj, cfg - nmj)),
                         2 * np.eye(nmj) + 0.1 * rng.standard_normal((n, nmj, nmj))], 2)
    at = np.array([(7 * j + 3) % n_tp for j in range(n)])
    states = np.empty((n, 2, cfg))
    for j, (nq, ndq) in enumerate(NOISE):
        states[j, 0] = tp[at[j], :cfg] + nq * rng.standard_normal(cfg)
        states[j, 1] = tp[at[j], cfg:2 * cfg] + ndq * rng.standard_normal(cfg)
    return dict(name=name, n_tp=n_tp, tp=np.ascontiguousarray(tp), Bt=Bt, states=states, at=at)


_SWEEP = {}


def sweep():
    """[(name, n_tp, n_cand, tauc, fixture, rollouts, [cpc_reference per rollout])], computed once. For n_cand = 1
    the on-path state is left out: its single loss is 0, the score 0 / 0 (HS_CPC_FLAG_NOSCORE)."""
    if not _SWEEP:
        rows = []
        for name in sorted(DIMS):
            for n_tp, nc in SHAPES:
                fx = make_fixture(name, n_tp)
                rollouts = [j for j in range(len(NOISE)) if not (nc == 1 and j == 0)]
                for tauc in TAUCS:
                    refs = [cpc_reference(fx["Bt"][j], fx["states"][j, 0], fx["states"][j, 1], fx["tp"], n_cand=nc,
                                          tauc=tauc) for j in rollouts]
                    rows.append((name, n_tp, nc, tauc, fx, rollouts, refs))
        _SWEEP["rows"] = rows
    return _SWEEP["rows"]


# ---- 1. the conditions on the fixtures
def test_fixture_margins_passes_and_tpdist():
    worst, passes, low = np.inf, set(), set()
    for name, n_tp, nc, tauc, fx, rollouts, refs in sweep():
        for j, r in zip(rollouts, refs):
            assert r["flags"] == 0, (name, n_tp, nc, tauc, j)
            assert r["margin"] > MARGIN, (name, n_tp, nc, tauc, j, r["margins"])
            worst = min(worst, r["margin"])
            passes.add(r["passes"])
            low.add(r["low_tpdist"])
    print(f"smallest ordering margin of the sweep: {worst:.3e}; passes seen {sorted(passes)}")
    assert 1 in passes and 5 in passes and passes & {2, 3, 4}, passes
    assert passes <= {1, 2, 3, 4, 5}
    assert low == {0, 1}


def test_fixture_conditioning():
    for name in DIMS:
        fx = make_fixture(name, 70)
        cfg, nmj = DIMS[name]
        c = [np.linalg.cond(fx["Bt"][j][:, cfg - nmj:]) for j in range(len(NOISE))]
        print(f"{name}: cond(B_chi) {min(c):.2f} .. {max(c):.2f}")
        assert max(c) < 3


# ---- 2. known answers
@pytest.mark.parametrize("name", sorted(DIMS))
def test_on_path_known_answer(name):
    """state = target point i, n_cand >= 2, tauc = 1e9: t0 = 0, s = 1, loss = 0, tpi = i, tau = tau_tp[i]"""
    cfg, nmj = DIMS[name]
    for n_tp, nc in ((70, 10), (10, 10), (130, 4)):
        fx = make_fixture(name, n_tp)
        i = int(fx["at"][0])
        for low in (0, 1):
            r = cpc_reference(fx["Bt"][0], fx["states"][0, 0], fx["states"][0, 1], fx["tp"], low_tpdist=low, n_cand=nc,
                              tauc=1e9)
            assert r["last_tpi"] == i and r["cand_tpi"][0] == i and r["i_best"] == 0 and r["passes"] == 1
            assert abs(r["cand_t0s"][0, 0]) < 1e-14 and abs(r["cand_t0s"][0, 1] - 1) < 1e-13
            assert r["loss"][i] < 1e-24
            assert np.abs(r["tau"] - fx["tp"][i, 2 * cfg:]).max() < 1e-12
            assert r["low_tpdist"] == 1 and r["flags"] == 0
            assert np.abs(fx["Bt"][0] @ r["b"]).max() <= 1e-14  # Bt b = 0: b spans the uncontrolled directions


def test_reference_undefined_cases():
    fx = make_fixture("myant", 70)
    cfg, nmj = DIMS["myant"]
    Bt, (q, dq), tp = fx["Bt"][1], fx["states"][1], fx["tp"]
    base = cpc_reference(Bt, q, dq, tp)
    # a zero-velocity target point: denom = 0, the loss is not finite, it sorts last and changes nothing else
    z = tp[5].copy()
    z[cfg:2 * cfg] = 0
    r = cpc_reference(Bt, q, dq, np.vstack([tp, z]))
    assert r["flags"] == FLAG_NONFINITE and not np.isfinite(r["loss"][-1])
    assert np.array_equal(r["cand_tpi"], base["cand_tpi"]) and np.array_equal(r["tau"], base["tau"])
    # exactly equal losses are both kept, the lower index first
    r = cpc_reference(Bt, q, dq, np.vstack([tp, tp[base["cand_tpi"][0]]]))
    assert list(r["cand_tpi"][:2]) == [base["cand_tpi"][0], 70] and r["margins"]["loss order"] == 0
    # n_cand = 1 on the path: 0 / 0
    r = cpc_reference(fx["Bt"][0], fx["states"][0, 0], fx["states"][0, 1], tp, n_cand=1, tauc=1e9)
    assert r["flags"] == FLAG_NOSCORE and r["i_best"] == 0 and r["last_tpi"] == fx["at"][0]
    # the carried state: own s against sg
    a, b = cpc_reference(Bt, q, dq, tp, low_tpdist=0), cpc_reference(Bt, q, dq, tp, low_tpdist=1)
    assert (b["cand_t0s"][:, 1] == 1).all() and (a["cand_t0s"][:, 1] != 1).all()
    assert np.array_equal(a["cand_t0s"][:, 0], b["cand_t0s"][:, 0])
    c = cpc_reference(Bt, q, dq, tp, low_tpdist=0, tpdist_switch=0)
    assert (c["cand_t0s"][:, 1] == 1).all()


# ---- 3. structs, exports
def test_struct_offsets_match_the_header(tmp_path):
    from hslabs_amd import capi

    P, A, S = capi.CpcParamsC, capi.CpcArgsC, capi.SimCpcArgsC
    probes = [("hs_cpc_params", P, ("w", "tp_dist", "n_cand", "goal_t0s", "tpdist_switch", "mask")),
              ("hs_cpc_args", A, ("n_tp", "params", "Bt", "state", "state_stride", "tp", "tp_stride", "low_tpdist", "tau",
                                  "last_tpi", "flags", "loss", "cand_tpi", "cand_t0s", "passes", "i_best", "stream")),
              ("hs_sim_cpc_args", S, ("trial", "cpc", "m", "n_tp", "dtau", "dtau_step_stride", "tp", "tp_stride", "ders",
                                      "tau0", "low_tpdist", "last_tpi", "flags", "rank", "workspace", "workspace_bytes"))]
    exprs, want = [], []
    for cname, cls, fields in probes:
        exprs.append(f"sizeof({cname})")
        want.append(ctypes.sizeof(cls))
        for f in fields:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(cls, f).offset)
    exprs += ["(size_t)HSLABS_ABI_VERSION", "(size_t)HS_CPC_FLAG_NONFINITE", "(size_t)HS_CPC_FLAG_NOSCORE",
              "(size_t)HS_CPC_FLAG_RANK"]
    want += [capi.ABI_VERSION, capi.HS_CPC_FLAG_NONFINITE, capi.HS_CPC_FLAG_NOSCORE, capi.HS_CPC_FLAG_RANK]
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hslabs.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "offsets"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert capi.ABI_VERSION == 16
    assert (FLAG_NONFINITE, FLAG_NOSCORE, FLAG_RANK) == (capi.HS_CPC_FLAG_NONFINITE, capi.HS_CPC_FLAG_NOSCORE,
                                                         capi.HS_CPC_FLAG_RANK)


def test_library_exports_the_cpc_symbols(product):
    L = ctypes.CDLL(product.capi.lib_path())
    names = ("hs_cpc_default_params", "hs_cpc_torques", "hs_cpc_target_points", "hs_sim_cpc_workspace",
             "hs_sim_cpc_step")
    hdr = open(os.path.join(ROOT, "include", "hslabs.h")).read()
    for name in names:
        assert name in product.capi.EXPORTS
        assert hasattr(L, name), name
        assert f"{name}(" in hdr, name
    assert product.capi.ABI_VERSION == 16 and L.hs_abi_version() == 16


def test_default_params_are_the_references(product):
    p = product.SimBatch.cpc_default_params()
    got = dict(w=p.w, sg=p.sg, n_cand=p.n_cand, k0=p.k0, kc=p.kc, tauc=p.tauc, loss_cc=p.loss_cc, tp_dist=p.tp_dist,
               goal_t0s=p.goal_t0s, tpdist_switch=p.tpdist_switch,
               mask=tuple(i for i in range(32) if p.mask >> i & 1))
    assert got == DEFAULTS


# ---- 4. argument checks, no device
def check_argument_cases(product):
    """every HS_E_ARG case of hs_cpc_torques, hs_cpc_target_points and hs_sim_cpc_step; each is decided before
    any device call, so the pointers only need to be non-NULL"""
    capi = product.capi
    L = capi.load()
    m = product.KinematicModel(os.path.join(MODELS, "hexapod.xml"))
    h, nmj, cfg = m.handle, m.nmj, m.config_dim
    rec = 2 * cfg + nmj
    x = ctypes.create_string_buffer(64)
    p = ctypes.addressof(x)
    F64, F32, E = capi.HS_PREC_F64, capi.HS_PREC_F32, -1
    required = ("Bt", "state", "tp", "low_tpdist", "tau", "last_tpi", "flags")

    def cpc_args(n_cand=10, **kw):
        a = capi.CpcArgsC()
        a.n_rollouts, a.n_tp, a.precision = 1, 70, F64
        a.params = product.SimBatch.cpc_default_params()
        a.params.n_cand = n_cand
        a.state_stride = 3 * cfg
        for f in required:
            setattr(a, f, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.hs_cpc_torques(h, None) == E
    assert L.hs_cpc_torques(None, ctypes.byref(cpc_args())) == E
    for f in required:
        assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(**{f: None}))) == E, f
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(precision=F32))) == E
    assert b"double precision" in L.hs_last_error()
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(n_tp=9))) == E            # n_tp < n_cand
    assert b"n_tp < n_cand" in L.hs_last_error()
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(n_cand=65, n_tp=200))) == E
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(n_cand=0))) == E
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(state_stride=2 * cfg - 1))) == E
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(tp_stride=70 * rec - 1))) == E
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(n_tp=1 << 20))) == E       # beyond the kernel's LDS
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(n_rollouts=-1))) == E
    for k, v in (("kc", 0.0), ("kc", -1.0), ("k0", float("inf")), ("k0", float("nan"))):  # the gain loop would not end
        a = cpc_args()
        setattr(a.params, k, v)
        assert L.hs_cpc_torques(h, ctypes.byref(a)) == E, (k, v)
    assert L.hs_cpc_torques(h, ctypes.byref(cpc_args(n_rollouts=0))) == 0       # nothing to do
    # hs_cpc_target_points
    assert L.hs_cpc_target_points(None, 1, 70, p, p, p, 0x23, p, None) == E
    for i in (3, 4, 5, 7):
        a = [h, 1, 70, p, p, p, 0x23, p, None]
        a[i] = None
        assert L.hs_cpc_target_points(*a) == E, i
    assert L.hs_cpc_target_points(h, 1, 0, p, p, p, 0x23, p, None) == E
    assert L.hs_cpc_target_points(h, 0, 70, None, None, None, 0x23, None, None) == 0
    # hs_sim_cpc_step
    need = L.hs_sim_cpc_workspace(h, 1, cfg + 20)
    assert need >= (cfg + 20) * (2 * cfg + nmj) * 8
    step_required = ("dtau", "tp", "ders", "tau0", "low_tpdist", "last_tpi", "flags", "rank", "workspace")

    def step_args(sim=None, trial=None, **kw):
        c = capi.SimCpcArgsC()
        s = c.trial.sim
        s.n_rollouts, s.n_steps, s.n_t, s.precision = 1, 2, 1, F64
        s.params = product.SimBatch.default_params()
        s.body = s.seed = s.tsi = p
        c.trial.state = p
        c.cpc = product.SimBatch.cpc_default_params()
        c.m, c.n_tp = cfg + 20, 70
        for f in step_required:
            setattr(c, f, p)
        c.workspace_bytes = need
        for k, v in (sim or {}).items():
            setattr(s, k, v)
        for k, v in (trial or {}).items():
            setattr(c.trial, k, v)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert L.hs_sim_cpc_step(h, None) == E
    assert L.hs_sim_cpc_step(None, ctypes.byref(step_args())) == E
    for f in step_required:
        assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(**{f: None}))) == E, f
    for f in ("body", "seed", "tsi"):
        assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(sim={f: None}))) == E, f
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(trial={"state": None}))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(workspace_bytes=need - 1))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(sim={"precision": F32}))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(sim={"n_steps": -1}))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(m=nmj))) == E              # 0 < m < nmj + 1
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(n_tp=9))) == E
    cp = product.SimBatch.cpc_default_params()
    cp.n_cand = 65
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(cpc=cp, n_tp=200))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(trial={"torque_limit": -1.0}))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(trial={"kick_every": 5, "kick_phase": 5, "kick_dv": p}))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(trial={"kick_every": 5, "kick_phase": 4}))) == E  # no kick_dv
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(dtau_step_stride=1))) == E
    assert L.hs_sim_cpc_step(h, ctypes.byref(step_args(sim={"n_steps": 0}))) == 0  # nothing to do


def test_argument_validation(product):
    check_argument_cases(product)
