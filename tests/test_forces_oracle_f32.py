"""The single-precision build of the oracle (oracle/hs_oracle_f32.cpp) on solve_forces, off the GPU: what
makes it a reference the fp32 solve_forces kernel can be bounded by (tests/test_gpu_forces_f32_oracle.py and
tests/test_gpu.py import the helpers below).

Inputs (gait_inputs): synth.gen_params(48, name, id0=4321) straight and curved, and the stretched set
gen_params(128, name, id0=11) with step_length * 2.5; n_t = 20, k0 = 0, H = 20. Torques (perturbed_tau): the
fp64 oracle's own (fast basis) + 0.25 cos(step + motor), rounded to float, so the least squares is
inconsistent (a residual of order 1) and both builds and the kernel are handed the same bits.

On these inputs neither build flags HS_FLAG_GENERAL or HS_FLAG_NEAR_RANK on any step (the smallest squared
pivot over the largest reduced diagonal stays at or above 10^-2.4, far from the 1e-10 and 1e-4 guards), and
spread() -- per step, the largest |f32 - f64| over the force components relative to max(1, max |f64|) of
the step -- stays within FP32_TOL. Measured here (printed by test_f32_build_within_fp32_tol), max / median:
  ordinary (straight and curved)  hexapod 3.4e-5 / 7e-7   spider 2.5e-5 / 6e-7   myant 1.6e-5 / 5e-7
  stretched (x 2.5)               hexapod 3.5e-5          spider 1.2e-5          myant 9.5e-6

The lifted-torso cases (tests/test_oracle.py LIFTED_CASES) are where a force column is dropped. The fp64
build drops at 1e-10 of the largest reduced diagonal, the single-precision build at the kernel's float
kFastPivotGuard, 1e-4 (1e-10 is under float epsilon: no column would ever drop). Where the two builds drop
other columns their answers differ at order 1, legitimately: the solution is not unique. What can be held
on every such step is that the answer is a least-squares solution over its own kept columns, gamma():
  gamma = max |A_f^T r| / (max diag(A_f^T A_f) * max(1, max |y|)),
A_f the kept force columns of the dense system (test_oracle.forces_system) with the wrench columns projected
out, r the projected right-hand side minus A_f y. It is first order in the error of y (the residual norm is
second order and does not separate a 1 % error from float rounding). Measured: fp64 build 1.4e-15, single-
precision build 7e-7.

block_ratio() restates what routes a step of the kernel in HS_SOLVE_AUTO (the foot blocks' LDL^T pivot ratio
against kForcesBlockGuard), so that the GPU test can tell which route a step took.
"""
import os

import numpy as np
import pytest

from conftest import MODELS, record_to_oracle_gait
from test_oracle import LIFTED_CASES, forces_system

FP32_TOL = 1e-3  # the project's stated single-precision bound (tests/test_gpu.py)
NAMES = ("hexapod", "spider", "myant")
KINDS = ("straight", "curved", "stretched")
N_T = 20
BAD = 64 | 512 | 256 | 8  # GENERAL | DEPENDENT | NEAR_RANK | NAN
CLEAN_DROP = 16 | 64 | 512  # 592: clamped, a column dropped, no decision near its threshold


def f32(a):
    """a rounded to float, as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="session")
def omodels32(oracle_mod):
    """the models of conftest's omodels, owned by the single-precision build"""
    L = oracle_mod.lib_f32()
    return {name: oracle_mod.Model(os.path.join(MODELS, f"{name}.xml"), L=L) for name in NAMES}


def gait_inputs(name, kind):
    """the GAIT_DTYPE records of an input set: 48 straight or curved gaits, or the 128 stretched ones"""
    from hslabs_amd import synth

    if kind == "stretched":
        p = synth.gen_params(128, name, id0=11)
        p["step_length"] *= 2.5
        return p
    return synth.gen_params(48, name, id0=4321, curved=(kind == "curved"))


def gait_record(g):
    """an oracle GaitParams (no record transform) as a GAIT_DTYPE record"""
    from hslabs_amd import GAIT_DTYPE

    r = np.zeros((), GAIT_DTYPE)
    r["torso_pos"], r["torso_angles"] = g.torso_pos, g.torso_angles
    for k in ("step_duration", "period", "step_length", "step_height", "curvature", "foot_shift", "foot_shift_type"):
        r[k] = getattr(g, k)
    assert g.rec_transform is None
    return r


def perturbed_tau(O, om, gaits, H=N_T):
    """[B][H][nmj]: the fp64 oracle's torques + 0.25 cos(step + motor), rounded to float"""
    tau = O.batch(om, gaits, N_T, 0, H, basis=O.BASIS_FAST, n_threads=8)["tau"]
    return f32(tau + 0.25 * np.cos(np.arange(H)[None, :, None] + np.arange(om.nmj)[None, None, :]))


def spread(cf, ref):
    """per step [...]: the largest |cf - ref| over the force components, relative to max(1, max |ref|) of the step"""
    cf, ref = np.asarray(cf, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(cf - ref).max(axis=-1) / np.maximum(1.0, np.abs(ref).max(axis=-1))


def both_builds(O, om, om32, params):
    """gaits, the perturbed torques and solve_forces of both builds on them: (gaits, tau, r64, r32)"""
    gaits = [record_to_oracle_gait(O, r) for r in params]
    tau = perturbed_tau(O, om, gaits)
    return gaits, tau, O.forces_batch(om, gaits, tau, N_T, n_threads=8), O.forces_batch(om32, gaits, tau, N_T, n_threads=8)


def dropped_set(cf):
    """[..., 3 nf] bool: the components that are exactly 0 (a dropped column's)"""
    return np.asarray(cf) == 0


def dependent_where_zero(cf, flags):
    """GENERAL | DEPENDENT set exactly on the steps with a component that is exactly 0"""
    z = dropped_set(cf).any(axis=-1)
    fl = np.asarray(flags)
    return bool(np.array_equal((fl & 512) != 0, z) and np.array_equal((fl & 64) != 0, z))


def gamma(O, om, g, step, z, y):
    """the gradient of the least squares at y over y's kept columns (module docstring); om: the fp64 model"""
    A, b, y0 = forces_system(O, om, g, step, z)
    y = np.asarray(y, dtype=np.float64)
    U, s, _ = np.linalg.svd(A[:, :y0], full_matrices=False)
    U = U[:, s > 1e-12 * s[0]]
    kept = np.nonzero(y != 0)[0]
    Af = A[:, y0 + kept]
    Af = Af - U @ (U.T @ Af)
    r = (b - U @ (U.T @ b)) - Af @ y[kept]
    if len(kept) == 0:
        return 0.0
    return float(np.abs(Af.T @ r).max() / ((Af * Af).sum(axis=0).max() * max(1.0, np.abs(y).max())))


def gammas(O, om, g, z, cf, steps=None):
    steps = range(len(cf)) if steps is None else steps
    return np.array([gamma(O, om, g, int(s), z[s], cf[s]) for s in steps])


FORCES_BLOCK_GUARD_F32 = 1e-3  # the kernel's float kForcesBlockGuard (hslabs_amd/csrc/hs_step_solve.h)
ROUTE_BAND = 2.0               # a step's route is decided when its ratio is this factor away from the guard


def block_ratio(O, om, g, step):
    """What routes a step of forces_solve in HS_SOLVE_AUTO: over the feet, the smallest LDL^T pivot (natural
    order) of the foot's block B_f = C_mf^T M_l^-1 C_mf over B_f's largest diagonal entry, from the fp64 oracle's
    dynamics record (forces_rows and forces_foot restated: the limb's three hinge parts p0 < p1 < p2 above the
    foot, part p_i in the subtrees of motors 0 .. i, M_l = I + sum of the motors' unit-rate momenta products,
    C_mf the torques of a unit force at the foot about the three axes). A step takes the 6 x 6 route iff every
    foot's ratio is above kForcesBlockGuard. In float the ratio carries the rounding of B_f's entries (a few
    1e-7 of its diagonal, so 1e-3 of the guard's 1e-3): ROUTE_BAND = 2 is far outside it."""
    d = O.dynrec_dump(om, g, N_T, int(step))
    par, ratios = d["parents"], []
    for fi, p2 in enumerate(d["footis"]):
        p = [par[par[p2]], par[p2], p2]
        assert set(p) <= set(d["hinge_ids"].tolist())
        J, Z, P, fp = d["jpos"][p], d["jz"][p], d["pos"][p], d["fpos"][fi]
        M = np.eye(3)
        for k in range(3):
            for k2 in range(3):
                for i in range(max(k, k2), 3):
                    M[k, k2] += np.cross(J[k] - P[i], Z[k]) @ np.cross(J[k2] - P[i], Z[k2]) + Z[k] @ Z[k2]
        C = np.array([[Z[k] @ np.cross(fp - J[k], e) for e in np.eye(3)] for k in range(3)])
        a = C.T @ np.linalg.solve(M, C)
        mx, piv = a.diagonal().max(), []
        for j in range(3):
            piv.append(a[j, j])
            if not a[j, j] > 0:
                break
            a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j, j + 1:]) / a[j, j]
        ratios.append(min(piv) / mx)
    return min(ratios)


def block_ratios(O, om, gaits):
    """[B][20]: block_ratio of every step"""
    return np.array([[block_ratio(O, om, g, s) for s in range(N_T)] for g in gaits])


def lifted_runs(O, omodels, omodels32):
    """LIFTED_CASES: per case (name, gait, tau [20][nmj], r64, r32)"""
    out = []
    for name, g in LIFTED_CASES(O):
        tau = perturbed_tau(O, omodels[name], [g])[0]
        out.append((name, g, tau, O.forces(omodels[name], g, tau, N_T), O.forces(omodels32[name], g, tau, N_T)))
    return out


@pytest.fixture(scope="module")
def runs(oracle_mod, omodels, omodels32):
    """(name, kind) -> both builds' forces on the input set; computed once, read only"""
    return {(n, k): both_builds(oracle_mod, omodels[n], omodels32[n], gait_inputs(n, k)) for n in NAMES for k in KINDS}


@pytest.fixture(scope="module")
def lifted(oracle_mod, omodels, omodels32):
    return lifted_runs(oracle_mod, omodels, omodels32)


def test_forces_run_on_the_models_build(oracle_mod, omodels, omodels32):
    """forces and forces_batch call the build that owns the model with inputs of its precision: the
    single-precision build returns float values and is handed float torques and gaits, so torques that are
    no float values give what their rounded values give; the one-rollout and the batch form agree bitwise"""
    O = oracle_mod
    g = record_to_oracle_gait(O, gait_inputs("hexapod", "straight")[3])
    tau = perturbed_tau(O, omodels["hexapod"], [g])[0]
    a, b = O.forces(omodels32["hexapod"], g, tau + 1e-9, N_T), O.forces(omodels32["hexapod"], g, tau, N_T)
    assert np.array_equal(a["cf"], b["cf"]) and np.array_equal(f32(a["cf"]), a["cf"])
    c = O.forces_batch(omodels32["hexapod"], [g], tau[None], N_T)
    assert np.array_equal(c["cf"][0], b["cf"]) and np.array_equal(c["flags"][0], b["flags"])
    d = O.forces(omodels["hexapod"], g, tau, N_T)
    assert not np.array_equal(f32(d["cf"]), d["cf"]) and not np.array_equal(d["cf"], b["cf"])
    assert np.array_equal(O.forces_batch(omodels["hexapod"], [g], tau[None], N_T)["cf"][0], d["cf"])


@pytest.mark.parametrize("name", NAMES)
def test_f32_build_within_fp32_tol(runs, name):
    for kind in KINDS:
        _, tau, r64, r32 = runs[name, kind]
        assert np.isfinite(r32["cf"]).all() and np.isfinite(r64["cf"]).all()
        assert not (r64["flags"] & BAD).any() and not (r32["flags"] & BAD).any(), (name, kind)
        assert np.array_equal(r64["flags"], r32["flags"])
        sp = spread(r32["cf"], r64["cf"])
        print(f"{name} {kind}: f32 build vs fp64 build over {sp.size} steps: max {sp.max():.2e} median {np.median(sp):.2e}")
        assert 0 < sp.max() < FP32_TOL, (name, kind, sp.max())
        assert np.abs(r64["cf"]).max() > 1  # forces of order 1 and more: the bound is a relative one


def test_perturbed_torques_are_inconsistent(oracle_mod, omodels, runs):
    """the perturbation leaves the least squares a residual: the forces are not the control loop's own"""
    O = oracle_mod
    gaits, tau, r64, _ = runs["hexapod", "straight"]
    own = O.batch(omodels["hexapod"], gaits, N_T, 0, N_T, basis=O.BASIS_FAST, n_threads=8)
    assert np.abs(r64["cf"] - own["cf"]).max() > 0.05


def test_lifted_cases_both_builds(oracle_mod, omodels, lifted):
    """LIFTED_CASES: GENERAL | DEPENDENT exactly where a component is exactly 0, for both builds; the fp64
    build's flag values and counts; gamma of both builds' answers"""
    O = oracle_mod
    n592 = 0
    for name, g, tau, r64, r32 in lifted:
        lift = g.torso_pos[2]
        for what, r in (("fp64", r64), ("f32", r32)):
            assert np.isfinite(r["cf"]).all() and not (r["flags"] & 8).any()
            assert dependent_where_zero(r["cf"], r["flags"]), (name, lift, what)
            gm = gammas(O, omodels[name], g, tau, r["cf"])
            vals, counts = np.unique(r["flags"], return_counts=True)
            print(f"{name} lifted {lift}: {what} build flags {dict(zip(vals.tolist(), counts.tolist()))}, "
                  f"gamma max {gm.max():.2e}")
            assert gm.max() < (1e-12 if what == "fp64" else 1e-4)  # a least-squares solution over its kept columns
        n592 += int((r64["flags"] == CLEAN_DROP).sum())
        same = (dropped_set(r64["cf"]) == dropped_set(r32["cf"])).all(axis=-1)
        if same.any():
            print(f"  dropped sets equal on {int(same.sum())} of 20 steps: f32 vs fp64 "
                  f"{spread(r32['cf'], r64['cf'])[same].max():.2e}")
        if name == "myant":  # straight legs, B_f singular, the system of full rank
            assert (r64["flags"] == 16).all() and (r32["flags"] == 16).all()
            assert spread(r32["cf"], r64["cf"]).max() < FP32_TOL
    assert n592 >= 12


def test_gamma_is_first_order(oracle_mod, omodels, lifted):
    """the metric can fail: a 1 % error on one kept component shows at order 1e-3 and more"""
    O = oracle_mod
    name, g, tau, r64, _ = lifted[0]
    y = r64["cf"][5].copy()
    k = int(np.argmax(np.abs(y)))
    base = gamma(O, omodels[name], g, 5, tau[5], y)
    y[k] *= 1.01
    assert base < 1e-12 and gamma(O, omodels[name], g, 5, tau[5], y) > 1e-4


def test_block_ratio_on_known_legs(oracle_mod, omodels, lifted):
    """the routing ratio where the answer is known: a leg clamped straight has a singular B_f (the force along it
    meets no motor), the spider's bent legs are far from it; myant's ordinary gaits hold steps on both sides of
    the float guard, decided ones (what lets the GPU test pin the guard from both sides)"""
    O = oracle_mod
    for name, g, _, _, _ in lifted:
        assert max(block_ratio(O, omodels[name], g, s) for s in (0, 7, 13)) < 1e-12
    spider = [record_to_oracle_gait(O, r) for r in gait_inputs("spider", "straight")[:4]]
    assert block_ratios(O, omodels["spider"], spider).min() > 0.1
    myant = [record_to_oracle_gait(O, r) for r in gait_inputs("myant", "straight")[:48]]
    rho = block_ratios(O, omodels["myant"], myant)
    fast, dense = rho > FORCES_BLOCK_GUARD_F32 * ROUTE_BAND, rho < FORCES_BLOCK_GUARD_F32 / ROUTE_BAND
    print(f"myant straight: {int(fast.sum())} steps decided for the 6 x 6 route, {int(dense.sum())} for the dense one, "
          f"{int((~fast & ~dense).sum())} undecided; {int((fast & (rho < 0.1)).sum())} of the first under 0.1, "
          f"{int((dense & (rho > 1e-5)).sum())} of the second over 1e-5")
    assert (fast & (rho < 0.1)).sum() >= 100 and (dense & (rho > 1e-5)).sum() >= 4
