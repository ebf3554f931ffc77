"""The fp32 build of solve_forces (forces_solve in hslabs_amd/csrc/hs_step_solve.h through hs_run_forces and
hs_run_forces_calls with HS_PREC_F32) against the oracle, one step at a time, bounded by the oracle's own
single-precision build (oracle/hs_oracle_f32.cpp; tests/test_forces_oracle_f32.py makes it trustworthy for
forces and holds the inputs and helpers).

Shape. Per model (hexapod, spider, myant) and gait kind (straight, curved, stretched: test_forces_oracle_f32.
gait_inputs, the first 48 rollouts) one batch of B = 48, n_t = 20, k0 = 0, H = 20; tau_in is the fp64 oracle's
torques + 0.25 cos(step + motor) rounded to float and uploaded as it is, so the least squares is inconsistent.
Runs, all float: hs_run_forces in HS_SOLVE_AUTO and in HS_SOLVE_REFERENCE (every step through the dense normal
equations), hs_run_forces_calls with 20 calls of H = 1 (bitwise the first), and params[:47] (an idle half-wavefront).

Bound (held). No step is excluded: neither the fp64 oracle nor the kernel flags GENERAL, DEPENDENT, NEAR_RANK or
NAN, the kernel's flags are the fp64 oracle's, and |kernel - f64 oracle| <= 4 x spread on every step, relative to
max(1, max |f|) of the step, spread = the largest |f32 oracle - f64 oracle| over the case's steps, computed here
from the same inputs (the project's hold_to_oracles rule; never measured against the kernel).

Route. HS_SOLVE_AUTO sets no flag that says which route a step took, so the test restates what routes it: the
smallest LDL^T pivot of a foot's block B_f over its largest diagonal (test_forces_oracle_f32.block_ratio, from
the oracle's dynamics record). Steps whose ratio is above 2 x the float kForcesBlockGuard (1e-3) took the 6 x 6
route and must differ from REFERENCE in a bit; steps under half of it took the dense route and must have
REFERENCE's bits. hexapod and myant have decided steps on both sides of a guard 100 times larger, myant of one
100 times smaller.

Measured on MI355X (profiles/forces_f32_oracle.txt holds every printed line), kernel vs f64 oracle as a multiple
of the spread, AUTO / REFERENCE, and the steps decided for the 6 x 6 route / the dense route / undecided:
  hexapod  straight 1.29 / 1.29 (spread 3.6e-6)  curved 1.00 / 1.00 (3.4e-5)  stretched 1.03 / 1.02 (7.4e-6)   960 / 0 / 0, 960 / 0 / 0, 940 / 20 / 0
  spider   straight 1.01 / 1.02 (9.6e-6)         curved 1.01 / 1.01 (2.5e-5)  stretched 1.08 / 1.09 (9.6e-6)   960 / 0 / 0 each
  myant    straight 0.76 / 0.76 (1.2e-5)         curved 1.00 / 1.00 (1.6e-5)  stretched 0.56 / 0.56 (9.4e-6)   904 / 48 / 8, 904 / 48 / 8, 648 / 308 / 4
Every decided step took its route (AUTO and REFERENCE differ in a bit on 960, 960, 940; 960 x 3; 912, 912, 650 steps).
  myant lifted to 1.2 (every B_f singular, full rank)      1.02 / 1.02 (spread 7.1e-6 over its 20 steps), AUTO with
      REFERENCE's bits; the ordinary rollouts of the batch 0.67 / 0.67
  hexapod lifted to 1.5 and 1.0 (components dropped)       the f32 oracle's dropped set on 40 of 40 steps (14 of them
      without NEAR_RANK), gamma 6.6e-7 = 0.91 x the f32 oracle's 7.2e-7, forces vs the f32 oracle 4.9e-5 = 0.65 x the
      oracle builds' 7.5e-5 (taken over the 16 steps where the two builds drop the same components)

What these tests found. Before forces_solve's dense route took its corrected-semi-normal-
equations step, it missed the bound wherever a foot block is near singular (a nearly straight leg): the normal
equations' error is cond(N) eps, the oracle builds' Householder QR's sqrt(cond(N)) eps, and the spread is theirs.
Then: myant stretched 6.78 x (rollout 10, steps 8 and 18, cond(N) 3.3e3, dense route in both modes), myant lifted
to 1.2 20.76 x (12 of 20 steps over 4 x), the hexapod's dropped steps 62.4 x (cond(N) of the kept columns up to 1e5).
"""
import numpy as np
import pytest

from conftest import record_to_oracle_gait
from forces_gpu_kit import kernel_forces, lifted_batch
from limb_gpu_kit import gpu, hmodels  # noqa: F401
from test_forces_oracle_f32 import (BAD, FORCES_BLOCK_GUARD_F32, KINDS, N_T, NAMES, ROUTE_BAND, block_ratios,
                                    dependent_where_zero, dropped_set, gait_inputs, gammas, omodels32, perturbed_tau,
                                    spread)  # noqa: F401

pytestmark = pytest.mark.gpu

B = 48
FACTOR = 4.0  # the project's hold_to_oracles rule: |kernel - f64 oracle| <= 4 x the largest |f32 oracle - f64 oracle|


def held(what, kern, r64, r32, rows=slice(None)):
    """the rule of the plain cases on the rollouts `rows`: nobody flags GENERAL, DEPENDENT, NEAR_RANK or NAN, the
    kernel's flags are the fp64 oracle's, and on every step |kernel - f64 oracle| <= FACTOR x the largest
    |f32 oracle - f64 oracle| over these steps, relative to max(1, max |f|) of the step. Prints the kernel's
    multiple of the spread; returns what does not hold (a test asserts that it is empty once every line of it is printed)"""
    k, a, b = kern["cf"][rows], r64["cf"][rows], r32["cf"][rows]
    assert not (r64["flags"][rows] & BAD).any(), what
    fails = []
    if (kern["flags"][rows] & BAD).any() or not np.array_equal(kern["flags"][rows], r64["flags"][rows]):
        fails.append((what, "flags", np.unique(kern["flags"][rows]).tolist(), np.unique(r64["flags"][rows]).tolist()))
    if not np.isfinite(k).all():
        fails.append((what, "not finite"))
    sp = float(spread(b, a).max())
    dev = spread(k, a)
    worst = np.unravel_index(int(np.nanargmax(dev)), dev.shape)
    print(f"{what}: spread {sp:.2e} over {dev.size} steps, kernel vs f64 oracle {dev.max():.2e} = {dev.max() / sp:.2f} x "
          f"(rollout, step {tuple(int(i) for i in worst)}; {int((dev > FACTOR * sp).sum())} steps over {FACTOR:g} x), "
          f"kernel vs f32 oracle {spread(k, b).max():.2e}")
    assert sp > 0
    if not dev.max() <= FACTOR * sp:
        fails.append((what, f"{dev.max() / sp:.2f} x the spread {sp:.2e}"))
    return fails


@pytest.fixture(scope="module")
def oracle_runs(oracle_mod, omodels, omodels32):
    """(name, kind) -> (params, tau, r64, r32, the steps' routing ratios) of the case's 48 rollouts; each computed
    once, read only"""
    O, cache = oracle_mod, {}

    def get(name, kind):
        if (name, kind) not in cache:
            params = gait_inputs(name, kind)[:B]
            gaits = [record_to_oracle_gait(O, r) for r in params]
            tau = perturbed_tau(O, omodels[name], gaits)
            cache[name, kind] = (params, tau, O.forces_batch(omodels[name], gaits, tau, N_T, n_threads=8),
                                 O.forces_batch(omodels32[name], gaits, tau, N_T, n_threads=8),
                                 block_ratios(O, omodels[name], gaits))
        return cache[name, kind]
    return get


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_fp32_forces_every_step(gpu, hmodels, oracle_runs, name, kind):
    """Both routes of forces_solve on every step of 48 rollouts x 20 steps: HS_SOLVE_AUTO (the 6 x 6 system after
    the limbs' block elimination wherever every B_f passes the float kForcesBlockGuard) and HS_SOLVE_REFERENCE
    (every step through the dense normal equations); the fused per-call form and the idle half-wavefront."""
    import torch

    params, tau, r64, r32, rho = oracle_runs(name, kind)
    m, f = hmodels[name], torch.float32
    auto = kernel_forces(gpu, m, params, tau, f, gpu.capi.HS_SOLVE_AUTO)
    dense = kernel_forces(gpu, m, params, tau, f, gpu.capi.HS_SOLVE_REFERENCE)
    calls = kernel_forces(gpu, m, params, tau, f, gpu.capi.HS_SOLVE_AUTO, calls=True)
    odd = kernel_forces(gpu, m, params[:B - 1], tau[:B - 1], f, gpu.capi.HS_SOLVE_AUTO)
    fails = held(f"{name} {kind} AUTO", auto, r64, r32)
    fails += held(f"{name} {kind} REFERENCE", dense, r64, r32)
    fails += held(f"{name} {kind} AUTO B = {B - 1}", odd, r64, r32, rows=slice(0, B - 1))
    # the route HS_SOLVE_AUTO took, which no flag tells: where every foot's block passes the float guard by
    # ROUTE_BAND (test_forces_oracle_f32.block_ratio) the step took the 6 x 6 route, another algorithm than
    # REFERENCE's, whose 3 nf floats it does not reproduce; where a block misses it by ROUTE_BAND the step took
    # REFERENCE's dense route and has its bits. A guard 100 times larger or smaller moves decided steps across
    differ = (auto["cf"] != dense["cf"]).any(axis=-1)
    fast, slow = rho > FORCES_BLOCK_GUARD_F32 * ROUTE_BAND, rho < FORCES_BLOCK_GUARD_F32 / ROUTE_BAND
    print(f"{name} {kind}: AUTO and REFERENCE differ in a bit on {int(differ.sum())} of {differ.size} steps; decided "
          f"for the 6 x 6 route {int(fast.sum())} ({int((fast & ~differ).sum())} of them with REFERENCE's bits), for the "
          f"dense route {int(slow.sum())} ({int((slow & differ).sum())} of them with other bits), undecided "
          f"{int((~fast & ~slow).sum())}")
    assert differ[fast].all() and not differ[slow].any()
    assert np.array_equal(calls["cf"], auto["cf"]) and np.array_equal(calls["flags"], auto["flags"])
    assert not fails, fails


def test_fp32_forces_singular_blocks_full_rank(gpu, hmodels, oracle_mod, omodels, omodels32):
    """myant lifted to 1.2 among ordinary rollouts: straight legs, every B_f singular and the system of full rank,
    so every one of its 20 steps takes the dense route in HS_SOLVE_AUTO too, drops nothing, and is held as the
    plain cases are, with the spread of those 20 steps"""
    import torch

    O = oracle_mod
    params, gaits, tau, rows = lifted_batch(O, omodels["myant"], "myant")
    r64 = O.forces_batch(omodels["myant"], gaits, tau, N_T)
    r32 = O.forces_batch(omodels32["myant"], gaits, tau, N_T)
    assert (r64["flags"][rows] == 16).all()
    plain = [b for b in range(len(params)) if b not in rows]
    auto = kernel_forces(gpu, hmodels["myant"], params, tau, torch.float32, gpu.capi.HS_SOLVE_AUTO)
    calls = kernel_forces(gpu, hmodels["myant"], params, tau, torch.float32, gpu.capi.HS_SOLVE_AUTO, calls=True)
    assert np.array_equal(calls["cf"], auto["cf"]) and np.array_equal(calls["flags"], auto["flags"])
    dense = kernel_forces(gpu, hmodels["myant"], params, tau, torch.float32, gpu.capi.HS_SOLVE_REFERENCE)
    fails = []
    for mode, k in (("AUTO", auto), ("REFERENCE", dense)):
        fails += held(f"myant lifted 1.2 {mode}", k, r64, r32, rows=rows)
        fails += held(f"myant lifted batch, the ordinary rollouts, {mode}", k, r64, r32, rows=plain)
    # every B_f of the lifted rollout is singular: HS_SOLVE_AUTO takes the dense route there, REFERENCE's bits
    assert np.array_equal(auto["cf"][rows], dense["cf"][rows])
    assert not fails, fails


def rank_deficient_run(gpu, hmodels, oracle_mod, omodels, omodels32):
    """the hexapod's lifted batch in fp32 and everything about it that holds; returns (the kernel's largest
    deviation from the f32 oracle where both drop the same components, the oracle builds' spread)"""
    import torch

    O, om = oracle_mod, omodels["hexapod"]
    params, gaits, tau, rows = lifted_batch(O, om, "hexapod")
    r64 = O.forces_batch(om, gaits, tau, N_T)
    r32 = O.forces_batch(omodels32["hexapod"], gaits, tau, N_T)
    kern = kernel_forces(gpu, hmodels["hexapod"], params, tau, torch.float32)
    calls = kernel_forces(gpu, hmodels["hexapod"], params, tau, torch.float32, calls=True)
    assert np.array_equal(calls["cf"], kern["cf"]) and np.array_equal(calls["flags"], kern["flags"])
    plain = [b for b in range(len(params)) if b not in rows]
    fails = held("hexapod lifted batch, the ordinary rollouts", kern, r64, r32, rows=plain)
    k, a, b = kern["cf"][rows], r64["cf"][rows], r32["cf"][rows]
    assert np.isfinite(k).all() and not (kern["flags"][rows] & 8).any()
    assert dependent_where_zero(k, kern["flags"][rows])
    assert dependent_where_zero(b, r32["flags"][rows])
    g_k = np.array([gammas(O, om, gaits[r], tau[r], kern["cf"][r]) for r in rows])
    g_o = np.array([gammas(O, om, gaits[r], tau[r], r32["cf"][r]) for r in rows])
    print(f"hexapod lifted fp32: gamma of the kernel's answers {g_k.max():.2e}, of the f32 oracle's {g_o.max():.2e} "
          f"({g_k.max() / g_o.max():.2f} x)")
    o_same = (dropped_set(b) == dropped_set(a)).all(axis=-1)  # the f32 oracle drops what the fp64 oracle drops
    k_same = (dropped_set(k) == dropped_set(b)).all(axis=-1)  # the kernel drops what the f32 oracle drops
    assert o_same.any()
    sp = float(spread(b, a)[o_same].max())
    dev = spread(k, b)
    print(f"hexapod lifted fp32: {k.shape[0] * k.shape[1]} steps, {int(dropped_set(k).any(axis=-1).sum())} drop a component; "
          f"kernel's dropped set = f32 oracle's on {int(k_same.sum())}, other on {int((~k_same).sum())}; f32 oracle's = "
          f"fp64 oracle's on {int(o_same.sum())}: spread {sp:.2e}; kernel vs f32 oracle where the sets agree "
          f"{(dev[k_same].max() if k_same.any() else 0.0):.2e} = {(dev[k_same].max() / sp if k_same.any() else 0.0):.2f} x "
          f"({int((dev[k_same] > FACTOR * sp).sum())} steps over {FACTOR:g} x)")
    # a rank decision the kernel does not flag as within 4 x of its guard is the oracle's (the project's fp64 rule,
    # with the f32 oracle, which carries the kernel's float guard, in the fp64 oracle's place)
    clear = (kern["flags"][rows] & 256) == 0
    print(f"hexapod lifted fp32: {int(clear.sum())} steps without HS_FLAG_NEAR_RANK, the f32 oracle's dropped set on "
          f"{int(k_same[clear].sum())} of them")
    assert g_k.max() <= FACTOR * g_o.max()
    assert clear.any() and k_same[clear].all()
    assert not fails, fails
    return dev[k_same].max(), sp


def test_fp32_forces_rank_deficient_steps(gpu, hmodels, oracle_mod, omodels, omodels32):
    """The hexapod lifted to 1.5 and to 1.0 among ordinary rollouts: chol_packed drops force components at the
    float guard. On every such step the answer is finite, flagged GENERAL | DEPENDENT exactly where a component
    is exactly 0, and a least-squares solution over its own kept columns (gamma within 4 x the f32 oracle's);
    the fused per-call form is bitwise the same; the ordinary rollouts of the batch are held as the plain cases."""
    rank_deficient_run(gpu, hmodels, oracle_mod, omodels, omodels32)


def test_fp32_forces_rank_deficient_steps_agree(gpu, hmodels, oracle_mod, omodels, omodels32):
    """The same steps, where the kernel drops the components the f32 oracle drops (the solution is not unique, so
    no parity is claimed elsewhere): forces within 4 x the f32 oracle's own spread against the fp64 oracle, that
    spread taken over the steps where the two oracle builds drop the same components."""
    dev, sp = rank_deficient_run(gpu, hmodels, oracle_mod, omodels, omodels32)
    assert dev <= FACTOR * sp, f"{dev / sp:.2f} x the spread {sp:.2e}"
