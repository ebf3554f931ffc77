"""The joint rates and range bits the preparation pass tabulates per table row (hslabs_amd/csrc: RolloutWS::kvel and
kbig, written by hs_prep_kernel beside ktab and kbad; read by the limb kernel's tile loop, limb_tile_kd, in place
of five ktab rows, nine range tests and three wrapped differences per tile).

A table says where a value comes from, never the value. So tau, cf, flags, work_cot and the best key are BITWISE
the same on the product's route (no switch set), on the tile route at HS_LIMB_TILE_LOOP = 1, 2 and 5, on the packed
mapping (HS_LIMB_TILE=0) and on hs_rollout_kernel (HS_LIMB=0), neither of which reads the new tables, and as many
steps are deferred (limb_deferred) as by the packed mapping. The tables themselves are read back
(hs_debug_limb_tables) and held bit for bit to wrap_rate and sincos_big restated in numpy float64 on the ktab rows
read back with them: a subtraction, two additions of 2 pi, two compares and a division by 2 dt, nothing a compiler
could contract."""
import numpy as np
import pytest

from conftest import transformed
import limb_gpu_kit as kit
from limb_gpu_kit import PACKED, ROLLOUT, TILE, gpu, hmodels, product_route  # noqa: F401

pytestmark = pytest.mark.gpu

TLS = (1, 2, 5)
NS = 5  # samples of the derivative stencil


def table_rows(K, Hc=1, k0=0, n_t=20):
    """hs::ktab_range: the samples [lo, lo + n) that K calls of Hc steps from k0 read"""
    first = [(k0 + c * Hc) % n_t for c in range(min(K, n_t))]
    lo = min(first)
    return lo, max(first) + Hc + NS - 1 - lo


def check(go, what, tile=True, product_tile=True):
    """go(switches) on the product's route and on the tile route at every TL against the packed mapping and
    hs_rollout_kernel (tile: the call keeps a table, so the forced runs take the tile route; product_tile: so does
    the product's rule, a launch of 40 steps or more)"""
    packed, rollout = go(PACKED), go(ROLLOUT)
    assert packed["tile_launches"] == 0 and rollout["limb_launches"] == 0, what
    kit.same(packed, rollout, f"{what}: packed / HS_LIMB=0")
    runs = {"product": go(product_route())}
    for tl in TLS:
        runs[tl] = go(dict(TILE, HS_LIMB_TILE_LOOP=str(tl)))
    for name, r in runs.items():
        if tile and (product_tile or name != "product"):
            assert r["tile_launches"] > 0, f"{what} {name}: not the tile route"
        if tile and name in (2, 5):
            assert r["loop_launches"] == r["tile_launches"], f"{what} TL={name}: not the tile loop"
        kit.same(r, packed, f"{what}: {name} / packed", deferred=True)
        kit.same(r, rollout, f"{what}: {name} / HS_LIMB=0")
    return runs, packed


def check_batch(gpu, model, params, what, tile=True, product_tile=True, **kw):
    kw.setdefault("K", 40)
    return check(lambda sw: kit.run(gpu, model, params, sw, **kw), what, tile, product_tile)


def wrap_rate(qp, qm, dt):
    """hs_step_kin.h's, in float64"""
    dd = qp - qm
    lo, hi = dd - 2 * np.pi, dd + 2 * np.pi
    with np.errstate(invalid="ignore"):
        return np.where(dd > np.pi, lo, np.where(dd < -np.pi, hi, dd)) / (2 * dt)


def check_tables(gpu, model, rollouts, n, what):
    """the tables the last call left for `rollouts`: kbig on every row of the call's n, kvel on rows 1 .. n - 2"""
    nl = model.n_limbs
    bits = 0
    for b in rollouts:
        t = gpu.api.limb_tables(model, b, n)
        q, dt = t["ktab"][:, :nl], t["dt"]
        assert dt > 0, f"{what}: rollout {b}'s setup record was not written"
        with np.errstate(invalid="ignore"):
            big = (~(np.abs(q) < 2.0 ** 20)).any(axis=2)
        assert np.array_equal(t["kbig"][:, :nl] != 0, big), f"{what}: rollout {b}'s kbig"
        want, got = wrap_rate(q[2:], q[:-2], dt), t["kvel"][1:n - 1, :nl]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: rollout {b}'s kvel, the entries that are not numbers"
        assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), \
            f"{what}: rollout {b}'s kvel differs on {int((got[~nan] != want[~nan]).sum())} of {got.size} entries"
        bits += int(big.sum())
    return bits


def test_straight_and_its_tables(gpu, hmodels):
    """hexapod, B = 9 (the second batch wavefront holds one live rollout), 40 steps, n_t = 20: 24 rows in five
    chunks, every chunk's neighbours lanes of its wavefront; the steps' centre rows run from row 2 to row 21,
    the first and the last row that has a kvel row on either side"""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(9, "hexapod", id0=4321)
    lo, n = table_rows(40)
    assert (lo, n) == (0, 24)
    runs, _ = check_batch(gpu, m, p, "hexapod B=9 K=40")
    assert np.isfinite(runs[5]["tau"]).all()
    assert check_tables(gpu, m, (0, 4, 8), n, "hexapod B=9 K=40") == 0


def test_one_period_is_the_whole_interior(gpu, hmodels):
    """20 steps of n_t = 20 from k0 = 7: the call's rows are samples [0, 24) again, and the 20 steps' centre rows
    are exactly the interior rows lo + 2 .. lo + n - 3, each read once (the product's rule keeps a launch of 20
    steps packed; the forced runs read the tables)"""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(9, "hexapod", id0=31)
    check_batch(gpu, m, p, "hexapod B=9 K=20 k0=7", product_tile=False, K=20, k0=7)
    check_tables(gpu, m, (0, 8), 24, "hexapod B=9 K=20 k0=7")


def test_rows_wrap(gpu, hmodels):
    """calls of H = 4 steps from k0 = 13: the rows advance within a call, jump between calls and wrap with the
    period inside tiles"""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(9, "hexapod", id0=31)
    check_batch(gpu, m, p, "hexapod B=9 H=4 K=10 k0=13", K=10, Hc=4, k0=13)
    check_tables(gpu, m, (0, 8), table_rows(10, 4, 13)[1], "hexapod H=4 k0=13")


def test_calls_of_two_steps(gpu, hmodels):
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=77)
    check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 H=2 K=20", K=20, Hc=2)


def test_last_rows_and_halo_rows(gpu, hmodels):
    """n_t = 56, a whole period of 56 steps from k0 = 13: 60 rows in twelve chunks over wavefronts of ten lane
    groups, so chunks have their neighbours in another wavefront and compute those rows themselves; the tile loop
    reads kvel up to row 57"""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(9, "hexapod", id0=4321)
    lo, n = table_rows(56, 1, 13, 56)
    assert (lo, n) == (0, 60)
    check_batch(gpu, m, p, "hexapod B=9 K=56 n_t=56", K=56, k0=13, n_t=56)
    check_tables(gpu, m, range(9), n, "hexapod B=9 K=56 n_t=56")


def test_curved(gpu, hmodels):
    """turning gaits: the two-pass rows of the preparation pass, whose joint values take the targets' place in LDS"""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(9, "hexapod", id0=5, curved=True)
    check_batch(gpu, m, p, "hexapod curved B=9 K=40")
    check_tables(gpu, m, (0, 4, 8), 24, "hexapod curved")
    check_batch(gpu, m, p, "hexapod curved B=9 K=56 n_t=56", K=56, k0=13, n_t=56)
    check_tables(gpu, m, range(9), 60, "hexapod curved n_t=56")


def test_transformed_record(gpu, hmodels):
    """transformed records beside plain ones: lanes of both row loops in one wavefront of the preparation pass"""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p, on = transformed(synth.gen_params(9, "hexapod", id0=900), np.random.default_rng(17), tilt=0.05)
    assert on.any() and not on.all()
    check_batch(gpu, m, p, "hexapod transformed B=9 K=40")
    check_tables(gpu, m, range(9), 24, "hexapod transformed")
    check_batch(gpu, m, p, "hexapod transformed B=9 K=56 n_t=56", K=56, k0=13, n_t=56)
    check_tables(gpu, m, range(9), 60, "hexapod transformed n_t=56")


def test_myant_defers_inside_a_chunk(gpu, hmodels):
    """four limbs (sixteen lane groups per wavefront of the preparation pass), ids 4719 .. 4727: tier-2 deferrals
    in tiles that are not the chunk's last, and the same steps deferred"""
    from hslabs_amd import synth

    m = hmodels["myant"]
    p = synth.gen_params(9, "myant", id0=4719)
    runs, packed = check_batch(gpu, m, p, "myant B=9 K=40")
    print(f"myant: {packed['deferred']} steps deferred (packed), {runs[5]['deferred']} (TL=5)")
    assert packed["deferred"] > 0
    check_tables(gpu, m, (0, 8), 24, "myant")


def test_mixed_plan(gpu, hmodels):
    """myant + hexapod, B = 16: lane groups of different models in one wavefront of the preparation pass"""
    from hslabs_amd import synth

    params, idx = synth.gen_mixed(16)
    assert set(idx.tolist()) == {0, 1}
    ms = [hmodels[n] for n in synth.MIXED_MODELS]
    runs, _ = check(lambda sw: kit.run_mixed(gpu, ms, idx, params, sw, 40), "mixed B=16 K=40")
    assert np.isfinite(runs[5]["tau"]).all() and np.isfinite(runs[5]["cf"]).all()


def test_two_launches(gpu, hmodels):
    """300 steps on one batch: a launch of 256 steps and one of 44, both reading the one call's tables (the
    product's rule keeps the second packed: its last tile would be half empty)"""
    from hslabs_amd import synth

    p = synth.gen_params(9, "hexapod", id0=77)
    runs, _ = check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 K=300", K=300)
    assert all(runs[tl]["tile_launches"] == 2 for tl in TLS) and runs["product"]["tile_launches"] == 1


def test_past_the_table(gpu, hmodels):
    """64 steps of n_t = 64: 68 samples, past the table's 64 rows, so the call keeps no table and no route reads
    one (the steps compute their kinematics inline): the same outputs under every switch"""
    from hslabs_amd import synth

    assert table_rows(64, 1, 0, 64)[1] == 68
    p = synth.gen_params(9, "hexapod", id0=4321)
    runs, _ = check_batch(gpu, hmodels["hexapod"], p, "hexapod B=9 K=64 n_t=64", tile=False, K=64, n_t=64)
    assert all(r["limb_launches"] == 0 for r in runs.values())


def test_not_a_number_gait(gpu, hmodels):
    """The route from a set kbig bit to a deferred step. A limb's joint values are the IK's atan2 and acos
    results, at most pi in size, so no gait record holds a finite joint value of 2^20 or more; one that is not a
    number takes the same route, and a step height that is not a number gives such rows (on the CPU, the oracle's
    set_jvalues_with_lik of that gait's record returns every limb joint as NaN, and its rollout ends with
    HS_FLAG_NAN). Rollouts 2 and 6 get such a step height: their kbig bits are set, kbig is sincos_big of the
    rows on every rollout, every route defers the same steps and stores the same outputs, and the other
    rollouts' outputs are those of the batch without the two."""
    from hslabs_amd import synth

    m = hmodels["hexapod"]
    p = synth.gen_params(9, "hexapod", id0=4321)
    clean, _ = check_batch(gpu, m, p, "hexapod B=9 K=40")
    q = p.copy()
    q["step_height"][[2, 6]] = np.nan
    runs, packed = check_batch(gpu, m, q, "hexapod B=9 K=40, two gaits not a number")
    bits = check_tables(gpu, m, range(9), 24, "two gaits not a number")
    print(f"not-a-number gaits: {bits} kbig bits set, {packed['deferred']} steps deferred (packed), "
          f"{runs[5]['deferred']} (TL=5)")
    assert bits > 0 and runs[5]["deferred"] > 0
    keep = [b for b in range(9) if b not in (2, 6)]
    for k in ("tau", "cf", "flags"):
        assert np.array_equal(runs[5][k][keep], clean[5][k][keep], equal_nan=True), k
