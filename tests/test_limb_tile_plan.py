"""The tile planner of the limb-lane kernel's tile mapping (hslabs_amd/csrc/hs_limb_tile.h, limb_tile_plan): a
launch's steps cut into chains whose table rows ascend by 2, every run of 8 a tile of its own, the remainders
packed into the remaining tiles; kept only where it needs fewer further FK passes than the parity order.

The header is compiled into a small program (as test_limb_tile_map.py does) that prints, per launch, the
planner's sequence, whether it is the chain-aligned one, and the header's pass counts of it and of the parity
order. This test replays the kernel's request rule (limb_tile_kd) in Python on its own."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = list(range(1, 65)) + [200, 250, 256]
S0S = [0, 256]
CALLS = [(1, 0, 20), (1, 13, 20), (5, 0, 20), (3, 5, 20), (32, 0, 20), (1, 0, 21), (1, 0, 70)]  # (h, k0, n_t)
LIMBS = [4, 6]
CASES = list(itertools.product(NS, S0S, CALLS, LIMBS))

PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "hs_limb_tile.h"
int main(int argc, char** argv) {
  for (int i = 1; i + 5 < argc; i += 6) {
    limb_tile_launch L;
    L.n = atoi(argv[i]), L.s0 = atoi(argv[i + 1]), L.h = atoi(argv[i + 2]), L.k0 = atoi(argv[i + 3]);
    L.n_t = atoi(argv[i + 4]), L.n_limbs = atoi(argv[i + 5]);
    int16_t step[HS_TILE_PLAN_STEPS], par[HS_TILE_PLAN_STEPS];
    int passes = -1, parity = -1;
    const bool planned = limb_tile_plan(L, step, &passes, &parity);
    limb_tile_parity_fill(L.n, par);
    printf("%d %d %d %d %d %d  %d %d %d %d %d", L.n, L.s0, L.h, L.k0, L.n_t, L.n_limbs, (int)planned, passes, parity,
           limb_tile_passes(L, step), limb_tile_passes(L, par));
    for (int s = 0; s < HS_TILE_SLOTS * limb_tile_count(L.n); s++) printf(" %d", step[s]);
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("tile_plan")
    src = d / "plan.cpp"
    src.write_text(PROG)
    exe = d / "plan"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hslabs_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    args = [str(v) for (n, s0, (h, k0, n_t), nl) in CASES for v in (n, s0, h, k0, n_t, nl)]
    out = subprocess.run([str(exe), *args], check=True, capture_output=True, text=True, timeout=60).stdout
    table = {}
    for line in out.splitlines():
        v = list(map(int, line.split()))
        n, s0, h, k0, n_t, nl = v[:6]
        table[(n, s0, (h, k0, n_t), nl)] = dict(planned=bool(v[6]), passes=v[7], parity=v[8], cost_step=v[9],
                                                cost_parity=v[10], step=v[11:])
    assert sorted(table) == sorted(CASES)
    return table


# ---- an independent replay of the kernel's arithmetic ----
def row(step, s0, h, k0, n_t):
    """hs_limb_kernel's table row of a local step (less the constant ktab_lo)"""
    s_glob = s0 + step
    call = s_glob // h
    return (k0 + call * h) % n_t + s_glob % h


def requests(tile, s0, call):
    """limb_tile_kd's requests of one tile: the minus row of a live slot is shared with the live slot before it
    when that one's row is exactly 2 lower, its plus row with the live slot after it when 2 higher"""
    rows = [row(s, s0, *call) if s >= 0 else None for s in tile]
    req = 0
    for g, r in enumerate(rows):
        if r is None:
            continue
        shm = g > 0 and rows[g - 1] is not None and rows[g - 1] + 2 == r
        shp = g < 7 and rows[g + 1] is not None and rows[g + 1] == r + 2
        req += (not shm) + (not shp)
    return req


def passes(slots, s0, call, nl):
    e0 = (8 * (8 - nl)) // nl
    return sum(-(-max(0, requests(slots[t:t + 8], s0, call) - e0) // 8) for t in range(0, len(slots), 8))


def parity_order(n):
    seq = list(range(0, n, 2)) + list(range(1, n, 2))
    return seq + [-1] * (8 * ((n + 7) // 8) - n)


def test_the_grid_is_the_issues():
    assert len(CASES) == 1876


@pytest.mark.parametrize("nl", LIMBS)
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("s0", S0S)
def test_invariants(plans, s0, call, nl):
    for n in NS:
        slots = plans[(n, s0, call, nl)]["step"]
        tiles = (n + 7) // 8
        assert len(slots) == 8 * tiles, n                                  # exactly limb_tile_count(n) tiles
        assert sorted(s for s in slots if s >= 0) == list(range(n)), n     # every step in exactly one slot
        assert all(s >= -1 for s in slots), n
        assert all(s >= 0 for s in slots[:n]) and all(s == -1 for s in slots[n:]), n  # idle: the last tile's end
        assert all(slots[8 * t] >= 0 for t in range(tiles)), n             # slot 0 of every tile is live


@pytest.mark.parametrize("nl", LIMBS)
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("s0", S0S)
def test_cost_function_equals_the_replay_and_never_worse(plans, s0, call, nl):
    for n in NS:
        p = plans[(n, s0, call, nl)]
        want_parity = passes(parity_order(n), s0, call, nl)
        want = passes(p["step"], s0, call, nl)
        assert p["cost_parity"] == want_parity == p["parity"], n
        assert p["cost_step"] == want == p["passes"], n
        assert want <= want_parity, n
        assert p["planned"] == (want < want_parity), n  # the parity order unless the plan needs fewer passes
        if not p["planned"]:
            assert p["step"] == parity_order(n), n


def test_strictly_better_somewhere_and_never_for_four_limbs(plans):
    better = sum(p["planned"] for p in plans.values())
    print("planned in", better, "of", len(plans))
    assert better > 0
    # E0 = 8 with four limbs: the parity order's one break per tile at most (6 requests) never takes a pass
    for (n, s0, call, nl), p in plans.items():
        if nl == 4 and call[2] == 20 and call[0] == 1:
            assert p["parity"] == 0 and not p["planned"]


@pytest.mark.parametrize("n,parity,planned", [(200, 15, 5), (40, 3, 1), (64, 6, 2), (256, 18, 6)])
def test_hexapod_pass_counts(plans, n, parity, planned):
    p = plans[(n, 0, (1, 0, 20), 6)]
    assert (p["parity"], p["passes"], p["planned"]) == (parity, planned, True)
