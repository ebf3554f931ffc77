"""The slot sequence of the limb-lane kernel's tile mapping (hslabs_amd/csrc/hs_limb_tile.h): a plain C++
header that host code, device code and this test compile. A launch of n local steps gives a rollout the
slots: all even steps ascending, then all odd ones; tile t is slots 8 t .. 8 t + 7."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = list(range(1, 41)) + [200, 256, 300]

PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "hs_limb_tile.h"
int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    const int n = atoi(argv[i]);
    printf("%d %d", n, limb_tile_count(n));
    for (int s = 0; s < HS_TILE_SLOTS * limb_tile_count(n); s++) printf(" %d", limb_tile_step(s, n));
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def slot_table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("tile_map")
    src = d / "map.cpp"
    src.write_text(PROG)
    exe = d / "map"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hslabs_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), *map(str, NS)], check=True, capture_output=True, text=True, timeout=60).stdout
    table = {}
    for line in out.splitlines():
        v = list(map(int, line.split()))
        table[v[0]] = (v[1], v[2:])
    assert sorted(table) == NS
    return table


@pytest.mark.parametrize("n", NS)
def test_every_step_in_exactly_one_slot(slot_table, n):
    tiles, slots = slot_table[n]
    assert tiles == (n + 7) // 8 and len(slots) == 8 * tiles
    assert sorted(s for s in slots if s >= 0) == list(range(n))
    assert all(s >= -1 for s in slots)


@pytest.mark.parametrize("n", NS)
def test_idle_slots_only_in_the_last_tile(slot_table, n):
    tiles, slots = slot_table[n]
    for t in range(tiles - 1):
        assert all(s >= 0 for s in slots[8 * t:8 * t + 8])
    last = slots[8 * (tiles - 1):]
    live = [s >= 0 for s in last]
    assert live[0] and live == sorted(live, reverse=True)  # the live groups first, then the idle ones


@pytest.mark.parametrize("n", NS)
def test_neighbours_two_steps_apart_but_for_the_parity_switch(slot_table, n):
    tiles, slots = slot_table[n]
    switches = 0
    for t in range(tiles):
        live = [s for s in slots[8 * t:8 * t + 8] if s >= 0]
        for a, b in zip(live, live[1:]):
            if b - a != 2:
                assert a % 2 == 0 and b == 1, (n, t, a, b)  # the last even step, then step 1
                switches += 1
    assert switches <= 1
