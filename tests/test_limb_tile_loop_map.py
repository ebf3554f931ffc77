"""The tile loop's chunk arithmetic (hslabs_amd/csrc/hs_limb_tile.h: limb_tile_chunks, limb_tile_chunk_first,
limb_tile_chunk_end), plain C++ that the launcher, the kernel and this test compile. A tile-mapped launch of
nt = limb_tile_count(n) tiles at TL tiles per wavefront runs ceil(nt / TL) chunks per rollout; chunk c runs
tiles c TL .. min((c + 1) TL, nt) - 1 in order. Every tile is run by exactly one chunk, the chunks in order
cover the tiles in order, no chunk is empty, and TL = 1 is the identity (chunk c = tile c)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = list(range(1, 65)) + [200, 250, 256]
TLS = list(range(1, 33))

rules = {}  # (launch steps, rollouts) -> tiles per wavefront under the routing rule (filled by chunk_table)

PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "hs_limb_tile.h"
int main(int argc, char** argv) {
  const int tl_max = atoi(argv[1]);
  for (int i = 2; i < argc; i++) {
    const int n = atoi(argv[i]), nt = limb_tile_count(n);
    for (int tl = 1; tl <= tl_max; tl++) {
      const int nc = limb_tile_chunks(nt, tl);
      printf("%d %d %d %d", n, tl, nt, nc);
      for (int c = 0; c < nc; c++) printf(" %d %d", limb_tile_chunk_first(c, tl), limb_tile_chunk_end(c, tl, nt));
      printf("\n");
    }
  }
  // the routing rule's arithmetic at the library's constants: 5 tiles, a queue of 4 x 2,048 wavefronts
  const int rule[][2] = {{200, 4096}, {64, 4096}, {40, 4096}, {200, 5000}, {200, 2048}, {200, 1024}, {200, 400},
                         {200, 13}, {8, 1 << 20}, {250, 4096}, {256, 4096}};
  for (const auto& r : rule) printf("rule %d %d %d\n", r[0], r[1], limb_tile_loop_rule(limb_tile_count(r[0]), r[1], 5, 4 * 2048));
  // a tile count below 1 per wavefront counts as 1
  printf("low %d %d %d %d\n", limb_tile_chunks(25, 0), limb_tile_chunks(25, -3), limb_tile_chunk_first(7, 0),
         limb_tile_chunk_end(7, -1, 25));
  return 0;
}
"""


@pytest.fixture(scope="module")
def chunk_table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("tile_loop_map")
    src = d / "map.cpp"
    src.write_text(PROG)
    exe = d / "map"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hslabs_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(TLS[-1]), *map(str, NS)], check=True, capture_output=True, text=True,
                         timeout=60).stdout
    table, low = {}, None
    rules.clear()
    for line in out.splitlines():
        if line.startswith("rule"):
            n, b, tl = map(int, line.split()[1:])
            rules[(n, b)] = tl
            continue
        if line.startswith("low"):
            low = list(map(int, line.split()[1:]))
            continue
        v = list(map(int, line.split()))
        table[(v[0], v[1])] = (v[2], v[3], list(zip(v[4::2], v[5::2])))
    assert sorted(table) == [(n, tl) for n in NS for tl in TLS]
    return table, low


@pytest.mark.parametrize("n", NS)
def test_every_tile_in_exactly_one_chunk_in_order(chunk_table, n):
    table, _ = chunk_table
    for tl in TLS:
        nt, nc, chunks = table[(n, tl)]
        assert nt == (n + 7) // 8 and nc == (nt + tl - 1) // tl == len(chunks), (n, tl)
        tiles = [t for first, end in chunks for t in range(first, end)]
        assert tiles == list(range(nt)), (n, tl)
        assert all(1 <= end - first <= tl for first, end in chunks), (n, tl)
        assert all(end - first == tl for first, end in chunks[:-1]), (n, tl)  # only the last chunk is short


@pytest.mark.parametrize("n", NS)
def test_one_tile_per_wavefront_is_the_identity(chunk_table, n):
    table, _ = chunk_table
    nt, nc, chunks = table[(n, 1)]
    assert nc == nt and chunks == [(t, t + 1) for t in range(nt)]


def test_a_count_below_one_counts_as_one(chunk_table):
    _, low = chunk_table
    assert low == [25, 25, 7, 8]


def test_routing_rule_arithmetic(chunk_table):
    """limb_tile_loop_rule at the library's constants (5 tiles per wavefront, at least 4 rounds of 2,048
    wavefronts in the launch's queue, the tiles spread evenly over the chunks): the benchmark's shapes and the
    batches at which the bound bites"""
    want = {(200, 4096): 5,   # 25 tiles in 5 chunks: 20,480 wavefronts
            (64, 4096): 4,    # 8 tiles: 5 per wavefront would leave 2 chunks of 5 + 3, evened to 4 + 4
            (40, 4096): 3,    # 5 tiles: 2 chunks, 3 + 2
            (200, 5000): 5,
            (200, 2048): 5,   # 5 chunks x 2048 = 10,240 >= 8,192
            (200, 1024): 3,   # 9 chunks of 3 (the last of 1): 9,216
            (200, 400): 1,    # 25 x 400 = 10,000 only at a tile per wavefront
            (200, 13): 1,
            (8, 1 << 20): 1,  # one tile
            (250, 4096): 5,   # 32 tiles: 7 chunks, evened from 5 to ceil(32 / 7) = 5
            (256, 4096): 5}
    assert rules == want
