"""The tile descriptor of the limb-lane kernel's tile mapping (hslabs_amd/csrc/hs_limb_tile.h, limb_tile_desc_build):
per tile every slot's local step and table row, the request mask M and the requests in service order, built on
the host from the launch's slot sequence and read by the TILE kernels in place of their per-lane derivation.

The header is compiled into a small program (as test_limb_tile_plan.py does) that prints, per launch and for the
planner's sequence, the parity order and the forced chain order (limb_tile_desc_build's modes 1, 0 and 2), the
sequence as the sequence functions give it and the descriptor as the launch's one entry builds it. This test replays limb_tile_kd's rule in
Python on its own -- rows, sharing, requests, and which lane's FK provides which row in which pass -- and compares.
The same program is built once more with -fsanitize=address,undefined and run over the same grid (host only)."""
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
SEQS = ["plan", "parity", "chain"]  # limb_tile_desc_build's modes 1, 0 and 2

PROG = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hs_limb_tile.h"
int main(int argc, char** argv) {
  for (int i = 1; i + 5 < argc; i += 6) {
    limb_tile_launch L;
    L.n = atoi(argv[i]), L.s0 = atoi(argv[i + 1]), L.h = atoi(argv[i + 2]), L.k0 = atoi(argv[i + 3]);
    L.n_t = atoi(argv[i + 4]), L.n_limbs = atoi(argv[i + 5]);
    const int modes[3] = {1, 0, 2};  // limb_tile_desc_build's mode of each sequence
    for (int seq = 0; seq < 3; seq++) {
      int16_t step[HS_TILE_PLAN_STEPS];
      int row[HS_TILE_PLAN_STEPS];
      limb_tile_rows(L, row);
      bool chain = seq == 2;
      if (seq == 0) chain = limb_tile_plan(L, step);
      else if (seq == 1) limb_tile_parity_fill(L.n, step);
      else limb_tile_chain_fill(row, L.n, step);
      limb_tile_desc d;
      memset(&d, 0xee, sizeof d);
      bool planned = !chain;
      if (!limb_tile_desc_build(L, modes[seq], d, &planned) || planned != chain) return 2;
      printf("%d %d %d %d %d %d %d  %d", L.n, L.s0, L.h, L.k0, L.n_t, L.n_limbs, seq, d.n_tiles);
      for (int s = 0; s < HS_TILE_SLOTS * limb_tile_count(L.n); s++) printf(" %d", step[s]);
      for (int t = 0; t < d.n_tiles; t++) {
        const limb_tile_entry& e = d.tile[t];
        for (int g = 0; g < HS_TILE_SLOTS; g++) printf(" %d %d", e.slot[g].step, e.slot[g].row);
        printf(" %u %u %llu %d", e.M, e.nreq, (unsigned long long)e.req, limb_tile_req_passes((int)e.nreq, L.n_limbs));
      }
      for (int t = d.n_tiles; t < HS_TILE_DESC_TILES; t++) {  // the tiles past the launch: idle, no request
        const limb_tile_entry& e = d.tile[t];
        for (int g = 0; g < HS_TILE_SLOTS; g++)
          if (e.slot[g].step != -1) return 3;
        if (e.M || e.nreq || e.req) return 3;
      }
      printf("\n");
    }
  }
  return 0;
}
"""


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return cxx


def _build(d, name, flags):
    src = d / "desc.cpp"
    src.write_text(PROG)
    exe = d / name
    subprocess.run([_cxx(), "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "hslabs_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    return exe


ARGS = [str(v) for (n, s0, (h, k0, n_t), nl) in CASES for v in (n, s0, h, k0, n_t, nl)]


@pytest.fixture(scope="module")
def descs(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("tile_desc"), "desc", [])
    out = subprocess.run([str(exe), *ARGS], check=True, capture_output=True, text=True, timeout=120).stdout
    table = {}
    for line in out.splitlines():
        v = list(map(int, line.split()))
        n, s0, h, k0, n_t, nl, seq, nt = v[:8]
        p = 8
        step = v[p:p + 8 * nt]
        p += 8 * nt
        tiles = []
        for _ in range(nt):
            sr = v[p:p + 16]
            tiles.append(dict(step=sr[0::2], row=sr[1::2], M=v[p + 16], nreq=v[p + 17], req=v[p + 18], passes=v[p + 19]))
            p += 20
        assert p == len(v)
        table[(n, s0, (h, k0, n_t), nl, SEQS[seq])] = dict(step=step, tiles=tiles)
    assert sorted(k[:4] for k in table if k[4] == "plan") == sorted(CASES)
    assert len(table) == len(SEQS) * len(CASES)
    return table


# ---- an independent replay of the kernel's arithmetic ----
def row(step, s0, h, k0, n_t):
    """hs_limb_kernel's table row of a local step (less the constant ktab_lo): limb_tile_row"""
    s_glob = s0 + step
    call = s_glob // h
    return (k0 + call * h) % n_t + s_glob % h


def parity_order(n):
    seq = list(range(0, n, 2)) + list(range(1, n, 2))
    return seq + [-1] * (8 * ((n + 7) // 8) - n)


def kd_rule(rows):
    """limb_tile_kd's rule on a tile's rows (None: idle): the share flags, M and the requests in service order"""
    shm, shp, M = [], [], 0
    for g, r in enumerate(rows):
        m = r is not None and g > 0 and rows[g - 1] is not None and rows[g - 1] + 2 == r
        p = r is not None and g < 7 and rows[g + 1] is not None and rows[g + 1] == r + 2
        shm.append(m)
        shp.append(p)
        if r is not None:
            M |= (not m) << (2 * g) | (not p) << (2 * g + 1)
    order = [b for b in range(16) if (M >> b) & 1]
    return shm, shp, M, order


def providers(rows, M, req, nl):
    """Which lane's FK fills which (group, side, limb) and in which pass, as limb_tile_kd assigns them from the
    descriptor's M and req: {(g, side, L): [(row in row0 units, pass), ...]}; and the further passes run."""
    nreq = bin(M).count("1")
    nidle = 8 - nl
    e0 = (8 * nidle) // nl
    nth = lambda r: (req >> (4 * r)) & 15
    got = {}
    live = [r is not None for r in rows]
    shm = [live[g] and not (M >> (2 * g)) & 1 for g in range(8)]
    shp = [live[g] and not (M >> (2 * g + 1)) & 1 for g in range(8)]
    for g in range(8):  # pass 0
        for l in range(8):
            if l < nl:  # a limb lane: its centre row to the neighbours that share it
                if rows[g] is None:
                    continue
                if shp[g]:
                    got.setdefault((g + 1, 0, l), []).append((rows[g] + 2, 0))
                if shm[g]:
                    got.setdefault((g - 1, 1, l), []).append((rows[g] + 2, 0))
            else:  # an idle lane: one of the first E0 requests
                j = g * nidle + (l - nl)
                rq, fl = divmod(j, nl)
                if rq < e0 and rq < nreq:
                    bit = nth(rq)
                    gr, side = bit >> 1, bit & 1
                    got.setdefault((gr, side, fl), []).append((rows[gr] + 4 * side, 0))
    base, npass = e0, 0
    while base < nreq:  # the further passes: request base + g on group g's limb lanes
        npass += 1
        for g in range(8):
            if base + g < nreq:
                bit = nth(base + g)
                gr, side = bit >> 1, bit & 1
                for l in range(nl):
                    got.setdefault((gr, side, l), []).append((rows[gr] + 4 * side, npass))
        base += 8
    return got, npass


def expected_pass(M, g, side, nl):
    """the pass limb_tile_kd's reader takes its minus / plus row from (its pm / pp)"""
    e0 = (8 * (8 - nl)) // nl
    bit = 2 * g + side
    if not (M >> bit) & 1:
        return 0
    rq = bin(M & ((1 << bit) - 1)).count("1")
    return 0 if rq < e0 else 1 + (rq - e0) // 8


def test_the_grid_is_the_plan_tests():
    assert len(CASES) == 1876


@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("nl", LIMBS)
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("s0", S0S)
def test_descriptor_equals_the_replay(descs, s0, call, nl, seq):
    for n in NS:
        d = descs[(n, s0, call, nl, seq)]
        slots = d["step"]
        if seq == "parity":
            assert slots == parity_order(n), n
        if seq == "chain":  # every step of the launch once, the idle slots at the end
            assert sorted(slots[:n]) == list(range(n)) and slots[n:] == [-1] * (8 * ((n + 7) // 8) - n), n
        assert len(d["tiles"]) == (n + 7) // 8, n
        for t, e in enumerate(d["tiles"]):
            tile = slots[8 * t:8 * t + 8]
            assert e["step"] == tile, (n, t)  # the local step, -1 idle
            rows = [row(s, s0, *call) if s >= 0 else None for s in tile]
            # every live slot's row is limb_tile_row; an idle slot carries the tile's first row (valid addresses)
            assert e["row"] == [r if r is not None else rows[0] for r in rows], (n, t)
            shm, shp, M, order = kd_rule(rows)
            assert e["M"] == M, (n, t)
            assert e["nreq"] == len(order) == bin(e["M"]).count("1"), (n, t)
            assert [(e["req"] >> (4 * r)) & 15 for r in range(len(order))] == order, (n, t)
            assert e["req"] >> (4 * len(order)) == 0, (n, t)
            # the share flags as the kernel reads them off M
            assert [r is not None and not (e["M"] >> (2 * g)) & 1 for g, r in enumerate(rows)] == shm, (n, t)
            assert [r is not None and not (e["M"] >> (2 * g + 1)) & 1 for g, r in enumerate(rows)] == shp, (n, t)


@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("nl", LIMBS)
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("s0", S0S)
def test_every_row_has_one_provider_of_the_right_row_and_pass(descs, s0, call, nl, seq):
    e0 = (8 * (8 - nl)) // nl
    for n in NS:
        d = descs[(n, s0, call, nl, seq)]
        for t, e in enumerate(d["tiles"]):
            rows = [row(s, s0, *call) if s >= 0 else None for s in e["step"]]
            got, npass = providers(rows, e["M"], e["req"], nl)
            want = {}
            for g, r in enumerate(rows):
                if r is None:
                    continue
                for side in (0, 1):
                    for l in range(nl):
                        want[(g, side, l)] = [(r + 4 * side, expected_pass(e["M"], g, side, nl))]
            assert got == want, (n, t)  # the reader's row, from exactly one lane, in the pass the reader expects
            # the further passes of the tile
            assert npass == e["passes"] == -(-max(0, e["nreq"] - e0) // 8), (n, t)


def test_builder_under_sanitizers(tmp_path):
    """limb_tile_desc_build over the whole grid in a stand-alone program with -fsanitize=address,undefined"""
    exe = _build(tmp_path, "desc_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), *ARGS], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == len(SEQS) * len(CASES)


def test_launches_a_descriptor_does_not_hold(tmp_path):
    """limb_tile_desc_ok: longer than a plan, or rows past 16 bits -- those launches stay packed (limb_tile())"""
    src = tmp_path / "ok.cpp"
    src.write_text(r"""
#include <cstdio>
#include "hs_limb_tile.h"
int main() {
  printf("%d %d %d %d %d %d\n", (int)limb_tile_desc_ok(256, 1, 0, 20), (int)limb_tile_desc_ok(257, 1, 0, 20),
         (int)limb_tile_desc_ok(200, 1, 0, 32766), (int)limb_tile_desc_ok(200, 1, 0, 32767),
         (int)limb_tile_desc_ok(0, 1, 0, 20), (int)limb_tile_desc_ok(8, 1, -1, 20));
  return 0;
}
""")
    exe = tmp_path / "ok"
    subprocess.run([_cxx(), "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hslabs_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["1", "0", "1", "0", "0", "0"]
