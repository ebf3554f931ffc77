"""Per-phase shader-clock breakdown of the limb-lane step kernel (hs_limb.h; the stamp
table is hs_step_base.h's, its readers hs_kernels.hip's; diagnostic -DHS_STAMPS build libhslabs_stamps.so, tools/stamps.py's). Runs the bench's fused path (hexapod B = 4096, 20 calls) and prints
mean / p50 / p90 cycles per phase over the wavefronts of one window of the launch (STEP=s: blocks from
s * 512). Tuning aid only.   python tools/limb_stamps.py [--build] [--steps K] [--tile]
--steps K: K calls instead of 20. --tile: the tile mapping at any K (HS_LIMB_TILE_MIN=1), its phases named
as limb_tile_kd stamps them: the one FK pass (centre rows and the first requests), the further passes
(taken at a break of the slot sequence), the exchange's barrier with the finite differences.
--tile --passes: instead of one window's phases, the share of the launch's tile wavefronts that take further FK
passes, from windows over the whole launch (the planner, hs_limb_tile.h, puts the tiles of chain remainders last,
so no single window shows it; HS_LIMB_TILE_PLAN=0 for the parity order). A wavefront counts as taking them when
its "further FK passes" phase lasts more than half its pass 0.
--tile --loop TL --iter I: TL tiles per wavefront (HS_LIMB_TILE_LOOP=TL), the stamps of the wavefronts' I-th tile
(0: the first). "tile start -> tv, o" is the step's own prelims, from the tile's start (the head's end in the
first tile); "prelims (tv, o)" counts from the wavefront's entry, so it is the head's cost only at I = 0.
The two "head" rows count from the kernel's entry (slot 18): to the stamp behind the link-record copy, and to
the first tile's start, which is the whole head with the staging of the wavefront's constants in LDS and its
barrier (meaningful at I = 0 only; a library without slot 18 prints its clock value there)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hslabs_amd import build as B  # noqa: E402

LIB = os.path.join(B.OUT_DIR, "libhslabs_stamps.so")
PHASES = [("prelims (tv, o)", 15, 0), ("outer t-2dt FK", 0, 1), ("outer t+2dt FK", 1, 2), ("centre FK + D", 2, 3),
          ("torso + sync", 3, 4), ("subtree sums + root", 4, 5), ("contact list + zeroth", 5, 6),
          ("contact blocks + Schur sums", 6, 7), ("6x6 + y", 7, 8), ("outputs", 8, 9), ("TOTAL", 15, 9)]


TILE_PHASES = [("head: entry -> link copy issued", 18, 15), ("head: entry -> first tile (I = 0)", 18, 23),
               ("prelims (tv, o)", 15, 0), ("tile start -> tv, o", 23, 0), ("FK pass 0 (centres + requests)", 0, 1), ("further FK passes", 1, 2),
               ("exchange sync + D", 2, 3)] + PHASES[4:]


def main():
    tile = "--tile" in sys.argv
    K = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 20
    tl = int(sys.argv[sys.argv.index("--loop") + 1]) if "--loop" in sys.argv else None
    it = int(sys.argv[sys.argv.index("--iter") + 1]) if "--iter" in sys.argv else 0
    if tile:
        os.environ["HS_LIMB_TILE_MIN"] = "1"
        if tl is not None:
            os.environ["HS_LIMB_TILE_LOOP"] = str(tl)
    else:
        os.environ["HS_LIMB_TILE"] = "0"
    if "--build" in sys.argv or not os.path.exists(LIB):
        B._compile(LIB, ["HS_STAMPS"])
    if "--build-only" in sys.argv:
        return
    import torch
    from hslabs_amd import capi
    L = ctypes.CDLL(LIB)
    capi._lib = None
    capi._build.LIB = LIB
    capi.load(build_if_missing=False)
    import hslabs_amd as H
    from hslabs_amd import synth

    n = 4096
    m = H.KinematicModel(os.path.join(ROOT, "models", "hexapod.xml"))
    params = synth.gen_params(n, "hexapod")
    b = H.DeviceBatch(m, params, n_t=20, k0=0, horizon=K, outputs=("tau", "cf", "work_cot", "flags"))
    b.run_calls(K, best=True)
    torch.cuda.synchronize()
    if tile and "--passes" in sys.argv:
        return passes_share(L, b, K, n)
    L.hs_debug_set_stamp_base(ctypes.c_uint(int(os.environ.get("STEP", "4" if tl is None else "0")) * (n // 8)))
    L.hs_debug_set_stamp_iter(ctypes.c_int(it))
    L.hs_debug_clear_stamps()
    b.run_calls(K, best=True)
    torch.cuda.synchronize()
    st = np.zeros((4096, 32), dtype=np.uint64)
    L.hs_debug_read_stamps(st.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), 4096)
    st = st.astype(np.int64)
    st = st[(st[:, 9] != 0) & (st[:, 15] != 0) & (st[:, 23] != 0)]
    if tile:
        print(f"tiles per wavefront: {tl if tl is not None else 'by the rule'}; tile {it} of each wavefront")
    for name, a, c in (TILE_PHASES if tile else PHASES):
        d = st[:, c] - st[:, a]
        print(f"{name:28s} mean {d.mean():9.0f}  p50 {np.median(d):9.0f}  p90 {np.percentile(d, 90):9.0f}  (n={len(d)})")
    t0 = st[:, 16].min()
    d = (st[:, 17] - st[:, 16]) / 100.0
    print(f"{'wave life (us)':28s} mean {d.mean():9.2f}  p50 {np.median(d):9.2f}  p90 {np.percentile(d, 90):9.2f}")
    s0 = (st[:, 16] - t0) / 100.0
    print(f"{'wave start (us)':28s} mean {s0.mean():9.2f}  max {s0.max():9.2f}")


def passes_share(L, b, K, n):
    """windows of 4096 blocks over the launch's (n / 8) * 8 * tiles blocks, a run each"""
    import torch

    blocks = (n // 8) * 8 * ((K + 7) // 8)
    took = total = 0
    extra = []
    for base in range(0, blocks, 4096):
        L.hs_debug_set_stamp_base(ctypes.c_uint(base))
        L.hs_debug_clear_stamps()
        b.run_calls(K, best=True)
        torch.cuda.synchronize()
        st = np.zeros((4096, 32), dtype=np.uint64)
        L.hs_debug_read_stamps(st.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), 4096)
        st = st.astype(np.int64)
        st = st[(st[:, 9] != 0) & (st[:, 15] != 0)]
        p0, further = st[:, 1] - st[:, 0], st[:, 2] - st[:, 1]
        hit = further > p0 // 2
        took += int(hit.sum())
        total += len(st)
        extra.extend(further[hit].tolist())
    print(f"K = {K}: {took} of {total} tile wavefronts take further FK passes ({100.0 * took / max(total, 1):.1f} %), "
          f"their further-passes phase p50 {np.median(extra) if extra else 0:.0f} cycles")


if __name__ == "__main__":
    main()
