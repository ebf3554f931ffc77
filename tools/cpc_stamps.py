"""Per-phase shader-clock breakdown of hs_cpc_kernel (diagnostic build, -DHS_CPC_STAMPS).

Builds hslabs_amd/_build/libhslabs_cpcstamps.so, walks a B-rollout batch two position-control steps with
estimates, runs the controller N_CALLS times on the estimated B and prints the mean cycles per call and
wavefront of each phase. Never used by the product path.
  N=4096 MODEL=hexapod python tools/cpc_stamps.py [--build | --build-only]
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hslabs_amd import build as Bd  # noqa: E402

LIB = os.path.join(Bd.OUT_DIR, "libhslabs_cpcstamps.so")
PHASES = ["state + compute_b (QR, bbt)", "loss scan", "selection", "B_chi_dec (QR)", "gain loop", "tp_dist + clip + out"]
PGS = {"hexapod": 8, "spider": 24, "myant": 9}


def main():
    if "--build" in sys.argv or not os.path.exists(LIB):
        Bd._compile(LIB, ["HS_CPC_STAMPS"])
    if "--build-only" in sys.argv:
        return
    import torch
    from hslabs_amd import capi
    L = ctypes.CDLL(LIB)
    capi._lib = None
    Bd.LIB = LIB
    capi.load(build_if_missing=False)
    import hslabs_amd as H
    n = int(os.environ.get("N", "4096"))
    calls = int(os.environ.get("N_CALLS", "10"))
    name = os.environ.get("MODEL", "hexapod")
    m = H.KinematicModel(os.path.join(ROOT, "models", name + ".xml"))
    p = H.read_pgs_config(os.path.join(ROOT, "models", "pgs_config.txt"), PGS[name])
    sb = H.SimBatch(m, [p] * n)
    for i in range(2):
        sb.estimate_B(seed=i)
        sb.step(1, outputs=("tau_cmd",))
    Bt = sb.estimate_B(seed=2)["Bt"]
    sb.cpc_torques(Bt)
    torch.cuda.synchronize()
    L.hs_debug_clear_cpc_stamps()
    for _ in range(calls):
        sb.low_tpdist.fill_(1)
        sb.cpc_torques(Bt)
    torch.cuda.synchronize()
    st = np.zeros((4096, 8), dtype=np.uint64)
    L.hs_debug_read_cpc_stamps(st.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), 4096)
    st = st[:min(n, 4096)].astype(np.float64) / calls
    tot = st[:, :6].sum(axis=1)
    print(f"{name}: B = {n}, n_tp = {sb.n_t}, {calls} calls; shader-clock cycles per wavefront and call")
    for i, ph in enumerate(PHASES):
        d = st[:, i]
        print(f"{ph:30s} mean {d.mean():10.0f}  p50 {np.median(d):10.0f}  p90 {np.percentile(d, 90):10.0f}"
              f"  ({100 * d.mean() / tot.mean():5.1f} %)")
    print(f"{'TOTAL':30s} mean {tot.mean():10.0f}; gain-loop passes per call {st[:, 6].mean():.2f}")


if __name__ == "__main__":
    main()
