"""tests/cpp/fall_test.cpp: the fall test through the C++ shim (set_flag("torso_kicks"),
set_fall_test, simulate_ode, fall_state) gives SimBatch.trial's verdict, time and torso."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, PGS_CONFIG
from test_cpp_shim import compile_prog

DT = 0.01


def window(tmin, tmax):
    """first tsi with tsi * dt >= tmin, last tsi with tsi * dt <= tmax (fall_check's comparisons)"""
    lo = next(i for i in range(10 ** 6) if not i * DT < tmin)
    hi = max(i for i in range(int(tmax / DT) + 3) if not i * DT > tmax)
    return lo, hi


@pytest.fixture(scope="module")
def exe(product, tmp_path_factory):
    return compile_prog(product, tmp_path_factory.mktemp("fall_test") / "fall_test", "fall_test.cpp")


def run(exe, dv, every, phase, hc, tmin, tmax, steps, *more):
    args = [str(exe), MODELS, *map(repr, dv), str(every), str(phase), repr(hc), repr(tmin), repr(tmax), str(steps),
            *map(repr, more)]
    out = subprocess.run(args, check=True, capture_output=True, text=True, timeout=300).stdout
    return out.splitlines()


@pytest.mark.gpu
@pytest.mark.parametrize("d,tmin,tmax,limit,verdict", [(40.0, 0.0, 1.0, None, "Fall at"), (20.0, 0.0, 1.0, None, "No fall by"),
                                                       (100.0, 0.7, 100.0, None, "Fall at"), (0.0, 0.0, 100.0, 0.5, "Fall at"),
                                                       (0.0, 0.0, 100.0, None, "Running")])
def test_shim_fall_test_matches_python(product, exe, d, tmin, tmax, limit, verdict):
    import torch

    steps = 150
    lines = run(exe, (0.0, d, 0.0), 1000, 12, 0.7, tmin, tmax, steps, *([limit] if limit else []))
    assert "unknown_flag_throws = 1" in lines
    line = [ln for ln in lines if ln.startswith(("Fall at", "No fall by", "Running"))][0]
    assert line.startswith(verdict), lines
    t = float(line.split("=")[1])
    vals = {ln.split("=")[0].strip(): [float(v) for v in ln.split("=")[1].split()] for ln in lines if "=" in ln}

    p = product.read_pgs_config(PGS_CONFIG, 8)
    m = product.KinematicModel(os.path.join(MODELS, "hexapod.xml"))
    sb = product.SimBatch(m, [p], tsi0=2)
    lo, hi = window(tmin, tmax)
    sb.trial(steps, kick_every=1000, kick_phase=12, kick_dv=np.array([[0.0, d, 0.0]]), hc=0.7, check_from=lo,
             check_until=hi, torque_limit=limit or 0.0, torso=True)
    torch.cuda.synchronize()
    st, tsi = int(sb.state[0]), int(sb.tsi[0])
    if verdict == "Fall at":
        assert st >= 0 and t == pytest.approx(st * DT, abs=1e-9)
    elif verdict == "No fall by":
        assert st == -2 and tsi == hi + 1 and t == pytest.approx(tsi * DT, abs=1e-9)
    else:
        assert st == -1 and tsi == 2 + steps
    assert vals["play_t"][0] == pytest.approx(tsi * DT, abs=1e-9)
    assert np.abs(np.array(vals["torso"]) - sb.body[0, 0, :3].cpu().numpy()).max() < 2e-12
    assert vals["below_hc"][0] == (1 if verdict == "Fall at" else 0)
