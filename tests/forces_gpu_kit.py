"""What solve_forces' GPU oracle tests share (tests/test_gpu_forces_f32_oracle.py and the lifted-torso test of
tests/test_gpu.py): the kernel's runner and the lifted-torso batches. Not a test module: the test files import
from it by name. The inputs, the perturbed torques, spread() and gamma() live in tests/test_forces_oracle_f32.py."""
import numpy as np

from conftest import record_to_oracle_gait
from test_forces_oracle_f32 import N_T, gait_inputs, gait_record, perturbed_tau
from test_oracle import LIFTED_CASES

# per model: the lifted-torso rows of its batch (a LIFTED_CASES index, or None for an ordinary rollout of
# gait_inputs(name, "straight")), interleaved so that a wavefront of either kernel (two rollouts of
# hs_rollout_kernel, eight of the limb-lane kernel) holds both kinds; myant's batch is odd (an idle half)
LIFTED_ROWS = {"hexapod": (0, None, 1, None, None, None), "myant": (2, None, None, None, None)}


def kernel_forces(gpu, model, params, tau, dtype, mode=None, calls=False):
    """solve_forces on tau [B][20][nmj] (uploaded as it is: float values): hs_run_forces, or (calls) hs_run_forces_calls
    with n_calls = 20, H = 1; cf (NaN first) as float64 and flags on the host"""
    import torch

    fb = gpu.DeviceBatch(model, params, n_t=N_T, k0=0, horizon=N_T, outputs=("cf", "flags"), dtype=dtype)
    if mode is not None:
        fb.solve_mode = mode
    fb.cf.fill_(float("nan"))
    t = torch.from_numpy(np.ascontiguousarray(tau)).to(device=fb.device, dtype=dtype)
    if calls:
        fb.run_forces_calls(t, N_T, call_horizon=1)
    else:
        fb.run_forces(t)
    torch.cuda.synchronize()
    assert fb.cf.dtype == dtype
    return dict(cf=fb.cf.double().cpu().numpy(), flags=fb.flags.cpu().numpy().astype(np.uint32))


def lifted_batch(O, om, name):
    """model `name`'s lifted-torso batch: (GAIT_DTYPE records, oracle gaits, perturbed torques [B][20][nmj],
    the lifted rows' indices)"""
    from hslabs_amd import GAIT_DTYPE

    cases = LIFTED_CASES(O)
    rows = LIFTED_ROWS[name]
    plain = iter(gait_inputs(name, "straight"))
    params = np.zeros(len(rows), GAIT_DTYPE)
    for b, c in enumerate(rows):
        if c is None:
            params[b] = next(plain)
        else:
            assert cases[c][0] == name
            params[b] = gait_record(cases[c][1])
    gaits = [record_to_oracle_gait(O, r) for r in params]
    return params, gaits, perturbed_tau(O, om, gaits), [b for b, c in enumerate(rows) if c is not None]
