// hs_sim_trial.hip -- the fall test's unit of the closed-loop simulation: the TRIAL instantiations of the
// simulation kernel (hs_sim_kernel.h; hs_sim_trial: open-loop torques, torque limit, torso kicks, fall
// check) and the tally of its state array, compiled apart from hs_sim_step's so that those stay the code
// they were (the header says why). Built with -ffp-contract=off like hs_sim.hip.
#include "hs_sim_kernel.h"

#include <climits>

namespace {

// Tally of a trial state array: grid-stride loop, cross-lane reduction per wavefront, one atomic
// per wavefront and counter. acc->min_fall_tsi starts at INT32_MAX, the rest at 0.
__global__ __launch_bounds__(256) void hs_trial_summary_kernel(const int32_t* __restrict__ state, int32_t n,
                                                                hs_trial_summary* __restrict__ acc) {
  int running = 0, survived = 0, fallen = 0, mn = INT32_MAX;
  long long sum = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int st = state[i];
    if (st == HS_TRIAL_RUNNING) running++;
    else if (st == HS_TRIAL_SURVIVED) survived++;
    else {
      fallen++;
      mn = min(mn, st);
      sum += st;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    running += __shfl_xor(running, off);
    survived += __shfl_xor(survived, off);
    fallen += __shfl_xor(fallen, off);
    mn = min(mn, __shfl_xor(mn, off));
    sum += __shfl_xor(sum, off);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (running) atomicAdd(&acc->running, running);
    if (survived) atomicAdd(&acc->survived, survived);
    if (fallen) {
      atomicAdd(&acc->fallen, fallen);
      atomicMin(&acc->min_fall_tsi, mn);
      atomicAdd(reinterpret_cast<unsigned long long*>(&acc->sum_fall_tsi), (unsigned long long)sum);
    }
  }
}

}  // namespace

// Diagnostic (tools/fall_test.py --occupancy; not part of hslabs.h): resident rollouts per CU of the
// simulation kernel's instantiations for a model of n parts and m_max rows, as
// {fp64, fp64 trial, fp32, fp32 trial, fp32 3 waves/SIMD, fp32 3 waves/SIMD trial}.
// (ahead of the launcher: the code object lists the kernels in the order the unit first names them, and
// this keeps it class by class, fp64 first)
extern "C" int hs_debug_sim_occupancy(int32_t n, int32_t m_max, int32_t* out6) {
  int32_t plain[3], trial[3];
  if (hs::sim_step_occupancy(n, m_max, plain) != 0 || sim_occupancy<true>(n, m_max, trial) != 0) return -1;
  for (int i = 0; i < 3; i++) {
    out6[2 * i] = plain[i];
    out6[2 * i + 1] = trial[i];
  }
  return 0;
}

namespace hs {

int launch_sim_trial(const sim_dev& dv, const hs_sim_trial_args& a) { return launch_sim<true>(dv, a); }

int launch_trial_summary(const int32_t* state, int32_t n, hs_trial_summary* acc, void* stream) {
  if (n <= 0) return 0;
  const int blocks = (int)((((long)n + 255) / 256 < 1024) ? ((long)n + 255) / 256 : 1024);
  hipLaunchKernelGGL(hs_trial_summary_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, state, n, acc);
  return (int)hipGetLastError();
}

}  // namespace hs
