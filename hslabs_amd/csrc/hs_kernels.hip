// hs_kernels.hip -- the fp64 unit of the step kernels: the device code of the headers below in double
// precision and its launcher table hs::kernels_f64, and what exists once whatever the precision: the
// pergen record kernel, the workspace size and table range the host plans with, and the readers of the
// diagnostic builds' tables (HS_STAMPS, HS_DBG).
#include "hs_rollout_kernel.h"
#include "hs_limb.h"

namespace {

// pergensetup::set_rec (pergen.cpp:225-239) after setup_pergen (pergen.cpp:453-507), for
// n_rollouts x n_times (rollout, time) items, two per wavefront: the gait setup of the item's
// rollout on its half-wave, then lane L < n_limbs writes lik limb L's foot target, lane 0 the
// torso position and angles. rec rows: [torso_pos(3), torso_angles(3), foot targets (3 n_limbs)].
__global__ __launch_bounds__(WAVE) void hs_pergen_rec_kernel(const hs_topo* __restrict__ T,
                                                             const hs_gait_params* __restrict__ params,
                                                             int32_t n_rollouts, const double* __restrict__ times,
                                                             int32_t n_times, double* __restrict__ rec) {
  __shared__ SetupL st[2];
  const int sub = threadIdx.x / HALF, lane = threadIdx.x % HALF;
  const int64_t n_items = (int64_t)n_rollouts * n_times;
  const int64_t item = (int64_t)blockIdx.x * 2 + sub;
  const bool live = item < n_items;
  const int64_t it = live ? item : n_items - 1;  // an idle half computes its neighbour's item, stores nothing
  const int b = (int)(it / n_times), ti = (int)(it % n_times);
  const GaitR g = load_gait(params[b]);
  gait_setup(T, g, 1, st[sub], lane);  // every lane of the wave takes part (wave_sync inside)
  const int nl = T->n_limbs;
  if (live && lane < nl) {
    real o0[3], o1[3], target[3];
    bool turned;
    gait_record<false>(g, params[b], limb_rec(st[sub], T->limb_pergen[lane]), (real)times[ti], o0, o1, turned, target);
    double* r = rec + it * (6 + 3 * nl);
    if (lane == 0)
      for (int i = 0; i < 3; i++) { r[i] = o0[i]; r[3 + i] = o1[i]; }
    for (int i = 0; i < 3; i++) r[6 + 3 * lane + i] = target[i];
  }
}

}  // namespace

#ifdef HS_DBG
extern "C" int hs_debug_read_dbg(double* out, int n) {
  if (n > (1 << 22)) n = 1 << 22;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(double) * n, 0, hipMemcpyDeviceToHost);
}
#endif

#ifdef HS_STAMPS
extern "C" int hs_debug_read_stamps(unsigned long long* out, int n_rows) {
  if (n_rows > 4096) n_rows = 4096;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 32 * n_rows, 0,
                                  hipMemcpyDeviceToHost);
}
extern "C" int hs_debug_set_stamp_base(unsigned int base) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_base), &base, sizeof(base), 0, hipMemcpyHostToDevice);
}
extern "C" int hs_debug_set_stamp_iter(int iter) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_iter), &iter, sizeof(iter), 0, hipMemcpyHostToDevice);
}
extern "C" int hs_debug_clear_stamps() {
  static unsigned long long zero[4096][32];
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice);
}
#endif

namespace hs {

size_t solve_workspace_bytes() { return sizeof(SolveWS); }  // >= the fp32 build's

int limb_tables_read(const void* workspace, int32_t rollout, int32_t n_rows, double* ktab, double* kvel, uint8_t* kbig,
                     uint8_t* kbad, double* dt, void* stream) {
  static_assert(std::is_same<real, double>::value, "the fp64 unit's RolloutWS");
  if (n_rows < 0 || n_rows > HS_KTAB) return (int)hipErrorInvalidValue;
  const RolloutWS* W = (const RolloutWS*)workspace + rollout;
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  const auto get = [&](void* dst, const void* src, size_t n) {
    if (e == hipSuccess && dst && n) e = hipMemcpy(dst, src, n, hipMemcpyDeviceToHost);
  };
  get(ktab, W->ktab, sizeof(W->ktab[0]) * n_rows);
  get(kvel, W->kvel, sizeof(W->kvel[0]) * n_rows);
  get(kbig, W->kbig, sizeof(W->kbig[0]) * n_rows);
  get(kbad, W->kbad, sizeof(W->kbad[0]) * n_rows);
  get(dt, &W->st.dt, sizeof(double));
  return (int)e;
}

void ktab_range(int32_t k0, int32_t n_t, int32_t horizon, int64_t n_calls, int32_t* lo_out, int32_t* n_out,
                int32_t* ttab_out) {
  // call c starts at centre sample (k0 + c horizon) % n_t + 2 (the fused and the per-step paths
  // alike) and its steps read that first k0 + [0, horizon + NS - 1); the first k0s repeat with a
  // period dividing n_t
  int64_t lo = INT64_MAX, hi = 0;
  const int64_t nc = n_calls < n_t ? n_calls : n_t;
  for (int64_t c = 0; c < nc; c++) {
    const int64_t f = ((int64_t)k0 + c * horizon) % n_t;
    lo = f < lo ? f : lo;
    hi = f + horizon + NS - 1 > hi ? f + horizon + NS - 1 : hi;
  }
  const int64_t n = nc > 0 ? hi - lo : 0;
  *lo_out = nc > 0 ? (int32_t)lo : 0;
  *n_out = n <= HS_KTAB ? (int32_t)n : 0;                // the IK table: every sample, or none
  *ttab_out = (int32_t)(n < HS_KTAB ? n : HS_KTAB);      // sample times: the first HS_KTAB samples
}

int launch_pergen_rec(const hs_topo* d_topo, const hs_gait_params* params, int32_t n_rollouts, const double* times,
                      int32_t n_times, double* rec, void* stream) {
  const int64_t items = (int64_t)n_rollouts * n_times;
  if (items <= 0) return 0;
  hipLaunchKernelGGL(hs_pergen_rec_kernel, dim3((unsigned)((items + 1) / 2)), dim3(WAVE), 0, (hipStream_t)stream,
                     d_topo, params, n_rollouts, times, n_times, rec);
  return (int)hipGetLastError();
}

#ifndef __HIP_DEVICE_COMPILE__  // host only: the device pass would emit a constant-initialised const object too
extern const kernels kernels_f64 = {general_workspace_bytes, launch_rollouts,     launch_fused,
                                    launch_limb,             launch_fused_reduce, limb_deferred};
#endif

}  // namespace hs
