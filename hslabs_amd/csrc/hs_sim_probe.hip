// hs_sim_probe.hip -- "dynamics from simulation" (modelplayer::estimate_B_by_regression, player.cpp:548-582)
// for a batch: the PROBE instantiations of the simulation kernel (hs_sim_kernel.h; a unit apart from
// hs_sim_step's and hs_sim_trial's so that those stay the code they were), get_ode_config, the
// derivative tracker and the regression of accelerations on torques. Built like hs_sim.hip, with
// -ffp-contract=off: the probes must step exactly as hs_sim_trial steps, and the tracker's
// subtract-then-scale (odestate.cpp:114-116) must not fuse.
#include "hs_sim_kernel.h"

#include <cfloat>

#include "hs_colpiv.h"

namespace {

// visualizer::get_ode_config (visualization.cpp:378-396), one lane per rollout: torso pose, then
// dJointGetHingeAngle of every motor in motor order (the P phase's hinge_angle).
template <class IO>
__global__ __launch_bounds__(WAVE) void hs_sim_config_kernel(const hs_topo* __restrict__ T0,
                                                              const hs_simtopo_t<IO>* __restrict__ S, int32_t n_rollouts,
                                                              const IO* __restrict__ body, IO* __restrict__ config,
                                                              int32_t stride) {
  const int b = blockIdx.x * WAVE + threadIdx.x;
  if (b >= n_rollouts) return;
  const hs_simtopo_t<IO>& T = *S;
  const IO* bd = body + (size_t)b * T.n * HS_SIM_BODY;
  IO* out = config + (size_t)b * stride;
  torso_config(T0, T.body_geom[0], bd, bd + 3, out);
  const BodyView<IO> view{{bd}};
  for (int j = 0; j < T.nmj; j++) out[6 + j] = hinge_angle(view, T.joint[T.motor_joint[j]]);
}

// configtimedertrack(2, config_dim, dt)::push_config (odestate.cpp:105-119), one lane per (rollout,
// coordinate): level by level, subtract then multiply by (1./dt). ders [B][3][cfg] starts at zero, so
// the first push leaves config / dt as "velocity", like the reference; no angle wrap, like the reference.
__global__ __launch_bounds__(256) void hs_track_push_kernel(int32_t n_rollouts, int32_t cfg,
                                                             const double* __restrict__ config, int32_t stride,
                                                             double h1, double* __restrict__ ders) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)n_rollouts * cfg) return;
  const int b = (int)(e / cfg), i = (int)(e % cfg);
  double* d = ders + (size_t)b * 3 * cfg + i;
  double nw = config[(size_t)b * stride + i], old = d[0];
  d[0] = nw;
  for (int lv = 1; lv <= 2; lv++) {  // compute_dern
    nw -= old;
    nw *= h1;
    old = d[lv * cfg];
    d[lv * cfg] = nw;
  }
}

// U[b][j] = ders[2] of a copy of rollout b's tracker after push_config(config_out[b][j])
// (player.cpp:564, 572-575; the copy takes levels 0 and 1, odestate.cpp:130-135)
__global__ __launch_bounds__(256) void hs_probe_accel_kernel(int32_t n_rollouts, int32_t m, int32_t cfg,
                                                              const double* __restrict__ config_out,
                                                              const double* __restrict__ ders, double h1,
                                                              double* __restrict__ U) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)n_rollouts * m * cfg) return;
  const int i = (int)(e % cfg);
  const int b = (int)(e / ((long)m * cfg));
  const double* d = ders + (size_t)b * 3 * cfg + i;
  double nw = config_out[e];
  nw -= d[0];
  nw *= h1;
  nw -= d[cfg];
  nw *= h1;
  U[e] = nw;
}

// B_from_T_U (player.cpp:531-546), one wavefront per rollout, everything in LDS: A = [T^T | 1]
// (m x (nmj + 1), column-major), Eigen 3.3 ColPivHouseholderQR of it (hs_colpiv.h, shared with the
// configuration path controller), then B.row(i) = solve(U.row(i)^T), one lane per right-hand side i, and
// Bt[j] = B.col(j) for j < nmj (the constant column is dropped). rank = Eigen's nonzeroPivots(), the
// count its solve uses.
__global__ __launch_bounds__(WAVE) void hs_regress_kernel(int32_t n_rollouts, int32_t m, int32_t nmj, int32_t cfg,
                                                           const double* __restrict__ Tg, const double* __restrict__ Ug,
                                                           double* __restrict__ Bt, int32_t* __restrict__ rank) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, b = blockIdx.x;
  if (b >= n_rollouts) return;
  double* bt = Bt + (size_t)b * nmj * cfg;
  if (m == 0) {  // set_Bt_unity (player.cpp:522-529)
    for (int e = lane; e < nmj * cfg; e += WAVE) bt[e] = (e % cfg == cfg - nmj + e / cfg) ? 1.0 : 0.0;
    if (lane == 0) rank[b] = 0;
    return;
  }
  const int n = nmj + 1;
  double* qr = lds;             // [n][m]: qr[r + c * m]
  double* C = qr + (size_t)m * n;  // right-hand sides [m][cfg]: C[r * cfg + i], lane i's column
  double* nu = C + (size_t)m * cfg;  // Eigen's colNormsUpdated / colNormsDirect / hCoeffs
  double* nd = nu + n;
  double* hc = nd + n;
  int* perm = reinterpret_cast<int*>(hc + n);
  const double* Tb = Tg + (size_t)b * m * nmj;
  const double* Ub = Ug + (size_t)b * m * cfg;
  for (int e = lane; e < m * nmj; e += WAVE) qr[e / nmj + (e % nmj) * m] = Tb[e];
  for (int r = lane; r < m; r += WAVE) qr[r + nmj * m] = 1.0;
  for (int e = lane; e < m * cfg; e += WAVE) C[e] = Ub[e];
  const int np = hs_colpiv::factor(qr, m, n, nu, nd, hc, perm, lane);
  // B.row(i)[perm[k]] = z[k]; lane = right-hand side
  const int i = lane;
  hs_colpiv::solve(qr, m, np, hc, C, cfg, lane);
  wave_sync();
  for (int k = 0; k < n; k++) {
    const int col = perm[k];
    if (col < nmj && i < cfg) bt[(size_t)col * cfg + i] = (k < np) ? C[k * cfg + i] : 0.0;
  }
  if (lane == 0) rank[b] = np;
}

// one wavefront per probe; the fp64 probe kernel is held to the 2-waves/SIMD budget, like the trial kernel
template <class R, class S>
int launch_probe_typed(const hs_topo* d_topo, const S* d_sim, const hs_simtopo& hs, const hs_sim_probe_kargs& ka) {
  const bool fits = sim_lds_class(hs.n, hs.m_max, [&](auto nm, auto mm) {
    constexpr int MINW = sizeof(R) == 8 ? 2 : 1;
    hipLaunchKernelGGL((hs_sim_kernel<decltype(nm)::value, decltype(mm)::value, R, MINW, false, true>),
                       dim3(ka.sim.n_rollouts * ka.m), dim3(WAVE), 0, (hipStream_t)ka.sim.stream, d_topo, d_sim, ka);
  });
  return fits ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

}  // namespace

namespace hs {

int launch_sim_config(const sim_dev& dv, int32_t n, const double* body, double* config, int32_t config_stride,
                      int32_t precision, void* stream) {
  if (n <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((n + WAVE - 1) / WAVE);
  if (precision == HS_PREC_F32)
    hipLaunchKernelGGL(hs_sim_config_kernel<float>, grid, dim3(WAVE), 0, st, dv.topo, dv.sim_f32, n,
                       reinterpret_cast<const float*>(body), reinterpret_cast<float*>(config), config_stride);
  else
    hipLaunchKernelGGL(hs_sim_config_kernel<double>, grid, dim3(WAVE), 0, st, dv.topo, dv.sim, n, body, config,
                       config_stride);
  return (int)hipGetLastError();
}

int launch_track_push(int32_t n, int32_t cfg, const double* config, int32_t config_stride, double dt, double* ders,
                      void* stream) {
  if (n <= 0) return 0;
  const long total = (long)n * cfg;
  hipLaunchKernelGGL(hs_track_push_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     cfg, config, config_stride, 1. / dt, ders);
  return (int)hipGetLastError();
}

int launch_sim_probe(const sim_dev& dv, const hs_sim_probe_kargs& a) {
  if (a.sim.n_rollouts <= 0 || a.m <= 0) return 0;
  if (a.sim.precision == HS_PREC_F32) return launch_probe_typed<float>(dv.topo, dv.sim_f32, dv.host, a);
  return launch_probe_typed<double>(dv.topo, dv.sim, dv.host, a);
}

int launch_probe_accel(int32_t n, int32_t m, int32_t cfg, const double* config_out, const double* ders, double dt,
                       double* U, void* stream) {
  if (n <= 0 || m <= 0) return 0;
  const long total = (long)n * m * cfg;
  hipLaunchKernelGGL(hs_probe_accel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     m, cfg, config_out, ders, 1. / dt, U);
  return (int)hipGetLastError();
}

size_t regress_lds_bytes(int32_t m, int32_t nmj, int32_t cfg) {
  const size_t n = (size_t)nmj + 1;
  return ((size_t)m * n + (size_t)m * cfg + 3 * n) * sizeof(double) + n * sizeof(int);
}

int launch_regress_B(int32_t n, int32_t m, int32_t nmj, int32_t cfg, const double* T, const double* U, double* Bt,
                     int32_t* rank, void* stream) {
  if (n <= 0) return 0;
  const size_t lds = m > 0 ? regress_lds_bytes(m, nmj, cfg) : 0;
  hipLaunchKernelGGL(hs_regress_kernel, dim3(n), dim3(WAVE), lds, (hipStream_t)stream, n, m, nmj, cfg, T, U, Bt, rank);
  return (int)hipGetLastError();
}

}  // namespace hs
