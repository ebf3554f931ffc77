// hs_cpc.hip -- configuration path control (cpccontroller, cpc.cpp) on the estimated B for a batch: one
// wavefront per rollout runs cpccontroller::get_motor_torques as modelplayer::set_cpc_torques drives it
// (player.cpp:465-481), scanning every target point (tpis_subset without efficientdata, cpc.cpp:437-443).
// A unit of its own, so that no existing kernel's code generation moves, built with
// -ffp-contract=off like the other simulation units: the controller's choices (candidate order, best score,
// the gain loop's exits) are comparisons of rounded values, held to the unfused CPU restatement.
// Also here: set_target_points_by_per from the controller tables, and the row copy of hs_sim_cpc_step.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>

#include "hs_colpiv.h"
#include "hs_internal.h"

namespace {

constexpr int WAVE = 64;
using hs_colpiv::sync;

// LDS of one wavefront, in doubles then ints. CFG = config_dim padded (24 or 32): the state, b^T and bbt are
// zero-padded to it, so the scan's loops over coordinates unroll over registers without guards (a padded
// coordinate behaves like a masked one: all its terms are products with 0).
struct cpc_lds {
  int q0, dq0, bT, bbt, qr, C, taus, nu, nd, hc, cl, ct0, cs, norms, L, T0, S, n_doubles;
  int perm, ctpi, taken, n_ints;
  __host__ __device__ cpc_lds(int CFG, int cfg, int nmj, int nc, int ntp) {
    const int psi = cfg - nmj;
    int o = 0;
    q0 = o; o += CFG;
    dq0 = o; o += CFG;
    bT = o; o += psi * CFG;        // b^T [psi][CFG]: bT[k * CFG + i] = b(i, k); broadcast reads
    bbt = o; o += CFG * CFG;       // bbt [CFG][CFG]; broadcast reads; later the 2 cfg squares of tp_dist_check
    qr = o; o += nmj * nmj;        // Bt_chi, then B_chi, factored in place (hs_colpiv.h)
    C = o; o += nmj * (psi > nc ? psi : nc);  // right-hand sides [nmj][nrhs], lane = column
    taus = o; o += nmj * nc;       // cand_taus [nmj][n_cand]
    nu = o; o += nmj;
    nd = o; o += nmj;
    hc = o; o += nmj;
    cl = o; o += nc;               // candidates: loss, t0, s
    ct0 = o; o += nc;
    cs = o; o += nc;
    norms = o; o += nc;
    L = o; o += ntp;               // per target point: loss, t0, s
    T0 = o; o += ntp;
    S = o; o += ntp;
    n_doubles = o;
    o = 0;
    perm = o; o += nmj;
    ctpi = o; o += nc;
    taken = o; o += ntp;
    n_ints = o;
  }
  __host__ __device__ size_t bytes() const { return (size_t)n_doubles * sizeof(double) + (size_t)n_ints * sizeof(int); }
};

// Diagnostic build (-DHS_CPC_STAMPS, tools/cpc_stamps.py): shader-clock cycles per phase and wavefront
#ifdef HS_CPC_STAMPS
__device__ unsigned long long g_cpc_stamps[4096][8];
#define CPC_ACC(slot)                                                                            \
  do {                                                                                           \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                \
    if (threadIdx.x == 0 && blockIdx.x < 4096) g_cpc_stamps[blockIdx.x][slot] += now_ - t_last;  \
    t_last = now_;                                                                               \
  } while (0)
#define CPC_T0() unsigned long long t_last = __builtin_amdgcn_s_memtime()
#else
#define CPC_ACC(slot) do {} while (0)
#define CPC_T0() do {} while (0)
#endif

// a value every lane holds alike, as the compiler sees it too (the gain loop's exit must be a scalar branch)
__device__ inline double uniform(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

template <int CFG>
__global__ __launch_bounds__(WAVE) void hs_cpc_kernel(const hs_cpc_args a, const int nmj, const int cfg) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, b = blockIdx.x;
  if (b >= a.n_rollouts) return;
  const hs_cpc_params P = a.params;
  const int psi = cfg - nmj, nc = P.n_cand, ntp = a.n_tp, rec = 2 * cfg + nmj;
  const cpc_lds O(CFG, cfg, nmj, nc, ntp);
  double* q0 = lds + O.q0;
  double* dq0 = lds + O.dq0;
  double* bT = lds + O.bT;
  double* bbt = lds + O.bbt;
  double* qr = lds + O.qr;
  double* C = lds + O.C;
  double* taus = lds + O.taus;
  double* nu = lds + O.nu;
  double* nd = lds + O.nd;
  double* hc = lds + O.hc;
  double* cl = lds + O.cl;
  double* ct0 = lds + O.ct0;
  double* cs = lds + O.cs;
  double* norms = lds + O.norms;
  double* L = lds + O.L;
  double* T0 = lds + O.T0;
  double* S = lds + O.S;
  int* ilds = reinterpret_cast<int*>(lds + O.n_doubles);
  int* perm = ilds + O.perm;
  int* ctpi = ilds + O.ctpi;
  int* taken = ilds + O.taken;
  const double* __restrict__ Btb = a.Bt + (size_t)b * nmj * cfg;
  const double* __restrict__ st = a.state + (size_t)b * a.state_stride;
  const double* __restrict__ tp = a.tp + (size_t)b * a.tp_stride;
  const int low_in = a.low_tpdist[b];
  uint32_t flags = 0;
  CPC_T0();

  // ---- 1. set_current_state + apply_mask (cpc.cpp:103-108, 476-483), on a copy
  if (lane < CFG) {
    const bool zero = lane >= cfg || ((P.mask >> lane) & 1u);
    q0[lane] = zero ? 0.0 : st[lane];
    dq0[lane] = zero ? 0.0 : st[cfg + lane];
  }
  // ---- 2. compute_b (cpc.cpp:111-121): Bt_chi X = the left psi columns of Bt
  for (int e = lane; e < nmj * nmj; e += WAVE) {
    const int r = e / nmj, c = e % nmj;
    qr[r + c * nmj] = Btb[r * cfg + psi + c];
  }
  for (int e = lane; e < nmj * psi; e += WAVE) C[e] = Btb[(e / psi) * cfg + e % psi];
  for (int e = lane; e < psi * CFG; e += WAVE) bT[e] = 0.0;
  const int np1 = hs_colpiv::factor(qr, nmj, nmj, nu, nd, hc, perm, lane);
  hs_colpiv::solve(qr, nmj, np1, hc, C, psi, lane);
  if (lane < psi) {
    bT[lane * CFG + lane] = -1.0;
    for (int k = 0; k < nmj; k++) bT[lane * CFG + psi + perm[k]] = (k < np1) ? C[k * psi + lane] : 0.0;
  }
  sync();
  for (int e = lane; e < CFG * CFG; e += WAVE) {  // bbt = b b^T
    const int i = e / CFG, j = e % CFG;
    double s = 0;
    for (int k = 0; k < psi; k++) s += bT[k * CFG + i] * bT[k * CFG + j];
    bbt[e] = s;
  }
  sync();
  CPC_ACC(0);
  // ---- 3. compute_prox_loss_over_tps (cpc.cpp:151-190), lane = target point
  bool nonfinite = false;
  for (int base = 0; base < ntp; base += WAVE) {
    const int t = base + lane;
    const bool active = t < ntp;
    const double* __restrict__ row = tp + (size_t)(active ? t : 0) * rec;
    double v0[CFG], v1[CFG];  // qd, dqd; then del_q - dqd t0 / s, dqd / s - dq0
#pragma unroll
    for (int j = 0; j < CFG; j++) {
      v0[j] = (j < cfg) ? row[j] : 0.0;
      v1[j] = (j < cfg) ? row[cfg + j] : 0.0;
    }
    double denom = 0, num_t = 0, num_s = 0;  // btildt . dq0, btildt . del_q, btildt . dqd
#pragma unroll
    for (int i = 0; i < CFG; i++) {
      double bt = 0;  // btildt[i] = (bbt dqd)[i]
#pragma unroll
      for (int j = 0; j < CFG; j++) bt += bbt[i * CFG + j] * v1[j];
      denom += bt * dq0[i];
      num_t += bt * (v0[i] - q0[i]);
      num_s += bt * v1[i];
    }
    const double t0 = num_t / denom;
    const double s = num_s / denom;
#pragma unroll
    for (int i = 0; i < CFG; i++) {
      v0[i] = (v0[i] - q0[i]) - v1[i] * t0 / s;
      v1[i] = v1[i] / s - dq0[i];
    }
    double cc0 = 0, cc1 = 0;
    for (int k = 0; k < psi; k++) {
      double c0 = 0, c1 = 0;
#pragma unroll
      for (int i = 0; i < CFG; i++) {
        c0 += bT[k * CFG + i] * v0[i];
        c1 += bT[k * CFG + i] * v1[i];
      }
      cc0 += c0 * c0;
      cc1 += c1 * c1;
    }
    const double w0 = P.w * t0, w1 = s - P.sg;  // prox_loss (cpc.cpp:183-190)
    const double loss = w0 * w0 + w1 * w1 + P.loss_cc * (cc0 + cc1);
    if (active) {
      L[t] = loss;
      T0[t] = t0;
      S[t] = s;
      taken[t] = 0;
      if (a.loss) a.loss[(size_t)b * ntp + t] = loss;
      if (!(fabs(loss) <= DBL_MAX)) nonfinite = true;
    }
  }
  if (__any(nonfinite)) flags |= HS_CPC_FLAG_NONFINITE;
  sync();
  CPC_ACC(1);
  // ---- 4. candidates (cpc.cpp:252-272): n_cand rounds of a wave-wide minimum; key = (loss, tpi), a loss
  // that is not finite counts as +inf
  const bool s_goal = P.goal_t0s && (!P.tpdist_switch || low_in);
  for (int r = 0; r < nc; r++) {
    double bk = INFINITY;
    int bt = INT_MAX;
    for (int base = 0; base < ntp; base += WAVE) {
      const int t = base + lane;
      if (t < ntp && !taken[t]) {
        const double l = L[t];
        const double k = (fabs(l) <= DBL_MAX) ? l : INFINITY;
        if (k < bk || (k == bk && t < bt)) { bk = k; bt = t; }
      }
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
      const double ok = __shfl_xor(bk, d, WAVE);
      const int ot = __shfl_xor(bt, d, WAVE);
      if (ok < bk || (ok == bk && ot < bt)) { bk = ok; bt = ot; }
    }
    bt = __builtin_amdgcn_readfirstlane(bt);
    if (bt >= ntp) bt = 0;  // cannot happen: the caller has checked n_tp >= n_cand
    if (lane == 0) {
      ctpi[r] = bt;
      cl[r] = L[bt];
      ct0[r] = T0[bt];
      cs[r] = s_goal ? P.sg : S[bt];
      taken[bt] = 1;
    }
    sync();
  }
  if (lane < nc) {
    if (a.cand_tpi) a.cand_tpi[(size_t)b * nc + lane] = ctpi[lane];
    if (a.cand_t0s) {
      a.cand_t0s[((size_t)b * nc + lane) * 2] = ct0[lane];
      a.cand_t0s[((size_t)b * nc + lane) * 2 + 1] = cs[lane];
    }
  }
  CPC_ACC(2);
  // ---- 5. B_chi_dec.compute(B_chi), B_chi = Bt_chi^T (cpc.cpp:113, 227)
  for (int e = lane; e < nmj * nmj; e += WAVE) {
    const int r = e / nmj, c = e % nmj;
    qr[r + c * nmj] = Btb[c * cfg + psi + r];
  }
  const int np2 = hs_colpiv::factor(qr, nmj, nmj, nu, nd, hc, perm, lane);
  if (np1 < nmj || np2 < nmj) flags |= HS_CPC_FLAG_RANK;
  CPC_ACC(3);
  // ---- 6. the gain loop (cpc.cpp:229-237) over cost2 (cpc.cpp:339-362), lane = candidate
  const int ci = lane < nc ? lane : 0;
  const double* __restrict__ crow = tp + (size_t)ctpi[ci] * rec;
  const double t0 = ct0[ci], s = cs[ci];
  double k = P.k0, nbest = 0;
  int passes = 0, ib = 0;
  do {
    const double k2 = 2 * sqrt(k);
    if (lane < nc) {  // controls (cpc.cpp:280-293)
      for (int r = 0; r < nmj; r++) {
        const double chid = crow[psi + r], dchid = crow[cfg + psi + r];
        C[r * nc + lane] = k * (q0[psi + r] - chid + dchid * t0 / s) + k2 * (dq0[psi + r] - dchid / s);
      }
    }
    hs_colpiv::solve(qr, nmj, np2, hc, C, nc, lane);
    if (lane < nc) {
      for (int kk = 0; kk < nmj; kk++) {
        const int r = perm[kk];
        const double del = (kk < np2) ? -C[kk * nc + lane] : 0.0;
        taus[r * nc + lane] = crow[2 * cfg + r] + del;
      }
      double sq = 0;
      for (int r = 0; r < nmj; r++) sq += taus[r * nc + lane] * taus[r * nc + lane];
      norms[lane] = sqrt(sq);
    }
    sync();
    double mean_norm = 0, mean_loss = 0;
    for (int j = 0; j < nc; j++) {
      mean_norm += norms[j];
      mean_loss += cl[j];
    }
    mean_norm /= nc;
    mean_loss /= nc;
    double score_min = 1e10;
    int i_min = -1;
    for (int j = 0; j < nc; j++) {
      const double score = norms[j] / mean_norm + cl[j] / mean_loss;
      if (score < score_min) { i_min = j; score_min = score; }
    }
    if (i_min < 0) {  // the reference indexes column -1
      flags |= HS_CPC_FLAG_NOSCORE;
      i_min = 0;
    }
    ib = __builtin_amdgcn_readfirstlane(i_min);
    nbest = uniform(norms[ib]);
    k /= 2;
    passes++;
    sync();
  } while (k > P.kc && nbest > P.tauc);
  CPC_ACC(4);
  // ---- 7. last_cand, tp_dist_check (cpc.cpp:485-494)
  const int ltpi = ctpi[ib];
  double* sq = bbt;
  if (lane < 2 * cfg) {
    const double cur = lane < cfg ? q0[lane] : dq0[lane - cfg];
    const double d = cur - tp[(size_t)ltpi * rec + lane];
    sq[lane] = d * d;
  }
  sync();
  double dist2 = 0;
  for (int e = 0; e < 2 * cfg; e++) dist2 += sq[e];
  const bool low = sqrt(dist2) < P.tp_dist;
  // ---- 8. clip_norm(tau, tauc)
  if (lane < nmj) {
    double tq = taus[lane * nc + ib];
    if (nbest > P.tauc) tq *= (P.tauc / nbest);
    a.tau[(size_t)b * nmj + lane] = tq;
  }
  if (lane == 0) {
    a.last_tpi[b] = ltpi;
    a.flags[b] = flags;
    a.low_tpdist[b] = low ? 1 : 0;
    if (a.passes) a.passes[b] = passes;
    if (a.i_best) a.i_best[b] = ib;
  }
  CPC_ACC(5);
#ifdef HS_CPC_STAMPS
  if (lane == 0 && b < 4096) g_cpc_stamps[b][6] += passes;
#endif
}

// set_target_points_by_per (cpc.cpp:51-63), one lane per entry: row i = get_complete_traj_rec(i)
// (periodic.cpp:408-417) = table row (i + n_t - 2) % n_t, then apply_mask
__global__ __launch_bounds__(256) void hs_cpc_tp_kernel(int32_t n_rollouts, int32_t n_t, int32_t cfg, int32_t nmj,
                                                         const double* __restrict__ q_tab,
                                                         const double* __restrict__ dq_tab,
                                                         const double* __restrict__ tau_tab, uint32_t mask,
                                                         double* __restrict__ tp) {
  const int rec = 2 * cfg + nmj;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)n_rollouts * n_t * rec) return;
  const int c = (int)(e % rec);
  const long bi = e / rec;
  const int i = (int)(bi % n_t);
  const long b = bi / n_t;
  const size_t row = (size_t)b * n_t + (i + n_t - 2) % n_t;
  double v;
  if (c < 2 * cfg) {
    const int j = c < cfg ? c : c - cfg;
    v = (c < cfg ? q_tab : dq_tab)[row * cfg + j];
    if (j < 32 && ((mask >> j) & 1u)) v = 0.0;
  } else {
    v = tau_tab[row * nmj + (c - 2 * cfg)];
  }
  tp[e] = v;
}

// dst[b] = src[b] (width doubles) for the rollouts that took the step (still HS_TRIAL_RUNNING after it)
__global__ __launch_bounds__(256) void hs_cpc_rows_kernel(int32_t n_rollouts, int32_t width,
                                                           const int32_t* __restrict__ state,
                                                           const double* __restrict__ src, double* __restrict__ dst) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)n_rollouts * width) return;
  if (state[e / width] == HS_TRIAL_RUNNING) dst[e] = src[e];
}

// a rollout frozen before the step keeps the seed it had before the step's estimate
__global__ __launch_bounds__(256) void hs_cpc_keep_seed_kernel(int32_t n_rollouts, const int32_t* __restrict__ state,
                                                                const uint32_t* __restrict__ saved,
                                                                uint32_t* __restrict__ seed) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_rollouts && state[b] != HS_TRIAL_RUNNING) seed[b] = saved[b];
}

}  // namespace

namespace hs {

static int cpc_pad(int32_t cfg) { return cfg <= 24 ? 24 : 32; }

size_t cpc_lds_bytes(int32_t n_tp, int32_t n_cand, int32_t nmj, int32_t cfg) {
  return cpc_lds(cpc_pad(cfg), cfg, nmj, n_cand, n_tp).bytes();
}

int launch_cpc_torques(const hs_cpc_args& a, int32_t nmj, int32_t cfg) {
  if (a.n_rollouts <= 0) return 0;
  if (cfg > 32 || nmj < 1 || nmj >= cfg) return (int)hipErrorInvalidValue;
  const size_t lds = cpc_lds_bytes(a.n_tp, a.params.n_cand, nmj, cfg);
  hipStream_t st = (hipStream_t)a.stream;
  if (cpc_pad(cfg) == 24)
    hipLaunchKernelGGL(hs_cpc_kernel<24>, dim3(a.n_rollouts), dim3(WAVE), lds, st, a, nmj, cfg);
  else
    hipLaunchKernelGGL(hs_cpc_kernel<32>, dim3(a.n_rollouts), dim3(WAVE), lds, st, a, nmj, cfg);
  return (int)hipGetLastError();
}

int launch_cpc_target_points(int32_t n, int32_t n_t, int32_t cfg, int32_t nmj, const double* q_tab, const double* dq_tab,
                             const double* tau_tab, uint32_t mask, double* tp, void* stream) {
  if (n <= 0 || n_t <= 0) return 0;
  const long total = (long)n * n_t * (2 * cfg + nmj);
  hipLaunchKernelGGL(hs_cpc_tp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, n_t,
                     cfg, nmj, q_tab, dq_tab, tau_tab, mask, tp);
  return (int)hipGetLastError();
}

int launch_cpc_rows(int32_t n, int32_t width, const int32_t* state, const double* src, double* dst, void* stream) {
  if (n <= 0 || width <= 0) return 0;
  const long total = (long)n * width;
  hipLaunchKernelGGL(hs_cpc_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     width, state, src, dst);
  return (int)hipGetLastError();
}

int launch_cpc_keep_seed(int32_t n, const int32_t* state, const uint32_t* saved, uint32_t* seed, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(hs_cpc_keep_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     state, saved, seed);
  return (int)hipGetLastError();
}

}  // namespace hs

#ifdef HS_CPC_STAMPS
extern "C" int hs_debug_read_cpc_stamps(unsigned long long* out, int n_rows) {
  if (n_rows > 4096) n_rows = 4096;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cpc_stamps), sizeof(unsigned long long) * 8 * n_rows, 0,
                                  hipMemcpyDeviceToHost);
}
extern "C" int hs_debug_clear_cpc_stamps() {
  static unsigned long long zero[4096][8];
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_cpc_stamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice);
}
#endif
