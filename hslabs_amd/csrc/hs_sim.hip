// hs_sim.hip -- hs_sim_step's unit of the closed-loop simulation: the plain instantiations of the
// simulation kernel (hs_sim_kernel.h, which describes the step), the reset of a batch of worlds to a
// configuration, and the readers of the diagnostic build's phase stamps. The fall test's and the probes'
// instantiations are units of their own (hs_sim_trial.hip, hs_sim_probe.hip; the header says why). Built
// with -ffp-contract=off (hslabs_amd/build.py).
#include "hs_sim_kernel.h"

namespace {

// init_play_config + orient_odebodys: lane = part, A_ground by walking the chain from the root
// (each product in the reference's order: J_A_ground = A_parent J_A_parent, then * E(q) * A_pj_body).
// IO = the precision of the configuration and body arrays; the pose is built in double and
// rounded once into a float state for the single-precision simulation.
template <class IO>
__global__ __launch_bounds__(WAVE) void hs_sim_reset_kernel(const hs_topo* __restrict__ T, const hs_simtopo* __restrict__ S,
                                                             int32_t n_rollouts, const IO* __restrict__ config,
                                                             int32_t stride, IO* __restrict__ body) {
  using namespace hsd;
  const int b = blockIdx.x, p = threadIdx.x;
  if (b >= n_rollouts || p >= T->n) return;
  double cf[6 + HS_NMAX];
  for (int i = 0; i < T->cfg; i++) cf[i] = (double)config[(size_t)b * stride + i];
  int chain[HS_NMAX], len = 0;
  for (int a = p; a >= 0; a = T->node[a].parent) chain[len++] = a;
  A34 A;
  for (int i = 0; i < 12; i++) A.m[i] = (i % 4 == 0) ? 1.0 : 0.0;  // unity (columns 0..2 of I, zero translation)
  for (int k = len - 1; k >= 0; k--) {
    const hs_node& nd = T->node[chain[k]];
    if (nd.jtype == HS_J_FREE) {
      A34 JA = mul(A, load34(nd.J_A_parent));
      A = mul(mul(JA, free_joint(cf)), load34(nd.A_pj_body));
    } else if (nd.jtype == HS_J_HINGE) {
      A34 JA = mul(A, load34(nd.J_A_parent));
      A = mul(mul(JA, hinge_joint(cf[6 + nd.hinge])), load34(nd.A_pj_body));
    } else {
      A = mul(A, load34(nd.A_pj_body));
    }
  }
  A34 G = mul(A, load34(S->body_geom[p]));
  double Rin[12], q[4], R[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Rin[r * 4 + c] = G(r, c);
    Rin[r * 4 + 3] = 0;
  }
  q_from_R(q, Rin);
  normalize4(q);
  IO* o = body + ((size_t)b * T->n + p) * HS_SIM_BODY;
  for (int i = 0; i < 3; i++) o[i] = (IO)G(i, 3);
  for (int i = 0; i < 4; i++) o[3 + i] = (IO)q[i];
  for (int i = 7; i < 13; i++) o[i] = 0;
  (void)R;
}

}  // namespace

#ifdef HS_SIM_STAMPS
extern "C" int hs_debug_read_sim_stamps(unsigned long long* out, int n_rows) {
  if (n_rows > 4096) n_rows = 4096;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sim_stamps), sizeof(unsigned long long) * 16 * n_rows, 0,
                                  hipMemcpyDeviceToHost);
}
extern "C" int hs_debug_clear_sim_stamps() {
  static unsigned long long zero[4096][16];
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_sim_stamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice);
}
#endif

namespace hs {

int launch_sim_reset(const sim_dev& dv, int32_t n_rollouts, const double* config, int32_t config_stride, double* body,
                     int32_t precision, void* stream) {
  if (n_rollouts <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (precision == HS_PREC_F32)
    hipLaunchKernelGGL(hs_sim_reset_kernel<float>, dim3(n_rollouts), dim3(WAVE), 0, st, dv.topo, dv.sim, n_rollouts,
                       reinterpret_cast<const float*>(config), config_stride, reinterpret_cast<float*>(body));
  else
    hipLaunchKernelGGL(hs_sim_reset_kernel<double>, dim3(n_rollouts), dim3(WAVE), 0, st, dv.topo, dv.sim, n_rollouts,
                       config, config_stride, body);
  return (int)hipGetLastError();
}

// (ahead of the launcher: the code object lists the kernels in the order the unit first names them, and
// this keeps it class by class, fp64 first)
int sim_step_occupancy(int32_t n, int32_t m_max, int32_t* out3) { return sim_occupancy<false>(n, m_max, out3); }

int launch_sim_steps(const sim_dev& dv, const hs_sim_args& a) { return launch_sim<false>(dv, a); }

}  // namespace hs
