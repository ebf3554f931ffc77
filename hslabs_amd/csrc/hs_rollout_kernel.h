// hs_rollout_kernel.h -- the 32-lanes-per-rollout step kernel (hs_rollout_kernel), the call's preparation
// pass (hs_prep_kernel) and their launchers.
//
// Two rollouts per wavefront (one 64-thread workgroup), 32 lanes each. Per
// rollout the half-wave
//   S  sets up the gait (pgssweeper::setup_pergen, pergen.cpp:453-507),
//   K  samples the trajectory: lane = (sample, limb) runs pergen set_rec
//      (pergen.cpp:225-239), the torso/body chain FK, limb IK (lik.cpp:151-223,
//      316-347) and the limb FK (model.cpp:183-201), and writes the dynamic
//      features of the parts it owns (dynrec.cpp:134-155) to LDS,
//   D  lane = part: 5-point finite differences (dynrec.cpp:175-224),
//   S1 lane = part, leaves -> root: particular solution of B0 x = f
//      (replaces the SparseQR solve of ftsolver.cpp:107-113 by the tree
//      back-substitution B0's block-triangular structure allows),
//   S3 the lexicographic least squares of ftsolver.cpp:185-236 in closed form
//      (one lane per contact + a 6x6 Schur complement); a conditioning guard
//      sends the step to the out-of-line Eigen-style FullPivLU/ColPivQR path
//      (tree-built null basis, Gram matrices in a global-memory workspace),
//   S4 motor torques, contact forces and positive work (periodic.cpp:261-343).
// (The LDS layout and the rounding against the oracle: hs_step_base.h.)
#pragma once
#include "hs_step_base.h"
#include "hs_step_kin.h"
#include "hs_step_solve.h"

namespace {

// ---------------------------------------------------------------------------
// One control-loop step at centre sample i (row = b * H + h of the outputs)
// ---------------------------------------------------------------------------
// DEFER: a step the closed form declines is not solved here but handed to the fixup launch (the
// step's half-wave stores nothing and `deferred` is set), so this instantiation has no call to the
// out-of-line general path: the call alone costs the whole kernel SGPRs (spills in the hot solve
// region) and 2.4 % of the step time
// dt (SetupL::dt) is loaded at the wave's start (a value read from the setup record later would be read
// again after every output store, which may alias it)
template <bool DEFER, class W, class SV>
__device__ __attribute__((always_inline)) inline void step(const hs_topo* T, const hs_run_args& a, const hs::launch_map& mp, real dt, SV& sv,
                     FastL& fl, const W& w, SolveWS* G, int b, bool live, int h,
                     real& work, bool& deferred, bool may_general, int lane) {
  const int n = T->n, nmj = T->nmj, nf = T->nf, cfg = T->cfg, nl = T->n_limbs;
  STAMP(3);
  // D writes, and S1's first stage reads, part i's rows on lane i only: no sync between them
  dynamics<false>(T, dt, sv, w, lane);
  STAMP(4);
  particular_sub(T, sv, w, lane);
  STAMP(5);
  // contact list in foot order (ftsolver contact columns)
  const uint32_t cmask = half_ballot(lane < nf && w.contact(0, lane));
  const int nc = __popc(cmask);
  if (lane < nf && ((cmask >> lane) & 1)) sv.cfoot[__popc(cmask & ((1u << lane) - 1))] = lane;
  wave_sync();
  int k = 3 * nc;
  uint32_t flags = 0;
  STAMP(6);
  // tier 2 (aug_solve) and the general path share the rollout's global workspace (SolveWS): the
  // general path runs only after tier 2 declined. may_general = false (the fixup's idle half) skips both
  bool fast_near = false;
  if (a.solve_mode == HS_SOLVE_AUTO && fast_solve(T, sv, fl, G->aug, w, nc, may_general, lane, fast_near)) {
    if (nc == 0) flags |= HS_FLAG_NO_CONTACT;
    if (nc == 1) flags |= HS_FLAG_FULL_RANK;
  } else {
    if constexpr (DEFER) {
      deferred = true;  // uniform over the half-wave: its outputs come from the fixup launch
      live = false;
    } else if (may_general) {
      flags = general_solve(T, sv, G->gen, w, k, lane) | HS_FLAG_GENERAL;
    }
  }
  if (fast_near) flags |= HS_FLAG_NEAR_RANK;  // the closed form's routing itself was a near decision
  STAMP(7);

  // S4: x = x_part + N y for the hinge torque rows, motor torques (periodic.cpp:328-343),
  // and the step's positive work (compute_vel_traj + work_over_period, periodic.cpp:261-307)
  const size_t row = (size_t)b * a.horizon + h;
  real tq = real(0);
  real* const wd = reinterpret_cast<WorkL&>(fl).wd;  // FastL is dead once y is known
  if (lane < nmj) {
    const int h_id = T->hinge_ids[lane], fi = T->hinge_foot[lane];  // this lane's motor's part and foot
    // contact index of foot fi: its rank among the feet down (the contact list's order)
    const int cc = (fi >= 0 && ((cmask >> fi) & 1)) ? __popc(cmask & ((1u << fi) - 1)) : -1;
    const real* Jp = w.jpos(0, h_id);
    const real* Jz = w.jz(0, h_id);
    // every operand read in one batch, without branches (a hinge with no foot in contact takes y = 0:
    // its terms are exact zeros, s stays +0 as when they were skipped)
    const real* fp = w.fpos(0, fi >= 0 ? fi : 0);
    const int yb = cc >= 0 ? 3 * cc : 0;
    real d[3], y3[3];
#pragma unroll
    for (int rr = 0; rr < 3; rr++) {
      d[rr] = Jp[rr] - fp[rr];
      const real yv = sv.y[yb + rr];
      y3[rr] = cc >= 0 ? yv : real(0);
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      real s = real(0);
#pragma unroll
      for (int jj = 0; jj < 3; jj++)
        if (jj != r) s = s + cross_e(d, jj, r) * y3[jj];  // (d x e_r)[r] = 0: skipped
      real xr = sv.x[3 * n + 3 * h_id + r] + s;
      tq = tq + Jz[r] * xr;
    }
    real dd = w.q(1)[6 + lane] - w.q(-1)[6 + lane];
    if (dd > kPi) dd -= 2 * kPi;
    else if (dd < -kPi) dd += 2 * kPi;
    real jvel = dd / (2 * dt);
    real dw = tq * jvel;
    wd[lane] = (dw > 0) ? dw : 0;
    if (mp.pd_tau && live) {  // linear_feedback_control (player.cpp:417-432), target = get_motor_adas
      const size_t o = row * mp.st_tau + lane;
      const real q0 = w.q(0)[6 + lane];
      real a1 = inp(mp.pd_q)[o] - q0;
      if (a1 > kPi) a1 -= 2 * kPi;  // arrayops::modulus(., 2 pi) (core.cpp:122-131)
      else if (a1 <= -kPi) a1 += 2 * kPi;
      a1 *= mp.pd_k1;
      real a2 = inp(mp.pd_dq)[o] - jvel;
      a2 *= mp.pd_k2;
      a1 += a2;
      outp(mp.pd_tau)[o] = tq + a1;
      if (mp.pd_q0) outp(mp.pd_q0)[o] = q0;
      if (mp.pd_dq0) outp(mp.pd_dq0)[o] = jvel;
    }
  }
  if (live && a.tau && lane < mp.st_tau) outp(a.tau)[row * mp.st_tau + lane] = tq;  // 0 past nmj
  if (half_ballot(lane < nmj && tq != tq) || half_ballot(lane < k && sv.y[lane] != sv.y[lane])) flags |= HS_FLAG_NAN;
  if (half_ballot(lane < nl && w.unreach(0, lane))) flags |= HS_FLAG_UNREACH;
  // contact forces z = -N_cont y (ftsolver.cpp:91, 276-284)
  if (live && a.cf && lane < mp.st_cf) {
    const int fi = lane / 3, j = lane % 3;
    real zv = (lane < 3 * nf) ? -real(0) : real(0);
    if (lane < 3 * nf && ((cmask >> fi) & 1)) zv = -(real(0) + (real(-1)) * sv.y[3 * __popc(cmask & ((1u << fi) - 1)) + j]);
    outp(a.cf)[row * mp.st_cf + lane] = zv;
  }
  if (live && a.x) {  // full joint force/torque vector x += N y
    for (int rI = lane; rI < 6 * n; rI += HALF) {
      int part = (rI < 3 * n) ? rI / 3 : (rI - 3 * n) / 3, comp = rI % 3;
      real s = real(0);
      for (int c = 0; c < nc; c++) {
        int foot = T->footis[sv.cfoot[c]];
        bool anc = false;
        for (int aa = foot; aa >= 0; aa = T->node[aa].parent) anc |= (aa == part);
        if (!anc) continue;
        if (rI < 3 * n) {
          s = s + (real(-1)) * sv.y[3 * c + comp];
        } else {
          const real* ref = (T->node[part].parent >= 0) ? w.jpos(0, part) : w.pos(0, part);
          const real* fp = w.fpos(0, sv.cfoot[c]);
          real d[3];
          for (int rr = 0; rr < 3; rr++) d[rr] = ref[rr] - fp[rr];
          for (int jj = 0; jj < 3; jj++) s = s + cross_e(d, jj, comp) * sv.y[3 * c + jj];
        }
      }
      outp(a.x)[row * mp.st_x + rI] = sv.x[rI] + s;
    }
    for (int rI = 6 * n + lane; rI < mp.st_x; rI += HALF) outp(a.x)[row * mp.st_x + rI] = real(0);
  }
  if (live && a.q && lane < mp.st_q) outp(a.q)[row * mp.st_q + lane] = (lane < cfg) ? w.q(0)[lane] : real(0);
  if (live && a.dq && lane < mp.st_q) {  // compute_vel_traj (periodic.cpp:261-282)
    real v = real(0);
    if (lane < cfg) {
      real d = w.q(1)[lane] - w.q(-1)[lane];
      if (d > kPi) d -= 2 * kPi;
      else if (d < -kPi) d += 2 * kPi;
      v = d / (2 * dt);
    }
    outp(a.dq)[row * mp.st_q + lane] = v;
  }
  if (live && a.flags && lane == 0) a.flags[row] = flags;
  // the joints' positive work summed in joint order, as work_over_period's loop does (periodic.cpp:
  // 294-300; a DPP tree sum rounds differently, which can reorder near-tied rollouts' COTs)
  wave_sync();
  real work_dt = real(0);
  for (int jj = 0; jj < nmj; jj++) work_dt += wd[jj];
  // work_over_period: work_dt *= dt; work += work_dt (two roundings, periodic.cpp:301-302); fused steps
  // hand back the joint sum itself and the reduce performs the same two operations in step order
  if (mp.fused_w) work = work_dt;
  else work = work_add(work, work_dt, dt);
  STAMP(8);
  RSTAMP(17);
}

template <class W, class SV>
__device__ __attribute__((always_inline)) inline void forces_step(const hs_topo* T, const hs_run_args& a, const hs::launch_map& mp, real dt,
                            SV& sv, ForceL& fr, const W& w, int b, bool live, int h, int lane) {
  const int nf = T->nf, cfg = T->cfg, nl = T->n_limbs, nq = 3 * nf;
  dynamics(T, dt, sv, w, lane);
  // the control step's subtree sums (round 6: the level-by-level recursion summed x in another order,
  // so the forces mode's x differed from the control step's -- and the limb-lane kernel's -- by rounding)
  particular_sub(T, sv, w, lane);
  wave_sync();  // particular_sub leaves x unsynchronised across lanes; forces_solve reads it across lanes
  STAMP(10);
  const size_t row = (size_t)b * a.horizon + h;
  const real* z = inp(mp.tau_in) + (live ? row : 0) * mp.st_tau;
  uint32_t flags = forces_solve(T, sv, fr, w, z, a.solve_mode == HS_SOLVE_REFERENCE, lane);
  if (half_ballot(lane < nq && sv.y[lane] != sv.y[lane])) flags |= HS_FLAG_NAN;
  if (half_ballot(lane < nl && w.unreach(0, lane))) flags |= HS_FLAG_UNREACH;
  if (live && a.cf && lane < mp.st_cf) outp(a.cf)[row * mp.st_cf + lane] = (lane < nq) ? sv.y[lane] : real(0);
  if (live && a.q && lane < mp.st_q) outp(a.q)[row * mp.st_q + lane] = (lane < cfg) ? w.q(0)[lane] : real(0);
  if (live && a.flags && lane == 0) a.flags[row] = flags;
  STAMP(11);
}

// ---------------------------------------------------------------------------
// The call's preparation pass (hs_prep_kernel): the gait setup of every rollout (pergensetup::
// setup_pergen, pergen.cpp:453-507), its sample times (periodic.cpp:171-181) and the IK table of the
// samples the call's steps read (with, for turning or transformed gaits, the torso record) -- in one launch.
//
// Lane = (rollout, limb L, chunk of HS_PREP_ROWS table rows). Every lane runs its limb's setup (torso
// frame, chain, hip frame J0, default foot position, lift-off entries) itself -- the lanes of one
// wavefront do it in the same instructions, so the repetition costs one pass per wavefront -- and then
// the rows of its chunk: the sample time, and for a straight gait J = J0 advanced by t v along the
// torso's x and the limb IK at the foot target (straight_ik's operations); for a turning or transformed
// gait kin_sample's record, torso FK, chain and limb IK, the torso's q6 and frame stored per row
// (RolloutWS::ktor, lane L = 0). The chunk-0 lanes store the
// setup record; max_radius (compute_max_radius, curved gaits) is the maximum over a rollout's limb
// lanes, exchanged in LDS. A rollout's limb lanes form a group that never crosses a wavefront (groups of
// nli lanes, floor(64 / nli) per wavefront). XCD-aware: block 8 jb + x runs groups of batch wavefronts
// w = x (mod 8), whose step launches run on XCD x (blocks are dealt round-robin over the 8 XCDs,
// MI355X_MICROARCH.md), so the record and rows are written into the L2 the steps read them from.
// ---------------------------------------------------------------------------
#ifndef HS_PREP_ROWS
#define HS_PREP_ROWS 5  // table rows per lane (round 4, B = 4096, 24 rows: 3, 4, 5, 6, 8 rows give 24.1, 25.0, 23.4, 24.9, 29.7 us)
#endif
#ifndef HS_PREP_WAVES
#define HS_PREP_WAVES 2  // waves per SIMD (251 VGPRs, 255 mixed, no scratch; at 3, 168 VGPRs and 336 B of spills: tools/isa_stats.py)
#endif
#ifndef HS_PREP_WPB
#define HS_PREP_WPB 4  // wavefronts per workgroup (each a group of lanes of its own: only wave-local exchanges);
                       // 4: the pass's wavefronts start sooner, 22.9 -> 20.5 us per driver job (r05_ab_t2.txt)
#endif
// an exchange through LDS among the lanes of one wavefront: LDS operations of a wavefront complete in
// order, so only the compiler must not move the accesses across it (no s_barrier: with several
// wavefronts per workgroup they take different paths)
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ inline int ktab_lanes(const hs::launch_map& mp) { return mp.ktab_nl > 0 ? mp.ktab_nl : HS_LMAX; }
__host__ __device__ inline int prep_chunks(int ttab_n) { return (ttab_n > 0 ? ttab_n + HS_PREP_ROWS - 1 : HS_PREP_ROWS) / HS_PREP_ROWS; }
// XCD units of the pass: prep_unit rollouts each (2: hs_rollout_kernel's wavefronts, 8: the limb kernel's)
__host__ __device__ inline int prep_units(const hs::launch_map& mp, int n_rollouts, int& R) {
  R = mp.prep_unit > 2 && !mp.wave_rollouts ? mp.prep_unit : 2;
  return R == 2 ? mp.n_waves : (n_rollouts + R - 1) / R;
}
__host__ __device__ inline int64_t prep_blocks(int n_units, int R, int ttab_n, int nli) {
  const int64_t groups_per_xcd = R * (int64_t)prep_chunks(ttab_n) * ((n_units + 7) / 8);
  const int gpw = WAVE / nli;
  const int64_t waves_per_xcd = (groups_per_xcd + gpw - 1) / gpw;
  return 8 * ((waves_per_xcd + HS_PREP_WPB - 1) / HS_PREP_WPB);
}

// MIXED: a mixed-topology launch (launch_map::wave_model), whose lane groups of one wavefront may hold
// different models; otherwise the topology pointer is the kernel argument itself, wave-uniform, so its
// rollout-independent entries come through the scalar cache
template <bool MIXED>
__global__ __launch_bounds__(WAVE * HS_PREP_WPB, HS_PREP_WAVES) void hs_prep_kernel(const hs_topo* __restrict__ T0,
                                                                   hs_run_args a, RolloutWS* __restrict__ rws,
                                                                   hs::launch_map mp) {
  __shared__ real rad_s[HS_PREP_WPB][WAVE];
  __shared__ real q6s_s[HS_PREP_WPB][HS_PREP_ROWS + 1][6][WAVE / 4];  // turning rows: [slot][q6 entry][group] (>= 4 limbs)
  __shared__ real tgs_s[HS_PREP_WPB][HS_PREP_ROWS + 1][3][WAVE];  // [slot][target entry, then joint value][lane]
  const int wv = (int)threadIdx.x / WAVE, tl = (int)threadIdx.x % WAVE;  // wavefront in the block, its lane
  real(&rad)[WAVE] = rad_s[wv];
  real(&q6s)[HS_PREP_ROWS + 1][6][WAVE / 4] = q6s_s[wv];
  real(&tgs)[HS_PREP_ROWS + 1][3][WAVE] = tgs_s[wv];
  RSTAMP(29);
  STAMP(24);
  if (blockIdx.x == 0)  // the call's fixup counters, before its step launches append to them
    for (int i = threadIdx.x; i < mp.fix_n_counts; i += blockDim.x) mp.fix_count[i] = 0;
  const int nli = ktab_lanes(mp), gpw = WAVE / nli;
  const int C = prep_chunks(mp.ttab_n);
  const int gl = tl / nli, L = tl % nli;
  // group (q, sub, chunk) in XCD x's sequence (x = blockIdx.x % 8: the block's XCD)
  const int gi = ((int)(blockIdx.x / 8) * HS_PREP_WPB + wv) * gpw + gl;
  int R;
  const int n_units = prep_units(mp, a.n_rollouts, R);
  const int chunk = gi % C, sub = (gi / C) % R, w = 8 * (gi / (R * C)) + (int)(blockIdx.x % 8);
  bool on = gl < gpw && w < n_units;
  int b = 0;
  const hs_topo* __restrict__ T = T0;
  if (on) {
    b = mp.wave_rollouts ? mp.wave_rollouts[2 * w + sub] : R * w + sub;
    if (MIXED) T = T0 + mp.wave_model[w];
    on = b >= 0 && b < a.n_rollouts && L < T->n_limbs;
  }
  GaitR g;
  A34 J0;
  real pos0[3], ts = 0, xs = 0, t_step = 0, dt = 0, v = 0;
  bool straight = false;
  real my_rad = 0;
  SC3 tsc;
  RolloutWS* __restrict__ ws = rws + b;
  LimbPlan plan;
  if (on) {
    plan = load_plan(T, L);  // issued before the gait parameters: its waits do not queue behind them
    g = load_gait(a.params[b]);
    straight = g.curvature == 0 && !g.rec_xf;  // kin_sample's turning / record-transform test
    const int nl = T->n_limbs, j = T->limb_pergen[L];
    tsc = sincos3(g.torso_angles[0], g.torso_angles[1], g.torso_angles[2]);
    const A34 A0 = torso_frame(T, g, tsc);
    limb_setup(T, g, A0, L, plan, J0, pos0, chunk == 0 ? &ws->kf : nullptr);
    t_step = step_fraction(g, nl);
    lift_off(nl, j, t_step, ts, xs);
    v = g.step_length / g.period;  // pergensetup::set_TLh
    dt = g.period / a.n_t;         // record_trajectory
    if (chunk == 0) {
      SetupL& st = ws->st;
      for (int i = 0; i < 3; i++) st.pos0[j][i] = pos0[i];
      st.ts[j] = ts;
      st.xs[j] = xs;
      if (L == 0) {
        st.t_step = t_step;
        st.v = v;
        st.dt = dt;
        st.tsc = tsc;
        const real com0[3] = {(real)T->node[0].com[0], (real)T->node[0].com[1], (real)T->node[0].com[2]};
        store_body(A0, com0, ws->kf.torso, 6);
      }
    }
    if (g.curvature != 0) my_rad = turn_radius(pos0, g.curvature);
  }
  STAMP(25);
  rad[tl] = my_rad;
  wave_lds_sync();
  real mr = 0;  // compute_max_radius over the rollout's limbs (every lane: turning rows read it)
  if (on && g.curvature != 0)
    for (int l = 0; l < T->n_limbs; l++) {
      const real r = rad[tl - L + l];
      if (r > mr) mr = r;
    }
  if (on && chunk == 0 && L == 0) ws->st.max_radius = mr;
  STAMP(26);
  if (!on) return;
  const int r0 = chunk * HS_PREP_ROWS, r1 = min(r0 + HS_PREP_ROWS, mp.ttab_n);
  if (r0 >= r1) return;
  const bool table = mp.ktab_n > 0;
  const hs_aff34& Jp0 = T->node[0].J_A_parent;
  const real u[3] = {(real)Jp0.m[0], (real)Jp0.m[1], (real)Jp0.m[2]};
  const real ls[3] = {(real)T->ls[0], (real)T->ls[1], (real)T->ls[2]};
  const int kind = T->lik_kind;
  const bool ir = a.ignore_reach != 0;
  // The joint rates of a chunk's first and last row (RolloutWS::kvel) read the neighbouring chunks' rows
  // next to them. Chunks c - 1 and c + 1 of a rollout are the lane groups gl - 1 and gl + 1 of this wavefront
  // (chunk = gi % C, gi consecutive in a wavefront), which leave their rows in LDS -- unless this group is the
  // wavefront's first or last: then the lane computes that one row itself (hrow: the halo row, its time the
  // same sum of dt), in one more turn of the row loop, taken only by the wavefronts that hold such a group
  // (none at C = 5 chunks and ten groups, the hexapod's 24-row calls). A lane has at most one halo row
  // (gpw >= WAVE / HS_LMAX groups).
  const int n = r1 - r0;
  const bool rates = table && mp.ktab_rates != 0;  // the call has a reader of kvel and kbig
  const int hrow = !rates ? -1 : (gl == 0 && r0 > 0 ? r0 - 1 : (gl == gpw - 1 && r1 < mp.ttab_n ? r1 : -1));
  const int nit = n + (__any(hrow >= 0) ? 1 : 0);
  // slot: a row's place in the wavefront's LDS arrays, the chunk's rows in order, then the halo row
  auto store_row = [&](int slot, int r, const real* ja, bool bad) {
    if (rates) {
#pragma unroll
      for (int kk = 0; kk < 3; kk++) tgs[slot][kk][tl] = ja[kk];
    }
    if (slot == HS_PREP_ROWS) return;  // a halo row: its own chunk's lane stores it
    real* e = ws->ktab[r][L];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) e[kk] = ja[kk];
    ws->kbad[r][L] = bad ? 1 : 0;
  };
  real t = sample_time_sum(dt, mp.ktab_lo + r0);
  // kin_sample's foot target, hip frame and limb IK at samples ktab_lo + r, one loop per kind of gait
  // (a lane's kind is fixed: the other loop's values are not live in this one)
  if (!table || straight) {
#pragma unroll 1
    for (int it = 0; it < nit; it++) {
      const bool mine = it < n;
      const int r = mine ? r0 + it : hrow, slot = mine ? it : HS_PREP_ROWS;
      if (r < 0) continue;
      if (!mine) t = sample_time_sum(dt, mp.ktab_lo + r);
      else if (it > 0) t += dt;  // the loop's next addition
      if (L == 0 && mine) ws->t_tab[r] = t;
      if (table) {  // straight_ik's: J = J0 advanced by t v
        real dx, dz;
        limb_step(g, t, ts, xs, t_step, dx, dz);
        const real target[3] = {dx + pos0[0], real(0) + pos0[1], dz + pos0[2]};
        real ja[3];
        bool bad;
        hip_ik_k(frame_at(J0, u, t * v), target, kind, ls, plan.ysign, ir, ja, bad);
        store_row(slot, r, ja, bad);
      }
      if (it == 0) STAMP(27);
    }
  } else {
    // turning or transformed gaits (kin_sample's sequence), in two passes over the rows so that the gait
    // record's values and the FK + IK's are not live together: (1) the record: the torso's q6 (lane L = 0,
    // per group) and the foot targets to LDS; (2) the torso FK (free_joint: sincos of the configured
    // angles when not turned, as free_joint_sc with the setup's), the chain, the hip frame, the limb IK
    // (whose joint values take the targets' place in LDS)
    const LimbRec rl{v, t_step, mr, ts, xs, {pos0[0], pos0[1], pos0[2]}, tsc};
    const hs_gait_params& gp = a.params[b];
#pragma unroll 1
    for (int it = 0; it < nit; it++) {
      const bool mine = it < n;
      const int r = mine ? r0 + it : hrow, slot = mine ? it : HS_PREP_ROWS;
      if (r < 0) continue;
      if (!mine) t = sample_time_sum(dt, mp.ktab_lo + r);
      else if (it > 0) t += dt;
      if (L == 0 && mine) ws->t_tab[r] = t;
      real o0[3], o1[3], target[3];
      bool turned;
      gait_record<false>(g, gp, rl, t, o0, o1, turned, target);
      if (L == 0) {
        const real q6[6] = {o0[0], o0[1], o0[2], o1[0], o1[1], o1[2]};
        for (int i = 0; i < 6; i++) q6s[slot][i][gl] = q6[i];
      }
      for (int i = 0; i < 3; i++) tgs[slot][i][tl] = target[i];
    }
    wave_lds_sync();
#pragma unroll 1
    for (int it = 0; it < nit; it++) {
      const bool mine = it < n;
      const int r = mine ? r0 + it : hrow, slot = mine ? it : HS_PREP_ROWS;
      if (r < 0) continue;
      real q6[6], target[3];
      for (int i = 0; i < 6; i++) q6[i] = q6s[slot][i][gl];
      for (int i = 0; i < 3; i++) target[i] = tgs[slot][i][tl];
      const A34 A0 = mul(mul(node_joint_parent(T, 0), free_joint(q6)), node_pj(T, 0));
      if (L == 0 && mine) {  // the torso record the step launches read (kin_sample_tab)
        real* tr = ws->ktor[r];
        for (int i = 0; i < 6; i++) tr[i] = q6[i];
        store34r(A0, tr + 6);
      }
      A34 A = A0;
      for (int k = 1; k < T->limb_chain_len[L]; k++) A = mul(A, node_pj(T, T->limb_chain[L][k]));
      real ja[3];
      bool bad;
      hip_ik(T, L, mul(A, node_joint_parent(T, T->limb_child[L])), target, ir, ja, bad);
      store_row(slot, r, ja, bad);
      if (it == 0) STAMP(27);
    }
  }
  if (rates) {
    // the rows' range bits, and the joint rates of the rows with both neighbours in the call's range: row
    // r - 1, r, r + 1's joint values from LDS (this lane's slots; the neighbouring chunks' last and first slot
    // on lanes tl - nli and tl + nli, or this lane's halo slot)
    wave_lds_sync();
    real qm[3] = {0, 0, 0}, q0[3], qp[3] = {0, 0, 0};
    const bool lane_m = hrow == r0 - 1, lane_p = hrow == r1;  // (r0 - 1 = -1: chunk 0, no row before it)
    if (r0 > 0)
      for (int kk = 0; kk < 3; kk++) qm[kk] = lane_m ? tgs[HS_PREP_ROWS][kk][tl] : tgs[HS_PREP_ROWS - 1][kk][tl - nli];
    for (int kk = 0; kk < 3; kk++) q0[kk] = tgs[0][kk][tl];
#pragma unroll 1
    for (int it = 0; it < n; it++) {
      const int r = r0 + it;
      const bool next = r + 1 < mp.ttab_n;
      if (next)
        for (int kk = 0; kk < 3; kk++)
          qp[kk] = it + 1 < n ? tgs[it + 1][kk][tl] : (lane_p ? tgs[HS_PREP_ROWS][kk][tl] : tgs[0][kk][tl + nli]);
      bool big = false;
      for (int kk = 0; kk < 3; kk++) big |= sincos_big(q0[kk]);
      ws->kbig[r][L] = big ? 1 : 0;
      if (r > 0 && next) {
        real* e = ws->kvel[r][L];
        for (int kk = 0; kk < 3; kk++) e[kk] = wrap_rate(qp[kk], qm[kk], dt);
      }
      for (int kk = 0; kk < 3; kk++) qm[kk] = q0[kk], q0[kk] = qp[kk];
    }
  }
  STAMP(28);
  RSTAMP(30);
}

// One wavefront's step: fused step fstep (0 outside fused launches) of batch wavefront wid. only_sub
// >= 0 (the fixup launch): only that half stores, the other computes a copy and stores nothing.
template <int NM, bool FORCES, bool DEFER>
__device__ __attribute__((always_inline)) inline void rollout_wave(const hs_topo* __restrict__ T0, const hs_run_args& a,
                                                                   RolloutWS* __restrict__ rws, const hs::launch_map& mp,
                                                                   Smem<NM, FORCES>* smem, int fstep, int wid,
                                                                   int only_sub) {
  const int sub = threadIdx.x / HALF;  // rollout slot within the wave
  const int lane = threadIdx.x % HALF; // lane within the rollout
  // one model per wavefront: the topology pointer stays wave-uniform (scalar loads)
  // (indexing the kernel argument keeps T a known-global pointer: global_load, not flat_load)
  const hs_topo* __restrict__ T = mp.wave_model ? T0 + mp.wave_model[wid] : T0;
  int b, bb;
  bool live;  // an idle half (odd group) computes a copy of its neighbour and stores nothing
  if (mp.wave_rollouts) {
    b = mp.wave_rollouts[2 * wid + sub];
    live = b >= 0;
    bb = live ? b : mp.wave_rollouts[2 * wid];
  } else {
    b = wid * 2 + sub;
    live = b < a.n_rollouts;
    bb = live ? b : a.n_rollouts - 1;
  }
  // fixup: the neighbour's step is already stored; that half runs along without storing and without
  // the general path, whose workspace (the idle slot) the fixup's other wavefronts would share
  const bool fix_idle = only_sub >= 0 && sub != only_sub;
  if (fix_idle) {
    bb = live ? b : bb;
    live = false;
  }
  SolveWS* G = mp.fused_gen ? &((SolveWS*)mp.fused_gen)[(size_t)fstep * (a.n_rollouts + 1) + (live ? b : a.n_rollouts)]
                            : &rws[live ? b : a.n_rollouts].sol;
  Smem<NM, FORCES>& sm = smem[sub];
  SolveRef sv;
  if constexpr (FORCES) {
    sv.f = sm.sv.xy.f;
    sv.x = sm.sv.xy.x;
    sv.y = sm.sv.xy.y;
  } else {
    sv.f = sm.d.post.f;
    sv.x = sm.d.post.x;
    sv.y = sm.d.post.y;
  }
  sv.cfoot = sm.sv.cfoot;
  sv.fch = sm.sv.fch;
  real work = (live && a.accumulate && a.work_cot && !mp.fused_w) ? outp(a.work_cot)[2 * (size_t)b] : real(0);
  int k0 = a.k0, h_row = mp.h_row;
  if (mp.fused_w) {
    const int s = mp.fused_s0 + fstep, c = s / mp.fused_h;
    k0 = (int)(((int64_t)a.k0 + (int64_t)c * mp.fused_h) % a.n_t) + s % mp.fused_h;
    h_row = s;
  }
#ifdef HS_DBG
  if (lane == 0) dbg_rows()[sub] = live ? b * a.horizon + h_row : -1;
  wave_sync();
#endif
  const int nl = T->n_limbs;
  // the gait setup of the rollout, stored by the call's preparation pass (hs_prep_kernel;
  // the idle half reads its neighbour's): read from global memory where it is used
  const SetupL& st = rws[bb].st;
  const int i = k0 + 2;  // centre sample of this launch's step
  const int sl = lane / nl, L = lane % nl;
  const real* kt = mp.ktab_n > 0 ? &rws[bb].ktab[0][0][0] : nullptr;
  const uint8_t* kb = &rws[bb].kbad[0][0];
#if HS_PRELOAD
  const StraightPre pre = straight_preload(st, rws[bb].t_tab, rws[bb].kf, HS_KTE_PRELOAD ? kt : nullptr, kb,
                                           i - 2 + (sl < NS ? sl : 0), mp.ktab_lo, mp.ttab_n, L);
#endif
  const real dt = st.dt;
  // the gait's kind from two of its parameters; the whole record (GaitR) is loaded only on the paths that
  // read it, so that it is not held in registers (at 4 waves/SIMD: spilled) across the step
  const hs_gait_params& gp = a.params[bb];
  const bool ignore_reach = a.ignore_reach != 0;
  const bool straight = (real)gp.curvature == 0 && !gp.rec_transform_flag;
#if HS_CURVED_LDS
  // a wave with a turning or transformed gait: the record in LDS for the turning path's many reads
  if (!kt && __ballot(!straight)) {
    constexpr int NW = sizeof(SetupL) / sizeof(real);
    const real* cache = reinterpret_cast<const real*>(&rws[bb].st);
    real* lds = reinterpret_cast<real*>(&smem[sub].st);
    for (int e = lane; e < NW; e += HALF) lds[e] = cache[e];
    wave_sync();
  }
  const SetupL& st_curved = smem[sub].st;
#else
  const SetupL& st_curved = st;
#endif

  STAMP(0);
  STAMP(1);

  // K: the five-sample window, lane = (sample, limb)
  {
    const real* t_tab = rws[bb].t_tab;
    // a straight, untransformed gait (the common case): its frames from the setup pass, its joint
    // values from the call's IK table when there is one (kin_sample_straight)
    if (sl < NS) {
      if (straight) {
#if !HS_PRELOAD
        const StraightPre pre = straight_preload(st, t_tab, rws[bb].kf, HS_KTE_PRELOAD ? kt : nullptr, kb,
                                                 i - 2 + sl, mp.ktab_lo, mp.ttab_n, L);
#endif
        kin_sample_straight(T, gp, st, i - 2 + sl, L, ignore_reach, OneWin<NM, FORCES>{&sm.d}, sl - 2,
                            pre, rws[bb].kf, kt, kb, mp.ktab_lo);
      } else if (kt) {  // a turning or transformed gait with the call's tables
        const int r = i - 2 + sl - mp.ktab_lo;
#if HS_PRELOAD && HS_KTE_PRELOAD
        const real* kte = pre.kte;
        const bool kbad = pre.bad;
#else
        const real* kte = kt + ((size_t)r * HS_LMAX + L) * KT_W;
        const bool kbad = kb[r * HS_LMAX + L] != 0;
#endif
        kin_sample_tab(T, L, OneWin<NM, FORCES>{&sm.d}, sl - 2, rws[bb].ktor[r], kte, kbad);
      } else {
        kin_sample<false>(T, load_gait(gp), gp, st_curved, i - 2 + sl, L, ignore_reach, OneWin<NM, FORCES>{&sm.d},
                          sl - 2, t_tab, mp.ktab_lo, mp.ttab_n);
      }
    }
    // the foot chains (hs_topo::foot_chain8), to LDS with the kinematics' stores: the contact blocks then
    // read them there instead of through two dependent global loads
    if (!FORCES && lane < 2 * HS_LMAX) (&sv.fch[0][0])[lane] = (&T->foot_chain8[0][0])[lane];
    wave_sync();
  }
  STAMP(2);
  if constexpr (FORCES) {
    forces_step(T, a, mp, dt, sv, sm.d.post, OneWin<NM, FORCES>{&sm.d}, b, live, h_row, lane);
    return;
  } else {
    bool deferred = false;
    step<DEFER>(T, a, mp, dt, sv, sm.d.post.fl, OneWin<NM, FORCES>{&sm.d}, G, b, live, h_row, work,
                deferred, !fix_idle, lane);
    if (DEFER && deferred) {  // the fixup launch solves this (step, rollout) with the general path
      if (lane == 0 && live) {
        const int it = atomicAdd(mp.fix_count, 1);
        mp.fix_items[2 * it] = fstep;
        mp.fix_items[2 * it + 1] = 2 * wid + sub;
      }
      return;
    }
  }
  if (DEFER || mp.fused_w) {  // this step's joint sum of positive work, summed over the steps in order by the reduce
    if (lane == 0 && live)
      reinterpret_cast<real*>(mp.fused_work)[(size_t)(mp.fused_s0 + fstep) * a.n_rollouts + b] = work;
    return;
  }
  const bool out = lane == 0 && live;
  if (out && a.work_cot) {
    real cot = work / ((real)T->total_mass * (real)gp.step_length);
    outp(a.work_cot)[2 * (size_t)b] = work;
    outp(a.work_cot)[2 * (size_t)b + 1] = cot;
  }
  if (a.best_key) {
    unsigned long long key = ~0ull;
    if (out) key = best_key(key_cot(work, (real)T->total_mass, (real)gp.step_length, a.n_t, a.key_steps), a.rollout_id_base + b);
    if constexpr (!DEFER) {  // both rollouts of the wave are here: their minimum first
      const unsigned long long o = __shfl_xor(key, HALF);
      key = o < key ? o : key;
    }
    // The key only decreases, so any value read from it bounds the final minimum from above: a key not
    // below it cannot win, and skipping its atomic keeps the last launch from queueing one atomic per
    // wave on a single address (~20 us per call at B = 4096)
    if ((DEFER ? lane : (int)threadIdx.x) == 0 && key != ~0ull &&
        key < __hip_atomic_load((unsigned long long*)a.best_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin((unsigned long long*)a.best_key, key);
  }
}

// MODE (hs::FIX_*): NONE, the step with the general path out of line; DEFER, the fused step launch
// without it; SOLVE, the fixup launch over the deferred items (its own instantiation, so the loop
// costs the other two nothing)
template <int NM, bool FORCES, int MODE>
__global__ __launch_bounds__(WAVE, FORCES ? HS_MIN_WAVES_FORCES
                                                 : (HS_REAL_IS_FLOAT ? (MODE == hs::FIX_DEFER ? HS_MIN_WAVES_F32_DEFER : HS_MIN_WAVES_F32)
                                                                     : (MODE == hs::FIX_DEFER ? HS_MIN_WAVES_DEFER : HS_MIN_WAVES))) void hs_rollout_kernel(const hs_topo* __restrict__ T0,
                                                                                 hs_run_args a, RolloutWS* __restrict__ rws,
                                                                                 hs::launch_map mp) {
  __shared__ Smem<NM, FORCES> smem[2];
  RSTAMP(16);
  STAMP(15);
  if constexpr (MODE == hs::FIX_SOLVE) {  // the deferred (step, rollout) items
    const int n = *mp.fix_count;           // written by the previous launch on this stream
    if (mp.fix_reduce) {  // workgroup w: the work reduce of rollouts 64 w .. 64 w + 63 after the items
      // fix_barrier: the items over every workgroup (a rollout whose legs stay straight defers many of its
      // steps: one workgroup fixing them in turn ran 200 us, configs[4]), then a grid barrier: the launch's
      // ceil(B / 64) <= 1024 one-wavefront workgroups are resident together (the host passes no barrier
      // otherwise); n is the same for all, so every workgroup arrives. Otherwise each workgroup fixes its
      // own rollouts' items in turn. (One call site of the step: a second inlined copy doubled the code.)
      const bool spread = mp.fix_barrier != nullptr;
      for (int it = spread ? (int)blockIdx.x : 0; it < n; it += spread ? (int)gridDim.x : 1) {
        const int fstep = mp.fix_items[2 * it], ws = mp.fix_items[2 * it + 1];
        const int rb = mp.wave_rollouts ? mp.wave_rollouts[ws] : ws;
        if (!spread && rb / WAVE != (int)blockIdx.x) continue;
        rollout_wave<NM, FORCES, false>(T0, a, rws, mp, smem, fstep, ws >> 1, ws & 1);
        wave_sync();
      }
      if (n > 0) __threadfence();  // the fixed steps' rows and work terms, before this workgroup's arrival
      if (spread && n > 0 && threadIdx.x == 0) {
        atomicAdd(mp.fix_barrier, 1);
        // bounded (~2^24 polls): a barrier that never fills ends the wait instead of hanging the device
        for (int spin = 0; spin < (1 << 24); spin++) {
          if (__hip_atomic_load(mp.fix_barrier, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= (int)gridDim.x) break;
          __builtin_amdgcn_s_sleep(2);
        }
      }
      __syncthreads();
      if (spread && n > 0) __threadfence();
      reduce_rollouts(a, (real)mp.red_total_mass, mp.red_rollout_mass, reinterpret_cast<const real*>(mp.fused_work),
                      mp.red_n_steps, mp.red_best_key, mp.red_key_steps);
      return;
    }
    for (int it = blockIdx.x; it < n; it += gridDim.x) {  // one item per wavefront
      const int fstep = mp.fix_items[2 * it], ws = mp.fix_items[2 * it + 1];
      rollout_wave<NM, FORCES, false>(T0, a, rws, mp, smem, fstep, ws >> 1, ws & 1);
      wave_sync();
    }
  } else {
    // fused steps: this wavefront's step and its wavefront within the batch
    int fstep = 0, wid = (int)blockIdx.x;
    if (mp.fused_w) fused_coords((int)blockIdx.x, mp.fused_w, mp.fused_n, fstep, wid);
    rollout_wave<NM, FORCES, MODE == hs::FIX_DEFER>(T0, a, rws, mp, smem, fstep, wid, -1);
  }
}

}  // namespace

namespace hs {

// the launchers of this unit's precision, exported as one table by the unit (hs::kernels)
static size_t general_workspace_bytes() { return sizeof(RolloutWS); }

template <int NM>
void launch_nm(const hs_topo* d_topo, const hs_run_args& a, RolloutWS* ws, const launch_map& mp, hipStream_t st) {
  if (mp.tau_in && mp.fix_mode == FIX_SOLVE)  // the limb-lane forces launch's deferred items
    hipLaunchKernelGGL((hs_rollout_kernel<NM, true, FIX_SOLVE>), dim3(mp.n_waves), dim3(WAVE), 0, st, d_topo, a, ws, mp);
  else if (mp.tau_in)
    hipLaunchKernelGGL((hs_rollout_kernel<NM, true, FIX_NONE>), dim3(mp.n_waves), dim3(WAVE), 0, st, d_topo, a, ws, mp);
  else if (mp.fix_mode == FIX_DEFER)
    hipLaunchKernelGGL((hs_rollout_kernel<NM, false, FIX_DEFER>), dim3(mp.n_waves), dim3(WAVE), 0, st, d_topo, a, ws, mp);
  else if (mp.fix_mode == FIX_SOLVE)
    hipLaunchKernelGGL((hs_rollout_kernel<NM, false, FIX_SOLVE>), dim3(mp.n_waves), dim3(WAVE), 0, st, d_topo, a, ws, mp);
  else
    hipLaunchKernelGGL((hs_rollout_kernel<NM, false, FIX_NONE>), dim3(mp.n_waves), dim3(WAVE), 0, st, d_topo, a, ws, mp);
}

static int launch_rollouts(const hs_topo* d_topo, const hs_run_args& a, void* workspace, const launch_map& mp) {
  if (a.n_rollouts <= 0 || mp.n_waves <= 0) return 0;
  hipStream_t st = (hipStream_t)a.stream;
  RolloutWS* ws = (RolloutWS*)workspace;
  // one launch per step of the horizon: step h writes output row h, work accumulates in
  // step order (periodic.cpp:291-304), the best key is taken after the last step
  for (int h = 0; h < a.horizon; h++) {
    hs_run_args ah = a;
    launch_map mh = mp;
    // position control reads the cycle at tsi mod n_t (hs_run_pd): its steps wrap within the call
    ah.k0 = mp.pd_tau ? (int32_t)(((int64_t)a.k0 + h) % a.n_t) : a.k0 + h;
    ah.accumulate = (h == 0) ? a.accumulate : 1;
    if (h + 1 < a.horizon) ah.best_key = nullptr;
    mh.h_row = h;
    if (h > 0 && mp.setup_io != SETUP_COMPUTE) mh.setup_io = SETUP_LOAD;
    with_lds_class(mp.max_parts, [&](auto nm) { launch_nm<decltype(nm)::value>(d_topo, ah, ws, mh, st); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

static int launch_fused(const hs_topo* d_topo, const hs_run_args& a, void* workspace, const launch_map& mp) {
  if (a.n_rollouts <= 0 || mp.n_waves <= 0) return 0;
  hipStream_t st = (hipStream_t)a.stream;
  RolloutWS* ws = (RolloutWS*)workspace;
  if (mp.setup_only) {  // the call's preparation pass: setup record, sample times, IK table
    int R;
    const int units = prep_units(mp, a.n_rollouts, R);
    const int64_t blocks = prep_blocks(units, R, mp.ttab_n, mp.ktab_nl > 0 ? mp.ktab_nl : HS_LMAX);
    if (mp.wave_model)
      hipLaunchKernelGGL(hs_prep_kernel<true>, dim3((unsigned)blocks), dim3(WAVE * HS_PREP_WPB), 0, st, d_topo, a, ws, mp);
    else
      hipLaunchKernelGGL(hs_prep_kernel<false>, dim3((unsigned)blocks), dim3(WAVE * HS_PREP_WPB), 0, st, d_topo, a, ws, mp);
    return (int)hipGetLastError();
  }
  launch_map m = mp;
  m.fused_w = mp.setup_only ? 0 : mp.n_waves;
  m.n_waves = mp.setup_only ? mp.n_waves : mp.n_waves * mp.fused_n;  // the grid
  // the fixup launch: in HS_SOLVE_AUTO a few wavefronts loop over the deferred items (usually none:
  // they exit at once); in HS_SOLVE_REFERENCE every step is an item, one wavefront each
  if (mp.fix_mode == FIX_SOLVE) m.n_waves = a.solve_mode != HS_SOLVE_AUTO ? 2 * m.n_waves : (m.n_waves < 256 ? m.n_waves : 256);
  if (mp.fix_mode == FIX_SOLVE && mp.fix_reduce) m.n_waves = (a.n_rollouts + WAVE - 1) / WAVE;  // 64 rollouts each
  with_lds_class(mp.max_parts, [&](auto nm) { launch_nm<decltype(nm)::value>(d_topo, a, ws, m, st); });
  return (int)hipGetLastError();
}

__global__ void hs_fused_reduce_kernel(hs_run_args a, real total_mass, const double* __restrict__ rollout_mass,
                                       const real* __restrict__ ws, int n_steps) {
  reduce_rollouts(a, total_mass, rollout_mass, ws, n_steps, reinterpret_cast<uint64_t*>(a.best_key), a.key_steps);
}

static int launch_fused_reduce(const hs_run_args& a, double total_mass, const double* rollout_mass,
                               const void* work_steps, int32_t n_steps) {
  if (a.n_rollouts <= 0 || !a.work_cot) return 0;
  // one wavefront per workgroup: B = 4096 spreads over 64 CUs instead of 16
  hipLaunchKernelGGL(hs_fused_reduce_kernel, dim3((a.n_rollouts + 63) / 64), dim3(64), 0, (hipStream_t)a.stream, a,
                     (real)total_mass, rollout_mass, (const real*)work_steps, n_steps);
  return (int)hipGetLastError();
}

}  // namespace hs
