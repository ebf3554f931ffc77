// hs_step_kin.h -- the kinematic half of a control step, shared by both step kernels: the gait setup (S),
// the trajectory sampler with the torso / chain FK, the limb IK and the limb FK (K), the finite differences
// (D) and the particular solution of B0 x = f (S1). The phase list is at the head of hs_rollout_kernel.h.
#pragma once
#include "hs_step_base.h"

namespace {

// gait parameters of one rollout in the working precision (hs_gait_params, pergen.h:137-146)
struct GaitR {
  real torso_pos[3], torso_angles[3];
  real step_duration, period, step_length, step_height, curvature, foot_shift;
  int foot_shift_type;
  int rec_xf;  // rec_transform_flag: the transform itself is read where it applies (gait_record)
};

__device__ inline GaitR load_gait(const hs_gait_params& p) {
  GaitR g;
  for (int i = 0; i < 3; i++) {
    g.torso_pos[i] = (real)p.torso_pos[i];
    g.torso_angles[i] = (real)p.torso_angles[i];
  }
  g.step_duration = (real)p.step_duration;
  g.period = (real)p.period;
  g.step_length = (real)p.step_length;
  g.step_height = (real)p.step_height;
  g.curvature = (real)p.curvature;
  g.foot_shift = (real)p.foot_shift;
  g.foot_shift_type = p.foot_shift_type;
  g.rec_xf = p.rec_transform_flag;
  return g;
}

// pergensetup::transform_rec (pergen.cpp:323-335) with rec_transform = affine_from_orientation(
// {rec_transl, rec_eas}) (set_rec_transform, pergen.cpp:316-320): the torso by transform_orientation
// (pergen.cpp:377-383: A1 = rec_transform A0, then its translation and Euler angles), the foot target
// by rec_transform.mult with w = 1
__device__ inline void transform_rec(const hs_gait_params& p, real* o0, real* o1, real* target) {
  const real tr[3] = {(real)p.rec_transl[0], (real)p.rec_transl[1], (real)p.rec_transl[2]};
  const A34 R = from_euler(tr, (real)p.rec_eas[0], (real)p.rec_eas[1], (real)p.rec_eas[2]);
  const A34 A1 = mul(R, from_euler(o0, o1[0], o1[1], o1[2]));
  o0[0] = A1(0, 3); o0[1] = A1(1, 3); o0[2] = A1(2, 3);
  euler_from(A1, o1);
  real t[3];
  mulp(R, target, t);
  target[0] = t[0]; target[1] = t[1]; target[2] = t[2];
}

// the straight gait's frame at tv = t v: [R | c + tv u] (KinFrames)
__device__ inline A34 frame_at(A34 A, const real* u, real tv) {
#pragma unroll
  for (int r = 0; r < 3; r++) A.at(r, 3) = fma(tv, u[r], A(r, 3));
  return A;
}
__device__ inline A34 load34r(const real* m) {
  A34 a;
#pragma unroll
  for (int i = 0; i < 12; i++) a.m[i] = m[i];
  return a;
}
__device__ inline void store34r(const A34& a, real* m) {
#pragma unroll
  for (int i = 0; i < 12; i++) m[i] = a.m[i];
}

// ---------------------------------------------------------------------------
// S: gait setup, lanes L < n_limbs (pergen.cpp:453-507, 30-51, 143-153)
// ---------------------------------------------------------------------------
// periodicgenerator::set_step_duration (pergen.cpp:30-51) for n limbs: the stepping fraction t_step and
// pergen index j's lift-off time ts and shift xs (the loop's entry k = j = jj + i jmax)
__device__ inline real step_fraction(const GaitR& g, int n) {
  const real f = g.step_duration;
  return f * (real(1) / 2 - real(1) / n) + real(1) / n;
}
__device__ inline void lift_off(int n, int j, real t_step, real& ts, real& xs) {
  const int jmax = n / 2;
  const int z = (jmax == 1) ? 1 : jmax - 1;
  const int i = j / jmax, jj = j % jmax;
  ts = jj * (real(1) / 2 - t_step) / z + real(i) / 2;
  xs = ts + t_step / 2 - real(1) / 2;
}

// the torso frame at the configured pose (orient_torso); tsc: sincos3 of the configured angles
__device__ inline A34 torso_frame(const hs_topo* T, const GaitR& g, const SC3& tsc) {
  const real q6[6] = {g.torso_pos[0], g.torso_pos[1], g.torso_pos[2],
                      g.torso_angles[0], g.torso_angles[1], g.torso_angles[2]};
  return mul(mul(node_joint_parent(T, 0), free_joint_sc(q6, tsc)), node_pj(T, 0));
}

// Limb L's part of the gait setup from the torso frame A0: the hip joint frame J0 (poslimb,
// lik.cpp:341-347) and the default foot position of its pergen index (get_limb_hip_pos, the foot
// shift, set_limb_poss; pergen.cpp:453-507). kf (optional): store the chain body frames this limb owns
// and its hip frame (KinFrames, the straight gaits' frames at tv = 0)
// The chain's products come precombined from the loader (hs_topo::limb_own_rel, limb_hip_rel): one product
// per frame, every load indexed by the limb alone
// A limb's setup constants (hs_topo::limb_*), loaded before the gait parameters they do not depend on
struct LimbPlan {
  A34 hip, own0;  // limb_hip_rel, limb_own_rel[0] (limb_own_n > 0)
  real ct[3], com0[3];
  int own_n, ysign;  // ysign: limb_ysign, read by the table rows' IK
};
__device__ __attribute__((always_inline)) inline LimbPlan load_plan(const hs_topo* T, int L) {
  LimbPlan p;
  p.own_n = T->limb_own_n[L];
  p.ysign = T->limb_ysign[L];
  p.hip = load34(T->limb_hip_rel[L]);
  p.own0 = load34(T->limb_own_rel[L][0]);
  for (int i = 0; i < 3; i++) {
    p.ct[i] = (real)T->limb_child_t[L][i];
    p.com0[i] = (real)T->limb_own_com[L][0][i];
  }
  return p;
}
__device__ __attribute__((always_inline)) inline void limb_setup(const hs_topo* T, const GaitR& g, const A34& A0, int L,
                                                                 const LimbPlan& pl, A34& J0, real* pos0,
                                                                 KinFrames* kf = nullptr) {
  if (kf)
    for (int m = 0; m < pl.own_n; m++) {
      real com[3];
      for (int i = 0; i < 3; i++) com[i] = m == 0 ? pl.com0[i] : (real)T->limb_own_com[L][m][i];
      store_body(mul(A0, m == 0 ? pl.own0 : load34(T->limb_own_rel[L][m])), com, kf->own[L][m], BF_W);
    }
  J0 = mul(A0, pl.hip);
  if (kf) store34r(J0, kf->J0[L]);
  // get_limb_hip_pos: the child's frame J0 Rz(0) pj_child (Rz(0) = I) at its translation
  real pos[3];
  mulp(J0, pl.ct, pos);
  if (g.foot_shift_type == 0) {                   // setup_foot_shift / shift_pos0
    real sh[3] = {real(0), g.foot_shift, real(0)}, ls[3];
    mulp(A0, sh, ls);
    if (L % 2) for (int i = 0; i < 3; i++) ls[i] *= -1;
    for (int i = 0; i < 3; i++) pos[i] += ls[i];
  } else if (g.foot_shift_type == 1) {
    real x = pos[0], y = pos[1];
    real f = g.foot_shift / sqrt(x * x + y * y);
    real d[3] = {x * f, y * f, real(0)};
    for (int i = 0; i < 3; i++) pos[i] += d[i];
  }
  pos0[0] = pos[0];
  pos0[1] = pos[1];
  pos0[2] = (real)T->rcap;  // set_limb_poss
}

// compute_max_radius's distance of one default foot position from the turning centre (0, 1 / curvature)
__device__ inline real turn_radius(const real* pos0, real curvature) {
  const real cy = real(1) / curvature;
  const real d0 = pos0[0] - real(0), d1 = pos0[1] - cy, d2 = pos0[2] - real(0);
  real s = 0;
  s += d0 * d0;
  s += d1 * d1;
  s += d2 * d2;
  return sqrt(s);
}

// The whole setup on a half-wave (hs_pergen_rec_kernel), lanes L < n_limbs: SetupL in LDS
__device__ __attribute__((always_inline)) inline void gait_setup(const hs_topo* T, const GaitR& g, int n_t, SetupL& st,
                                                                 int lane) {
  const int nl = T->n_limbs;
  const real t_step = step_fraction(g, nl);
  if (lane < nl) {
    const int L = lane;
    const SC3 tsc = sincos3(g.torso_angles[0], g.torso_angles[1], g.torso_angles[2]);
    if (L == 0) st.tsc = tsc;
    A34 J0;
    const int j = T->limb_pergen[L];
    limb_setup(T, g, torso_frame(T, g, tsc), L, load_plan(T, L), J0, st.pos0[j]);
    lift_off(nl, j, t_step, st.ts[j], st.xs[j]);
  }
  if (lane == 0) {
    st.t_step = t_step;
    st.v = g.step_length / g.period;  // pergensetup::set_TLh
    st.dt = g.period / n_t;           // record_trajectory
  }
  wave_sync();
  if (lane == 0) {  // compute_max_radius
    real mr = 0;
    if (g.curvature != 0)
      for (int j = 0; j < nl; j++) {
        const real rad = turn_radius(st.pos0[j], g.curvature);
        if (rad > mr) mr = rad;
      }
    st.max_radius = mr;
  }
  wave_sync();
}

// ---------------------------------------------------------------------------
// K: one (sample, limb) pair per lane
// ---------------------------------------------------------------------------
// pergen.cpp:143-153 step profiles: stepx(t) = (1 - cos(pi t)) / 2, stepz(t) = sin(pi t)^2, from one sincos
__device__ inline void step_profiles(real t, real& sx, real& sz) {
  real s, c;
  sincos(kPi * t, &s, &c);
  sx = (1 - c) / 2;
  sz = s * s;
}

// What the kinematics reads of one node, fetched in one batch of independent loads instead of
// one round trip per branch that consumes it (fetching earlier measured slower: the values
// stay live across the gait record and their waits land on its loads, vmcnt being in order).
struct NodeK {
  A34 Jp, pj;  // J_A_parent, A_pj_body
  real com[3], cap[3];
  int foot, hinge, owner;
};
__device__ __attribute__((always_inline)) inline NodeK load_nodek(const hs_topo* T, int v) {
  const hs_node& nd = T->node[v];
  NodeK r;
  r.Jp = load34(nd.J_A_parent);
  r.pj = load34(nd.A_pj_body);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    r.com[i] = (real)nd.com[i];
    r.cap[i] = (real)nd.cap[i];
  }
  r.foot = nd.foot;
  r.hinge = nd.hinge;
  r.owner = nd.owner_limb;
  return r;
}

template <class W>
__device__ __attribute__((always_inline)) inline void node_features(const hs_topo* T, int v, const NodeK& nd, const A34& A, const A34* J, const W& w, int k) {
  if (w.want_pos(k)) {
    real p[3];
    mulp(A, nd.com, p);
    real* P = w.pos(k, v);
    for (int i = 0; i < 3; i++) P[i] = p[i];
  }
  if (w.want_ust(k)) {
    real* U = w.ust(k, v);
    U[0] = (A(2, 1) - A(1, 2)) / 2;
    U[1] = (A(0, 2) - A(2, 0)) / 2;
    U[2] = (A(1, 0) - A(0, 1)) / 2;
  }
  if (w.want_centre(k)) {
    real* Jp = w.jpos(k, v);
    real* Jz = w.jz(k, v);
    for (int i = 0; i < 3; i++) Jp[i] = J ? (*J)(i, 3) : A(i, 3);
    for (int i = 0; i < 3; i++) Jz[i] = J ? (*J)(i, 2) : real(0);
    if (nd.foot >= 0) {
      real fp[3];
      mulp(A, nd.cap, fp);
      real* F = w.fpos(k, nd.foot);
      for (int i = 0; i < 3; i++) F[i] = fp[i];
      w.contact(k, nd.foot) = fp[2] < (real)(T->rcap + 1e-4);
    }
  }
}

// periodicgenerator::limb_positions' step of one pergen index at time t (pergen.cpp:82-94): the
// forward shift dx and lift dz of its foot, t_lift / xs its lift-off entries, t_step the stepping fraction
__device__ inline void limb_step(const GaitR& g, real t, real t_lift, real xs, real t_step, real& dx, real& dz) {
  const real tt = t / g.period;
  const int t_int = int(tt);
  const real t_frac = tt - t_int;
  real stepf;
  if (t_frac < t_lift) stepf = 0;
  else if (t_frac < t_lift + t_step) stepf = (t_frac - t_lift) / t_step;
  else stepf = 1;
  real sx, sz;
  step_profiles(stepf, sx, sz);
  dx = (t_int + xs + sx) * g.step_length;
  dz = sz * g.step_height;
}

// What gait_record reads of the gait setup for one pergen index j: the rollout's entries and j's
// (from the setup record, limb_rec, or from the preparation pass's registers)
struct LimbRec {
  real v, t_step, max_radius, ts, xs, pos0[3];
  SC3 tsc;
};
__device__ __attribute__((always_inline)) inline LimbRec limb_rec(const SetupL& st, int j) {
  LimbRec r;
  r.v = st.v;
  r.t_step = st.t_step;
  r.max_radius = st.max_radius;
  r.ts = st.ts[j];
  r.xs = st.xs[j];
  for (int i = 0; i < 3; i++) r.pos0[i] = st.pos0[j][i];
  r.tsc = st.tsc;
  return r;
}

// pergensetup::set_rec at time t for lik limb L (pergen.cpp:225-239): torso position o0 and Euler
// angles o1 (turn_torso, pergen.cpp:386-397; `turned` when the torso frame was rotated), and the
// limb's foot target (limb_positions of its pergen index, pergen.cpp:82-94, 160-183); st: that
// index's LimbRec
// STRAIGHT: the caller knows curvature == 0 (a wave of straight gaits), so the turning code is left
// out and the record is one basic block the scheduler can interleave with the torso FK
template <bool STRAIGHT = false>
__device__ __attribute__((always_inline)) inline void gait_record(const GaitR& g, const hs_gait_params& gp,
                                                                  const LimbRec& st, real t, real* o0, real* o1,
                                                                  bool& turned, real* target) {
  o0[0] = g.torso_pos[0]; o0[1] = g.torso_pos[1]; o0[2] = g.torso_pos[2];
  o1[0] = g.torso_angles[0]; o1[1] = g.torso_angles[1]; o1[2] = g.torso_angles[2];
  real tv = t * st.v;
  turned = false;
  real psi = 0;
  if (!STRAIGHT && g.curvature != 0) {
    int s = (g.curvature > 0) ? 1 : -1;
    psi = s * tv / st.max_radius;
    turned = psi != 0;
  }
  if (!turned) {
    o0[0] += tv;
  } else {
    real rc = real(1) / g.curvature;
    real sp, cp;
    sincos(psi, &sp, &cp);
    real tp[3] = {rc * sp, rc * (1 - cp), 0};
    A34 At = from_euler_sc(tp, SC3{real(0), real(1), real(0), real(1), sp, cp});  // sin 0 = 0, cos 0 = 1
    A34 A0 = from_euler_sc(o0, st.tsc);
    A34 A1 = mul(At, A0);
    o0[0] = A1(0, 3); o0[1] = A1(1, 3); o0[2] = A1(2, 3);
    euler_from(A1, o1);
  }
  // periodicgenerator::limb_positions for this limb's pergen index (pergen.cpp:82-94)
  real dx, dz;
  limb_step(g, t, st.ts, st.xs, st.t_step, dx, dz);
  real dy = 0;
  if (!STRAIGHT && g.curvature != 0) {  // turn_position (pergen.cpp:160-183)
    int s = (g.curvature > 0) ? 1 : -1;
    real x0 = st.pos0[0], y0 = st.pos0[1];
    real rc = real(1) / g.curvature;
    real rx = x0, ry = y0 - rc;
    real r = sqrt(rx * rx + ry * ry);
    real alpha = atan2(ry, rx);
    real beta = -s * dx / st.max_radius;
    real gamma = alpha - beta / 2;
    real sb = 2 * sin(beta / 2);
    real sg, cg;
    sincos(gamma, &sg, &cg);
    dx = r * sg * sb;
    dy += -r * cg * sb;
  }
  target[0] = dx + st.pos0[0];
  target[1] = dy + st.pos0[1];
  target[2] = dz + st.pos0[2];
  if (!STRAIGHT && g.rec_xf) {  // set_rec's last step (pergen.cpp:238)
    transform_rec(gp, o0, o1, target);
    turned = true;  // the torso angles are no longer the configured ones
  }
}

// sample times t_i = dt + dt + ... (i terms, periodic.cpp:171-181), stored once per rollout by the
// call's preparation pass (the same additions in the same order) for the samples its steps read:
// t_tab[r] = t_(lo + r), r < ttab_n
__device__ inline real sample_time_sum(real dt, int isample) {
  real t = 0;
  for (int i = 0; i < isample; i++) t += dt;
  return t;
}
__device__ inline real sample_time(const SetupL& st, const real* t_tab, int isample, int lo, int ttab_n) {
  const int r = isample - lo;
  if (t_tab && r >= 0 && r < ttab_n) return t_tab[r];
  return sample_time_sum(st.dt, isample);
}

// a joint value sincos_k_small (the limb kernel's FK) does not take, |x| >= 2^20 or not finite: the step is
// deferred (the preparation pass tabulates a row's test as RolloutWS::kbig)
__device__ inline bool sincos_big(real x) { return !(fabs(x) < (real)0x1p20); }
// a motor's joint rate at the centre (compute_vel_traj's wrapped difference of q at t + dt and t - dt), the
// +-pi wrap as selects (the limb kernel's; the preparation pass tabulates it as RolloutWS::kvel)
__device__ inline real wrap_rate(real q_plus, real q_minus, real dt) {
  const real dd = q_plus - q_minus;
  const real lo = dd - 2 * kPi, hi = dd + 2 * kPi;
  return (dd > kPi ? lo : (dd < -kPi ? hi : dd)) / (2 * dt);
}

// limb FK with the new joint values (compute_dynrecs' recompute_modelnodes, model.cpp:183-201) from the
// hip joint frame J, and the dynamic features of the links (dynrec.cpp:134-155), on the limb's
// precombined plan (hs_topo::link): per link k the hinge frame H = J_k Rz(q_k) (mul_hinge), its body frame
// A_k = H pj_k seen through the products the features need -- pos = H (pj_k com), the rotation skew of
// A_k (ust) from H's and pj_k's rotations, the foot H (pj_2 cap) -- and the next joint frame J_(k+1) =
// H (pj_k Jp_(k+1)): one 3 x 4 product per link where the node-by-node form takes two
// (sq, cq: sin and cos of the joint values ja)
template <class W>
__device__ __attribute__((always_inline)) inline void limb_fk(const hs_topo* T, int L, const A34& J, const real* ja,
                                                              const real* sq, const real* cq, bool wq, const W& w,
                                                              int k) {
  const int lv[3] = {T->limb_node[L][0], T->limb_node[L][1], T->limb_node[L][2]};
  A34 Jv = J, H;
#pragma unroll
  for (int kk = 0; kk < 3; kk++) {  // limb_child, its first kid, that one's first kid
    const hs_link& lk = T->link[L][kk];
    if (kk > 0) Jv = mul(H, load34(lk.P));
    H = mul_hinge(Jv, cq[kk], sq[kk]);
    if (wq) w.q(k)[6 + lk.hinge] = ja[kk];
    const int v = lv[kk];
    if (w.want_pos(k)) {
      const real c[3] = {(real)lk.com[0], (real)lk.com[1], (real)lk.com[2]};
      real p[3];
      mulp(H, c, p);
      real* P = w.pos(k, v);
      for (int i = 0; i < 3; i++) P[i] = p[i];
      if (k == 0) DBG(v, p[0], 1);
      if (k == -2) DBG(v, p[0], 12);
    }
    if (w.want_ust(k)) {  // (A(2,1) - A(1,2)) / 2 etc. of A = H pj: (r, c) = sum_m H(r, m) pj(m, c)
      real R[9];
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = (real)lk.Rpj[i];
      auto a_rc = [&](int r, int c) { return H(r, 0) * R[c * 3 + 0] + H(r, 1) * R[c * 3 + 1] + H(r, 2) * R[c * 3 + 2]; };
      real* U = w.ust(k, v);
      U[0] = (a_rc(2, 1) - a_rc(1, 2)) / 2;
      U[1] = (a_rc(0, 2) - a_rc(2, 0)) / 2;
      U[2] = (a_rc(1, 0) - a_rc(0, 1)) / 2;
      if (k == 0) DBG(v, U[0], 5);
      if (k == -2) DBG(v, U[0], 9);
      if (k == 2) DBG(v, U[0], 11);
    }
    if (w.want_centre(k)) {
      real* Jp = w.jpos(k, v);
      real* Jz = w.jz(k, v);
      for (int i = 0; i < 3; i++) Jp[i] = Jv(i, 3);
      for (int i = 0; i < 3; i++) Jz[i] = Jv(i, 2);
      if (lk.foot >= 0) {
        const real c[3] = {(real)lk.cap[0], (real)lk.cap[1], (real)lk.cap[2]};
        real fp[3];
        mulp(H, c, fp);
        real* F = w.fpos(k, lk.foot);
        for (int i = 0; i < 3; i++) F[i] = fp[i];
        if (k == 0) DBG(24 + lk.foot, fp[2], 25);
        w.contact(k, lk.foot) = fp[2] < (real)(T->rcap + 1e-4);
      }
    }
  }
}

template <bool STRAIGHT, class W>
__device__ __attribute__((always_inline)) inline void kin_sample(const hs_topo* T, const GaitR& g, const hs_gait_params& gp,
                                                                 const SetupL& st, int isample, int L, bool ignore_reach,
                                                                 const W& w, int k, const real* t_tab, int tlo,
                                                                 int ttab_n) {
  const int j = T->limb_pergen[L];
  const int ysign = T->limb_ysign[L];
  const int clen = T->limb_chain_len[L];
  const int lv[3] = {T->limb_node[L][0], T->limb_node[L][1], T->limb_node[L][2]};
  const real t = sample_time(st, t_tab, isample, tlo, ttab_n);  // t accumulates dt (periodic.cpp:171-181)
  real o0[3], o1[3], target[3];
  bool turned;
  gait_record<STRAIGHT>(g, gp, limb_rec(st, j), t, o0, o1, turned, target);
  STAMP(20);
  // set_jvalues_with_lik: torso + body chain FK, then limb IK (model.cpp:354-359, lik.cpp:89-99)
  real q6[6] = {o0[0], o0[1], o0[2], o1[0], o1[1], o1[2]};
  const A34 F = (!STRAIGHT && turned) ? free_joint(q6) : free_joint_sc(q6, st.tsc);  // straight: angles fixed
  const NodeK n0 = load_nodek(T, 0);  // the torso
  A34 A0 = mul(mul(n0.Jp, F), n0.pj);
  const bool wq = w.want_q(k);
  if (L == 0) {
    if (wq) for (int i = 0; i < 6; i++) w.q(k)[i] = q6[i];
    node_features(T, 0, n0, A0, &n0.Jp, w, k);  // torso joint frame J = I * J_A_parent
  }
  A34 A = A0;
  for (int kk = 1; kk < clen; kk++) {
    const int v = T->limb_chain[L][kk];
    const NodeK nc = load_nodek(T, v);
    A = mul(A, nc.pj);
    if (nc.owner == L) node_features(T, v, nc, A, nullptr, w, k);
  }
  NodeK nk = load_nodek(T, lv[0]);  // limb_child
  A34 J = mul(A, nk.Jp);  // poslimb (lik.cpp:341-347)
  A34 Jinv = invert(J);
  STAMP(21);
  real pl[3], ja[3];
  mulp(Jinv, target, pl);
  bool unreach = false, fail = false;
  const real ls[3] = {(real)T->ls[0], (real)T->ls[1], (real)T->ls[2]};
  limb_ik(T->lik_kind, ls, ysign, pl, ja, ignore_reach, unreach, fail);
  if (w.want_centre(k)) w.unreach(k, L) = (unreach || fail) ? 1 : 0;
  STAMP(22);
  real sq[3], cq[3];
#pragma unroll
  for (int kk = 0; kk < 3; kk++) sincos_k(ja[kk], &sq[kk], &cq[kk]);
  limb_fk(T, L, J, ja, sq, cq, wq, w, k);
}

// set_rec's foot target of limb L at time t and the limb IK from the hip frame J (kin_sample's
// sequence from the gait record on); bad = unreachable (ignore_reach) or failed
// the limb IK of limb L for a foot target, from its hip joint frame J (lik.cpp:341-347, 151-223)
// (kind, ls, ysign: the model's IK variant, link lengths and the limb's side, read by the caller)
__device__ __attribute__((always_inline)) inline void hip_ik_k(const A34& J, const real* target, int kind,
                                                               const real* ls, int ysign, bool ignore_reach, real* ja,
                                                               bool& bad) {
  const A34 Jinv = invert(J);
  real pl[3];
  mulp(Jinv, target, pl);
  bool unreach = false, fail = false;
  limb_ik(kind, ls, ysign, pl, ja, ignore_reach, unreach, fail);
  bad = unreach || fail;
}
__device__ __attribute__((always_inline)) inline void hip_ik(const hs_topo* T, int L, const A34& J, const real* target,
                                                             bool ignore_reach, real* ja, bool& bad) {
  const real ls[3] = {(real)T->ls[0], (real)T->ls[1], (real)T->ls[2]};
  hip_ik_k(J, target, T->lik_kind, ls, T->limb_ysign[L], ignore_reach, ja, bad);
}

__device__ __attribute__((always_inline)) inline void straight_ik(const hs_topo* T, const GaitR& g,
                                                                  const hs_gait_params& gp, const SetupL& st, real t,
                                                                  int L, const A34& J, bool ignore_reach, real* ja,
                                                                  bool& bad) {
  real o0[3], o1[3], target[3];
  bool turned;
  gait_record<true>(g, gp, limb_rec(st, T->limb_pergen[L]), t, o0, o1, turned, target);
  hip_ik(T, L, J, target, ignore_reach, ja, bad);
}

// What kin_sample_straight loads that no computed value feeds (the sample time, the torso speed, the
// hip frame, the IK table row): loaded at the wave's start, before the gait record decides the path,
// so these latencies overlap the gait parameters' instead of following them
struct StraightPre {
  real t, v;
  A34 J0;
  real kte[KT_W];
  bool bad;
  real own0[BF_W];  // the limb's first chain body (limb_own_n > 0), and the torso (lane L = 0)
  real tor[6];
};
// (kt: the table, whose row r holds sample lo + r)
__device__ __attribute__((always_inline)) inline StraightPre straight_preload(const SetupL& st, const real* t_tab,
                                                                             const KinFrames& kf, const real* kt,
                                                                             const uint8_t* kb, int isample, int lo,
                                                                             int ttab_n, int L) {
  StraightPre p;
  p.t = sample_time(st, t_tab, isample, lo, ttab_n);
  p.v = st.v;
  p.J0 = load34r(kf.J0[L]);
#pragma unroll
  for (int i = 0; i < BF_W; i++) p.own0[i] = kf.own[L][0][i];
#pragma unroll
  for (int i = 0; i < 6; i++) p.tor[i] = kf.torso[i];
  if (kt) {
    const real* e = kt + ((size_t)(isample - lo) * HS_LMAX + L) * KT_W;
#pragma unroll
    for (int i = 0; i < KT_W; i++) p.kte[i] = e[i];
    p.bad = kb[(isample - lo) * HS_LMAX + L] != 0;
  }
  return p;
}

// kin_sample for a straight, untransformed gait: the frames from kf (the gait setup's), the joint
// values from the IK table kt (null: solved here, with the table kernel's straight_ik); pre: the
// preloaded values (straight_preload)
template <class W>
__device__ __attribute__((always_inline)) inline void kin_sample_straight(
    const hs_topo* T, const hs_gait_params& gp, const SetupL& st, int isample, int L,
    bool ignore_reach, const W& w, int k, const StraightPre& pre, const KinFrames& kf, const real* kt,
    const uint8_t* kb, int ktab_lo) {
  const real t = pre.t;
  const real tv = t * pre.v;  // gait_record's torso advance
  const bool wq = w.want_q(k);
  const NodeK n0 = load_nodek(T, 0);
  const real u[3] = {n0.Jp(0, 0), n0.Jp(1, 0), n0.Jp(2, 0)};
  A34 J = pre.J0;
#if HS_KTE_PRELOAD
  const real* kte = pre.kte;
  const bool kbad = pre.bad;
#else
  real kte[KT_W];  // the table row, loaded once the gait is known to be straight
  bool kbad = false;
  if (kt) {
    const real* e = kt + ((size_t)(isample - ktab_lo) * HS_LMAX + L) * KT_W;
#pragma unroll
    for (int i = 0; i < KT_W; i++) kte[i] = e[i];
    kbad = kb[(isample - ktab_lo) * HS_LMAX + L] != 0;
  }
#endif
  for (int m = 0; m < T->limb_own_n[L]; m++) {  // the chain bodies this limb computes (never a foot)
    const int v = T->limb_own[L][m];
    real bf[BF_W];
#pragma unroll
    for (int i = 0; i < BF_W; i++) bf[i] = m == 0 ? pre.own0[i] : kf.own[L][m][i];
    if (w.want_pos(k)) {
      real* P = w.pos(k, v);
      for (int i = 0; i < 3; i++) P[i] = fma(tv, u[i], bf[i]);
    }
    if (w.want_ust(k)) {
      real* U = w.ust(k, v);
      for (int i = 0; i < 3; i++) U[i] = bf[3 + i];
    }
    if (w.want_centre(k)) {  // a body without a joint: J = its frame, no axis (node_features with J = null)
      real* Jp = w.jpos(k, v);
      real* Jz = w.jz(k, v);
      for (int i = 0; i < 3; i++) Jp[i] = fma(tv, u[i], bf[6 + i]);
      for (int i = 0; i < 3; i++) Jz[i] = real(0);
    }
  }
  if (L == 0) {
    if (wq) {
      real* q = w.q(k);
      q[0] = (real)gp.torso_pos[0] + tv;
      q[1] = (real)gp.torso_pos[1];
      q[2] = (real)gp.torso_pos[2];
      for (int i = 0; i < 3; i++) q[3 + i] = (real)gp.torso_angles[i];
    }
    // node_features of the torso: its joint frame J = I * J_A_parent, not a foot
    if (w.want_pos(k)) {
      real* P = w.pos(k, 0);
      for (int i = 0; i < 3; i++) P[i] = fma(tv, u[i], pre.tor[i]);
    }
    if (w.want_ust(k)) {
      real* U = w.ust(k, 0);
      for (int i = 0; i < 3; i++) U[i] = pre.tor[3 + i];
    }
    if (w.want_centre(k)) {
      real* Jp = w.jpos(k, 0);
      real* Jz = w.jz(k, 0);
      for (int i = 0; i < 3; i++) Jp[i] = n0.Jp(i, 3);
      for (int i = 0; i < 3; i++) Jz[i] = n0.Jp(i, 2);
    }
  }
  STAMP(20);
  J = frame_at(J, u, tv);
  real ja[3], sq[3], cq[3];
  bool bad;
  if (kt) {
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      ja[kk] = kte[kk];
      sincos_k(ja[kk], &sq[kk], &cq[kk]);
    }
    bad = kbad;
    STAMP(21);
  } else {
    straight_ik(T, load_gait(gp), gp, st, t, L, J, ignore_reach, ja, bad);  // untabulated calls only
#pragma unroll
    for (int kk = 0; kk < 3; kk++) sincos_k(ja[kk], &sq[kk], &cq[kk]);
  }
  if (w.want_centre(k)) w.unreach(k, L) = bad ? 1 : 0;
  STAMP(22);
  limb_fk(T, L, J, ja, sq, cq, wq, w, k);
}

// kin_sample for a turning or transformed gait from the preparation pass's rows: the torso's q6 and frame
// at the sample (tor, a RolloutWS::ktor row: the gait record and torso FK kin_sample forms) and the limb's
// joint values (kte, its ktab entry); the chain bodies and the hip frame from the torso frame as in
// kin_sample, then the limb FK
template <class W>
__device__ __attribute__((always_inline)) inline void kin_sample_tab(const hs_topo* T, int L, const W& w, int k,
                                                                     const real* tor, const real* kte, bool bad) {
  const int clen = T->limb_chain_len[L];
  const bool wq = w.want_q(k);
  const NodeK n0 = load_nodek(T, 0);
  const A34 A0 = load34r(tor + 6);
  if (L == 0) {
    if (wq) for (int i = 0; i < 6; i++) w.q(k)[i] = tor[i];
    node_features(T, 0, n0, A0, &n0.Jp, w, k);  // torso joint frame J = I * J_A_parent
  }
  A34 A = A0;
  for (int kk = 1; kk < clen; kk++) {
    const int v = T->limb_chain[L][kk];
    const NodeK nc = load_nodek(T, v);
    A = mul(A, nc.pj);
    if (nc.owner == L) node_features(T, v, nc, A, nullptr, w, k);
  }
  const A34 J = mul(A, node_joint_parent(T, T->limb_child[L]));  // poslimb (lik.cpp:341-347)
  STAMP(20);
  real ja[3], sq[3], cq[3];
#pragma unroll
  for (int kk = 0; kk < 3; kk++) {
    ja[kk] = kte[kk];
    sincos_k(ja[kk], &sq[kk], &cq[kk]);
  }
  if (w.want_centre(k)) w.unreach(k, L) = bad ? 1 : 0;
  STAMP(21);
  STAMP(22);
  limb_fk(T, L, J, ja, sq, cq, wq, w, k);
}

// ---------------------------------------------------------------------------
// D: finite differences at the centre sample, lane = part (dynrec.cpp:175-224)
// ---------------------------------------------------------------------------
// SYNC = false: the caller's next phase reads only this lane's rows (particular_sub's first stage)
template <bool SYNC = true, class W, class SV>
// dt: the sample spacing (SetupL::dt, read once at the wave's start)
__device__ __attribute__((always_inline)) inline void dynamics(const hs_topo* T, real dt, SV& sv, const W& w, int lane) {
  const int n = T->n;
  const int i = lane;
  const real m = (real)T->mass[lane < n ? lane : 0];
  real mr[3], amr[3];
  if (lane < n) {
    const real inv = real(1) / (2 * dt);
    const real *Pp = w.pos(2, i), *P0 = w.pos(0, i), *Pm = w.pos(-2, i);
    const real *Up = w.ust(2, i), *U0 = w.ust(0, i), *Um = w.ust(-2, i);
    real vp[3], vm[3], wp[3], wm[3];
    for (int j = 0; j < 3; j++) {
      vp[j] = Pp[j] - P0[j];
      vp[j] *= inv;
      vm[j] = P0[j] - Pm[j];
      vm[j] *= inv;
      real mp = vp[j] * m, mm = vm[j] * m;
      mr[j] = mp - mm;
      mr[j] *= inv;
      wp[j] = Up[j] - U0[j];
      wp[j] *= inv;
      wm[j] = U0[j] - Um[j];
      wm[j] *= inv;
    }
    // ang_mom = R (I (R^T w)) (compute_ang_mom, dynrec.cpp:205-216) with I the identity: every
    // inertia is ODE's default dMass (dBodyCreate; the reference sets no other, dynrec.cpp:62-68),
    // so R R^T w = w exactly in exact arithmetic and the two rotations (9 + 9 products and the
    // t +- dt rotations kept for them, 3.2 KB of LDS per hexapod rollout) are skipped: this rounds
    // ang_mom once instead of through R^T and R (a few ULPs of |w|, ~1e-15 relative)
    for (int j = 0; j < 3; j++) {
      amr[j] = wp[j] - wm[j];
      amr[j] *= inv;
    }
  }
  // PostL: f overlays the stencil, and lane i's f rows can land on another lane's stencil rows
  // (pos[1][n + i - NM]). Every lane's reads above happen before any lane's writes below only because
  // the wavefront executes them in program order: this wavefront-scope fence keeps the compiler from
  // moving a write above another lane's read; it emits no instruction
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (lane < n) {
    for (int j = 0; j < 3; j++) {
      sv.f[3 * i + j] = mr[j];
      sv.f[3 * (n + i) + j] = amr[j];
    }
    sv.f[3 * i + 2] += m * real(1);  // gravity, g = 1 (dynrec.cpp:291-295)
    DBG(i, mr[0], 2);
    DBG(i, amr[0], 10);
    DBG(i, sv.f[3 * i + 1], 13);
    DBG(i, sv.f[3 * i + 2], 14);
    DBG(i, sv.f[3 * (n + i) + 1], 16);
  }
  if (SYNC) wave_sync();
}

// ---------------------------------------------------------------------------
// S1: tree back-substitution B0 x = f, level by level (deepest first)
// ---------------------------------------------------------------------------
template <class W, class SV>
__device__ __attribute__((always_inline)) inline void particular(const hs_topo* T, SV& sv, const W& w, int lane) {
  const int n = T->n;
  // this lane's node links, loaded once (independent loads, not one L2 round trip per level)
  const hs_node& nd = T->node[lane < n ? lane : 0];
  const int depth = lane < n ? nd.depth : -1, parent = nd.parent, nk = nd.nkids;
  int kids[HS_CMAX];
#pragma unroll
  for (int kk = 0; kk < HS_CMAX; kk++) kids[kk] = nd.kids[kk];
  for (int level = T->max_depth; level >= 0; level--) {
    if (depth == level) {
      const int i = lane;
      const real* Pi = w.pos(0, i);
      real F[3], Tq[3];
      for (int j = 0; j < 3; j++) { F[j] = sv.f[3 * i + j]; Tq[j] = sv.f[3 * (n + i) + j]; }
#pragma unroll
      for (int kk = 0; kk < HS_CMAX; kk++) {
        if (kk >= nk) break;
        const int c = kids[kk];
        const real* Jc = w.jpos(0, c);
        for (int j = 0; j < 3; j++) F[j] += sv.x[3 * c + j];
        real r[3];
        for (int j = 0; j < 3; j++) r[j] = Pi[j] - Jc[j];
        const real* Fc = &sv.x[3 * c];
        Tq[0] -= r[1] * Fc[2] - r[2] * Fc[1];
        Tq[1] -= r[2] * Fc[0] - r[0] * Fc[2];
        Tq[2] -= r[0] * Fc[1] - r[1] * Fc[0];
        for (int j = 0; j < 3; j++) Tq[j] += sv.x[3 * (n + c) + j];
      }
      for (int j = 0; j < 3; j++) sv.x[3 * i + j] = F[j];
      if (parent >= 0) {
        const real* Ji = w.jpos(0, i);
        real r[3];
        for (int j = 0; j < 3; j++) r[j] = Ji[j] - Pi[j];
        Tq[0] -= r[1] * F[2] - r[2] * F[1];
        Tq[1] -= r[2] * F[0] - r[0] * F[2];
        Tq[2] -= r[0] * F[1] - r[1] * F[0];
      }
      for (int j = 0; j < 3; j++) sv.x[3 * (n + i) + j] = Tq[j];
    }
    wave_sync();
  }
}

// S1 as subtree sums: the recursion above, unrolled. With the torso COM p0 as the
// origin, x_i = (F_i, V_i - (J_i - p0) x F_i) (the root: (F_0, V_0)), where over i's subtree
// F_i = sum f_k and V_i = sum (t_k + (P_k - p0) x f_k) -- the same equations (B0 x = f), summed in
// another order. The node table is in preorder, so every subtree is the contiguous range
// [i, i + size_i): a non-root node sums its range directly (a body segment's, the longest, is 7
// parts on the hexapod), the root adds its children's sums; three wavefront syncs instead of one
// per tree level.
template <class W, class SV>
__device__ __attribute__((always_inline)) inline void particular_sub(const hs_topo* T, SV& sv, const W& w, int lane) {
  const int n = T->n;
  const bool on = lane < n;
  const hs_node& nd = T->node[on ? lane : 0];
  const int sz = on ? nd.size : 0, parent = nd.parent, nk = nd.nkids;
  int kids[HS_CMAX];
#pragma unroll
  for (int kk = 0; kk < HS_CMAX; kk++) kids[kk] = nd.kids[kk];
  const real* P0 = w.pos(0, 0);
  const real o[3] = {P0[0], P0[1], P0[2]};
  if (lane == 0) DBG(31, o[0], 15);
  if (lane == 0) DBG(30, o[1], 15);
  if (on) {  // g_i = (f_i, t_i + (P_i - p0) x f_i), the torque part in place
    const int i = lane;
    const real* Pi = w.pos(0, i);
    real f[3], t[3], d[3];
    for (int j = 0; j < 3; j++) { f[j] = sv.f[3 * i + j]; t[j] = sv.f[3 * (n + i) + j]; d[j] = Pi[j] - o[j]; }
    t[0] += d[1] * f[2] - d[2] * f[1];
    t[1] += d[2] * f[0] - d[0] * f[2];
    t[2] += d[0] * f[1] - d[1] * f[0];
    for (int j = 0; j < 3; j++) sv.x[3 * (n + i) + j] = t[j];
    DBG(i, t[0], 3);
  }
  wave_sync();
  real F[3] = {0, 0, 0}, V[3] = {0, 0, 0};
  const bool leafward = on && parent >= 0;
  if (leafward) {  // the subtree's range, in preorder
    for (int m = 0; m < sz; m++) {
      const int kx = lane + m;
      for (int j = 0; j < 3; j++) { F[j] += sv.x[3 * kx + j]; V[j] += sv.x[3 * (n + kx) + j]; }
    }
  }
  if (leafward)  // every lane's reads above precede these writes (one wavefront, in order)
    for (int j = 0; j < 3; j++) { sv.x[3 * lane + j] = F[j]; sv.x[3 * (n + lane) + j] = V[j]; }
  wave_sync();
  if (on && parent < 0) {  // the root: its own g plus its children's sums
    for (int j = 0; j < 3; j++) { F[j] = sv.x[3 * lane + j]; V[j] = sv.x[3 * (n + lane) + j]; }
#pragma unroll
    for (int kk = 0; kk < HS_CMAX; kk++) {
      if (kk >= nk) break;
      const int c = kids[kk];
      for (int j = 0; j < 3; j++) { F[j] += sv.x[3 * c + j]; V[j] += sv.x[3 * (n + c) + j]; }
    }
  }
  if (on) {  // x_i; the root's reads above precede these writes
    real d[3] = {0, 0, 0};
    if (parent >= 0) {
      const real* Ji = w.jpos(0, lane);
      for (int j = 0; j < 3; j++) d[j] = Ji[j] - o[j];
    }
    V[0] -= d[1] * F[2] - d[2] * F[1];
    V[1] -= d[2] * F[0] - d[0] * F[2];
    V[2] -= d[0] * F[1] - d[1] * F[0];
    for (int j = 0; j < 3; j++) { sv.x[3 * lane + j] = F[j]; sv.x[3 * (n + lane) + j] = V[j]; }
    DBG(lane, V[0], 4);
    DBG(lane, F[0], 18);
    DBG(lane, d[0], 17);
  }
  // no trailing sync: the caller's contact list ends with one before x is read across lanes
}

}  // namespace
