// hs_limb.h -- the limb-lane step kernel (round 6) and its launcher, the default kernel of hs_run_calls. Built
// on the step's shared parts (hs_step_base.h, hs_step_kin.h, hs_step_solve.h) and the tile planner
// (hs_limb_tile.h); it needs nothing of hs_rollout_kernel.h. Included by both units (hs_kernels.hip,
// hs_kernels_f32.hip), each with its own copy in its anonymous namespace.
//
// hs_rollout_kernel maps a rollout to 32 lanes and each phase to the lanes it can use: kinematics 30
// (sample, limb) lanes, dynamics and the particular solution one lane per part, the contact blocks four
// lanes per contact, the 6 x 6 Schur system one lane -- 16 % of the issued FP64 lane operations are
// useful. This kernel maps a rollout to a group of 8 lanes, one per limb (the torso
// on lane 7), and keeps a limb's whole step in its lane's registers: the limb FK at the stencil's three
// pos / ust samples, the finite differences of its parts, its links' subtree sums, its contact's blocks
// and its motors' torques -- the work of every phase is per limb, so 6 of 8 lanes are busy in every
// phase, and 8 rollouts share a wavefront. Cross-limb exchanges: the chain bodies' subtree sums and the
// root's through LDS, the contact blocks' Schur entries moved to lane = contact rank (ds_bpermute) and
// summed by DPP in fast_solve_lanes' pairwise order, the motors' work summed in joint order from LDS.
//
// Every value is computed by the same operations in the same order as hs_rollout_kernel's fused step
// (the same helpers, the same expressions), so the outputs are bitwise those of that kernel
// (tests/test_gpu_limb.py). The kernel takes the common case: a call with the preparation pass's IK
// table, a model of the limb-lane class (hs_topo::limb_lane_ok), HS_SOLVE_AUTO, no x / q / dq outputs,
// a step the closed form's tier 1 solves (0 to 6 contacts; a guard near its threshold sets
// HS_FLAG_NEAR_RANK as fast_solve does). Every other step -- a singular contact block (tier 2), nearly
// collinear feet (the Eigen-style path), a joint value past sincos_k_small's range -- is deferred to the
// fixup launch (hs_rollout_kernel FIX_SOLVE), which computes it with hs_rollout_kernel's whole machinery:
// the same (step, rollout) items the fused step launch defers. A mixed plan of limb-lane models runs
// eight rollouts of one model per wavefront (launch_map::limb_model / limb_rollouts).
//
// TILE (launch_map::limb_tile, hs_limb_tile.h): the same step with the wavefront turned around -- one
// rollout x eight steps two apart -- so that the stencil's three FK rows are shared between neighbouring
// groups through LDS (limb_tile_kd); routed by limb_tile() in hs_capi.cpp, the same outputs bitwise
// (tests/test_gpu_limb_tile.py). In step mode a tile-mapped wavefront runs several tiles of its rollout in turn
// (the tile loop, launch_map::limb_tile_loop; tests/test_gpu_limb_tile_loop.py).
#pragma once
#include "hs_limb_tile.h"
#include "hs_step_base.h"
#include "hs_step_kin.h"
#include "hs_step_solve.h"

namespace {

#ifndef HS_LIMB_WAVES
#define HS_LIMB_WAVES 2  // waves per SIMD the limb kernel is built for
#endif
#ifndef HS_LIMB_WAVES_F32
#define HS_LIMB_WAVES_F32 HS_LIMB_WAVES  // the single-precision build's (140 VGPRs, 10.9 KB: 3 fit)
#endif

constexpr int LG = 8;           // lanes per rollout group
constexpr int LGR = WAVE / LG;  // rollouts per wavefront

// HS_DBG builds (tools/limb_dbg.py): value n of the step to g_dbg, 32 slots per (rollout, global step) row
// (dbg_row: b * horizon + s_glob of the lane's group, -1 for an idle one)
__device__ inline int dbg_row(bool live, int b, int horizon, int s_glob) { return live ? b * horizon + s_glob : -1; }
#ifdef HS_DBG
#define LDBG(dbg_r, slot, val, n)                                                                                \
  do {                                                                                                           \
    if (HS_DBG == (n) && (dbg_r) >= 0 && (size_t)(dbg_r) * 32 + (slot) < (1u << 22)) g_dbg[(size_t)(dbg_r) * 32 + (slot)] = (double)(val); \
  } while (0)
#else
#define LDBG(dbg_r, slot, val, n) do {} while (0)
#endif

// steps this process's limb-lane launches deferred to the fixup launch (hs_limb_stats; one atomic per
// deferred step, rare)
__device__ unsigned long long g_limb_deferred;

template <int NM, bool FORCES = false>
struct LimbLds {
  real g[NM][6];     // per part g_i = (f_i, t_i + (P_i - p0) x f_i); a root kid's slot then its subtree sums
  real a[6];         // the root's x (torso force, torque): the zeroth-order right-hand side
  real wd[HS_NMAX];  // the motors' positive work of the step, in joint order
  real p[FORCES ? NM : 1][3];  // forces mode: the parts' positions at the centre sample (forces_solve's s, Q sums)
};

// a value of lane `src` of this lane's group (ds_bpermute)
__device__ inline real grp_get(real v, int src) { return __shfl(v, src); }
__device__ inline float grp_getf(float v, int src) { return __shfl(v, src); }
// any lane of the 8-lane group
__device__ inline bool grp_any(bool p, int gbase) { return ((__ballot(p) >> gbase) & 0xFFull) != 0; }
__device__ inline uint32_t grp_or(uint32_t v) {
  v |= (uint32_t)__shfl_xor((int)v, 1);
  v |= (uint32_t)__shfl_xor((int)v, 2);
  v |= (uint32_t)__shfl_xor((int)v, 4);
  return v;
}
// sum over the group's lanes 0..7 holding per-contact values by rank (0 past nc): ((v3 + v2) + (v1 + v0)) +
// ((v4 + v5) + (v6 + v7)) -- fast_solve_lanes' pairwise order over its contact lanes (row_shr 4, row_shr 8,
// xor 16: (v3 + v2) + (v1 + v0) and (v7 + v6) + (v5 + v4), then their sum); every lane gets the total
__device__ inline real rank8_sum(real v) {
  v += dpp_r<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_r<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_r<0x141>(v);  // row_half_mirror: lane i <- 7 - i, the other quad's sum
  return v;
}

// opaque_vals (hs_math.h): values made opaque where hs_rollout_kernel passes them through LDS

// The same pointer, opaque to the optimizer: the three samples' FK read the same topology entries (a
// limb's link products, rotations, COMs: 80 reals) and frames, and merged loads would keep them live
// across all three -- 160 VGPRs on top of the samples' results. Loads through a fresh opaque pointer per
// sample are issued again (L1 hits) where that sample uses them.
// (through an address-space-1 pointer: a generic one would turn the topology reads into flat loads)
__device__ inline const hs_topo* opaque_s(const hs_topo* p) {
  using gptr = const __attribute__((address_space(1))) hs_topo*;
  gptr q = (gptr)p;
  asm volatile("" : "+s"(q));
  return (const hs_topo*)q;
}

// One link of limb_fk (its operations): the next joint frame Jv (from the previous link's hinge frame H),
// the hinge frame H, the link's pos and ust, and at the centre sample its joint position and axis and
// (the foot link) the foot
template <bool CENTRE>
__device__ __attribute__((always_inline)) inline void fk_link(const hs_topo* T, const hs_link& lk, int kk, A34& Jv,
                                                              A34& H, real s, real c, real* P, real* U, real* Jp,
                                                              real* Jz, real* fp, bool& contact) {
  if (kk > 0) Jv = mul(H, load34(lk.P));
  H = mul_hinge(Jv, c, s);
  {
    const real cm[3] = {(real)lk.com[0], (real)lk.com[1], (real)lk.com[2]};
    mulp(H, cm, P);
  }
  {
    real R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (real)lk.Rpj[i];
    auto a_rc = [&](int r, int c) { return H(r, 0) * R[c * 3 + 0] + H(r, 1) * R[c * 3 + 1] + H(r, 2) * R[c * 3 + 2]; };
    U[0] = (a_rc(2, 1) - a_rc(1, 2)) / 2;
    U[1] = (a_rc(0, 2) - a_rc(2, 0)) / 2;
    U[2] = (a_rc(1, 0) - a_rc(0, 1)) / 2;
  }
  if (CENTRE) {
#pragma unroll
    for (int i = 0; i < 3; i++) Jp[i] = Jv(i, 3);
#pragma unroll
    for (int i = 0; i < 3; i++) Jz[i] = Jv(i, 2);
    if (kk == 2) {  // the foot link (hs_topo::limb_lane_ok)
      const real cp[3] = {(real)lk.cap[0], (real)lk.cap[1], (real)lk.cap[2]};
      mulp(H, cp, fp);
      contact = fp[2] < (real)(T->rcap + 1e-4);
    }
  }
}

// dynamics()' finite differences of one part (dynrec.cpp:175-224) from its pos / ust at t - 2dt, t, t + 2dt
__device__ inline void part_dyn(real m, real inv, const real* Pm, const real* P0, const real* Pp, const real* Um,
                                const real* U0, const real* Up, real* f) {
  real vp[3], vm[3], mr[3], wp[3], wm[3], amr[3];
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
  for (int j = 0; j < 3; j++) {
    amr[j] = wp[j] - wm[j];
    amr[j] *= inv;
  }
  for (int j = 0; j < 3; j++) {
    f[j] = mr[j];
    f[3 + j] = amr[j];
  }
  opaque_vals<6>(f);    // dynamics() stores f and adds gravity to the stored value
  f[2] += m * real(1);  // gravity, g = 1 (dynrec.cpp:291-295)
}

// particular_sub's first stage for one part: g = (f, t + (P - o) x f)
__device__ inline void part_g(const real* P, const real* o, real* f) {
  opaque_vals<6>(f);  // f as dynamics() stores it (LDS), then g as particular_sub stores it
  real d[3];
  for (int j = 0; j < 3; j++) d[j] = P[j] - o[j];
  f[3] += d[1] * f[2] - d[2] * f[1];
  f[4] += d[2] * f[0] - d[0] * f[2];
  f[5] += d[0] * f[1] - d[1] * f[0];
  opaque_vals<6>(f);
}

// pos and ust of a jointless chain body or of the torso at one sample: straight gaits from the setup's
// features at tv = 0 (kin_sample_straight), turning ones from the body frame A (node_features)
struct BodyS {
  real P[3], U[3];
};
__device__ inline BodyS body_straight(const real* bf, const real* u, real tv) {
  BodyS s;
  for (int i = 0; i < 3; i++) s.P[i] = fma(tv, u[i], bf[i]);
  for (int i = 0; i < 3; i++) s.U[i] = bf[3 + i];
  return s;
}
__device__ inline BodyS body_frame(const A34& A, const real* com) {
  BodyS s;
  mulp(A, com, s.P);
  s.U[0] = (A(2, 1) - A(1, 2)) / 2;
  s.U[1] = (A(0, 2) - A(2, 0)) / 2;
  s.U[2] = (A(1, 0) - A(0, 1)) / 2;
  return s;
}

// Limb L's hip joint frame J at one sample and its chain body's pos / ust (limb_own_n <= 1, hs_topo::
// limb_lane_ok): straight gaits from KinFrames at tv (kf: the rollout's, W.kf or the tile loop's copy of it
// in LDS), turning ones from the torso record's frame and the chain products (kin_sample_tab)
__device__ __attribute__((always_inline)) inline A34 limb_frame(const hs_topo* T, int L, bool straight, const bool own,
                                                                const RolloutWS& W, const KinFrames& kf, int row,
                                                                const real* u, real tv, BodyS& ob) {
  if (straight) {
    if (own) ob = body_straight(kf.own[L][0], u, tv);
    return frame_at(load34r(kf.J0[L]), u, tv);
  }
  A34 A = load34r(W.ktor[row] + 6);
  const int clen = T->limb_chain_len[L];
  for (int kk = 1; kk < clen; kk++) {
    const int v = T->limb_chain[L][kk];
    A = mul(A, node_pj(T, v));
    if (T->node[v].owner_limb == L) {
      const real com[3] = {(real)T->node[v].com[0], (real)T->node[v].com[1], (real)T->node[v].com[2]};
      ob = body_frame(A, com);
    }
  }
  return mul(A, node_joint_parent(T, T->limb_child[L]));
}

// the links' pos and ust at an outer sample of the stencil (the limb FK without the centre's features)
// (big: a joint value sincos_k_small does not take, sincos_big of hs_step_kin.h: the step is deferred)
__device__ __attribute__((always_inline)) inline void limb_outer(const hs_topo* T, const hs_link (&LK)[3], const A34& J,
                                                                 const real* ja, real (&P)[3][3], real (&U)[3][3],
                                                                 bool& big) {
  real sq[3], cq[3];
#pragma unroll
  for (int kk = 0; kk < 3; kk++) {
    big |= sincos_big(ja[kk]);
    sincos_k_small(ja[kk], &sq[kk], &cq[kk]);
  }
  A34 Jv = J, H;
  real nul[3];
  bool nc = false;
#pragma unroll
  for (int kk = 0; kk < 3; kk++) fk_link<false>(T, LK[kk], kk, Jv, H, sq[kk], cq[kk], P[kk], U[kk], nul, nul, nul, nc);
}

// sh.k.outer's rows, [Pm, Um, Pp, Up][link][component], a limb lane's column each: a sample's links to the
// minus rows (o0 = 0) or the plus rows (o0 = 18) of column col, and link kk's four vectors back
__device__ __attribute__((always_inline)) inline void outer_put(real (&outer)[36][LGR * HS_LMAX], int o0, int col,
                                                                const real (&P)[3][3], const real (&U)[3][3]) {
#pragma unroll
  for (int kk = 0; kk < 3; kk++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      outer[o0 + 3 * kk + j][col] = P[kk][j];
      outer[o0 + 9 + 3 * kk + j][col] = U[kk][j];
    }
}
__device__ __attribute__((always_inline)) inline void outer_get(const real (&outer)[36][LGR * HS_LMAX], int kk, int col,
                                                                real* Pm, real* Um, real* Pp, real* Up) {
#pragma unroll
  for (int j = 0; j < 3; j++) {
    Pm[j] = outer[3 * kk + j][col];
    Um[j] = outer[9 + 3 * kk + j][col];
    Pp[j] = outer[18 + 3 * kk + j][col];
    Up[j] = outer[27 + 3 * kk + j][col];
  }
}

// a joint value past sincos_k_small's range at any of the stencil's three rows defers the step
__device__ inline bool limb_rows_big(const real* qm, const real* q0, const real* qp) {
  bool big = false;
#pragma unroll
  for (int kk = 0; kk < 3; kk++) big |= sincos_big(qm[kk]);
#pragma unroll
  for (int kk = 0; kk < 3; kk++) big |= sincos_big(q0[kk]);
#pragma unroll
  for (int kk = 0; kk < 3; kk++) big |= sincos_big(qp[kk]);
  return big;
}

// the whole step to the fixup launch (hs_rollout_kernel FIX_SOLVE): the group's first lane lists it.
// item: the rollout's slot in hs_rollout_kernel's layout (2 * wavefront + half)
__device__ inline void limb_defer(const hs::launch_map& mp, bool live, int l, int s_glob, int item) {
  if (l == 0 && live) {
    atomicAdd(&g_limb_deferred, 1ull);  // hs_limb_stats
    const int it = atomicAdd(mp.fix_count, 1);
    mp.fix_items[2 * it] = s_glob - mp.fused_s0;  // the local step (formed here: not a register held up to here)
    mp.fix_items[2 * it + 1] = item;
  }
}

// the limb whose foot holds contact rank `rank` of the group's contact mask cm (foot order; 0 where none does)
__device__ inline int rank_limb(const hs_topo* T, uint32_t cm, int nl, int rank) {
  int src = 0;
  for (int L2 = 0; L2 < nl; L2++) {
    const int f2 = T->link[L2][2].foot;
    if (((cm >> f2) & 1) && __popc(cm & ((1u << f2) - 1)) == rank) src = L2;
  }
  return src;
}

// A contact's first-order block D_c (packed lower: 00 10 11 20 21 22) and g_c on its limb lane
// (fast_solve_lanes: joint m of the foot's chain, foot link first, on lane m of a quad, summed
// ((m0 + m1) + (m2 + m3)); the chain's jointless bodies add exact zeros)
__device__ __attribute__((always_inline)) inline void contact_block(const real (&Jp)[3][3], const real (&Jz)[3][3],
                                                                    const real (&xt)[3][3], const real* fp, real* Dp6,
                                                                    real* gc) {
  real tD[3][6], tg[3][3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const int p = 2 - m;
    real Dp[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    real da[3], va[3][3];
    for (int r = 0; r < 3; r++) da[r] = Jp[p][r] - fp[r];
    cross_rows(da, va);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const real w2 = Jz[p][r] * Jz[p][r];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        if (i == r) continue;
#pragma unroll
        for (int j = 0; j <= i; j++)
          if (j != r) Dp[i * (i + 1) / 2 + j] += w2 * va[r][i] * va[r][j];
        g[i] += w2 * va[r][i] * xt[p][r];
      }
    }
    for (int e = 0; e < 6; e++) tD[m][e] = Dp[e];
    for (int i = 0; i < 3; i++) tg[m][i] = g[i];
  }
#pragma unroll
  for (int e = 0; e < 6; e++) Dp6[e] = (tD[0][e] + tD[1][e]) + (tD[2][e] + real(0));
#pragma unroll
  for (int i = 0; i < 3; i++) gc[i] = (tg[0][i] + tg[1][i]) + (tg[2][i] + real(0));
}

// hs_limb_kernel's forces mode after S1 (forces_solve's fast path, every value by its operations in its
// order): the parts' s, Q sums over nodes 1 .. n - 1 in node order (every lane of the group), the limb's
// blocks on its lane (forces_limb_block), the sums over the limbs in limb order (a DPP chain: lane l adds
// its term to lane l - 1's partial sum, the total on lane nl - 1), the 6 x 6 system on every lane, each
// limb's foot forces on its lane
template <int NM>
__device__ __attribute__((always_inline)) inline void limb_forces(const hs_topo* T, const hs_run_args& a,
                                                                  const hs::launch_map& mp, LimbLds<NM, true>& S, bool limb,
                                                                  int l, int L, int gbase, int nl, bool live, int b,
                                                                  int s_glob, const real* o,
                                                                  const real (&Jp)[3][3], const real (&Jz)[3][3],
                                                                  const real (&Pc)[3][3], const real* fp,
                                                                  const real (&xt)[3][3], bool bad, bool big) {
  const int n = T->n;
  [[maybe_unused]] const int dbg_r = dbg_row(live, b, a.horizon, s_glob);
  real ts[9];
#pragma unroll
  for (int q = 0; q < 9; q++) ts[q] = 0;
  for (int i = 1; i < n; i++) {
    real r[3];
    for (int t = 0; t < 3; t++) r[t] = S.p[i][t] - o[t];
    // forces_solve's lanes select between r_a and the product r_a r_b before adding (a lane-dependent
    // select): the product is rounded, then added -- not one FMA
    real q[6] = {r[0] * r[0], r[1] * r[1], r[2] * r[2], r[0] * r[1], r[0] * r[2], r[1] * r[2]};
    opaque_vals<6>(q);
    ts[0] += r[0];
    ts[1] += r[1];
    ts[2] += r[2];
    for (int j = 0; j < 6; j++) ts[3 + j] += q[j];
  }
  opaque_vals<9>(ts);  // forces_solve keeps them in LDS (sv.y)
  const int dbg_f = T->link[L][2].foot;
  (void)dbg_f;
  if (l == 0) LDBG(dbg_r, 0, ts[3], 30);
  const size_t orow = (size_t)b * a.horizon + s_glob;
  // the limb's blocks (forces_solve's stages), its 27 terms of the sums over the limbs formed as soon as
  // both factors exist: K_f - S_l (packed lower), q_f + e_l -- forces_solve's fr.b - fr.a / fr.b + fr.a,
  // each product rounded as its LDS rows hold it (the two 27-entry blocks are never live together)
  real Ct[18], Bd[6], Bl[9], rdB[3], rb[3], vl[27];
  bool okB = true;
  if (limb) {
    const real* z = inp(mp.tau_in) + (live ? orow : 0) * mp.st_tau;
    real zz[3];
    for (int kk = 0; kk < 3; kk++) zz[kk] = z[T->node[T->limb_node[L][kk]].hinge];
    ForcesRows F;
    forces_rows(F, Jp, Jz, Pc, fp, o, xt, zz);
    okB = forces_foot(F, fp, o, Ct, Bd, Bl, rdB, rb);
    LDBG(dbg_r, 24 + dbg_f, Ct[0], 36);
    LDBG(dbg_r, 24 + dbg_f, rb[0], 37);
    if (okB) {
      ForcesV G;
      forces_v(G, Ct, Bl, rdB, rb);
#pragma unroll
      for (int e = 0; e < 27; e++) {
        const TriWalk<> t(e < 21 ? e : 0);
        real pa = e < 21 ? F.prod(t.r, t.c) : F.prod(e - 21, 9);
        real pb = e < 21 ? G.vprod(t.r, t.c) : G.vprod(e - 21, 6);
        opaque_vals<1>(&pa);  // fr.a / fr.b (LDS)
        opaque_vals<1>(&pb);
        vl[e] = (e < 21) ? pb - pa : pb + pa;
      }
    }
  }
  const bool fast = !grp_any(limb && !okB, gbase);
  if (!fast || grp_any(big, gbase)) {  // the dense normal equations: the forces fixup's (forces_solve)
    limb_defer(mp, live, l, s_glob, b);
    return;
  }
  // K = W_tt - sum S_l + sum K_f, rhs = sum (q_f + e_l) - d_t
  real kv[27];
#pragma unroll
  for (int e = 0; e < 27; e++) {
    const real v = limb ? vl[e] : real(0);
    real s = real(0) + v;
    for (int k = 1; k < nl; k++) {
      const real prev = dpp_r<0x111>(s);  // row_shr 1: lane l - 1's partial sum
      if (l >= 1) s = prev + v;
    }
    const real tot = grp_get(s, gbase + nl - 1);
    const real dtv = (e < 21) ? real(0) : (e < 24 ? S.a[e - 21] : S.a[e - 21]);
    kv[e] = (e < 21) ? wtt_entry(e, ts, n) + tot : tot - dtv;
  }
  opaque_vals<27>(kv);  // fr.a[0] (LDS)
  if (l == 0) LDBG(dbg_r, 1, kv[0], 33);
  real K[36], rd[6], lam[6];
#pragma unroll
  for (int r = 0; r < 6; r++) {
#pragma unroll
    for (int c = 0; c < 6; c++) K[6 * r + c] = (c <= r) ? kv[pk(r, c)] : real(0);
    lam[r] = kv[21 + r];
  }
  ldl_n<6>(K, real(0), rd);  // >= I
  ldl_solve_n<6>(K, rd, lam);
  if (l == 0) LDBG(dbg_r, 2, lam[0], 34);
  bool nan = false;
  real t[3] = {0, 0, 0};
  if (limb) {  // y_f = B_f^-1 (r_f - C~_f^T lam)
    for (int k = 0; k < 3; k++) {
      real s = rb[k];
      for (int r = 0; r < 6; r++) s -= Ct[3 * r + k] * lam[r];
      t[k] = s;
    }
    ldl_solve_n<3>(Bl, rdB, t);
    LDBG(dbg_r, 24 + dbg_f, t[0], 35);
    for (int k = 0; k < 3; k++) nan |= t[k] != t[k];
    const int f = T->link[L][2].foot;
    if (live && a.cf)
      for (int k = 0; k < 3; k++) outp(a.cf)[orow * mp.st_cf + 3 * f + k] = t[k];
  }
  if (live && a.cf)  // a mixed plan's columns past this model's feet
    for (int c = 3 * T->nf + l; c < mp.st_cf; c += LG) outp(a.cf)[orow * mp.st_cf + c] = real(0);
  const bool any_nan = grp_any(nan, gbase), any_bad = grp_any(limb && bad, gbase);
  if (l == 0 && live && a.flags) a.flags[orow] = (any_nan ? HS_FLAG_NAN : 0u) | (any_bad ? HS_FLAG_UNREACH : 0u);
}

// The tile loop's wavefront constants. What a tile reads of the model per limb lane and of the rollout's
// record is the same in every tile of the chunk, and read from global memory it is a chain of dependent
// round trips per tile (limb_node -> mass, the slot -> t_tab -> the frames) that only the SIMD's one other
// wave can cover. The head stages it in LDS once per wavefront, beside the link records.
// A limb lane's model constants (entry l: limb l; for l < nkids also the root's kid l)
struct LimbLaneK {
  real m[3], mown;  // masses of the limb's three links and of the chain body it owns
  uint32_t nodes;   // the links' nodes, a byte each (top first), the owned chain body's node in byte 3
  uint32_t hf;      // the links' hinges, a byte each, the foot index in byte 3
  uint32_t kid;     // byte 0: the root's kid l, byte 1: its subtree size, byte 2: the limb owns a chain body
  uint32_t pad_;
};
static_assert(HS_NMAX < 256 && HS_LMAX < 256, "LimbLaneK packs node, hinge and foot indices into bytes");
// the rollout's sample times and straight-gait frames as RolloutWS holds them (one contiguous copy)
struct LimbRolloutK {
  real t_tab[HS_KTAB];
  KinFrames kf;
};
static_assert(offsetof(RolloutWS, kf) == offsetof(RolloutWS, t_tab) + sizeof(real[HS_KTAB]) &&
                  offsetof(LimbRolloutK, kf) == sizeof(real[HS_KTAB]),
              "LimbRolloutK mirrors RolloutWS from t_tab through kf");

// What limb_step and limb_tile_kd read of the model per limb lane: from the topology (the packed mapping,
// forces mode, the fp32 build), or from the wavefront's LimbLaneK block in LDS (the tile loop)
template <bool LOOP>
struct LimbModelK {
  const hs_topo* T;
  const LimbLaneK* k;
  __device__ bool own(int L) const {
    if constexpr (LOOP) return (k[L].kid >> 16) & 1;
    else return T->limb_own_n[L] > 0;
  }
  __device__ int node(int L, int kk) const {
    if constexpr (LOOP) return (k[L].nodes >> (8 * kk)) & 255;
    else return T->limb_node[L][kk];
  }
  __device__ int own_node(int L) const {
    if constexpr (LOOP) return k[L].nodes >> 24;
    else return T->limb_own[L][0];
  }
  __device__ real mass(int L, int kk) const {
    if constexpr (LOOP) return k[L].m[kk];
    else return (real)T->mass[T->limb_node[L][kk]];
  }
  __device__ real mass_own(int L) const {
    if constexpr (LOOP) return k[L].mown;
    else return (real)T->mass[T->limb_own[L][0]];
  }
  __device__ int hinge(int L, int kk) const {
    if constexpr (LOOP) return (k[L].hf >> (8 * kk)) & 255;
    else return T->link[L][kk].hinge;
  }
  __device__ int foot(int L) const {
    if constexpr (LOOP) return k[L].hf >> 24;
    else return T->link[L][2].foot;
  }
  __device__ int kid(int l) const {
    if constexpr (LOOP) return k[l].kid & 255;
    else return T->node[0].kids[l];
  }
  __device__ int kid_size(int l, int c) const {
    if constexpr (LOOP) return (k[l].kid >> 8) & 255;
    else return T->node[c].size;
  }
};

// ---- the tile mapping's K and D phase ----
// A tile-mapped wavefront is one rollout x eight steps: group g runs the local step of slot 8 tile + g of the
// launch's sequence (hs_limb_tile.h), two rows after group g - 1's wherever the sequence has no break, so
// its stencil rows t - 2dt and t + 2dt are its neighbours' centre rows. Every limb lane runs the FK of its
// group's centre row only and
// stores the links' pos / ust into the outer rows of the groups that read them (sh.k.outer, the packed
// mapping's layout: the step's lanes read their own columns as before). A row no neighbour's centre holds
// -- the minus row of the tile's first group, the plus row of its last, both sides of a break -- is a
// request: the first of them run in the same pass on the lanes idle in every group (l >= n_limbs), the
// rest, eight at a time, in further passes taken only when there are any. Whether a neighbour holds a row
// is decided from the rows themselves (row0 of the neighbour against this group's), so sharing changes
// where a value is computed, never the value. A turning gait's chain body (its pos / ust come out of
// limb_frame with the hip frame) is pushed from the FK's lane to the reading lane (ds_permute).

// a tile's entry of the launch's descriptor (the TILE kernels' last argument)
__device__ inline const limb_tile_entry& limb_tile_entry_of(const limb_tile_desc& d, int tile) { return d.tile[tile]; }
// v sent to lane dst: a lane receives what the one lane naming it sent. A lane with nothing to send names
// lane LG - 1 (group 0's torso lane), which is no limb's lane and reads nothing it receives
static_assert(HS_LMAX < LG, "lane LG - 1 of a group must not be a limb lane (lane_push's idle target)");
__device__ inline real lane_push(real v, int dst) {
  if constexpr (sizeof(real) == 8) {
    const double d = (double)v;
    const int lo = __builtin_amdgcn_ds_permute(dst << 2, __double2loint(d));
    const int hi = __builtin_amdgcn_ds_permute(dst << 2, __double2hiint(d));
    return (real)__hiloint2double(hi, lo);
  } else {
    return (real)__int_as_float(__builtin_amdgcn_ds_permute(dst << 2, __float_as_int((float)v)));
  }
}

// What the K and D phase of either mapping leaves to the phases after it, per limb lane
struct LimbKD {
  real g3[3][6];  // the links' g (f, then f's torque part moved about o)
  real Jp[3][3], Jz[3][3], fp[3];
  bool contact = false;
  bool own = false;  // this limb computes a chain body (limb_own_n = 1)
  real gown[6];
  real jvel[3];
  real Pc[3][3], Pown[3];  // forces mode: the links' and the chain body's positions at the centre
  bool bad = false, big = false;
};

// One link of the centre row once its FK is done, the same in both mappings: the fences where
// hs_rollout_kernel's later phases read the features from LDS, the link's outer rows, its finite differences
// and its g about o, with the K and D phase's HS_DBG taps. BARRIER: the packed mapping's sched_barrier ahead of
// the outer reads.
template <bool FORCES, bool BARRIER, bool LOOP>
__device__ __attribute__((always_inline)) inline void limb_centre_link(
    const LimbModelK<LOOP>& mk, const real (&outer)[36][LGR * HS_LMAX], int ol, int l, int L, int kk, real* P0, real* U0,
    real* Jp, real* Jz, real* fp, real* Pc, const real* o, real inv, real* g, int dbg_r) {
  opaque_vals<3>(P0);
  if constexpr (FORCES)
    for (int j = 0; j < 3; j++) Pc[j] = P0[j];
  opaque_vals<3>(U0);
  opaque_vals<3>(Jp);
  opaque_vals<3>(Jz);
  if (kk == 2) opaque_vals<3>(fp);
  real Pm[3], Um[3], Pp[3], Up[3];
  if constexpr (BARRIER) __builtin_amdgcn_sched_barrier(0);
  outer_get(outer, kk, ol, Pm, Um, Pp, Up);
  part_dyn(mk.mass(L, kk), inv, Pm, P0, Pp, Um, U0, Up, g);
  [[maybe_unused]] const int node = mk.node(L, kk);  // (HS_DBG builds: the part's row)
  LDBG(dbg_r, node, P0[0], 1);
  LDBG(dbg_r, node, U0[0], 5);
  LDBG(dbg_r, node, g[0], 2);
  LDBG(dbg_r, node, g[3], 10);
  LDBG(dbg_r, node, g[1], 13);
  LDBG(dbg_r, node, g[2], 14);
  LDBG(dbg_r, node, g[4], 16);
  if (l == 0) LDBG(dbg_r, 31, o[0], 15);
  if (l == 0) LDBG(dbg_r, 30, o[1], 15);
  LDBG(dbg_r, node, Um[0], 9);
  LDBG(dbg_r, node, Up[0], 11);
  LDBG(dbg_r, node, Pm[0], 12);
  part_g(P0, o, g);
  LDBG(dbg_r, node, g[3], 3);
}

// The tile loop's reads of what the preparation pass tabulated per table row (RolloutWS::kvel, kbig, beside
// kbad): the centre row's joint rates and the range bits of the stencil's three FK rows, seven loads whose
// values nothing needs before the K and D phase ends. issue() starts them; finish() is their first use (the
// bytes enter it as opaque values: their tests formed where they are loaded would wait for the loads there).
struct LimbTileRates {
  real v[3];
  uint32_t big0, big2, big4, bad;
  __device__ __attribute__((always_inline)) inline void issue(const RolloutWS& W, int row0, int L) {
#pragma unroll
    for (int kk = 0; kk < 3; kk++) v[kk] = W.kvel[row0 + 2][L][kk];
    big0 = W.kbig[row0][L];
    big2 = W.kbig[row0 + 2][L];
    big4 = W.kbig[row0 + 4][L];
    bad = W.kbad[row0 + 2][L];
  }
  __device__ __attribute__((always_inline)) inline void finish(LimbKD& kd) {
    asm volatile("" : "+v"(big0), "+v"(big2), "+v"(big4), "+v"(bad));
    kd.bad = bad != 0;
    kd.big |= (big0 | big2 | big4) != 0;
#pragma unroll
    for (int kk = 0; kk < 3; kk++) kd.jvel[kk] = v[kk];
  }
};

#ifdef HS_STAMPS
#undef HS_STAMP_GATE
#define HS_STAMP_GATE stamp_on  // limb_tile_kd's and limb_step's: the tile loop's chosen iteration
#endif
// mk, kf, ttab: the model's per-lane constants, the rollout's straight-gait frames and its sample times, from
// global memory or (LOOP) from the wavefront's copies in LDS
template <bool FORCES, bool LOOP>
__device__ __attribute__((always_inline)) inline void limb_tile_kd(
    const hs_topo* T_, const LimbModelK<LOOP>& mk, const KinFrames& kf, const real* ttab,
    real (&outer)[36][LGR * HS_LMAX], hs_link (&links)[HS_LMAX][3], const RolloutWS& W, bool straight,
    const real* u, real v, int lane, int nl, bool limb, int L, bool live, int row0, uint32_t M, uint64_t req,
    const real* tv, const real* o, real inv, real dt, LimbKD& kd, int dbg_r, bool stamp_on) {
  (void)dbg_r;
  (void)stamp_on;  // (HS_STAMPS builds: this tile stamps)
  const int grp = lane >> 3, l = lane & 7;
  // The tile's requests, from its descriptor (wave-uniform): M's bit 2 g is group g's minus row, bit 2 g + 1
  // its plus row, served in bit order; req lists them in that order, 4 bits each. A live group's row that is
  // no request is its neighbour's centre row.
  const bool shm = live && !((M >> (2 * grp)) & 1);      // group g - 1's centre row is this group's minus row
  const bool shp = live && !((M >> (2 * grp + 1)) & 1);  // group g + 1's centre row is this group's plus row
  const int nreq = __popc(M);
  auto nth_req = [req](int r) { return (int)(req >> (4 * r)) & 15; };  // the r-th request's bit of M (r < 16)
  const int nidle = LG - nl;             // lanes of a group the step leaves idle in this phase
  const int E0 = (LGR * nidle) / nl;     // requests the first pass takes on them
  // the pass that serves this group's minus / plus row (a turning gait's chain body arrives with it)
  const int rqm = __popc(M & ((1u << (2 * grp)) - 1)), rqp = __popc(M & ((1u << (2 * grp + 1)) - 1));
  const int pm = shm || rqm < E0 ? 0 : 1 + (rqm - E0) / LGR, pp = shp || rqp < E0 ? 0 : 1 + (rqp - E0) / LGR;
  auto col = [](int ln) { return (ln >> 3) * HS_LMAX + (ln & 7); };  // a limb lane's column of sh.k.outer
  real P[3][3], U[3][3];  // a limb lane's links at its centre row
  BodyS om, op, oc;       // its chain body at the three rows
  kd.own = limb && mk.own(L);
  [[maybe_unused]] LimbTileRates tr;
  // ---- pass 0: the centre rows on the limb lanes, the first requests on the idle lanes ----
  {
    int rq = 0, fL = L;
    bool extra = false;
    if (!limb) {
      const int j = grp * nidle + (l - nl);
      rq = j / nl;
      fL = j - rq * nl;
      extra = rq < E0 && rq < nreq;
      if (!extra) rq = 0, fL = 0;
    }
    const int bit = nth_req(rq), gr = bit >> 1, side = bit & 1;
    const int rr = __shfl(row0, gr * LG);
    const int frow = limb ? row0 + 2 : rr + 4 * side;
    const int dst = gr * LG + fL;
    // the lanes whose minus / plus rows this lane's FK fills (-1: none)
    const int dm = limb ? (shp ? lane + LG : -1) : (extra && side == 0 ? dst : -1);
    const int dp = limb ? (shm ? lane - LG : -1) : (extra && side == 1 ? dst : -1);
    BodyS ob;
#pragma unroll
    for (int j = 0; j < 3; j++) ob.P[j] = ob.U[j] = real(0);
    if (limb || extra) {
      const hs_topo* T = opaque_s(T_);
      const bool fown = LimbModelK<LOOP>{T, mk.k}.own(fL);
      // (tile loop: a limb lane's row is its centre row, whose time it holds; only a request looks one up)
      const real tvf = LOOP && limb ? tv[2] : ttab[frow] * v;
      const A34 J = limb_frame(T, fL, straight, fown, W, kf, frow, u, tvf, ob);
      const real* ja = W.ktab[frow][fL];
      real sq[3], cq[3];
#pragma unroll
      for (int kk = 0; kk < 3; kk++) sincos_k_small(ja[kk], &sq[kk], &cq[kk]);
      A34 Jv = J, H;
#pragma unroll
      for (int kk = 0; kk < 3; kk++)
        fk_link<true>(T, links[fL][kk], kk, Jv, H, sq[kk], cq[kk], P[kk], U[kk], kd.Jp[kk], kd.Jz[kk], kd.fp, kd.contact);
      if (dm >= 0) outer_put(outer, 0, col(dm), P, U);
      if (dp >= 0) outer_put(outer, 18, col(dp), P, U);
    }
    if (!limb) kd.contact = false;
    oc = ob;
    if (!straight) {  // (the same on every lane: one rollout)
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const real val = j < 3 ? ob.P[j] : ob.U[j - 3];
        const real vm = lane_push(val, dm >= 0 ? dm : LG - 1), vp = lane_push(val, dp >= 0 ? dp : LG - 1);  // (lane LG - 1: see lane_push)
        if (pm == 0) (j < 3 ? om.P[j] : om.U[j - 3]) = vm;
        if (pp == 0) (j < 3 ? op.P[j] : op.U[j - 3]) = vp;
      }
    }
  }
  STAMP(1);
  // ---- further passes: eight requests each, request base + g on group g's limb lanes ----
  for (int base = E0, pass = 1; base < nreq; base += LGR, pass++) {
    const bool act = limb && base + grp < nreq;
    const int bit = nth_req(act ? base + grp : 0), gr = bit >> 1, side = bit & 1;
    const int frow = __shfl(row0, gr * LG) + 4 * side;
    const int dst = act ? gr * LG + L : -1;
    BodyS ob;
#pragma unroll
    for (int j = 0; j < 3; j++) ob.P[j] = ob.U[j] = real(0);
    __builtin_amdgcn_sched_barrier(0);
    if (act) {
      real P2[3][3], U2[3][3];
      bool nb = false;
      const hs_topo* T = opaque_s(T_);
      limb_outer(T, links[L], limb_frame(T, L, straight, kd.own, W, kf, frow, u, ttab[frow] * v, ob), W.ktab[frow][L], P2,
                 U2, nb);
      outer_put(outer, side ? 18 : 0, col(dst), P2, U2);
    }
    if (!straight) {
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const real val = j < 3 ? ob.P[j] : ob.U[j - 3];
        const real vm = lane_push(val, act && side == 0 ? dst : LG - 1), vp = lane_push(val, act && side == 1 ? dst : LG - 1);
        if (pm == pass) (j < 3 ? om.P[j] : om.U[j - 3]) = vm;
        if (pp == pass) (j < 3 ? op.P[j] : op.U[j - 3]) = vp;
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  STAMP(2);
  if constexpr (LOOP)
    if (limb) tr.issue(W, row0, L);
  wave_sync();  // every group's outer rows
  if (limb) {
    if (kd.own) {
      if (straight) {  // kin_sample_straight's features: limb_frame's own expressions at the outer rows
        om = body_straight(kf.own[L][0], u, tv[0]);
        op = body_straight(kf.own[L][0], u, tv[4]);
      }
      part_dyn(mk.mass_own(L), inv, om.P, oc.P, op.P, om.U, oc.U, op.U, kd.gown);
      part_g(oc.P, o, kd.gown);
      if constexpr (FORCES)
        for (int j = 0; j < 3; j++) kd.Pown[j] = oc.P[j];
    }
    const int ol = grp * HS_LMAX + l;
#pragma unroll
    for (int kk = 0; kk < 3; kk++)
      limb_centre_link<FORCES, false>(mk, outer, ol, l, L, kk, P[kk], U[kk], kd.Jp[kk], kd.Jz[kk], kd.fp, kd.Pc[kk], o, inv, kd.g3[kk], dbg_r);
    if constexpr (LOOP) {
      tr.finish(kd);
      return;
    }
    kd.bad = W.kbad[row0 + 2][L] != 0;
    kd.big |= limb_rows_big(W.ktab[row0][L], W.ktab[row0 + 2][L], W.ktab[row0 + 4][L]);
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      if constexpr (FORCES) break;
      kd.jvel[kk] = wrap_rate(W.ktab[row0 + 3][L][kk], W.ktab[row0 + 1][L][kk], dt);
    }
  }
}

// ---- the packed mapping's K and D phase (a limb lane's: the caller tests limb) ----
// Liveness drives the order (the step's peak registers are here): the outer samples' pos / ust first, then the
// centre link by link, each link's finite differences as soon as its centre values exist
template <bool FORCES>
__device__ __attribute__((always_inline)) inline void limb_packed_kd(
    const hs_topo* T_, real (&outer)[36][LGR * HS_LMAX], hs_link (&links)[HS_LMAX][3], const RolloutWS& W, bool straight,
    const real* u, int l, int L, int ol, int row, const real* tv, const real* o, real inv, real dt, LimbKD& kd, int dbg_r,
    bool stamp_on) {
  (void)stamp_on;  // (HS_STAMPS builds: this step stamps)
  kd.own = T_->limb_own_n[L] > 0;
  // the outer samples (t - 2dt, t + 2dt): the links' pos / ust to LDS (36 reals; held in registers across
  // the centre's FK they pushed the kernel past 256 VGPRs), the chain body's pos / ust kept
  BodyS om, op, oc;
  {
    real P[3][3], U[3][3];
    const hs_topo* Ts = opaque_s(T_);
    limb_outer(Ts, links[L], limb_frame(Ts, L, straight, kd.own, W, W.kf, row, u, tv[0], om), W.ktab[row][L], P, U, kd.big);
    outer_put(outer, 0, ol, P, U);
  }
  STAMP(1);
  // (sched_barrier: the machine scheduler would interleave the independent samples for ILP, holding
  // two samples' FK working sets at once)
  __builtin_amdgcn_sched_barrier(0);
  {
    real P[3][3], U[3][3];
    const hs_topo* Ts = opaque_s(T_);
    limb_outer(Ts, links[L], limb_frame(Ts, L, straight, kd.own, W, W.kf, row + 4, u, tv[4], op), W.ktab[row + 4][L], P, U,
               kd.big);
    outer_put(outer, 18, ol, P, U);
  }
  __builtin_amdgcn_sched_barrier(0);
  STAMP(2);
  {
    const hs_topo* T = opaque_s(T_);
    const A34 J = limb_frame(T, L, straight, kd.own, W, W.kf, row + 2, u, tv[2], oc);
    if (kd.own) {  // the chain body's differences first: its three samples are dead before the links' FK
      part_dyn((real)T->mass[T->limb_own[L][0]], inv, om.P, oc.P, op.P, om.U, oc.U, op.U, kd.gown);
      part_g(oc.P, o, kd.gown);
      if constexpr (FORCES)
        for (int j = 0; j < 3; j++) kd.Pown[j] = oc.P[j];
    }
    const real* ja = W.ktab[row + 2][L];
    real sq[3], cq[3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      kd.big |= sincos_big(ja[kk]);
      sincos_k_small(ja[kk], &sq[kk], &cq[kk]);
    }
    A34 Jv = J, H;
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      real P0[3], U0[3];
      fk_link<true>(T, links[L][kk], kk, Jv, H, sq[kk], cq[kk], P0, U0, kd.Jp[kk], kd.Jz[kk], kd.fp, kd.contact);
      // (its sched_barrier: the link's outer values are read after its FK, not hoisted above it)
      limb_centre_link<FORCES, true>(LimbModelK<false>{T, nullptr}, outer, ol, l, L, kk, P0, U0, kd.Jp[kk], kd.Jz[kk], kd.fp, kd.Pc[kk], o,
                                     inv, kd.g3[kk], dbg_r);
    }
  }
  kd.bad = W.kbad[row + 2][L] != 0;
  // the motors' joint rates at the centre (compute_vel_traj's wrapped difference of q at t +- dt)
#pragma unroll
  for (int kk = 0; kk < 3; kk++) {
    if constexpr (FORCES) break;
    kd.jvel[kk] = wrap_rate(W.ktab[row + 3][L][kk], W.ktab[row + 1][L][kk], dt);
  }
}

// FORCES: hs_run_forces_calls' solve_forces step (contact forces given motor torques, forces_solve's fast
// path: a limb's blocks on its lane, the sums over the limbs in limb order by a DPP chain, the 6 x 6 on
// every lane of the group; a B_f near singular defers the step to the forces fixup launch)
// TILE: the tile mapping (a wavefront = one rollout x eight steps, limb_tile_kd above); else a wavefront =
// eight rollouts x one step
// PLAN: none, or with TILE the launch's tile descriptor (limb_tile_desc, hs_limb_tile.h: the slot sequence with
// every slot's row and every tile's requests), read from the kernel argument segment
//
// The kernel is a head and a step. The head (hs_limb_kernel) forms what belongs to the wavefront's rollouts
// and not to a step -- the model, the rollout and its record, dt, v, the torso's direction -- and copies
// the link records into LDS; limb_step runs one step per group from the table rows on. The packed mapping
// runs the step once; the tile mapping runs it for each tile of the wavefront's chunk in turn (the tile
// loop, launch_map::limb_tile_loop), so the head, all per rollout there and wave-uniform, is paid once per
// chunk and not once per tile. The tile loop's head also stages the wavefront's constants in LDS (LimbLaneK,
// LimbRolloutK above), so that a tile reads them without a round trip to global memory.

// The kernel's LDS. Kinematics: the outer samples' pos / ust of every limb lane's links and the limbs' link
// records (read by every sample's FK: from LDS, not through three rounds of L1/L2 latency per sample); then
// the groups' exchange arrays over them: 17.4 KB per wavefront, 8 per CU at 2 waves / SIMD
template <int NM, bool FORCES, bool LOOP>
struct LimbShared {
  union {
    struct {
      real outer[36][LGR * HS_LMAX];  // [Pm, Um, Pp, Up][link][component][limb lane]: one conflict-free row per value
      hs_link links[HS_LMAX][3];
    } k;
    LimbLds<NM, FORCES> g[LGR];
  };
  __device__ hs_link (&links())[HS_LMAX][3] { return k.links; }
};
// The tile loop keeps the link records beside the overlay, so that a wavefront copies them once for all the
// tiles it runs, and the wavefront constants after them: 17,856 + 2,384 B, under the 20,480 B that leave 8
// one-wavefront workgroups per CU (160 KiB / 8)
template <int NM, bool FORCES>
struct LimbShared<NM, FORCES, true> {
  union {
    struct {
      real outer[36][LGR * HS_LMAX];
    } k;
    LimbLds<NM, FORCES> g[LGR];
  };
  hs_link tl[HS_LMAX][3];
  LimbRolloutK rk;
  LimbLaneK lk[LG];
  __device__ hs_link (&links())[HS_LMAX][3] { return tl; }
};
static_assert(sizeof(LimbShared<HS_NMAX, false, true>) <= 20480, "a looping wavefront's LDS: 8 per CU's 160 KB");

// what hs_limb_kernel's head hands to limb_step: the lane's place, its rollout and the rollout's constants
// (tile mapping: wave-uniform, all but the lane's place)
struct LimbHead {
  int lane;
  int rslot, b;          // the group's rollout of the batch wavefront's eight, and the rollout itself
  bool live;             // the rollout exists (tile mapping: always, its step decides per tile)
  bool straight;
  const RolloutWS* W;
  real u[3];             // the torso's direction of advance
};

// The same pointer to memory this kernel only reads (the model, a rollout's record), wave-uniform, opaque to
// the optimizer: loads through a pointer made opaque once per tile are issued in that tile instead of being
// hoisted out of the tile loop, where their values would stay in registers across every tile. Through a
// constant-address-space pointer: behind the previous tile's stores a global one would turn the uniform
// reads (scalar loads, SGPRs) into vector loads.
template <class P>
__device__ inline const P* opaque_u(const P* p) {
  using cptr = const __attribute__((address_space(4))) P*;
  cptr q = (cptr)p;
  asm volatile("" : "+s"(q));
  return (const P*)q;
}

// a reference into the kernel argument segment, opaque to the optimizer: the fields read through it are
// loaded where they are used (scalar loads)
template <class P>
__device__ inline const P& opaque_k(const P& r) {
  using kptr = const __attribute__((address_space(4))) P*;
  kptr q = (kptr)&r;
  asm volatile("" : "+s"(q));
  return *(const P*)q;
}

// One step per group. fstep: the packed mapping's local step; the tile mapping's tile, whose slot 8 tile + g
// group g runs.
template <int NM, bool FORCES, bool TILE, bool LOOP, class... PLAN>
__device__ __attribute__((always_inline)) inline void limb_step(LimbShared<NM, FORCES, LOOP>& sh, const hs_topo* __restrict__ T,
                                                                const hs_run_args& a0, const hs::launch_map& mp0,
                                                                const LimbHead& h, int fstep, bool stamp_on,
                                                                const PLAN&... plan) {
  (void)stamp_on;  // (HS_STAMPS builds: this step stamps; slot 23 is the step's start, the head's end in the first)
  STAMP(23);
  // (tile loop: the lane's place and the model's counts are formed again in every tile, from a lane index
  // and a model pointer made opaque here. Hoisted out of the tile loop, everything derived from them -- LDS
  // columns, exchange lanes, request masks -- would stay in registers across all of a tile's phases)
  int lane = h.lane;
  if constexpr (LOOP) {
    asm volatile("" : "+v"(lane));
    T = opaque_u(T);
  }
  const int grp = lane >> 3, l = lane & 7, gbase = lane & ~7, rslot = h.rslot, b = h.b;
  const int nl = T->n_limbs, nmj = T->nmj;
  const bool limb = l < nl, tlane = l == LG - 1, straight = h.straight;
  const int L = limb ? l : 0;
  const real u[3] = {h.u[0], h.u[1], h.u[2]};
  bool live = h.live;
  int tile_row = 0;       // tile mapping: the group's row as limb_tile_row forms it,
  uint32_t tile_M = 0;    // the tile's request mask
  uint64_t tile_req = 0;  // and its requests in service order (limb_tile_entry)
  if constexpr (TILE) {
    // group g runs slot 8 tile + g's local step. An idle group (a slot past the sequence, last tile only)
    // takes the tile's first step for its indices, so every address it forms is valid, but it is neither a
    // share target nor a request: its outer rows in LDS are never written, its finite differences and all
    // that follows are computed on whatever the LDS holds (possibly NaN), and nothing of it is stored or
    // counted (every store, atomic and fix item is gated on live)
    // The step and its table row come from the launch's tile descriptor (hs_limb_tile.h), the same for
    // every rollout: one load per lane from the kernel argument segment, no row arithmetic here.
    const limb_tile_entry& te = limb_tile_entry_of(plan..., fstep);
    limb_tile_slot sl;
    int first;
    if constexpr (LOOP) {
      // the tile's eight slots by one scalar load beside M and req, the group's selected from them: a load
      // per lane would be a round trip at the head of every tile, ahead of everything that hangs on the row
      static_assert(sizeof(limb_tile_slot) == 4 && HS_TILE_SLOTS == 8, "a slot is one word: step low, row high");
      uint32_t w[HS_TILE_SLOTS];
      __builtin_memcpy(w, te.slot, sizeof(w));
      uint32_t ws = w[0];
#pragma unroll
      for (int g = 1; g < HS_TILE_SLOTS; g++) ws = grp == g ? w[g] : ws;
      sl.step = (int16_t)(ws & 0xFFFFu);
      sl.row = (int16_t)(ws >> 16);
      first = (int16_t)(w[0] & 0xFFFFu);
    } else {
      sl = te.slot[(unsigned)grp];
      first = te.slot[0].step;
    }
    live = sl.step >= 0;
    fstep = live ? sl.step : first;
    tile_row = sl.row;
    tile_M = te.M;
    tile_req = te.req;
  }
  const RolloutWS* Wp = h.W;
  if constexpr (LOOP) Wp = opaque_u(Wp);
  const RolloutWS& W = *Wp;
  // (read per tile, warm scalar loads: 1 / (2 dt) is a VALU result, two VGPRs across the tile loop if the
  // head formed it)
  const real dt = W.st.dt;
  const real v = W.st.v;
  const real inv = real(1) / (2 * dt);
  LimbLds<NM, FORCES>& S = sh.g[grp];
  const int ol = grp * HS_LMAX + (l < HS_LMAX ? l : 0);  // this limb lane's column of sh.k.outer
  const int s_glob = mp0.fused_s0 + fstep;
  int k0;
  if constexpr (TILE) {
    k0 = tile_row;
  } else {
    const int call = s_glob / mp0.fused_h;
    k0 = (int)(((int64_t)a0.k0 + (int64_t)call * mp0.fused_h) % a0.n_t) + s_glob % mp0.fused_h;
  }
  const int row0 = k0 - mp0.ktab_lo;  // table row of sample i - 2 (centre i = k0 + 2)
  // the model's per-lane constants, the rollout's sample times and straight-gait frames: the tile loop's
  // copies in LDS (the head's), else global memory
  const real* ttab;
  const KinFrames* kfp;
  LimbModelK<LOOP> mk{T, nullptr};
  if constexpr (LOOP) {
    ttab = sh.rk.t_tab;
    kfp = &sh.rk.kf;
    mk.k = sh.lk;
  } else {
    ttab = W.t_tab;
    kfp = &W.kf;
  }
  real tv[5];
#pragma unroll
  for (int k = 0; k < 5; k += 2) tv[k] = ttab[row0 + k] * v;  // gait_record's torso advance
  // the torso COM at the centre sample (particular_sub's origin o = pos(0, 0)), on every lane
  real o[3];
  const real com0[3] = {(real)T->node[0].com[0], (real)T->node[0].com[1], (real)T->node[0].com[2]};  // load_nodek's
  if (straight) {
    for (int i = 0; i < 3; i++) o[i] = fma(tv[2], u[i], W.kf.torso[i]);
  } else {
    mulp(load34r(W.ktor[row0 + 2] + 6), com0, o);
  }
  [[maybe_unused]] const int dbg_r = dbg_row(live, b, a0.horizon, s_glob);

  // the torso's g (node 0; its joint frame J = I * J_A_parent, node_features), on every lane: its loads and
  // arithmetic overlap the limbs' (a torso-lane branch after them would expose its load latency)
  real g0[6];
  {
    BodyS tb[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (straight) tb[k] = body_straight(W.kf.torso, u, tv[2 * k]);
      else tb[k] = body_frame(load34r(W.ktor[row0 + 2 * k] + 6), com0);
    }
    part_dyn((real)T->mass[0], inv, tb[0].P, tb[1].P, tb[2].P, tb[0].U, tb[1].U, tb[2].U, g0);
    part_g(tb[1].P, o, g0);
  }
  STAMP(0);
  // ---- K and D: the limb's links and its chain body (limb lanes), the torso (lane 7) ----
  LimbKD kd;
  if constexpr (TILE) {
    limb_tile_kd<FORCES, LOOP>(T, mk, *kfp, ttab, sh.k.outer, sh.links(), W, straight, u, v, lane, nl, limb, L, live, row0, tile_M,
                               tile_req, tv, o, inv, dt, kd, dbg_r, stamp_on);
  } else if (limb) {
    limb_packed_kd<FORCES>(T, sh.k.outer, sh.k.links, W, straight, u, l, L, ol, row0, tv, o, inv, dt, kd, dbg_r, stamp_on);
  }
  STAMP(3);
  wave_sync();  // S.g overlays sh.k: every lane's outer and link reads first
  if (limb) {
    // g to LDS (the chain bodies' and the root's subtree sums read them)
#pragma unroll
    for (int kk = 0; kk < 3; kk++)
      for (int j = 0; j < 6; j++) S.g[mk.node(L, kk)][j] = kd.g3[kk][j];
    if (kd.own)
      for (int j = 0; j < 6; j++) S.g[mk.own_node(L)][j] = kd.gown[j];
    if constexpr (FORCES) {
#pragma unroll
      for (int kk = 0; kk < 3; kk++)
        for (int j = 0; j < 3; j++) S.p[mk.node(L, kk)][j] = kd.Pc[kk][j];
      if (kd.own)
        for (int j = 0; j < 3; j++) S.p[mk.own_node(L)][j] = kd.Pown[j];
    }
  } else if (tlane) {
    for (int j = 0; j < 6; j++) S.g[0][j] = g0[j];
  }
  wave_sync();

  STAMP(4);
  // ---- S1: subtree sums (particular_sub's stage 2) ----
  // links: their own range in registers (the limb's links are consecutive in preorder, sizes 3, 2, 1); the
  // root on the torso lane: its own g plus each kid's subtree sum (the kid's preorder range, in order),
  // particular_sub's two levels of sums
  real xt[3][3];  // the links' x torque rows
  if (limb) {
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      real F[3] = {0, 0, 0}, V[3] = {0, 0, 0};
#pragma unroll
      for (int m = kk; m < 3; m++)
        for (int j = 0; j < 3; j++) { F[j] += kd.g3[m][j]; V[j] += kd.g3[m][3 + j]; }
      // particular_sub applies stage 3 in a block of its own (after a wavefront barrier): F, V enter it
      // as opaque values
      opaque_vals<3>(F);
      opaque_vals<3>(V);
      real d[3];
      for (int j = 0; j < 3; j++) d[j] = kd.Jp[kk][j] - o[j];
      V[0] -= d[1] * F[2] - d[2] * F[1];
      V[1] -= d[2] * F[0] - d[0] * F[2];
      V[2] -= d[0] * F[1] - d[1] * F[0];
      for (int j = 0; j < 3; j++) xt[kk][j] = V[j];
      opaque_vals<3>(xt[kk]);  // x as the later phases read it (LDS)
      LDBG(dbg_r, T->limb_node[L][kk], V[0], 4);
      LDBG(dbg_r, T->limb_node[L][kk], F[0], 18);
      LDBG(dbg_r, T->limb_node[L][kk], d[0], 17);
    }
  }
  // the root's kids' range sums on lanes 0 .. nk - 1 of the group, in parallel (each range in preorder, as
  // the torso lane would sum it), into the kid's own slot (ranges are disjoint: no lane reads another's)
  {
    const int nk = T->node[0].nkids;
    if (l < nk && l < HS_CMAX) {
      const int c = mk.kid(l), sz = mk.kid_size(l, c);
      real Fk[3] = {0, 0, 0}, Vk[3] = {0, 0, 0};
#pragma unroll
      for (int r = 0; r < 8; r++)
        if (r < sz)
          for (int j = 0; j < 3; j++) { Fk[j] += S.g[c + r][j]; Vk[j] += S.g[c + r][3 + j]; }
      for (int r = 8; r < sz; r++)
        for (int j = 0; j < 3; j++) { Fk[j] += S.g[c + r][j]; Vk[j] += S.g[c + r][3 + j]; }
      for (int j = 0; j < 3; j++) { S.g[c][j] = Fk[j]; S.g[c][3 + j] = Vk[j]; }
    }
  }
  wave_sync();
  if (tlane) {  // x_0 = (F, V - 0 x F): its own g plus the kids' sums, in kid order
    real F[3], V[3];
    for (int j = 0; j < 3; j++) { F[j] = S.g[0][j]; V[j] = S.g[0][3 + j]; }
    const int nk = T->node[0].nkids;
    for (int kk = 0; kk < HS_CMAX; kk++) {
      if (kk >= nk) break;
      const int c = T->node[0].kids[kk];
      for (int j = 0; j < 3; j++) { F[j] += S.g[c][j]; V[j] += S.g[c][3 + j]; }
    }
    const real d[3] = {0, 0, 0};
    V[0] -= d[1] * F[2] - d[2] * F[1];
    V[1] -= d[2] * F[0] - d[0] * F[2];
    V[2] -= d[0] * F[1] - d[1] * F[0];
    for (int j = 0; j < 3; j++) { S.a[j] = F[j]; S.a[3 + j] = V[j]; }
  }
  wave_sync();  // S.a before the Schur system reads it

  STAMP(5);
  // (tile loop: what the phases from here on read of the kernel's arguments -- the output arrays, their
  // strides, the fixup's lists -- is read here, not held in SGPRs across the K and D phase's peak)
  const hs_run_args& a = LOOP ? opaque_k(a0) : a0;
  const hs::launch_map& mp = LOOP ? opaque_k(mp0) : mp0;
  if constexpr (FORCES) {
    limb_forces<NM>(T, a, mp, S, limb, l, L, gbase, nl, live, b, s_glob, o, kd.Jp, kd.Jz, kd.Pc, kd.fp, xt, kd.bad, kd.big);
    return;
  }
  // ---- contact list in foot order (ftsolver's contact columns) ----
  const int fiL = mk.foot(L);
  const uint32_t cm = grp_or((limb && kd.contact) ? 1u << fiL : 0u);
  const int nc = __popc(cm);
  const bool mine = limb && kd.contact;
  if (limb) LDBG(dbg_r, 24 + fiL, kd.fp[2], 25);
  // the limb lane holding contact rank l (lane l < nc of the group gathers that contact's values)
  const int src = rank_limb(T, cm, nl, l) + gbase;
  const bool slot = l < nc;
  // joint values outside sincos_k_small's range: the fixup's
  bool defer = grp_any(kd.big, gbase);
  // a routing decision within kNearBand of its guard: HS_FLAG_NEAR_RANK, as fast_solve sets it (the values
  // are hs_rollout_kernel's bitwise, so the decisions are its own)
  bool nearf = false;
  real y3[3] = {0, 0, 0};
  real d0[3] = {0, 0, 0}, Dinv[9], gc[3], Dp6[6];
  if (mine)
    for (int r = 0; r < 3; r++) d0[r] = o[r] - kd.fp[r];  // A_c = [-I; [d0_c]x]
  if (mine && nc >= 2) contact_block(kd.Jp, kd.Jz, xt, kd.fp, Dp6, gc);
  if (nc >= 3) {
    // zeroth_well_posed: the feet's scatter, in single precision, the contacts' d0 on lanes 0 .. nc - 1
    float e0 = grp_getf(float(o[0] - kd.fp[0]), src), e1 = grp_getf(float(o[1] - kd.fp[1]), src),
          e2 = grp_getf(float(o[2] - kd.fp[2]), src);
    if (!slot) e0 = e1 = e2 = 0.f;
    {
      const float s0 = group8_sum(e0), s1 = group8_sum(e1), s2 = group8_sum(e2);
      const float q00 = group8_sum(e0 * e0), q11 = group8_sum(e1 * e1), q22 = group8_sum(e2 * e2);
      const float q01 = group8_sum(e0 * e1), q02 = group8_sum(e0 * e2), q12 = group8_sum(e1 * e2);
      const float k = float(nc);
      const float c00 = k * q00 - s0 * s0, c11 = k * q11 - s1 * s1, c22 = k * q22 - s2 * s2;
      const float c01 = k * q01 - s0 * s1, c02 = k * q02 - s0 * s2, c12 = k * q12 - s1 * s2;
      const float c2 = (c00 * c11 - c01 * c01) + (c00 * c22 - c02 * c02) + (c11 * c22 - c12 * c12);
      const float tq = q00 + q11 + q22;
      const float md = fmaxf(k, fmaxf(tq - q00, fmaxf(tq - q11, tq - q22)));
      const float t = kZerothGuard * k * (c00 + c11 + c22) * md;
      const bool well = c2 >= t;
      const bool nearz = c2 >= t / float(kNearBand) && c2 <= t * float(kNearBand);
      defer |= !well;  // the same on every lane of the group (group8_sum)
      nearf |= nearz;
    }
    STAMP(6);
    // the contact's Schur block of its first-order block D_c (contact_block)
    real sch[27];
#pragma unroll
    for (int e = 0; e < 27; e++) sch[e] = 0;
    bool lnear = false, ok = true;
    if (mine) {
      const real* Dp = Dp6;
      opaque_vals<3>(d0);
      const real D[9] = {Dp[0], Dp[1], Dp[3], Dp[1], Dp[2], Dp[4], Dp[3], Dp[4], Dp[5]};
      LDBG(dbg_r, 24 + fiL, Dp[0], 6);
      LDBG(dbg_r, 24 + fiL, gc[0], 7);
      real Lm[9];
      for (int i = 0; i < 9; i++) Lm[i] = D[i];
      real rl[3];
      ok = ldl_n<3>(Lm, kFastPivotGuard, rl, lnear);
      if (ok) {
        for (int j = 0; j < 3; j++) {
          real e[3] = {0, 0, 0};
          e[j] = 1;
          ldl_solve_n<3>(Lm, rl, e);
          for (int i = 0; i < 3; i++) Dinv[3 * i + j] = e[i];
        }
        // the block's Schur entries: row r of E = A_c D_c^-1, then (E A_c^T)(r, q) for q <= r, and h_r
#pragma unroll
        for (int r = 0; r < 6; r++) {
          real E[3];
#pragma unroll
          for (int j = 0; j < 3; j++) {
            real acc = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) acc += a_entry(d0, r, i) * Dinv[3 * i + j];
            E[j] = acc;
          }
#pragma unroll
          for (int qq = 0; qq <= r; qq++) {
            real vv = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) vv += E[j] * a_entry(d0, qq, j);
            sch[sch_lower(r, qq)] = vv;
          }
          real hh = 0;
          for (int j = 0; j < 3; j++) hh += E[j] * gc[j];
          sch[SCH_H + r] = hh;
        }
      }
    }
    defer |= grp_any(mine && !ok, gbase);  // a singular D_c: tier 2's
    nearf |= grp_any(mine && lnear, gbase);
    // what fast_solve_lanes stores in FastL and reads back for y (LDS): g_c, d0_c, D_c^-1
    opaque_vals<3>(gc);
    opaque_vals<9>(Dinv);
    // the blocks summed over the contacts by rank
    real Ssum[27];
#pragma unroll
    for (int e = 0; e < 27; e++) {
      real vv = grp_get(sch[e], src);
      Ssum[e] = rank8_sum(slot ? vv : real(0));
    }
    STAMP(7);
    // the 6 x 6 Schur complement system (every lane of the group: the same values)
    real lam[6];
    {
      opaque_vals<27>(Ssum);  // FastL::sc.Ssum
      real Sm[36], rl6[6];
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) Sm[6 * i + j] = (j <= i) ? Ssum[sch_lower(i, j)] : real(0);
      for (int r = 0; r < 6; r++) lam[r] = S.a[r] - Ssum[SCH_H + r];
      bool near6 = false;
      const bool ok6 = ldl_n<6>(Sm, kFastPivotGuard, rl6, near6);
      defer |= !ok6;
      nearf |= near6;
      if (ok6) ldl_solve_n<6>(Sm, rl6, lam);
      opaque_vals<6>(lam);  // FastL::sc.lam
    }
    if (mine) {  // y_c = -D_c^-1 (g_c + A_c^T lam)
      real t[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        real s = gc[i];
#pragma unroll
        for (int r = 0; r < 6; r++) {
          if (r < 3 && r != i) continue;
          if (r >= 3 && r - 3 == i) continue;
          s += a_entry(d0, r, i) * lam[r];
        }
        t[i] = s;
      }
      for (int i = 0; i < 3; i++) {
        real s = 0;
        for (int j = 0; j < 3; j++) s += Dinv[3 * i + j] * t[j];
        y3[i] = -s;
      }
      LDBG(dbg_r, 24 + fiL, y3[0], 8);
      opaque_vals<3>(y3);  // sv.y
    }
  }
  if (nc == 1 || nc == 2) {
    // fast_solve_lanes' one- and two-contact closed forms (its lane 0, from FastL): here on every lane of
    // the group, the contacts' values gathered from their limb lanes
    const int s0 = rank_limb(T, cm, nl, 0) + gbase, s1 = rank_limb(T, cm, nl, 1) + gbase;
    const real a[6] = {S.a[0], S.a[1], S.a[2], S.a[3], S.a[4], S.a[5]};
    bool lnear = false, ok;
    real y[6];
    if (nc == 1) {  // unique least-squares solution (A^T A) w = -A^T a
      real dd[3];
      for (int r = 0; r < 3; r++) dd[r] = grp_get(d0[r], s0);
      real M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0};
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
          for (int r = 0; r < 6; r++) M[3 * i + j] += a_entry(dd, r, i) * a_entry(dd, r, j);
        for (int r = 0; r < 6; r++) bv[i] -= a_entry(dd, r, i) * a[r];
      }
      real rl[3];
      if (mine) LDBG(dbg_r, 24 + fiL, M[4], 19);
      if (mine) LDBG(dbg_r, 24 + fiL, bv[1], 20);
      ok = chol_n<3>(M, kFastPivotGuard, rl, lnear);
      if (ok) chol_solve_n<3>(M, rl, bv);
      for (int i = 0; i < 3; i++) y[i] = bv[i];
      if (mine && ok) LDBG(dbg_r, 24 + fiL, bv[0], 21);
    } else {  // rank 5: kernel n = (u,-u)/sqrt2 along the line between the feet
      real f0[3], f1[3], dA[2][3], Dc[2][6], gg[2][3];
      for (int r = 0; r < 3; r++) {
        f0[r] = grp_get(kd.fp[r], s0);
        f1[r] = grp_get(kd.fp[r], s1);
        dA[0][r] = grp_get(d0[r], s0);
        dA[1][r] = grp_get(d0[r], s1);
        gg[0][r] = grp_get(gc[r], s0);
        gg[1][r] = grp_get(gc[r], s1);
      }
      for (int e = 0; e < 6; e++) {
        Dc[0][e] = grp_get(Dp6[e], s0);
        Dc[1][e] = grp_get(Dp6[e], s1);
      }
      const real Dm[2][9] = {{Dc[0][0], Dc[0][1], Dc[0][3], Dc[0][1], Dc[0][2], Dc[0][4], Dc[0][3], Dc[0][4], Dc[0][5]},
                             {Dc[1][0], Dc[1][1], Dc[1][3], Dc[1][1], Dc[1][2], Dc[1][4], Dc[1][3], Dc[1][4], Dc[1][5]}};
      real u[3], un = 0;
      for (int r = 0; r < 3; r++) { u[r] = f0[r] - f1[r]; un += u[r] * u[r]; }
      un = sqrt(un);
      ok = un > real(1e-12);
      real nv[6], M[36], bv[6], rl[6];
      if (ok) {
        for (int r = 0; r < 3; r++) { nv[r] = u[r] / un / sqrt(real(2)); nv[3 + r] = -nv[r]; }
        const bool first = mine && __popc(cm & ((1u << fiL) - 1)) == 0;
        if (first) LDBG(dbg_r, 24 + fiL, nv[2], 26);
        for (int i = 0; i < 6; i++) {
          const real* di = dA[i / 3];
          for (int j = 0; j < 6; j++) {
            const real* dj = dA[j / 3];
            real sv = 0;
            for (int r = 0; r < 6; r++) sv += a_entry(di, r, i % 3) * a_entry(dj, r, j % 3);
            M[6 * i + j] = sv + nv[i] * nv[j];
          }
          real sv = 0;
          for (int r = 0; r < 6; r++) sv += a_entry(di, r, i % 3) * a[r];
          bv[i] = -sv;
        }
        if (first) LDBG(dbg_r, 24 + fiL, M[5], 27);
        opaque_vals<36>(M);  // as hs_rollout_kernel's fast_solve_lanes fences them
        opaque_vals<6>(bv);
        opaque_vals<6>(nv);
        ok = chol_n<6>(M, kFastPivotGuard, rl, lnear);
      }
      if (ok) {
        chol_solve_n<6>(M, rl, bv);
        opaque_vals<6>(bv);
        real nDn = 0, nr = 0;
        for (int c = 0; c < 2; c++)
          for (int i = 0; i < 3; i++) {
            real Dw = 0, Dn = 0;
            for (int j = 0; j < 3; j++) { Dw += Dm[c][3 * i + j] * bv[3 * c + j]; Dn += Dm[c][3 * i + j] * nv[3 * c + j]; }
            nr += nv[3 * c + i] * (Dw + gg[c][i]);
            nDn += nv[3 * c + i] * Dn;
          }
        ok = nDn > 0;
        if (ok) {
          real t = -nr / nDn;
          for (int i = 0; i < 6; i++) y[i] = bv[i] + t * nv[i];
          if (mine && __popc(cm & ((1u << fiL) - 1)) == 0) {
            LDBG(dbg_r, 24 + fiL, y[0], 22);
            LDBG(dbg_r, 24 + fiL, bv[0], 23);
            LDBG(dbg_r, 24 + fiL, t, 24);
          }
        }
      }
    }
    defer |= !ok;  // the same on every lane of the group
    nearf |= lnear;
    if (mine && ok) {
      const int rk = __popc(cm & ((1u << fiL) - 1));
      for (int i = 0; i < 3; i++) y3[i] = rk == 0 ? y[i] : y[3 + i];
      opaque_vals<3>(y3);  // sv.y
    }
  }
  STAMP(8);
  if (defer) {
    limb_defer(mp, live, l, s_glob, mp.limb_slots ? mp.limb_slots[rslot] : b);
    return;
  }

  // ---- S4: motor torques, contact forces, work (step()'s outputs) ----
  const size_t orow = (size_t)b * a.horizon + s_glob;
  bool nan = false;
  if (limb) {
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      const int hh = mk.hinge(L, kk);
      real d[3], yy[3];
#pragma unroll
      for (int rr = 0; rr < 3; rr++) {
        d[rr] = kd.Jp[kk][rr] - kd.fp[rr];
        yy[rr] = mine ? y3[rr] : real(0);
      }
      real tq = real(0);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        real s = real(0);
#pragma unroll
        for (int jj = 0; jj < 3; jj++)
          if (jj != r) s = s + cross_e(d, jj, r) * yy[jj];
        real xr = xt[kk][r] + s;
        tq = tq + kd.Jz[kk][r] * xr;
      }
      real dw = tq * kd.jvel[kk];
      S.wd[hh] = (dw > 0) ? dw : 0;
      nan |= tq != tq;
      if (live && a.tau) outp(a.tau)[orow * mp.st_tau + hh] = tq;
    }
    if (mine)
      for (int j = 0; j < 3; j++) nan |= y3[j] != y3[j];
    if (live && a.cf)
      for (int j = 0; j < 3; j++) {
        real zv = -real(0);
        if (mine) zv = -(real(0) + (real(-1)) * y3[j]);
        outp(a.cf)[orow * mp.st_cf + 3 * fiL + j] = zv;
      }
  }
  // a mixed plan's rows past this model's joints and feet (hs_rollout_kernel writes them 0; a single model's
  // rows have none: the loops' code is kept off its path, ~1 % at K = 200, r06_t17)
  if (live && mp.limb_rollouts) {
    if (a.tau)
      for (int c = nmj + l; c < mp.st_tau; c += LG) outp(a.tau)[orow * mp.st_tau + c] = real(0);
    if (a.cf)
      for (int c = 3 * T->nf + l; c < mp.st_cf; c += LG) outp(a.cf)[orow * mp.st_cf + c] = real(0);
  }
  const bool any_nan = grp_any(nan, gbase), any_bad = grp_any(limb && kd.bad, gbase);
  wave_sync();
  if (l == 0 && live) {
    uint32_t flags = 0;
    if (nc == 0) flags |= HS_FLAG_NO_CONTACT;
    if (nc == 1) flags |= HS_FLAG_FULL_RANK;
    if (nearf) flags |= HS_FLAG_NEAR_RANK;
    if (any_nan) flags |= HS_FLAG_NAN;
    if (any_bad) flags |= HS_FLAG_UNREACH;
    if (a.flags) a.flags[orow] = flags;
    // the joints' positive work in joint order (work_over_period's loop, periodic.cpp:294-300), summed over
    // the steps in order by the reduce
    real work_dt = real(0);
    for (int jj = 0; jj < nmj; jj++) work_dt += S.wd[jj];
    reinterpret_cast<real*>(mp.fused_work)[(size_t)s_glob * a.n_rollouts + b] = work_dt;
  }
  STAMP(9);
  RSTAMP(17);
}
#ifdef HS_STAMPS
#undef HS_STAMP_GATE
#define HS_STAMP_GATE true
#endif

// hs_limb_kernel's arguments of the tile mapping as the kernel argument segment holds them: in order, each
// at its type's alignment (the code object's metadata lists the same offsets: 0, 8, 136, 144, 424)
struct LimbTileArgs {
  const hs_topo* T0;
  hs_run_args a;
  RolloutWS* rws;
  hs::launch_map mp;
  limb_tile_desc plan;
};

template <int NM, bool FORCES, bool TILE = false, class... PLAN>
__global__ __launch_bounds__(WAVE, HS_REAL_IS_FLOAT ? HS_LIMB_WAVES_F32 : HS_LIMB_WAVES) void hs_limb_kernel(const hs_topo* __restrict__ T0, hs_run_args a,
                                                                      RolloutWS* __restrict__ rws, hs::launch_map mp, PLAN... plan) {
  static_assert(sizeof...(PLAN) == (TILE ? 1 : 0), "the tile mapping takes the launch's tile descriptor, the packed mapping nothing");
  // (LimbTileArgs above restates this parameter list for the tile loop: change both together)
  static_assert(!TILE || (std::is_same<PLAN, limb_tile_desc>::value && ...), "LimbTileArgs holds a limb_tile_desc");
  static_assert(offsetof(LimbTileArgs, a) == 8 && offsetof(LimbTileArgs, rws) == 8 + sizeof(hs_run_args) &&
                    offsetof(LimbTileArgs, mp) == 16 + sizeof(hs_run_args) &&
                    offsetof(LimbTileArgs, plan) == 16 + sizeof(hs_run_args) + sizeof(hs::launch_map) &&
                    alignof(hs_run_args) == 8 && alignof(hs::launch_map) == 8,
                "LimbTileArgs: the kernel argument segment packs the arguments in order at their alignment");
  // The tile loop is the step mode's. Forces mode runs a tile per wavefront: with the loop around it its
  // instantiations spill (12 to 36 bytes of scratch at 256 VGPRs, the peak is forces_solve's blocks), and
  // launch_limb gives its launches one tile per wavefront
  // The fp32 build (reached through HS_LIMB_TILE_MIN only) keeps a tile per wavefront too: its loop was
  // neither measured nor tested.
  constexpr bool LOOP = TILE && !FORCES && !HS_REAL_IS_FLOAT;
  __shared__ LimbShared<NM, FORCES, LOOP> sh;
  int fstep = 0, q = (int)blockIdx.x;
  // tile mapping: the block's virtual step is (chunk of tiles, rollout of the batch wavefront's eight)
  const int nt = TILE ? limb_tile_count(mp.fused_n) : 0, tl = LOOP ? mp.limb_tile_loop : 1;
  fused_coords((int)blockIdx.x, mp.fused_w, TILE ? HS_TILE_SLOTS * limb_tile_chunks(nt, tl) : mp.fused_n, fstep, q);
  const hs_topo* __restrict__ T = mp.limb_model ? T0 + mp.limb_model[q] : T0;  // a mixed plan's wavefront model
  STAMP(18);
  {  // the link records, 8 bytes per lane and load
    const uint64_t* src = reinterpret_cast<const uint64_t*>(&T->link[0][0]);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&sh.links()[0][0]);
    constexpr int NW = sizeof(hs_link[HS_LMAX][3]) / sizeof(uint64_t);
    for (int e = (int)threadIdx.x; e < NW; e += WAVE) dst[e] = src[e];
    if constexpr (LOOP) {
      // the model's per-lane constants, formed by the group's first lanes: entry l is limb l's and the root's
      // kid l's (LimbLaneK). Two dependent loads deep, once per wavefront instead of once per tile.
      const int l = (int)threadIdx.x;
      if (l < LG) {
        LimbLaneK e;
        e.m[0] = e.m[1] = e.m[2] = e.mown = real(0);
        e.nodes = e.hf = e.kid = e.pad_ = 0;
        if (l < T->n_limbs) {
          const bool own = T->limb_own_n[l] > 0;
          const int on = own ? T->limb_own[l][0] : 0;
#pragma unroll
          for (int kk = 0; kk < 3; kk++) {
            const int v = T->limb_node[l][kk];
            e.m[kk] = (real)T->mass[v];
            e.nodes |= (uint32_t)v << (8 * kk);
            e.hf |= (uint32_t)T->link[l][kk].hinge << (8 * kk);
          }
          if (own) e.mown = (real)T->mass[on];
          e.nodes |= (uint32_t)on << 24;
          e.hf |= (uint32_t)T->link[l][2].foot << 24;
          e.kid = (uint32_t)own << 16;
        }
        if (l < T->node[0].nkids && l < HS_CMAX) {
          const int c = T->node[0].kids[l];
          e.kid |= (uint32_t)c | (uint32_t)T->node[c].size << 8;
        }
        sh.lk[l] = e;
      }
    } else {
      wave_sync();
    }
  }
  RSTAMP(16);
  STAMP(15);
  LimbHead h;
  h.lane = (int)threadIdx.x;
  h.rslot = q * LGR + (TILE ? fstep % LGR : h.lane >> 3);
  h.b = mp.limb_rollouts ? mp.limb_rollouts[h.rslot] : h.rslot;
  h.live = h.b >= 0 && h.b < a.n_rollouts;
  if (TILE && !h.live) return;  // the whole wavefront: one rollout
  // an idle group computes a copy of a rollout of its wavefront's model and stores nothing
  const int bb = h.live ? h.b : (mp.limb_rollouts ? mp.limb_rollouts[q * LGR] : a.n_rollouts - 1);
  h.W = &rws[bb];
  const hs_gait_params& gp = a.params[bb];
  h.straight = (real)gp.curvature == 0 && !gp.rec_transform_flag;
  {
    const NodeK n0 = load_nodek(T, 0);
    for (int i = 0; i < 3; i++) h.u[i] = n0.Jp(i, 0);
  }
  if constexpr (LOOP) {
    {  // the rollout's sample times and straight-gait frames (LimbRolloutK), 8 bytes per lane and load
      const real* src = h.W->t_tab;
      real* dst = sh.rk.t_tab;
      constexpr int NR = sizeof(LimbRolloutK) / sizeof(real);
      for (int e = (int)threadIdx.x; e < NR; e += WAVE) dst[e] = src[e];
      wave_sync();  // with the link records and the lane constants above
    }
    // the chunk's tiles in order. Between two tiles every lane meets again, whichever way it left the step
    // (a deferred step ends its group's tile, not the wavefront), and the tile's last LDS reads (S.wd, S.a)
    // come before the next tile's outer rows are written over them
    // Each tile reads the kernel's arguments again, from the kernel argument segment through a pointer made
    // opaque in the tile (scalar loads, warm after the first tile): read once at the kernel's entry they
    // would all stay in SGPRs across the loop, ~70 on top of the head's, and spill.
    const int c = fstep / LGR;
    for (int t0 = limb_tile_chunk_first(c, tl), t = t0, te = limb_tile_chunk_end(c, tl, nt); t < te; t++) {
      using kptr = const __attribute__((address_space(4))) LimbTileArgs*;
      kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ka));
      const LimbTileArgs& k = *(const LimbTileArgs*)ka;
#ifdef HS_STAMPS
      const bool stamp_on = t - t0 == g_stamp_iter;
#else
      const bool stamp_on = true;
#endif
      limb_step<NM, FORCES, true, true>(sh, T, k.a, k.mp, h, t, stamp_on, k.plan);
      wave_sync();
    }
  } else {
    limb_step<NM, FORCES, TILE, false>(sh, T, a, mp, h, TILE ? fstep / LGR : fstep, true, plan...);
  }
}

}  // namespace

namespace hs {

static int limb_deferred(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_limb_deferred), sizeof(unsigned long long), 0,
                                  hipMemcpyDeviceToHost);
}

static int launch_limb(const hs_topo* d_topo, const hs_run_args& a, void* workspace, const launch_map& mp,
                       int32_t tile_plan, int32_t* tile_planned) {
  if (tile_planned) *tile_planned = 0;
  if (a.n_rollouts <= 0 || mp.fused_n <= 0) return 0;
  hipStream_t st = (hipStream_t)a.stream;
  RolloutWS* ws = (RolloutWS*)workspace;
  launch_map m = mp;
  m.fused_w = mp.limb_rollouts ? mp.limb_waves : (a.n_rollouts + LGR - 1) / LGR;  // wavefronts per step: 8 rollouts each
  // the tile loop: a wavefront per chunk of limb_tile_loop tiles
  // (forces mode and the fp32 build: a tile per wavefront, their instantiations have no tile loop)
  m.limb_tile_loop = mp.limb_tile_loop < 1 || mp.tau_in || HS_REAL_IS_FLOAT ? 1 : mp.limb_tile_loop;
  const int wsteps = mp.limb_tile ? HS_TILE_SLOTS * limb_tile_chunks(limb_tile_count(mp.fused_n), m.limb_tile_loop) : mp.fused_n;
  const dim3 grid((unsigned)((int64_t)m.fused_w * wsteps));
  // the tile mapping's slot sequence as the kernel's tile descriptor (hs_limb_tile.h: limb_tile_desc_build, which
  // reads tile_plan). (A launch no descriptor holds is routed to the packed mapping by limb_tile() in hs_capi.cpp.)
  limb_tile_desc plan = {};
  if (mp.limb_tile) {
    const limb_tile_launch L = {mp.fused_n, mp.fused_s0, mp.fused_h, a.k0, a.n_t, mp.ktab_nl > 0 ? mp.ktab_nl : HS_LMAX};
    bool planned = false;
    if (!limb_tile_desc_build(L, tile_plan, plan, &planned)) return (int)hipErrorInvalidValue;
    if (tile_planned) *tile_planned = planned;
  }
  with_lds_class(mp.max_parts, [&](auto nm) {
    constexpr int NM = decltype(nm)::value;
    if (mp.tau_in) {  // solve_forces (hs_run_forces_calls)
      if (mp.limb_tile)
        hipLaunchKernelGGL((hs_limb_kernel<NM, true, true, limb_tile_desc>), grid, dim3(WAVE), 0, st, d_topo, a, ws, m, plan);
      else
        hipLaunchKernelGGL((hs_limb_kernel<NM, true, false>), grid, dim3(WAVE), 0, st, d_topo, a, ws, m);
    } else {
      if (mp.limb_tile)
        hipLaunchKernelGGL((hs_limb_kernel<NM, false, true, limb_tile_desc>), grid, dim3(WAVE), 0, st, d_topo, a, ws, m, plan);
      else
        hipLaunchKernelGGL((hs_limb_kernel<NM, false, false>), grid, dim3(WAVE), 0, st, d_topo, a, ws, m);
    }
  });
  return (int)hipGetLastError();
}

}  // namespace hs
