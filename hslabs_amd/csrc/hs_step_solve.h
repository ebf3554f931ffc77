// hs_step_solve.h -- the solves of a control step, shared by both step kernels: the Eigen-style general path
// (S2 / S3 general), the closed form of the same lexicographic least squares (S3 fast path) with its
// factorisations and DPP sums, the work and best-key arithmetic of the outputs (S4) and the work reduce,
// and the forces-given-torques solve (forcetorquesolver::solve_forces).
#pragma once
#include "hs_step_base.h"

namespace {

// Tree-basis null-space entry for a torque row: (arm x e_jj)[row], arm = ref - fpos
template <class T>
__device__ inline T cross_e(const T* d, int jj, int row) {
  // d x e0 = (0, d2, -d1); d x e1 = (-d2, 0, d0); d x e2 = (d1, -d0, 0)
  if (jj == 0) return row == 0 ? T(0) : (row == 1 ? d[2] : -d[1]);
  if (jj == 1) return row == 0 ? -d[2] : (row == 1 ? T(0) : d[0]);
  return row == 0 ? d[1] : (row == 1 ? -d[0] : T(0));
}

// ===========================================================================
// General path (rare: the fast solve's guard tripped): Gram matrices of the
// tree-built null basis and the Eigen 3.3 FullPivLU / ColPivHouseholderQR rank
// loop of ftsolver.cpp:185-303 (oracle/hs_oracle.cpp tree mode, same
// operation order). G is the LDS or the global workspace (GenMats).
// ===========================================================================

// S2: Gram matrices of the masked, penalty-weighted null basis (ftsolver.cpp:185-207)
template <class W, class SV, class G>
__device__ void build_grams(const hs_topo* T, const SV& sv, G& g, const W& w, int k, int lane) {
  constexpr int LD = G::LD;
  const int n = T->n;
  const int nc = k / 3;
  const real* P0 = w.pos(0, 0);
  // switch_torso_penalty (ftsolver.cpp:262-273): the torso rows of mask0 (bit 0: force rows, bit 1:
  // torque rows; the reference's (1,1) is 3). Rows outside mask0 belong to mask1 with weight 1, ahead
  // of the joint torque rows in row order (set_penal_mask1, ftsolver.cpp:291-303)
  const int tm = T->torso_mask;
  const bool t_force0 = (tm & 1) != 0, t_torque0 = (tm & 2) != 0;
  // zeroth order: rows {0,1,2} = -I, rows {3n..3n+2} = (pos_0 - fpos) x e_jj, weight 1
  for (int e = lane; e < k * k; e += HALF) {
    int ci = e % k, cj = e / k;
    const real* fa = w.fpos(0, sv.cfoot[ci / 3]);
    const real* fb = w.fpos(0, sv.cfoot[cj / 3]);
    int ja = ci % 3, jb = cj % 3;
    greal da[3], db[3];
    for (int r = 0; r < 3; r++) { da[r] = P0[r] - fa[r]; db[r] = P0[r] - fb[r]; }
    greal s = greal(0);
    if (t_force0)
      for (int r = 0; r < 3; r++) {
        greal na = (r == ja) ? greal(-1) : greal(0), nb = (r == jb) ? greal(-1) : greal(0);
        s = s + na * nb;
      }
    if (t_torque0)
      for (int r = 0; r < 3; r++) s = s + cross_e(da, ja, r) * cross_e(db, jb, r);
    g.ntn0[ci + cj * LD] = s;
  }
  if (lane < k) {
    int ci = lane, ja = ci % 3;
    const real* fa = w.fpos(0, sv.cfoot[ci / 3]);
    greal da[3];
    for (int r = 0; r < 3; r++) da[r] = P0[r] - fa[r];
    greal s = greal(0);
    if (t_force0)
      for (int r = 0; r < 3; r++) s = s + ((r == ja) ? greal(-1) : greal(0)) * (greal(1) * sv.x[r]);
    if (t_torque0)
      for (int r = 0; r < 3; r++) s = s + cross_e(da, ja, r) * (greal(1) * sv.x[3 * n + r]);
    g.ntx0[ci] = s;
    // the first-order torso rows (one group at most: mask0 is never empty), for the coupling terms
    for (int r = 0; r < 3; r++)
      g.u1[r][ci] = !t_force0 ? ((r == ja) ? greal(-1) : greal(0)) : (!t_torque0 ? cross_e(da, ja, r) : greal(0));
  }
  if (lane == 0) g.coupled = tm != 3;
  // first order: torque rows of the non-root ancestors of each contact foot,
  // weighted by the joint-axis components (set_action_penalties, ftsolver.cpp:239-246),
  // after the torso rows mask0 leaves out
  for (int e = lane; e < nc * 9 + k; e += HALF) {
    bool is_vec = e >= nc * 9;
    int cc = is_vec ? (e - nc * 9) / 3 : e / 9;
    int a_col = is_vec ? (e - nc * 9) % 3 : (e % 9) % 3;
    int b_col = is_vec ? 0 : (e % 9) / 3;
    int foot = T->footis[sv.cfoot[cc]];
    const real* fp = w.fpos(0, sv.cfoot[cc]);
    // ancestors of foot below the root, in ascending part order (top of the chain first)
    int chain[HS_NMAX], len = 0;
    for (int a = foot; a >= 0 && T->node[a].parent >= 0; a = T->node[a].parent) chain[len++] = a;
    greal s = greal(0);
    if (!t_force0)  // torso force rows 0..2: N = -I per contact, x1 = x
      for (int r = 0; r < 3; r++) {
        greal na = (r == a_col) ? greal(-1) : greal(0);
        greal nb = is_vec ? greal(1) * sv.x[r] : ((r == b_col) ? greal(-1) : greal(0));
        s = s + na * nb;
      }
    if (!t_torque0) {  // torso torque rows 3n..3n+2: N = [pos_0 - fpos]x
      greal d0[3];
      for (int r = 0; r < 3; r++) d0[r] = P0[r] - fp[r];
      for (int r = 0; r < 3; r++) {
        greal na = cross_e(d0, a_col, r);
        greal nb = is_vec ? greal(1) * sv.x[3 * n + r] : cross_e(d0, b_col, r);
        s = s + na * nb;
      }
    }
    for (int t = len - 1; t >= 0; t--) {
      int a = chain[t];
      const real* Ja = w.jpos(0, a);
      const real* Za = w.jz(0, a);
      greal d[3];
      for (int r = 0; r < 3; r++) d[r] = Ja[r] - fp[r];
      for (int r = 0; r < 3; r++) {
        greal wz = Za[r];
        greal na = wz * cross_e(d, a_col, r);
        greal nb = is_vec ? wz * sv.x[3 * n + 3 * a + r] : wz * cross_e(d, b_col, r);
        s = s + na * nb;
      }
    }
    if (is_vec) g.ntx1[3 * cc + a_col] = s;
    else g.n1[cc][b_col * 3 + a_col] = s;
  }
  gsync<G>();
}

// first-order Gram entry (block diagonal)
template <class G>
__device__ inline greal ntn1_at(const G& g, int i, int j) {
  return (i / 3 == j / 3) ? g.n1[i / 3][(j % 3) * 3 + (i % 3)] : greal(0);
}
// with torso rows in the first order (g.coupled): the off-block entries are their products, summed
// in row order (the blocks already start with them)
template <class G>
__device__ inline greal ntn1_full(const G& g, int i, int j) {
  if (i / 3 == j / 3) return g.n1[i / 3][(j % 3) * 3 + (i % 3)];
  greal s = greal(0);
  for (int r = 0; r < 3; r++) s = s + g.u1[r][i] * g.u1[r][j];
  return s;
}

// half-wave argmax with first-index tie break
__device__ inline void wave_argmax(greal& v, int& idx) {
  for (int off = HALF / 2; off >= 1; off >>= 1) {
    greal ov = __shfl_xor(v, off);
    int oi = __shfl_xor(idx, off);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
}

struct LUInfo {
  int nz;          // nonzero pivots
  greal maxpivot;
};

// Eigen FullPivLU::computeInPlace of ntn0 into g.lu (k x k)
template <class G>
__device__ LUInfo fullpiv_lu(G& g, int k, int lane) {
  constexpr int LD = G::LD;
  for (int e = lane; e < k * k; e += HALF) {
    int i = e % k, j = e / k;
    g.lu[i + j * LD] = g.ntn0[i + j * LD];
  }
  gsync<G>();
  LUInfo info{k, greal(0)};
  for (int p = 0; p < k; p++) {
    const int m = k - p;
    greal best = greal(-1);
    int bidx = 1 << 30;
    for (int e = lane; e < m * m; e += HALF) {
      greal a = fabs(g.lu[(p + e % m) + (p + e / m) * LD]);
      if (a > best || (a == best && e < bidx)) { best = a; bidx = e; }
    }
    wave_argmax(best, bidx);
    if (best == 0) {
      info.nz = p;
      for (int i = p + lane; i < k; i += HALF) { g.rowsT[i] = i; g.colsT[i] = i; }
      break;
    }
    if (best > info.maxpivot) info.maxpivot = best;
    const int bi = p + bidx % m, bj = p + bidx / m;
    if (lane == 0) { g.rowsT[p] = bi; g.colsT[p] = bj; }
    if (bi != p && lane < k) {
      greal t = g.lu[p + lane * LD];
      g.lu[p + lane * LD] = g.lu[bi + lane * LD];
      g.lu[bi + lane * LD] = t;
    }
    gsync<G>();
    if (bj != p && lane < k) {
      greal t = g.lu[lane + p * LD];
      g.lu[lane + p * LD] = g.lu[lane + bj * LD];
      g.lu[lane + bj * LD] = t;
    }
    gsync<G>();
    if (p < k - 1) {
      greal piv = g.lu[p + p * LD];
      if (lane > p && lane < k) g.lu[lane + p * LD] /= piv;
      gsync<G>();
      const int mm = k - p - 1;
      for (int e = lane; e < mm * mm; e += HALF) {
        int i = p + 1 + e % mm, j = p + 1 + e / mm;
        g.lu[i + j * LD] -= g.lu[i + p * LD] * g.lu[p + j * LD];
      }
      gsync<G>();
    }
  }
  if (lane == 0) {
    for (int i = 0; i < k; i++) g.q[i] = i;
    for (int p = 0; p < k; p++) { int t = g.q[p]; g.q[p] = g.q[g.colsT[p]]; g.q[g.colsT[p]] = t; }
  }
  gsync<G>();
  return info;
}

// any nonzero pivot within kNearBand of the rank threshold maxpivot * thr (the decisions lu_rank takes)
template <class G>
__device__ inline bool lu_near(const G& g, const LUInfo& info, greal thr) {
  constexpr int LD = G::LD;
  const greal pt = fabs(info.maxpivot) * thr;
  bool nr = false;
  for (int i = 0; i < info.nz; i++) nr |= near_thr(fabs(g.lu[i + i * LD]), pt, greal(kNearBand));
  return nr;
}

template <class G>
__device__ inline int lu_rank(const G& g, const LUInfo& info, greal thr) {
  constexpr int LD = G::LD;
  greal pt = fabs(info.maxpivot) * thr;
  int r = 0;
  for (int i = 0; i < info.nz; i++) r += fabs(g.lu[i + i * LD]) > pt;
  return r;
}

// column-oriented upper-triangular solve of vec[0..r) against U (ld LD), all lanes
template <class G>
__device__ void upper_solve_shared(const greal* U, greal* vec, int r, int lane) {
  constexpr int LD = G::LD;
  for (int i = r - 1; i >= 0; i--) {
    greal ci = vec[i];
    if (ci != 0) {
      greal xi = ci / U[i + i * LD];
      if (lane < i) vec[lane] -= xi * U[lane + i * LD];
      if (lane == i) vec[i] = xi;
    }
    gsync<G>();
  }
}

// FullPivLU::solve(-ntx0) -> g.y0
template <class G>
__device__ void lu_solve(G& g, const LUInfo& info, int k, int r, int lane) {
  constexpr int LD = G::LD;
  if (lane == 0) {
    for (int i = 0; i < k; i++) g.c[i] = -g.ntx0[i];
    for (int p = 0; p < k; p++) { greal t = g.c[p]; g.c[p] = g.c[g.rowsT[p]]; g.c[g.rowsT[p]] = t; }
  }
  if (lane < k) g.y0[lane] = greal(0);
  gsync<G>();
  if (r == 0) return;
  for (int j = 0; j < k; j++) {  // unit lower
    greal cj = g.c[j];
    if (lane > j && lane < k) g.c[lane] -= cj * g.lu[lane + j * LD];
    gsync<G>();
  }
  upper_solve_shared<G>(g.lu, g.c, r, lane);
  if (lane < r) g.y0[g.q[lane]] = g.c[lane];
  gsync<G>();
}

// FullPivLU::kernel() -> g.Ny (k x dimker); uses g.qr as scratch; g.piv/rycol set
template <class G>
__device__ void lu_kernel_image(G& g, const LUInfo& info, int k, int r, greal thr, int lane) {
  constexpr int LD = G::LD;
  if (lane == 0) {
    greal pt = info.maxpivot * thr;
    int p = 0;
    for (int i = 0; i < info.nz; i++)
      if (fabs(g.lu[i + i * LD]) > pt) g.piv[p++] = i;
    for (int i = 0; i < r; i++) g.rycol[i] = g.q[g.piv[i]];  // image columns
  }
  gsync<G>();
  const int dimker = k - r;
  if (dimker == 0) return;
  greal* mm = g.qr;  // r x k trapezoid
  for (int e = lane; e < r * k; e += HALF) {
    int i = e % r, j = e / r;
    mm[i + j * LD] = (j >= i) ? g.lu[g.piv[i] + j * LD] : greal(0);
  }
  gsync<G>();
  if (lane < r) {  // bring non-negligible pivots to the front (rows own a column swap each)
    for (int i = 0; i < r; i++) {
      int pc = g.piv[i];
      if (pc != i) { greal t = mm[lane + i * LD]; mm[lane + i * LD] = mm[lane + pc * LD]; mm[lane + pc * LD] = t; }
    }
  }
  gsync<G>();
  if (lane < dimker) {  // solve U11 X = U12, one right-hand column per lane
    greal* col = &mm[(r + lane) * LD];
    for (int i = r - 1; i >= 0; i--) {
      if (col[i] != 0) {
        col[i] /= mm[i + i * LD];
        for (int rr = 0; rr < i; rr++) col[rr] -= col[i] * mm[rr + i * LD];
      }
    }
  }
  gsync<G>();
  if (lane < r) {
    for (int i = r - 1; i >= 0; i--) {
      int pc = g.piv[i];
      if (pc != i) { greal t = mm[lane + i * LD]; mm[lane + i * LD] = mm[lane + pc * LD]; mm[lane + pc * LD] = t; }
    }
  }
  gsync<G>();
  for (int e = lane; e < k * dimker; e += HALF) {
    int i = e % k, kk = e / k;
    int row = g.q[i];
    greal v;
    if (i < r) v = -mm[i + (r + kk) * LD];
    else v = (i == r + kk) ? greal(1) : greal(0);
    g.Ny[row + kk * LD] = v;
  }
  gsync<G>();
}

// entry (i, j) of m = [ntn1 Ny, ntn0 Ry] (ftsolver.cpp:222-226), evaluated where needed
template <class G>
__device__ inline greal m_at(const G& g, int k, int dimker, int i, int j) {
  constexpr int LD = G::LD;
  greal s = greal(0);
  if (j < dimker) {
    if (g.coupled) {
      for (int kk = 0; kk < k; kk++) s = s + ntn1_full(g, i, kk) * g.Ny[kk + j * LD];
    } else {
      int b0 = (i / 3) * 3;
      for (int kk = b0; kk < b0 + 3; kk++) s = s + ntn1_at(g, i, kk) * g.Ny[kk + j * LD];
    }
  } else {
    int col = g.rycol[j - dimker];
    for (int kk = 0; kk < k; kk++) s = s + g.ntn0[i + kk * LD] * g.ntn0[kk + col * LD];
  }
  return s;
}

// Eigen 3.3 ColPivHouseholderQR on g.qr (k x k, holding m); returns nonzero pivots
// near: a nonzero-pivot decision (Eigen's |col|^2 < threshold_helper (k - p)) within kNearBand^2
template <class G>
__device__ int colpiv_qr(G& g, int k, int lane, bool& near) {
  constexpr int LD = G::LD;
  if (lane < k) {
    greal s = 0;
    for (int i = 0; i < k; i++) s += g.qr[i + lane * LD] * g.qr[i + lane * LD];
    g.nd[lane] = sqrt(s);
    g.nu[lane] = g.nd[lane];
  }
  gsync<G>();
  greal mx = 0;
  for (int j = 0; j < k; j++) mx = fmax(mx, g.nu[j]);
  const greal th = mx * gEps;
  const greal threshold_helper = th * th / (greal)k;
  const greal ndt = sqrt(gEps);
  int np = k;
  for (int p = 0; p < k; p++) {
    int bi = p;
    greal bv = g.nu[p];
    for (int j = p + 1; j < k; j++)
      if (g.nu[j] > bv) { bv = g.nu[j]; bi = j; }
    if (np == k) near |= near_thr(bv * bv, threshold_helper * (greal)(k - p), greal(kNearBand) * greal(kNearBand));
    if (np == k && bv * bv < threshold_helper * (greal)(k - p)) np = p;
    gsync<G>();
    if (lane == 0) g.cperm[p] = bi;
    if (bi != p) {
      if (lane < k) {
        greal t = g.qr[lane + p * LD];
        g.qr[lane + p * LD] = g.qr[lane + bi * LD];
        g.qr[lane + bi * LD] = t;
      }
      if (lane == 0) {
        greal t = g.nu[p]; g.nu[p] = g.nu[bi]; g.nu[bi] = t;
        t = g.nd[p]; g.nd[p] = g.nd[bi]; g.nd[bi] = t;
      }
    }
    gsync<G>();
    // makeHouseholderInPlace on column p, rows p..k-1
    const int len = k - p;
    greal c0 = g.qr[p + p * LD];
    greal tail = 0;
    for (int i = 1; i < len; i++) tail += g.qr[p + i + p * LD] * g.qr[p + i + p * LD];
    greal tau, beta;
    if (len == 1 || tail <= gTiny) {
      tau = 0;
      beta = c0;
      if (lane >= 1 && lane < len) g.qr[p + lane + p * LD] = 0;
    } else {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0) beta = -beta;
      greal den = c0 - beta;
      if (lane >= 1 && lane < len) g.qr[p + lane + p * LD] /= den;
      tau = (beta - c0) / beta;
    }
    gsync<G>();
    if (lane == 0) { g.qr[p + p * LD] = beta; g.hc[p] = tau; }
    // apply to columns p+1..k-1, then downdate their norms (one column per lane)
    const int j = lane;
    if (j > p && j < k) {
      if (len == 1) {
        g.qr[p + j * LD] *= (1 - tau);
      } else if (tau != 0) {
        greal tmp = 0;
        for (int i = 1; i < len; i++) tmp += g.qr[p + i + p * LD] * g.qr[p + i + j * LD];
        tmp += g.qr[p + j * LD];
        g.qr[p + j * LD] -= tau * tmp;
        for (int i = 1; i < len; i++) g.qr[p + i + j * LD] -= tau * g.qr[p + i + p * LD] * tmp;
      }
      if (g.nu[j] != 0) {
        greal temp = fabs(g.qr[p + j * LD]) / g.nu[j];
        temp = (1 + temp) * (1 - temp);
        temp = temp < 0 ? 0 : temp;
        greal ratio = g.nu[j] / g.nd[j];
        greal temp2 = temp * (ratio * ratio);
        if (temp2 <= ndt) {
          greal s = 0;
          for (int i = p + 1; i < k; i++) s += g.qr[i + j * LD] * g.qr[i + j * LD];
          g.nd[j] = sqrt(s);
          g.nu[j] = g.nd[j];
        } else {
          g.nu[j] *= sqrt(temp);
        }
      }
    }
    gsync<G>();
  }
  return np;
}

// QR solve m z = b (least squares, basic solution) -> g.z
template <class G>
__device__ void qr_solve(G& g, int k, int np, int lane) {
  constexpr int LD = G::LD;
  if (lane < k) { g.c[lane] = g.b[lane]; g.z[lane] = greal(0); }
  gsync<G>();
  if (np == 0) return;
  for (int p = 0; p < np; p++) {
    const int len = k - p;
    const greal tau = g.hc[p];
    if (len == 1) {
      if (lane == p) g.c[p] *= (1 - tau);
    } else if (tau != 0) {
      greal tmp = 0;
      for (int i = 1; i < len; i++) tmp += g.qr[p + i + p * LD] * g.c[p + i];
      tmp += g.c[p];
      gsync<G>();
      if (lane == 0) g.c[p] -= tau * tmp;
      if (lane >= 1 && lane < len) g.c[p + lane] -= tau * g.qr[p + lane + p * LD] * tmp;
    }
    gsync<G>();
  }
  upper_solve_shared<G>(g.qr, g.c, np, lane);
  if (lane == 0) {
    int perm[HS_KMAX];
    for (int i = 0; i < k; i++) perm[i] = i;
    for (int p = 0; p < k; p++) { int t = perm[p]; perm[p] = perm[g.cperm[p]]; perm[g.cperm[p]] = t; }
    for (int i = 0; i < np; i++) g.z[perm[i]] = g.c[i];
  }
  gsync<G>();
}

// S3 general: adaptive-rank two-stage least squares (ftsolver.cpp:185-236) -> sv.y.
// The reference re-runs FullPivLU on the same zeroth-order Gram every pass; it
// is factorized once here (identical factors), only the rank threshold moves.
template <class SV, class G>
__device__ uint32_t contact_solve(SV& sv, G& g, int k, int lane) {
  constexpr int LD = G::LD;
  uint32_t flags = 0;
  if (k == 0) return HS_FLAG_NO_CONTACT;
  const LUInfo info = fullpiv_lu(g, k, lane);
  STAMP(10);
  int rank0 = k;
  int iters = 0;
  greal rel_error = 0;
  bool ill = false;  // the last pass's second stage ill-conditioned (gCondQR)
  do {
    iters++;
    greal thr = gEps * (greal)k;
    int r = lu_rank(g, info, thr);
    for (int guard = 0; guard < 2100 && r > rank0; guard++) {  // setThreshold doubling
      thr = 2 * thr;
      r = lu_rank(g, info, thr);
      flags |= HS_FLAG_NEAR_RANK;  // the threshold now sits within 2x of a pivot by construction
    }
    if (lu_near(g, info, thr)) flags |= HS_FLAG_NEAR_RANK;
    lu_solve(g, info, k, r, lane);
    lu_kernel_image(g, info, k, r, thr, lane);
    STAMP(11);
    if (r == k) flags |= HS_FLAG_FULL_RANK;
    rank0 = r;
    const int dimker = k - r;
    // b = -(ntx1 + ntn1 y0)
    if (lane < k) {
      int i = lane, b0 = (i / 3) * 3;
      greal t = greal(0);
      if (g.coupled)
        for (int kk = 0; kk < k; kk++) t = t + ntn1_full(g, i, kk) * g.y0[kk];
      else
        for (int kk = b0; kk < b0 + 3; kk++) t = t + ntn1_at(g, i, kk) * g.y0[kk];
      g.b[i] = -(g.ntx1[i] + t);
    }
    for (int e = lane; e < k * k; e += HALF) {  // m, built straight into the QR buffer
      int i = e % k, j = e / k;
      g.qr[i + j * LD] = m_at(g, k, dimker, i, j);
    }
    gsync<G>();
    STAMP(12);
    bool qr_near = false;
    int np = colpiv_qr(g, k, lane, qr_near);
    if (qr_near) flags |= HS_FLAG_NEAR_RANK;
    {  // the smallest kept pivot of this pass (the last pass's decides)
      greal rmin = greal(INFINITY);
      for (int i = 0; i < np; i++) rmin = fmin(rmin, fabs(g.qr[i + i * LD]));
      ill = np > 0 && rmin < gCondQR * fabs(g.qr[0]);
    }
    STAMP(13);
    qr_solve(g, k, np, lane);
    STAMP(14);
    // rel_error = |m z - b| / |b|
    if (lane < k) {
      greal s = greal(0);
      for (int j = 0; j < k; j++) s = s + m_at(g, k, dimker, lane, j) * g.z[j];
      g.c[lane] = s - g.b[lane];
    }
    gsync<G>();
    greal rn = 0, bn = 0;
    for (int i = 0; i < k; i++) { rn += g.c[i] * g.c[i]; bn += g.b[i] * g.b[i]; }
    rel_error = sqrt(rn) / sqrt(bn);
    if (near_thr(rel_error, gRelTol, greal(10))) flags |= HS_FLAG_NEAR_RANK;
    rank0--;
    if (lane < k) {
      greal s = greal(0);
      for (int j = 0; j < dimker; j++) s = s + g.Ny[lane + j * LD] * g.z[j];
      sv.y[lane] = g.y0[lane] + s;
    }
    gsync<G>();
    if (rel_error > gRelTol && rank0 <= 0) { flags |= HS_FLAG_LOOP_EXHAUST; break; }
  } while (rel_error > gRelTol && iters <= HS_KMAX + 1);
  if (iters > 1) flags |= HS_FLAG_RANK_RETRY;
  if (ill) flags |= HS_FLAG_NEAR_RANK;
  return flags;
}

// The general path is an out-of-line call: it keeps its own register allocation apart from the
// kernel body's 168-VGPR budget (3 waves/SIMD). Inlined at that budget (the former HS_GENERAL_INLINE
// build) hipcc of ROCm 7.2 spills 7 VGPRs in the block that fullpiv_lu's lane-0 permutation loop
// falls through to when its last lane leaves -- before that block restores EXEC, so the spill stores
// run with EXEC == 0 and write nothing, and their reloads return stale scratch: wrong forces on every
// HS_SOLVE_REFERENCE step. tools/isa_check.py finds the pattern in the built
// library and hslabs_amd/build.py refuses a library that has it. The call costs only the steps that
// take it (stack frame in scratch, 288 B per lane).
template <class W, class SV, class G>
__device__ __attribute__((noinline)) uint32_t general_solve(const hs_topo* T, SV& sv, G& g, const W& w, int k, int lane) {
  build_grams(T, sv, g, w, k, lane);
  STAMP(9);
  return contact_solve(sv, g, k, lane);
}

// ---------------------------------------------------------------------------
// S3 fast path: closed form of the same lexicographic least squares
// (oracle/hs_oracle.cpp fast_contact_solve, identical operation order).
// One lane per contact builds A_c, D_c, g_c; >= 3 contacts: 6x6 Schur
// complement of the zeroth-order constraints; 1 contact: unique LS; 2 contacts:
// rank-5 kernel along the feet line. Returns false (wave-uniform) when a
// Cholesky pivot falls under the guard -> general path.
// ---------------------------------------------------------------------------
// conditioning guard of the closed-form Cholesky pivots (relative to the largest diagonal)
constexpr real kFastPivotGuard = HS_REAL_IS_FLOAT ? real(1e-4) : real(1e-10);

// Nearly collinear contact feet (nc >= 3): the zeroth-order Gram G = A A^T = sum_c A_c A_c^T is
// close to rank 5. The reference's loop (ftsolver.cpp:205-232) then sees a rank-deficient first-order
// system (its ntn0 * Ry columns carry G's conditioning squared), finds rel_error > 1e-6 and retries at
// lower ranks, landing on a different answer from the closed form's exact minimizer. G's smallest
// eigenvalue is that of J = sum_c [e_c]x [e_c]x^T = tr(C) I - C (the Schur complement of its
// translation block; e_c = d0_c - mean d0, C = sum_c e_c e_c^T), i.e. mu2 + mu3 for C's eigenvalues
// mu1 >= mu2 >= mu3, which c2(C) / tr(C) gives to within a factor of 4 (c2 = the sum of C's principal
// 2x2 minors). The closed form is taken only when c2(C) / (tr(C) maxdiag(G)) >= kZerothGuard; the
// ratio follows the reference's 6th FullPivLU pivot ratio to within ~2x. Over the oracle's tree mode on
// 120k transformed steps every retry had it below 2.5e-5; plain synthetic gaits stay
// above 1e-2. Steps under the guard take the Eigen-style path, which restates the reference's loop.
// No division: with s = sum d0_c and Q = sum d0_c d0_c^T, C' = nc Q - s s^T = nc C, so the test reads
// c2(C') >= kZerothGuard * nc * tr(C') * maxdiag(G), maxdiag(G) = max(nc, tr Q - Q_ii). A heuristic
// with a 40x margin on each side, so it runs in single precision: contact lane c holds d0_c, the nine
// moments are summed over the 8-lane group by DPP (quad xor 1, xor 2, half-row mirror), and lanes past
// nc add zeros. Every lane of the half-wave calls it; the verdict is the same on lanes 0 .. 7.
constexpr float kZerothGuard = 1e-3f;

template <int CTRL>
__device__ inline float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ inline float group8_sum(float v) {
  v += dpp_f<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_f<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_f<0x141>(v);  // row_half_mirror: lane i <- 7 - i, the other quad's sum
  return v;
}

// a real moved across lanes by DPP control CTRL (a double as two 32-bit moves)
template <int CTRL>
__device__ inline real dpp_r(real x) {
#if HS_REAL_IS_FLOAT
  return dpp_f<CTRL>(x);
#else
  const long long u = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_mov_dpp((int)u, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(u >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
#endif
}
// sum over the 4-lane quad (DPP quad_perm xor 1, xor 2): every lane of the quad gets the same value
// (each addition is commutative in its two operands)
__device__ inline real quad_sum(real v) {
  v += dpp_r<0xB1>(v);
  v += dpp_r<0x4E>(v);
  return v;
}

// bit 0: well posed (take the closed form); bit 1: the ratio lies within kNearBand of the guard
// (HS_FLAG_NEAR_RANK: another rounding may route the step the other way)
template <class W, class SV>
__device__ inline int zeroth_well_posed(const real* P0, const W& w, const SV& sv, int nc, int lane) {
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  if (lane < nc) {
    const real* fp = w.fpos(0, sv.cfoot[lane]);
    d0 = float(P0[0] - fp[0]); d1 = float(P0[1] - fp[1]); d2 = float(P0[2] - fp[2]);
  }
  const float s0 = group8_sum(d0), s1 = group8_sum(d1), s2 = group8_sum(d2);
  const float q00 = group8_sum(d0 * d0), q11 = group8_sum(d1 * d1), q22 = group8_sum(d2 * d2);
  const float q01 = group8_sum(d0 * d1), q02 = group8_sum(d0 * d2), q12 = group8_sum(d1 * d2);
  const float k = float(nc);
  const float c00 = k * q00 - s0 * s0, c11 = k * q11 - s1 * s1, c22 = k * q22 - s2 * s2;
  const float c01 = k * q01 - s0 * s1, c02 = k * q02 - s0 * s2, c12 = k * q12 - s1 * s2;
  const float c2 = (c00 * c11 - c01 * c01) + (c00 * c22 - c02 * c02) + (c11 * c22 - c12 * c12);
  const float tq = q00 + q11 + q22;
  const float md = fmaxf(k, fmaxf(tq - q00, fmaxf(tq - q11, tq - q22)));
  const float t = kZerothGuard * k * (c00 + c11 + c22) * md;
  return (c2 >= t ? 1 : 0) | (c2 >= t / float(kNearBand) && c2 <= t * float(kNearBand) ? 2 : 0);  // 0 on NaN
}

// rl (N): receives 1 / L_jj, the reciprocal each pivot's column was scaled by, for chol_solve_n
// near: set when a pivot lies within kNearBand of the guard (HS_FLAG_NEAR_RANK)
template <int N>
__device__ inline bool chol_n(real* a, real guard, real* rl_out, bool& near) {  // row-major, in place
  real mx = 0;
#pragma unroll
  for (int i = 0; i < N; i++) mx = fmax(mx, a[i * N + i]);
#pragma unroll
  for (int j = 0; j < N; j++) {
    real s = a[j * N + j];
#pragma unroll
    for (int k = 0; k < j; k++) s -= a[j * N + k] * a[j * N + k];
    near |= near_thr(s, guard * mx, kNearBand);
    if (!(s > guard * mx)) return false;
    const real l = sqrt(s), rl = real(1) / l;  // one division per pivot (oracle chol)
    a[j * N + j] = l;
    rl_out[j] = rl;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      real t = a[i * N + j];
#pragma unroll
      for (int k = 0; k < j; k++) t -= a[i * N + k] * a[j * N + k];
      a[i * N + j] = t * rl;
    }
  }
  return true;
}

// rl: chol_n's reciprocals of the pivots (1 / L_ii, the same divisions, not recomputed)
template <int N>
__device__ inline void chol_solve_n(const real* L, const real* rl, real* b) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    real s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[i * N + k] * b[k];
    b[i] = s * rl[i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    real s = b[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s -= L[k * N + i] * b[k];
    b[i] = s * rl[i];
  }
}

// LDL^T of an N x N SPD matrix in place (row-major; lower part: unit-lower L, diagonal: d), no
// square roots: pivot d_j = a_jj - sum_k L_jk (L_jk d_k), the Cholesky pivot in exact arithmetic, so
// the guard (d_j > guard * max diagonal) decides like chol_n's. rd: 1 / d_j. False: a pivot under it.
// 1 / x for a positive normal pivot: v_rcp_f64 refined by two Newton steps (within an ulp of the
// correctly rounded quotient), five instructions instead of the IEEE division's scale / fixup sequence
__device__ inline real pivot_rcp(real x) {
#if !HS_REAL_IS_FLOAT
  real r = __builtin_amdgcn_rcp(x);
  real e = fma(-x, r, real(1));
  r = fma(r, e, r);
  e = fma(-x, r, real(1));
  return fma(r, e, r);
#else
  return real(1) / x;
#endif
}

// near (guarded factorizations): set when a pivot lies within kNearBand of the guard
template <int N>
__device__ inline bool ldl_n(real* a, real guard, real* rd, bool& near) {
  real mx = 0;
#pragma unroll
  for (int i = 0; i < N; i++) mx = fmax(mx, a[i * N + i]);
#pragma unroll
  for (int j = 0; j < N; j++) {
    real v[N];  // L_jk d_k
#pragma unroll
    for (int k = 0; k < j; k++) v[k] = a[j * N + k] * a[k * N + k];
    real dj = a[j * N + j];
#pragma unroll
    for (int k = 0; k < j; k++) dj -= a[j * N + k] * v[k];
    near |= near_thr(dj, guard * mx, kNearBand);
    if (!(dj > guard * mx)) return false;
    const real r = pivot_rcp(dj);
    a[j * N + j] = dj;
    rd[j] = r;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      real t = a[i * N + j];
#pragma unroll
      for (int k = 0; k < j; k++) t -= a[i * N + k] * v[k];
      a[i * N + j] = t * r;
    }
  }
  return true;
}

// unguarded (guard 0: SPD by construction, no decision taken)
template <int N>
__device__ inline bool ldl_n(real* a, real guard, real* rd) {
  bool unused = false;
  return ldl_n<N>(a, guard, rd, unused);
}

// solve L D L^T x = b in place with ldl_n's factors
template <int N>
__device__ inline void ldl_solve_n(const real* L, const real* rd, real* b) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    real s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[i * N + k] * b[k];
    b[i] = s;
  }
#pragma unroll
  for (int i = 0; i < N; i++) b[i] *= rd[i];
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    real s = b[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s -= L[k * N + i] * b[k];
    b[i] = s;
  }
}

__device__ inline void cross_rows(const real* d, real v[3][3]) {
  v[0][0] = 0;     v[0][1] = -d[2]; v[0][2] = d[1];
  v[1][0] = d[2];  v[1][1] = 0;     v[1][2] = -d[0];
  v[2][0] = -d[1]; v[2][1] = d[0];  v[2][2] = 0;
}

// entry (r, j) of A_c = [-I; [d0]x] (the values cross_rows lays out)
__device__ inline real a_entry(const real* d0, int r, int j) {
  if (r < 3) return (r == j) ? real(-1) : real(0);
  const int i = r - 3;
  if (i == j) return real(0);
  const real v = d0[3 - i - j];
  return ((j - i + 3) % 3 == 1) ? -v : v;
}

// In-place Cholesky of a k x k SPD matrix (row-major, lower triangle used) by
// the half-wave, right-looking: element (i, j) gets its products subtracted in
// increasing order, exactly like the oracle's left-looking chol(). False (wave-
// uniform) when a pivot falls to guard * (max original diagonal) or below.
// rdiag (optional) receives 1 / L_jj.
// (GLOBAL: K lives in global memory, so the exchanges need the workgroup's global-memory fences)
template <bool GLOBAL>
__device__ inline void ws_sync() {
  if constexpr (GLOBAL) __syncthreads();
  else wave_sync();
}

// Lane-strided walks over matrix entries without integer divisions (a 32-bit division by a
// runtime size is ~40 VALU instructions) or per-step loops. TriWalk: the packed lower triangle row
// by row ((0,0), (1,0), (1,1), (2,0), ...) with rows of r + 1 + EXTRA entries, entries p = lane,
// lane + 32, ...: the row from a single-precision square root (exact for p < 2^20), corrected by
// one step either way
template <int EXTRA = 0>
struct TriWalk {
  int p, r, c;
  __device__ explicit TriWalk(int p_) : p(p_) { locate(); }
  // first index of row r: r (r + 1) / 2 + EXTRA r = r (r + 1 + 2 EXTRA) / 2
  __device__ static int row0(int r) { return r * (r + 1 + 2 * EXTRA) / 2; }
  __device__ void locate() {
    const float b = 1.0f + 2.0f * EXTRA;  // r^2 + b r - 2 p = 0
    r = (int)((sqrtf(b * b + 8.0f * (float)p) - b) * 0.5f);
    if (row0(r + 1) <= p) r++;
    if (row0(r) > p) r--;
    c = p - row0(r);
  }
  __device__ void next() {
    p += HALF;
    locate();
  }
};
// RectWalk: row-major entries of an (any) x ld rectangle
struct RectWalk {
  int r, c, ld;
  __device__ RectWalk(int p, int ld_) : r(0), c(p), ld(ld_) { settle(); }
  __device__ void settle() {
    while (c >= ld) { c -= ld; r++; }
  }
  __device__ void next() { c += HALF; settle(); }
};

template <bool GLOBAL>
__device__ __attribute__((always_inline)) inline bool chol_half(real* K, int k, real guard, int lane, bool& near,
                                                                 real* rdiag = nullptr) {
  real mx = 0;
  for (int i = 0; i < k; i++) mx = fmax(mx, K[i * k + i]);
  for (int j = 0; j < k; j++) {
    const real s = K[j * k + j];
    near |= near_thr(s, guard * mx, kNearBand);
    if (!(s > guard * mx)) return false;
    const real l = sqrt(s), rl = real(1) / l;
    if (lane == 0) {
      K[j * k + j] = l;
      if (rdiag) rdiag[j] = rl;
    }
    for (int i = j + 1 + lane; i < k; i += HALF) K[i * k + j] = K[i * k + j] * rl;
    ws_sync<GLOBAL>();
    const int m = k - 1 - j;
    for (int e = lane; e < m * m; e += HALF) {
      const int i = j + 1 + e / m, c2 = j + 1 + e % m;
      if (c2 <= i) K[i * k + c2] -= K[i * k + j] * K[c2 * k + j];
    }
    ws_sync<GLOBAL>();
  }
  return true;
}

// packed lower-triangle index (row-major: row r holds r + 1 entries)
__device__ inline int pk(int r, int c) { return r * (r + 1) / 2 + c; }

// chol_half's right-looking Cholesky on a packed lower triangle in LDS (solve_forces: its normal
// matrix), the same operations per entry; the trailing update walks the packed entries. A pivot at or
// under guard * (largest diagonal) drops its variable (returned in the mask): its column is zeroed, so
// the later pivots are those of the system without it, and the caller's solves leave it at 0 -- the
// basic solution of a rank-deficient least squares (SparseQR's, ftsolver.cpp:349-353, in the natural
// column order). near: a pivot within kNearBand of the guard (HS_FLAG_NEAR_RANK).
__device__ __attribute__((always_inline)) inline uint32_t chol_packed(real* K, int k, real guard, int lane,
                                                                      bool& near) {
  real mx = 0;
  for (int i = 0; i < k; i++) mx = fmax(mx, K[pk(i, i)]);
  uint32_t dropped = 0;
  // one pivot's column: scaled by 1 / L_jj, or zeroed when the pivot is dropped (L_jj = 1 then)
  auto pivot = [&](int j) {
    const real s = K[pk(j, j)];
    near |= near_thr(s, guard * mx, kNearBand);
    const bool keep = s > guard * mx;  // false on NaN
    const real l = keep ? sqrt(s) : real(1), rl = keep ? real(1) / l : real(0);
    if (!keep) dropped |= 1u << j;
    if (lane == 0) K[pk(j, j)] = l;
    for (int i = j + 1 + lane; i < k; i += HALF) K[pk(i, j)] = K[pk(i, j)] * rl;
    wave_sync();
  };
  // two pivots per trailing pass: pivot j, column j + 1 updated by it, pivot j + 1, then every
  // entry right of both takes pivot j's product and pivot j + 1's in that order -- each entry sees
  // the operations of one pivot at a time, in pivot order, as in chol_half
  for (int j = 0; j < k; j += 2) {
    const bool two = j + 1 < k;
    pivot(j);
    if (two) {
      for (int i = j + 1 + lane; i < k; i += HALF) K[pk(i, j + 1)] -= K[pk(i, j)] * K[pk(j + 1, j)];
      wave_sync();
      pivot(j + 1);
    }
    const int j1 = two ? j + 2 : j + 1, m = k - j1;
    for (TriWalk<> t(lane); t.r < m; t.next()) {  // the trailing lower triangle, entry by entry
      const int i = j1 + t.r, c2 = j1 + t.c;
      real v = K[pk(i, c2)];
      v -= K[pk(i, j)] * K[pk(c2, j)];
      if (two) v -= K[pk(i, j + 1)] * K[pk(c2, j + 1)];
      K[pk(i, c2)] = v;
    }
    wave_sync();
  }
  return dropped;
}

// nc >= 3 with a singular D_c (straight, IK-clamped leg) or Schur complement:
// augmented system K = D + rho A^T A, w = -K^-1 (g~ + A^T lam),
// (A K^-1 A^T) lam = a - A K^-1 g~ (oracle aug_solve, same operation order; the
// half-wave right-looking Cholesky subtracts in the oracle's left-looking order).
// False when the minimizer is not unique (a pivot under the guard).
template <class SV>
__device__ __attribute__((always_inline)) inline bool aug_solve(FastL& fl, AugL& ag, SV& sv, const real* a, int nc,
                                                                int lane, bool& near) {
  const int k = 3 * nc;
  auto Aat = [&](int r, int i) { return a_entry(fl.d0[i / 3], r, i % 3); };  // A (6 x k)
  real md = 0, ma = 0;
  for (int c = 0; c < nc; c++)
    for (int i = 0; i < 3; i++) {
      md = fmax(md, fl.D[c][4 * i]);
      real s = 0;
      for (int r = 0; r < 6; r++) s += Aat(r, 3 * c + i) * Aat(r, 3 * c + i);
      ma = fmax(ma, s);
    }
  const real rho = (md > 0 && ma > 0) ? md / ma : real(1);
  for (int e = lane; e < k * k; e += HALF) {
    const int i = e / k, j = e % k;
    real s = 0;
    for (int r = 0; r < 6; r++) s += Aat(r, i) * Aat(r, j);
    ag.K[i * k + j] = ((i / 3 == j / 3) ? fl.D[i / 3][3 * (i % 3) + j % 3] : real(0)) + rho * s;
  }
  for (int e = lane; e < k * 7; e += HALF) {
    const int i = e / 7, q = e % 7;
    real v;
    if (q < 6) {
      v = Aat(q, i);
    } else {
      real s = 0;
      for (int r = 0; r < 6; r++) s += Aat(r, i) * a[r];
      v = fl.g[i / 3][i % 3] + rho * s;
    }
    ag.X[i * 7 + q] = v;
  }
  __syncthreads();
  if (!chol_half<true>(ag.K, k, kFastPivotGuard, lane, near, ag.rdiag)) return false;
  __syncthreads();
  if (lane < 7) {  // K X = [A^T | g~], one right-hand column per lane
    const int q = lane;
    for (int i = 0; i < k; i++) {
      real s = ag.X[i * 7 + q];
      for (int m = 0; m < i; m++) s -= ag.K[i * k + m] * ag.X[m * 7 + q];
      ag.X[i * 7 + q] = s * ag.rdiag[i];
    }
    for (int i = k - 1; i >= 0; i--) {
      real s = ag.X[i * 7 + q];
      for (int m = i + 1; m < k; m++) s -= ag.K[m * k + i] * ag.X[m * 7 + q];
      ag.X[i * 7 + q] = s * ag.rdiag[i];
    }
  }
  __syncthreads();
  for (int e = lane; e < 42; e += HALF) {
    const int r = e / 7, q = e % 7;
    real s = 0;
    for (int i = 0; i < k; i++) s += Aat(r, i) * ag.X[i * 7 + q];
    if (q < 6) ag.St[6 * r + q] = s;
    else ag.lam[r] = a[r] - s;
  }
  __syncthreads();
  if (lane == 0) {
    real St[36], lam[6];
    for (int i = 0; i < 36; i++) St[i] = ag.St[i];
    for (int i = 0; i < 6; i++) lam[i] = ag.lam[i];
    real rl[6];
    int ok = chol_n<6>(St, kFastPivotGuard, rl, near);
    if (ok) {
      chol_solve_n<6>(St, rl, lam);
      for (int i = 0; i < 6; i++) ag.lam[i] = lam[i];
    }
    ag.ok = ok;
  }
  __syncthreads();
  if (!ag.ok) return false;
  for (int i = lane; i < k; i += HALF) {
    real s = ag.X[i * 7 + 6];
    for (int r = 0; r < 6; r++) s += ag.X[i * 7 + r] * ag.lam[r];
    sv.y[i] = -s;
  }
  __syncthreads();
  return true;
}

// aug_ok = false (the fixup launch's idle half, which stores nothing): decline instead of using the
// augmented system, whose global workspace is the idle slot every fixup wavefront shares
// lnear: this lane saw a routing decision within kNearBand of its guard (fast_solve ballots it)
template <class W, class SV>
__device__ __attribute__((always_inline)) inline bool fast_solve_lanes(const hs_topo* T, SV& sv, FastL& fl, AugL& ag,
                                                                       const W& w, int nc, bool aug_ok, int lane,
                                                                       bool& lnear) {
  const int n = T->n;
  if (nc == 0) return true;
  const real* P0 = w.pos(0, 0);
  const int zw = nc >= 3 ? zeroth_well_posed(P0, w, sv, nc, lane) : 1;
  const int coll = (zw & 1) ? 0 : 2;
  lnear |= (zw & 2) != 0 && lane < 8;  // the group of lanes 0 .. 7 holds the contacts' sums
  // four lanes per contact (lane = 4 c + s): lane s sums the D_c / g_c terms of the foot chain's
  // joints s, s + 4, the quad adds them (DPP), every lane of the quad factorizes D_c, and the Schur
  // block's rows are split {s, 5 - s} (seven packed entries and two of h per lane; lane 3 repeats
  // lane 2's rows and stores D_c, g_c, d0_c and D_c^-1 instead) -- one instruction stream, the lanes
  // differing only in data. The blocks are summed over the contacts across the lanes (sch below)
  real sch[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // this lane's 7 packed entries and 2 of h; 0 past nc
  {
    const int c = lane >> 2, s4 = lane & 3;
    if (c < nc) {
      const int fi = sv.cfoot[c];
      const real* fp = w.fpos(0, fi);
      real d0[3];
      for (int r = 0; r < 3; r++) d0[r] = P0[r] - fp[r];
      real Dp[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};  // packed lower 00 10 11 20 21 22
      const uint8_t* fch = reinterpret_cast<const uint8_t*>(sv.fch[fi]);
      const int nch = fch[0];
      for (int m = s4; m < nch; m += 4) {
        const int p = fch[1 + m];
        const real* Jp = w.jpos(0, p);
        const real* Jz = w.jz(0, p);
        real da[3], va[3][3];
        for (int r = 0; r < 3; r++) da[r] = Jp[r] - fp[r];
        cross_rows(da, va);
#pragma unroll
        for (int r = 0; r < 3; r++) {
          const real w2 = Jz[r] * Jz[r];
#pragma unroll
          for (int i = 0; i < 3; i++) {
            if (i == r) continue;
#pragma unroll
            for (int j = 0; j <= i; j++)
              if (j != r) Dp[i * (i + 1) / 2 + j] += w2 * va[r][i] * va[r][j];
            g[i] += w2 * va[r][i] * sv.x[3 * n + 3 * p + r];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 6; e++) Dp[e] = quad_sum(Dp[e]);
#pragma unroll
      for (int i = 0; i < 3; i++) g[i] = quad_sum(g[i]);
      const real D[9] = {Dp[0], Dp[1], Dp[3], Dp[1], Dp[2], Dp[4], Dp[3], Dp[4], Dp[5]};
      if (s4 == 0) DBG(24 + fi, Dp[0], 6);
      if (s4 == 0) DBG(24 + fi, g[0], 7);
      if (s4 == 3) {
        for (int r = 0; r < 3; r++) fl.d0[c][r] = d0[r];
        for (int i = 0; i < 9; i++) fl.D[c][i] = D[i];
        for (int i = 0; i < 3; i++) fl.g[c][i] = g[i];
      }
      int ok = 1;
      if (nc >= 3) {
        real L[9];
        for (int i = 0; i < 9; i++) L[i] = D[i];
        real rl[3];
        ok = ldl_n<3>(L, kFastPivotGuard, rl, lnear);
        if (ok) {
          real Dinv[9];
          for (int j = 0; j < 3; j++) {
            real e[3] = {0, 0, 0};
            e[j] = 1;
            ldl_solve_n<3>(L, rl, e);
            for (int i = 0; i < 3; i++) Dinv[3 * i + j] = e[i];
          }
          if (s4 == 3)
            for (int i = 0; i < 9; i++) fl.sc.Dinv[c][i] = Dinv[i];
          const int sr = s4 < 3 ? s4 : 2, r0 = sr, r1 = 5 - sr;
          real E0[3], E1[3];  // rows r0, r1 of E = A_c D_c^-1
#pragma unroll
          for (int j = 0; j < 3; j++) {
            real a = 0, b = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
              a += a_entry(d0, r0, i) * Dinv[3 * i + j];
              b += a_entry(d0, r1, i) * Dinv[3 * i + j];
            }
            E0[j] = a;
            E1[j] = b;
          }
#pragma unroll
          for (int t = 0; t < 7; t++) {  // row r0's r0 + 1 entries, then row r1's
            const bool first = t <= r0;  // entry (r0, t) or (r1, t - r0 - 1)
            const int q = first ? t : t - r0 - 1;
            real v = 0;
#pragma unroll
            for (int j = 0; j < 3; j++) v += (first ? E0[j] : E1[j]) * a_entry(d0, q, j);
            if (s4 < 3) sch[t] = v;
          }
          real h0 = 0, h1 = 0;
          for (int j = 0; j < 3; j++) {
            h0 += E0[j] * g[j];
            h1 += E1[j] * g[j];
          }
          if (s4 < 3) {
            sch[7] = h0;
            sch[8] = h1;
          }
        }
      }
      if (s4 == 0) fl.ok[c] = ok | coll;
    }
  }
  // sum over the contacts c = 0 .. 7 of lanes 4 c + s: within each 16-lane row by DPP (row_shr 4, then
  // 8: lane 12 + s holds its row's four contacts), then the two rows (xor 16). Lanes 12 .. 14 store the
  // packed [S | h] (a pairwise order, not the contacts' sequence: ULPs of the Schur complement)
#pragma unroll
  for (int e = 0; e < 9; e++) {
    real v = sch[e];
    v += dpp_r<0x114>(v);
    v += dpp_r<0x118>(v);
    sch[e] = v + __shfl_xor(v, 16);
  }
  {
    const int s4 = lane & 3, r0 = s4, r1 = 5 - s4;
    if ((lane & ~3) == 12 && s4 < 3) {
#pragma unroll
      for (int t = 0; t < 7; t++) {
        const bool first = t <= r0;
        fl.sc.Ssum[first ? sch_lower(r0, t) : sch_lower(r1, t - r0 - 1)] = sch[t];
      }
      fl.sc.Ssum[SCH_H + r0] = sch[7];
      fl.sc.Ssum[SCH_H + r1] = sch[8];
    }
  }
  wave_sync();
  STAMP(18);
  const real a[6] = {sv.x[0], sv.x[1], sv.x[2], sv.x[3 * n], sv.x[3 * n + 1], sv.x[3 * n + 2]};
  if (nc >= 3 && (fl.ok[0] & 2)) return false;  // nearly collinear contacts: the Eigen-style path
  for (int c = 0; c < nc; c++)
    if (!(fl.ok[c] & 1)) return aug_ok ? aug_solve(fl, ag, sv, a, nc, lane, lnear) : false;  // only nc >= 3 factors D_c
  int ok = 1;
  if (nc == 1) {  // unique least-squares solution (A^T A) w = -A^T a
    if (lane == 0) {
      real M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
      const real* d0 = fl.d0[0];
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
          for (int r = 0; r < 6; r++) M[3 * i + j] += a_entry(d0, r, i) * a_entry(d0, r, j);
        for (int r = 0; r < 6; r++) b[i] -= a_entry(d0, r, i) * a[r];
      }
      real rl[3];
      DBG(24 + sv.cfoot[0], M[4], 19);
      DBG(24 + sv.cfoot[0], b[1], 20);
      ok = chol_n<3>(M, kFastPivotGuard, rl, lnear);
      if (ok) {
        chol_solve_n<3>(M, rl, b);
        for (int i = 0; i < 3; i++) sv.y[i] = b[i];
        DBG(24 + sv.cfoot[0], b[0], 21);
      }
      fl.ok[0] = ok;
    }
  } else if (nc == 2) {  // rank 5: kernel n = (u,-u)/sqrt2 along the line between the feet
    if (lane == 0) {
      const real* f0 = w.fpos(0, sv.cfoot[0]);
      const real* f1 = w.fpos(0, sv.cfoot[1]);
      real u[3], un = 0;
      for (int r = 0; r < 3; r++) { u[r] = f0[r] - f1[r]; un += u[r] * u[r]; }
      un = sqrt(un);
      ok = un > real(1e-12);
      real nv[6], M[36], b[6], rl[6];
      if (ok) {
        for (int r = 0; r < 3; r++) { nv[r] = u[r] / un / sqrt(real(2)); nv[3 + r] = -nv[r]; }
        DBG(24 + sv.cfoot[0], nv[2], 26);
        for (int i = 0; i < 6; i++) {
          const real* di = fl.d0[i / 3];
          for (int j = 0; j < 6; j++) {
            const real* dj = fl.d0[j / 3];
            real s = 0;
            for (int r = 0; r < 6; r++) s += a_entry(di, r, i % 3) * a_entry(dj, r, j % 3);
            M[6 * i + j] = s + nv[i] * nv[j];
          }
          real s = 0;
          for (int r = 0; r < 6; r++) s += a_entry(di, r, i % 3) * a[r];
          b[i] = -s;
        }
        DBG(24 + sv.cfoot[0], M[5], 27);
        opaque_vals<36>(M);  // the assembled system (hs_limb_kernel fences the same values)
        opaque_vals<6>(b);
        opaque_vals<6>(nv);
        ok = chol_n<6>(M, kFastPivotGuard, rl, lnear);
      }
      if (ok) {
        chol_solve_n<6>(M, rl, b);
        opaque_vals<6>(b);
        real nDn = 0, nr = 0;
        for (int c = 0; c < 2; c++)
          for (int i = 0; i < 3; i++) {
            real Dw = 0, Dn = 0;
            for (int j = 0; j < 3; j++) { Dw += fl.D[c][3 * i + j] * b[3 * c + j]; Dn += fl.D[c][3 * i + j] * nv[3 * c + j]; }
            nr += nv[3 * c + i] * (Dw + fl.g[c][i]);
            nDn += nv[3 * c + i] * Dn;
          }
        ok = nDn > 0;
        if (ok) {
          real t = -nr / nDn;
          for (int i = 0; i < 6; i++) sv.y[i] = b[i] + t * nv[i];
          DBG(24 + sv.cfoot[0], sv.y[0], 22);
          DBG(24 + sv.cfoot[0], b[0], 23);
          DBG(24 + sv.cfoot[0], t, 24);
        }
      }
      fl.ok[0] = ok;
    }
  } else {  // Schur complement of the 6 zeroth-order constraints (its entries summed above)
    if (lane == 0) {
      real Sm[36], h[6];
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) Sm[6 * i + j] = (j <= i) ? fl.sc.Ssum[sch_lower(i, j)] : real(0);  // upper: unread
      for (int i = 0; i < 6; i++) h[i] = fl.sc.Ssum[SCH_H + i];
      real lam[6], rl[6];
      for (int r = 0; r < 6; r++) lam[r] = a[r] - h[r];
      ok = ldl_n<6>(Sm, kFastPivotGuard, rl, lnear);
      if (ok) {
        ldl_solve_n<6>(Sm, rl, lam);
        for (int r = 0; r < 6; r++) fl.sc.lam[r] = lam[r];
      }
      fl.ok[0] = ok;
    }
    wave_sync();
    STAMP(19);
    if (!fl.ok[0]) return aug_ok ? aug_solve(fl, ag, sv, a, nc, lane, lnear) : false;
    if (lane < nc) {
      const int c = lane;
      const real* d0 = fl.d0[c];
      real t[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {  // g + A_c^T lam, A_c's zero entries skipped (exact zeros)
        real s = fl.g[c][i];
#pragma unroll
        for (int r = 0; r < 6; r++) {
          if (r < 3 && r != i) continue;
          if (r >= 3 && r - 3 == i) continue;
          s += a_entry(d0, r, i) * fl.sc.lam[r];
        }
        t[i] = s;
      }
      for (int i = 0; i < 3; i++) {
        real s = 0;
        for (int j = 0; j < 3; j++) s += fl.sc.Dinv[c][3 * i + j] * t[j];
        sv.y[3 * c + i] = -s;
      }
      DBG(24 + sv.cfoot[c], sv.y[3 * c], 8);
    }
  }
  wave_sync();
  return fl.ok[0] != 0;
}

// near (uniform over the half-wave): a routing decision of the closed form lay within kNearBand of its
// guard on some lane (HS_FLAG_NEAR_RANK)
template <class W, class SV>
__device__ __attribute__((always_inline)) inline bool fast_solve(const hs_topo* T, SV& sv, FastL& fl, AugL& ag, const W& w,
                                                                 int nc, bool aug_ok, int lane, bool& near) {
  bool lnear = false;
  const bool ok = fast_solve_lanes(T, sv, fl, ag, w, nc, aug_ok, lane, lnear);
  near = half_ballot(lnear) != 0;
  return ok;
}

// work_over_period's accumulation (periodic.cpp:301-302): work_dt *= dt_traj; work_period += work_dt --
// two roundings, as the reference's x86-64 build performs them (the step kernels are otherwise contracted)
__device__ inline real work_add(real work, real work_dt, real dt) {
#pragma clang fp contract(off)
  const real wdt = work_dt * dt;
  return work + wdt;
}

// selection COT of the best-rollout key (hs_best_key_cot, include/hslabs.h): one cycle's work over
// sum m * |L|; |L| under HS_KEY_MIN_STEP_LENGTH gives NaN (never selected)
__device__ inline real key_cot(real work, real mass, real L, int n_t, int steps) {
  const real aL = fabs(L);
  if (!(aL >= (real)HS_KEY_MIN_STEP_LENGTH) || steps < 1) return (real)NAN;
  return work * ((real)n_t / (real)steps) / (mass * aL);
}

__device__ inline uint64_t best_key(real cot, int64_t id) {
  float c = (float)cot;
  uint32_t bits = __float_as_uint(c);
  uint32_t ord = (c != c) ? 0xFFFFFFFFu : ((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u));
  return ((uint64_t)ord << 32) | (uint32_t)id;
}

// The work reduce of a fused call for rollouts blockIdx.x * 64 + lane (one wavefront per workgroup):
// work_cot[b] = (w, w / (total mass * step length)) with w = (accumulate ? work_cot[b][0] : 0) + the
// steps' joint work sums times dt in step order, then the best key
__device__ inline void reduce_rollouts(const hs_run_args& a, real total_mass, const double* __restrict__ rollout_mass,
                                       const real* __restrict__ ws, int n_steps, uint64_t* best_key_out,
                                       int key_steps) {
  const int b0 = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = b0 < a.n_rollouts;
  const int b = live ? b0 : a.n_rollouts - 1;  // dead lanes load a valid row and store nothing
  if (rollout_mass) total_mass = (real)rollout_mass[b];  // a mixed plan: the rollout's model
  real w = a.accumulate ? outp(a.work_cot)[2 * (size_t)b] : real(0);
  const real dt = (real)a.params[b].period / a.n_t;  // gait_setup's st.dt
  // periodic.cpp:302-303, in step order; the loads of up to 32 steps issue together ahead of their
  // FMAs (a 20-step job: one round trip)
  for (int s = 0; s < n_steps; s += 32) {
    real v[32];
#pragma unroll
    for (int j = 0; j < 32; j++) v[j] = s + j < n_steps ? ws[(size_t)(s + j) * a.n_rollouts + b] : real(0);
#pragma unroll
    for (int j = 0; j < 32; j++)
      if (s + j < n_steps) w = work_add(w, v[j], dt);
  }
  const real L = (real)a.params[b].step_length;
  const real cot = w / (total_mass * L);
  if (live) {
    outp(a.work_cot)[2 * (size_t)b] = w;
    outp(a.work_cot)[2 * (size_t)b + 1] = cot;
  }
  if (best_key_out) {  // the wave's minimum first: one atomic per wave, not one per rollout on one address
    const real kc = key_cot(w, total_mass, L, a.n_t, key_steps);
    unsigned long long k = live ? (unsigned long long)best_key(kc, a.rollout_id_base + b) : ~0ull;
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(k, off);
      k = o < k ? o : k;
    }
    if (threadIdx.x == 0) atomicMin((unsigned long long*)best_key_out, k);
  }
}

// ---------------------------------------------------------------------------
// Contact forces given motor torques: forcetorquesolver::solve_forces
// (ftsolver.cpp:331-378; oracle solve_forces). Least squares over the tree
// rows, the torso rows (torso force/torque forced to zero) and the torque rows
// jz_h . x_h = z_h, unknowns = non-root joint wrenches + forces of ALL feet.
// The tree rows' coefficient block is unit triangular, so eliminating the
// joint wrenches exactly leaves (Woodbury)
//   y = argmin (C y - d)^T (I + G G^T)^-1 (C y - d)
// over m = 6 + nmj rows: G = (torso, torque) rows composed with the tree
// inverse -- T_i = -[[I, 0], [[p_i - p_0]x, I]] for the torso, (u_hi, jz_h) with
// u_hi = (jpos_h - pos_i) x jz_h on the subtree of hinge h -- C = [I; [fpos -
// p_0]x] and jz_h . [(jpos_h - fpos)x] (the tree basis seen by those rows),
// d = (torso part of x_part, z - jz . x_part). Rank-deficient normal matrix
// (a straight leg): HS_FLAG_GENERAL and the basic solution (the dependent
// forces, in foot order, at 0: SparseQR's kind of answer, ftsolver.cpp:349-353).
// ---------------------------------------------------------------------------

__device__ inline void cross3(const real* a, const real* b, real* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// Block elimination by limbs. Every hinge is a limb link and a limb's three links are its own
// subtree (the loader's topology class), so W = I + G G^T couples motors of one limb only: ordered
// (motors, torso) it is W = [[M, W_mt], [W_tm, W_tt]] with M = diag(M_l), 3 x 3 per limb, and C's motor
// rows touch only their limb's foot. With S = W_tt - W_tm M^-1 W_mt (>= I), C~ = C_t - W_tm M^-1 C_m,
// d~ = d_t - W_tm M^-1 d_m and, per foot, B_f = C_mf^T M_l^-1 C_mf, r_f = C_mf^T M_l^-1 d_m, the normal
// equations are N y = r with N = diag(B_f) + C~^T S^-1 C~, r = r_b + C~^T S^-1 d~ (the same N as
// (L^-1 C)^T (L^-1 C) for W = L L^T). When every B_f is well conditioned (LDL^T pivots above
// kForcesBlockGuard of its diagonal), the Schur complement of diag(B_f) in the KKT system gives
//   (S + sum_f C~_f B_f^-1 C~_f^T) lam = sum_f C~_f B_f^-1 r_f - d~,   y_f = B_f^-1 (r_f - C~_f^T lam),
// a 6 x 6 system (>= I); otherwise (a straight leg: B_f singular) N is formed and factorized as a
// dense 3 nf x 3 nf Cholesky, pivot guard kFastPivotGuard: a pivot under it drops its force component
// (HS_FLAG_GENERAL, the basic solution; chol_packed), followed by one step of the corrected semi-normal
// equations, which takes the squared conditioning of N back out of the answer. Lanes: one per limb for the limb's blocks (M_l = L D L^T: every product Y_a^T D^-1 Y_b,
// Y = L^-1 [W_mt | C_m | d_m]), one per packed entry for the sums over limbs (in limb order).
constexpr real kForcesBlockGuard = HS_REAL_IS_FLOAT ? real(1e-3) : real(1e-6);
constexpr int FSUM = 27;  // packed 6 x 6 lower triangle (21) + a 6-vector

// entry e < 21 of W_tt = I + sum_{i >= 1} T_i T_i^T from s = sum r_i, Q = sum r_i r_i^T (r_i = p_i - p_0;
// T_i's torso block [[I, 0], [[r_i]x, I]]): n I; [s]x rows; (n + tr Q) I - Q
__device__ inline real wtt_entry(int e, const real* ts, int n) {
  const TriWalk<> t(e);
  const int r = t.r, c = t.c;
  if (r < 3) return (r == c) ? real(n) : real(0);
  if (c < 3) return cross_e(ts, c, r - 3);
  const int a = r - 3, b = c - 3;
  const real* q = ts + 3;  // Q00 Q11 Q22 Q01 Q02 Q12
  const real qab = (a == b) ? q[a] : q[a + b + 2];
  return ((a == b) ? real(n) + q[0] + q[1] + q[2] : real(0)) - qab;
}

// One limb's blocks of forces_solve (lane = limb), in stages both kernels share: the raw rows and M's
// LDL^T (forces_rows), the foot's C~_f / B_f / r_f (forces_foot), B_f's factor and V = L_B^-1 [C~^T | r_f]
// (forces_v). J, Z, P: the limb's three links' joint positions, axes and part positions at the centre
// sample, fp its foot, P0 the torso's position, X the links' x torque rows, zz the motors' torques.
// After forces_rows, prod(a, b) = (L^-1 R)_a^T D^-1 (L^-1 R)_b: S_l (packed lower) and e_l are prod(r, c)
// and prod(r, 9); after forces_v, vprod(a, b): K_f and q_f.
struct ForcesRows {
  real R[3][10], rdM[3];
  __device__ real prod(int a, int b) const {
    return R[0][a] * rdM[0] * R[0][b] + R[1][a] * rdM[1] * R[1][b] + R[2][a] * rdM[2] * R[2][b];
  }
};
struct ForcesV {
  real V[3][7], rdB[3];
  __device__ real vprod(int a, int b) const {
    return V[0][a] * rdB[0] * V[0][b] + V[1][a] * rdB[1] * V[1][b] + V[2][a] * rdB[2] * V[2][b];
  }
};
__device__ __attribute__((always_inline)) inline void forces_rows(ForcesRows& F, const real (&J)[3][3],
                                                                  const real (&Z)[3][3], const real (&P)[3][3],
                                                                  const real* fp, const real* P0,
                                                                  const real (&X)[3][3], const real* zz) {
  // raw rows of motor k: R[k] = (W_mt row (6), C_m row vs foot f (3), d_m (1)); M lower (k' <= k)
  real M[9];
  auto& R = F.R;
  for (int k = 0; k < 3; k++) {
    for (int c = 0; c < 10; c++) R[k][c] = 0;
    for (int c = 0; c < 3; c++) M[3 * k + c] = (c == k) ? real(1) : real(0);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {  // part p[i] lies in the subtrees of motors 0 .. i
    real ri[3], u[3][3];
    for (int t = 0; t < 3; t++) ri[t] = P[i][t] - P0[t];
#pragma unroll
    for (int k = 0; k <= i; k++) {
      real a3[3], ru[3];
      for (int t = 0; t < 3; t++) a3[t] = J[k][t] - P[i][t];
      cross3(a3, Z[k], u[k]);
      cross3(ri, u[k], ru);
      for (int c = 0; c < 3; c++) R[k][c] += -u[k][c];
      for (int c = 0; c < 3; c++) R[k][3 + c] += -(ru[c] + Z[k][c]);
#pragma unroll
      for (int k2 = 0; k2 <= k; k2++)
        M[3 * k + k2] += (u[k][0] * u[k2][0] + u[k][1] * u[k2][1] + u[k][2] * u[k2][2]) +
                         (Z[k][0] * Z[k2][0] + Z[k][1] * Z[k2][1] + Z[k][2] * Z[k2][2]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    real dd[3];
    for (int t = 0; t < 3; t++) dd[t] = J[k][t] - fp[t];
    for (int jj = 0; jj < 3; jj++) {
      real v = 0;
      for (int t = 0; t < 3; t++) v += Z[k][t] * cross_e(dd, jj, t);
      R[k][6 + jj] = v;
    }
    real t0 = 0;
    for (int t = 0; t < 3; t++) t0 += Z[k][t] * X[k][t];
    R[k][9] = zz[k] - t0;
  }
  ldl_n<3>(M, real(0), F.rdM);  // M >= I
#pragma unroll
  for (int c = 0; c < 10; c++) {  // Y = L^-1 R
    R[1][c] -= M[3] * R[0][c];
    R[2][c] -= M[6] * R[0][c] + M[7] * R[1][c];
  }
}
// C~_f (Ct), B_f raw (Bd) and its LDL^T (Bl / rdB), r_f (rb); returns whether B_f factors
__device__ __attribute__((always_inline)) inline bool forces_foot(const ForcesRows& F, const real* fp, const real* P0,
                                                                  real* Ct, real* Bd, real* Bl, real* rdB, real* rb) {
  real d[3];
  for (int t = 0; t < 3; t++) d[t] = fp[t] - P0[t];
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int jj = 0; jj < 3; jj++) {
      const real ct = (r < 3) ? ((r == jj) ? real(1) : real(0)) : cross_e(d, jj, r - 3);
      Ct[3 * r + jj] = ct - F.prod(r, 6 + jj);
    }
  Bd[0] = F.prod(6, 6); Bd[1] = F.prod(7, 6); Bd[2] = F.prod(7, 7);
  Bd[3] = F.prod(8, 6); Bd[4] = F.prod(8, 7); Bd[5] = F.prod(8, 8);
  for (int jj = 0; jj < 3; jj++) rb[jj] = F.prod(6 + jj, 9);
  Bl[0] = Bd[0]; Bl[3] = Bd[1]; Bl[4] = Bd[2]; Bl[6] = Bd[3]; Bl[7] = Bd[4]; Bl[8] = Bd[5];
  return ldl_n<3>(Bl, kForcesBlockGuard, rdB);
}
// K_f = C~ B^-1 C~^T, q_f = C~ B^-1 r_f, through V = L_B^-1 [C~^T | r_f]
__device__ __attribute__((always_inline)) inline void forces_v(ForcesV& G, const real* Ct, const real* Bl,
                                                               const real* rdB, const real* rb) {
  auto& V = G.V;
  for (int c = 0; c < 6; c++)
    for (int k = 0; k < 3; k++) V[k][c] = Ct[3 * c + k];
  for (int k = 0; k < 3; k++) V[k][6] = rb[k];
#pragma unroll
  for (int c = 0; c < 7; c++) {
    V[1][c] -= Bl[3] * V[0][c];
    V[2][c] -= Bl[6] * V[0][c] + Bl[7] * V[1][c];
  }
  for (int k = 0; k < 3; k++) G.rdB[k] = rdB[k];
}
// hs_rollout_kernel's form: S_l / e_l to fa, K_f / q_f to fb (its LDS ForceL rows)
__device__ __attribute__((always_inline)) inline bool forces_limb_block(const real (&J)[3][3], const real (&Z)[3][3],
                                                                        const real (&P)[3][3], const real* fp,
                                                                        const real* P0, const real (&X)[3][3],
                                                                        const real* zz, real* fa, real* fb, real* Ct,
                                                                        real* Bd, real* Bl, real* rdB, real* rb,
                                                                        real* dbgv = nullptr) {
  ForcesRows F;
  forces_rows(F, J, Z, P, fp, P0, X, zz);
  if (dbgv) { dbgv[0] = zz[0] - F.R[0][9]; dbgv[1] = zz[0]; dbgv[2] = X[0][0]; dbgv[3] = Z[0][0]; }
#pragma unroll
  for (int e = 0; e < 21; e++) {  // S_l = W_tm M^-1 W_mt (packed lower)
    const TriWalk<> t(e);
    fa[e] = F.prod(t.r, t.c);
  }
#pragma unroll
  for (int r = 0; r < 6; r++) fa[21 + r] = F.prod(r, 9);  // e_l = W_tm M^-1 d_m
  const bool okB = forces_foot(F, fp, P0, Ct, Bd, Bl, rdB, rb);
  if (okB) {
    ForcesV G;
    forces_v(G, Ct, Bl, rdB, rb);
#pragma unroll
    for (int e = 0; e < 21; e++) {
      const TriWalk<> t(e);
      fb[e] = G.vprod(t.r, t.c);
    }
#pragma unroll
    for (int r = 0; r < 6; r++) fb[21 + r] = G.vprod(r, 6);
  }
  return okB;
}

template <class W, class SV>
__device__ __attribute__((always_inline)) inline uint32_t forces_solve(const hs_topo* T, SV& sv, ForceL& fr, const W& w,
                                                                       const real* z, bool dense, int lane) {
  const int n = T->n, nl = T->n_limbs, nq = 3 * T->nf;
  const real* P0 = w.pos(0, 0);
  real* ts = sv.y;  // the 9 part sums until y is written
  if (lane < 9) {   // s (3), Q (6)
    const int a = lane < 3 ? lane : (lane < 6 ? lane - 3 : (lane == 6 ? 0 : (lane == 7 ? 0 : 1)));
    const int b = lane < 6 ? (lane < 3 ? -1 : lane - 3) : (lane == 6 ? 1 : 2);
    real s = 0;
    for (int i = 1; i < n; i++) {
      const real* Pi = w.pos(0, i);
      const real ra = Pi[a] - P0[a];
      s += (b < 0) ? ra : ra * (Pi[b] - P0[b]);
    }
    ts[lane] = s;
    if (lane == 3) DBG(0, s, 30);
  }
  // per limb: C~_f (6 x 3), B_f (raw and LDL^T), r_f stay in registers to the end
  real Ct[18], Bd[6], Bl[9], rdB[3], rb[3];
  int f = 0;
  bool okB = true;
  if (lane < nl) {
    const int L = lane;
    int p[3];
    for (int k = 0; k < 3; k++) p[k] = T->limb_node[L][k];
    f = T->node[p[2]].foot;
    real J[3][3], Z[3][3], P[3][3], X[3][3], zz[3];
    for (int k = 0; k < 3; k++) {
      for (int t = 0; t < 3; t++) {
        J[k][t] = w.jpos(0, p[k])[t];
        Z[k][t] = w.jz(0, p[k])[t];
        P[k][t] = w.pos(0, p[k])[t];
        X[k][t] = sv.x[3 * n + 3 * p[k] + t];
      }
      zz[k] = z[T->node[p[k]].hinge];
    }
#ifdef HS_DBG
    real dbgv[4] = {0, 0, 0, 0};
    okB = forces_limb_block(J, Z, P, w.fpos(0, f), P0, X, zz, fr.a[L], fr.b[L], Ct, Bd, Bl, rdB, rb, dbgv);
    DBG(24 + f, dbgv[0], 40);
    DBG(24 + f, dbgv[1], 41);
    DBG(24 + f, dbgv[2], 42);
    DBG(24 + f, dbgv[3], 43);
#else
    okB = forces_limb_block(J, Z, P, w.fpos(0, f), P0, X, zz, fr.a[L], fr.b[L], Ct, Bd, Bl, rdB, rb);
#endif
    DBG(24 + f, fr.a[L][0], 31);
    DBG(24 + f, fr.b[L][0], 32);
    DBG(24 + f, Ct[0], 36);
    DBG(24 + f, rb[0], 37);
    DBG(24 + f, fr.a[L][21], 38);
  }
  const bool fast = !dense && half_ballot(lane < nl && !okB) == 0;
  wave_sync();
  STAMP(4);
  if (lane < FSUM) {  // sums over the limbs, in limb order; W_tt and the torso part of d added
    real s = 0;
    for (int L = 0; L < nl; L++) s += fast ? ((lane < 21) ? fr.b[L][lane] - fr.a[L][lane] : fr.b[L][lane] + fr.a[L][lane])
                                          : fr.a[L][lane];
    const real dt = (lane < 21) ? real(0) : (lane < 24 ? sv.x[lane - 21] : sv.x[3 * n + lane - 24]);
    // fast: K = W_tt - sum S_l + sum K_f, rhs = sum (q_f + e_l) - d_t; else S = W_tt - sum S_l, d~ = d_t - sum e_l
    const real v = (lane < 21) ? (fast ? wtt_entry(lane, ts, n) + s : wtt_entry(lane, ts, n) - s)
                               : (fast ? s - dt : dt - s);
    fr.a[0][lane] = v;  // lane reads column `lane` only, so slot 0 takes the sums in place
    if (lane == 0) DBG(1, v, 33);
  }
  wave_sync();
  STAMP(5);
  uint32_t flags = 0;
  if (fast) {
    real K[36], rd[6], lam[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
      for (int c = 0; c < 6; c++) K[6 * r + c] = (c <= r) ? fr.a[0][pk(r, c)] : real(0);
      lam[r] = fr.a[0][21 + r];
    }
    ldl_n<6>(K, real(0), rd);  // >= I
    ldl_solve_n<6>(K, rd, lam);
    if (lane == 0) DBG(2, lam[0], 34);
    if (lane < nl) {  // y_f = B_f^-1 (r_f - C~_f^T lam)
      real t[3];
      for (int k = 0; k < 3; k++) {
        real s = rb[k];
        for (int r = 0; r < 6; r++) s -= Ct[3 * r + k] * lam[r];
        t[k] = s;
      }
      ldl_solve_n<3>(Bl, rdB, t);
      DBG(24 + f, t[0], 35);
      for (int k = 0; k < 3; k++) sv.y[3 * f + k] = t[k];
    }
    wave_sync();
    STAMP(9);
    return flags;
  }
  // dense normal equations over the feet (a B_f near singular): N = diag(B_f) + V^T D_S^-1 V with
  // S = L_S D_S L_S^T, V = L_S^-1 C~, r = r_b + V^T D_S^-1 L_S^-1 d~
  real* const base = &fr.a[0][0];
  real* const Vm = base + FSUM;       // [6][HS_KMAX]
  real* const vv = Vm + 6 * HS_KMAX;  // 6
  real* const rdS = vv + 6;           // 6
  real* const N = rdS + 6;            // packed lower, nq x nq
  real* const rr = N + HS_KMAX * (HS_KMAX + 1) / 2;
  {
    real S[36], rd[6], v6[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
      for (int c = 0; c < 6; c++) S[6 * r + c] = (c <= r) ? base[pk(r, c)] : real(0);
      v6[r] = base[21 + r];
    }
    ldl_n<6>(S, real(0), rd);  // >= I
    for (int i = 0; i < 6; i++) {
      real s = v6[i];
      for (int k = 0; k < i; k++) s -= S[6 * i + k] * v6[k];
      v6[i] = s;
    }
    if (lane < nl) {
      for (int jj = 0; jj < 3; jj++) {
        real col[6];
        for (int i = 0; i < 6; i++) {
          real s = Ct[3 * i + jj];
          for (int k = 0; k < i; k++) s -= S[6 * i + k] * col[k];
          col[i] = s;
        }
        for (int i = 0; i < 6; i++) Vm[i * HS_KMAX + 3 * f + jj] = col[i];
      }
    }
    if (lane == 0)
      for (int i = 0; i < 6; i++) {
        vv[i] = v6[i];
        rdS[i] = rd[i];
      }
  }
  wave_sync();
  for (TriWalk<1> t(lane); t.r < nq; t.next()) {  // V^T D^-1 V and its rhs, entry by entry
    const int p = t.r, q = (t.c == p + 1) ? nq : t.c;
    real s = 0;
    for (int k = 0; k < 6; k++) s += Vm[k * HS_KMAX + p] * rdS[k] * ((q < nq) ? Vm[k * HS_KMAX + q] : vv[k]);
    if (q < nq) N[pk(p, q)] = s;
    else rr[p] = s;
  }
  wave_sync();
  if (lane < nl) {  // + the feet's own blocks
    const int q0 = 3 * f;
    N[pk(q0, q0)] += Bd[0];
    N[pk(q0 + 1, q0)] += Bd[1];
    N[pk(q0 + 1, q0 + 1)] += Bd[2];
    N[pk(q0 + 2, q0)] += Bd[3];
    N[pk(q0 + 2, q0 + 1)] += Bd[4];
    N[pk(q0 + 2, q0 + 2)] += Bd[5];
    for (int k = 0; k < 3; k++) rr[q0 + k] += rb[k];
  }
  wave_sync();
  bool rank_near = false;  // a rank decision within kNearBand of the guard (HS_FLAG_NEAR_RANK)
  const uint32_t dropped = chol_packed(N, nq, kFastPivotGuard, lane, rank_near);
  if (dropped) flags = HS_FLAG_GENERAL | HS_FLAG_DEPENDENT;  // least squares not unique: its basic solution
  if (rank_near) flags |= HS_FLAG_NEAR_RANK;
  STAMP(8);
  // the two triangular solves with the vector in registers (nq <= HS_KMAX): y = N^-1 rr (add = false), or
  // y += N^-1 rr, a correction
  auto solve_kept = [&](bool add) {
    real yv[HS_KMAX];
#pragma unroll
    for (int i = 0; i < HS_KMAX; i++) yv[i] = (i < nq) ? rr[i] : real(0);
#pragma unroll
    for (int i = 0; i < HS_KMAX; i++) {
      if (i < nq) {
        real s = yv[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= N[pk(i, k)] * yv[k];
        yv[i] = ((dropped >> i) & 1) ? real(0) : s / N[pk(i, i)];
      }
    }
#pragma unroll
    for (int i = HS_KMAX - 1; i >= 0; i--) {
      if (i < nq) {
        real s = yv[i];
#pragma unroll
        for (int k = i + 1; k < HS_KMAX; k++)
          if (k < nq) s -= N[pk(k, i)] * yv[k];
        yv[i] = ((dropped >> i) & 1) ? real(0) : s / N[pk(i, i)];
      }
    }
#pragma unroll
    for (int i = 0; i < HS_KMAX; i++)
      if (i < nq) sv.y[i] = add ? sv.y[i] + yv[i] : yv[i];
  };
  if (lane == 0) solve_kept(false);
  wave_sync();
  // One step of the corrected semi-normal equations. N = G^T G for G = [D_M^-1/2 Y_f per limb; D_S^-1/2 V], the
  // least squares min |G y - g| with g = [D_M^-1/2 Y_d; D_S^-1/2 L_S^-1 d~]: forming N squares G's conditioning, so
  // y above carries cond(N) eps. The residual g - G y from G's own entries (Y = L_M^-1 [C_m | d_m] recomputed from
  // the limb's rows, V and L_S^-1 d~ as stored) costs no such squaring, and y += N^-1 G^T (g - G y) leaves
  // cond(G) eps, as a QR of the system would, while cond(N) eps < 1. A dropped component stays 0.
  {
    real gl[3] = {0, 0, 0};
    if (lane < nl) {
      int p[3];
      for (int k = 0; k < 3; k++) p[k] = T->limb_node[lane][k];
      real J[3][3], Z[3][3], P[3][3], X[3][3], zz[3];
      for (int k = 0; k < 3; k++) {
        for (int t = 0; t < 3; t++) {
          J[k][t] = w.jpos(0, p[k])[t];
          Z[k][t] = w.jz(0, p[k])[t];
          P[k][t] = w.pos(0, p[k])[t];
          X[k][t] = sv.x[3 * n + 3 * p[k] + t];
        }
        zz[k] = z[T->node[p[k]].hinge];
      }
      ForcesRows F;
      forces_rows(F, J, Z, P, w.fpos(0, f), P0, X, zz);
      real e[3];
      for (int k = 0; k < 3; k++) {
        real s = F.R[k][9];
        for (int jj = 0; jj < 3; jj++) s -= F.R[k][6 + jj] * sv.y[3 * f + jj];
        e[k] = F.rdM[k] * s;
      }
      for (int jj = 0; jj < 3; jj++) gl[jj] = F.R[0][6 + jj] * e[0] + F.R[1][6 + jj] * e[1] + F.R[2][6 + jj] * e[2];
    }
    real u[6];  // D_S^-1 (L_S^-1 d~ - V y), by every lane
    for (int k = 0; k < 6; k++) {
      real s = vv[k];
      for (int q = 0; q < nq; q++) s -= Vm[k * HS_KMAX + q] * sv.y[q];
      u[k] = rdS[k] * s;
    }
    for (int q = lane; q < nq; q += HALF) {
      real s = 0;
      for (int k = 0; k < 6; k++) s += Vm[k * HS_KMAX + q] * u[k];
      rr[q] = s;
    }
    wave_sync();
    if (lane < nl)
      for (int k = 0; k < 3; k++) rr[3 * f + k] += gl[k];
    wave_sync();
    if (lane == 0) solve_kept(true);
  }
  wave_sync();
  STAMP(9);
  return flags;
}

}  // namespace
