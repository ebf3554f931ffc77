// hs_colpiv.h -- Eigen 3.3's ColPivHouseholderQR for one wavefront, sized at run time, everything in LDS:
// the column-norm downdate, the nonzero-pivot rule and the solve as hs_step_solve.h's colpiv_qr / qr_solve
// restate them for the square systems of the contact solve. Used by the regression of accelerations on
// torques (hs_sim_probe.hip: rectangular, m x (nmj + 1)) and by the configuration path controller
// (hs_cpc.hip: the two square nmj x nmj systems of compute_b and B_chi_dec).
// Pivot search and Householder norm run on every lane over LDS broadcasts (wave-uniform loops): no
// single-lane loop, the shape tools/isa_check.py guards against. Reflections: lane = column; solve:
// lane = right-hand side. Both are called by all 64 lanes of a one-wavefront block.
// Bank rule (ds_read_b64: bank = (byte / 4) mod 64 within a 32-lane half): the lane = column accesses
// qr[r + lane * m] are m doubles apart, so lanes j and j' collide when (j - j') m = 0 mod 32: never for odd
// m, two-way for columns 16 apart at m = 18 and 8 apart at m = 12 (two resp. four column pairs of the
// controller's systems); the lane = right-hand side accesses C[r * nrhs + lane] are contiguous.
#pragma once
#include <cfloat>

namespace hs_colpiv {

__device__ inline void sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ColPivHouseholderQR::compute of the m x n matrix qr[r + c * m] (column-major, m >= 1, 1 <= n <= 64), in
// place: R above and on the diagonal, the essential parts of the reflections below. nu / nd / hc [n]:
// Eigen's colNormsUpdated / colNormsDirect / hCoeffs; perm [n]: column k of the factorization is column
// perm[k] of the matrix. The caller has written qr (no barrier needed after it). Returns Eigen's
// nonzeroPivots(), the count its solve uses, the same on every lane.
__device__ inline int factor(double* qr, int m, int n, double* nu, double* nd, double* hc, int* perm, int lane) {
  constexpr int WAVE = 64;
  if (lane < n) perm[lane] = lane;
  sync();
  if (lane < n) {
    double s = 0;
    for (int i = 0; i < m; i++) s += qr[i + lane * m] * qr[i + lane * m];
    nd[lane] = sqrt(s);
    nu[lane] = nd[lane];
  }
  sync();
  double mx = 0;
  for (int j = 0; j < n; j++) mx = fmax(mx, nu[j]);
  const double th = mx * DBL_EPSILON;
  const double threshold_helper = th * th / (double)m;
  const double ndt = sqrt(DBL_EPSILON);
  const int size = m < n ? m : n;  // Eigen's diagSize(): the number of reflections
  int np = size;
  for (int p = 0; p < size; p++) {
    int bi = p;
    double bv = nu[p];
    for (int j = p + 1; j < n; j++)
      if (nu[j] > bv) { bv = nu[j]; bi = j; }
    bi = __builtin_amdgcn_readfirstlane(bi);
    if (np == size && bv * bv < threshold_helper * (double)(m - p)) np = p;
    sync();
    if (bi != p) {
      for (int r = lane; r < m; r += WAVE) {
        const double t = qr[r + p * m];
        qr[r + p * m] = qr[r + bi * m];
        qr[r + bi * m] = t;
      }
      if (lane == 0) {
        double t = nu[p]; nu[p] = nu[bi]; nu[bi] = t;
        t = nd[p]; nd[p] = nd[bi]; nd[bi] = t;
        const int ti = perm[p]; perm[p] = perm[bi]; perm[bi] = ti;
      }
    }
    sync();
    // makeHouseholderInPlace on column p, rows p..m-1
    const int len = m - p;
    const double c0 = qr[p + p * m];
    double tail = 0;
    for (int i = 1; i < len; i++) tail += qr[p + i + p * m] * qr[p + i + p * m];
    double tau, beta;
    if (len == 1 || tail <= DBL_MIN) {
      tau = 0;
      beta = c0;
      for (int i = 1 + lane; i < len; i += WAVE) qr[p + i + p * m] = 0;
    } else {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0) beta = -beta;
      const double den = c0 - beta;
      for (int i = 1 + lane; i < len; i += WAVE) qr[p + i + p * m] /= den;
      tau = (beta - c0) / beta;
    }
    sync();
    if (lane == 0) { qr[p + p * m] = beta; hc[p] = tau; }
    // apply to columns p+1..n-1, then downdate their norms (one column per lane)
    const int j = lane;
    if (j > p && j < n) {
      if (len == 1) {
        qr[p + j * m] *= (1 - tau);
      } else if (tau != 0) {
        double tmp = 0;
        for (int i = 1; i < len; i++) tmp += qr[p + i + p * m] * qr[p + i + j * m];
        tmp += qr[p + j * m];
        qr[p + j * m] -= tau * tmp;
        for (int i = 1; i < len; i++) qr[p + i + j * m] -= tau * qr[p + i + p * m] * tmp;
      }
      if (nu[j] != 0) {
        double temp = fabs(qr[p + j * m]) / nu[j];
        temp = (1 + temp) * (1 - temp);
        temp = temp < 0 ? 0 : temp;
        const double ratio = nu[j] / nd[j];
        const double temp2 = temp * (ratio * ratio);
        if (temp2 <= ndt) {
          double s = 0;
          for (int i = p + 1; i < m; i++) s += qr[i + j * m] * qr[i + j * m];
          nd[j] = sqrt(s);
          nu[j] = nd[j];
        } else {
          nu[j] *= sqrt(temp);
        }
      }
    }
    sync();
  }
  return __builtin_amdgcn_readfirstlane(np);
}

// ColPivHouseholderQR::solve for nrhs <= 64 right-hand sides C[r * nrhs + i] (m rows, lane i's column), in
// place: c = Q^T u (the first np reflections), R z = c. Afterwards rows k < np of C hold z[k], the
// solution's component perm[k]; the components perm[k], k >= np, are Eigen's zeros (the basic solution
// of a rank-deficient system) and are the caller's to write. No barrier inside: a lane touches its own
// column of C only, and qr / hc are read only.
__device__ inline void solve(const double* qr, int m, int np, const double* hc, double* C, int nrhs, int lane) {
  const int i = lane;
  for (int p = 0; p < np; p++) {
    const int len = m - p;
    const double tau = hc[p];
    if (i < nrhs) {
      if (len == 1) {
        C[p * nrhs + i] *= (1 - tau);
      } else if (tau != 0) {
        double tmp = 0;
        for (int r = 1; r < len; r++) tmp += qr[p + r + p * m] * C[(p + r) * nrhs + i];
        tmp += C[p * nrhs + i];
        C[p * nrhs + i] -= tau * tmp;
        for (int r = 1; r < len; r++) C[(p + r) * nrhs + i] -= tau * qr[p + r + p * m] * tmp;
      }
    }
  }
  for (int r = np - 1; r >= 0; r--) {
    if (i < nrhs) {
      double x = C[r * nrhs + i];
      for (int j = r + 1; j < np; j++) x -= qr[r + j * m] * C[j * nrhs + i];
      C[r * nrhs + i] = x / qr[r + r * m];
    }
  }
}

}  // namespace hs_colpiv
