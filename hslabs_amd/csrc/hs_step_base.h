// hs_step_base.h -- what both step kernels (hs_rollout_kernel.h, hs_limb.h) are built on: the per-precision
// and occupancy constants, the LDS layouts and global workspaces, the wave-level synchronisation and the
// diagnostic builds' stamp / debug tables.
//
// Included by the two units of the step kernels, hs_kernels.hip (fp64) and hs_kernels_f32.hip (fp32: HS_REAL
// and HS_REAL_IS_FLOAT set before the first include). Everything sits in an anonymous namespace: `real` and
// with it every layout and kernel here differ between the two units, so each keeps its own copy.
//
// LDS layout (PostL, round 5): a launch solves one step per rollout, so the
// five stencil samples keep only what that step reads -- pos/ust at t-2dt, t,
// t+2dt, q at t-dt..t+dt, joint/foot features at t -- and once D has consumed
// the stencil, the particular solution x, the closed-form blocks and the forces
// y live in its place: 5.1 KB per hexapod rollout, 10.1 KB per workgroup, 16
// workgroups per CU = 4 waves/SIMD for the fused step launch. A horizon H > 1
// is H steps (hs_capi.cpp), each recomputing its window on 30 lanes: the
// sampler is latency-bound, and a ring of five full samples (26 KB per
// rollout) measured half the throughput.
//
// The floating-point operation sequences follow oracle/hs_oracle.cpp's fast mode
// (built with -ffp-contract=off like the reference's x86-64 g++ -O2), but the two
// units are compiled with -ffp-contract=fast-honor-pragmas (hslabs_amd/build.py):
// a*b+c is one FMA except where `#pragma clang fp contract(off)` says otherwise
// (work_add: work_over_period's two roundings), so results differ from the
// oracle by FMA roundings (<= 2.3e-12 on the per-joint torques,
// profiles/r01_parity_report.txt) and by ULPs of the device
// sin/cos/atan2/acos/asin.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <type_traits>

#ifndef HS_REAL_IS_FLOAT
#define HS_REAL_IS_FLOAT 0
#endif
#include "hs_internal.h"
#include "hs_math.h"

namespace {

using namespace hsd;

// Measured per precision (interleaved A/B, one box): fp32 configs[2] (spider, curved synthetic gaits)
// 370 -> 383 M steps/s with both; fp64 hexapod -5 % with the LDS copy (straight waves included),
// -0.8 % at K = 200 without the preload
#ifndef HS_CURVED_LDS
#define HS_CURVED_LDS HS_REAL_IS_FLOAT  // waves with a turning gait copy the setup record to LDS
#endif
#ifndef HS_PRELOAD
#define HS_PRELOAD (!HS_REAL_IS_FLOAT)  // straight_preload at wave start (0: inside the straight branch)
#endif
#ifndef HS_KTE_PRELOAD
// the IK table row loaded at wave start, before the gait is known to be straight (fp64: +1.3 % at
// K = 200 on hexapod); in the fp32 build inside the straight branch (spider, whose synthetic gaits are
// curved, 346 -> 370 M steps/s: the row's registers stay out of the turning path)
#define HS_KTE_PRELOAD (!HS_REAL_IS_FLOAT)
#endif

constexpr int WAVE = 64;
constexpr int HALF = 32;     // lanes per rollout: two rollouts per wavefront
constexpr int NS = 5;        // samples in the derivative stencil (periodic.cpp:192-202)
static_assert(NS * HS_LMAX <= HALF && 6 + HS_NMAX <= HALF && HS_KMAX <= HALF, "a rollout's lane maps exceed 32");
#ifndef HS_MIN_WAVES
// fp64: <= 168 VGPRs: the per-step launch (its general path called out of line, scratch frame) and the
// fixup launch; 4 waves/SIMD measured 7-10 % slower for the per-step launch (profiles/r05_s4_ab.txt)
#define HS_MIN_WAVES 3
#endif
#ifndef HS_MIN_WAVES_DEFER
// the fused step launch (FIX_DEFER: no general-path call) at 4 waves/SIMD: 128 VGPRs, its spills (52 B)
// all in the two-contact 6 x 6 system (tools/spill_lines.py; the entry's 108 B of round 5's first 4-wave
// build were removed, DESIGN.md section 4 Registers); the PostL layout's 10.1 KB of LDS per hexapod
// workgroup fits 16 workgroups/CU. Same box, interleaved: driver command 286.4 -> 296.2 M steps/s,
// K = 200 365.8 -> 381.9 M (profiles/r05_s4_ab.txt)
#define HS_MIN_WAVES_DEFER 4
#endif
#ifndef HS_MIN_WAVES_FORCES
#define HS_MIN_WAVES_FORCES 3  // solve_forces mode (hs_run_forces): the control step's LDS layout
#endif
#ifndef HS_MIN_WAVES_F32
#define HS_MIN_WAVES_F32 4  // fp32: 5.5 KB LDS per hexapod workgroup; the per-step and fixup launches 128 VGPRs
#endif
#ifndef HS_MIN_WAVES_F32_DEFER
// fp32's fused step launch at 5 waves/SIMD: 95 VGPRs, its 84 B of spills in the two-contact path only
// (tools/spill_lines.py --file hs_kernels_f32.hip); same box against 4: configs[2] 551 -> 606 M steps/s,
// hexapod fp32 K = 200 522 -> 570 M (profiles/r05_s11_ab.txt). At 6 (80 VGPRs) the entry and the outputs
// spill and it is no faster
#define HS_MIN_WAVES_F32_DEFER 5
#endif

// ---------------------------------------------------------------------------
// LDS layouts
// ---------------------------------------------------------------------------
// NM = part capacity of the LDS layouts (the host picks the smallest instantiation >= n,
// so LDS per rollout follows the model: hexapod 5.1 KB in the PostL layout).

// packed per-contact Schur entries: the lower triangle of S_c row by row (r (r + 1) / 2 + q), then h_c
constexpr int SCH_H = 21, SCH_N = 27;
__host__ __device__ constexpr int sch_lower(int r, int q) { return r * (r + 1) / 2 + q; }

struct SchurL {  // Schur complement of the contacts (all D_c invertible)
  real Dinv[HS_LMAX][9];
  real Ssum[SCH_N];  // sum over contacts of the packed [S_c | h_c] (summed across the contact lanes)
  real lam[6];
};

// augmented system K = D + rho A^T A (tier 2: a singular D_c); rare, so it lives in the rollout's
// global workspace (aliasing the general path's, which runs only after it declines)
struct AugL {
  real K[HS_KMAX * HS_KMAX], X[HS_KMAX * 7], St[36], lam[6], rdiag[HS_KMAX];
  int ok;
};

struct FastL {  // blocks of the closed-form solve
  real d0[HS_LMAX][3];  // A_c = [-I; [d0_c]x] (d0_c = torso COM - contact foot), kept as d0_c
  real D[HS_LMAX][9], g[HS_LMAX][3];
  int ok[HS_LMAX];
  SchurL sc;
};

struct WorkL {  // per-joint positive work of the step (outputs phase; FastL is dead by then)
  real wd[HS_NMAX];
};

// Workspace of the general path (k x k matrices, leading dimension LD >= k).
// SHARED: in LDS; otherwise (GenWS, the only instance) one global-memory slot per rollout.
// The path computes in double in both builds (greal): in single precision FullPivLU's rank test
// (pivots against eps * k) and ColPivQR's nonzero-pivot rule would decide on float rounding of the
// Grams -- a third of the fp32 hexapod steps sat within the HS_FLAG_NEAR_RANK band (round 4) --
// while the Grams of float inputs formed in double keep the exact rank structure (A^T A of a 6 x k A
// has rank <= 6 to double rounding), so the decisions are the fp64 path's. Only the inputs (positions,
// axes, the particular solution) are float there, and the forces are rounded to float once.
using greal = double;
// Eigen's epsilon / min and ftsolver.cpp:228-232's loop tolerance
constexpr greal gEps = DBL_EPSILON;
constexpr greal gTiny = DBL_MIN;
constexpr greal gRelTol = 1e-6;
// the conditioning test: the last pass's second-stage system with a kept ColPivQR pivot under gCondQR of
// its first (condition above 1e7): rounding-level changes of the inputs move the answer by more than the
// parity bound there (oracle NearTrack::ill)
constexpr greal gCondQR = 1e-7;
template <int LD_, bool SHARED_>
struct GenMats {
  static constexpr int LD = LD_;
  static constexpr bool SHARED = SHARED_;
  greal ntn0[LD * LD], lu[LD * LD], Ny[LD * LD], qr[LD * LD];
  greal n1[LD / 3][9];  // 3x3 diagonal blocks of the first-order Gram (column-major)
  greal ntx0[LD], ntx1[LD], y0[LD], b[LD], z[LD], c[LD], hc[LD], nu[LD], nd[LD];
  greal u1[3][LD];  // torso rows of N in the first-order stage (switch_torso_penalty other than (1,1))
  int coupled;     // u1 is set: the first-order Gram couples the contacts
  int8_t rowsT[LD], colsT[LD], q[LD], piv[LD], rycol[LD], cperm[LD];
};
using GenWS = GenMats<HS_KMAX, false>;
// A rollout's global solve workspace: tier 2's augmented system (fast_solve) or the Eigen-style path's
// matrices. Tier 2 runs first and the general path only after it declined; each writes every entry it
// reads before reading it, so the members never carry values from one to the other.
union SolveWS {
  GenWS gen;
  AugL aug;
};

template <int NM>
struct StencilL {  // fields only the finite differences read
  real pos[2][NM][3];  // t-2dt, t+2dt
  real ust[3][NM][3];  // t-2dt, t, t+2dt
};

template <int NM>
struct CentreL {  // fields read after D
  real pos[NM][3], jpos[NM][3], jz[NM][3], fpos[HS_LMAX][3];
  real q[3][6 + 3 * HS_LMAX];  // t-dt, t, t+dt (every hinge is a limb hinge: config_dim <= 24)
  int contact[HS_LMAX];
  int unreach[HS_LMAX];
};

struct ForceL {  // solve_forces by limbs (forces_solve): per limb S_l and e_l (a), per foot K_f and q_f
                 // (b); the dense fallback reuses the space from a[0][27] on (336 reals in all)
  real a[HS_LMAX][27];
  real b[HS_LMAX][27];
  real spare[12];
};

// What the control step keeps once D has consumed the stencil, in the stencil's place: D writes each
// part's f rows over that part's own stencil rows (every lane reads its rows before it writes, one
// wavefront in program order), the particular solution x overwrites f in place, the closed form's
// blocks and the forces y follow it (round 5: the layout that brought the step to 10 KB of LDS per
// workgroup, 4 waves per SIMD)
template <int NM>
struct PostL {
  union {
    real f[6 * NM];
    real x[6 * NM];
  };
  FastL fl;
  real y[HS_KMAX];
};

template <int NM, bool FORCES>
struct OneStore {
  union {
    StencilL<NM> sten;
    // forces-given-torques mode: its blocks (x and y stay in SolveL, which forces_solve reads with them)
    typename std::conditional<FORCES, ForceL, PostL<NM>>::type post;
  };
  CentreL<NM> c;
};

struct SetupL {
  real pos0[HS_LMAX][3];  // default foot positions, pergen order
  real ts[HS_LMAX], xs[HS_LMAX];
  real t_step, max_radius, v, dt;
  SC3 tsc;  // sin / cos of the configured torso angles (every sample of a straight gait)
};

// Straight, untransformed gaits (curvature 0, no record transform): the torso keeps its configured
// angles and moves by tv = t v along x (pergen.cpp:386-397 without the turn), and every body above
// the limbs is jointless (the loader's topology check), so the torso frame, the chain's body frames
// and each limb's hip joint frame (poslimb, lik.cpp:341-347) are a constant rotation with a
// translation affine in tv: A(t) = [R | c + tv u], u = column 0 of the torso's J_A_parent. The gait
// setup keeps them at tv = 0 (the products kin_sample forms, once per rollout instead of per sample):
// the hip frames whole, and for the torso and the chain bodies the features themselves -- a body's
// position A(t) com = (R com + c) + tv u, its rotation's skew part (constant) and its frame origin
// c + tv u -- so a sample adds tv u to two points.
// IK table entry (RolloutWS::ktab): the joint values of a limb at a sample; its unreachable-or-failed
// flag is a byte of RolloutWS::kbad (24 B entries in fp64: the table is written and read once per call)
constexpr int KT_W = 3;
// torso record row (RolloutWS::ktor), turning or transformed gaits: the torso's q6 (set_rec's position and
// Euler angles) and its frame A0 = J_A_parent free_joint(q6) A_pj_body at a sample
constexpr int KR_W = 18;
constexpr int BF_W = 9;  // a body's features at tv = 0: position R com + c, skew part of R (ust), origin c
struct KinFrames {
  real J0[HS_LMAX][12];                 // each limb's hip joint frame
  real own[HS_LMAX][HS_OWN_MAX][BF_W];  // the chain bodies each limb computes (hs_topo::limb_own)
  real torso[6];                        // the torso (node 0): position and ust (its joint frame is J_A_parent)
};
// the features of a body with frame A (node_features' pos and ust; the origin for a jointless body's jpos)
__device__ inline void store_body(const A34& A, const real* com, real* bf, int n) {
  real p[3];
  mulp(A, com, p);
  for (int i = 0; i < 3; i++) bf[i] = p[i];
  bf[3] = (A(2, 1) - A(1, 2)) / 2;
  bf[4] = (A(0, 2) - A(2, 0)) / 2;
  bf[5] = (A(1, 0) - A(0, 1)) / 2;
  if (n > 6)
    for (int i = 0; i < 3; i++) bf[6 + i] = A(i, 3);
}

template <int NM>
struct SolveXY {
  union {  // particular() overwrites each part's f with its x in place
    real f[6 * NM];
    real x[6 * NM];
  };
  real y[HS_KMAX];
};
struct SolveNone {};
template <int NM, bool FORCES>
struct SolveL {
  typename std::conditional<FORCES, SolveXY<NM>, SolveNone>::type xy;  // the control step keeps them in PostL
  int cfoot[HS_LMAX];
  uint32_t fch[HS_LMAX][2];  // hs_topo::foot_chain8, copied at the wave's start (the contact blocks' chains)
};
// The solve's LDS arrays as the phases see them (sv.f, sv.x, sv.y, sv.cfoot, sv.fch)
struct SolveRef {
  real* f;
  real* x;
  real* y;
  int* cfoot;
  uint32_t (*fch)[2];
};

template <int NM, bool FORCES>
struct Smem {
  OneStore<NM, FORCES> d;
  SolveL<NM, FORCES> sv;
#if HS_CURVED_LDS
  SetupL st;  // the setup pass's record, copied per step in waves with a curved gait
#endif
};

// Cross-lane exchange through LDS inside the single wave of a workgroup: an
// LDS-only workgroup fence (lgkmcnt, no vmcnt, so HBM stores stay in flight).
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// HS_FLAG_NEAR_RANK bands (include/hslabs.h; oracle/hs_oracle.cpp NearTrack): a decision whose value lies
// within kNearBand of its threshold (rel_error: within 10x of gRelTol; ColPivQR's squared column norms:
// within kNearBand^2) is flagged, since another rounding may take it the other way
constexpr real kNearBand = real(4);
// v is within `band` of threshold t (both positive; a NaN is not)
template <class T>
__device__ inline bool near_thr(T v, T t, T band) { return v >= t / band && v <= t * band; }

// The ABI's arrays are double*; in the fp32 build they hold floats.
__device__ inline real* outp(double* p) { return reinterpret_cast<real*>(p); }
__device__ inline const real* inp(const double* p) { return reinterpret_cast<const real*>(p); }

// The general path with a global workspace also needs its HBM stores performed.
template <class G>
__device__ inline void gsync() {
  if constexpr (G::SHARED) wave_sync();
  else __syncthreads();
}

#ifdef HS_STAMPS
// diagnostic build only: per-phase shader-clock stamps of the first 4096 rollouts
// (slots 16, 17: the constant 100 MHz clock at wave entry and exit, comparable across CUs)
__device__ unsigned long long g_stamps[4096][32];  // slots 24..31: hs_prep_kernel's
__device__ unsigned int g_stamp_base;  // row r holds block g_stamp_base + r (hs_debug_set_stamp_base)
__device__ int g_stamp_iter;  // the limb kernel's tile loop: the iteration that stamps (hs_debug_set_stamp_iter; 0: the first)
// (HS_STAMP_GATE: true but inside the limb kernel's step, where it names the step's stamp_on)
#define HS_STAMP_GATE true
#define STAMP(slot)                                                                                    \
  do {                                                                                                 \
    const unsigned r_ = blockIdx.x - g_stamp_base;                                                     \
    if (threadIdx.x == 0 && r_ < 4096u && (HS_STAMP_GATE)) g_stamps[r_][slot] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#define RSTAMP(slot)                                                                                   \
  do {                                                                                                 \
    const unsigned r_ = blockIdx.x - g_stamp_base;                                                     \
    if (threadIdx.x == 0 && r_ < 4096u) g_stamps[r_][slot] = __builtin_amdgcn_s_memrealtime();         \
  } while (0)
#else
#define STAMP(slot) do {} while (0)
#define RSTAMP(slot) do {} while (0)
#endif

// HS_DBG = n (diagnostic variant builds only): intermediate value n of every part written to g_dbg[row][slot]
// by both step kernels (the limb-lane kernel's bitwise check, tests/test_gpu_limb.py)
#ifdef HS_DBG
__device__ double g_dbg[1 << 22];
__device__ inline int* dbg_rows() {
  __shared__ int r[8];
  return r;
}
#define DBG(slot, val, n)                                                        \
  do {                                                                           \
    if (HS_DBG == (n)) {                                                         \
      const int r_ = dbg_rows()[threadIdx.x / HALF];                             \
      if (r_ >= 0 && (size_t)r_ * 32 + (slot) < (1u << 22)) g_dbg[(size_t)r_ * 32 + (slot)] = (double)(val); \
    }                                                                            \
  } while (0)
#else
#define DBG(slot, val, n) do {} while (0)
#endif

// ballot over the 32 lanes of this rollout (bit l = sub-lane l)
__device__ inline uint32_t half_ballot(bool pred) {
  return (uint32_t)(__ballot(pred) >> (threadIdx.x & HALF));
}

__device__ inline A34 node_joint_parent(const hs_topo* T, int v) { return load34(T->node[v].J_A_parent); }
__device__ inline A34 node_pj(const hs_topo* T, int v) { return load34(T->node[v].A_pj_body); }

// ---------------------------------------------------------------------------
// Sample views. k = offset from the step's centre sample (-2..2).
// ---------------------------------------------------------------------------
template <int NM, bool FORCES>
struct OneWin {
  OneStore<NM, FORCES>* d;
  __device__ bool want_pos(int k) const { return (k & 1) == 0; }
  __device__ bool want_ust(int k) const { return (k & 1) == 0; }
  __device__ bool want_q(int k) const { return k >= -1 && k <= 1; }
  __device__ bool want_centre(int k) const { return k == 0; }
  __device__ real* pos(int k, int v) const { return k == 0 ? d->c.pos[v] : d->sten.pos[k > 0][v]; }
  __device__ real* ust(int k, int v) const { return d->sten.ust[(k + 2) >> 1][v]; }
  __device__ real* q(int k) const { return d->c.q[k + 1]; }
  __device__ real* jpos(int, int v) const { return d->c.jpos[v]; }
  __device__ real* jz(int, int v) const { return d->c.jz[v]; }
  __device__ real* fpos(int, int f) const { return d->c.fpos[f]; }
  __device__ int& contact(int, int f) const { return d->c.contact[f]; }
  __device__ int& unreach(int, int L) const { return d->c.unreach[L]; }
};

// Global per-rollout workspace: the general path's scratch, and the call's gait setup record, sample
// times, straight-gait frames and IK table, stored by the call's preparation pass (hs_prep_kernel) for
// every step launch of the call.
#ifndef HS_KTAB
#define HS_KTAB 64  // table rows: the samples [ktab_lo, ktab_lo + n) a call's steps read (hs::ktab_range)
#endif
struct RolloutWS {
  SolveWS sol;
  SetupL st;
  real t_tab[HS_KTAB];  // sample times of the call's rows (sample_time): t_tab[r] = t_(ktab_lo + r)
  KinFrames kf;         // a straight gait's frames
  real ktab[HS_KTAB][HS_LMAX][KT_W];  // limb L's joint values at sample ktab_lo + r
  real ktor[HS_KTAB][KR_W];           // turning or transformed gaits: the torso at sample ktab_lo + r
  uint8_t kbad[HS_KTAB][HS_LMAX];     // 1: ktab[r][L]'s limb IK unreachable or failed
  // what the limb kernel's tile loop would form from ktab again in every step that reads a row, formed once
  // per call by the pass that writes the row (hs_prep_kernel): the motors' joint rates at an interior row c of
  // the call's range, wrap_rate(ktab[c + 1], ktab[c - 1], dt), and a row's range bit, any sincos_big(ktab[r])
  real kvel[HS_KTAB][HS_LMAX][KT_W];
  uint8_t kbig[HS_KTAB][HS_LMAX];
};
static_assert(sizeof(SetupL) % sizeof(real) == 0, "SetupL is copied as reals");

// A fused launch's block -> (local step, batch wavefront): groups of kFusedGroup batch wavefronts
// (a multiple of 8, so a wavefront's steps stay on its XCD, block % 8), each group's steps in order,
// the group's wavefronts fastest. A rollout's steps then run close together in time, and its setup
// record, frames and table rows, read by every step, are fetched into the XCD's L2 once per call
// instead of once per sweep of the whole batch over a step (whose output stores evict them).
// Exception: the last group, gw = W - g0 wavefronts, is narrower when W is not a multiple of
// kFusedGroup, and when gw is not a multiple of 8 either its wavefronts change XCD from step to step
// (a locality loss only; every step is independent, outputs are unaffected). The BASELINE shapes have
// none: W = 2048 (configs[1], [4]), 8192 (configs[2]), 16384 (configs[3]'s shard)
// Both step kernels order their blocks this way (hs_rollout_kernel's wavefronts hold 2 rollouts, the limb
// kernel's 8; its groups of 128 and 64 measured the same, profiles/r06_t25_t26_group_size.txt).
constexpr int kFusedGroup = 256;
__device__ inline void fused_coords(int blk, int W, int n, int& fstep, int& wid) {
  const int q = blk / (kFusedGroup * n), g0 = q * kFusedGroup;
  const int gw = W - g0 < kFusedGroup ? W - g0 : kFusedGroup;  // the last group may be narrower
  const int r = blk - g0 * n;
  fstep = r / gw;
  wid = g0 + r % gw;
}

}  // namespace

namespace hs {

// The LDS class of a launch: the smallest part capacity NM the kernels are instantiated for that holds the
// launch's largest model (myant 17 parts, spider 19, hexapod 22), so LDS per rollout follows the model.
// f is called with NM as a compile-time constant: f(std::integral_constant<int, NM>{}).
template <class F>
inline void with_lds_class(int max_parts, F&& f) {
  if (max_parts <= 18) f(std::integral_constant<int, 18>{});
  else if (max_parts <= 22) f(std::integral_constant<int, 22>{});
  else f(std::integral_constant<int, HS_NMAX>{});
}

}  // namespace hs
