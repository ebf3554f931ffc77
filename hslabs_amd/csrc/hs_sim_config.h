// hs_sim_config.h -- visualizer::get_ode_config (visualization.cpp:378-396) on a simulated world: the
// inverse of hs_sim_reset's pose construction. Included by hs_sim_kernel.h: the PROBE instantiations' tail
// and hs_sim_config (hs_sim_probe.hip) share these functions, so the two agree bitwise on the same body
// state. Like the kernel they are local to the unit that includes them.
#pragma once
#include "hs_internal.h"
#include "hs_math.h"
#include "hs_ode.h"

namespace {

// A body array [n_parts][HS_SIM_BODY] seen the way hinge_angle reads the kernel's LDS world (s.q[part])
template <class Real>
struct BodyView {
  using real = Real;
  struct Quats {
    const Real* base;
    __device__ const Real* operator[](int p) const { return base + (size_t)p * HS_SIM_BODY + 3; }
  } q;
};

// Torso part of the configuration: C = A_ground(root joint)^-1 . A_ground_body_from_odebody . A_pj_body^-1
// (visualization.cpp:382-389), with A_ground_body_from_odebody = [R(q) | pos] . A_body_geom^-1
// (visualization.cpp:608-631; the body's rotation is dQtoR of its quaternion, as dxStepBody leaves it).
// Translation -> out[0:3], euler_angles_from_affine -> out[3:6]. Computed in double whatever the
// state's precision (the pose of a float state is built in double and rounded once, like the reset).
template <class IO>
__device__ inline void torso_config(const hs_topo* T, const hs_aff34& body_geom, const IO* pos, const IO* q, IO* out) {
  using namespace hsd;
  const double qd[4] = {(double)q[0], (double)q[1], (double)q[2], (double)q[3]};
  double R[12];
  hsode::q_to_R(qd, R);
  A34 A;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) A.at(r, c) = R[r * 4 + c];
    A.at(r, 3) = (double)pos[r];
  }
  const hs_node& nd = T->node[0];
  A34 unity;
  for (int i = 0; i < 12; i++) unity.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
  const A34 JA = mul(unity, load34(nd.J_A_parent));       // the root joint's A_ground, as the reset forms it
  const A34 Ab = mul(A, invert(load34(body_geom)));       // get_A_ground_body_from_odebody
  const A34 C = mul(mul(invert(JA), Ab), invert(load34(nd.A_pj_body)));  // C.mult(A); C.mult(B)
  double ang[3];
  euler_from(C, ang);
  for (int i = 0; i < 3; i++) {
    out[i] = (IO)C(i, 3);
    out[3 + i] = (IO)ang[i];
  }
}

}  // namespace
