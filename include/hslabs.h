/*
 * hslabs.h -- C ABI of the MI355X-native HSLabs control-loop path.
 *
 * Drop-in boundary for the reference's pergen -> lik -> FK -> dynrec ->
 * ftsolver -> motor-torque path. The reference exposes this path only as C++
 * classes (no FFI); each entry point below names the reference interface it
 * replaces (file:line in underactuated/HSLabs). Plain pointers and sizes only;
 * no HIP or torch types. All functions return 0 on success and a negative
 * HS_E* code on failure (never exit(), unlike lik.cpp:321-330 / pergen.cpp:12);
 * hs_last_error() returns a thread-local message for the last failure.
 *
 * Threading: a model handle is immutable after load and may be shared by
 * threads; hs_run() calls on distinct streams are independent.
 */
#ifndef HSLABS_H
#define HSLABS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HSLABS_ABI_VERSION 16

enum {
  HS_OK = 0,
  HS_E_ARG = -1,        /* bad argument / size */
  HS_E_IO = -2,         /* file not found / unreadable */
  HS_E_PARSE = -3,      /* malformed XML or config line (model.cpp:224-244, player.cpp:170-208) */
  HS_E_TOPOLOGY = -4,   /* model outside the supported topology class */
  HS_E_NOLIK = -5,      /* no limb IK variant for this model (lik.cpp:7-20) */
  HS_E_DEVICE = -6,     /* HIP runtime error */
  HS_E_NOTFOUND = -7    /* config id not present (player.cpp:243) */
};

/* Per-step flag bits (hs_run_args.flags). */
#define HS_FLAG_RANK_RETRY   1u  /* adaptive-rank loop iterated (ftsolver.cpp:208-232) */
#define HS_FLAG_FULL_RANK    2u  /* zeroth-order Gram full rank (reference asserts in its comma initializer) */
#define HS_FLAG_LOOP_EXHAUST 4u  /* rank loop reached rank 0 without converging */
#define HS_FLAG_NAN          8u  /* NaN in torques or contact forces */
#define HS_FLAG_UNREACH     16u  /* an IK target was clamped (ignore_reach, lik.cpp:250-253) */
#define HS_FLAG_NO_CONTACT  32u  /* no foot in contact (k = 0) */
#define HS_FLAG_GENERAL     64u  /* closed-form solve declined (conditioning guard): Eigen-style
                                    FullPivLU/ColPivQR path used (informational) */
#define HS_FLAG_NEAR_RANK  256u  /* a rank or routing decision of the step lay within rounding of its
                                    threshold, so another rounding (another basis, FMA contraction,
                                    the other precision) may decide it the other way: a FullPivLU pivot
                                    within 4x of the rank threshold in use (ftsolver.cpp:208-214), the
                                    threshold doubled (:212-214), rel_error in [1e-7, 1e-5] against the
                                    loop's 1e-6 (:228-232), a ColPivQR column norm within 4x of its
                                    nonzero-pivot threshold, the closed form's collinearity guard or
                                    pivot guards within 4x of theirs; the Eigen-style path's second
                                    stage ill-conditioned (a kept ColPivQR pivot under 1e-7 of the first,
                                    the parity bound); solve_forces: a normal-matrix pivot within 4x of
                                    its rank guard (ftsolver.cpp:349-353). The
                                    step's outputs are the path's answer; equality with another
                                    implementation is only expected where neither side sets this, or
                                    where the answer does not depend on the decision. */
#define HS_FLAG_DEPENDENT  512u  /* solve_forces only (hs_run_forces*), with HS_FLAG_GENERAL: the least
                                    squares is numerically rank deficient under the kernel's guard (a
                                    reduced normal-matrix pivot under 1e-10 of its largest diagonal) and
                                    the dropped force components are 0 -- the basic solution, one point
                                    of a non-unique solution set. The reference's SparseQR
                                    (ftsolver.cpp:349-353) drops a column only under
                                    20 (rows + cols) eps max |column| (~1e-12 relative, its COLAMD
                                    order), so on such steps it may keep the column and return the
                                    ill-conditioned full solution: parity is not claimed here. */

/* Gait setup of one rollout: the fields of pgsconfigparams (pergen.h:137-146),
 * same meaning and units as a pgs_config.txt line (player.cpp:170-208), plus
 * pergensetup's record transform (pergen.h:75-76). 192 bytes; the kernels read
 * the first 104 and the transform only where rec_transform_flag is set. */
typedef struct {
  double torso_pos[3];     /* "torso_pos" */
  double torso_angles[3];  /* "torso_angles" (Euler phi, theta, psi; model.cpp:45) */
  double step_duration;    /* in [0,1] (pergen.cpp:30-51) */
  double period;           /* T */
  double step_length;      /* L */
  double step_height;      /* h */
  double curvature;        /* 0 = straight (pergen.cpp:160-198) */
  double foot_shift;       /* lateral_foot_shift / radial_foot_shift value */
  int32_t foot_shift_type; /* -1 none, 0 lateral, 1 radial */
  int32_t rec_transform_flag; /* pergensetup::rec_transform_flag (pergen.cpp:206, 319): 1 = every
                                 record is transformed by rec_transform (set_rec, pergen.cpp:238) */
  double rec_transl[3];    /* rec_transform = affine_from_orientation({rec_transl, rec_eas})   */
  double rec_eas[3];       /* (set_rec_transform / set_rec_rotation, pergen.cpp:309-320)       */
  double reserved[5];
} hs_gait_params;

typedef struct hs_model_s* hs_model_t;

typedef struct {
  int32_t n_parts;     /* dynparts / model nodes (periodic.h:45) */
  int32_t nmj;         /* motor joints (model.h:114 number_of_motor_joints) */
  int32_t nfeet;       /* periodic.h:48 get_nfeet */
  int32_t config_dim;  /* model.h:125 get_config_dim */
  int32_t n_limbs;     /* liksolver::get_number_of_limbs (lik.h:48) */
  int32_t lik_kind;    /* 0 = y-x-x legs (lik.cpp:151), 1 = z-x-x legs (lik.cpp:189) */
  double total_mass;   /* periodic::get_total_mass (periodic.cpp:320) */
  double rcap;         /* liksolver::get_rcap (lik.h:50) */
} hs_model_dims;

/* Replaces kinematicmodel::load_fromxml (model.cpp:224-244) + liksolver ctor
 * (lik.cpp:7-20) + periodic::set_dynparts (periodic.cpp:34-58). The IK variant
 * is chosen by basename like lik.cpp:9-11 ("myant.xml", "hexapod.xml",
 * "spider.xml"); hs_model_load_ex(lik_variant >= 0) selects it explicitly
 * (0 = myant, 1 = hexapod, 2 = spider tables). */
int hs_model_load(const char* xml_path, hs_model_t* out);
int hs_model_load_ex(const char* xml_path, int lik_variant, hs_model_t* out);
void hs_model_free(hs_model_t model);
int hs_model_get_dims(hs_model_t model, hs_model_dims* out);

/* periodic::switch_torso_penalty -> forcetorquesolver::switch_torso_penalty (ftsolver.cpp:262-273):
 * which torso rows form the zeroth-order stage of the contact solve (penal_mask0: the torso force
 * rows with `force`, the torso torque rows with `torque`); the other torso rows join the first-order
 * stage with weight 1 (set_penal_mask1, ftsolver.cpp:291-303; set_action_penalties 239-246). Applies
 * to every later call on this model (hs_run*, hs_batch_*, and mixed plans created afterwards).
 * The default is the reference's only call, (1,1) (player.cpp:263); with another mask every step
 * takes the Eigen-style path (the closed form is the (1,1) problem's; flags carry HS_FLAG_GENERAL).
 * (0,0) is HS_E_ARG: the reference exits with "mask0 not set" (ftsolver.cpp:245). Waits for the
 * work queued on the devices that hold the model. Not concurrent with hs_run* on the same model
 * (like the reference's solver state, the setting belongs to the model): a launch issued by another
 * thread while this call runs may see the old mask on the device and the new one on the host. */
int hs_model_set_torso_penalty(hs_model_t model, int32_t force, int32_t torque);
int hs_model_get_torso_penalty(hs_model_t model, int32_t* force, int32_t* torque);

/* One model node (modelnode, model.h:64-86; kinematicmodel::get_mnode, model.h:108), nodes in XML
 * preorder (the order of mnodes, odeparts and dynparts). */
#define HS_NODE_MAX_KIDS 6
typedef struct {
  int32_t parent;     /* get_parent() index, -1 for the root */
  int32_t jtype;      /* get_joint()->get_type(): -1 no joint (ODE fixed joint), 0 free6, 1 hinge (model.h:26) */
  int32_t hinge;      /* hinge: motor index, its value at configuration index 6 + hinge; else -1 */
  int32_t foot;       /* foot index (periodic::get_nfeet order, periodic.cpp:34-58), else -1 */
  int32_t limb;       /* lik limb whose top link this node is (liklimb::child, lik.cpp:295-301), else -1 */
  int32_t n_kids;
  int32_t kids[HS_NODE_MAX_KIDS]; /* child_nodes in order (get_first_child = kids[0]) */
  double com[3];      /* odepart body position in the node frame (A_body_geom translation,
                         visualization.cpp:541-545) */
  double foot_pos[3]; /* foot: capsule end in the node frame (odepart::get_foot_pos,
                         visualization.cpp:553-568); else 0 */
  double mass;        /* dBodyGetMass (dynpart::set_inertial_params, dynrec.cpp:62-68) */
} hs_node_info;
int hs_model_get_node(hs_model_t model, int32_t i, hs_node_info* out);

/* Replaces modelplayer::get_rec_str + get_pgs_config_params (player.cpp:170-244):
 * reads line `setup_id` of a pgs_config.txt. xml_file receives the model name. */
int hs_pgs_config_read(const char* path, int setup_id, hs_gait_params* out, char* xml_file, int32_t xml_file_len);

/*
 * One batched pass of the hot path. Rollout b (0 <= b < n_rollouts) runs the
 * gait setup (pgssweeper::setup_pergen, pergen.cpp:453-507), samples the
 * trajectory at t_i = i * (period / n_t) for i = k0 .. k0+H+3 (record_trajectory,
 * periodic.cpp:77-96: pergen set_rec + lik + FK), builds dynamics records
 * (periodic.cpp:149-202, dynrec.cpp:134-224) and solves steps
 * i = k0+2 .. k0+H+1 (compute_torques_over_period, periodic.cpp:377-391).
 * With k0 = 0 and H = n_t this is exactly one reference cycle and work_cot[1]
 * is the reference COT (player.cpp:269-285).
 *
 * All arrays are DEVICE pointers on the current HIP device, row-major. Outputs
 * may be NULL. The call is asynchronous on `stream` (a hipStream_t, NULL =
 * default stream).
 */
typedef struct {
  int32_t n_rollouts;
  int32_t horizon;        /* H >= 1 */
  int32_t k0;             /* first step index (0 = reference i = 2) */
  int32_t n_t;            /* samples per period (measure_cot n_t, main.cpp:69) */
  int32_t ignore_reach;   /* liksolver::set_ignore_reach_flag (lik.cpp:142-147) */
  int32_t accumulate;     /* 1: add this call's work to work_cot[b][0] (successive H-step calls
                             then sum work in the reference's step order, periodic.cpp:291-304) */
  const hs_gait_params* params; /* [n_rollouts] */
  double* q;              /* [B][H][config_dim]: configuration at each solved sample */
  double* tau;            /* [B][H][nmj]: motor torques (periodic.cpp:328-343) */
  double* cf;             /* [B][H][3*nfeet]: contact forces (ftsolver.cpp:163) */
  double* x;              /* [B][H][6*n_parts]: joint forces/torques (ftsolver.cpp:166) */
  uint32_t* flags;        /* [B][H] */
  double* work_cot;       /* [B][2]: positive work, work/(sum m * step_length) */
  uint64_t* best_key;     /* scalar; atomically min-reduced with the rollouts' keys after the LAST
                             step of the call (hs_best_key_encode of hs_best_key_cot; needs work_cot) */
  int64_t rollout_id_base;/* global id of rollout 0 (shard offset) */
  void* stream;           /* hipStream_t */
  double* dq;             /* [B][H][config_dim]: rates at each solved sample (compute_vel_traj,
                             periodic.cpp:261-282: wrapped central difference / 2 dt) */
  int32_t precision;      /* HS_PREC_F64 (0) or HS_PREC_F32 (1, BASELINE configs[2]): with F32 the
                             arithmetic is single precision and every floating-point array of the
                             call (q, dq, tau, cf, x, work_cot; hs_pd_args; hs_run_forces' tau_in)
                             holds float (the pointer types stay double*). params stay double. */
  int32_t solve_mode;     /* HS_SOLVE_AUTO (0): the contact solve's closed form, the Eigen-style
                             path only where the minimizer is not unique; HS_SOLVE_REFERENCE (1):
                             every step through the Eigen-style FullPivLU / ColPivHouseholderQR
                             adaptive-rank loop of ftsolver.cpp:185-236 (same results where the
                             minimizer is unique; much slower; flags carry HS_FLAG_GENERAL). In
                             hs_run_forces[_calls]: every step through the dense normal equations
                             over the feet instead of the 6 x 6 system (same results) */
  int32_t key_steps;      /* control steps whose work the best key covers (0: the steps of this
                             call, i.e. H for hs_run, n_calls * H for hs_run_steps / hs_run_calls);
                             callers that accumulate work over several calls pass the total */
} hs_run_args;

#define HS_PREC_F64 0
#define HS_PREC_F32 1
#define HS_SOLVE_AUTO 0
#define HS_SOLVE_REFERENCE 1

int hs_run(hs_model_t model, const hs_run_args* args);

/* n_calls successive hs_run launches on args->stream: call c solves steps
 * k0_c = (args->k0 + c * horizon) mod n_t .. k0_c + horizon - 1, i.e. the
 * control loop marching through the gait cycle (compute_torques_over_period's
 * step order, periodic.cpp:377-391, wrapped); outputs are overwritten per call
 * and work_cot accumulates when args->accumulate is set. The best key (if
 * args->best_key) is taken once, after the last call, over the accumulated work
 * (key_steps 0 = n_calls * horizon steps). kernel_events, if not
 * NULL, holds 2 * n_calls caller-created hipEvent_t recorded immediately before
 * and after each launch (per-launch kernel timing on the launch stream). Every call
 * (hs_run, hs_run_steps, hs_run_calls, the forces and PD forms) first runs the setup
 * pass: each rollout's gait setup, a straight gait's frames and, when the steps read
 * more samples than it holds, the limb IK of those samples (before the events). */
int hs_run_steps(hs_model_t model, const hs_run_args* args, int32_t n_calls, void* const* kernel_events);

/* Position control (modelplayer::set_position_control_torques +
 * linear_feedback_control, player.cpp:388-432): for each solved step, with the
 * target state of periodic::get_motor_adas (periodic.cpp:394-404: motor angles
 * of the centre sample, rates by the wrapped central difference of
 * compute_vel_traj, periodic.cpp:261-282) and the step's computed torques as
 * feedforward (get_computed_torques),
 *   tau_cmd = tau_ff + (k1 * mod2pi(q - q0) + k2 * (dq - dq0)),
 *   k1 = -k, k2 = -2 sqrt(k), mod2pi into (-pi, pi] (arrayops::modulus).
 * The reference's step index tsi (mod n_t, lifted to [2, n_t + 1]) is the
 * centre sample: args->k0 = tsi - 2. Step h of a call is the cycle's step
 * (k0 + h) mod n_t: a call that runs past the cycle's end wraps, as tsi does
 * (hs_run's steps do not wrap: one period later a turning gait's torques are
 * not the cycle's). All arrays DEVICE, [B][H][nmj]. */
typedef struct {
  const double* q_meas;   /* measured motor angles (get_ode_motor_adas) */
  const double* dq_meas;  /* measured motor rates */
  double k;               /* position gain (player.cpp:393: 100) */
  double* tau_cmd;        /* out: feedforward + feedback */
  double* q_target;       /* out, optional: get_motor_adas angles */
  double* dq_target;      /* out, optional: get_motor_adas rates */
} hs_pd_args;
/* The n_calls control steps of hs_run_steps (call c solves steps k0_c .. k0_c + H - 1 with
 * k0_c = (k0 + c H) mod n_t) fused into few launches over (step, rollout), so the SIMDs are
 * refilled from one queue of wavefronts instead of each step ending on its batch's slowest ones.
 * Every step keeps its own output rows: q, dq, tau, cf, x, flags are [B][n_calls * H][...]
 * (row c H + h). work_cot receives the same work (summed in step order, bitwise equal to
 * hs_run_steps with accumulate) and COT; the best key is taken once, after the last step
 * (needs work_cot). Asynchronous on args->stream like hs_run. */
int hs_run_calls(hs_model_t model, const hs_run_args* args, int32_t n_calls);

int hs_run_pd(hs_model_t model, const hs_run_args* args, const hs_pd_args* pd);

/* Contact forces given motor torques: forcetorquesolver::solve_forces via
 * periodic::solve_contforces_given_torques (ftsolver.cpp:331-378,
 * periodic.cpp:368-374) for steps k0 .. k0+H-1 of every rollout. tau_in is a
 * DEVICE array [B][H][nmj]; args->cf receives the least-squares forces of ALL
 * feet (airborne ones included, contact_feet_flag = false), torso force and
 * torque forced to zero; args->q and args->flags as in hs_run (HS_FLAG_GENERAL
 * = the least squares is rank deficient, e.g. a straight leg; then the
 * Tikhonov-regularized solution is returned). tau, x, work_cot and best_key are
 * not written. */
int hs_run_forces(hs_model_t model, const hs_run_args* args, const double* tau_in);
/* n_calls calls of hs_run_forces (call horizon args->horizon, k0 marching by it), fused like
 * hs_run_calls: a setup pass stores each rollout's gait setup once, then launches of up to 512k
 * wavefronts over (step, rollout); every step S = n_calls * horizon keeps its own row. tau_in is a
 * DEVICE array [B][S][nmj], args->cf / q / flags have S rows per rollout. Outputs are bitwise those
 * of hs_run_forces with horizon S. (periodic::solve_contforces_given_torques over a trajectory,
 * periodic.cpp:368-374, as called per sample by modelplayer::test_dynamics,
 * playerexperim.cpp:95-121.) */
int hs_run_forces_calls(hs_model_t model, const hs_run_args* args, int32_t n_calls, const double* tau_in);
/* Host-buffer, synchronous form: tau_in [B][H][nmj] -> cf [B][H][3*nfeet], flags [B][H] (may be NULL). */
int hs_run_forces_host(hs_model_t model, const hs_gait_params* params, int32_t n_rollouts, int32_t n_t, int32_t k0,
                       int32_t horizon, int32_t ignore_reach, const double* tau_in, double* cf, uint32_t* flags);

/* Mixed-topology batches (BASELINE configs[4], e.g. myant + hexapod interleaved):
 * rollout b runs models[model_index[b]]. The reference runs one kinematicmodel
 * per periodic object (periodic.cpp:34-58); a plan batches several in one
 * launch. It groups each model's rollouts two per wavefront, so topology reads
 * stay wave-uniform, and is reusable across calls on the device current at
 * creation. Models must outlive the plan. model_index is a HOST array. */
typedef struct hs_mixed_s* hs_mixed_t;
int hs_mixed_create(const hs_model_t* models, int32_t n_models, const int32_t* model_index, int32_t n_rollouts,
                    hs_mixed_t* out);
void hs_mixed_free(hs_mixed_t plan);
/* Output row strides of the plan's batches = the maxima over its models:
 * tau rows hold max nmj, cf 3 * max nfeet, q max config_dim, x 6 * max n_parts
 * (the other fields of *out are those of the model with the most parts).
 * Entries past a rollout's own dimensions are written as 0. */
int hs_mixed_get_dims(hs_mixed_t plan, hs_model_dims* out);
/* hs_run / hs_run_steps over a plan (args->n_rollouts must equal the plan's). */
int hs_run_mixed(hs_mixed_t plan, const hs_run_args* args);
int hs_run_mixed_steps(hs_mixed_t plan, const hs_run_args* args, int32_t n_calls, void* const* kernel_events);
/* hs_run_calls for a mixed plan (rows with the plan's strides) */
int hs_run_mixed_calls(hs_mixed_t plan, const hs_run_args* args, int32_t n_calls);

/* Host-buffer convenience wrapper of hs_run (copies in/out, synchronous).
 * Replaces periodic::compute_torques_over_period + get_motor_torques +
 * work_over_period for a batch of rollouts. Output pointers may be NULL. */
int hs_run_host(hs_model_t model, const hs_gait_params* params, int32_t n_rollouts, int32_t n_t,
                int32_t k0, int32_t horizon, int32_t ignore_reach, double* q, double* tau, double* cf,
                double* x, uint32_t* flags, double* work_cot);

/* periodic::get_complete_traj (periodic.cpp:406-426) for a batch of rollouts
 * (synchronous, host buffers): rec[b][tsi] for tsi = 0 .. n_t-1 (tsi < 2 read
 * at tsi + n_t, like get_complete_traj_rec) = [configuration (config_dim),
 * rates (config_dim), computed torques (nmj)] -- the records
 * modelplayer::record_per_traj writes to traj.txt (player.cpp:619-629).
 * rec holds n_rollouts * n_t * (2 * config_dim + nmj) doubles. */
int hs_complete_traj(hs_model_t model, const hs_gait_params* params, int32_t n_rollouts, int32_t n_t,
                     int32_t ignore_reach, double* rec);

/* save_2d_array (core.cpp:46-61): n_rows rows of rec_len doubles, space
 * separated, default ostream formatting, appended when append != 0. */
int hs_traj_save(const char* path, const double* rec, int32_t n_rows, int32_t rec_len, int32_t append);

/*
 * Per-configuration kinematics: the kinematicmodel / pergensetup entry points every caller
 * outside periodic binds (model.h:122-130, pergen.h:68-108; player.cpp:69, 122, 354,
 * ghost.cpp:53-54, periodic.cpp:89-90), for batches of n configurations. DEVICE arrays on the
 * current HIP device, asynchronous on stream (a hipStream_t, NULL = default stream); the _host
 * forms take host arrays and are synchronous. fp64 only.
 */
/* Row length of a trajectory record: torso position and Euler angles, then the foot position of
 * every limb in lik order (liksolver::place_limbs, lik.cpp:87-99; pergensetup::set_rec,
 * pergen.cpp:220-239). = 6 + 3 * n_limbs = config_dim for the shipped models. */
#define HS_REC_LEN(dims) (6 + 3 * (dims).n_limbs)

/* pergensetup::set_rec (pergen.cpp:225-239) after pgssweeper::setup_pergen (pergen.cpp:453-507):
 * rec[b][i] = the record of rollout b's gait at time times[i] (t in the units of period), for
 * n_rollouts x n_times items. params [n_rollouts], times [n_times], rec [B][n_times][rec_len]. */
int hs_pergen_rec(hs_model_t model, const hs_gait_params* params, int32_t n_rollouts, const double* times,
                  int32_t n_times, double* rec, void* stream);
int hs_pergen_rec_host(hs_model_t model, const hs_gait_params* params, int32_t n_rollouts, const double* times,
                       int32_t n_times, double* rec);

#define HS_FLAG_LIK_FAILED 128u /* hs_model_lik status: a foot target out of reach with ignore_reach = 0
                                   (the reference prints the limb and exits, lik.cpp:321-330); the
                                   limb's angles are then NaN */
#define HS_LIK_LIMB_BIT(L) (1u << (16 + (L))) /* hs_model_lik status: limb L's target was out of reach */
/* kinematicmodel::set_jvalues_with_lik (model.cpp:354-359 -> liksolver::place_limbs,
 * lik.cpp:89-99, liklimb::place_limb / poslimb, lik.cpp:316-347): rec [n][rec_len] -> config
 * [n][config_dim] (joint values in get_jvalues order, model.cpp:368-372). Only the torso's six
 * values and the limbs' hinge values are written; other entries keep what config held (the
 * reference leaves the other joint values as they were). ignore_reach as
 * liksolver::set_ignore_reach_flag (lik.cpp:142-147): a target beyond reach is clamped to the
 * stretched limb (status HS_FLAG_UNREACH); without it status gets HS_FLAG_LIK_FAILED; either way
 * HS_LIK_LIMB_BIT(L) names the limb. status [n] may be NULL. The host form returns HS_E_ARG when any row failed (after writing all rows). */
int hs_model_lik(hs_model_t model, int32_t n, const double* rec, int32_t ignore_reach, double* config,
                 uint32_t* status, void* stream);
int hs_model_lik_host(hs_model_t model, int32_t n, const double* rec, int32_t ignore_reach, double* config,
                      uint32_t* status);

/* kinematicmodel::recompute_modelnodes (model.cpp:314-318; modelnode::recompute_A_ground,
 * model.cpp:183-201) for n configurations config [n][config_stride] (config_stride >=
 * config_dim): the ground transform of every model node, get_mnode(i)->get_A_ground()
 * (model.h:73, 108), into a_ground [n][n_parts][12], and of every node's joint,
 * get_joint()->get_A_ground() (model.h:45), into a_joint [n][n_parts][12] (may be NULL; zeros
 * for a node without a joint). Each transform is the 3x4 top of the reference's column-major 4x4
 * affine (matrix.h:27-28): element (row r, column c) at [c * 3 + r], c = 3 the translation. Node
 * order = model nodes in XML preorder (kinematicmodel::mnodes). */
int hs_model_fk(hs_model_t model, int32_t n, const double* config, int32_t config_stride, double* a_ground,
                double* a_joint, void* stream);
int hs_model_fk_host(hs_model_t model, int32_t n, const double* config, int32_t config_stride, double* a_ground,
                     double* a_joint);

/* Best-rollout key: (order-preserving bits of (float)c) << 32 | (uint32)rollout id, where c is
 * the selection COT of hs_best_key_cot. NaN maps to the largest key (never selected); ties go to
 * the lowest id. Initial value for a reduction: UINT64_MAX.
 *
 * Selection COT (a deliberate deviation from the signed COT player.cpp:269-285 prints, which
 * work_cot[1] keeps): the cost of transport of ONE gait cycle of forward or backward walking,
 *   c = work * (n_t / steps) / (total_mass * |step_length|),
 * steps = the control steps the accumulated work covers (hs_run_args.key_steps), so a key taken
 * after K != n_t steps ranks rollouts like measure_cot over one cycle would; |step_length| <
 * HS_KEY_MIN_STEP_LENGTH gives NaN (a gait that does not travel has no meaningful COT). The
 * reference only prints per-setup COTs of its sweep (player.cpp:311-321) and never selects. */
#define HS_KEY_MIN_STEP_LENGTH 1e-3
double hs_best_key_cot(double work, double total_mass, double step_length, int32_t n_t, int32_t steps);
uint64_t hs_best_key_encode(double cot, int64_t rollout_id);
void hs_best_key_decode(uint64_t key, float* cot, int64_t* rollout_id);

/*
 * Batch handle sharded over the devices of one process (SURVEY.md 8b exports 2-5): the
 * in-process counterpart of one process per GPU. Rollouts split into contiguous ranges, one per
 * device set in device_mask (bit d = HIP device d; the same ranges as hslabs_amd/dist.py shard),
 * each range run on its device's own stream with rollout_id_base = its first id. Parameters and
 * outputs live on the devices; hs_batch_run copies the requested outputs to caller-owned HOST
 * arrays laid out for the whole batch. Replaces the loop of pgssweeper::setup_pergen +
 * modelplayer::measure_cot over a parameter sweep (player.cpp:259-321).
 */
typedef struct hs_batch_s* hs_batch_t;

typedef struct {         /* host arrays, any may be NULL; float instead of double with HS_PREC_F32 */
  double* q;             /* [B][H][config_dim] */
  double* tau;           /* [B][H][nmj] */
  double* cf;            /* [B][H][3*nfeet] */
  double* x;             /* [B][H][6*n_parts] */
  uint32_t* flags;       /* [B][H] */
  double* work;          /* [B]: positive work of the run's steps (work_over_period) */
  double* cot;           /* [B]: work / (sum m * step_length) (player.cpp:269-285) */
} hs_batch_outputs;

int hs_batch_create(hs_model_t model, int32_t n_rollouts, int32_t horizon, int32_t n_t, int32_t precision,
                    uint32_t device_mask, hs_batch_t* out);
/* host params[n_rollouts] (pgsconfigparams fields, pergen.h:137-146) -> the devices' shards */
int hs_batch_set_params(hs_batch_t batch, const hs_gait_params* params);
/* steps k0 .. k0+H-1 of every rollout (hs_run semantics), synchronous; resets and refills the
 * per-device best keys */
int hs_batch_run(hs_batch_t batch, int32_t k0, int32_t ignore_reach, const hs_batch_outputs* out);
/* hs_batch_run into caller-owned DEVICE buffers (same [B] layouts; each may be on any device of the
 * process: a shard's rows are copied device-to-device, peer-to-peer when the buffer is on another
 * GPU; float arrays with HS_PREC_F32), synchronous. periodic::get_motor_torques and
 * solve_torques_contforces write caller-allocated arrays the same way (periodic.cpp:328-343). */
int hs_batch_run_device(hs_batch_t batch, int32_t k0, int32_t ignore_reach, const hs_batch_outputs* out);
/* The best-rollout reduce inside one process: minimum of the per-device keys of the last run
 * (lowest selection COT, ties to the lowest id), by host reads of the devices' 8-byte keys. */
int hs_select_best(hs_batch_t batch, float* cot, int64_t* rollout_id);
/* device pointer of the uint64 best key of the i-th device of the batch (in mask order) */
uint64_t* hs_batch_best_key_device(hs_batch_t batch, int32_t i);
void hs_batch_free(hs_batch_t batch);

/*
 * One process per GPU: the path's single collective, the best-rollout reduce, as
 * ONE RCCL all-reduce (ncclUint64, ncclMin) of the 8-byte key over xGMI. It replaces the serial
 * sweep whose minimum a caller of player.cpp:311-321 would take. The communicator spans the ranks
 * of the job, one HIP device each: rank 0 creates the id with hs_comm_unique_id, the caller
 * broadcasts its HS_COMM_ID_BYTES bytes (MPI, torch.distributed, a file ...), every rank calls
 * hs_comm_init with the device it runs on current. Rollouts are sharded in contiguous id ranges
 * (rollout_id_base), so the reduced key names the global winner.
 */
#define HS_COMM_ID_BYTES 128
typedef struct hs_comm_s* hs_comm_t;
int hs_comm_unique_id(char id[HS_COMM_ID_BYTES]);
int hs_comm_init(int32_t n_ranks, int32_t rank, const char id[HS_COMM_ID_BYTES], hs_comm_t* out);
void hs_comm_free(hs_comm_t comm);
int hs_comm_size(hs_comm_t comm, int32_t* n_ranks, int32_t* rank);
/* in-place all-reduce(MIN) of the uint64 key at key (DEVICE pointer, the comm's device), async
 * on stream (a hipStream_t, NULL = default stream) */
int hs_comm_reduce_best(hs_comm_t comm, uint64_t* key, void* stream);
/* hs_select_best across the ranks: this process's minimum over its batch's devices (the batch
 * must run on the comm's device only), all-reduced over the communicator, decoded on every rank.
 * The reduce runs in the comm's own 8-byte device buffer: the batch's per-device keys keep their
 * local values (a later hs_select_best still returns this process's minimum). Collective: every
 * rank must call it. A rank whose batch fails the checks (not run, another device, null outputs) or
 * whose local keys cannot be read back still takes part, contributing the largest key, and then
 * returns the error, so its peers complete (with the minimum over the other ranks). Two failures
 * return before the collective and leave the peers waiting: a null comm, and a HIP runtime error on
 * the comm's own device while staging the key (the communicator is unusable then). */
int hs_select_best_comm(hs_batch_t batch, hs_comm_t comm, float* cot, int64_t* rollout_id);

/*
 * Closed-loop simulation: modelplayer::simulate_ode with position control
 * (player.cpp:325-339) for a batch of independent robots, each in its own ODE
 * world as the reference sets it up (visualization.cpp:140-150: gravity 1,
 * ERP .8, a z = 0 plane; one body per part with ODE's default mass, hinge and
 * fixed joints from kinematicmodel::set_ode_joints, model.cpp:375-400). One
 * step is
 *   set_position_control_torques (player.cpp:388-432): targets and
 *     feedforward torques of the controller tables at tsi, measured hinge
 *     angles / rates (dJointGetHingeAngle/Rate), k1 = -k, k2 = -2 sqrt(k);
 *   dJointAddHingeTorque for every motor (visualization.cpp:350-356);
 *   dSpaceCollide + nearCallback (visualization.cpp:296-326): one contact per
 *     capsule / sphere touching the plane, Bounce|SoftCFM, mu = inf;
 *   dWorldQuickStep (visualization.cpp:333-337): the projected Gauss-Seidel
 *     (SOR-LCP) constraint solve, `iterations` sweeps with ODE's random
 *     reordering every 8 sweeps, then the semi-implicit body update;
 *   tsi += 1 (play_t += play_dt).
 * The ODE formulas are restated from ODE 0.13 (the reference links an
 * unpinned -lode); see DESIGN.md.
 */
#define HS_SIM_BODY_STRIDE 13 /* per part: pos[3], quaternion (w,x,y,z)[4], lvel[3], avel[3] */

typedef struct {
  double dt;          /* play_dt (player.cpp:23: 0.01) */
  double k;           /* position gain (player.cpp:393: 100); <= 0: no position control */
  double sor_w;       /* dWorldSetQuickStepW (ODE default 1.3) */
  double erp;         /* dWorldSetERP (visualization.cpp:146: 0.8) */
  double cfm;         /* global CFM (ODE double-precision default 1e-10) */
  double gravity;     /* visualization.cpp:144: 1 */
  double bounce;      /* nearCallback surface (visualization.cpp:310-320): .5 */
  double bounce_vel;  /* .1 */
  double soft_cfm;    /* .001 */
  double mu;          /* dInfinity */
  int32_t iterations; /* dWorldSetQuickStepNumIterations (ODE default 20) */
  int32_t reserved;
} hs_sim_params;

/* The reference's values (above). */
void hs_sim_default_params(hs_sim_params* p);

/* init_play_config (player.cpp:351-356) + orient_odebodys (model.cpp:295-305):
 * body states of B configurations (joint values, config [B][config_stride],
 * DEVICE), zero velocities. body: DEVICE [B][n_parts][HS_SIM_BODY_STRIDE].
 * precision HS_PREC_F32: config and body hold floats (the pose is built in
 * double and rounded once). */
int hs_sim_reset(hs_model_t model, int32_t n_rollouts, const double* config, int32_t config_stride, double* body,
                 int32_t precision, void* stream);

typedef struct {
  int32_t n_rollouts;
  int32_t n_steps;         /* simulation steps of this call (one launch runs them all) */
  int32_t n_t;             /* controller table rows (setup_per_controller: int(T / play_dt + .5)) */
  int32_t precision;       /* HS_PREC_F64, or HS_PREC_F32 (BASELINE configs[2]): single-precision
                              arithmetic; body, the tables and the outputs hold floats (pointer types
                              stay double*, like hs_run_args); seed/tsi/n_contacts unchanged */
  hs_sim_params params;
  /* per-rollout state, DEVICE, read and advanced */
  double* body;            /* [B][n_parts][HS_SIM_BODY_STRIDE] */
  uint32_t* seed;          /* [B] ODE dRand state (dRandInt reshuffles of the SOR rows) */
  int32_t* tsi;            /* [B] play step index, int(play_t / play_dt + .5) */
  /* controller tables, DEVICE: exactly what hs_run writes with k0 = 0, H = n_t (row h = trajectory
     sample h + 2; get_motor_adas / get_computed_torques of tsi read row (tsi mod n_t + n_t - 2) mod n_t) */
  const double* q_tab;     /* [B][n_t][config_dim] (hs_run_args.q) */
  const double* dq_tab;    /* [B][n_t][config_dim] (hs_run_args.dq) */
  const double* tau_tab;   /* [B][n_t][nmj] (hs_run_args.tau) */
  /* optional per-step outputs, DEVICE (NULL to skip) */
  double* tau_cmd;         /* [B][n_steps][nmj] motor torques applied */
  double* q_meas;          /* [B][n_steps][nmj] hinge angles at the start of the step */
  double* torso;           /* [B][n_steps][3] root body position after the step */
  int32_t* n_contacts;     /* [B][n_steps] */
  double* normal_force;    /* [B][n_steps] sum of the contact normal constraint forces */
  void* stream;            /* hipStream_t */
} hs_sim_args;

/* n_steps closed-loop steps of every rollout, one launch (state stays on chip between steps). */
int hs_sim_step(hs_model_t model, const hs_sim_args* args);

/*
 * Batched fall test (ABI 16): the flagged pieces modelplayer::simulate_ode (player.cpp:326-340)
 * runs around the QuickStep besides position control, per rollout, in hs_sim_step's launch shape.
 * One trial step, in simulate_ode's order:
 *   torque law: open_loop != 0 -> tau = tau_tab[row(tsi)], no feedback, whatever k is
 *     (set_open_loop_torques, playerexperim.cpp:143-148); else the PD law of hs_sim_step (k > 0).
 *     q_meas is written either way;
 *   torque limit (torque_limit > 0): where |tau| > limit, tau = limit * tau / |tau|
 *     (clip_torque, player.cpp:753-762), before the torques are applied; tau_cmd records the clipped
 *     value (set_ode_motor_torques clips, applies, then saves: player.cpp:740-745);
 *   kick (kick_every > 0 and tsi % kick_every == kick_phase): the force f = kick_dv[b] / dt on the root
 *     body for this step (kick_torso, player.cpp:585-605: dBodyAddForce before the stepper,
 *     visualization.cpp:406-411; gravity is added on top). The reference's live values are
 *     kick_every 500, kick_phase 499, dv (4, 0, 0). Deviation: the reference tests
 *     int(play_t / play_dt) of an accumulated double, this library its integer tsi;
 *   fall check (fall_check, player.cpp:669-681), before the step: nothing while tsi < check_from;
 *     tsi > check_until (check_until >= 0) -> survived ("No fall by t"); else root pos[2] < hc ->
 *     fallen at this tsi ("Fall at t"). Instead of exit(1) the rollout is frozen: the step is not
 *     taken, body / seed / tsi stay as they are, its remaining per-step output rows are not
 *     written, and its wavefront ends (the slot goes to the next rollout of the grid). A rollout
 *     that enters a launch frozen does nothing;
 *   otherwise the step of hs_sim_step.
 */
#define HS_TRIAL_RUNNING (-1)
#define HS_TRIAL_SURVIVED (-2)

typedef struct {
  hs_sim_args sim;         /* as for hs_sim_step */
  int32_t open_loop;       /* != 0: feed-forward torques only */
  int32_t kick_every;      /* <= 0: no kicks */
  int32_t kick_phase;      /* in [0, kick_every) */
  int32_t check_from;      /* first tsi at which the fall check runs */
  int32_t check_until;     /* last tsi at which a fall counts; < 0: never "survived" */
  int32_t reserved;
  double torque_limit;     /* 0: no limit */
  double hc;               /* fall height of the root body */
  const double* kick_dv;   /* DEVICE [B][3] velocity change per kick; NULL = no kicks; floats with HS_PREC_F32 */
  int32_t* state;          /* DEVICE [B], read and advanced: HS_TRIAL_RUNNING, HS_TRIAL_SURVIVED, else the
                              tsi at which the rollout fell */
  double* fall_z;          /* DEVICE [B], optional: the height seen by the check that froze the rollout
                              (floats with HS_PREC_F32) */
} hs_sim_trial_args;

/* n_steps trial steps of every rollout, one launch. HS_E_ARG for a NULL state, kick_every > 0 with
 * kick_phase outside [0, kick_every) or a NULL kick_dv, torque_limit < 0, open_loop without tables,
 * and everything hs_sim_step rejects. */
int hs_sim_trial(hs_model_t model, const hs_sim_trial_args* args);

typedef struct {
  int32_t running, survived, fallen;
  int32_t min_fall_tsi;    /* -1 when nothing fell */
  int64_t sum_fall_tsi;
} hs_trial_summary;

/* Tally of state [n] (DEVICE) into *out_host (HOST); one reduction launch on stream, synchronous. */
int hs_sim_trial_summary(const int32_t* state, int32_t n, hs_trial_summary* out_host, void* stream);

/*
 * Dynamics from simulation (additive exports: HSLABS_ABI_VERSION stays 16, no existing layout or
 * meaning changes): modelplayer::estimate_B_by_regression (player.cpp:548-582), the first line of
 * simulate_ode when dynamics_from_simulation_flag is set (player.cpp:327), for every rollout of a batch.
 * The m one-step probe simulations of a rollout, which the reference runs one after another from a
 * saved odestate, are m wavefronts of one launch. All arrays are DEVICE arrays; with HS_PREC_F32 the
 * double* arrays hold floats, as in hs_sim_args.
 */

/* visualizer::get_ode_config (visualization.cpp:378-396) of n body states: torso translation ->
 * config[0:3], euler_angles_from_affine of the torso pose -> config[3:6], dJointGetHingeAngle of every
 * motor in motor order -> config[6:]. The inverse of hs_sim_reset. body [n][n_parts][HS_SIM_BODY_STRIDE],
 * config [n][config_stride]. Deviation: the rotation of a body is dQtoR of its quaternion, also for a
 * state that was just reset (ODE keeps the matrix dBodySetRotation was given until the first step). */
int hs_sim_config(hs_model_t model, int32_t n, const double* body, double* config, int32_t config_stride,
                  int32_t precision, void* stream);

/* configtimedertrack(2, config_dim, dt)::push_config (odestate.cpp:105-119) of n trackers:
 * ders [n][3][config_dim] = configuration, first and second backward difference, read and advanced.
 * Level by level: subtract, then multiply by (1./dt). A tracker starts as zeros (odestate.cpp:93), so its
 * first push yields config / dt as "velocity", like the reference; angles are not wrapped, like the
 * reference. HS_PREC_F64 only (HS_E_ARG otherwise): the second difference divides rounding by dt^2. */
int hs_sim_track_push(hs_model_t model, int32_t n, const double* config, int32_t config_stride, double dt,
                      double* ders, int32_t precision, void* stream);

/* The probe loop of estimate_B_by_regression (player.cpp:563-577). Probe j of rollout b starts from
 * body[b] (read only: odestate::save / load), applies tau0[b] + dtau[b][j] as
 * visualizer::set_ode_motor_torques does (no PD, no clip, no kick, no fall check), and takes one step of
 * hs_sim_step's simulation. The perturbations are the caller's (the reference draws them with libc's
 * rand(), player.cpp:567, which is not restated; hslabs_amd.synth.gen_torque_perturbations draws from the
 * same distribution). dRand: odestate does not hold ODE's stream, so the reference's probes consume it in
 * turn; probe j starts from seed[b] advanced by j steps' worth of draws (every probe of a rollout has the
 * same contact set, hence the same number of draws), and seed[b] after the call is the seed after m probes. */
typedef struct {
  int32_t n_rollouts;
  int32_t m;               /* probes per rollout; the reference's is config_dim + 20 */
  int32_t precision;       /* HS_PREC_F64 or HS_PREC_F32 */
  int32_t reserved;
  hs_sim_params params;
  const double* body;      /* [B][n_parts][HS_SIM_BODY_STRIDE], read only */
  uint32_t* seed;          /* [B], read and advanced */
  const double* tau0;      /* [B][nmj] last motor torques; NULL = zeros */
  const double* dtau;      /* [B][m][nmj] perturbations */
  double* config_out;      /* [B][m][config_dim] hs_sim_config of the stepped probe */
  double* tau_out;         /* [B][m][nmj] torques applied, tau0 + dtau */
  double* body_out;        /* optional [B][m][n_parts][HS_SIM_BODY_STRIDE] */
  int32_t* n_contacts;     /* optional [B][m] */
  void* stream;            /* hipStream_t */
} hs_sim_probe_args;

/* One launch of B * m wavefronts. HS_E_ARG for a NULL body, seed, dtau, config_out or tau_out, m < 0,
 * and the parameter checks of hs_sim_step. m == 0 does nothing. */
int hs_sim_probe(hs_model_t model, const hs_sim_probe_args* args);

/* B_from_T_U (player.cpp:531-546) per rollout: A = [T^T | 1] (m x (nmj + 1)), Eigen 3.3
 * ColPivHouseholderQR, B.row(i) = solve(U.row(i)^T) for the config_dim right-hand sides,
 * Bt[b][j][:] = B.col(j) for j < nmj (the constant column is dropped). T [B][m][nmj], U [B][m][config_dim],
 * Bt [B][nmj][config_dim], rank [B] = the nonzero pivots the solve used. m == 0: set_Bt_unity
 * (player.cpp:522-529), rank 0. HS_E_ARG for NULL arrays, m < 0, HS_PREC_F32, a system too large for
 * the kernel's 64 KB of LDS, and 0 < m < nmj + 1. Deviation: for the latter the reference returns Eigen's
 * rank-deficient basic solution, which is not pinned here. */
int hs_sim_regress_B(hs_model_t model, int32_t n, int32_t m, const double* T, const double* U, double* Bt,
                     int32_t* rank, int32_t precision, void* stream);

/* One estimate_B_by_regression for every rollout, in the reference's order: hs_sim_config of the
 * current state; hs_sim_track_push into ders (player.cpp:557-558: the call advances the tracker);
 * hs_sim_probe; U[b][j] = the second difference of a copy of tracker b after pushing config_out[b][j]
 * (player.cpp:564, 572-575); hs_sim_regress_B with T = tau_out. The torques of the next real step are the
 * caller's business, and so is tau0. */
typedef struct {
  hs_sim_probe_args probe; /* precision must be HS_PREC_F64; config_out and tau_out (= T) are required */
  double* ders;            /* [B][3][config_dim], read and advanced */
  double* U;               /* [B][m][config_dim] probe accelerations */
  double* Bt;              /* [B][nmj][config_dim] */
  int32_t* rank;           /* [B] */
  void* workspace;         /* hs_sim_estimate_workspace(model, B, m) bytes, caller-owned, 8-byte aligned */
  size_t workspace_bytes;
} hs_sim_estimate_args;

/* Bytes of workspace hs_sim_estimate_B needs (the current configuration and a copy of the seeds). */
size_t hs_sim_estimate_workspace(hs_model_t model, int32_t n_rollouts, int32_t m);

/* HS_E_ARG for everything hs_sim_probe and hs_sim_regress_B reject, a NULL ders, U, Bt, rank or
 * workspace, and a workspace smaller than hs_sim_estimate_workspace. */
int hs_sim_estimate_B(hs_model_t model, const hs_sim_estimate_args* args);

/*
 * Configuration path control (CPC) on the estimated B (additive exports: HSLABS_ABI_VERSION stays 16):
 * cpccontroller::get_motor_torques (cpc.cpp:215-250) as modelplayer::set_cpc_torques drives it
 * (player.cpp:465-481), for every rollout of a batch, one wavefront per rollout, HS_PREC_F64 only.
 * The controller scans every target point (cpccontroller::tpis_subset without efficientdata,
 * cpc.cpp:437-443); the ball-tree prefilter, poscontrol mode, cost / cost1 and set_ghost_cpc_state are not
 * restated. All arrays are DEVICE arrays.
 * Per rollout, in the reference's order: set_current_state + apply_mask (a copy is masked, never the
 * caller's array); compute_b (cpc.cpp:111-121: b = [-I ; X], Bt_chi X = the left psi = config_dim - nmj
 * columns of Bt, Bt_chi = its right nmj columns, Eigen 3.3 ColPivHouseholderQR; bbt = b b^T);
 * compute_prox_loss_over_tps over all n_tp points (cpc.cpp:151-190); candidates (cpc.cpp:252-272): the
 * n_cand smallest losses, ascending; B_chi_dec = ColPivHouseholderQR(Bt_chi^T); the gain loop
 * (cpc.cpp:229-237) over cost2 (cpc.cpp:339-362) and controls (cpc.cpp:280-293); last_cand and
 * tp_dist_check (cpc.cpp:485-494); clip_norm(tau, tauc).
 * Where the reference is undefined, this library defines the result and says so in flags:
 *   - map<double, cand> collapses exactly equal losses into one candidate; here ties are kept, the lower
 *     target point index first (no flag: nothing is lost).
 *   - a target point whose loss is not finite (denom = 0, e.g. a zero target velocity) sorts after every
 *     finite loss, lower index first, and HS_CPC_FLAG_NONFINITE is set (the reference keys its map with NaN).
 *   - if no candidate's score is finite and below cost2's 1e10 (e.g. n_cand = 1 with loss exactly 0: 0 / 0),
 *     i_best = 0 and HS_CPC_FLAG_NOSCORE is set (the reference indexes column -1).
 *   - a rank-deficient Bt_chi or B_chi takes Eigen's basic solution, as hs_sim_regress_B does, and
 *     HS_CPC_FLAG_RANK is set.
 *   - n_tp < n_cand (the reference iterates past the map's end), n_cand < 1 or > 64, a NULL required
 *     pointer, a precision other than HS_PREC_F64, a stride too small, or target points beyond the
 *     kernel's 64 KB of LDS (three doubles and a word per point): HS_E_ARG. So is a k0 that is not finite
 *     or a kc <= 0, for which the reference's gain loop does not end.
 */
#define HS_CPC_FLAG_NONFINITE 1u
#define HS_CPC_FLAG_NOSCORE 2u
#define HS_CPC_FLAG_RANK 4u

typedef struct {
  double w;              /* loss weight of t0 (player.cpp:453: 10) */
  double sg;             /* goal speed factor (1) */
  double k0;             /* first gain of the gain loop (200) */
  double kc;             /* the loop ends once k <= kc (10) */
  double tauc;           /* torque norm limit (20) */
  double loss_cc;        /* prox_loss's weight on cc0 + cc1 (cpc.cpp:188: 10) */
  double tp_dist;        /* tp_dist_check's distance (cpc.cpp:490: 0.5) */
  int32_t n_cand;        /* candidates (10); 1..64 */
  int32_t goal_t0s;      /* player.cpp:458: 1 */
  int32_t tpdist_switch; /* set_flag("goal_t0s") switches it on (cpc.cpp:451): 1 */
  uint32_t mask;         /* bit i: coordinate i of q and dq is zeroed (cpc.cpp:40-41: {0, 1, 5} = 0x23) */
} hs_cpc_params;

/* The reference's live values (above). */
void hs_cpc_default_params(hs_cpc_params* p);

typedef struct {
  int32_t n_rollouts;
  int32_t n_tp;            /* target points per set */
  int32_t precision;       /* HS_PREC_F64 */
  int32_t reserved;
  hs_cpc_params params;
  const double* Bt;        /* [B][nmj][config_dim] (hs_sim_estimate_B) */
  const double* state;     /* rollout b: q at state + b * state_stride, dq config_dim doubles further (the
                              tracker's ders[b][0], ders[b][1]) */
  int64_t state_stride;    /* doubles, >= 2 * config_dim; 3 * config_dim passes hs_sim_track_push's ders as it is */
  const double* tp;        /* [n_tp][2 * config_dim + nmj] = (q, dq, tau) per target point, masked
                              (hs_cpc_target_points, or any array of this layout: load_tpset's case) */
  int64_t tp_stride;       /* doubles between the sets of consecutive rollouts; 0: one set shared by the batch */
  int32_t* low_tpdist;     /* [B] carried state, read and advanced; starts 1 (cpc.cpp:42) */
  double* tau;             /* [B][nmj] motor torques */
  int32_t* last_tpi;       /* [B] last_cand.tpi */
  uint32_t* flags;         /* [B] HS_CPC_FLAG_* */
  /* optional diagnostics (NULL to skip) */
  double* loss;            /* [B][n_tp] */
  int32_t* cand_tpi;       /* [B][n_cand] ascending loss */
  double* cand_t0s;        /* [B][n_cand][2] t0 and the s the controls use (sg where goal_t0s applies) */
  int32_t* passes;         /* [B] passes of the gain loop */
  int32_t* i_best;         /* [B] */
  void* stream;            /* hipStream_t */
} hs_cpc_args;

int hs_cpc_torques(hs_model_t model, const hs_cpc_args* args);

/* cpccontroller::set_target_points_by_per (cpc.cpp:51-63) from the controller tables of hs_sim_args
 * (q_tab, dq_tab [B][n_t][config_dim], tau_tab [B][n_t][nmj]): tp[b][i] = periodic::get_complete_traj_rec(i)
 * (periodic.cpp:408-417: sample i, lifted by n_t when i < 2, which is table row (i + n_t - 2) mod n_t),
 * masked. tp [B][n_t][2 * config_dim + nmj]. HS_PREC_F64 tables only. */
int hs_cpc_target_points(hs_model_t model, int32_t n_rollouts, int32_t n_t, const double* q_tab, const double* dq_tab,
                         const double* tau_tab, uint32_t mask, double* tp, void* stream);

/* n_steps of simulate_ode with cpc_control_flag and dynamics_from_simulation_flag (player.cpp:326-340),
 * enqueued on the stream with no host synchronisation between steps. Per step: hs_sim_estimate_B (pushes
 * the tracker, probes around tau0); hs_cpc_torques on ders[0..1]; one hs_sim_trial step, open loop, with
 * the CPC torques as a one-row table (set_ode_motor_torques' clip, the kicks and the fall check come with
 * it); the torques applied become tau0. A rollout the fall check has frozen keeps body, seed, tsi, its
 * tau0 row and its per-step output rows. The estimate and the controller still run on it (the launches
 * cover the batch): its tracker is pushed with the same configuration again (so its rates become 0, every
 * loss 0 / 0, and its flags HS_CPC_FLAG_NONFINITE | HS_CPC_FLAG_NOSCORE), low_tpdist, last_tpi, flags and
 * rank are written, and the seed the probes advanced is put back, which costs time and changes nothing
 * else. A rollout that freezes in step k keeps the seed after step k's estimate, as the reference's process
 * would have drawn before its fall_check exits. The reference's first two steps (play_t < 2 play_dt -> position control,
 * player.cpp:468) are the caller's: hs_sim_estimate_B + hs_sim_step for those, so that the tracker has its
 * two pushes. */
typedef struct {
  hs_sim_trial_args trial; /* sim.n_steps = the steps of this call; the tables and open_loop are ignored (the
                              step is open loop on the CPC torques); sim.precision must be HS_PREC_F64. The
                              per-step outputs are STEP-major here: tau_cmd / q_meas [n_steps][B][nmj],
                              torso [n_steps][B][3], n_contacts / normal_force [n_steps][B] */
  hs_cpc_params cpc;
  int32_t m;               /* probes per rollout and step (config_dim + 20) */
  int32_t n_tp;
  const double* dtau;      /* [n_steps or 1][B][m][nmj] perturbations */
  int64_t dtau_step_stride;/* doubles between steps; 0 reuses one set */
  const double* tp;        /* as hs_cpc_args */
  int64_t tp_stride;
  double* ders;            /* [B][3][config_dim] tracker, read and advanced */
  double* tau0;            /* [B][nmj] last motor torques, read and advanced */
  int32_t* low_tpdist;     /* [B] read and advanced */
  int32_t* last_tpi;       /* [B] */
  uint32_t* flags;         /* [B] the last step's HS_CPC_FLAG_* */
  int32_t* rank;           /* [B] the last step's regression rank */
  void* workspace;         /* hs_sim_cpc_workspace(model, B, m) bytes, caller-owned, 8-byte aligned */
  size_t workspace_bytes;
} hs_sim_cpc_args;

size_t hs_sim_cpc_workspace(hs_model_t model, int32_t n_rollouts, int32_t m);

/* HS_E_ARG for everything hs_sim_estimate_B, hs_cpc_torques and hs_sim_trial reject, and a missing or
 * small workspace. */
int hs_sim_cpc_step(hs_model_t model, const hs_sim_cpc_args* args);

/* Host-side handle over the calls above, for callers without device memory of their own
 * (the C++ shim's modelplayer): owns the device tables and state of B rollouts.
 * hs_sim_create = modelplayer::setup_per_controller (player.cpp:370-382) for every rollout:
 * n_t = int(period / params->dt + .5) controller rows from hs_run (same n_t for the whole
 * batch, else HS_E_ARG), play_t = int(t0 / dt + .5) dt, bodies at that trajectory sample
 * at rest (init_play_config). params is HOST memory; sim_params NULL = hs_sim_default_params. */
typedef struct hs_sim_s* hs_sim_t;
int hs_sim_create(hs_model_t model, const hs_gait_params* params, int32_t n_rollouts, const hs_sim_params* sim_params,
                  double t0, hs_sim_t* out);
/* n_steps of simulate_ode (synchronous); HOST outputs as in hs_sim_args, each may be NULL. */
int hs_sim_advance(hs_sim_t sim, int32_t n_steps, double* tau_cmd, double* q_meas, double* torso, int32_t* n_contacts,
                   double* normal_force);
/* HOST copies of the state: body [B][n_parts][HS_SIM_BODY_STRIDE], tsi [B] (either may be NULL). */
int hs_sim_get_state(hs_sim_t sim, double* body, int32_t* tsi);
/* The handle's trial settings (hs_sim_trial_args; kick_dv_host: HOST [B][3] or NULL = no kicks). Every
 * rollout's state becomes HS_TRIAL_RUNNING, and hs_sim_advance runs hs_sim_trial from now on. A handle
 * on which this was never called runs hs_sim_step. */
int hs_sim_set_trial(hs_sim_t sim, int32_t open_loop, double torque_limit, int32_t kick_every, int32_t kick_phase,
                     const double* kick_dv_host, double hc, int32_t check_from, int32_t check_until);
/* HOST copy of the trial state [B] (HS_E_ARG before hs_sim_set_trial). */
int hs_sim_get_trial_state(hs_sim_t sim, int32_t* state_host);
void hs_sim_free(hs_sim_t sim);

/* The fused step launches' kernel (ABI 15). hs_run_calls takes the limb-lane kernel (lane = (rollout,
 * limb), eight rollouts per wavefront) for a model of its class (*ok = 1: every shipped
 * model), HS_SOLVE_AUTO, no x / q / dq rows, and calls whose samples fit the IK table; in fp64 its outputs
 * are bitwise hs_rollout_kernel's (the steps it does not take go to the same fixup launch). In fp32
 * (HS_PREC_F32) they are close, not bitwise (float contraction differs by context): the tests hold torques
 * to 1e-3 relative and flags to equality on more than 99.9 % of steps (tests/test_gpu_limb.py). HS_LIMB=0
 * in the environment keeps hs_rollout_kernel, HS_LIMB_F32=0 keeps it for fp32 calls only.
 * hs_limb_launches: the limb-lane launches this process has made.
 * An fp64 fused limb-lane launch of at least 40 steps whose last tile is nearly full (at most 1 idle slot
 * in 32) runs the tile mapping instead (a wavefront = one rollout x eight steps two apart, which share the
 * stencil's limb FK through LDS), the same outputs bitwise; shorter launches, fp32
 * calls and hs_run_steps keep eight rollouts per wavefront. Environment: HS_LIMB_TILE=0 keeps every launch
 * packed; HS_LIMB_TILE_MIN=<n> (a positive decimal number, else ignored) replaces the rule by "at least
 * <n> steps" for every precision -- a test and measurement switch, slower than the rule where the rule
 * says packed. hs_limb_tile_launches: the limb-lane launches of this process that ran the tile mapping
 * (an additive export: HSLABS_ABI_VERSION stays 16, no existing layout or meaning changes).
 * A tile-mapped launch of up to 256 steps orders its steps over the tiles by a planner (chains of steps
 * whose table rows ascend by 2, a tile per run of 8) where that saves limb FK passes over the order "even
 * steps, then odd steps", which it keeps elsewhere; the outputs are the same bitwise under either.
 * HS_LIMB_TILE_PLAN=0 keeps the even/odd order everywhere, =2 takes the planner's order even where it saves
 * nothing (tests). hs_limb_tile_plan_launches: the tile-mapped launches that ran the planner's order (an
 * additive export as well).
 * A tile-mapped wavefront may run several tiles of its rollout one after the other (the tile loop), so that
 * the rollout's share of a step is paid once per wavefront; the outputs are the same bitwise at any number.
 * HS_LIMB_TILE_LOOP=<n> (a positive decimal number, else ignored) forces n tiles per wavefront, 1 a tile per
 * wavefront. hs_limb_tile_loop_launches: the tile-mapped launches whose wavefronts ran more than one tile
 * (an additive export as well). */
int hs_model_limb_lane(hs_model_t model, int32_t* ok);
int64_t hs_limb_launches(void);
int64_t hs_limb_tile_launches(void);
int64_t hs_limb_tile_plan_launches(void);
int64_t hs_limb_tile_loop_launches(void);
/* Diagnostics of the limb-lane kernel: its launches and the steps it deferred to the fixup launch (one,
 * two contacts, guards near their thresholds, ...) in this process; *deferred is read from the device
 * (synchronous on the current device). Either pointer may be NULL. */
int hs_limb_stats(int64_t* launches, int64_t* deferred);
/* Diagnostics of the preparation pass's per-row tables: what the last fp64 call of `model` on `stream` (and
 * the current device) left for `rollout` in its workspace, rows [0, n_rows), n_rows <= 64, of the call's IK
 * table: ktab[row][limb][3] the limbs' joint values, kvel[row][limb][3] the joint rates the limb kernel's
 * tile loop reads (rows 1 .. n - 2 of a call of n rows; the others are never written), kbig[row][limb] a row's
 * range bit (a joint value of 2^20 or more, or not finite), kbad[row][limb] its IK's failed-or-unreachable
 * bit, limb stride 6, and the rollout's dt. Synchronous (the stream is drained first); a pointer may be NULL.
 * Which rows a call writes: samples [lo, lo + n) of the period, n <= 64 (calls that read more samples keep no
 * table). kvel and kbig are written only by a call one of whose step launches takes the tile mapping. Not to be
 * called while another thread runs a call on the same model (the workspace may be regrown under the read). An
 * additive export as well. */
int hs_debug_limb_tables(hs_model_t model, void* stream, int32_t rollout, int32_t n_rows, double* ktab, double* kvel,
                         uint8_t* kbig, uint8_t* kbad, double* dt);

const char* hs_last_error(void);
int hs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
