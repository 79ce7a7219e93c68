// rbl_api_internal.hpp -- internals shared by the translation units that implement include/rbl.h:
//   rbl_core.hip      context, errors, device buffers, copies, timings, parameters / configuration
//   rbl_options.hip   named options (rbl_set_option / rbl_get_option)
//   rbl_comm.hip      multi-GPU communicator: RCCL inside the library, or the caller's callbacks
//   rbl_products.hip  mobility products (kernel choice, launches), positions, dense entry points
//   rbl_bodies.hip    K operators, preconditioners, per-body factors, saddle operator
//   rbl_roots.hip     M^{1/2} W: dense Cholesky path and the Lanczos roots
//   rbl_solvers.hip   GMRES on the saddle operator
//   rbl_steps.hip     whole time steps, the stochastic midpoint scheme (free and mixed), random finite differences
//   rbl_forces.hip    configuration-dependent forces (weight, wall and steric repulsion, tabulated potentials, traps)
//   rbl_ensemble.hip  ensembles of independent replicas of one small system: the one-step calls, what every step enqueues
//   rbl_ens_run.hip   runs of ensemble steps: one request, its plan, the loop with its joints, observers and drive parts
//   rbl_ens_field.hip the flow at probe points of every replica of an ensemble, the observers' share of a run's commit
//   rbl_ens_drive.hip the time-dependent body input of a driven ensemble run, its lock-in sums
//   rbl_field.hip     the fluid velocity at arbitrary points from blob forces
//   rbl_mixed.hip     prescribed kinematics: held or driven bodies among free ones, the loads that takes; the entry points of their Brownian step
//   rbl_flow.hip      imposed linear flow and body-frame slip added to every step's slip, first moments of the blob forces
//   rbl_periodic.hip  the periodic cell in x and y: its state, and the refusals of what it is not offered with
// None of these symbols is exported from librbl.so.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "rbl_internal.hpp"

#pragma GCC visibility push(hidden)

// ---- requests -----------------------------------------------------------------------------------------------------
// What a solver asks of one product, preconditioner application or saddle product beyond the plain operator, and what that call
// did about it, travel in these structs: a default-constructed one is the plain operator, and no call leaves anything behind in
// rbl_ctx for the next one.  Fields marked "answer" are written by the callee.
struct RblProductReq {                   // apply_M_enqueue, apply_M_multi_enqueue
  bool relaxed = false;                  // far tile pairs in packed single precision (inexact Krylov iterations only)
  bool undamped = false;                 // skip the damping B in this product even while RBL_OPT_NO_DAMP is off (preconditioned root)
  const RblSaddleFuse *fuse = nullptr;   // the slab reduction of a symmetric product also writes the saddle epilogue
  bool fused = false;                    // answer: it did (ordered kernel, sharded product: it did not)
};
constexpr double RBL_PC_FSIGN_REFERENCE = -1.0;   // apply_PC as the reference defines it (see rbl_ctx::gmres_pc_sign_fix)
struct RblPcReq {                        // apply_PC_dev
  double fsign = RBL_PC_FSIGN_REFERENCE; // sign of the force block
  const RblNormFold *fold = nullptr;     // d_in is an un-normalised Arnoldi vector (refused unless pc_can_fold)
  bool leave_ktl = false;                // also leave K^T Lambda of the output ...
  const double *ktl = nullptr;           // answer: ... here; NULL: this form does not produce it (diagonal, sharded context)
};
struct RblSaddleReq {                    // apply_saddle_dev
  const double *ktl = nullptr;           // K^T Lambda of d_x as the preconditioner left it (RblPcReq::ktl), or NULL
  bool relaxed = false;                  // see RblProductReq
  const double *dotV = nullptr;          // first Gram-Schmidt pass of the Arnoldi step that follows: the basis, ...
  int dotK = 0;                          // ... its vectors so far ...
  double *dotPart = nullptr;             // ... and where their partial sums go (see RblSaddleFuse)
  int dots_np = 0;                       // answer: partial sums per vector (0: not done)
};

// ---- rbl_core.hip -------------------------------------------------------------------------------------------------
int need_params(rbl_ctx *c);
int need_config(rbl_ctx *c);
int need_K(rbl_ctx *c);                       // (rbl_bodies.hip)
// Krylov coefficients (<= 512 doubles, slot 0 or 1) to the device through a pinned buffer: no stream drain
int upload_coef(rbl_ctx *c, double *d_dst, const double *src, int count, int slot);
int copy_h2d(rbl_ctx *c, void *dst, const void *src, size_t bytes);   // synchronous for large pageable sources
int copy_d2h(rbl_ctx *c, void *dst, const void *src, size_t bytes);
int read_back(rbl_ctx *c, void *dst, const void *d_src, size_t bytes);   // small device -> host read the host needs NOW
// the context's pinned buffer behind read_back (allocated at first use); NULL: `bytes` does not fit it
int pin_buffer(rbl_ctx *c, size_t bytes, void **h_pin);
// Which side the caller's arrays of a call live on.  An entry point's host form and its _dev form are one core that moves the
// caller's data with these two: Host is copy_h2d / copy_d2h (pageable arrays, synchronous above 64 KB), Device an asynchronous
// device-to-device copy on the context's stream.  d_dst of xfer_in and d_src of xfer_out are the library's own workspace
enum class RblSide { Host, Device };
int xfer_in(rbl_ctx *c, RblSide side, void *d_dst, const void *src, size_t bytes);
int xfer_out(rbl_ctx *c, RblSide side, void *dst, const void *d_src, size_t bytes);
int finish_and_check(rbl_ctx *c);             // drain the stream, read + clear the latched device flags
RblParams ctx_params(const rbl_ctx *c, bool force_no_damp);   // undamped when RBL_OPT_NO_DAMP or the caller asks

// ---- rbl_comm.hip -------------------------------------------------------------------------------------------------
bool comm_on(const rbl_ctx *c);
void comm_body_range(const rbl_ctx *c, int *b0, int *b1);              // this rank's bodies
void comm_body_range_of(const rbl_ctx *c, int rank, int *b0, int *b1);
int comm_allreduce(rbl_ctx *c, double *d_buf, int64_t count);
// Complete per-body results in place: every rank has written the entries of ITS bodies; with a native communicator / an
// all-gather callback the owners' segments are gathered, otherwise the caller must have ZEROED what it does not own
// (comm_gather_needs_zero) and a sum all-reduce over the span completes it.
bool comm_gather_needs_zero(const rbl_ctx *c);
// per_body doubles per body (body-major, first body at offset base) of nvec vectors `pitch` apart in d_buf
int comm_allgather_bodies(rbl_ctx *c, double *d_buf, int64_t base, int64_t per_body, int nvec, int64_t pitch);
// two per-body parts in ONE fused collective (the preconditioner's [lambda ; U]; lever arms + positions)
int comm_allgather_bodies2(rbl_ctx *c, double *d_buf1, int64_t base1, int64_t per_body1, double *d_buf2, int64_t base2, int64_t per_body2);
// rows [row_bounds[r], row_bounds[r + 1]) x `width` doubles of every rank r, in place in one vector (the row split's product)
int comm_allgather_rows(rbl_ctx *c, double *d_buf, const int64_t *row_bounds, int64_t width);
void comm_release(rbl_ctx *c);                // destroy a native communicator (rbl_destroy)

// ---- rbl_products.hip ---------------------------------------------------------------------------------------------
int apply_M_enqueue(rbl_ctx *c, bool wall, const double *d_F, const double *d_r, int64_t nbl, int64_t row_begin, int64_t row_end,
                    double *d_out, RblProductReq *rq = nullptr);
int apply_M_multi_enqueue(rbl_ctx *c, bool wall, const double *d_F, const double *d_r, int64_t nbl, int nrhs, double *d_out,
                          int64_t ldF = 0, int64_t ldO = 0, RblProductReq *rq = nullptr);
int ensure_xq_dev(rbl_ctx *c);
int positions_dev(rbl_ctx *c, int b0, int b1, double *d_out);

// ---- rbl_bodies.hip -----------------------------------------------------------------------------------------------
int sync_bodies(rbl_ctx *c);
int pc_block_factors(rbl_ctx *c, int b0 = 0, int b1 = -1);
bool bf_on(const rbl_ctx *c);
int bf_build(rbl_ctx *c);
int blk_prepare(rbl_ctx *c, int b0, int b1);
int blk_solve(rbl_ctx *c, int b0, int nbo, const double *in, double *out, int nv, int64_t pitch, int mode, bool allow_f32 = true);
int blk_trmv(rbl_ctx *c, int b0, int nbo, const double *in, double *out);
bool pc_can_fold(rbl_ctx *c);
// the workers behind rbl_apply_PC_dev / rbl_apply_saddle_dev (which pass default requests)
int apply_PC_dev(rbl_ctx *c, const double *d_in, double *d_out, RblPcReq &rq);
int apply_PC_multi_dev(rbl_ctx *c, const double *d_in, double *d_out, double *d_scratch, int nv, int64_t pitch, double fsign);
int apply_saddle_dev(rbl_ctx *c, const double *d_x, double *d_out, RblSaddleReq &rq);
int blk_trmv_multi(rbl_ctx *c, int b0, int nbo, const double *in, double *out, int nv, int64_t pitch);

// ---- rbl_roots.hip ------------------------------------------------------------------------------------------------
int tl_build(rbl_ctx *c);
int tl_apply(rbl_ctx *c, const double *w, double *wo, int nvec, int64_t pitch, int op);
int mhalf_dev_multi(rbl_ctx *c, const double *d_r, int64_t nbl, const double *d_W, int nvec, int method, double *d_out);

// ---- rbl_solvers.hip ----------------------------------------------------------------------------------------------
// the library's GMRES (Arnoldi kernels, host Givens solve, overlapped convergence test) on a system of the saddle system's size whose
// operator and right preconditioner the caller supplies (rbl_mixed.hip).  The shortcuts fused into the ordinary saddle solve
// (K^T lambda by-product, Gram-Schmidt sums in the product, normalisation folded into the preconditioner, relaxed products) are
// requests to the library's own operators (RblPcReq, RblSaddleReq): such a solve makes none; the one-kernel solver and the
// iteration-count memory stay off too.  extra: unknowns the caller's system has behind the 3 N + 6 N_bod of the saddle system (the
// joint forces of rbl_joints.hip); every vector the callbacks see is that much longer.
struct RblSolveOps {
  int (*op)(rbl_ctx *c, void *user, const double *d_x, double *d_out);
  int (*pc)(rbl_ctx *c, void *user, const double *d_in, double *d_out);
  void *user;
  int64_t extra = 0;
};
int gmres_core_with_ops(rbl_ctx *c, const RblSolveOps *ops, const double *d_rhs, int max_iter, double rtol, double *d_x, int *iters_out,
                        double *resid_out);
// The lock-step analogue: k <= 16 right-hand sides (d_rhs, d_x: k vectors of the system's size one after the other), each with its
// own recurrence and stopping test, whose operator and preconditioner are ONE call per iteration for all of them.  The vectors a
// callback reads and writes are `pitch` doubles apart; `live` has bit c set while column c iterates: a callback need not touch a
// column whose bit is clear (its input slot is zeroed, its output is never read).  d_scratch: room for one vector per column,
// `pitch` apart too.
struct RblMultiOps {
  int (*op)(rbl_ctx *c, void *user, const double *d_x, double *d_out, int k, int64_t pitch, unsigned live);
  int (*pc)(rbl_ctx *c, void *user, const double *d_in, double *d_out, double *d_scratch, int k, int64_t pitch, unsigned live);
  void *user;
};
int gmres_multi_with_ops(rbl_ctx *c, const RblMultiOps *ops, const double *d_rhs, int k, int max_iter, double rtol, double *d_x,
                         int *iters_out, double *resid_out);

// ---- rbl_steps.hip ------------------------------------------------------------------------------------------------
// the lengths the context's configuration gives every vector: blobs, 3 N, 6 N_bod, and the saddle system's 3 N + 6 N_bod
struct RblSizes { size_t N, n3, nb6, nsys; };
RblSizes sizes_of(const rbl_ctx *c);
// The stages every whole-step entry point of a single context shares (rbl_step_deterministic, rbl_step_brownian, rbl_step_jointed,
// the steps of rbl_mixed.hip).  A model that enters every step has these places to go:
// step_begin: the flow model's checks, the device, then RBL_ERR_ARG with `missing` when the caller names a required argument that
// is NULL (the refusal's place in the order, behind the device), then the previous record of moments is dropped
int step_begin(rbl_ctx *c, const char *missing = nullptr);
// the slip of a call into d_slip (3 N): the caller's (either side; NULL: none) and, with `model`, the flow model's term at q^n
// added.  *have_slip: d_slip holds something (nothing is written otherwise)
int step_slip(rbl_ctx *c, RblSide side, const double *slip, double *d_slip, bool model, bool *have_slip);
// the inputs of a step at q^n from host arrays: d_slip (3 N) = slip (NULL: zero) + the flow model's term, then d_force (6 N_bod) =
// F_body - K^T f_phys of the force model (which ends in a drain and a check of the latched flags while it is on)
int step_inputs(rbl_ctx *c, const double *F_body, const double *slip, double *d_force, double *d_slip);
// the end of a step's solve: RBL_OPT_RECORD_MOMENTS of d_lambda at the configuration the context is at, U (6 N_bod, from d_U) and,
// when `more` is not NULL, n_more doubles from d_more to the host, then the stream drained -- by finish_and_check when
// `check_flags`, by a plain synchronisation otherwise
int step_commit(rbl_ctx *c, const double *d_lambda, const double *d_U, double *U, const double *d_more, double *more, size_t n_more,
                bool check_flags);
// The stochastic midpoint scheme, once for rbl_step_brownian and rbl_step_brownian_mixed (rbl_mixed.hip): the all-free step is the
// mixed one with no mask (h_mask, d_mask, d_body_in all NULL).  d_s = slip - kBT M_RFD - BI may alias d_slip; d_slip NULL: zero.
// per: mask entries per body, 1 or 6 (a mask per velocity component whose rotation entries are all equal within a body)
int rhs_and_midpoint_core(rbl_ctx *c, const uint8_t *h_mask, const uint8_t *d_mask, const double *d_body_in, const double *d_slip,
                          const double *d_W, uint64_t seed, int method, int split_rand, double delta, double *d_s, double *X_half,
                          double *Q_half, int per = 1);
// rbl_mixed.hip: the masks per velocity component that the Brownian step takes (every body's rotation entries all equal), for
// prescribed6[R 6 N_bod]; RBL_ERR_ARG names `who`, the first offending body and, with R > 1, its replica.  Touches no device
int rbl_bd_mask6_check(rbl_ctx *c, const char *who, const uint8_t *prescribed6, int R, int N_bod);
// the body loads the last rbl_step_deterministic / rbl_step_brownian solved with, on the device (6 N_bod; step_buffers' layout)
const double *step_force_dev(const rbl_ctx *c);
// the host's noise W (9 N_blobs) into d_W; *d_W = NULL when W is NULL
int step_upload_W(rbl_ctx *c, const double *W, double **d_W);
// save q^n, rhs(X_half, Q_half), operators at q^{n+1/2}, solve(U: 6 N_bod, host), back to q^n (also on failure), evolve by dt U
int step_midpoint(rbl_ctx *c, const std::function<int(double *, double *)> &rhs, const std::function<int(double *)> &solve);

// ---- rbl_forces.hip -----------------------------------------------------------------------------------------------
// any term of the model is switched on: the built-in one, a pair table, a height table, the traps, dipole pairs or the field torque
bool ia_any(const rbl_ctx *c);
// the model's PHYSICAL forces at the context's configuration: d_f (3 N, may be NULL), d_FT = K^T f (6 N_bod, may be NULL),
// per-blob energies d_e (N, may be NULL); enqueued on the context's stream under RBL_T_FORCES
int ia_eval(rbl_ctx *c, double *d_f, double *d_FT, double *d_e);
// the steps' use of it: d_force (6 N_bod, reference convention) -= K^T f_phys at the current configuration, then the latched
// device flags are checked (a neighbour-list overflow fails the step).  No-op while the model is off.
int ia_add_to_step_force(rbl_ctx *c, double *d_force);
// the model for `reps` independent copies of N_bod bodies (an ensemble, rbl_ensemble.hip): body centres d_X (3 N_bod reps), blob
// positions and lever arms of all copies; steric and dipole pairs only inside a copy.  d_Q (4 N_bod reps): the orientations, for
// the dipoles.  d_work: ia_batch_bytes; *d_f -> the blob forces (3 N reps, inside d_work); d_FT (6 N_bod reps) and per-blob
// energies d_e may be NULL.  d_accepted (a run): copy r evaluates the field at its field time + dt * d_accepted[r]
size_t ia_batch_bytes(int N_bod, int N_blb, int reps);
int ia_eval_batch(rbl_ctx *c, const double *d_X, const double *d_Q, const double *d_pos, const double *d_lever, int N_bod, int reps,
                  void *d_work, double **d_f, double *d_FT, double *d_e, unsigned *d_err, const int *d_accepted = nullptr);

// ---- rbl_flow.hip -------------------------------------------------------------------------------------------------
// the model's checks that need no device (wall consistency, the pattern's structure, n_scale against n_bod bodies); RBL_OK while
// both parts are off
int flow_check(rbl_ctx *c, int n_bod);
// the steps' use of the term t = scale R s_body - u_inf at the context's configuration: d_slip (3 N) becomes slip + t when
// *have_slip, t otherwise, and *have_slip becomes true.  While both parts are off: nothing (no launch, no allocation)
int flow_add_to_step_slip(rbl_ctx *c, double *d_slip, bool *have_slip);
// the same for `reps` replicas of N_bod bodies in one launch (positions and orientations of all of them).  d_caller (a run's
// resident slip, uploaded once): the caller's slip is read there and d_slip is only written, so it is never added to twice
int flow_add_batch(rbl_ctx *c, const double *d_pos, const double *d_Q, int N_bod, int reps, double *d_slip, bool *have_slip,
                   const double *d_caller = nullptr);
bool flow_on(const rbl_ctx *c);               // either part of the model is switched on
// D_b = sum l lambda^T of n_bodies bodies, Nb a replica; d_lever, or NULL and (d_Q, d_cfg) to rebuild the lever arms
void flow_launch_moments(rbl_ctx *c, const double *d_lever, const double *d_Q, const double *d_cfg, const double *d_lam, int Nb,
                         int n_bodies, int64_t rep_stride, double *d_D);
// a whole-step entry point begins: with RBL_OPT_RECORD_MOMENTS on the previous record is dropped, so a step whose solve fails
// leaves nothing to read
void flow_begin_step(rbl_ctx *c);
// RBL_OPT_RECORD_MOMENTS: the moments of d_lambda at the configuration the context is at; no-op while the option is off
int flow_record_moments(rbl_ctx *c, const double *d_lambda);

// ---- rbl_ensemble.hip / rbl_ens_field.hip ---------------------------------------------------------------------------
// The ensemble as the one-shot field reads it (after ens_state_check, the refusals that look at the context's state alone): the
// device touched, the current configuration of all replicas, the reference configuration, the cell (checked as a step checks it)
struct RblEnsView {
  const double *X, *Q, *cfg;
  int R, Nb, nbl;
  bool cell;
  RblSmallCell C;
  const RblEnsCellRec *cells;                 // a cell per replica: the table on the device (C is then unused); NULL: the shared cell C
};
int ens_view(rbl_ctx *c, RblEnsView *v);
// One launch of the probe kernel (include/rbl.h section 5, observers): u[R 3 P] of P points per replica from the blob forces lam
// (replica r's at lam + r lam_stride) at the configuration (X, Q) of all R replicas.  pts_stride: 0 for one shared point set,
// 3 P for one per replica; body >= 0: the points are offsets fixed in that body.  rerr: one error word per replica
struct RblEnsProbe {
  const double *X, *Q, *cfg;
  const double *lam;
  long lam_stride;
  const double *pts;
  long pts_stride;
  double *u;
  unsigned *rerr;
  int Nb, nbl, P, body;
};
// a non-finite coordinate of points[sets 3 P] (host) is RBL_ERR_ARG naming `who`, the set and the point
int ens_points_check(rbl_ctx *c, const char *who, const double *points, int64_t n_points, int sets);
struct RblEnsProbeGeom { int NI, waves; int64_t tiles; };
RblEnsProbeGeom ens_probe_geometry(int64_t n_points, int R, int n_cu);
// cell: the shared cell, or NULL: none; cells (a cell per replica, device): replica r sums over the images of cells[r], cell is unused
void ens_probe_launch(hipStream_t st, const RblParams &P, bool wall, const RblSmallCell *cell, const RblEnsProbe &A, int R, int n_cu,
                      const RblEnsCellRec *cells = nullptr);
// a run's step, behind ens_probe_launch with rerr = d_oerr (R words, zero before the run's first step): rerr[r] = oerr[r] where
// rerr[r] is still clear, oerr cleared again
void ens_obs_flags_launch(hipStream_t st, unsigned *d_rerr, unsigned *d_oerr, int R);

// ---- rbl_ensemble.hip, as rbl_ens_run.hip reads it: what one step enqueues, and the checks a run makes before it ------------------
// a bump allocator over one device buffer (256-byte aligned pieces; base NULL: only the sizes)
struct RblCarve {
  char *base; size_t off = 0;
  template <class T> T *take(size_t count)
  {
    T *p = (T *)(base ? base + off : nullptr);
    off += (sizeof(T) * count + 255) & ~(size_t)255;
    return p;
  }
};
struct EnsWork {
  double *lever, *pos, *F, *FT, *slip, *W, *Lm, *Linv, *MW, *dq, *Xh, *Qh, *rhs, *x, *gm, *e;
  double *jr;                                // the jointed step: the joint rows the caller gave (joint_rhs / joint_velocity), 3 n_joints per replica
  void *ia;
  // read-back block: residuals | iterations | error word per replica | one error word for the batch
  double *resid; int *iters; unsigned *rerr, *gerr;
  size_t rb_bytes;
  // prescribed bodies: U and F of the masked solve follow the read-back block (rb_mx_bytes reaches their end) and stand in front
  // of x in one piece [U | F | x], as the masked rbl_launch_gmres_small_ens wants them; body_in is uploaded where F_body goes (F)
  double *U, *Fo; unsigned char *mask;
  size_t rb_mx_bytes;
};
// the jointed variant of a step (hard joints): the joint table on the device, coef = -gamma / dt of a time step, whether w.jr holds
// joint rows the caller gave, and the caller's name for a refusal
struct EnsJtStep { const char *who; RblEnsJoints T; double coef; bool have_jr; };
// The observers of a run (rbl_ensemble_run_observed), as one step sees them: device pointers into the run's buffer.  P probe
// points (sets: 1 shared set or R; body >= 0: offsets fixed in that body) whose field goes to u_step, and D_step (moments) for
// the first moments of the step's lambda.  They travel with the step's inputs (EnsStepIn); nothing of them is context state
struct EnsObs {
  int P = 0, sets = 1, body = -1;
  bool moments = false;
  const double *pts = nullptr;
  double *u_step = nullptr, *D_step = nullptr;
  unsigned *oerr = nullptr;                 // the probe kernel's flags of the step, R words (k_ens_obs_flags passes them on and clears them)
};
// What one step reads.  A one-step call passes host arrays, which the enqueueing part uploads; a run (rbl_ensemble_run) has uploaded
// them once: resident -- prescribed then only says that the step is the masked one (w.mask is filled), F_body is unused (w.F is
// filled), slip is the run's device copy, W is NULL.  chol_err: the batched Cholesky's error stride (0: the batch word)
struct EnsStepIn {
  const EnsObs *obs = nullptr;              // a run with observers: evaluated on the step's lambda just before the update
  const uint8_t *prescribed = nullptr;
  int per = 1;                              // entries of prescribed per body: 1 (whole bodies) or 6 (velocity components)
  const double *F_body = nullptr, *slip = nullptr, *W = nullptr;
  bool resident = false;
  int64_t chol_err = 0;
  const int *accepted = nullptr;            // a run: the device counters of accepted steps, the field's clock (section 4)
};
int ens_work(rbl_ctx *c, int max_iter, EnsWork *w, int nj = -1);   // nj < 0: the joints of the active set, none when they are off
// everything the deterministic / the stochastic step enqueues, from the uploads to the update (jt: the jointed solve or step)
int ens_enqueue_det(rbl_ctx *c, const EnsWork &w, const EnsStepIn &in, int max_iter, double rtol, bool move, const EnsJtStep *jt = nullptr);
int ens_enqueue_bd(rbl_ctx *c, const EnsWork &w, const EnsStepIn &in, uint64_t seed, int split_rand, double delta, int max_iter,
                   double rtol);
int ens_upload_mask(rbl_ctx *c, const EnsWork &w, const uint8_t *prescribed, int per);
int ens_jt_upload(rbl_ctx *c, RblEnsJoints *T);           // the joint table on the device, uploaded when stale
// the two configuration buffers (c->ens_cur: the committed one) and, behind them, the reference configuration
inline double *ens_X(rbl_ctx *c, int which) { return (double *)c->d_ens.p + (size_t)which * 7 * c->ens_R * c->ens_Nb; }
inline double *ens_Q(rbl_ctx *c, int which) { return ens_X(c, which) + (size_t)3 * c->ens_R * c->ens_Nb; }
inline double *ens_cfg(rbl_ctx *c) { return ens_X(c, 2); }
// the state and solver checks; only ens_ready touches a device.  pre: the caller's name with ": " behind it, or nothing; ens_state_check:
// no ensemble, a changed structure, a communicator
bool ens_jt_active(const rbl_ctx *c);
bool ens_cell_on(const rbl_ctx *c);
int ens_cell_refuse(rbl_ctx *c, const char *who);
int ens_flow_check(rbl_ctx *c);
int ens_state_check(rbl_ctx *c, const std::string &pre, bool comm_last = false);
int ens_ready(rbl_ctx *c);
std::string ens_beyond(const std::string &pre = "");
int ens_check_solver(rbl_ctx *c, int max_iter);
int ens_mx_check(rbl_ctx *c, const char *who, const uint8_t *prescribed, const double *body_in, int max_iter, double rtol, int per = 1);
int ens_jt_check(rbl_ctx *c, const char *who, const double *F_body, int max_iter, double rtol);

// ---- rbl_ens_field.hip: the observers of a run as ens_run carries them, a part with the life cycle of the joints' and the drive's ----
struct RblEnsObsRun {
  const rbl_run_obs_opts *o = nullptr;
  rbl_run_obs_out *out = nullptr;
  EnsObs step;                                   // what every step of the run is handed (EnsStepIn::obs)
  size_t nu = 0, nD = 0;                         // entries of u (R 3 P) and of D (R 9 N_bod, with moments)
  // device: points | this step's u (step.u_step), the last accepted one, the sum | the same three of D | frames | flags (step.oerr)
  double *u_last = nullptr, *u_sum = nullptr, *D_last = nullptr, *D_sum = nullptr, *fU = nullptr, *fD = nullptr;
};
size_t ens_obs_carve(RblEnsObsRun &O, void *base, int R, int Nb, size_t n_frames);   // as ens_drive_carve
// the points go up once; last, sum and the flags start at zero
int ens_obs_begin(rbl_ctx *c, RblEnsObsRun &O, void *base, int R, int Nb, size_t n_frames);
// after the run's commit, once for u and once for D (frame < 0: a step that records none)
void ens_obs_after(rbl_ctx *c, const RblEnsObsRun &O, int R, const int *d_stopped, const unsigned *d_vflag, long frame);
int ens_obs_end(rbl_ctx *c, const RblEnsObsRun &O, size_t nfr);   // the read-back: the sums, the nfr frames the run completed

// ---- rbl_ens_drive.hip --------------------------------------------------------------------------------------------
// The drive of rbl_ensemble_run_driven (include/rbl.h section 5) as ens_run carries it through a run: the checked options with
// the per-replica arrays spread to R on the host, and the device pieces carved behind the run's own buffer
struct RblEnsDriveRun {
  const rbl_run_drive_opts *o = nullptr;
  rbl_run_drive_out *out = nullptr;
  bool masked = false;                           // the run has a mask: F_c, F_s are kept
  std::vector<int> cum, start;                   // host: the prefix sums of phase_steps (n_phases + 1, or empty), the starting positions [R]
  std::vector<double> omega, t0;                 // host: [R] each
  // device
  double *A0 = nullptr, *C = nullptr, *S = nullptr, *P = nullptr, *om = nullptr, *t0d = nullptr, *cs_sn = nullptr, *sums = nullptr,
         *t_end = nullptr;
  int *cum_d = nullptr, *pos = nullptr;
};
// the drive's own refusals, none needing a device (R == 0, no ensemble: the checks that need R are left to the underlying run's
// RBL_ERR_STATE); *empty: no harmonic part, no phases, no lock-in.  Fills D's host side
int ens_drive_check(rbl_ctx *c, const char *who, const rbl_run_drive_opts *d, int R, int Nb, bool *empty, RblEnsDriveRun *D);
// D's device pieces from base (NULL: none) -> their bytes
size_t ens_drive_carve(RblEnsDriveRun &D, void *base, int R, int Nb);
// A0 (host, [R 6 N_bod]) and the drive's arrays go up once, the sums start at zero
int ens_drive_begin(rbl_ctx *c, RblEnsDriveRun &D, void *base, int R, int Nb, const double *A0);
// k_ens_drive: the step's input of every replica into d_in, from the replicas' accepted counters and cycle positions
void ens_drive_step(rbl_ctx *c, const RblEnsDriveRun &D, int R, int Nb, const int *d_accepted, double *d_in);
// k_ens_drive_commit, after the run's commit: Xo the body centres the step started from, U (replica r's six per body at
// U + r u_stride) the velocities the update read, Fo the masked solve's loads or NULL
void ens_drive_after(rbl_ctx *c, const RblEnsDriveRun &D, int R, int Nb, const int *d_stopped, const unsigned *d_vflag,
                     const int *d_accepted, const double *d_Xo, const double *d_U, long u_stride, const double *d_Fo);
int ens_drive_end(rbl_ctx *c, const RblEnsDriveRun &D, int R, int Nb);   // the read-back into the caller's arrays (enqueued; the caller drains)
// out of an empty drive: cycle_pos zeros, t_end = t0 + dt accepted on the host
void ens_drive_empty_out(const rbl_ctx *c, const RblEnsDriveRun &D, int R, const int *accepted);

// ---- rbl_periodic.hip ---------------------------------------------------------------------------------------------
bool periodic_on(const rbl_ctx *c);           // a cell is set and switched on
// RBL_ERR_STATE "<who>: not offered with a periodic cell ..." while the cell is on, RBL_OK otherwise; touches no device
int periodic_refuse(rbl_ctx *c, const char *who);
// the checks a cell meets at use, shared by the single context's product and the ensembles' steps: RBL_ERR_STATE "periodic cell: the
// wall term is off ..." / "... no longer exceeds 4a ... (call <setter> again)"; L: the cell's two lengths
// replica >= 0 (an ensemble with a cell per replica): the message names it, "periodic cell: replica 3: Lx ..."
int periodic_use_check(rbl_ctx *c, bool wall, const double *L, const char *setter, int replica = -1);
// an ensemble's cells are stored per replica (rbl_ensemble_set_cells; on or off), not as the one shared cell
bool ens_cells_stored(const rbl_ctx *c);
// the table of those cells on the device (rbl_ctx::d_ens_cells), in units of the current blob radius: uploaded when the cells are
// set, and by the callers at use when a has changed since -- never per step.  Nothing while the table is current
int ens_cells_upload(rbl_ctx *c);

#pragma GCC visibility pop
