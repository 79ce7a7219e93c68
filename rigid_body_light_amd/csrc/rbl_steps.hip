// rbl_steps.hip -- whole time steps and the random-finite-difference family (reference C++-only members).
// Part of the implementation of the C ABI in include/rbl.h (split from the former rbl_api.hip along its sections);
// shared internals are declared in rbl_api_internal.hpp.  Nothing here falls back to a CPU path.
//
// The stochastic midpoint scheme stands here once, for the all-free step and for the one with prescribed bodies (rbl_mixed.hip,
// which passes its mask and its solver): rhs_and_midpoint_core (right-hand side and predictor at q^n) and step_midpoint (save q^n,
// operators at q^{n+1/2}, solve, back to q^n, evolve).  So do the two ways of displacing by +- (delta/2) dq that the RFD family
// needs: at_displaced_config (the context's own configuration, restored afterwards) and on_displaced_copies (a copy of the body state).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "rbl_api_internal.hpp"

// ---- whole time steps in one call (what krylov.py's steppers do, for hosts without a Python driver) ----------

RblSizes sizes_of(const rbl_ctx *c)
{
  const size_t N = (size_t)c->S.N_bod * (size_t)c->S.N_blb, nb6 = 6 * (size_t)c->S.N_bod;
  return {N, 3 * N, nb6, 3 * N + nb6};
}

static int step_buffers(rbl_ctx *c, const RblSizes &z, double **rhs, double **x, double **slip, double **force)
{
  int rc = rbl_dev_reserve(c, c->d_step, sizeof(double) * (2 * z.nsys + z.n3 + z.nb6));
  if (rc) return rc;
  if (c->step_x_size != (int64_t)z.nsys) { c->step_hist_n = 0; c->step_x_size = (int64_t)z.nsys; }
  *x = (double *)c->d_step.p;
  *rhs = *x + z.nsys;
  *slip = *rhs + z.nsys;
  *force = *slip + z.n3;
  return RBL_OK;
}

// where the last rbl_step_deterministic / rbl_step_brownian left the body loads it solved with (F_body with the force model's
// share at q^n): the step with component masks echoes them when nothing is prescribed (rbl_mixed.hip)
const double *step_force_dev(const rbl_ctx *c)
{
  const RblSizes z = sizes_of(c);
  return (const double *)c->d_step.p + 2 * z.nsys + z.n3;
}

// ---- the stages the whole-step entry points share (rbl_api_internal.hpp) ---------------------------------------

int step_begin(rbl_ctx *c, const char *missing)
{
  int rc = flow_check(c, c->S.N_bod); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (missing) return rbl_fail(c, RBL_ERR_ARG, missing);
  flow_begin_step(c);
  return RBL_OK;
}

int step_slip(rbl_ctx *c, RblSide side, const double *slip, double *d_slip, bool model, bool *have_slip)
{
  int rc;
  *have_slip = slip != nullptr;
  if (slip && (rc = xfer_in(c, side, d_slip, slip, sizeof(double) * sizes_of(c).n3))) return rc;
  return model ? flow_add_to_step_slip(c, d_slip, have_slip) : RBL_OK;   // imposed flow and body slip at q^n (include/rbl.h section 8)
}

int step_inputs(rbl_ctx *c, const double *F_body, const double *slip, double *d_force, double *d_slip)
{
  const RblSizes z = sizes_of(c);
  bool have_slip;
  int rc = step_slip(c, RblSide::Host, slip, d_slip, true, &have_slip); if (rc) return rc;
  if (!have_slip) RBL_HIP(c, hipMemsetAsync(d_slip, 0, sizeof(double) * z.n3, c->stream));
  if ((rc = copy_h2d(c, d_force, F_body, sizeof(double) * z.nb6))) return rc;
  return ia_add_to_step_force(c, d_force);                               // the force model at q^n (include/rbl.h section 4)
}

int step_commit(rbl_ctx *c, const double *d_lambda, const double *d_U, double *U, const double *d_more, double *more, size_t n_more,
                bool check_flags)
{
  int rc = flow_record_moments(c, d_lambda); if (rc) return rc;
  if ((rc = copy_d2h(c, U, d_U, sizeof(double) * sizes_of(c).nb6))) return rc;
  if (more && (rc = copy_d2h(c, more, d_more, sizeof(double) * n_more))) return rc;
  if (check_flags) return finish_and_check(c);
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

// One deterministic time step on the object's own configuration: solve [M -K; K^T 0][lambda; U] = [slip; -F] by
// right-preconditioned GMRES (rbl_gmres_saddle_dev), then evolve_X_Q(U) (:865-878).  F = F_body - K^T f_phys(q^n) when the
// force model is on (rbl_set_interactions), F_body otherwise.  F_body: host, 6 N_bod;
// slip: host, 3 N_blobs, or NULL for zero.  warm_start: 0 cold; 1 start from the previous call's solution x_n; 2 from
// 2 x_n - x_{n-1}; 3 from 3 x_n - 3 x_{n-1} + x_{n-2} (as far as the history reaches): under a smooth forcing the solution
// moves smoothly with the configuration, and at cfg 3 GMRES then needs 12 / 6 / 2-3 iterations to 1e-8 instead of 18.
int rbl_step_deterministic(rbl_ctx *c, const double *F_body, const double *slip, int max_iter, double rtol,
                           int warm_start, int *iters, double *resid)
{
  int rc = need_K(c); if (rc) return rc;
  if ((rc = step_begin(c, F_body ? nullptr : "step_deterministic: F_body is NULL"))) return rc;
  const RblSizes z = sizes_of(c);
  double *rhs, *x, *dslip, *dforce;
  if ((rc = step_buffers(c, z, &rhs, &x, &dslip, &dforce))) return rc;
  if ((rc = step_inputs(c, F_body, slip, dforce, rhs))) return rc;     // the slip is the right-hand side's top as it stands
  rbl_launch_axpby(c->stream, (int64_t)z.nb6, -1.0, dforce, 0.0, nullptr, rhs + z.n3);
  if ((rc = rbl_dev_reserve(c, c->d_hist, sizeof(double) * 3 * z.nsys))) return rc;
  double *H = (double *)c->d_hist.p;
  auto slot = [&](int age) { return H + (size_t)((c->step_hist_head + age) % 3) * z.nsys; };   // age 0 = newest
  int order = warm_start < 0 ? 0 : (warm_start > 3 ? 3 : warm_start);
  if (order > c->step_hist_n) order = c->step_hist_n;
  if (order == 1) RBL_HIP(c, hipMemcpyAsync(x, slot(0), sizeof(double) * z.nsys, hipMemcpyDeviceToDevice, c->stream));
  if (order == 2) rbl_launch_axpby(c->stream, (int64_t)z.nsys, 2.0, slot(0), -1.0, slot(1), x);
  if (order == 3) {
    rbl_launch_axpby(c->stream, (int64_t)z.nsys, 3.0, slot(0), -3.0, slot(1), x);
    rbl_launch_axpby(c->stream, (int64_t)z.nsys, 1.0, x, 1.0, slot(2), x);
  }
  if ((rc = rbl_gmres_saddle_dev(c, rhs, max_iter, rtol, x, order > 0 ? 1 : 0, iters, resid))) { c->step_hist_n = 0; return rc; }
  c->step_hist_head = (c->step_hist_head + 2) % 3;                     // the oldest slot becomes the newest
  RBL_HIP(c, hipMemcpyAsync(slot(0), x, sizeof(double) * z.nsys, hipMemcpyDeviceToDevice, c->stream));
  if (c->step_hist_n < 3) ++c->step_hist_n;
  std::vector<double> U(z.nb6);
  if ((rc = step_commit(c, x, x + z.n3, U.data(), nullptr, nullptr, 0, false))) return rc;   // moments: lever arms of q^n
  return rbl_evolve_X_Q(c, U.data());
}

// the noise of a stochastic step on the device: *d_W = the host's W = [W1 | W2 | W_rfd] (9 N_blobs) uploaded into d_W, or NULL
// when W is NULL (the right-hand side then draws it from the seed)
int step_upload_W(rbl_ctx *c, const double *W, double **d_W)
{
  *d_W = nullptr;
  if (!W) return RBL_OK;
  const size_t bytes = sizeof(double) * 3 * sizes_of(c).n3;
  int rc = rbl_dev_reserve(c, c->d_W, bytes); if (rc) return rc;
  *d_W = (double *)c->d_W.p;
  return copy_h2d(c, *d_W, W, bytes);
}

// The stochastic midpoint scheme around its two solver-specific parts (reference :917-976): rhs(X_half, Q_half) leaves the
// right-hand side of q^n on the device and returns the predictor configuration; solve(U) solves at q^{n+1/2} and brings the body
// velocities (6 N_bod) to the host.  The update starts from q^n with dt U.
int step_midpoint(rbl_ctx *c, const std::function<int(double *, double *)> &rhs, const std::function<int(double *)> &solve)
{
  const int Nb = c->S.N_bod;
  c->step_hist_n = 0;                                       // the random part of the solution does not carry over
  const std::vector<double> Xn = c->S.X, Qn = c->S.Q;
  std::vector<double> Xh((size_t)3 * Nb), Qh((size_t)4 * Nb), U((size_t)6 * Nb);
  int rc = rhs(Xh.data(), Qh.data()); if (rc) return rc;
  if ((rc = rbl_set_config(c, Xh.data(), Qh.data(), Nb))) return rc;       // operators and lever arms at q^{n+1/2}
  rc = solve(U.data());
  const int rc2 = rbl_set_config(c, Xn.data(), Qn.data(), Nb);              // the update starts from q^n (also on failure)
  if (rc) return rc;
  if (rc2) return rc2;
  return rbl_evolve_X_Q(c, U.data());
}

// One stochastic midpoint step: right-hand side and predictor configuration at q^n (rbl_RHS_and_Midpoint_dev), saddle solve at
// q^{n+1/2} (step_midpoint).  W: host, [W1 | W2 | W_rfd] = 9 N_blobs standard normals, or NULL to draw them from `seed`.
int rbl_step_brownian(rbl_ctx *c, const double *F_body, const double *slip, const double *W, uint64_t seed, int method,
                      int split_rand, double delta, int max_iter, double rtol, int *iters, double *resid)
{
  int rc = need_K(c); if (rc) return rc;
  if ((rc = step_begin(c, F_body ? nullptr : "step_brownian: F_body is NULL"))) return rc;
  const RblSizes z = sizes_of(c);
  double *rhs, *x, *dslip, *dforce, *dW;
  if ((rc = step_buffers(c, z, &rhs, &x, &dslip, &dforce))) return rc;
  if ((rc = step_inputs(c, F_body, slip, dforce, dslip))) return rc;   // at q^n, where RHS_and_Midpoint takes its Slip and Force
  if ((rc = step_upload_W(c, W, &dW))) return rc;
  return step_midpoint(
      c,
      [&](double *Xh, double *Qh) { return rbl_RHS_and_Midpoint_dev(c, dslip, dforce, dW, seed, method, split_rand, delta, rhs, Xh, Qh); },
      [&](double *U) {
        const int r = rbl_gmres_saddle_dev(c, rhs, max_iter, rtol, x, 0, iters, resid);
        return r ? r : step_commit(c, x, x + z.n3, U, nullptr, nullptr, 0, false);   // moments: lever arms of q^{n+1/2}
      });
}

// ---- random finite differences (reference C++-only members) ---------------

// f(0) with the context's configuration at q + (delta/2) dq, then f(1) at q - (delta/2) dq (dq[6 N_bod], host; :783-788); q and
// the validity of its device copy are restored after each, whatever f returns.  The first failure ends it.
template <class Fn>
static int at_displaced_config(rbl_ctx *c, const double *dq, double delta, Fn &&f)
{
  RblBodyState &S = c->S;
  std::vector<double> win((size_t)6 * S.N_bod), Xs, Qs;
  const std::vector<double> X0 = S.X, Q0 = S.Q;
  for (int sgn = 0; sgn < 2; ++sgn) {
    const double h = (sgn == 0 ? 0.5 : -0.5) * delta;
    for (size_t i = 0; i < win.size(); ++i) win[i] = h * dq[i];
    rbl_body_update_X_Q(S, win.data(), Xs, Qs);
    S.X = Xs; S.Q = Qs; c->dev_xq_valid = false;                      // displaced configuration, temporarily
    const int rc = f(sgn);
    S.X = X0; S.Q = Q0; c->dev_xq_valid = false;
    if (rc) return rc;
  }
  return RBL_OK;
}

// The same on a copy of the body state with its K built (the host-side differences, :755-761, :853-859): f(T, w) with T at
// q + (delta/2) dq and w = 1/delta, then at q - (delta/2) dq with w = -1/delta.  The context is not touched.
template <class Fn>
static int on_displaced_copies(rbl_ctx *c, const double *dq, double delta, Fn &&f)
{
  const RblBodyState &S = c->S;
  std::vector<double> win((size_t)6 * S.N_bod);
  for (int sgn = 0; sgn < 2; ++sgn) {
    const double h = (sgn == 0 ? 0.5 : -0.5) * delta;
    for (size_t i = 0; i < win.size(); ++i) win[i] = h * dq[i];
    RblBodyState T = S;
    rbl_body_update_X_Q(S, win.data(), T.X, T.Q);
    const int rc = rbl_body_set_K(T, c->last_error); if (rc) return rc;
    f(T, (sgn == 0 ? 1.0 : -1.0) / delta);
  }
  return RBL_OK;
}

// d_out = (1/delta)[M(q + delta/2 dq) - M(q - delta/2 dq)] W for a displacement direction dq[6 N_bod] (host): the shared core of
// M_RFD (:776-794, dq = Kinv W), M_RFD_from_U (:820-842, dq = the caller's U) and the stochastic right-hand side (dq masked to
// the free bodies).  d_r: n3 scratch, d_work: 2 n3 scratch.
static int m_rfd_dir(rbl_ctx *c, const double *d_W, const double *dq, double delta, double *d_out, double *d_r, double *d_work)
{
  RblPhase ph_total(c, RBL_T_TOTAL);
  const int64_t N = (int64_t)sizes_of(c).N, n3 = 3 * N;
  double *dM[2] = {d_work, d_work + n3};
  const int rc = at_displaced_config(c, dq, delta, [&](int sgn) {
    const int r = positions_dev(c, 0, c->S.N_bod, d_r);
    return r ? r : apply_M_enqueue(c, c->S.wall, d_W, d_r, N, 0, N, dM[sgn]);          // :790-791
  });
  if (rc) return rc;
  rbl_launch_axpby(c->stream, n3, 1.0 / delta, dM[0], -1.0 / delta, dM[1], d_out);   // :793
  return RBL_OK;
}

// M_RFD (U == NULL: along Kinv W; W == NULL: drawn from the seed) and M_RFD_from_U (along the caller's U), checks done: W up, the two
// products on the GPU at the two displaced configurations, the quotient down
static int m_rfd_host(rbl_ctx *c, const double *W, uint64_t seed, const double *U, double delta, double *out)
{
  const size_t n3 = sizes_of(c).n3, vb = sizeof(double) * n3;
  int rc;
  if ((rc = rbl_dev_reserve(c, c->d_W, vb))) return rc;
  if ((rc = rbl_dev_reserve(c, c->d_r, vb))) return rc;
  if ((rc = rbl_dev_reserve(c, c->d_U, 2 * vb))) return rc;
  std::vector<double> Wh, uom;
  if (W) {
    if ((rc = copy_h2d(c, c->d_W.p, W, vb))) return rc;
  } else {  // rand_vector (:730-741) replaced by the seeded device generator
    Wh.resize(n3);
    rbl_launch_normal(c->stream, seed, 0, (int64_t)n3, (double *)c->d_W.p);
    if ((rc = copy_d2h(c, Wh.data(), c->d_W.p, vb))) return rc;
    RBL_HIP(c, hipStreamSynchronize(c->stream));
    W = Wh.data();
  }
  if (!U) {
    uom.resize((size_t)6 * c->S.N_bod);
    rbl_body_Kinv_x_V(c->S, W, uom.data());                          // UOM = Kinv W (:776), O(N) host work
    U = uom.data();
  }
  double *dU = (double *)c->d_U.p;
  if ((rc = m_rfd_dir(c, (const double *)c->d_W.p, U, delta, dU, (double *)c->d_r.p, dU))) return rc;
  if ((rc = copy_d2h(c, out, dU, vb))) return rc;
  return finish_and_check(c);
}

// M_RFD(), c_rigid_obj.cpp:769-796
int rbl_M_RFD(rbl_ctx *c, const double *W, uint64_t seed, double delta, double *out)
{
  int rc = need_K(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!(delta > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "M_RFD: delta must be positive");
  return m_rfd_host(c, W, seed, nullptr, delta, out);
}

// update_X_Q(U), c_rigid_obj.cpp:798-863: the configuration displaced by U (displacement units: translation
// and rotation vector per body), WITHOUT committing it.
int rbl_update_X_Q(rbl_ctx *c, const double *U, double *X_out, double *Q_out)
{
  int rc = need_config(c); if (rc) return rc;
  if (!U || !X_out || !Q_out) return rbl_fail(c, RBL_ERR_ARG, "update_X_Q: null argument");
  std::vector<double> Xo, Qo;
  rbl_body_update_X_Q(c->S, U, Xo, Qo);
  std::memcpy(X_out, Xo.data(), sizeof(double) * Xo.size());
  std::memcpy(Q_out, Qo.data(), sizeof(double) * Qo.size());
  return RBL_OK;
}

// Right-hand side and predictor of the stochastic midpoint step at q^n (c_rigid_obj.cpp:917-976), with any subset of the velocity
// components prescribed (include/rbl.h section 7); the all-free scheme is the one with no mask.  Checks done by the caller, dt and
// delta positive when kBT > 1e-10 among them.  h_mask / d_mask: the 0/1 mask on the host and on the device, d_body_in: the
// prescribed components' velocities in their slots -- all three NULL: every body is free.  per: mask entries per body, 1 (whole
// bodies: none or all six of a body's components) or 6 (one per lab-frame velocity component, every body's rotation entries all
// equal: the caller has checked it).  ONE path for both: k_mx_bd_sums decodes the mask on the device, the loop below on the host;
// D_f and D_p are diagonal 0/1 over the 6 N_bod slots.  d_slip: 3 N_blobs or NULL for zero; d_W: [W1 | W2 | W_rfd] (3 n3) or NULL
// (drawn from `seed`).
//   d_s (3 N_blobs, may be d_slip) = slip - kBT M_RFD - BI,  M_RFD along dq = D_f Kinv W_rfd,
//   q^{n+1/2} = q^n displaced by D_f (dt/2 c1) Kinv M^{1/2}W1 + D_p (dt/2) U_p.
// M is all blobs': the mask does not enter the square roots.  One read-back of 12 numbers per body (18 with a mask: U_p echoed).
int rhs_and_midpoint_core(rbl_ctx *c, const uint8_t *h_mask, const uint8_t *d_mask, const double *d_body_in, const double *d_slip,
                          const double *d_W, uint64_t seed, int method, int split_rand, double delta, double *d_s, double *X_half,
                          double *Q_half, int per)
{
  RblBodyState &S = c->S;
  const RblSizes z = sizes_of(c);
  const int64_t N = (int64_t)z.N, n3 = (int64_t)z.n3, nb6 = (int64_t)z.nb6;
  const size_t vb = sizeof(double) * z.n3;
  int rc;
  if (!d_slip) {
    RBL_HIP(c, hipMemsetAsync(d_s, 0, vb, c->stream));
    d_slip = d_s;
  }
  if (!(S.kBT > 1e-10)) {                                                              // no Brownian terms (:967-970)
    if (d_slip != d_s) RBL_HIP(c, hipMemcpyAsync(d_s, d_slip, vb, hipMemcpyDeviceToDevice, c->stream));
    std::memcpy(X_half, S.X.data(), sizeof(double) * S.X.size());
    std::memcpy(Q_half, S.Q.data(), sizeof(double) * S.Q.size());
    return finish_and_check(c);
  }
  if (method == RBL_MHALF_CHOLESKY && (rc = periodic_refuse(c, "Brownian step with the dense Cholesky root"))) return rc;
  // workspace: [W1 | W2 | W_rfd] (when drawn here), M^{1/2}W1, M^{1/2}W2, M_RFD, positions, 2 scratch, the sums per body
  if ((rc = rbl_dev_reserve(c, c->d_bd, 9 * vb + (d_mask ? 3 : 2) * sizeof(double) * (size_t)nb6))) return rc;
  double *base = (double *)c->d_bd.p;
  double *dWown = base, *dMW = base + 3 * n3 /* 2 vectors */, *dRFD = base + 5 * n3, *dr = base + 6 * n3,
         *dwork = base + 7 * n3, *dt12 = base + 9 * n3;
  if (!d_W) {                                                                          // rand_vector (:730-741)
    rbl_launch_normal(c->stream, seed, 0, 3 * n3, dWown);
    d_W = dWown;
  }
  if ((rc = positions_dev(c, 0, S.N_bod, dr))) return rc;                              // multi_body_pos (:662)
  if ((rc = mhalf_dev_multi(c, dr, N, d_W, split_rand ? 2 : 1, method, dMW))) return rc;   // M_half_W1/2 (:927-936)
  // Kinv of the RFD noise (M_RFD's direction, :776) and of M^{1/2}W1 (the predictor, :955): the sums over the blobs on the device
  // with the lever arms of q^n, the 6 x 6 blocks on the host after one small read-back (the reference brings the 3 N-vectors, :408)
  if ((rc = sync_bodies(c))) return rc;
  rbl_launch_mx_bd_sums(c->stream, (const double *)c->d_lever.p, d_mask, per, d_body_in, d_W + 2 * n3, dMW, S.N_blb, S.N_bod, dt12);
  std::vector<double> t((size_t)((d_mask ? 3 : 2) * nb6)), dq((size_t)nb6), pre((size_t)nb6), Xo, Qo;
  if ((rc = read_back(c, t.data(), dt12, sizeof(double) * t.size()))) return rc;
  const double c1 = split_rand ? 2.0 * std::sqrt(S.kBT / S.dt) : std::sqrt(2.0 * S.kBT / S.dt);   // :945-952
  const double c2 = split_rand ? std::sqrt(S.kBT / S.dt) : std::sqrt(2.0 * S.kBT / S.dt);
  const double half_dt = 0.5 * S.dt, scale = half_dt * c1;
  for (int b = 0; b < S.N_bod; ++b) {
    const double *Kb = &S.KTKinv[(size_t)36 * b], *tr = t.data() + 6 * (size_t)b, *tp = tr + nb6;
    const uint8_t *hm = h_mask ? h_mask + (size_t)per * b : nullptr;                    // the body's per mask entries
    for (int p = 0; p < 6; ++p) {
      double sr = 0.0, sp = 0.0;
      for (int q = 0; q < 6; ++q) { sr += Kb[6 * p + q] * tr[q]; sp += Kb[6 * p + q] * tp[q]; }
      const bool pres = hm && hm[p % per] != 0;                                         // component p: its own entry of six, or the body's one
      dq[6 * (size_t)b + p] = pres ? 0.0 : sr;                                          // D_f Kinv W_rfd
      pre[6 * (size_t)b + p] = pres ? half_dt * tp[nb6 + p] : scale * sp;               // (:955-959) and D_p (dt/2) U_p: the third block
    }
  }
  if ((rc = m_rfd_dir(c, d_W + 2 * n3, dq.data(), delta, dRFD, dr, dwork))) return rc;  // M_RFD (:940)
  // Slip -= kBT M_RFD + BI,  BI = c2 (M^{1/2}W1 - M^{1/2}W2)  or  c2 M^{1/2}W1   (:948,953,963)
  rbl_launch_rhs_combine(c->stream, n3, d_slip, S.kBT, dRFD, c2, dMW, split_rand ? dMW + n3 : nullptr, d_s);
  rbl_body_update_X_Q(S, pre.data(), Xo, Qo);
  std::memcpy(X_half, Xo.data(), sizeof(double) * Xo.size());
  std::memcpy(Q_half, Qo.data(), sizeof(double) * Qo.size());
  return finish_and_check(c);
}

// RHS_and_Midpoint(Slip, Force), c_rigid_obj.cpp:917-976 -- device-resident form.  d_W = [W1 | W2 | W_rfd]
// (3 n3) or NULL (drawn from `seed`).  d_RHS = [Slip - (kBT M_RFD + BI) ; -Force]  (n3 + 6 N_bod).
int rbl_RHS_and_Midpoint_dev(rbl_ctx *c, const double *d_Slip, const double *d_Force, const double *d_W,
                             uint64_t seed, int method, int split_rand, double delta, double *d_RHS,
                             double *X_half, double *Q_half)
{
  int rc = need_K(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!d_Slip || !d_Force || !d_RHS || !X_half || !Q_half) return rbl_fail(c, RBL_ERR_ARG, "RHS_and_Midpoint: null argument");
  const RblBodyState &S = c->S;
  const RblSizes z = sizes_of(c);
  rbl_launch_axpby(c->stream, (int64_t)z.nb6, -1.0, d_Force, 0.0, nullptr, d_RHS + z.n3);          // Force *= -1 (:972)
  if (S.kBT > 1e-10 && (!(S.dt > 0.0) || !(delta > 0.0)))
    return rbl_fail(c, RBL_ERR_ARG, "RHS_and_Midpoint: dt and delta must be positive");
  return rhs_and_midpoint_core(c, nullptr, nullptr, nullptr, d_Slip, d_W, seed, method, split_rand, delta, d_RHS, X_half, Q_half);
}

// host-pointer form of the same
int rbl_RHS_and_Midpoint(rbl_ctx *c, const double *Slip, const double *Force, const double *W, uint64_t seed,
                         int method, int split_rand, double delta, double *RHS, double *X_half, double *Q_half)
{
  int rc = need_K(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!Slip || !Force || !RHS) return rbl_fail(c, RBL_ERR_ARG, "RHS_and_Midpoint: null argument");
  const size_t n3 = sizes_of(c).n3, nb6 = sizes_of(c).nb6, vb = sizeof(double) * n3, fb = sizeof(double) * nb6;
  if ((rc = rbl_dev_reserve(c, c->d_bd2, (W ? 4 : 1) * vb + 2 * (vb + fb)))) return rc;
  double *dSlip = (double *)c->d_bd2.p, *dForce = dSlip + n3, *dRHS = dForce + nb6, *dW = dRHS + n3 + nb6;
  if ((rc = copy_h2d(c, dSlip, Slip, vb))) return rc;
  if ((rc = copy_h2d(c, dForce, Force, fb))) return rc;
  if (W && (rc = copy_h2d(c, dW, W, 3 * vb))) return rc;
  if ((rc = rbl_RHS_and_Midpoint_dev(c, dSlip, dForce, W ? dW : nullptr, seed, method, split_rand, delta, dRHS,
                                     X_half, Q_half))) return rc;
  if ((rc = copy_d2h(c, RHS, dRHS, vb + fb))) return rc;
  return finish_and_check(c);
}

// KTinv_RFD(), c_rigid_obj.cpp:743-767:  K^T (1/delta) [ Kinv(q+)^T - Kinv(q-)^T ] W, W of length 6 N_bod
int rbl_KTinv_RFD(rbl_ctx *c, const double *W, double delta, double *out)
{
  int rc = need_K(c); if (rc) return rc;
  if (!W || !(delta > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "KTinv_RFD: need W and delta > 0");
  const size_t n3 = sizes_of(c).n3;
  std::vector<double> acc(n3, 0.0), tmp(n3);
  rc = on_displaced_copies(c, W, delta, [&](const RblBodyState &T, double w) {
    rbl_body_KTinv_x_F(T, W, tmp.data());
    for (size_t i = 0; i < n3; ++i) acc[i] += w * tmp[i];            // :763-764
  });
  if (rc) return rc;
  rbl_body_KT_x_Lam(c->S, acc.data(), out);                          // :766
  return RBL_OK;
}

// M_RFD_from_U(U, W), c_rigid_obj.cpp:820-842: the same random finite difference along the caller's displacement U[6 N_bod]
int rbl_M_RFD_from_U(rbl_ctx *c, const double *U, const double *W, double delta, double *out)
{
  int rc = need_config(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!U || !W || !out || !(delta > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "M_RFD_from_U: need U, W, out and delta > 0");
  return m_rfd_host(c, W, 0, U, delta, out);
}

// M_RFD_cfgs(U, delta), c_rigid_obj.cpp:798-818: blob positions at q +- (delta/2) U
int rbl_M_RFD_cfgs(rbl_ctx *c, const double *U, double delta, double *r_plus, double *r_minus)
{
  int rc = need_config(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!U || !r_plus || !r_minus) return rbl_fail(c, RBL_ERR_ARG, "M_RFD_cfgs: null argument");
  const size_t vb = sizeof(double) * sizes_of(c).n3;
  if ((rc = rbl_dev_reserve(c, c->d_r, vb))) return rc;
  return at_displaced_config(c, U, delta, [&](int sgn) {               // :808, :811
    int r = positions_dev(c, 0, c->S.N_bod, (double *)c->d_r.p);
    if (!r) r = copy_d2h(c, sgn == 0 ? r_plus : r_minus, c->d_r.p, vb);
    if (!r && hipStreamSynchronize(c->stream) != hipSuccess) r = RBL_ERR_HIP;
    return r;
  });
}

// KT_RFD_from_U(U, W), c_rigid_obj.cpp:844-863: (1/delta) [K(q+)^T - K(q-)^T] W, W[3N] -> out[6 N_bod] (O(N) host work)
int rbl_KT_RFD_from_U(rbl_ctx *c, const double *U, const double *W, double delta, double *out)
{
  int rc = need_K(c); if (rc) return rc;
  if (!U || !W || !out || !(delta > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "KT_RFD_from_U: need U, W, out and delta > 0");
  const size_t nb6 = sizes_of(c).nb6;
  std::vector<double> tmp(nb6);
  for (size_t i = 0; i < nb6; ++i) out[i] = 0.0;
  return on_displaced_copies(c, U, delta, [&](const RblBodyState &T, double w) {
    rbl_body_KT_x_Lam(T, W, tmp.data());
    for (size_t i = 0; i < nb6; ++i) out[i] += w * tmp[i];           // :861
  });
}

// evolve_X_Q_RFD(U), c_rigid_obj.cpp:880-893: commit q displaced by U (displacement units), rebuild K, KEEP the
// preconditioner (:892 PC_mat_Set = true): the factors of q go on serving q + U, whose size is an RFD delta.
int rbl_evolve_X_Q_RFD(rbl_ctx *c, const double *U)
{
  int rc = need_config(c); if (rc) return rc;
  if (!U) return rbl_fail(c, RBL_ERR_ARG, "evolve_X_Q_RFD: U is NULL");
  RblBodyState &S = c->S;
  std::vector<double> Xo, Qo;
  rbl_body_update_X_Q(S, U, Xo, Qo);                                  // :886 (no dt)
  S.X.swap(Xo);
  S.Q.swap(Qo);
  c->dev_bodies_valid = false; c->dev_xq_valid = false;
  c->pc_keep_once = c->dev_pc_valid;                                  // the next re-synchronisation leaves the device preconditioner alone
  return rbl_body_set_K(S, c->last_error);                            // :891; S.pc_set is left as it is (:892)
}
