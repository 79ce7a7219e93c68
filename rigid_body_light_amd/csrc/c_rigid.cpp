// c_rigid.cpp -- pybind11 module `c_rigid` exposing class CManyBodies with the
// same Python-visible names as the reference's nanobind module
// (reference src/c_rigid_obj.cpp:997-1027).  It is a thin shim: every method
// calls one extern "C" entry point of include/rbl.h (librbl.so) and nothing else.
//
// Differences a caller can observe (all listed in DESIGN.md):
//   * multi_body_pos() returns a numpy array instead of a Python list (the
//     reference wrapper wraps it in np.array() anyway, src/Rigid.py:55);
//   * error conditions that make the reference exit() raise RuntimeError;
//   * inputs are never modified (the reference mutates `cfg` and `U` C++-side).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rbl.h"

namespace py = pybind11;
using darr = py::array_t<double, py::array::c_style | py::array::forcecast>;

namespace {

static int mhalf_method(const std::string &method)
{
  if (method == "cholesky") return RBL_MHALF_CHOLESKY;
  if (method == "lanczos") return RBL_MHALF_LANCZOS;
  if (method == "lanczos_pc") return RBL_MHALF_LANCZOS_PC;
  throw std::runtime_error("M_half_W: method must be 'cholesky', 'lanczos' or 'lanczos_pc'");
}

struct CManyBodies {
  rbl_ctx *ctx;
  CManyBodies() : ctx(rbl_create())
  {
    if (!ctx) throw std::runtime_error("rbl_create failed");
  }
  ~CManyBodies() { rbl_destroy(ctx); }
  CManyBodies(const CManyBodies &) = delete;
  CManyBodies &operator=(const CManyBodies &) = delete;

  void check(int rc) const
  {
    if (rc != RBL_OK) throw std::runtime_error(std::string(rbl_last_error(ctx)) + " [rbl status " + std::to_string(rc) + "]");
  }
  int n_bod() const { int a = 0, b = 0; rbl_get_sizes(ctx, &a, &b); return a; }
  int n_blb() const { int a = 0, b = 0; rbl_get_sizes(ctx, &a, &b); return b; }
  py::ssize_t n3() const { return (py::ssize_t)3 * n_bod() * n_blb(); }

  // setParameters(a, dt, kBT, eta, cfg)   reference :183
  void setParameters(double a, double dt, double kBT, double eta, darr cfg)
  {
    if (cfg.size() % 3 != 0) throw std::runtime_error("Rigid config must have length 3N");
    check(rbl_set_parameters(ctx, a, dt, kBT, eta, cfg.data(), (int)(cfg.size() / 3)));
  }
  void setBlkPC(bool v) { check(rbl_set_blk_pc(ctx, v)); }      // :197
  void setWallPC(bool v) { check(rbl_set_wall_pc(ctx, v)); }    // :199

  void setConfig(darr X, darr Q)                                 // :201
  {
    if (X.size() % 3 != 0 || Q.size() != 4 * (X.size() / 3))
      throw std::runtime_error("setConfig: X must have length 3*N_bod and Q length 4*N_bod");
    check(rbl_set_config(ctx, X.data(), Q.data(), (int)(X.size() / 3)));
  }

  py::tuple getConfig()                                          // :235
  {
    const int nb = n_bod();
    darr X(3 * (py::ssize_t)nb), Q(4 * (py::ssize_t)nb);
    check(rbl_get_config(ctx, X.mutable_data(), Q.mutable_data()));
    return py::make_tuple(X, Q);
  }

  void set_K_mats() { check(rbl_set_K_mats(ctx)); }              // :395

  darr K_x_U(darr U)                                             // :404
  {
    if (U.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("K_x_U: U must have length 6*N_bod");
    darr out(n3());
    check(rbl_K_x_U(ctx, U.data(), out.mutable_data()));
    return out;
  }

  darr KT_x_Lam(darr lam)                                        // :410
  {
    if (lam.size() != n3()) throw std::runtime_error("KT_x_Lam: lambda must have length 3*N_blobs");
    darr out(6 * (py::ssize_t)n_bod());
    check(rbl_KT_x_Lam(ctx, lam.data(), out.mutable_data()));
    return out;
  }

  darr multi_body_pos()                                          // :295
  {
    darr out(n3());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_multi_body_pos(ctx, out.mutable_data());
    }
    check(rc);
    return out;
  }

  darr apply_PC(darr in)                                         // :589
  {
    const py::ssize_t n = n3() + 6 * (py::ssize_t)n_bod();
    if (in.size() != n) throw std::runtime_error("apply_PC: input must have length 3*N_blobs + 6*N_bod");
    darr out(n);
    check(rbl_apply_PC(ctx, in.data(), out.mutable_data()));
    return out;
  }

  py::object csc(bool inverse)                                   // get_K :978 / get_Kinv :986
  {
    int64_t nnz = 0, nr = 0, nc = 0;
    auto fn = inverse ? rbl_get_Kinv_csc : rbl_get_K_csc;
    check(fn(ctx, &nnz, &nr, &nc, nullptr, nullptr, nullptr));
    py::array_t<double> data(nnz);
    py::array_t<int32_t> indices(nnz), indptr(nc + 1);
    check(fn(ctx, &nnz, &nr, &nc, data.mutable_data(), indices.mutable_data(), indptr.mutable_data()));
    py::object csc_matrix = py::module_::import("scipy.sparse").attr("csc_matrix");
    return csc_matrix(py::make_tuple(data, indices, indptr), py::arg("shape") = py::make_tuple(nr, nc));
  }
  py::object get_K() { return csc(false); }
  py::object get_Kinv() { return csc(true); }

  void evolve_X_Q(darr U)                                        // :865
  {
    if (U.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("evolve_X_Q: U must have length 6*N_bod");
    check(rbl_evolve_X_Q(ctx, U.data()));
  }

  darr apply_M(darr F, darr r_vecs)                              // :641
  {
    if (F.size() != r_vecs.size()) throw std::runtime_error("Positions and forces must be of the same size");
    darr out(F.size());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_apply_M(ctx, F.data(), r_vecs.data(), (int64_t)F.size(), out.mutable_data());
    }
    check(rc);
    return out;
  }

  // ---- extensions (not in the reference's Python surface) -------------------
  darr apply_M_multi(darr F, darr r_vecs)  // F: (nrhs, n3) C-order = n3 x nrhs column-major
  {
    if (F.ndim() != 2 || F.shape(1) != r_vecs.size()) throw std::runtime_error("apply_M_multi: F must be (nrhs, 3N)");
    darr out({F.shape(0), F.shape(1)});
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_apply_M_multi(ctx, F.data(), r_vecs.data(), (int64_t)r_vecs.size(), (int)F.shape(0), out.mutable_data());
    }
    check(rc);
    return out;
  }

  darr M_half_W(py::object W, uint64_t seed, const std::string &method)   // :661 (unbound in the reference)
  {
    const int m = mhalf_method(method);
    darr out(n3());
    int rc;
    if (W.is_none()) {
      py::gil_scoped_release rel;
      rc = rbl_M_half_W(ctx, nullptr, seed, m, out.mutable_data());
    } else {
      darr Wa = W.cast<darr>();
      if (Wa.size() != n3()) throw std::runtime_error("M_half_W: W must have length 3*N_blobs");
      py::gil_scoped_release rel;
      rc = rbl_M_half_W(ctx, Wa.data(), seed, m, out.mutable_data());
    }
    check(rc);
    return out;
  }

  darr M_half_W_r(darr r_vecs, darr W, const std::string &method)
  {
    const int m = mhalf_method(method);
    if (W.size() != r_vecs.size()) throw std::runtime_error("M_half_W_r: W and r_vecs must have the same length");
    darr out(W.size());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_M_half_W_r(ctx, r_vecs.data(), (int64_t)r_vecs.size(), W.data(), 0, m, out.mutable_data());
    }
    check(rc);
    return out;
  }

  darr M_RFD(py::object W, uint64_t seed, double delta)             // :769 (unbound in the reference)
  {
    darr out(n3());
    int rc;
    if (W.is_none()) {
      py::gil_scoped_release rel;
      rc = rbl_M_RFD(ctx, nullptr, seed, delta, out.mutable_data());
    } else {
      darr Wa = W.cast<darr>();
      if (Wa.size() != n3()) throw std::runtime_error("M_RFD: W must have length 3*N_blobs");
      py::gil_scoped_release rel;
      rc = rbl_M_RFD(ctx, Wa.data(), seed, delta, out.mutable_data());
    }
    check(rc);
    return out;
  }

  darr KTinv_RFD(darr W, double delta)                              // :743 (unbound in the reference)
  {
    if (W.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("KTinv_RFD: W must have length 6*N_bod");
    darr out(6 * (py::ssize_t)n_bod());
    check(rbl_KTinv_RFD(ctx, W.data(), delta, out.mutable_data()));
    return out;
  }

  py::tuple update_X_Q(darr U)                                      // :798 (unbound in the reference)
  {
    if (U.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("update_X_Q: U must have length 6*N_bod");
    darr X(3 * (py::ssize_t)n_bod()), Q(4 * (py::ssize_t)n_bod());
    check(rbl_update_X_Q(ctx, U.data(), X.mutable_data(), Q.mutable_data()));
    return py::make_tuple(X, Q);
  }

  // whole time steps inside librbl (no counterpart in the reference, which ships no driver) -> (iterations, residual)
  py::tuple step_deterministic(darr F, py::object slip, int max_iter, double rtol, int warm_start)
  {
    if (F.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("step_deterministic: F must have length 6*N_bod");
    darr sl;
    const double *sp = nullptr;
    if (!slip.is_none()) {
      sl = slip.cast<darr>();
      if (sl.size() != n3()) throw std::runtime_error("step_deterministic: slip must have length 3*N_blobs");
      sp = sl.data();
    }
    int it = 0, rc; double res = 0.0;
    {
      py::gil_scoped_release rel;
      rc = rbl_step_deterministic(ctx, F.data(), sp, max_iter, rtol, warm_start, &it, &res);
    }
    check(rc);
    return py::make_tuple(it, res);
  }

  py::tuple step_brownian(darr F, py::object slip, py::object W, uint64_t seed, const std::string &method, bool split_rand,
                          double delta, int max_iter, double rtol)
  {
    if (F.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("step_brownian: F must have length 6*N_bod");
    darr sl, Wa;
    const double *sp = nullptr, *wp = nullptr;
    if (!slip.is_none()) {
      sl = slip.cast<darr>();
      if (sl.size() != n3()) throw std::runtime_error("step_brownian: slip must have length 3*N_blobs");
      sp = sl.data();
    }
    if (!W.is_none()) {
      Wa = W.cast<darr>();
      if (Wa.size() != 3 * n3()) throw std::runtime_error("step_brownian: W must have length 9*N_blobs (W1|W2|W_rfd)");
      wp = Wa.data();
    }
    const int m = mhalf_method(method);
    int it = 0, rc; double res = 0.0;
    {
      py::gil_scoped_release rel;
      rc = rbl_step_brownian(ctx, F.data(), sp, wp, seed, m, split_rand ? 1 : 0, delta, max_iter, rtol, &it, &res);
    }
    check(rc);
    return py::make_tuple(it, res);
  }

  // RHS_and_Midpoint(Slip, Force) :917 (unbound in the reference) -> (RHS, X_half, Q_half)
  py::tuple RHS_and_Midpoint(darr Slip, darr Force, py::object W, uint64_t seed, const std::string &method,
                             bool split_rand, double delta)
  {
    const py::ssize_t nb = n_bod();
    if (Slip.size() != n3()) throw std::runtime_error("RHS_and_Midpoint: Slip must have length 3*N_blobs");
    if (Force.size() != 6 * nb) throw std::runtime_error("RHS_and_Midpoint: Force must have length 6*N_bod");
    const int m = mhalf_method(method);
    darr RHS(n3() + 6 * nb), X(3 * nb), Q(4 * nb);
    darr Wa;
    const double *Wp = nullptr;
    if (!W.is_none()) {
      Wa = W.cast<darr>();
      if (Wa.size() != 3 * n3()) throw std::runtime_error("RHS_and_Midpoint: W must have length 9*N_blobs (W1|W2|W_rfd)");
      Wp = Wa.data();
    }
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_RHS_and_Midpoint(ctx, Slip.data(), Force.data(), Wp, seed, m, split_rand ? 1 : 0, delta,
                                RHS.mutable_data(), X.mutable_data(), Q.mutable_data());
    }
    check(rc);
    return py::make_tuple(RHS, X, Q);
  }

  py::tuple lanczos_report()
  {
    int it = 0; double res = 0;
    rbl_get_lanczos_report(ctx, &it, &res);
    return py::make_tuple(it, res);
  }
  void set_lanczos(int max_iter, double tol) { check(rbl_set_lanczos(ctx, max_iter, tol)); }

  darr rotne_prager_tensor(darr r_vecs, bool scale_damp)       // :413 -> (n3, n3) column-major
  {
    const py::ssize_t n = r_vecs.size();
    py::array_t<double, py::array::f_style> out({n, n});
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_rotne_prager_tensor(ctx, r_vecs.data(), (int64_t)n, scale_damp, out.mutable_data());
    }
    check(rc);
    return out;
  }

  py::array cholesky_lower(py::array_t<double, py::array::f_style | py::array::forcecast> M)
  {
    if (M.ndim() != 2 || M.shape(0) != M.shape(1)) throw std::runtime_error("cholesky_lower: square matrix expected");
    py::array_t<double, py::array::f_style> A({M.shape(0), M.shape(1)});
    std::memcpy(A.mutable_data(), M.data(), sizeof(double) * (size_t)M.size());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_cholesky_lower(ctx, A.mutable_data(), (int64_t)M.shape(0));
    }
    check(rc);
    return A;
  }

  darr pair_blocks(darr ri, darr rj, py::array_t<int32_t, py::array::c_style | py::array::forcecast> ii,
                   py::array_t<int32_t, py::array::c_style | py::array::forcecast> jj, bool wall, int mode)
  {
    const py::ssize_t n = ii.size();
    if (ri.size() != 3 * n || rj.size() != 3 * n || jj.size() != n) throw std::runtime_error("pair_blocks: size mismatch");
    darr out({n, (py::ssize_t)3, (py::ssize_t)3});
    check(rbl_debug_pair_blocks(ctx, ri.data(), rj.data(), ii.data(), jj.data(), (int64_t)n, wall, mode, out.mutable_data()));
    return out;
  }

  // [M lambda - K U ; K^T lambda], src/Rigid.py:73-80 in ONE boundary crossing
  darr apply_saddle(darr x)
  {
    const py::ssize_t n = n3() + 6 * (py::ssize_t)n_bod();
    if (x.size() != n) throw std::runtime_error("apply_saddle: input must have length 3*N_blobs + 6*N_bod");
    darr out(n);
    check(rbl_apply_saddle(ctx, x.data(), out.mutable_data()));
    return out;
  }

  // right-preconditioned GMRES on the saddle operator inside the library (host vectors) -> (x, iterations, residual estimate)
  py::tuple solve_saddle(darr rhs, int max_iter, double rtol, py::object x0)
  {
    const py::ssize_t n = n3() + 6 * (py::ssize_t)n_bod();
    if (rhs.size() != n) throw std::runtime_error("solve_saddle: rhs must have length 3*N_blobs + 6*N_bod");
    darr x(n);
    int use_x0 = 0;
    if (!x0.is_none()) {
      darr g = x0.cast<darr>();
      if (g.size() != n) throw std::runtime_error("solve_saddle: x0 must have length 3*N_blobs + 6*N_bod");
      std::memcpy(x.mutable_data(), g.data(), sizeof(double) * (size_t)n);
      use_x0 = 1;
    }
    int it = 0;
    double res = 0.0;
    check(rbl_gmres_saddle(ctx, rhs.data(), max_iter, rtol, x.mutable_data(), use_x0, &it, &res));
    return py::make_tuple(x, it, res);
  }

  // nrhs right-hand sides in lock step (rhs: (nrhs, 3 N_blobs + 6 N_bod)): products on the fp64 matrix cores, 16 at a time
  py::tuple solve_saddle_multi(darr rhs, int max_iter, double rtol)
  {
    const py::ssize_t n = n3() + 6 * (py::ssize_t)n_bod();
    if (rhs.ndim() != 2 || rhs.shape(1) != n || rhs.shape(0) < 1)
      throw std::runtime_error("solve_saddle_multi: rhs must have shape (nrhs, 3*N_blobs + 6*N_bod)");
    const int nrhs = (int)rhs.shape(0);
    darr x({(py::ssize_t)nrhs, n});
    py::array_t<int> its(nrhs);
    darr res(nrhs);
    check(rbl_gmres_saddle_multi(ctx, rhs.data(), nrhs, max_iter, rtol, x.mutable_data(), its.mutable_data(), res.mutable_data()));
    return py::make_tuple(x, its, res);
  }

  py::tuple M_RFD_cfgs(darr U, double delta)                        // :798 (unbound in the reference)
  {
    if (U.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("M_RFD_cfgs: U must have length 6*N_bod");
    darr rp(n3()), rm(n3());
    check(rbl_M_RFD_cfgs(ctx, U.data(), delta, rp.mutable_data(), rm.mutable_data()));
    return py::make_tuple(rp, rm);
  }

  darr M_RFD_from_U(darr U, darr W, double delta)                   // :820 (unbound in the reference)
  {
    if (U.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("M_RFD_from_U: U must have length 6*N_bod");
    if (W.size() != n3()) throw std::runtime_error("M_RFD_from_U: W must have length 3*N_blobs");
    darr out(n3());
    check(rbl_M_RFD_from_U(ctx, U.data(), W.data(), delta, out.mutable_data()));
    return out;
  }

  darr KT_RFD_from_U(darr U, darr W, double delta)                  // :844 (unbound in the reference)
  {
    if (U.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("KT_RFD_from_U: U must have length 6*N_bod");
    if (W.size() != n3()) throw std::runtime_error("KT_RFD_from_U: W must have length 3*N_blobs");
    darr out(6 * (py::ssize_t)n_bod());
    check(rbl_KT_RFD_from_U(ctx, U.data(), W.data(), delta, out.mutable_data()));
    return out;
  }

  void evolve_X_Q_RFD(darr U)                                       // :880 (unbound in the reference)
  {
    if (U.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error("evolve_X_Q_RFD: U must have length 6*N_bod");
    check(rbl_evolve_X_Q_RFD(ctx, U.data()));
  }

  // configuration-dependent forces (include/rbl.h section 4; the reference has none)
  // fluid velocity at points[3P] from blob forces lambda[3N] on blobs r_vecs[3N] (None: the object's own blobs)
  darr velocity_field(darr points, darr lambda, py::object r_vecs)
  {
    if (points.size() % 3 != 0 || lambda.size() % 3 != 0) throw std::runtime_error("velocity_field: points and lambda must have length 3P, 3N");
    darr r;
    const bool own = r_vecs.is_none();
    if (!own) {
      r = darr::ensure(r_vecs);
      if (!r || r.size() != lambda.size()) throw std::runtime_error("velocity_field: r_vecs and lambda must be of the same size");
    }
    darr out(points.size());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_velocity_field(ctx, points.data(), (int64_t)(points.size() / 3), lambda.data(), own ? nullptr : r.data(),
                              (int64_t)(lambda.size() / 3), out.mutable_data());
    }
    check(rc);
    return out;
  }
  // prescribed kinematics (include/rbl.h section 7): mask[N_bod] 0/1, body_in[6 N_bod] loads of the free bodies / velocities of the
  // prescribed ones -> (lambda, U, F, iterations, residual estimate).  per: mask entries per body, 1, or 6 for a mask per velocity
  // component in body_in's order (the _dof methods, which call the _dof entry points); one body serves each pair of methods
  using marr = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;
  [[noreturn]] static void bad_mixed_arg(int per, const std::string &msg)   // the whole-body methods raise RuntimeError, the _dof ones ValueError
  {
    if (per == 6) throw py::value_error(msg);
    throw std::runtime_error(msg);
  }
  const double *mixed_args(const char *who, int per, const marr &mask, const darr &body_in, const py::object &slip, darr &sl) const
  {
    if (mask.size() != per * (py::ssize_t)n_bod())
      bad_mixed_arg(per, std::string(who) + (per == 6 ? ": prescribed must have length 6*N_bod" : ": prescribed must have length N_bod"));
    if (body_in.size() != 6 * (py::ssize_t)n_bod()) bad_mixed_arg(per, std::string(who) + ": body_in must have length 6*N_bod");
    if (slip.is_none()) return nullptr;
    sl = slip.cast<darr>();
    if (sl.size() != n3()) bad_mixed_arg(per, std::string(who) + ": slip must have length 3*N_blobs");
    return sl.data();
  }
  py::tuple solve_mixed_any(const char *who, int per, const marr &mask, const darr &body_in, const py::object &slip, int max_iter, double rtol)
  {
    darr sl;
    const double *sp = mixed_args(who, per, mask, body_in, slip, sl);
    darr lam(n3()), U(6 * (py::ssize_t)n_bod()), F(6 * (py::ssize_t)n_bod());
    int it = 0, rc; double res = 0.0;
    {
      py::gil_scoped_release rel;
      rc = (per == 6 ? rbl_solve_mixed_dof : rbl_solve_mixed)(ctx, mask.data(), body_in.data(), sp, max_iter, rtol, lam.mutable_data(),
                                                              U.mutable_data(), F.mutable_data(), &it, &res);
    }
    check(rc);
    return py::make_tuple(lam, U, F, it, res);
  }
  // the solve, then evolve_X_Q(U) -> (F, iterations, residual estimate)
  py::tuple step_mixed_any(const char *who, int per, const marr &mask, const darr &body_in, const py::object &slip, int max_iter, double rtol)
  {
    darr sl;
    const double *sp = mixed_args(who, per, mask, body_in, slip, sl);
    darr F(6 * (py::ssize_t)n_bod());
    int it = 0, rc; double res = 0.0;
    {
      py::gil_scoped_release rel;
      rc = (per == 6 ? rbl_step_mixed_dof : rbl_step_mixed)(ctx, mask.data(), body_in.data(), sp, max_iter, rtol, F.mutable_data(), &it, &res);
    }
    check(rc);
    return py::make_tuple(F, it, res);
  }
  py::tuple solve_mixed(marr mask, darr body_in, py::object slip, int max_iter, double rtol)
  {
    return solve_mixed_any("solve_mixed", 1, mask, body_in, slip, max_iter, rtol);
  }
  py::tuple step_mixed(marr mask, darr body_in, py::object slip, int max_iter, double rtol)
  {
    return step_mixed_any("step_mixed", 1, mask, body_in, slip, max_iter, rtol);
  }
  py::tuple solve_mixed_dof(marr mask, darr body_in, py::object slip, int max_iter, double rtol)
  {
    return solve_mixed_any("solve_mixed_dof", 6, mask, body_in, slip, max_iter, rtol);
  }
  py::tuple step_mixed_dof(marr mask, darr body_in, py::object slip, int max_iter, double rtol)
  {
    return step_mixed_any("step_mixed_dof", 6, mask, body_in, slip, max_iter, rtol);
  }
  // k right-hand sides under one mask in lock step (rbl_solve_mixed_multi, rbl_solve_mixed_dof_multi): body_in (k, 6 N_bod), slip None
  // or (k, 3 N_blobs) -> (lambda (k, 3 N_blobs), U (k, 6 N_bod), F (k, 6 N_bod), iterations (k,), residual estimates (k,))
  py::tuple solve_mixed_multi_any(const char *who, int per, const marr &mask, const darr &body_in, const py::object &slip, int max_iter,
                                  double rtol)
  {
    const py::ssize_t nb6 = 6 * (py::ssize_t)n_bod();
    if (mask.size() != per * (py::ssize_t)n_bod())
      throw py::value_error(std::string(who) + (per == 6 ? ": prescribed must have length 6*N_bod" : ": prescribed must have length N_bod"));
    if (body_in.ndim() != 2 || body_in.shape(0) < 1 || body_in.shape(1) != nb6)
      throw py::value_error(std::string(who) + ": body_in must have shape (k, 6*N_bod), k >= 1");
    const py::ssize_t k = body_in.shape(0);
    darr sl;
    const double *sp = nullptr;
    if (!slip.is_none()) {
      sl = slip.cast<darr>();
      if (sl.ndim() != 2 || sl.shape(0) != k || sl.shape(1) != n3()) throw py::value_error(std::string(who) + ": slip must have shape (k, 3*N_blobs)");
      sp = sl.data();
    }
    darr lam({k, (py::ssize_t)n3()}), U({k, nb6}), F({k, nb6}), res(k);
    py::array_t<int> it(k);
    int rc;
    {
      py::gil_scoped_release rel;
      rc = (per == 6 ? rbl_solve_mixed_dof_multi : rbl_solve_mixed_multi)(ctx, mask.data(), (int)k, body_in.data(), sp, max_iter, rtol,
                                                                          lam.mutable_data(), U.mutable_data(), F.mutable_data(),
                                                                          it.mutable_data(), res.mutable_data());
    }
    check(rc);
    return py::make_tuple(lam, U, F, it, res);
  }
  py::tuple solve_mixed_multi(marr mask, darr body_in, py::object slip, int max_iter, double rtol)
  {
    return solve_mixed_multi_any("solve_mixed_multi", 1, mask, body_in, slip, max_iter, rtol);
  }
  py::tuple solve_mixed_dof_multi(marr mask, darr body_in, py::object slip, int max_iter, double rtol)
  {
    return solve_mixed_multi_any("solve_mixed_dof_multi", 6, mask, body_in, slip, max_iter, rtol);
  }
  // the Brownian midpoint step with prescribed bodies: right-hand side and predictor at q^n -> (s, X_half, Q_half), nothing committed
  const double *noise_arg(const char *who, const py::object &W, darr &Wa) const
  {
    if (W.is_none()) return nullptr;
    Wa = W.cast<darr>();
    if (Wa.size() != 3 * n3()) throw std::runtime_error(std::string(who) + ": W must have length 9*N_blobs (W1|W2|W_rfd)");
    return Wa.data();
  }
  py::tuple RHS_and_Midpoint_mixed_any(const char *who, int per, const marr &mask, const darr &body_in, const py::object &slip,
                                       const py::object &W, uint64_t seed, const std::string &method, bool split_rand, double delta)
  {
    darr sl, Wa;
    const double *sp = mixed_args(who, per, mask, body_in, slip, sl);
    const double *wp = noise_arg(who, W, Wa);
    const int m = mhalf_method(method);
    const py::ssize_t nb = n_bod();
    darr s(n3()), X(3 * nb), Q(4 * nb);
    int rc;
    {
      py::gil_scoped_release rel;
      rc = (per == 6 ? rbl_RHS_and_Midpoint_mixed_dof : rbl_RHS_and_Midpoint_mixed)(ctx, mask.data(), body_in.data(), sp, wp, seed, m,
                                                                                    split_rand ? 1 : 0, delta, s.mutable_data(),
                                                                                    X.mutable_data(), Q.mutable_data());
    }
    check(rc);
    return py::make_tuple(s, X, Q);
  }
  // the whole step -> (F, iterations, residual estimate)
  py::tuple step_brownian_mixed_any(const char *who, int per, const marr &mask, const darr &body_in, const py::object &slip,
                                    const py::object &W, uint64_t seed, const std::string &method, bool split_rand, double delta,
                                    int max_iter, double rtol)
  {
    darr sl, Wa;
    const double *sp = mixed_args(who, per, mask, body_in, slip, sl);
    const double *wp = noise_arg(who, W, Wa);
    const int m = mhalf_method(method);
    darr F(6 * (py::ssize_t)n_bod());
    int it = 0, rc; double res = 0.0;
    {
      py::gil_scoped_release rel;
      rc = (per == 6 ? rbl_step_brownian_mixed_dof : rbl_step_brownian_mixed)(ctx, mask.data(), body_in.data(), sp, wp, seed, m,
                                                                              split_rand ? 1 : 0, delta, max_iter, rtol, F.mutable_data(),
                                                                              &it, &res);
    }
    check(rc);
    return py::make_tuple(F, it, res);
  }
  py::tuple RHS_and_Midpoint_mixed(marr mask, darr body_in, py::object slip, py::object W, uint64_t seed, const std::string &method,
                                   bool split_rand, double delta)
  {
    return RHS_and_Midpoint_mixed_any("RHS_and_Midpoint_mixed", 1, mask, body_in, slip, W, seed, method, split_rand, delta);
  }
  py::tuple step_brownian_mixed(marr mask, darr body_in, py::object slip, py::object W, uint64_t seed, const std::string &method,
                                bool split_rand, double delta, int max_iter, double rtol)
  {
    return step_brownian_mixed_any("step_brownian_mixed", 1, mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol);
  }
  py::tuple RHS_and_Midpoint_mixed_dof(marr mask, darr body_in, py::object slip, py::object W, uint64_t seed, const std::string &method,
                                       bool split_rand, double delta)
  {
    return RHS_and_Midpoint_mixed_any("RHS_and_Midpoint_mixed_dof", 6, mask, body_in, slip, W, seed, method, split_rand, delta);
  }
  py::tuple step_brownian_mixed_dof(marr mask, darr body_in, py::object slip, py::object W, uint64_t seed, const std::string &method,
                                    bool split_rand, double delta, int max_iter, double rtol)
  {
    return step_brownian_mixed_any("step_brownian_mixed_dof", 6, mask, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol);
  }
  void set_interactions(double w, double eps_wall, double b_wall, double eps_blob, double b_blob, double r_cut, bool on)
  {
    check(rbl_set_interactions(ctx, w, eps_wall, b_wall, eps_blob, b_blob, r_cut, on ? 1 : 0));
  }
  void set_pair_table(darr U, darr dU, double r_min, double r_cut, bool on)
  {
    if (U.ndim() != 1 || dU.ndim() != 1 || U.size() != dU.size()) throw std::runtime_error("set_pair_table: U and dU must be one-dimensional and of one length");
    check(rbl_set_pair_table(ctx, U.data(), dU.data(), (int)U.size(), r_min, r_cut, on ? 1 : 0));
  }
  void set_height_table(darr U, darr dU, double h_min, double h_cut, bool on)
  {
    if (U.ndim() != 1 || dU.ndim() != 1 || U.size() != dU.size()) throw std::runtime_error("set_height_table: U and dU must be one-dimensional and of one length");
    check(rbl_set_height_table(ctx, U.data(), dU.data(), (int)U.size(), h_min, h_cut, on ? 1 : 0));
  }
  void set_traps(darr k, darr X0, bool on)
  {
    if (k.size() != X0.size() || k.size() % 3 || !k.size()) throw std::runtime_error("set_traps: k and X0 must both hold 3 entries per body");
    check(rbl_set_traps(ctx, k.data(), X0.data(), (int)(k.size() / 3), on ? 1 : 0));
  }
  // m: 3 entries per body; None with on = false only switches the dipoles off
  void set_dipoles(py::object m, double c_dd, double r_core, double r_cut, bool on)
  {
    if (m.is_none()) { check(rbl_set_dipoles(ctx, nullptr, 0, c_dd, r_core, r_cut, on ? 1 : 0)); return; }
    darr ma = m.cast<darr>();
    if (ma.size() % 3 || !ma.size()) throw std::runtime_error("set_dipoles: m_body must hold 3 entries per body");
    check(rbl_set_dipoles(ctx, ma.data(), (int)(ma.size() / 3), c_dd, r_core, r_cut, on ? 1 : 0));
  }
  py::dict dipoles() const
  {
    int n = 0, on = 0;
    double c_dd = 0.0, r_core = 0.0, r_cut = 0.0;
    rbl_get_dipoles(ctx, &n, &c_dd, &r_core, &r_cut, &on, nullptr);
    darr m(std::vector<py::ssize_t>{(py::ssize_t)n, 3});
    if (n) rbl_get_dipoles(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, m.mutable_data());
    py::dict d;
    d["on"] = on != 0; d["c_dd"] = c_dd; d["r_core"] = r_core; d["r_cut"] = r_cut; d["m_body"] = m;
    return d;
  }
  void set_magnetic_field(py::object B0, py::object B1, py::object B2, double omega, bool on)
  {
    if (B0.is_none() && B1.is_none() && B2.is_none()) { check(rbl_set_magnetic_field(ctx, nullptr, nullptr, nullptr, omega, on ? 1 : 0)); return; }
    darr b[3] = {B0.cast<darr>(), B1.cast<darr>(), B2.cast<darr>()};
    for (const darr &v : b)
      if (v.size() != 3) throw std::runtime_error("set_magnetic_field: B0, B1 and B2 must have 3 entries each");
    check(rbl_set_magnetic_field(ctx, b[0].data(), b[1].data(), b[2].data(), omega, on ? 1 : 0));
  }
  py::dict magnetic_field() const
  {
    darr B(std::vector<py::ssize_t>{3, 3});
    double omega = 0.0;
    int on = 0;
    rbl_get_magnetic_field(ctx, B.mutable_data(), &omega, &on);
    py::dict d;
    d["on"] = on != 0; d["omega"] = omega; d["B"] = B;
    return d;
  }
  void set_field_time(darr t) { check(rbl_set_field_time(ctx, t.data(), (int)t.size())); }
  darr field_time() const
  {
    int n = 0;
    rbl_get_field_time(ctx, &n, nullptr);
    darr t(n);
    rbl_get_field_time(ctx, nullptr, t.mutable_data());
    return t;
  }
  // body: 2 per bond, anchor: 6 per bond, kind: 1 per bond or None, param: (k, l0) per bond; body None only switches the bonds off
  void set_bonds(py::object body, py::object anchor, py::object kind, py::object param, bool on)
  {
    if (body.is_none()) { check(rbl_set_bonds(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, on ? 1 : 0)); return; }
    typedef py::array_t<int, py::array::c_style | py::array::forcecast> iarr;
    iarr b = body.cast<iarr>();
    darr an = anchor.cast<darr>(), pa = param.cast<darr>();
    const py::ssize_t n = b.size() / 2;
    if (b.size() % 2 || !n || an.size() != 6 * n || pa.size() != 2 * n)
      throw std::runtime_error("set_bonds: body must hold 2, anchor 6 and param 2 entries per bond");
    iarr ki;
    if (!kind.is_none()) {
      ki = kind.cast<iarr>();
      if (ki.size() != n) throw std::runtime_error("set_bonds: kind must hold one entry per bond");
    }
    check(rbl_set_bonds(ctx, (int)n, b.data(), an.data(), kind.is_none() ? nullptr : ki.data(), pa.data(), 1, on ? 1 : 0));
  }
  void set_bond_table(darr U, darr dU, double r_min, double r_cut, bool on)
  {
    if (U.ndim() != 1 || dU.ndim() != 1 || U.size() != dU.size()) throw std::runtime_error("set_bond_table: U and dU must be one-dimensional and of one length");
    check(rbl_set_bond_table(ctx, U.data(), dU.data(), (int)U.size(), r_min, r_cut, on ? 1 : 0));
  }
  // (length, tension, energy) of every bond
  py::tuple bond_state()
  {
    int n = 0;
    rbl_get_bonds(ctx, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    darr len(n), ten(n), en(n);
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_bond_state(ctx, len.mutable_data(), ten.mutable_data(), en.mutable_data());
    }
    check(rc);
    return py::make_tuple(len, ten, en);
  }
  // hard joints (include/rbl.h section 9).  body: 2 per joint, anchor: 6 per joint; body None only switches the joints off
  void set_joints(py::object body, py::object anchor, bool on)
  {
    if (body.is_none()) { check(rbl_set_joints(ctx, 0, nullptr, nullptr, on ? 1 : 0)); return; }
    typedef py::array_t<int, py::array::c_style | py::array::forcecast> iarr;
    iarr b = body.cast<iarr>();
    darr an = anchor.cast<darr>();
    const py::ssize_t n = b.size() / 2;
    if (b.size() % 2 || !n || an.size() != 6 * n) throw std::runtime_error("set_joints: body must hold 2 and anchor 6 entries per joint");
    check(rbl_set_joints(ctx, (int)n, b.data(), an.data(), on ? 1 : 0));
  }
  // -> (on, body (2 n,), anchor (6 n,))
  py::tuple joints() const
  {
    int n = 0, on = 0;
    rbl_get_joints(ctx, &n, &on, nullptr, nullptr);
    py::array_t<int> b(2 * (py::ssize_t)n);
    darr an(6 * (py::ssize_t)n);
    rbl_get_joints(ctx, nullptr, nullptr, b.mutable_data(), an.mutable_data());
    return py::make_tuple(on != 0, b, an);
  }
  py::ssize_t joints_active() const
  {
    int n = 0, on = 0;
    rbl_get_joints(ctx, &n, &on, nullptr, nullptr);
    return on ? n : 0;
  }
  const double *jointed_args(const char *who, const darr &F, const py::object &slip, const py::object &jv, const char *jname, darr &sl,
                             darr &jr, const double **jp) const
  {
    if (F.size() != 6 * (py::ssize_t)n_bod()) throw std::runtime_error(std::string(who) + ": F_body must have length 6*N_bod");
    *jp = nullptr;
    if (!jv.is_none()) {
      jr = jv.cast<darr>();
      if (jr.size() != 3 * joints_active()) throw std::runtime_error(std::string(who) + ": " + jname + " must have length 3*n_joints (of the joints that are on)");
      *jp = jr.size() ? jr.data() : nullptr;
    }
    if (slip.is_none()) return nullptr;
    sl = slip.cast<darr>();
    if (sl.size() != n3()) throw std::runtime_error(std::string(who) + ": slip must have length 3*N_blobs");
    return sl.data();
  }
  // -> (lambda, U, phi, iterations, residual estimate); phi is empty while the joints are off
  py::tuple solve_jointed(darr F, py::object slip, py::object joint_rhs, int max_iter, double rtol)
  {
    darr sl, jr;
    const double *jp = nullptr;
    const double *sp = jointed_args("solve_jointed", F, slip, joint_rhs, "joint_rhs", sl, jr, &jp);
    darr lam(n3()), U(6 * (py::ssize_t)n_bod()), phi(3 * joints_active());
    int it = 0, rc; double res = 0.0;
    {
      py::gil_scoped_release rel;
      rc = rbl_solve_jointed(ctx, F.data(), sp, jp, max_iter, rtol, lam.mutable_data(), U.mutable_data(), phi.mutable_data(), &it, &res);
    }
    check(rc);
    return py::make_tuple(lam, U, phi, it, res);
  }
  // the step -> (phi, iterations, residual estimate)
  py::tuple step_jointed(darr F, py::object slip, py::object joint_velocity, double gamma, int max_iter, double rtol)
  {
    darr sl, jr;
    const double *jp = nullptr;
    const double *sp = jointed_args("step_jointed", F, slip, joint_velocity, "joint_velocity", sl, jr, &jp);
    darr phi(3 * joints_active());
    int it = 0, rc; double res = 0.0;
    {
      py::gil_scoped_release rel;
      rc = rbl_step_jointed(ctx, F.data(), sp, jp, gamma, max_iter, rtol, phi.mutable_data(), &it, &res);
    }
    check(rc);
    return py::make_tuple(phi, it, res);
  }
  // (gaps (3 n,), phi of the last jointed solve or step (3 n,))
  py::tuple joint_state()
  {
    int n = 0;
    rbl_get_joints(ctx, &n, nullptr, nullptr, nullptr);
    darr gap(3 * (py::ssize_t)n), phi(3 * (py::ssize_t)n);
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_joint_state(ctx, gap.mutable_data(), phi.mutable_data());
    }
    check(rc);
    return py::make_tuple(gap, phi);
  }
  int interactions_active() const
  {
    int m = 0;
    rbl_interactions_active(ctx, &m);
    return m;
  }
  // the model's body forces in the REFERENCE convention, -K^T f_phys (6 N_bod): add them to F in rhs = [0; -F]
  darr interaction_forces()
  {
    darr out(6 * (py::ssize_t)n_bod());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_interaction_forces(ctx, nullptr, out.mutable_data(), nullptr);
    }
    check(rc);
    double *o = out.mutable_data();
    for (py::ssize_t i = 0; i < out.size(); ++i) o[i] = -o[i];
    return out;
  }
  double interaction_energy()
  {
    double E = 0.0;
    check(rbl_interaction_forces(ctx, nullptr, nullptr, &E));
    return E;
  }

  // ---- imposed flow and active slip, first moments (include/rbl.h section 8) ----
  void set_background_flow(darr u0, darr G, bool on)
  {
    if (u0.size() != 3 || G.size() != 9) throw std::runtime_error("set_background_flow: u0 must have 3 entries, G 9");
    check(rbl_set_background_flow(ctx, u0.data(), G.data(), on ? 1 : 0));
  }
  void set_body_slip(darr slip_body, py::object scale, bool on)
  {
    if (slip_body.size() != (py::ssize_t)3 * n_blb()) throw std::runtime_error("set_body_slip: slip_body must have 3 N_blb entries");
    darr sc;
    if (!scale.is_none()) sc = scale.cast<darr>();
    check(rbl_set_body_slip(ctx, slip_body.data(), scale.is_none() ? nullptr : sc.data(), scale.is_none() ? 0 : (int)sc.size(), on ? 1 : 0));
  }
  py::tuple flow_model() const
  {
    darr v(12);
    int f = 0, b = 0;
    check(rbl_get_flow_model(ctx, v.mutable_data(), &f, &b));
    return py::make_tuple(v, f != 0, b != 0);
  }
  darr flow_slip()
  {
    darr out(n3());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_flow_slip(ctx, out.mutable_data());
    }
    check(rc);
    return out;
  }
  darr first_moments(darr lam)
  {
    if (lam.size() != n3()) throw std::runtime_error("first_moments: lambda must have 3 N_blobs entries");
    darr out(9 * (py::ssize_t)n_bod());
    int rc;
    {
      py::gil_scoped_release rel;
      rc = rbl_first_moments(ctx, lam.data(), out.mutable_data());
    }
    check(rc);
    return out;
  }
  darr step_moments()
  {
    darr out(9 * (py::ssize_t)n_bod());
    check(rbl_step_moments(ctx, out.mutable_data()));
    return out;
  }

  void set_option(const std::string &name, int64_t value)
  {
    const int key = rbl_option_key(name.c_str());
    if (!key) throw std::runtime_error("set_option: unknown option '" + name + "'");
    check(rbl_set_option(ctx, key, value));
  }
  int64_t get_option(const std::string &name) const
  {
    const int key = rbl_option_key(name.c_str());
    int64_t v = 0;
    if (!key || rbl_get_option(ctx, key, &v)) throw std::runtime_error("get_option: unknown option '" + name + "'");
    return v;
  }
  uintptr_t handle() const { return (uintptr_t)ctx; }
};

}  // namespace

PYBIND11_MODULE(c_rigid, m)
{
  m.doc() = "Rigid code (MI355X-native librbl behind the reference's CManyBodies surface)";
  py::class_<CManyBodies>(m, "CManyBodies")
      .def(py::init<>())
      .def("getConfig", &CManyBodies::getConfig, "get the X and Q vectors for the current position")
      .def("setParameters", &CManyBodies::setParameters, "Set parameters for the module")
      .def("setBlkPC", &CManyBodies::setBlkPC, "set PC type")
      .def("setWallPC", &CManyBodies::setWallPC, "use wall corrections")
      .def("set_K_mats", &CManyBodies::set_K_mats, "Set the K,K^T,K^-1 matrices for the module")
      .def("K_x_U", &CManyBodies::K_x_U, "Multiply K by U", py::arg("U"))
      .def("KT_x_Lam", &CManyBodies::KT_x_Lam, "Multiply K^T by lambda", py::arg("lambda"))
      .def("multi_body_pos", &CManyBodies::multi_body_pos, "Get the blob positions")
      .def("apply_PC", &CManyBodies::apply_PC, "apply for PC")
      .def("setConfig", &CManyBodies::setConfig, "Set the X and Q vectors for the current position",
           py::arg("X"), py::arg("Q"))
      .def("get_K", &CManyBodies::get_K, "get K")
      .def("get_Kinv", &CManyBodies::get_Kinv, "get Kinv")
      .def("evolve_X_Q", &CManyBodies::evolve_X_Q, "evolve rigid bodies", py::arg("U"))
      .def("apply_M", &CManyBodies::apply_M, "mobility matrix mult", py::arg("F"), py::arg("r_vecs"))
      // extensions
      .def("apply_M_multi", &CManyBodies::apply_M_multi, py::arg("F"), py::arg("r_vecs"))
      .def("M_half_W", &CManyBodies::M_half_W, py::arg("W") = py::none(), py::arg("seed") = 0,
           py::arg("method") = "cholesky")
      .def("M_half_W_r", &CManyBodies::M_half_W_r, py::arg("r_vecs"), py::arg("W"), py::arg("method") = "cholesky")
      .def("M_RFD", &CManyBodies::M_RFD, py::arg("W") = py::none(), py::arg("seed") = 0, py::arg("delta") = 1.0e-4)
      .def("KTinv_RFD", &CManyBodies::KTinv_RFD, py::arg("W"), py::arg("delta") = 1.0e-4)
      .def("update_X_Q", &CManyBodies::update_X_Q, py::arg("U"))
      .def("step_deterministic", &CManyBodies::step_deterministic, py::arg("F"), py::arg("slip") = py::none(),
           py::arg("max_iter") = 50, py::arg("rtol") = 1.0e-8, py::arg("warm_start") = 0)
      .def("step_brownian", &CManyBodies::step_brownian, py::arg("F"), py::arg("slip") = py::none(),
           py::arg("W") = py::none(), py::arg("seed") = 0, py::arg("method") = "lanczos_pc", py::arg("split_rand") = true,
           py::arg("delta") = 1.0e-4, py::arg("max_iter") = 50, py::arg("rtol") = 1.0e-8)
      .def("RHS_and_Midpoint", &CManyBodies::RHS_and_Midpoint, py::arg("Slip"), py::arg("Force"),
           py::arg("W") = py::none(), py::arg("seed") = 0, py::arg("method") = "cholesky",
           py::arg("split_rand") = true, py::arg("delta") = 1.0e-4)
      .def("lanczos_report", &CManyBodies::lanczos_report)
      .def("set_lanczos", &CManyBodies::set_lanczos, py::arg("max_iter"), py::arg("tol"))
      .def("rotne_prager_tensor", &CManyBodies::rotne_prager_tensor, py::arg("r_vecs"), py::arg("scale_damp") = false)
      .def("cholesky_lower", &CManyBodies::cholesky_lower, py::arg("M"))
      .def("pair_blocks", &CManyBodies::pair_blocks)
      .def("apply_saddle", &CManyBodies::apply_saddle, py::arg("x"))
      .def("solve_saddle", &CManyBodies::solve_saddle, py::arg("rhs"), py::arg("max_iter") = 100, py::arg("rtol") = 1.0e-8,
           py::arg("x0") = py::none())
      .def("solve_saddle_multi", &CManyBodies::solve_saddle_multi, py::arg("rhs"), py::arg("max_iter") = 100, py::arg("rtol") = 1.0e-8)
      .def("M_RFD_cfgs", &CManyBodies::M_RFD_cfgs, py::arg("U"), py::arg("delta") = 1.0e-4)
      .def("M_RFD_from_U", &CManyBodies::M_RFD_from_U, py::arg("U"), py::arg("W"), py::arg("delta") = 1.0e-3)
      .def("KT_RFD_from_U", &CManyBodies::KT_RFD_from_U, py::arg("U"), py::arg("W"), py::arg("delta") = 1.0e-3)
      .def("evolve_X_Q_RFD", &CManyBodies::evolve_X_Q_RFD, py::arg("U"))
      .def("set_interactions", &CManyBodies::set_interactions, py::arg("w"), py::arg("eps_wall"), py::arg("b_wall"), py::arg("eps_blob"),
           py::arg("b_blob"), py::arg("r_cut"), py::arg("on") = true)
      .def("set_pair_table", &CManyBodies::set_pair_table, py::arg("U"), py::arg("dU"), py::arg("r_min"), py::arg("r_cut"), py::arg("on") = true)
      .def("set_height_table", &CManyBodies::set_height_table, py::arg("U"), py::arg("dU"), py::arg("h_min"), py::arg("h_cut"),
           py::arg("on") = true)
      .def("set_traps", &CManyBodies::set_traps, py::arg("k"), py::arg("X0"), py::arg("on") = true)
      .def("set_dipoles", &CManyBodies::set_dipoles, py::arg("m_body"), py::arg("c_dd"), py::arg("r_core"), py::arg("r_cut"),
           py::arg("on") = true)
      .def("dipoles", &CManyBodies::dipoles)
      .def("set_magnetic_field", &CManyBodies::set_magnetic_field, py::arg("B0"), py::arg("B1"), py::arg("B2"), py::arg("omega"),
           py::arg("on") = true)
      .def("magnetic_field", &CManyBodies::magnetic_field)
      .def("set_field_time", &CManyBodies::set_field_time, py::arg("t"))
      .def("field_time", &CManyBodies::field_time)
      .def("set_bonds", &CManyBodies::set_bonds, py::arg("body"), py::arg("anchor"), py::arg("kind"), py::arg("param"), py::arg("on") = true)
      .def("set_bond_table", &CManyBodies::set_bond_table, py::arg("U"), py::arg("dU"), py::arg("r_min"), py::arg("r_cut"), py::arg("on") = true)
      .def("bond_state", &CManyBodies::bond_state, "(length, tension dU/dd, energy) of every bond")
      .def("set_joints", &CManyBodies::set_joints, "hard joints: ball joints and pivots imposed by solve_jointed / step_jointed", py::arg("body"),
           py::arg("anchor"), py::arg("on") = true)
      .def("joints", &CManyBodies::joints, "(on, body, anchor) of the stored joints")
      .def("solve_jointed", &CManyBodies::solve_jointed, "the saddle solve with the joints as constraints -> (lambda, U, phi, iterations, residual)",
           py::arg("F_body"), py::arg("slip") = py::none(), py::arg("joint_rhs") = py::none(), py::arg("max_iter") = 100, py::arg("rtol") = 1.0e-8)
      .def("step_jointed", &CManyBodies::step_jointed, "one deterministic time step with the joints -> (phi, iterations, residual)",
           py::arg("F_body"), py::arg("slip") = py::none(), py::arg("joint_velocity") = py::none(), py::arg("gamma") = 1.0,
           py::arg("max_iter") = 50, py::arg("rtol") = 1.0e-8)
      .def("joint_state", &CManyBodies::joint_state, "(gaps at the current configuration, phi of the last jointed solve or step)")
      .def("interactions_active", &CManyBodies::interactions_active,
           "bit 0 built-in terms, 1 pair table, 2 height table, 3 traps, 4 dipole pairs, 5 field torque, 6 bonds")
      .def("interaction_forces", &CManyBodies::interaction_forces, "force model's body forces/torques, reference convention (-K^T f)")
      .def("interaction_energy", &CManyBodies::interaction_energy)
      .def("velocity_field", &CManyBodies::velocity_field, "fluid velocity at points from blob forces", py::arg("points"),
           py::arg("lambda"), py::arg("r_vecs") = py::none())
      .def("solve_mixed", &CManyBodies::solve_mixed, "prescribed kinematics: velocities given on some bodies, loads on the others",
           py::arg("prescribed"), py::arg("body_in"), py::arg("slip") = py::none(), py::arg("max_iter") = 100, py::arg("rtol") = 1.0e-8)
      .def("step_mixed", &CManyBodies::step_mixed, py::arg("prescribed"), py::arg("body_in"), py::arg("slip") = py::none(),
           py::arg("max_iter") = 50, py::arg("rtol") = 1.0e-8)
      .def("solve_mixed_dof", &CManyBodies::solve_mixed_dof, "prescribed kinematics per velocity component: prescribed has 6 N_bod entries",
           py::arg("prescribed"), py::arg("body_in"), py::arg("slip") = py::none(), py::arg("max_iter") = 100, py::arg("rtol") = 1.0e-8)
      .def("step_mixed_dof", &CManyBodies::step_mixed_dof, py::arg("prescribed"), py::arg("body_in"), py::arg("slip") = py::none(),
           py::arg("max_iter") = 50, py::arg("rtol") = 1.0e-8)
      .def("solve_mixed_multi", &CManyBodies::solve_mixed_multi, "prescribed kinematics, k right-hand sides under one mask in lock step",
           py::arg("prescribed"), py::arg("body_in"), py::arg("slip") = py::none(), py::arg("max_iter") = 100, py::arg("rtol") = 1.0e-8)
      .def("solve_mixed_dof_multi", &CManyBodies::solve_mixed_dof_multi, "the same with a mask per velocity component (6 N_bod entries)",
           py::arg("prescribed"), py::arg("body_in"), py::arg("slip") = py::none(), py::arg("max_iter") = 100, py::arg("rtol") = 1.0e-8)
      .def("RHS_and_Midpoint_mixed", &CManyBodies::RHS_and_Midpoint_mixed, py::arg("prescribed"), py::arg("body_in"),
           py::arg("slip") = py::none(), py::arg("W") = py::none(), py::arg("seed") = 0, py::arg("method") = "cholesky",
           py::arg("split_rand") = true, py::arg("delta") = 1.0e-4)
      .def("step_brownian_mixed", &CManyBodies::step_brownian_mixed, py::arg("prescribed"), py::arg("body_in"),
           py::arg("slip") = py::none(), py::arg("W") = py::none(), py::arg("seed") = 0, py::arg("method") = "lanczos_pc",
           py::arg("split_rand") = true, py::arg("delta") = 1.0e-4, py::arg("max_iter") = 50, py::arg("rtol") = 1.0e-8)
      .def("RHS_and_Midpoint_mixed_dof", &CManyBodies::RHS_and_Midpoint_mixed_dof, py::arg("prescribed"), py::arg("body_in"),
           py::arg("slip") = py::none(), py::arg("W") = py::none(), py::arg("seed") = 0, py::arg("method") = "cholesky",
           py::arg("split_rand") = true, py::arg("delta") = 1.0e-4)
      .def("step_brownian_mixed_dof", &CManyBodies::step_brownian_mixed_dof, py::arg("prescribed"), py::arg("body_in"),
           py::arg("slip") = py::none(), py::arg("W") = py::none(), py::arg("seed") = 0, py::arg("method") = "lanczos_pc",
           py::arg("split_rand") = true, py::arg("delta") = 1.0e-4, py::arg("max_iter") = 50, py::arg("rtol") = 1.0e-8)
      .def("set_background_flow", &CManyBodies::set_background_flow, "u_inf(r) = u0 + G r added to every step's slip as -u_inf",
           py::arg("u0"), py::arg("G"), py::arg("on") = true)
      .def("set_body_slip", &CManyBodies::set_body_slip, "slip pattern in the body frame, a factor per body", py::arg("slip_body"),
           py::arg("scale") = py::none(), py::arg("on") = true)
      .def("flow_model", &CManyBodies::flow_model, "([u0 | G], flow on, body slip on)")
      .def("flow_slip", &CManyBodies::flow_slip, "the flow model's term at the current configuration, 3 N_blobs")
      .def("first_moments", &CManyBodies::first_moments, "D_b = sum (r_i - X_b) lambda_i^T per body, 9 N_bod", py::arg("lambda"))
      .def("step_moments", &CManyBodies::step_moments, "first moments recorded by the last step (option record_moments)")
      .def("set_option", &CManyBodies::set_option, py::arg("name"), py::arg("value"))
      .def("get_option", &CManyBodies::get_option, py::arg("name"))
      .def("handle", &CManyBodies::handle, "address of the underlying rbl_ctx (for the ctypes device API)")
      .def_property_readonly_static("precision", [](py::object) { return std::string(rbl_precision()); },
                                    "Compilation precision, a string holding either single or double.");
}
