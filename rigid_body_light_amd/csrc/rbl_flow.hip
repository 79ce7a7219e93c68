// rbl_flow.hip -- imposed flow, body-frame slip and first moments of the blob forces (include/rbl.h section 8).
//
// The other half of the right-hand side next to the force model (rbl_forces.hip): a linear background flow u_inf(r) = u0 + G r
// and a slip pattern carried by the bodies are kept in the context and evaluated on the device at q^n inside every step family,
// in the sign convention of the `slip` argument (M lambda - K U = slip: a blob that moves with the fluid gets slip = -u_inf).
//
// Two kernels:
//   k_flow_slip       one lane per blob: t_i = scale_b R(q_b) s_body,i - (u0 + G r_i) from the resident positions and
//                     orientations, written or added to the caller's slip (slip + t, in that order).  No sums over blobs: the
//                     same configuration gives bitwise the same term on every call, every rank and for every replica.
//   k_first_moments   one workgroup per body: D_b = sum_i l_i lambda_i^T with the lever arms of the K kernels (its antisymmetric
//                     part is the torque of k_KT_x_Lam, its symmetric traceless part the stresslet), LDS tree in one fixed order,
//                     no atomics.  For an ensemble the lever arms are rebuilt from the replica's orientations as k_body_geom
//                     builds them (the one-kernel solver keeps its own in LDS).
#include <cmath>
#include <cstring>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"

namespace {

constexpr int FT = 256;

struct FlowParams {
  double u0[3], G[9];
  int flow, slip;
};

// Nb: bodies per replica (the scale of body b of every replica is scale[b % Nb]); add: NULL or the caller's slip, which may
// be out itself (the steps add in place: neither of the two is __restrict__)
__global__ __launch_bounds__(FT) void k_flow_slip(const double *__restrict__ pos, const double *__restrict__ Q,
                                                  const double *__restrict__ sbody, const double *__restrict__ scale, FlowParams P,
                                                  int N_blb, int Nb, long N, const double *add, double *out)
{
  const long idx = (long)blockIdx.x * FT + threadIdx.x;
  if (idx >= N) return;
  const long b = idx / N_blb;
  const int k = (int)(idx - b * N_blb);
  double a[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
  if (P.slip) {                                          // the pattern seen through the body's rotation
    double R[9];
    quat_rot(Q + 4 * b, R);
    const double s0 = sbody[3 * k], s1 = sbody[3 * k + 1], s2 = sbody[3 * k + 2];
    const double sc = scale ? scale[b % Nb] : 1.0;
    for (int p = 0; p < 3; ++p) a[p] = sc * (R[3 * p] * s0 + R[3 * p + 1] * s1 + R[3 * p + 2] * s2);
  }
  if (P.flow) {
    const double x = pos[3 * idx], y = pos[3 * idx + 1], z = pos[3 * idx + 2];
    for (int p = 0; p < 3; ++p) u[p] = P.u0[p] + (P.G[3 * p] * x + P.G[3 * p + 1] * y + P.G[3 * p + 2] * z);
  }
  for (int p = 0; p < 3; ++p) {
    const double t = a[p] - u[p];
    out[3 * idx + p] = add ? add[3 * idx + p] + t : t;
  }
}

// body g = blockIdx.x, replica g / Nb: its lambda starts at lam + (g / Nb) rep_stride + 3 (g % Nb) N_blb (one system: Nb = N_bod).
// lever: the resident lever arms of all bodies, or NULL: l_k = R(Q_g) c_k rebuilt here, term for term as k_body_geom
__global__ __launch_bounds__(FT) void k_first_moments(const double *__restrict__ lever, const double *__restrict__ Q,
                                                      const double *__restrict__ cfg, const double *__restrict__ lam, int N_blb,
                                                      int Nb, long rep_stride, double *__restrict__ D)
{
  __shared__ double s[9][FT];
  const int g = blockIdx.x, t = threadIdx.x;
  const double *lb = lam + (size_t)(g / Nb) * (size_t)rep_stride + 3 * (size_t)(g % Nb) * N_blb;
  double R[9];
  if (!lever) quat_rot(Q + 4 * (size_t)g, R);
  double d[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = t; k < N_blb; k += FT) {
    double l[3];
    if (lever) {
      const double *lv = lever + 3 * ((size_t)g * N_blb + k);
      l[0] = lv[0]; l[1] = lv[1]; l[2] = lv[2];
    } else {
      const double c0 = cfg[3 * k], c1 = cfg[3 * k + 1], c2 = cfg[3 * k + 2];
      {
#pragma clang fp contract(off)
        l[0] = c0 * R[0] + c1 * R[1] + c2 * R[2];
        l[1] = c0 * R[3] + c1 * R[4] + c2 * R[5];
        l[2] = c0 * R[6] + c1 * R[7] + c2 * R[8];
      }
    }
    const double *v = lb + 3 * (size_t)k;
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) d[3 * p + q] += l[p] * v[q];
  }
  rbl_block_sum<9, FT>(d, s, t);
  if (t < 9) D[9 * (size_t)g + t] = d[t];
}

bool fl_on(const rbl_ctx *c) { return c->fl_flow_on || c->fl_slip_on; }

// the pattern and the scales on the device (once per rbl_set_body_slip)
int fl_upload(rbl_ctx *c)
{
  if (!c->fl_slip_on || c->fl_dev_valid) return RBL_OK;
  const size_t ns = c->fl_slip_body.size(), nc = c->fl_scale.size();
  int rc = rbl_dev_reserve(c, c->d_flow, sizeof(double) * (ns + nc)); if (rc) return rc;
  if ((rc = copy_h2d(c, c->d_flow.p, c->fl_slip_body.data(), sizeof(double) * ns))) return rc;
  if (nc && (rc = copy_h2d(c, (double *)c->d_flow.p + ns, c->fl_scale.data(), sizeof(double) * nc))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  c->fl_dev_valid = true;
  return RBL_OK;
}

void fl_launch(rbl_ctx *c, const double *d_pos, const double *d_Q, int Nb, int64_t N, const double *d_add, double *d_out)
{
  FlowParams P;
  std::memcpy(P.u0, c->fl_u0, sizeof(P.u0));
  std::memcpy(P.G, c->fl_G, sizeof(P.G));
  P.flow = c->fl_flow_on ? 1 : 0;
  P.slip = c->fl_slip_on ? 1 : 0;
  const double *sb = c->fl_slip_on ? (const double *)c->d_flow.p : nullptr;
  const double *sc = c->fl_slip_on && !c->fl_scale.empty() ? sb + c->fl_slip_body.size() : nullptr;
  hipLaunchKernelGGL(k_flow_slip, dim3((unsigned)((N + FT - 1) / FT)), dim3(FT), 0, c->stream, d_pos, d_Q, sb, sc, P, c->S.N_blb, Nb,
                     (long)N, d_add, d_out);
}

}  // namespace

// what every use of the model checks first, without a device: the wall-corrected mobility assumes no slip at z = 0, so with the
// wall only u = (G02 z, G12 z, 0) is a flow; the pattern belongs to the current structure, the scales to n_bod bodies
int flow_check(rbl_ctx *c, int n_bod)
{
  if (!fl_on(c)) return RBL_OK;
  if (c->fl_flow_on && c->S.wall) {
    const double *u = c->fl_u0, *G = c->fl_G;
    if (u[0] != 0.0 || u[1] != 0.0 || u[2] != 0.0 || G[0] != 0.0 || G[1] != 0.0 || G[3] != 0.0 || G[4] != 0.0 || G[6] != 0.0 ||
        G[7] != 0.0 || G[8] != 0.0)
      return rbl_fail(c, RBL_ERR_ARG, "background flow: with the wall only u = (G02 z, G12 z, 0) vanishes at z = 0 (u0, the lateral gradients and G22 must be 0)");
  }
  if (c->fl_slip_on) {
    if (c->fl_slip_gen != c->params_gen || c->fl_slip_body.size() != 3 * (size_t)c->S.N_blb)
      return rbl_fail(c, RBL_ERR_STATE, "body slip: rbl_set_parameters was called since rbl_set_body_slip (the pattern belongs to the structure: set it again)");
    if (!c->fl_scale.empty() && c->fl_scale.size() != (size_t)n_bod)
      return rbl_fail(c, RBL_ERR_ARG, "body slip: n_scale = " + std::to_string(c->fl_scale.size()) + " but the configuration has " +
                                          std::to_string(n_bod) + " bodies");
  }
  return RBL_OK;
}

// the steps' use of it on the context's own configuration: d_slip (3 N) = slip + t when the caller passed a slip (*have_slip),
// t otherwise, and *have_slip becomes true.  No-op (no launch, no allocation) while both parts are off.
int flow_add_to_step_slip(rbl_ctx *c, double *d_slip, bool *have_slip)
{
  if (!fl_on(c)) return RBL_OK;
  int rc = sync_bodies(c); if (rc) return rc;            // resident positions of q^n ...
  if ((rc = ensure_xq_dev(c))) return rc;                // ... and its orientations (a random finite difference may have left displaced ones)
  if ((rc = fl_upload(c))) return rc;
  const RblBodyState &S = c->S;
  fl_launch(c, (const double *)c->d_pos.p, (const double *)c->d_XQ.p + 3 * (size_t)S.N_bod, S.N_bod, (int64_t)S.N_bod * S.N_blb,
            *have_slip ? d_slip : nullptr, d_slip);
  *have_slip = true;
  return RBL_OK;
}

// the same for `reps` replicas of N_bod bodies (rbl_ensemble.hip): positions and orientations of all of them, one launch
bool flow_on(const rbl_ctx *c) { return fl_on(c); }

int flow_add_batch(rbl_ctx *c, const double *d_pos, const double *d_Q, int N_bod, int reps, double *d_slip, bool *have_slip,
                   const double *d_caller)
{
  if (!fl_on(c)) return RBL_OK;
  int rc = fl_upload(c); if (rc) return rc;
  fl_launch(c, d_pos, d_Q, N_bod, (int64_t)reps * N_bod * c->S.N_blb, *have_slip ? (d_caller ? d_caller : d_slip) : nullptr, d_slip);
  *have_slip = true;
  return RBL_OK;
}

void flow_launch_moments(rbl_ctx *c, const double *d_lever, const double *d_Q, const double *d_cfg, const double *d_lam, int Nb,
                         int n_bodies, int64_t rep_stride, double *d_D)
{
  hipLaunchKernelGGL(k_first_moments, dim3((unsigned)n_bodies), dim3(FT), 0, c->stream, d_lever, d_Q, d_cfg, d_lam, c->S.N_blb, Nb,
                     (long)rep_stride, d_D);
}

// RBL_OPT_RECORD_MOMENTS: the first moments of a step's lambda with the lever arms of the configuration the context is at
void flow_begin_step(rbl_ctx *c)
{
  if (c->record_mom) c->mom_nb = 0;                      // only a step that recorded leaves a readable set
}

int flow_record_moments(rbl_ctx *c, const double *d_lambda)
{
  if (!c->record_mom) return RBL_OK;
  int rc = sync_bodies(c); if (rc) return rc;
  const int nb = c->S.N_bod;
  if ((rc = rbl_dev_reserve(c, c->d_mom, sizeof(double) * 9 * (size_t)nb))) return rc;
  flow_launch_moments(c, (const double *)c->d_lever.p, nullptr, nullptr, d_lambda, nb, nb, 0, (double *)c->d_mom.p);
  c->mom_nb = nb;
  return RBL_OK;
}

// ---- C ABI (include/rbl.h section 8) --------------------------------------------------------------------------------

int rbl_set_background_flow(rbl_ctx *c, const double *u0, const double *G, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!u0 || !G) return rbl_fail(c, RBL_ERR_ARG, "set_background_flow: u0 or G is NULL");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(u0[i])) return rbl_fail(c, RBL_ERR_ARG, "set_background_flow: u0 and G must be finite");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(G[i])) return rbl_fail(c, RBL_ERR_ARG, "set_background_flow: u0 and G must be finite");
  std::memcpy(c->fl_u0, u0, sizeof(c->fl_u0));
  std::memcpy(c->fl_G, G, sizeof(c->fl_G));
  c->fl_flow_on = on != 0;
  return RBL_OK;
}

int rbl_set_body_slip(rbl_ctx *c, const double *slip_body, const double *slip_scale, int n_scale, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!c->S.params_set) return rbl_fail(c, RBL_ERR_STATE, "set_body_slip: setParameters has not been called (the pattern has one entry per blob of the structure)");
  if (!slip_body) return rbl_fail(c, RBL_ERR_ARG, "set_body_slip: slip_body is NULL");
  if (slip_scale && n_scale < 1) return rbl_fail(c, RBL_ERR_ARG, "set_body_slip: n_scale must be >= 1 with a scale vector");
  const size_t ns = 3 * (size_t)c->S.N_blb;
  for (size_t i = 0; i < ns; ++i)
    if (!std::isfinite(slip_body[i])) return rbl_fail(c, RBL_ERR_ARG, "set_body_slip: the pattern must be finite");
  for (int i = 0; slip_scale && i < n_scale; ++i)
    if (!std::isfinite(slip_scale[i])) return rbl_fail(c, RBL_ERR_ARG, "set_body_slip: the scales must be finite");
  c->fl_slip_body.assign(slip_body, slip_body + ns);
  if (slip_scale) c->fl_scale.assign(slip_scale, slip_scale + n_scale);
  else c->fl_scale.clear();
  c->fl_slip_on = on != 0;
  c->fl_slip_gen = c->params_gen;
  c->fl_dev_valid = false;
  return RBL_OK;
}

int rbl_get_flow_model(const rbl_ctx *c, double *u0G12, int *flow_on, int *body_slip_on)
{
  if (!c) return RBL_ERR_ARG;
  if (u0G12) {
    std::memcpy(u0G12, c->fl_u0, sizeof(c->fl_u0));
    std::memcpy(u0G12 + 3, c->fl_G, sizeof(c->fl_G));
  }
  if (flow_on) *flow_on = c->fl_flow_on ? 1 : 0;
  if (body_slip_on) *body_slip_on = c->fl_slip_on ? 1 : 0;
  return RBL_OK;
}

int rbl_flow_slip_dev(rbl_ctx *c, double *d_out)
{
  int rc = need_config(c); if (rc) return rc;
  if (!d_out) return rbl_fail(c, RBL_ERR_ARG, "flow_slip: out is NULL");
  if ((rc = flow_check(c, c->S.N_bod))) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  bool have = false;
  if ((rc = flow_add_to_step_slip(c, d_out, &have))) return rc;
  if (!have) RBL_HIP(c, hipMemsetAsync(d_out, 0, sizeof(double) * 3 * (size_t)c->S.N_bod * c->S.N_blb, c->stream));
  return RBL_OK;
}

int rbl_flow_slip(rbl_ctx *c, double *out)
{
  int rc = need_config(c); if (rc) return rc;
  if (!out) return rbl_fail(c, RBL_ERR_ARG, "flow_slip: out is NULL");
  if ((rc = flow_check(c, c->S.N_bod))) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const size_t vb = sizeof(double) * 3 * (size_t)c->S.N_bod * c->S.N_blb;
  if ((rc = rbl_dev_reserve(c, c->d_flow_w, vb))) return rc;
  if ((rc = rbl_flow_slip_dev(c, (double *)c->d_flow_w.p))) return rc;
  if ((rc = copy_d2h(c, out, c->d_flow_w.p, vb))) return rc;
  return finish_and_check(c);
}

int rbl_first_moments_dev(rbl_ctx *c, const double *d_lambda, double *d_D)
{
  int rc = need_config(c); if (rc) return rc;
  if (!d_lambda || !d_D) return rbl_fail(c, RBL_ERR_ARG, "first_moments: null argument");
  if ((rc = sync_bodies(c))) return rc;
  const int nb = c->S.N_bod;
  flow_launch_moments(c, (const double *)c->d_lever.p, nullptr, nullptr, d_lambda, nb, nb, 0, d_D);
  return RBL_OK;
}

int rbl_first_moments(rbl_ctx *c, const double *lambda, double *D)
{
  int rc = need_config(c); if (rc) return rc;
  if (!lambda || !D) return rbl_fail(c, RBL_ERR_ARG, "first_moments: null argument");
  if ((rc = rbl_dev_init(c))) return rc;
  const size_t n3 = 3 * (size_t)c->S.N_bod * c->S.N_blb, nd = 9 * (size_t)c->S.N_bod;
  if ((rc = rbl_dev_reserve(c, c->d_flow_w, sizeof(double) * (n3 + nd)))) return rc;
  double *dl = (double *)c->d_flow_w.p, *dD = dl + n3;
  if ((rc = copy_h2d(c, dl, lambda, sizeof(double) * n3))) return rc;
  if ((rc = rbl_first_moments_dev(c, dl, dD))) return rc;
  if ((rc = copy_d2h(c, D, dD, sizeof(double) * nd))) return rc;
  return finish_and_check(c);
}

int rbl_step_moments(rbl_ctx *c, double *D)
{
  if (!c) return RBL_ERR_ARG;
  if (!D) return rbl_fail(c, RBL_ERR_ARG, "step_moments: D is NULL");
  if (!c->mom_nb || c->mom_nb != c->S.N_bod)
    return rbl_fail(c, RBL_ERR_STATE, "step_moments: no step has recorded first moments for this configuration (rbl_set_option record_moments, then a step)");
  int rc = copy_d2h(c, D, c->d_mom.p, sizeof(double) * 9 * (size_t)c->mom_nb); if (rc) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

int rbl_ensemble_step_moments(rbl_ctx *c, double *D)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_step_moments");
  if (!D) return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_moments: D is NULL");
  if (!c->ens_mom_R || c->ens_mom_R != c->ens_R || c->ens_mom_nb != c->ens_Nb)
    return rbl_fail(c, RBL_ERR_STATE, "ensemble_step_moments: no ensemble step has recorded first moments for this ensemble (rbl_set_option record_moments, then a step)");
  int rc = copy_d2h(c, D, c->d_ens_mom.p, sizeof(double) * 9 * (size_t)c->ens_mom_R * c->ens_mom_nb); if (rc) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}
