// rbl_forces.hip -- configuration-dependent forces on the blobs (include/rbl.h section 4): buoyant weight, a screened wall
// repulsion and a steric repulsion between blobs of different bodies, evaluated on the GPU at the context's configuration and
// reduced to body forces / torques with K^T.  The reference has no force model; what it would have needed is a host loop.
//
// Two kernels:
//   k_body_neighbours    one wave per body i: the bodies j != i of i's window (an ensemble's replica; one system: all bodies)
//                        with |X_i - X_j| <= 2 R_body + r_cut, written in increasing j
//                        by a ballot and a prefix count (no atomics: the lists are the same on every call and every rank).
//                        Exact cull: a blob lies within R_body of its body's centre, so two blobs of bodies further apart
//                        than 2 R_body + r_cut are further apart than r_cut.
//   k_blob_interactions  one workgroup per (body i, tile of i's blobs): the neighbours' blob positions are staged through LDS
//                        in list order, every lane accumulates the force on ITS blob in registers over the ordered pairs
//                        (i <- j; the pair j <- i is evaluated by j's workgroup), weight and wall are added in the epilogue.
//                        No fp64 atomics, one summation order: bitwise reproducible.  The software exp and the division are
//                        taken only inside r_cut.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rbl_api_internal.hpp"

namespace {

constexpr int IA_CAP_MAX = 1024;      // neighbour-list length per body (beyond it: RBL_ERR_CAPACITY)
constexpr int IA_CHUNK = 512;         // neighbour blobs staged per pass (x, y, z, pad: 16 KB of LDS)
constexpr int IA_BT = 256;            // lanes per workgroup of the pair kernel for bodies of more than 128 blobs

struct IaParams {
  double w, a, eps_w, inv_bw, eps_b, inv_bb, two_a, rc2;
  int wall;
};

// win: bodies per window -- body i only sees the bodies [i - i % win, i - i % win + win) (the replicas of an ensemble do not
// interact); win = N_bod: every body
__global__ __launch_bounds__(64) void k_body_neighbours(const double *__restrict__ X, int N_bod, int win, double cut2, int cull,
                                                        int cap, int *__restrict__ cnt, int *__restrict__ list, unsigned *__restrict__ err)
{
  const int i = blockIdx.x, t = threadIdx.x;
  const double xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
  const int jb = i - i % win, je = min(jb + win, N_bod);
  int base = 0;
  for (int j0 = jb; j0 < je; j0 += 64) {
    const int j = j0 + t;
    bool take = false;
    if (j < je && j != i) {
      if (!cull) take = true;
      else {
        const double dx = X[3 * (size_t)j] - xi, dy = X[3 * (size_t)j + 1] - yi, dz = X[3 * (size_t)j + 2] - zi;
        take = dx * dx + dy * dy + dz * dz <= cut2;
      }
    }
    const unsigned long long m = __ballot(take);
    const int below = __popcll(m & ((1ull << t) - 1ull));
    if (take && base + below < cap) list[(size_t)i * cap + base + below] = j;
    base += __popcll(m);
  }
  if (t == 0) {
    cnt[i] = base;                                       // may exceed cap: the pair kernel walks min(cnt, cap) and the overflow is reported
    if (base > cap) atomicOr(err, (unsigned)RBL_FLAG_CAPACITY);
  }
}

__global__ __launch_bounds__(IA_BT) void k_blob_interactions(const double *__restrict__ pos, const int *__restrict__ cnt,
                                                             const int *__restrict__ list, int cap, int N_blb, int tiles,
                                                             IaParams p, double *__restrict__ f, double *__restrict__ e,
                                                             int *__restrict__ npairs)
{
  __shared__ double s[IA_CHUNK][4];
  const int i = blockIdx.x / tiles, k = (blockIdx.x - i * tiles) * blockDim.x + threadIdx.x;
  const bool own = k < N_blb;
  const size_t gi = (size_t)i * N_blb + (own ? k : 0);
  const double xi = pos[3 * gi], yi = pos[3 * gi + 1], zi = pos[3 * gi + 2];
  double fx = 0.0, fy = 0.0, fz = 0.0, en = 0.0;
  int np = 0;
  const int nn = min(cnt[i], cap);
  for (int q = 0; q < nn; ++q) {
    const double *pj = pos + 3 * (size_t)list[(size_t)i * cap + q] * N_blb;
    for (int c0 = 0; c0 < N_blb; c0 += IA_CHUNK) {
      const int m = min(IA_CHUNK, N_blb - c0);
      __syncthreads();                                   // the previous chunk has been read by every lane
      for (int u = threadIdx.x; u < m; u += blockDim.x) {
        s[u][0] = pj[3 * (size_t)(c0 + u)];
        s[u][1] = pj[3 * (size_t)(c0 + u) + 1];
        s[u][2] = pj[3 * (size_t)(c0 + u) + 2];
      }
      __syncthreads();
      if (!own) continue;
      for (int u = 0; u < m; ++u) {
        const double dx = xi - s[u][0], dy = yi - s[u][1], dz = zi - s[u][2];
        const double r2 = dx * dx + dy * dy + dz * dz;
        if (r2 > p.rc2) continue;                        // beyond the cutoff: skipped, not multiplied by zero
        const double r = sqrt(r2);
        double U, g;                                     // energy of the pair, -U'(r) / r
        if (r >= p.two_a) {
          U = p.eps_b * (p.two_a / r) * exp(-(r - p.two_a) * p.inv_bb);
          g = U * (1.0 / r + p.inv_bb) / r;
        } else {                                         // the tangent at r = 2a continued inwards
          const double slope = p.eps_b * (1.0 / p.two_a + p.inv_bb);
          U = p.eps_b + slope * (p.two_a - r);
          g = r > 0.0 ? slope / r : 0.0;
        }
        fx += g * dx; fy += g * dy; fz += g * dz;
        en += 0.5 * U;
        ++np;
      }
    }
  }
  if (!own) return;
  fz -= p.w;                                             // weight
  en += p.w * zi;
  if (p.wall) {                                          // wall repulsion, tangent continued below h = a
    double Fw, Uw;
    if (zi >= p.a) { Uw = p.eps_w * exp(-(zi - p.a) * p.inv_bw); Fw = Uw * p.inv_bw; }
    else { Fw = p.eps_w * p.inv_bw; Uw = p.eps_w + Fw * (p.a - zi); }
    fz += Fw;
    en += Uw;
  }
  f[3 * gi] = fx; f[3 * gi + 1] = fy; f[3 * gi + 2] = fz;
  if (e) e[gi] = en;
  npairs[gi] = np;
}

struct IaLayout {
  double *f, *e, *ft;
  int *cnt, *list, *np;
};

int ia_cap(int N_bod) { return std::max(1, std::min(N_bod - 1, IA_CAP_MAX)); }

// d_ia = f_blob [3 N] | energy per blob [N] | K^T f [6 N_bod] | neighbour counts [N_bod] | lists [N_bod x cap] | pairs per blob [N]
size_t ia_bytes(int nb, int nblb, int cap)
{
  const size_t N = (size_t)nb * nblb;
  return sizeof(double) * (4 * N + 6 * (size_t)nb) + sizeof(int) * ((size_t)nb * (1 + (size_t)cap) + N);
}

IaLayout ia_layout(void *p, int nb, int nblb, int cap)
{
  const size_t N = (size_t)nb * nblb;
  IaLayout L;
  L.f = (double *)p;
  L.e = L.f + 3 * N;
  L.ft = L.e + N;
  L.cnt = (int *)(L.ft + 6 * (size_t)nb);
  L.list = L.cnt + nb;
  L.np = L.list + (size_t)nb * cap;
  return L;
}

int ia_reserve(rbl_ctx *c, IaLayout &L)
{
  const RblBodyState &S = c->S;
  const int cap = ia_cap(S.N_bod);
  int rc = rbl_dev_reserve(c, c->d_ia, ia_bytes(S.N_bod, S.N_blb, cap)); if (rc) return rc;
  L = ia_layout(c->d_ia.p, S.N_bod, S.N_blb, cap);
  return RBL_OK;
}

}  // namespace

// the model over n_win windows of win bodies each (resident X of the body centres, blob positions and lever arms): neighbour
// lists inside each window, the pair kernel, K^T f.  d_f (3 N) is required here; d_FT (6 N_bod total) and d_e may be NULL.
static int ia_launch(rbl_ctx *c, const double *d_X, const double *d_pos, const double *d_lever, int win, int n_win, double *d_cl,
                     double *d_f, double *d_FT, double *d_e, unsigned *d_err)
{
  const RblBodyState &S = c->S;
  if (!(c->ia_r_cut >= 2.0 * S.a))
    return rbl_fail(c, RBL_ERR_STATE, "interactions: r_cut is below 2a of the current parameters (call rbl_set_interactions again)");
  RblPhase ph(c, RBL_T_FORCES);
  const int nbod = win * n_win, cap = ia_cap(win);
  IaLayout L = ia_layout(d_cl, nbod, S.N_blb, cap);
  double R2 = 0.0;                                       // R_body: largest blob distance from the centre, body frame (mean removed)
  for (int k = 0; k < S.N_blb; ++k) {
    const double *q = &S.ref_cfg[3 * (size_t)k];
    R2 = std::max(R2, q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  }
  // a hair of slack for the rounding of the rotated lever arms and of the distances: it can only add candidates, whose
  // pairs beyond r_cut are then skipped one by one
  const double cut = (2.0 * std::sqrt(R2) + c->ia_r_cut) * (1.0 + 1e-12) + 1e-12;
  hipLaunchKernelGGL(k_body_neighbours, dim3(nbod), dim3(64), 0, c->stream, d_X, nbod, win, cut * cut, c->ia_cull ? 1 : 0, cap,
                     L.cnt, L.list, d_err);
  IaParams P;
  P.w = c->ia_w; P.a = S.a; P.eps_w = c->ia_eps_wall; P.inv_bw = 1.0 / c->ia_b_wall; P.eps_b = c->ia_eps_blob;
  P.inv_bb = 1.0 / c->ia_b_blob; P.two_a = 2.0 * S.a; P.rc2 = c->ia_r_cut * c->ia_r_cut; P.wall = S.wall ? 1 : 0;
  const int bt = S.N_blb > 128 ? IA_BT : (S.N_blb + 63) / 64 * 64, tiles = (S.N_blb + bt - 1) / bt;
  hipLaunchKernelGGL(k_blob_interactions, dim3((unsigned)(tiles * nbod)), dim3(bt), 0, c->stream, d_pos, (const int *)L.cnt,
                     (const int *)L.list, cap, S.N_blb, tiles, P, d_f, d_e, L.np);
  if (d_FT) rbl_launch_KT_x_Lam(c->stream, d_lever, d_f, S.N_blb, nbod, d_FT);
  return RBL_OK;
}

int ia_eval(rbl_ctx *c, double *d_f, double *d_FT, double *d_e)
{
  int rc = sync_bodies(c); if (rc) return rc;            // resident positions and lever arms of the current configuration
  const RblBodyState &S = c->S;
  IaLayout L;
  if ((rc = ia_reserve(c, L))) return rc;
  if ((rc = ia_launch(c, (const double *)c->d_XQ.p, (const double *)c->d_pos.p, (const double *)c->d_lever.p, S.N_bod, 1,
                      (double *)c->d_ia.p, d_f ? d_f : L.f, d_FT, d_e, c->d_err))) return rc;
  c->ia_nb = S.N_bod; c->ia_nblb = S.N_blb; c->ia_cap = ia_cap(S.N_bod);
  return RBL_OK;
}

size_t ia_batch_bytes(int N_bod, int N_blb, int reps)
{
  return ia_bytes(N_bod * reps, N_blb, ia_cap(N_bod));
}

int ia_eval_batch(rbl_ctx *c, const double *d_X, const double *d_pos, const double *d_lever, int N_bod, int reps, void *d_work,
                  double **d_f, double *d_FT, double *d_e, unsigned *d_err)
{
  IaLayout L = ia_layout(d_work, N_bod * reps, c->S.N_blb, ia_cap(N_bod));
  *d_f = L.f;
  return ia_launch(c, d_X, d_pos, d_lever, N_bod, reps, (double *)d_work, L.f, d_FT, d_e, d_err);
}

int ia_add_to_step_force(rbl_ctx *c, double *d_force)
{
  if (!c->ia_on) return RBL_OK;
  IaLayout L;
  int rc = ia_reserve(c, L); if (rc) return rc;
  if ((rc = ia_eval(c, nullptr, L.ft, nullptr))) return rc;
  rbl_launch_axpby(c->stream, 6 * (int64_t)c->S.N_bod, 1.0, d_force, -1.0, L.ft, d_force);   // reference convention: F_body - K^T f_phys
  return finish_and_check(c);
}

// ---- C ABI (include/rbl.h section 4) --------------------------------------------------------------------------------

int rbl_set_interactions(rbl_ctx *c, double w, double eps_wall, double b_wall, double eps_blob, double b_blob, double r_cut, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!c->S.params_set) return rbl_fail(c, RBL_ERR_STATE, "set_interactions: setParameters has not been called (r_cut is checked against 2a)");
  const double v[6] = {w, eps_wall, b_wall, eps_blob, b_blob, r_cut};
  for (double x : v)
    if (!std::isfinite(x)) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: every parameter must be finite");
  if (!(b_wall > 0.0) || !(b_blob > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: b_wall and b_blob must be positive");
  if (eps_wall < 0.0 || eps_blob < 0.0) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: eps_wall and eps_blob must be >= 0 (repulsions)");
  if (!(r_cut >= 2.0 * c->S.a)) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: r_cut must be >= 2a");
  c->ia_w = w; c->ia_eps_wall = eps_wall; c->ia_b_wall = b_wall; c->ia_eps_blob = eps_blob; c->ia_b_blob = b_blob; c->ia_r_cut = r_cut;
  c->ia_on = on != 0;
  return RBL_OK;
}

int rbl_get_interactions(const rbl_ctx *c, double *params6, int *on)
{
  if (!c) return RBL_ERR_ARG;
  if (params6) {
    const double v[6] = {c->ia_w, c->ia_eps_wall, c->ia_b_wall, c->ia_eps_blob, c->ia_b_blob, c->ia_r_cut};
    std::memcpy(params6, v, sizeof(v));
  }
  if (on) *on = c->ia_on ? 1 : 0;
  return RBL_OK;
}

int rbl_interaction_forces_dev(rbl_ctx *c, double *d_f_blob, double *d_FT_body, double *energy)
{
  int rc = need_config(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!c->ia_on) return rbl_fail(c, RBL_ERR_STATE, "interaction_forces: no force model is switched on (rbl_set_interactions)");
  if (!energy) return ia_eval(c, d_f_blob, d_FT_body, nullptr);
  IaLayout L;
  if ((rc = ia_reserve(c, L))) return rc;
  if ((rc = ia_eval(c, d_f_blob, d_FT_body, L.e))) return rc;
  const size_t N = (size_t)c->S.N_bod * c->S.N_blb;
  std::vector<double> e(N);
  if ((rc = copy_d2h(c, e.data(), L.e, sizeof(double) * N))) return rc;
  if ((rc = finish_and_check(c))) return rc;
  double E = 0.0;                                        // one order: blob index
  for (double x : e) E += x;
  *energy = E;
  return RBL_OK;
}

int rbl_interaction_forces(rbl_ctx *c, double *f_blob, double *FT_body, double *energy)
{
  int rc = need_config(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!c->ia_on) return rbl_fail(c, RBL_ERR_STATE, "interaction_forces: no force model is switched on (rbl_set_interactions)");
  const size_t N = (size_t)c->S.N_bod * c->S.N_blb, nb6 = (size_t)6 * c->S.N_bod;
  IaLayout L;
  if ((rc = ia_reserve(c, L))) return rc;
  if ((rc = rbl_interaction_forces_dev(c, nullptr, L.ft, energy))) return rc;
  if (f_blob && (rc = copy_d2h(c, f_blob, L.f, sizeof(double) * 3 * N))) return rc;
  if (FT_body && (rc = copy_d2h(c, FT_body, L.ft, sizeof(double) * nb6))) return rc;
  return finish_and_check(c);
}

int rbl_interaction_stats(rbl_ctx *c, int64_t *body_pairs, int64_t *blob_pairs)
{
  if (!c) return RBL_ERR_ARG;
  if (!c->ia_nb) return rbl_fail(c, RBL_ERR_STATE, "interaction_stats: nothing has been evaluated yet");
  const size_t N = (size_t)c->ia_nb * c->ia_nblb;
  std::vector<int> cnt((size_t)c->ia_nb), np(N);
  const IaLayout L = ia_layout(c->d_ia.p, c->ia_nb, c->ia_nblb, c->ia_cap);
  int rc = copy_d2h(c, cnt.data(), L.cnt, sizeof(int) * cnt.size()); if (rc) return rc;
  if ((rc = copy_d2h(c, np.data(), L.np, sizeof(int) * N))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  int64_t bp = 0, pp = 0;
  for (int x : cnt) bp += std::min(x, c->ia_cap);
  for (int x : np) pp += x;
  if (body_pairs) *body_pairs = bp;
  if (blob_pairs) *blob_pairs = pp;
  return RBL_OK;
}
