// rbl_ens_field.hip -- the flow at probe points for every replica of an ensemble, and the observers' share of a run's commit
// (include/rbl.h section 5, observers).
//
//   u_r(x_p) = nf d(z_p) sum_j sum_images M(x_p, r_j + image) d(z_j) lambda_{r,j}
//
// section 6's definition (rbl_field.hip) with replica r's own blobs as sources: the same pair block (rbl_pair_accum), the same
// damping, a coincident point (|x_p - r_j| < 1e-12 a) takes the self block, with the wall a point at z_p <= 0 gets u = 0.
//
//   k_ens_probe<WALL, PER, NI>   grid (point tiles, R), 64 .. 256 threads.  Prologue: the replica's N <= 256 blobs are placed from
//                                (X, Q, reference configuration) term for term as k_body_geom places them (contraction off) and
//                                staged ONCE per workgroup in LDS, radius-scaled positions and damped forces, 48 B each (<= 12 KB),
//                                read as broadcasts.  One point per lane and register set, NI sets per lane.  Every point sums
//                                over the blobs in index order; PER: the nearest-image reduction once per (point, blob), then
//                                the images p, then q, innermost (sweep_tile_per's order, rbl_kernels.hip); an open axis has a
//                                zero reciprocal and no images (RblSmallCell), so its reduction leaves the displacement alone.
//                                CELLS: replica r's own cell, read from the table of rbl_ensemble_set_cells.
//                                Points fixed in a body (body >= 0) are placed at X_b + R(Q_b) s_p of the same configuration.
//   k_ens_obs_flags              one thread per replica, behind the probe kernel in a run: its flags enter the replica's error word
//                                only where the step has not failed already
//   k_ens_obs_commit             one thread per entry, after k_ens_commit: where the replica committed, sum += step and
//                                last = step; the frame slot takes last (frame_F's convention, rbl_ens_run.hip)
//
// A point's sum does not depend on NI, on the workgroup's size or on R: replica r of R returns the bits of the R = 1 launch, and
// two launches agree bitwise.  No atomics on doubles, no scratch.  Flags (a blob below the wall, a non-finite result) are ORed
// into a word per replica: the one-shot call's own, or in a run the observers' (k_ens_obs_flags passes them on).
//
// The geometry is ens_probe_geometry, one function of (P, R, CU count).  The sources are never split over workgroups: at R = 1
// with few points the launch is a handful of waves that each walk all N blobs, bound by that walk's latency and not by the
// machine -- accepted, because inside a run the kernel stands beside a solve that is latency-bound in the same way, and a split
// would cost a second launch and a slab for the partial sums.
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"
#include "rbl_small_dev.hpp"

namespace {

constexpr int EP_N_MAX = 256;       // the one-kernel solver's blob limit (rbl_gmres_small_fits)
constexpr int EP_WAVES_MAX = 4;     // waves per workgroup at most: the prologue is shared by 256 NI points

struct __attribute__((aligned(16))) EpBlob {
  double x, y, z, fx, fy, fz;   // radius-scaled position, damped force: three 16-B LDS broadcasts per source
};

struct EpNoCell {};

// x = R s + X, each row's products and sums rounded one after the other (k_body_geom's statements)
__device__ __forceinline__ void ep_place(const double *Rm, const double *X, double s0, double s1, double s2, double &p0, double &p1,
                                         double &p2)
{
#pragma clang fp contract(off)
  const double l0 = s0 * Rm[0] + s1 * Rm[1] + s2 * Rm[2];
  const double l1 = s0 * Rm[3] + s1 * Rm[4] + s2 * Rm[5];
  const double l2 = s0 * Rm[6] + s1 * Rm[7] + s2 * Rm[8];
  p0 = l0 + X[0]; p1 = l1 + X[1]; p2 = l2 + X[2];
}

// CELLS (a cell per replica, rbl_ensemble_set_cells): Cin is the table of R records and the workgroup reads its replica's first, a
// scalar load at a workgroup-uniform index; the sums that follow are those of the launch with that cell by value
template <bool WALL, bool PER, int NI, bool CELLS = false>
__global__ __launch_bounds__(64 * EP_WAVES_MAX) void k_ens_probe(RblParams P, RblEnsProbe A,
                                                                  std::conditional_t<CELLS, const RblEnsCellRec *, std::conditional_t<PER, RblSmallCell, EpNoCell>> Cin)
{
  static_assert(WALL || !PER, "the free-space lattice sum diverges: a cell needs the wall");
  static_assert(PER || !CELLS, "a table of cells is a periodic launch");
  __shared__ EpBlob sj[EP_N_MAX];
  const int r = blockIdx.y, t = threadIdx.x, nt = blockDim.x;
  RblSmallCell C = {};
  if constexpr (CELLS) C = Cin[r].S;
  else if constexpr (PER) C = Cin;
  (void)C;
  const int N = A.Nb * A.nbl;
  const double *X = A.X + (size_t)r * 3 * A.Nb, *Q = A.Q + (size_t)r * 4 * A.Nb;
  const double *lam = A.lam + (size_t)r * (size_t)A.lam_stride;
  unsigned flags = 0;
  // sources: blob j of the replica at the configuration evaluated at
  for (int j = t; j < N; j += nt) {
    const int b = j / A.nbl, k = j - b * A.nbl;
    double Rm[9], p0, p1, p2;
    quat_rot(Q + 4 * b, Rm);
    ep_place(Rm, X + 3 * b, A.cfg[3 * k], A.cfg[3 * k + 1], A.cfg[3 * k + 2], p0, p1, p2);
    double d = 1.0;
    if (WALL) {
      if (p2 < 0.0) flags |= RBL_FLAG_BELOW_WALL;
      d = (p2 >= P.a) ? 1.0 : p2 / P.a;                 // c_rigid_obj.cpp:629-633
    }
    sj[j].x = p0 * P.inv_a; sj[j].y = p1 * P.inv_a; sj[j].z = p2 * P.inv_a;
    sj[j].fx = d * lam[3 * j]; sj[j].fy = d * lam[3 * j + 1]; sj[j].fz = d * lam[3 * j + 2];
  }
  // targets: the lane's NI points, lab points or offsets fixed in a body
  const RblParams Pu = rbl_small_unit_params(P);
  const RblWallK WK = rbl_wall_k_resident<RBL_UNIT_RADIUS>();
  const long q0 = (long)blockIdx.x * ((long)nt * NI);
  const double *pts = A.pts + (size_t)r * (size_t)A.pts_stride;
  double Rb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (A.body >= 0) quat_rot(Q + 4 * A.body, Rb);
  double xi[NI], yi[NI], zi[NI], zp[NI], ux[NI], uy[NI], uz[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    long p = q0 + t + (long)k * nt;
    if (p >= A.P) p = A.P - 1;                          // masked lane: a copy of the last point, never written
    double x0 = pts[3 * p], x1 = pts[3 * p + 1], x2 = pts[3 * p + 2];
    if (A.body >= 0) ep_place(Rb, X + 3 * A.body, x0, x1, x2, x0, x1, x2);
    zp[k] = x2;                                         // the physical height, as apply_M damps with
    xi[k] = x0 * P.inv_a; yi[k] = x1 * P.inv_a; zi[k] = x2 * P.inv_a;
    ux[k] = 0.0; uy[k] = 0.0; uz[k] = 0.0;
  }
  __syncthreads();
#pragma unroll 1     // (NI pairs per source already)
  for (int j = 0; j < N; ++j) {
    const double bx = sj[j].x, by = sj[j].y, bz = sj[j].z, fx = sj[j].fx, fy = sj[j].fy, fz = sj[j].fz;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      if constexpr (PER) {
        double dx = xi[k] - bx, dy = yi[k] - by;
        const double dz = zi[k] - bz;
        dx = __builtin_fma(-C.Lx, rint(dx * C.iLx), dx);   // 1 / L is 0 on an open axis: rint(0) = 0 leaves d alone
        dy = __builtin_fma(-C.Ly, rint(dy * C.iLy), dy);
        const bool coinc = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)) < Pu.tiny2;
        for (int p = -C.nx; p <= C.nx; ++p) {
          const double x = __builtin_fma((double)p, C.Lx, dx);
          for (int q = -C.ny; q <= C.ny; ++q) {
            const double y = __builtin_fma((double)q, C.Ly, dy);
            if (p == 0 && q == 0)   // wave-uniform
              rbl_pair_accum<true, true, RBL_UNIT_RADIUS>(Pu, x, y, zi[k], 0.0, 0.0, bz, fx, fy, fz, coinc, ux[k], uy[k], uz[k], flags, WK);
            else
              rbl_pair_accum<true, false, RBL_UNIT_RADIUS>(Pu, x, y, zi[k], 0.0, 0.0, bz, fx, fy, fz, false, ux[k], uy[k], uz[k], flags, WK);
          }
        }
      } else {
        const double dx = xi[k] - bx, dy = yi[k] - by, dz = zi[k] - bz;
        const bool coinc = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)) < Pu.tiny2;
        rbl_pair_accum<WALL, true, RBL_UNIT_RADIUS>(Pu, xi[k], yi[k], zi[k], bx, by, bz, fx, fy, fz, coinc, ux[k], uy[k], uz[k], flags, WK);
      }
    }
  }
  double *out = A.u + (size_t)r * 3 * (size_t)A.P;
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const long p = q0 + t + (long)k * nt;
    if (p >= A.P) continue;
    double sc = P.nf;
    if (WALL) sc *= (zp[k] >= P.a) ? 1.0 : zp[k] / P.a;
    double vx = sc * ux[k], vy = sc * uy[k], vz = sc * uz[k];
    if (WALL && !(zp[k] > 0.0)) { vx = 0.0; vy = 0.0; vz = 0.0; }   // outside the fluid: u = 0 (d(0) = 0 already)
    if (!(isfinite(vx) && isfinite(vy) && isfinite(vz))) flags |= RBL_FLAG_NONFINITE;
    out[3 * p] = vx; out[3 * p + 1] = vy; out[3 * p + 2] = vz;
  }
  if (flags) atomicOr(A.rerr + r, flags);
}

__global__ __launch_bounds__(256) void k_ens_obs_commit(const int *__restrict__ stopped, const unsigned *__restrict__ vflag,
                                                        const double *__restrict__ step, double *__restrict__ last,
                                                        double *__restrict__ sum, double *__restrict__ frame, long per_rep, long n)
{
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const long r = idx / per_rep;
  const bool ok = stopped[0] == 0 && vflag[r] == 0;    // k_ens_commit's decision
  double v = last[idx];
  if (ok) { v = step[idx]; last[idx] = v; sum[idx] += v; }
  if (frame) frame[idx] = v;
}

// One thread per replica, between the probe kernel and the update of a run's step: the probe kernel's flags of the step (oerr, its
// own words) enter the replica's error word only where the step has not failed already, and oerr is cleared for the next step.  A
// replica whose solve failed keeps exactly the word the unobserved run gives it
__global__ __launch_bounds__(256) void k_ens_obs_flags(unsigned *__restrict__ rerr, unsigned *__restrict__ oerr, int R)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const unsigned f = oerr[r];
  if (!f) return;
  if (rerr[r] == 0) rerr[r] = f;
  oerr[r] = 0;
}

template <bool WALL, bool PER, int NI>
void ep_launch(hipStream_t st, const RblParams &P, const RblSmallCell *cell, const RblEnsCellRec *cells, const RblEnsProbe &A, int R,
               const RblEnsProbeGeom &g)
{
  const dim3 grid((unsigned)g.tiles, (unsigned)R), block((unsigned)(64 * g.waves));
  if constexpr (PER) {
    if (cells) hipLaunchKernelGGL((k_ens_probe<WALL, true, NI, true>), grid, block, 0, st, P, A, cells);
    else hipLaunchKernelGGL((k_ens_probe<WALL, true, NI>), grid, block, 0, st, P, A, *cell);
  } else hipLaunchKernelGGL((k_ens_probe<WALL, false, NI>), grid, block, 0, st, P, A, EpNoCell{});
}

template <bool WALL, bool PER>
void ep_launch_ni(hipStream_t st, const RblParams &P, const RblSmallCell *cell, const RblEnsCellRec *cells, const RblEnsProbe &A, int R,
                  const RblEnsProbeGeom &g)
{
  if (g.NI == 4) ep_launch<WALL, PER, 4>(st, P, cell, cells, A, R, g);
  else if (g.NI == 2) ep_launch<WALL, PER, 2>(st, P, cell, cells, A, R, g);
  else ep_launch<WALL, PER, 1>(st, P, cell, cells, A, R, g);
}

// the one-shot field's argument checks that need no device; *noop: n_points == 0
int ep_check_args(rbl_ctx *c, const char *who, const double *points, int64_t n_points, int point_sets, int probe_body, const double *lambda,
                  const double *u, bool host, bool *noop)
{
  *noop = false;
  if (!c) return RBL_ERR_ARG;
  const std::string w(who);
  if (periodic_on(c)) return periodic_refuse(c, who);
  if (n_points < 0) return rbl_fail(c, RBL_ERR_ARG, w + ": n_points must be >= 0");
  if (n_points == 0) { *noop = true; return RBL_OK; }
  if (!points || !lambda || !u) return rbl_fail(c, RBL_ERR_ARG, w + ": points, lambda or u is NULL");
  if (n_points > 0x7fffffffLL / 3) return rbl_fail(c, RBL_ERR_SIZE, w + ": n_points must stay below 2^31 / 3");
  if (point_sets < 1) return rbl_fail(c, RBL_ERR_ARG, w + ": point_sets must be 1 or R");
  if (probe_body < -1) return rbl_fail(c, RBL_ERR_ARG, w + ": probe_body must be -1 (lab points) or a body index");
  int rc = need_params(c); if (rc) return rc;
  if ((rc = ens_state_check(c, std::string(who) + ": "))) return rc;
  if (point_sets != 1 && point_sets != c->ens_R)
    return rbl_fail(c, RBL_ERR_ARG, w + ": point_sets must be 1 or R = " + std::to_string(c->ens_R));
  if (probe_body >= c->ens_Nb)
    return rbl_fail(c, RBL_ERR_ARG, w + ": probe_body must be -1 (lab points) or a body index below N_bod = " + std::to_string(c->ens_Nb));
  if (host) return ens_points_check(c, who, points, n_points, point_sets);
  return RBL_OK;
}

// enqueue, read the replicas' words back, name the first failing replica
int ep_run(rbl_ctx *c, const RblEnsView &v, const double *d_pts, int64_t n_points, int point_sets, int probe_body, const double *d_lam,
           double *d_u, unsigned *d_err)
{
  const int R = v.R;
  const long n3 = 3L * v.Nb * v.nbl;
  RBL_HIP(c, hipMemsetAsync(d_err, 0, sizeof(unsigned) * (size_t)R, c->stream));
  const RblEnsProbe A = {v.X, v.Q, v.cfg, d_lam, n3, d_pts, point_sets == 1 ? 0L : 3L * (long)n_points, d_u, d_err, v.Nb, v.nbl,
                         (int)n_points, probe_body};
  {
    RblPhase ph(c, RBL_T_PRODUCT);
    ens_probe_launch(c->stream, rbl_make_params(c->S.a, c->S.eta), c->S.wall, v.cell ? &v.C : nullptr, A, R, c->n_cu,
                     v.cell ? v.cells : nullptr);
    RBL_HIP(c, hipGetLastError());
  }
  std::vector<unsigned> h((size_t)R);
  int rc = read_back(c, h.data(), d_err, sizeof(unsigned) * (size_t)R); if (rc) return rc;
  for (int r = 0; r < R; ++r)
    if (h[(size_t)r]) {
      rc = rbl_flags_to_status(c, h[(size_t)r]);
      c->last_error = "ensemble_velocity_field: replica " + std::to_string(r) + ": " + c->last_error;
      return rc;
    }
  return RBL_OK;
}

}  // namespace

// a non-finite coordinate of points[sets 3 P] is RBL_ERR_ARG naming the set and the point (shared with rbl_ensemble_run_observed)
int ens_points_check(rbl_ctx *c, const char *who, const double *points, int64_t n_points, int sets)
{
  for (int s = 0; s < sets; ++s)
    for (int64_t p = 0; p < n_points; ++p) {
      const double *x = points + 3 * ((size_t)s * (size_t)n_points + (size_t)p);
      if (!(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2])))
        return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": points: set " + std::to_string(s) + ", point " + std::to_string(p) +
                                            " has a non-finite coordinate");
    }
  return RBL_OK;
}

// NI: points per lane.  More of them share one LDS read of a source, fewer spread a small job over more waves: 2 (4) once every
// CU gets eight waves of that size.  waves: as many as the points of one replica fill, four at most -- the prologue (the
// replica's blobs placed and staged) is paid once per workgroup
RblEnsProbeGeom ens_probe_geometry(int64_t n_points, int R, int n_cu)
{
  RblEnsProbeGeom g;
  const int64_t cu = n_cu > 0 ? n_cu : 256, lanes = (int64_t)R * n_points;
  g.NI = lanes >= 64 * 4 * 8 * cu ? 4 : lanes >= 64 * 2 * 8 * cu ? 2 : 1;
  const int64_t per_wave = 64 * (int64_t)g.NI;
  g.waves = (int)std::min<int64_t>(EP_WAVES_MAX, std::max<int64_t>(1, (n_points + per_wave - 1) / per_wave));
  const int64_t per_wg = per_wave * g.waves;
  g.tiles = (n_points + per_wg - 1) / per_wg;
  return g;
}

void ens_probe_launch(hipStream_t st, const RblParams &P, bool wall, const RblSmallCell *cell, const RblEnsProbe &A, int R, int n_cu,
                      const RblEnsCellRec *cells)
{
  if (A.P <= 0) return;
  const RblEnsProbeGeom g = ens_probe_geometry(A.P, R, n_cu);
  if (cell || cells) ep_launch_ni<true, true>(st, P, cell, cells, A, R, g);   // (a cell needs the wall: the callers' periodic_use_check)
  else if (wall) ep_launch_ni<true, false>(st, P, nullptr, nullptr, A, R, g);
  else ep_launch_ni<false, false>(st, P, nullptr, nullptr, A, R, g);
}

void ens_obs_flags_launch(hipStream_t st, unsigned *d_rerr, unsigned *d_oerr, int R)
{
  hipLaunchKernelGGL(k_ens_obs_flags, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, d_rerr, d_oerr, R);
}

// ---- the observers as a part of a run (RblEnsObsRun): bytes, begin, after the commit, end ----------------------------------------
size_t ens_obs_carve(RblEnsObsRun &O, void *base, int R, int Nb, size_t n_frames)
{
  const size_t Rz = (size_t)R;
  O.nu = Rz * 3 * (size_t)O.o->n_probes;
  O.nD = O.o->moments ? Rz * 9 * (size_t)Nb : 0;
  RblCarve C{(char *)base};
  O.step.pts = C.take<double>(O.nu ? 3 * (size_t)O.o->n_probes * (size_t)O.o->point_sets : 0);
  O.step.u_step = C.take<double>(O.nu); O.u_last = C.take<double>(O.nu); O.u_sum = C.take<double>(O.nu);
  O.step.D_step = C.take<double>(O.nD); O.D_last = C.take<double>(O.nD); O.D_sum = C.take<double>(O.nD);
  O.fU = C.take<double>(n_frames * O.nu); O.fD = C.take<double>(n_frames * O.nD);
  O.step.oerr = C.take<unsigned>(O.nu ? Rz : 0);
  return C.off;
}

int ens_obs_begin(rbl_ctx *c, RblEnsObsRun &O, void *base, int R, int Nb, size_t n_frames)
{
  ens_obs_carve(O, base, R, Nb, n_frames);
  O.step.P = O.o->n_probes; O.step.sets = O.o->point_sets; O.step.body = O.o->probe_body; O.step.moments = O.o->moments != 0;
  int rc;
  if (O.nu) {
    if ((rc = copy_h2d(c, (void *)O.step.pts, O.o->points, sizeof(double) * 3 * (size_t)O.o->n_probes * (size_t)O.o->point_sets))) return rc;
    RBL_HIP(c, hipMemsetAsync(O.u_last, 0, sizeof(double) * O.nu, c->stream));
    RBL_HIP(c, hipMemsetAsync(O.u_sum, 0, sizeof(double) * O.nu, c->stream));
    RBL_HIP(c, hipMemsetAsync(O.step.oerr, 0, sizeof(unsigned) * (size_t)R, c->stream));
  }
  if (O.nD) {
    RBL_HIP(c, hipMemsetAsync(O.D_last, 0, sizeof(double) * O.nD, c->stream));
    RBL_HIP(c, hipMemsetAsync(O.D_sum, 0, sizeof(double) * O.nD, c->stream));
  }
  return RBL_OK;
}

// k_ens_obs_commit for u and for D, n = R per_rep entries each; frame >= 0: a recording step's slot
void ens_obs_after(rbl_ctx *c, const RblEnsObsRun &O, int R, const int *d_stopped, const unsigned *d_vflag, long frame)
{
  auto commit = [&](const double *step, double *last, double *sum, double *frames, size_t n) {
    if (n)
      hipLaunchKernelGGL(k_ens_obs_commit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_stopped, d_vflag, step, last, sum,
                         frame >= 0 ? frames + (size_t)frame * n : nullptr, (long)(n / (size_t)R), (long)n);
  };
  commit(O.step.u_step, O.u_last, O.u_sum, O.fU, O.nu);
  commit(O.step.D_step, O.D_last, O.D_sum, O.fD, O.nD);
}

int ens_obs_end(rbl_ctx *c, const RblEnsObsRun &O, size_t nfr)
{
  rbl_run_obs_out *q = O.out;
  int rc;
  if (O.nu && q->u_sum && (rc = copy_d2h(c, q->u_sum, O.u_sum, sizeof(double) * O.nu))) return rc;
  if (O.nD && q->D_sum && (rc = copy_d2h(c, q->D_sum, O.D_sum, sizeof(double) * O.nD))) return rc;
  if (nfr && O.nu && (rc = copy_d2h(c, q->frame_u, O.fU, sizeof(double) * nfr * O.nu))) return rc;
  if (nfr && O.nD && (rc = copy_d2h(c, q->frame_D, O.fD, sizeof(double) * nfr * O.nD))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

// ---- C ABI (include/rbl.h section 5, observers) ---------------------------------------------------------------------

int rbl_ensemble_velocity_field_dev(rbl_ctx *c, const double *d_points, int64_t n_points, int point_sets, int probe_body,
                                    const double *d_lambda, double *d_u)
{
  bool noop;
  int rc = ep_check_args(c, "ensemble_velocity_field_dev", d_points, n_points, point_sets, probe_body, d_lambda, d_u, false, &noop);
  if (rc || noop) return rc;
  RblEnsView v;
  if ((rc = ens_view(c, &v))) return rc;
  if ((rc = rbl_dev_reserve(c, c->d_ens_obs, sizeof(unsigned) * (size_t)v.R))) return rc;
  return ep_run(c, v, d_points, n_points, point_sets, probe_body, d_lambda, d_u, (unsigned *)c->d_ens_obs.p);
}

int rbl_ensemble_velocity_field(rbl_ctx *c, const double *points, int64_t n_points, int point_sets, int probe_body, const double *lambda,
                                double *u)
{
  bool noop;
  int rc = ep_check_args(c, "ensemble_velocity_field", points, n_points, point_sets, probe_body, lambda, u, true, &noop);
  if (rc || noop) return rc;
  RblEnsView v;
  if ((rc = ens_view(c, &v))) return rc;
  // staging: [points sets 3P | lambda R 3N | u R 3P | error words R]
  const size_t np = 3 * (size_t)n_points * (size_t)point_sets, nl = (size_t)v.R * 3 * (size_t)v.Nb * (size_t)v.nbl,
               nu = (size_t)v.R * 3 * (size_t)n_points;
  if ((rc = rbl_dev_reserve(c, c->d_ens_obs, sizeof(double) * (np + nl + nu) + sizeof(unsigned) * (size_t)v.R))) return rc;
  double *d_pts = (double *)c->d_ens_obs.p, *d_lam = d_pts + np, *d_u = d_lam + nl;
  if ((rc = copy_h2d(c, d_pts, points, sizeof(double) * np))) return rc;
  if ((rc = copy_h2d(c, d_lam, lambda, sizeof(double) * nl))) return rc;
  if ((rc = ep_run(c, v, d_pts, n_points, point_sets, probe_body, d_lam, d_u, (unsigned *)(d_u + nu)))) return rc;
  if ((rc = copy_d2h(c, u, d_u, sizeof(double) * nu))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

int rbl_ensemble_probe_info(const rbl_ctx *cc, int64_t n_points, int *ni, int *waves, int64_t *tiles)
{
  rbl_ctx *c = const_cast<rbl_ctx *>(cc);
  if (!c) return RBL_ERR_ARG;
  if (n_points < 0) return rbl_fail(c, RBL_ERR_ARG, "ensemble_probe_info: n_points must be >= 0");
  int rc = ens_state_check(c, "ensemble_probe_info: "); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const RblEnsProbeGeom g = ens_probe_geometry(n_points, c->ens_R, c->n_cu);
  if (ni) *ni = g.NI;
  if (waves) *waves = g.waves;
  if (tiles) *tiles = g.tiles;
  return RBL_OK;
}
