// rbl_ensemble.hip -- ensembles of R independent replicas of one small system (include/rbl.h section 5).
//
// All replicas share the context's structure, parameters (a, eta, dt, kBT), wall flag and force model; each has its own X
// and Q, resident on the device.  One ensemble step advances every replica with a fixed number of launches whatever R is:
// the scheme of rbl_step_deterministic / rbl_step_brownian (the reference's stochastic midpoint step with RFD,
// c_rigid_obj.cpp:917-976), with the host loops over bodies of the single-system path moved onto the device and the
// replicas riding in the grid:
//
//   k_normal (batched)        noise: replica r draws 3 n3 normals from Philox offset r ceil(3 n3 / 2)
//   k_body_geom               lever arms + blob positions of all R N_bod bodies
//   force model               k_body_neighbours with a replica window, k_blob_interactions, K^T f   (rbl_forces.hip)
//   k_build_M (batched)       B M B of every replica (one matrix per replica, its flags in the replica's error word)
//   batched Cholesky, k_block_trmv (x2)   M^1/2 W1, M^1/2 W2 of every replica
//   k_ens_midpoint            per body: Kinv W_rfd (the RFD direction) and the predictor q^{n+1/2} (update_X_Q, :798-863)
//   k_ens_rfd_rhs             per replica (one workgroup): (1/delta)[M(q + delta/2 dq) - M(q - delta/2 dq)] W_rfd with the pair
//                             sweep of the one-kernel solver, then the right-hand side [slip - kBT M_RFD - BI ; -F]
//   k_gmres_small (grid R)    the saddle solve of every replica at q^{n+1/2}
//   k_ens_evolve              per body: q^{n+1} = update_X_Q(q^n, dt U)
//
// followed by ONE read-back (iterations, residuals, one error word per replica).  The step writes the other of two
// configuration buffers and commits (swaps) only when every replica succeeded: on any error no replica moves.
// Replicas never interact: the pair sweeps are per replica, the force model's neighbour lists stop at the replica's bodies.
//
// With prescribed bodies (rbl_ensemble_solve_mixed / _step_mixed / _step_brownian_mixed and their _dof forms; the semantics of
// include/rbl.h section 7 per replica, the restatement of rbl_mixed.hip's mx_solve / mx_step and of rbl_steps.hip's
// rhs_and_midpoint_core): a 0/1 mask travels with the call, one entry per body and replica or (the _dof forms, runs with
// prescribed_per = 6) one per velocity component, and NULL for it is the unmasked step: ens_step_det and ens_step_bd serve all.
// `per`, the entries per body, is decided once at the exported function; the mask goes up as the caller gave it and every kernel
// that reads it is told per (mx_lane_bits / mx_bits, rbl_body_dev.hpp).  In the Brownian step a mask per component must have every
// body's rotation entries all equal; a Brownian RUN with such a mask stays refused.
// The same launches with three differences: k_ens_midpoint is followed by k_ens_midpoint_masked (dq = 0 and the predictor
// displacement (dt/2) U_p on a prescribed component; one more launch, so that a free body goes through the very same code), the
// solve is the masked k_gmres_small (it adds K_p U_p to the right-hand side with the lever arms of the configuration it solves at, zeroes
// the prescribed bodies' balance rows and splits the solution into U and F per body), and
// k_ens_evolve reads the U the solver wrote.  The right-hand-side kernels are the unmasked ones: body_in stands where F_body stood,
// so the model's K^T f reaches the bottom rows of the free bodies and what they write on a prescribed body's rows is overwritten
// by the solver.  U and F follow the error words in the ONE read-back.  A free body's arithmetic and its order are unchanged: with
// nobody prescribed the configurations and iteration counts are bitwise those of the unmasked steps.
//
// Each step function is an enqueueing part (ens_enqueue_det / ens_enqueue_bd) and a finish (ens_finish: the read-back, the host's
// verdict, the swap); the one-step calls are the two in a row.  A run of n steps in one call (rbl_ensemble_run and its jointed,
// observed and driven forms) is rbl_ens_run.hip: it enqueues the first part per step with the inputs resident, and its observers
// reach a step as an argument (EnsObs in EnsStepIn), never as context state: without them nothing here launches anything else.
//
// In a periodic cell (rbl_ensemble_set_periodic; the cell's state and checks are in rbl_periodic.hip): the same launches with the
// cell's instantiations -- k_gmres_small_per (rbl_small_per.hip) and k_ens_rfd_rhs<true, true> (the image sum inside rbl_small_pair_sweep),
// k_build_M_per for the dense root, the minimum-image force kernels (ia_eval_batch passes the ensemble's cell).  The jointed calls
// are refused with the cell on.  Cell off: nothing here launches anything else than before.
// With a cell PER REPLICA (rbl_ensemble_set_cells): the same launches again with the forms that read the replica's cell from the
// table of R records on the device (ens_cell_table) -- k_gmres_small_cells (rbl_small_cells.hip), k_ens_rfd_rhs<true, true, true>,
// k_build_M_cells, the probe kernel's and the force kernels' table forms.  ens_cell_use is the one check at use, per replica.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"
#include "rbl_small_dev.hpp"

namespace {

constexpr int ET = 256;          // threads of the per-body / per-entry kernels
constexpr int EW = RBL_SG_THREADS / 64;
constexpr int ENS_R_MAX = 65535;

// (ens_update_body, update_X_Q of one body: rbl_body_dev.hpp, shared with the Metropolis sampler)

// Kinv V = (K^T K)^-1 K^T V of one body (:390, :406): the K^T sums over its blobs in blob order, then the 6 x 6 blocks of
// (K^T K)^-1 = diag(1/N_blb I, (sum |c|^2 I - R MOI R^T)^-1) (:302-326; the reference configuration has its mean removed)
__device__ void ens_kinv_body(const double *R, const double *cfg, int nbl, const double *V, double *out)
{
  double f[6] = {0, 0, 0, 0, 0, 0}, sumr2 = 0.0, MOI[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < nbl; ++k) {
    const double c0 = cfg[3 * k], c1 = cfg[3 * k + 1], c2 = cfg[3 * k + 2];
    double l0, l1, l2;
    {
#pragma clang fp contract(off)
      l0 = c0 * R[0] + c1 * R[1] + c2 * R[2];
      l1 = c0 * R[3] + c1 * R[4] + c2 * R[5];
      l2 = c0 * R[6] + c1 * R[7] + c2 * R[8];
    }
    const double *v = V + 3 * k;
    f[0] += v[0]; f[1] += v[1]; f[2] += v[2];
    f[3] += l1 * v[2] - l2 * v[1];
    f[4] += l2 * v[0] - l0 * v[2];
    f[5] += l0 * v[1] - l1 * v[0];
    const double cc[3] = {c0, c1, c2};
    sumr2 += c0 * c0 + c1 * c1 + c2 * c2;
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) MOI[3 * p + q] += cc[p] * cc[q];
  }
  double T[9], D[9];
  for (int p = 0; p < 3; ++p)
    for (int q = 0; q < 3; ++q) T[3 * p + q] = R[3 * p] * MOI[q] + R[3 * p + 1] * MOI[3 + q] + R[3 * p + 2] * MOI[6 + q];
  for (int p = 0; p < 3; ++p)
    for (int q = 0; q < 3; ++q)
      D[3 * p + q] = (p == q ? sumr2 : 0.0) - (T[3 * p] * R[3 * q] + T[3 * p + 1] * R[3 * q + 1] + T[3 * p + 2] * R[3 * q + 2]);
  const double c00 = D[4] * D[8] - D[5] * D[7], c01 = D[5] * D[6] - D[3] * D[8], c02 = D[3] * D[7] - D[4] * D[6];
  const double id = 1.0 / (D[0] * c00 + D[1] * c01 + D[2] * c02);   // non-singular: checked once for the structure (set_config)
  const double S[9] = {c00 * id, (D[2] * D[7] - D[1] * D[8]) * id, (D[1] * D[5] - D[2] * D[4]) * id,
                       c01 * id, (D[0] * D[8] - D[2] * D[6]) * id, (D[2] * D[3] - D[0] * D[5]) * id,
                       c02 * id, (D[1] * D[6] - D[0] * D[7]) * id, (D[0] * D[4] - D[1] * D[3]) * id};
  const double ainv = 1.0 / (1.0 * nbl);
  for (int p = 0; p < 3; ++p) out[p] = ainv * f[p];
  for (int p = 0; p < 3; ++p) out[3 + p] = (S[3 * p] * f[3] + S[3 * p + 1] * f[4]) + S[3 * p + 2] * f[5];
}

// right-hand side of the deterministic step: [slip (or 0) ; -(F - FT) ; jr (or 0)] per replica (FT: the model's K^T f_phys, or
// NULL; the nj3 = 3 n_joints joint rows of the jointed step, none otherwise)
__global__ __launch_bounds__(ET) void k_ens_rhs_jt(int R, int n3, int nb6, int nj3, const double *__restrict__ slip, const double *__restrict__ F,
                                                   const double *__restrict__ FT, const double *__restrict__ jr, double *__restrict__ rhs)
{
  const long nsys = (long)n3 + nb6 + nj3, idx = (long)blockIdx.x * ET + threadIdx.x;
  if (idx >= (long)R * nsys) return;
  const long r = idx / nsys, e = idx - r * nsys;
  if (e < n3) { rhs[idx] = slip ? slip[r * n3 + e] : 0.0; return; }
  if (e >= n3 + nb6) { rhs[idx] = jr ? jr[r * nj3 + e - n3 - nb6] : 0.0; return; }
  double f = F[r * nb6 + e - n3];
  if (FT) f = 1.0 * f + -1.0 * FT[r * nb6 + e - n3];                 // F_body - K^T f_phys (include/rbl.h section 4)
  rhs[idx] = -1.0 * f + 0.0;                                           // Force *= -1 (:972)
}

// per body: dq = Kinv W_rfd (the RFD direction, :776) and the predictor q^{n+1/2} = update_X_Q(q^n, scale Kinv M^1/2 W1)
// (:955-959, scale = dt/2 c1).  W: [W1 | W2 | W_rfd] per replica (3 n3), MW: [M^1/2 W1 | M^1/2 W2 | unused] per replica (3 n3,
// the stride of W: k_block_trmv takes one vector stride)
__global__ __launch_bounds__(ET) void k_ens_midpoint(int nbod, int Nb, int nbl, const double *__restrict__ X,
                                                     const double *__restrict__ Q, const double *__restrict__ cfg,
                                                     const double *__restrict__ W, const double *__restrict__ MW, double scale,
                                                     double *__restrict__ dq, double *__restrict__ Xh, double *__restrict__ Qh)
{
  const int g = blockIdx.x * ET + threadIdx.x;
  if (g >= nbod) return;
  const int r = g / Nb, b = g - r * Nb;
  const size_t n3 = (size_t)3 * Nb * nbl, boff = (size_t)3 * b * nbl;
  double Rm[9];
  rbl_quat_rot9(Q + 4 * (size_t)g, Rm);
  ens_kinv_body(Rm, cfg, nbl, W + (size_t)r * 3 * n3 + 2 * n3 + boff, dq + 6 * (size_t)g);
  double u[6];
  ens_kinv_body(Rm, cfg, nbl, MW + (size_t)r * 3 * n3 + boff, u);
  for (int p = 0; p < 6; ++p) u[p] *= scale;
  ens_update_body(X + 3 * (size_t)g, Q + 4 * (size_t)g, u, Xh + 3 * (size_t)g, Qh + 4 * (size_t)g);
}

// k_ens_midpoint with a mask (per entries per body, body_in[6 nbod]) is k_ens_midpoint itself on every body, then
// k_ens_midpoint_masked on the bodies with any component prescribed: a prescribed component takes no random displacement -- dq = 0
// -- and moves by (dt/2) U_p in the predictor (k_mx_bd_sums, rbl_body_dev.hip, and the host loop of rhs_and_midpoint_core,
// rbl_steps.hip).  One kernel with the free and the prescribed case as branches was tried: the compiler joins the branches' common
// tail (the update), scale * u of a free body then no longer fuses into X + u as it does in k_ens_midpoint, and a free body's
// configuration differs in the last bit from the unmasked step's.  Running the unmasked kernel first and leaving the free bodies
// alone here gives the same bits by construction, for one more small launch per step.
//
// A body with all six components prescribed (every prescribed body of a whole-body mask) sits at q^n + (dt/2) U_p.  Its
// statements stand in a function of their own, out of line, so that the compiler contracts them the same way whatever surrounds
// the call: whole rows of a component mask give the whole-body step's bits.
__device__ __noinline__ void ens_midpoint_whole_body(const double *X, const double *Q, const double *body_in, double half_dt, double *dq,
                                                     double *Xh, double *Qh)
{
  double u[6];
  for (int p = 0; p < 6; ++p) { dq[p] = 0.0; u[p] = half_dt * body_in[p]; }
  ens_update_body(X, Q, u, Xh, Qh);
}

// A partly prescribed body (per = 6 only; its rotation entries all equal: the entry point has checked it) keeps k_ens_midpoint's dq
// on its free components (D_f Kinv W_rfd: (K^T K)^-1 has no translation-rotation coupling) and gets 0 on the prescribed ones; its
// predictor displacement is (dt/2) U_p on the prescribed components and scale Kinv M^1/2 W1, computed again here, on the free
// ones, taken in ONE update_X_Q.  One thread per body: the bit set differs lane by lane (mx_lane_bits, nothing broadcast)
__global__ __launch_bounds__(ET) void k_ens_midpoint_masked(int nbod, int Nb, int nbl, const double *__restrict__ X,
                                                            const double *__restrict__ Q, const double *__restrict__ cfg,
                                                            const unsigned char *__restrict__ mask, int per,
                                                            const double *__restrict__ body_in, const double *__restrict__ MW,
                                                            double scale, double half_dt, double *__restrict__ dq,
                                                            double *__restrict__ Xh, double *__restrict__ Qh)
{
  const int g = blockIdx.x * ET + threadIdx.x;
  if (g >= nbod) return;
  const unsigned pm = mx_lane_bits(mask, per, (size_t)g);
  if (!pm) return;
  if (pm == 63u) {
    ens_midpoint_whole_body(X + 3 * (size_t)g, Q + 4 * (size_t)g, body_in + 6 * (size_t)g, half_dt, dq + 6 * (size_t)g, Xh + 3 * (size_t)g,
                            Qh + 4 * (size_t)g);
    return;
  }
  const int r = g / Nb, b = g - r * Nb;
  const size_t n3 = (size_t)3 * Nb * nbl, boff = (size_t)3 * b * nbl;
  double Rm[9], u[6];
  rbl_quat_rot9(Q + 4 * (size_t)g, Rm);
  ens_kinv_body(Rm, cfg, nbl, MW + (size_t)r * 3 * n3 + boff, u);
  for (int p = 0; p < 6; ++p) {
    const bool pres = pm >> p & 1u;
    if (pres) dq[6 * (size_t)g + p] = 0.0;
    u[p] = pres ? half_dt * body_in[6 * (size_t)g + p] : scale * u[p];
  }
  ens_update_body(X + 3 * (size_t)g, Q + 4 * (size_t)g, u, Xh + 3 * (size_t)g, Qh + 4 * (size_t)g);
}

// One workgroup per replica: the random finite difference of the mobility along dq (m_rfd_dir: positions at q +- delta/2 dq,
// B M B W_rfd at each, (1/delta) difference) and the right-hand side of the stochastic step (rbl_RHS_and_Midpoint_dev):
//   top = slip - kBT M_RFD - c2 M^1/2 W1 (+ c2 M^1/2 W2 with split_rand),  bottom = -(F - FT).
// Also checks the replica's dense factor: a diagonal entry that is not positive and finite is RBL_FLAG_NOT_SPD.
// PER (the ensemble's periodic cell, wall only): both products are the cell's -- the pair sweep sums over the images and takes in
// every blob's own; the cell is one more kernel argument (an empty one otherwise: the two open instantiations keep their code).
// CELLS (a cell per replica, rbl_ensemble_set_cells): the argument is the table of R records, and the workgroup reads its
// replica's before anything else -- a scalar load at a workgroup-uniform index, so the cell sits in scalar registers as before.
struct EnsNoCell {};
template <bool WALL, bool PER = false, bool CELLS = false>
__global__ __launch_bounds__(RBL_SG_THREADS) void k_ens_rfd_rhs(RblParams P, int Nb, int nbl, const double *__restrict__ X,
                                                                const double *__restrict__ Q, const double *__restrict__ cfg,
                                                                const double *__restrict__ dq, double delta,
                                                                const double *__restrict__ W, const double *__restrict__ MW,
                                                                const double *__restrict__ Lm, const double *__restrict__ slip,
                                                                const double *__restrict__ F, const double *__restrict__ FT,
                                                                double kBT, double c2, int split, double *__restrict__ rhs,
                                                                unsigned *__restrict__ rerr,
                                                                std::conditional_t<CELLS, const RblEnsCellRec *, std::conditional_t<PER, RblSmallCell, EnsNoCell>> C = {})
{
  static_assert(PER || !CELLS, "a table of cells is a periodic launch");
  extern __shared__ double sm[];
  const int r = blockIdx.x, t = threadIdx.x;
  RblSmallCell Cr = {};
  if constexpr (CELLS) Cr = C[r].S;
  else if constexpr (PER) Cr = C;
  (void)Cr;
  const int N = Nb * nbl, n3 = 3 * N, nb6 = 6 * Nb;
  double *pos = sm, *dmp = pos + n3, *su = dmp + N, *vin = su + n3, *acc = vin + n3, *Xs = acc + n3, *Qs = Xs + 3 * Nb,
         *part = Qs + 4 * Nb;
  const RblParams Pu = rbl_small_unit_params(P);
  unsigned flags = 0;
  X += (size_t)r * 3 * Nb; Q += (size_t)r * 4 * Nb; dq += (size_t)r * nb6;
  for (int i = t; i < n3; i += RBL_SG_THREADS) vin[i] = W[(size_t)r * 3 * n3 + 2 * n3 + i];
  const double id = 1.0 / delta;
  for (int sgn = 0; sgn < 2; ++sgn) {
    if (t < Nb) {                                      // q +- delta/2 dq (:783-788)
      const double f = (sgn == 0 ? 0.5 : -0.5) * delta;
      double u[6];
      for (int p = 0; p < 6; ++p) u[p] = f * dq[6 * t + p];
      ens_update_body(X + 3 * t, Q + 4 * t, u, Xs + 3 * t, Qs + 4 * t);
    }
    __syncthreads();
    if (t < N) {                                       // positions / a, wall damping (:629-633), self block
      const int b = t / nbl, k = t - b * nbl;
      double Rm[9];
      rbl_quat_rot9(Qs + 4 * b, Rm);
      const double c0 = cfg[3 * k], c1 = cfg[3 * k + 1], c2_ = cfg[3 * k + 2];
      double p0, p1, p2;
      {
#pragma clang fp contract(off)
        p0 = c0 * Rm[0] + c1 * Rm[1] + c2_ * Rm[2] + Xs[3 * b];
        p1 = c0 * Rm[3] + c1 * Rm[4] + c2_ * Rm[5] + Xs[3 * b + 1];
        p2 = c0 * Rm[6] + c1 * Rm[7] + c2_ * Rm[8] + Xs[3 * b + 2];
      }
      pos[3 * t] = p0 * P.inv_a; pos[3 * t + 1] = p1 * P.inv_a; pos[3 * t + 2] = p2 * P.inv_a;
      double d = 1.0;
      if (WALL) {
        if (p2 < 0.0) flags |= RBL_FLAG_BELOW_WALL;
        d = (p2 >= P.a) ? 1.0 : p2 / P.a;
      }
      dmp[t] = d;
    }
    __syncthreads();
    if (t < N) {
      const double di = dmp[t];
      double ux = 0.0, uy = 0.0, uz = 0.0;
      rbl_pair_accum<WALL, true, RBL_UNIT_RADIUS>(Pu, pos[3 * t], pos[3 * t + 1], pos[3 * t + 2], pos[3 * t], pos[3 * t + 1], pos[3 * t + 2],
                                       di * vin[3 * t], di * vin[3 * t + 1], di * vin[3 * t + 2], true, ux, uy, uz, flags);
      su[3 * t] = ux; su[3 * t + 1] = uy; su[3 * t + 2] = uz;
    }
    if constexpr (PER) rbl_small_pair_sweep<WALL, true>(Pu, pos, dmp, vin, N, part, flags, Cr);
    else rbl_small_pair_sweep<WALL>(Pu, pos, dmp, vin, N, part, flags);
    for (int e = t; e < n3; e += RBL_SG_THREADS) {
      double s = su[e];
      for (int w = 0; w < EW; ++w) s += part[(size_t)w * n3 + e];
      const double u = (WALL ? P.nf * dmp[e / 3] : P.nf) * s;
      if (sgn == 0) acc[e] = u;
      else acc[e] = id * acc[e] + -id * u;             // (1/delta)(M+ W - M- W)  (:793)
    }
    __syncthreads();
  }
  const size_t nsys = (size_t)n3 + nb6;
  for (int e = t; e < n3; e += RBL_SG_THREADS) {       // Slip -= kBT M_RFD + BI   (:948, 953, 963; k_rhs_combine's order)
    const double *mw = MW + (size_t)r * 3 * n3;
    double v = (slip ? slip[(size_t)r * n3 + e] : 0.0) - kBT * acc[e];
    v = v - c2 * mw[e];
    if (split) v = v + c2 * mw[n3 + e];
    if (!isfinite(v)) flags |= RBL_FLAG_NONFINITE;
    rhs[(size_t)r * nsys + e] = v;
    const double dd = Lm[(size_t)r * n3 * n3 + (size_t)e * (n3 + 1)];
    if (!(dd > 0.0) || !isfinite(dd)) flags |= RBL_FLAG_NOT_SPD;
  }
  if (t < nb6) {
    double f = F[(size_t)r * nb6 + t];
    if (FT) f = 1.0 * f + -1.0 * FT[(size_t)r * nb6 + t];
    rhs[(size_t)r * nsys + n3 + t] = -1.0 * f + 0.0;
  }
  if (flags) atomicOr(rerr + r, flags);
}

// per body: q^{n+1} = update_X_Q(q^n, dt U), U = the body block of the replica's saddle solution (evolve_X_Q, :865-878)
__global__ __launch_bounds__(ET) void k_ens_evolve(int nbod, int Nb, long nsys, long n3, double dt, const double *__restrict__ x,
                                                   const double *__restrict__ X, const double *__restrict__ Q,
                                                   double *__restrict__ Xo, double *__restrict__ Qo, unsigned *__restrict__ rerr)
{
  const int g = blockIdx.x * ET + threadIdx.x;
  if (g >= nbod) return;
  const int r = g / Nb, b = g - r * Nb;
  const double *U = x + (size_t)r * nsys + n3 + 6 * (size_t)b;
  double u[6];
  for (int p = 0; p < 6; ++p) u[p] = U[p] * dt;
  double *xo = Xo + 3 * (size_t)g, *qo = Qo + 4 * (size_t)g;
  ens_update_body(X + 3 * (size_t)g, Q + 4 * (size_t)g, u, xo, qo);
  bool ok = true;
  for (int p = 0; p < 3; ++p) ok = ok && isfinite(xo[p]);
  for (int p = 0; p < 4; ++p) ok = ok && isfinite(qo[p]);
  if (!ok) atomicOr(rerr + r, (unsigned)RBL_FLAG_NONFINITE);
}

size_t rfd_lds_bytes(int Nb, int nbl)
{
  const size_t N = (size_t)Nb * nbl;
  return sizeof(double) * (13 * N + 7 * (size_t)Nb + (size_t)EW * 3 * N);
}

}  // namespace

// ---- the host side.  What rbl_ens_run.hip calls is declared in rbl_api_internal.hpp (EnsWork, EnsStepIn, EnsJtStep, the enqueueing
// parts, the state and solver checks); everything else is static ----------------------------------------------------------------------

// nj: the joints of a jointed solve, whose rhs, x and solver workspace hold 3 nj more per replica (0: the sizes of the unjointed one)
static EnsWork ens_carve(void *base, int R, int Nb, int nbl, int max_iter, int nj, size_t *bytes)
{
  const size_t N = (size_t)Nb * nbl, n3 = 3 * N, nb6 = 6 * (size_t)Nb, nsys = n3 + nb6 + 3 * (size_t)nj, Rz = (size_t)R;
  RblCarve C{(char *)base};
  EnsWork w;
  w.resid = C.take<double>(Rz);                        // the read-back block first, contiguous
  w.iters = C.take<int>(Rz);
  w.rerr = C.take<unsigned>(Rz + 1);
  w.gerr = w.rerr ? w.rerr + Rz : nullptr;
  w.rb_bytes = C.off;
  w.U = C.take<double>(Rz * (2 * nb6 + nsys));         // [U | F | x]
  w.Fo = w.U ? w.U + Rz * nb6 : nullptr;
  w.x = w.U ? w.U + 2 * Rz * nb6 : nullptr;
  w.rb_mx_bytes = w.rb_bytes + sizeof(double) * 2 * Rz * nb6;
  w.lever = C.take<double>(Rz * n3); w.pos = C.take<double>(Rz * n3);
  w.F = C.take<double>(Rz * nb6); w.FT = C.take<double>(Rz * nb6); w.slip = C.take<double>(Rz * n3);
  w.W = C.take<double>(Rz * 3 * n3); w.MW = C.take<double>(Rz * 3 * n3);
  w.Lm = C.take<double>(Rz * n3 * n3);
  w.Linv = C.take<double>(rbl_cholesky_batched_work_bytes((int64_t)n3, R) / sizeof(double));
  w.dq = C.take<double>(Rz * nb6); w.Xh = C.take<double>(Rz * 3 * Nb); w.Qh = C.take<double>(Rz * 4 * Nb);
  w.rhs = C.take<double>(Rz * nsys);
  w.mask = C.take<unsigned char>(Rz * nb6);             // room for one entry per velocity component (whole bodies use Rz * Nb of it)
  w.gm = C.take<double>(Rz * rbl_gmres_small_work_doubles(nbl, Nb, max_iter, nj));
  w.jr = C.take<double>(Rz * 3 * (size_t)nj);
  w.e = C.take<double>(Rz * N);
  w.ia = C.take<char>(ia_batch_bytes(Nb, nbl, R));
  *bytes = C.off;
  return w;
}

// the flow model's host-side refusals (wall consistency, n_scale) for the ensemble's body count, made by the step entry points
// and the query before ens_ready touches the device; without an ensemble there is nothing to check (ens_ready says so)
int ens_flow_check(rbl_ctx *c) { return c->ens_R ? flow_check(c, c->ens_Nb) : RBL_OK; }

// pre: the caller's name with ": " behind it, or nothing
static int ens_fail_state(rbl_ctx *c, const std::string &pre = "")
{
  return rbl_fail(c, RBL_ERR_STATE, pre + "ensemble: no ensemble configuration (rbl_ensemble_set_config)");
}

std::string ens_beyond(const std::string &pre)
{
  return pre + "ensemble step: the system is beyond the one-kernel solver (<= 256 blobs, <= 64 bodies, max_iter <= 255)";
}

// the refusals that look at the context's state alone, before any device work: a communicator, no ensemble, a structure changed
// since.  comm_last: ens_ready's order, which looks for the ensemble first
int ens_state_check(rbl_ctx *c, const std::string &pre, bool comm_last)
{
  auto comm = [&] { return rbl_fail(c, RBL_ERR_ARG, pre + "ensemble: not on a context with a communicator (run one ensemble per process)"); };
  if (comm_on(c) && !comm_last) return comm();
  if (!c->ens_R) return ens_fail_state(c, pre);
  if (c->S.N_blb != c->ens_Nblb) return rbl_fail(c, RBL_ERR_STATE, pre + "ensemble: the structure changed since rbl_ensemble_set_config");
  return comm_on(c) ? comm() : RBL_OK;
}

// the ensemble's periodic cell (rbl_ensemble_set_periodic; include/rbl.h section 5): on, and as the one-workgroup kernels take it
bool ens_cell_on(const rbl_ctx *c) { return c->ens_per_on; }
static RblSmallCell ens_cell(const rbl_ctx *c) { return rbl_small_cell(c->S.a, c->ens_per_L, c->ens_per_n); }
// a cell per replica (rbl_ensemble_set_cells): the table on the device, R records -- NULL while the cell is the shared one, and
// every launch that takes a cell then takes ens_cell(c) by value as it always did
static const RblEnsCellRec *ens_cell_table(const rbl_ctx *c)
{
  return ens_cells_stored(c) ? (const RblEnsCellRec *)c->d_ens_cells.p : nullptr;
}

// what a step, a solve or the one-shot field asks of the ensemble's cell at use, before any device work: the wall term and lengths
// the current parameters have not outgrown (periodic_use_check) -- replica by replica with a cell per replica, the first offending
// one named --, then the table in the current parameters' units.  Nothing while the cell is off
static int ens_cell_use(rbl_ctx *c)
{
  if (!ens_cell_on(c)) return RBL_OK;
  if (!ens_cells_stored(c)) return periodic_use_check(c, c->S.wall, c->ens_per_L, "rbl_ensemble_set_periodic");
  int rc;
  for (size_t r = 0; 2 * r < c->ens_cells_L.size(); ++r)
    if ((rc = periodic_use_check(c, c->S.wall, &c->ens_cells_L[2 * r], "rbl_ensemble_set_cells", (int)r))) return rc;
  return ens_cells_upload(c);
}

// what is not offered with the ensemble's cell on: RBL_ERR_STATE before any device work
int ens_cell_refuse(rbl_ctx *c, const char *who)
{
  if (!ens_cell_on(c)) return RBL_OK;
  return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": not offered with the ensemble's periodic cell (rbl_ensemble_set_periodic; switch the cell off first)");
}

// parameters set, ensemble set for the current structure, single GPU; uploads the reference configuration when it changed
int ens_ready(rbl_ctx *c)
{
  int rc = need_params(c); if (rc) return rc;
  if ((rc = ens_state_check(c, "", true))) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (c->ens_cfg_host != c->S.ref_cfg) {
    if ((rc = copy_h2d(c, ens_cfg(c), c->S.ref_cfg.data(), sizeof(double) * c->S.ref_cfg.size()))) return rc;
    c->ens_cfg_host = c->S.ref_cfg;
  }
  return RBL_OK;
}

// the step's flags: the first failing replica names the error; nothing is committed unless every replica succeeded
static int ens_finish(rbl_ctx *c, const EnsWork &w, int R, int *iters, double *resid, bool commit, double *U = nullptr, double *F = nullptr)
{
  const size_t bytes = (U || F) ? w.rb_mx_bytes : w.rb_bytes;
  std::vector<char> h(bytes);
  int rc = read_back(c, h.data(), w.resid, bytes); if (rc) return rc;
  const double *hr = (const double *)h.data();
  const int *hi = (const int *)(h.data() + ((char *)w.iters - (char *)w.resid));
  const unsigned *hf = (const unsigned *)(h.data() + ((char *)w.rerr - (char *)w.resid));
  if (iters) std::memcpy(iters, hi, sizeof(int) * (size_t)R);
  if (resid) std::memcpy(resid, hr, sizeof(double) * (size_t)R);
  for (int r = 0; r < R; ++r)
    if (hf[r]) {
      rc = rbl_flags_to_status(c, hf[r]);
      c->last_error = "ensemble replica " + std::to_string(r) + ": " + c->last_error;
      return rc;
    }
  if (hf[R]) {
    rc = rbl_flags_to_status(c, hf[R]);
    c->last_error = "ensemble: " + c->last_error;
    return rc;
  }
  const size_t ub = sizeof(double) * (size_t)6 * c->ens_Nb * (size_t)R;       // U and F of the masked solve
  if (U) std::memcpy(U, h.data() + w.rb_bytes, ub);
  if (F) std::memcpy(F, h.data() + w.rb_bytes + ub, ub);
  if (commit) c->ens_cur ^= 1;
  if (commit && c->record_mom) { c->ens_mom_R = R; c->ens_mom_nb = c->ens_Nb; }
  return RBL_OK;
}

// ens_finish of a one-step call that returns pieces of the solution: x of every replica (3 N + 6 N_bod + nj3 each) is read back
// in front of it and cut into whichever of lambda, U and phi (the nj3 joint rows) were asked for once the step has succeeded
static int ens_finish_x(rbl_ctx *c, const EnsWork &w, size_t nj3, int *iters, double *resid, bool commit, double *lambda, double *U, double *phi,
                 double *U_mx = nullptr, double *F_mx = nullptr)
{
  const int R = c->ens_R;
  const size_t n3 = (size_t)3 * c->ens_Nb * c->S.N_blb, nb6 = (size_t)6 * c->ens_Nb, nsys = n3 + nb6 + nj3;
  std::vector<double> x;
  int rc;
  if (lambda || U || phi) {
    x.resize((size_t)R * nsys);
    if ((rc = copy_d2h(c, x.data(), w.x, sizeof(double) * x.size()))) return rc;
  }
  if ((rc = ens_finish(c, w, R, iters, resid, commit, U_mx, F_mx))) return rc;
  for (int r = 0; r < R && !x.empty(); ++r) {
    const double *xr = x.data() + (size_t)r * nsys;
    if (lambda) std::memcpy(lambda + (size_t)r * n3, xr, sizeof(double) * n3);
    if (U) std::memcpy(U + (size_t)r * nb6, xr + n3, sizeof(double) * nb6);
    if (phi) std::memcpy(phi + (size_t)r * nj3, xr + n3 + nb6, sizeof(double) * nj3);
  }
  return RBL_OK;
}

// upload F (R 6 N_bod) and slip (R n3 or NULL), clear the read-back block, evaluate the force model at q^n when it is on and
// the caller wants its loads (model): *FT -> K^T f_phys of every replica (NULL otherwise).  The flow model (include/rbl.h
// section 8) goes the same way: one launch adds its term at q^n to every replica's slip.  *SL -> the slip the right-hand side
// takes: the caller's, the term, their sum, or NULL for zero.  resident (a run, rbl_ensemble_run): nothing is uploaded -- w.F
// holds F_body since the run began and slip is the DEVICE copy made then, which the flow model's term is added to into w.slip
// (never in place: the copy serves every step).  accepted (a run): the replicas' step counters, the clock of the magnetic field
static int ens_begin(rbl_ctx *c, const EnsWork &w, const double *F_body, const double *slip, const double **FT, const double **SL,
              bool model = true, bool resident = false, const int *accepted = nullptr)
{
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  const size_t n3 = (size_t)3 * Nb * nbl, nb6 = (size_t)6 * Nb;
  int rc;
  if (!resident) {
    if ((rc = copy_h2d(c, w.F, F_body, sizeof(double) * nb6 * R))) return rc;
    if (slip && (rc = copy_h2d(c, w.slip, slip, sizeof(double) * n3 * R))) return rc;
  }
  RBL_HIP(c, hipMemsetAsync(w.resid, 0, w.rb_bytes, c->stream));
  const double *X = ens_X(c, c->ens_cur), *Q = ens_Q(c, c->ens_cur);
  rbl_launch_body_geom(c->stream, X, Q, ens_cfg(c), nbl, (int64_t)R * Nb * nbl, w.lever, w.pos);
  *FT = nullptr;
  if (model && ia_any(c)) {
    double *f = nullptr;
    if ((rc = ia_eval_batch(c, X, Q, w.pos, w.lever, Nb, R, w.ia, &f, w.FT, nullptr, w.gerr, accepted))) return rc;
    *FT = w.FT;
  }
  bool have_slip = slip != nullptr;
  const bool flow = model && flow_on(c);
  if (flow && (rc = flow_add_batch(c, w.pos, Q, Nb, R, w.slip, &have_slip, resident ? slip : nullptr))) return rc;
  *SL = !have_slip ? nullptr : (resident && !flow) ? slip : w.slip;
  return RBL_OK;
}

// hard joints switched on (include/rbl.h section 9's set, shared by the replicas)
bool ens_jt_active(const rbl_ctx *c) { return c->jt_on && c->jt_n > 0; }

// nj < 0: the joints of the active set, none when they are off
int ens_work(rbl_ctx *c, int max_iter, EnsWork *w, int nj)
{
  if (nj < 0) nj = ens_jt_active(c) ? c->jt_n : 0;
  size_t bytes = 0;
  ens_carve(nullptr, c->ens_R, c->ens_Nb, c->S.N_blb, max_iter, nj, &bytes);
  int rc = rbl_dev_reserve(c, c->d_ens_w, bytes); if (rc) return rc;
  *w = ens_carve(c->d_ens_w.p, c->ens_R, c->ens_Nb, c->S.N_blb, max_iter, nj, &bytes);
  return RBL_OK;
}

int ens_check_solver(rbl_ctx *c, int max_iter)
{
  if (max_iter < 1) return rbl_fail(c, RBL_ERR_ARG, "ensemble step: max_iter must be >= 1");
  if (!rbl_gmres_small_fits(c->S.N_blb, c->ens_Nb, max_iter, false))
    return rbl_fail(c, RBL_ERR_SIZE, ens_beyond());
  return RBL_OK;
}

// The solve of every replica at (Xs, Qs) and the update from q^n: the one place that launches the one-kernel solver.  The variant
// is chosen once -- mixed: the masked solve (w.mask, body_in in w.F); the update then reads the U it wrote (a prescribed body:
// dt U_p exactly); the ensemble's cell on (the wall is: the callers' periodic_use_check): k_gmres_small_per; jt: the jointed
// solve, rhs and x with the joint rows behind.  evolve = false: the solve alone
static int ens_solve_evolve(rbl_ctx *c, const EnsWork &w, const double *Xs, const double *Qs, int max_iter, double rtol, bool mixed = false,
                     bool evolve = true, bool record = true, int per = 1, const EnsJtStep *jt = nullptr, const EnsObs *obs = nullptr)
{
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  const long n3 = 3L * Nb * nbl, nsys = n3 + 6L * Nb + (jt ? 3L * jt->T.n : 0L);
  const RblParams P = rbl_make_params(c->S.a, c->S.eta);
  const RblSmallEns S = {Xs, Qs, ens_cfg(c), nbl, Nb, R, w.rhs, w.x, max_iter, rtol, w.gm, w.iters, w.resid, w.rerr};
  const unsigned char *mask = mixed ? w.mask : nullptr;
  int rc = jt               ? rbl_launch_gmres_small_ens_jt(c->stream, P, c->S.wall, S, jt->T, evolve ? 1 : 0, jt->coef)
           : ens_cell_table(c) && ens_cell_on(c) ? rbl_launch_gmres_small_ens_cells(c->stream, P, ens_cell_table(c), S, mask, w.F, per)
           : ens_cell_on(c) ? rbl_launch_gmres_small_ens_per(c->stream, P, ens_cell(c), S, mask, w.F, per)
                            : rbl_launch_gmres_small_ens(c->stream, P, c->S.wall, S, mask, w.F, per);
  if (rc)
    return rbl_fail(c, rc, jt ? std::string(jt->who) + ": the one-kernel jointed solver does not fit this device's LDS"
                              : std::string("ensemble step: the one-kernel solver does not fit this device's LDS"));
  if (!evolve) return RBL_OK;
  const int nbod = R * Nb;
  if (c->record_mom) c->ens_mom_R = 0;                   // valid once a step committed; a run (record = false) leaves nothing to read
  if (c->record_mom && record) {                         // RBL_OPT_RECORD_MOMENTS: lambda is the top of every replica's x, the lever
                                                         // arms those of the configuration solved at
    if ((rc = rbl_dev_reserve(c, c->d_ens_mom, sizeof(double) * 9 * (size_t)nbod))) return rc;
    flow_launch_moments(c, nullptr, Qs, ens_cfg(c), w.x, Nb, nbod, nsys, (double *)c->d_ens_mom.p);
  }
  if (obs) {                                             // a run's observers: lambda where the solver left it, the configuration solved at
    if (obs->moments) flow_launch_moments(c, nullptr, Qs, ens_cfg(c), w.x, Nb, nbod, nsys, obs->D_step);
    if (obs->P > 0) {
      const RblSmallCell cell = ens_cell(c);
      const RblEnsProbe A = {Xs, Qs, ens_cfg(c), w.x, nsys, obs->pts, obs->sets == 1 ? 0L : 3L * obs->P, obs->u_step, obs->oerr, Nb, nbl,
                             obs->P, obs->body};
      ens_probe_launch(c->stream, P, c->S.wall, ens_cell_on(c) ? &cell : nullptr, A, R, c->n_cu, ens_cell_on(c) ? ens_cell_table(c) : nullptr);
      ens_obs_flags_launch(c->stream, w.rerr, obs->oerr, R);   // into the replica's word, unless its step has failed already
    }
  }
  hipLaunchKernelGGL(k_ens_evolve, dim3((unsigned)((nbod + ET - 1) / ET)), dim3(ET), 0, c->stream, nbod, Nb, mixed ? 6L * Nb : nsys,
                     mixed ? 0L : n3, c->S.dt, mixed ? (const double *)w.U : (const double *)w.x, (const double *)ens_X(c, c->ens_cur),
                     (const double *)ens_Q(c, c->ens_cur), ens_X(c, c->ens_cur ^ 1), ens_Q(c, c->ens_cur ^ 1), w.rerr);
  return RBL_OK;
}

// the checks of the entry points with prescribed bodies: none needs a device
// per: mask entries per body, 1 (whole bodies) or 6 (velocity components, the _dof entry points)
int ens_mx_check(rbl_ctx *c, const char *who, const uint8_t *prescribed, const double *body_in, int max_iter, double rtol, int per)
{
  int rc = need_params(c); if (rc) return rc;
  const std::string w(who);
  const char *pn = per == 6 ? "prescribed6" : "prescribed";
  if (!prescribed || !body_in) return rbl_fail(c, RBL_ERR_ARG, w + ": " + pn + " or body_in is NULL");
  if (max_iter < 1 || !(rtol >= 0.0)) return rbl_fail(c, RBL_ERR_ARG, w + ": need max_iter >= 1 and rtol >= 0");
  const std::string beyond = ens_beyond(w + ": ");
  if (max_iter > 255) return rbl_fail(c, RBL_ERR_SIZE, beyond);
  if ((rc = ens_state_check(c, w + ": "))) return rc;
  const size_t nent = (size_t)c->ens_R * c->ens_Nb * (size_t)per;
  for (size_t g = 0; g < nent; ++g)
    if (prescribed[g] > 1)
      return rbl_fail(c, RBL_ERR_ARG, w + ": entries of " + pn + " must be 0 or 1 (replica " + std::to_string(g / ((size_t)c->ens_Nb * per)) + ")");
  if (!rbl_gmres_small_fits(c->S.N_blb, c->ens_Nb, max_iter, false, true))
    return rbl_fail(c, RBL_ERR_SIZE, rbl_gmres_small_fits(c->S.N_blb, c->ens_Nb, max_iter, false)
                                         ? w + ": this shape fits the one-kernel solver without prescribed bodies, but not with the mask's 6 N_bod doubles of LDS"
                                         : beyond);
  return RBL_OK;
}

// the deterministic step of every replica (checks and ens_ready done by the caller).  prescribed == NULL:
// rbl_ensemble_step_deterministic -- the unmasked solver, lambda, U and F NULL; otherwise body_in stands where F_body stands and
// the solve is the masked one.  move = false: the solve alone, at the current configuration and without the model's loads
// (rbl_ensemble_solve_mixed)

// the mask as the caller gave it: per entries per body (the solver is told which, k_gmres_small's `per`)
int ens_upload_mask(rbl_ctx *c, const EnsWork &w, const uint8_t *prescribed, int per)
{
  return copy_h2d(c, w.mask, prescribed, (size_t)c->ens_R * c->ens_Nb * (size_t)per);
}

// everything the deterministic step enqueues, from the uploads to the update: the one-step calls and the run share it
// jt: the jointed solve or step (move: c of a time step is formed in the solver from the gaps)
int ens_enqueue_det(rbl_ctx *c, const EnsWork &w, const EnsStepIn &in, int max_iter, double rtol, bool move, const EnsJtStep *jt)
{
  const bool mixed = in.prescribed != nullptr;
  const double *FT, *SL;
  int rc;
  if ((rc = ens_cell_use(c))) return rc;
  if (mixed && !in.resident && (rc = ens_upload_mask(c, w, in.prescribed, in.per))) return rc;
  if ((rc = ens_begin(c, w, in.F_body, in.slip, &FT, &SL, move, in.resident, in.accepted))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb;
  const int n3 = 3 * Nb * c->S.N_blb, nb6 = 6 * Nb, nj3 = jt ? 3 * jt->T.n : 0;
  const long tot = (long)R * (n3 + nb6 + nj3);
  hipLaunchKernelGGL(k_ens_rhs_jt, dim3((unsigned)((tot + ET - 1) / ET)), dim3(ET), 0, c->stream, R, n3, nb6, nj3, SL,
                     (const double *)w.F, FT, jt && jt->have_jr ? (const double *)w.jr : nullptr, w.rhs);
  // a jointed step records its moments in a run too, as it always did
  return ens_solve_evolve(c, w, ens_X(c, c->ens_cur), ens_Q(c, c->ens_cur), max_iter, rtol, mixed, move, jt || !in.resident, in.per, jt,
                          in.obs);
}

static int ens_step_det(rbl_ctx *c, const uint8_t *prescribed, const double *F_body, const double *slip, int max_iter, double rtol, bool move,
                 double *lambda, double *U, double *F, int *iters, double *resid, int per = 1)
{
  const bool mixed = prescribed != nullptr;
  EnsWork w;
  int rc;
  if ((rc = ens_work(c, max_iter, &w))) return rc;
  EnsStepIn in;
  in.prescribed = prescribed; in.per = per; in.F_body = F_body; in.slip = slip;
  if ((rc = ens_enqueue_det(c, w, in, max_iter, rtol, move))) return rc;
  std::vector<double> Ft;
  if (mixed && !F) { Ft.resize((size_t)c->ens_R * 6 * c->ens_Nb); F = Ft.data(); }   // the masked read-back is chosen by U or F
  // lambda, the blob forces: the top of every replica's solution; U (unmasked: rbl_ensemble_solve_jointed with the joints off): below it
  return ens_finish_x(c, w, 0, iters, resid, move, lambda, mixed ? nullptr : U, nullptr, mixed ? U : nullptr, mixed ? F : nullptr);
}

// the stochastic midpoint step of every replica (checks done by the caller).  prescribed == NULL: rbl_ensemble_step_brownian;
// otherwise body_in stands where F_body stands, the predictor and the solve are the masked ones and F_out takes the loads
// everything the stochastic step enqueues, from the uploads and the noise to the update: shared as ens_enqueue_det is
int ens_enqueue_bd(rbl_ctx *c, const EnsWork &w, const EnsStepIn &in, uint64_t seed, int split_rand, double delta, int max_iter,
                   double rtol)
{
  const RblBodyState &S = c->S;
  const bool mixed = in.prescribed != nullptr, per_cell = ens_cell_on(c);
  int rc;
  if ((rc = ens_cell_use(c))) return rc;
  if (mixed && !in.resident && (rc = ens_upload_mask(c, w, in.prescribed, in.per))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = S.N_blb, N = Nb * nbl;
  const int64_t n3 = 3 * (int64_t)N;
  if (in.W) { if ((rc = copy_h2d(c, w.W, in.W, sizeof(double) * 3 * (size_t)n3 * R))) return rc; }
  else rbl_launch_normal_batched(c->stream, seed, 3 * n3, R, w.W);            // rand_vector (:730-741), one draw per replica
  const double *FT, *SL;
  if ((rc = ens_begin(c, w, in.F_body, in.slip, &FT, &SL, true, in.resident, in.accepted))) return rc;
  const double *X = ens_X(c, c->ens_cur), *Q = ens_Q(c, c->ens_cur);
  // dense root of every replica: B M B (:667-669), lower Cholesky (:670-671), L W1 and L W2 (:672)
  const RblParams P = rbl_make_params(S.a, S.eta);
  const RblEnsCellRec *cells = per_cell ? ens_cell_table(c) : nullptr;   // a cell per replica: every kernel below reads its replica's
  if (cells) rbl_launch_build_M_cells_batched(c->stream, P, true, w.pos, N, R, w.Lm, n3 * n3, w.rerr, 1, cells);
  else if (per_cell)
    rbl_launch_build_M_per_batched(c->stream, P, true, w.pos, N, R, w.Lm, n3 * n3, w.rerr, 1, c->ens_per_L[0], c->ens_per_L[1],
                                   c->ens_per_n[0], c->ens_per_n[1]);
  else
    rbl_launch_build_M_batched(c->stream, P, S.wall, true, w.pos, N, R, w.Lm, n3 * n3, w.rerr, 0, 1);
  if ((rc = rbl_launch_cholesky_batched(c->stream, w.Lm, n3, R, n3 * n3, in.chol_err ? w.rerr : w.gerr, w.Linv, in.chol_err)))
    return rbl_fail(c, rc, "ensemble: batched Cholesky launch failed");
  const int split = split_rand ? 1 : 0;
  for (int v = 0; v <= split; ++v)
    rbl_launch_block_trmv(c->stream, w.Lm, n3, R, n3 * n3, w.W + v * n3, w.MW + v * n3, 3 * n3);
  // Kinv of the RFD noise and the predictor (:776, :955-959), then M_RFD and the right-hand side (:940-963)
  const double c1 = split_rand ? 2.0 * std::sqrt(S.kBT / S.dt) : std::sqrt(2.0 * S.kBT / S.dt);   // :945-952
  const double c2 = split_rand ? std::sqrt(S.kBT / S.dt) : std::sqrt(2.0 * S.kBT / S.dt);
  const int nbod = R * Nb;
  hipLaunchKernelGGL(k_ens_midpoint, dim3((unsigned)((nbod + ET - 1) / ET)), dim3(ET), 0, c->stream, nbod, Nb, nbl, X, Q, ens_cfg(c),
                     (const double *)w.W, (const double *)w.MW, 0.5 * S.dt * c1, w.dq, w.Xh, w.Qh);
  if (mixed)                                             // the prescribed components: dq = 0, (dt/2) U_p in the predictor displacement
    hipLaunchKernelGGL(k_ens_midpoint_masked, dim3((unsigned)((nbod + ET - 1) / ET)), dim3(ET), 0, c->stream, nbod, Nb, nbl, X, Q, ens_cfg(c),
                       (const unsigned char *)w.mask, in.per, (const double *)w.F, (const double *)w.MW, 0.5 * S.dt * c1, 0.5 * S.dt, w.dq,
                       w.Xh, w.Qh);
  const size_t lds = rfd_lds_bytes(Nb, nbl);
  // the instantiation (the cell's, the wall's, the open one) is chosen once; its last argument is the cell or its empty stand-in
  auto rfd_rhs = [&](auto kern, auto cell) {
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      return rbl_fail(c, RBL_ERR_SIZE, "ensemble: the RFD product does not fit this device's LDS");
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)R), dim3(RBL_SG_THREADS), lds, c->stream, P, Nb, nbl, X, Q, ens_cfg(c),
                       (const double *)w.dq, delta, (const double *)w.W, (const double *)w.MW, (const double *)w.Lm,
                       SL, (const double *)w.F, FT, S.kBT, c2, split, w.rhs, w.rerr, cell);
    return (int)RBL_OK;
  };
  if ((rc = cells    ? rfd_rhs(k_ens_rfd_rhs<true, true, true>, cells)
            : per_cell ? rfd_rhs(k_ens_rfd_rhs<true, true>, ens_cell(c))
            : S.wall ? rfd_rhs(k_ens_rfd_rhs<true>, EnsNoCell{})
                     : rfd_rhs(k_ens_rfd_rhs<false>, EnsNoCell{})))
    return rc;
  // saddle solve at q^{n+1/2}, update from q^n
  return ens_solve_evolve(c, w, w.Xh, w.Qh, max_iter, rtol, mixed, true, !in.resident, in.per, nullptr, in.obs);
}

static int ens_step_bd(rbl_ctx *c, const uint8_t *prescribed, const double *F_body, const double *slip, const double *W, uint64_t seed,
                int split_rand, double delta, int max_iter, double rtol, double *F_out, int *iters, double *resid, int per = 1)
{
  const bool mixed = prescribed != nullptr;
  int rc;
  EnsWork w;
  if ((rc = ens_work(c, max_iter, &w))) return rc;
  EnsStepIn in;
  in.prescribed = prescribed; in.per = per; in.F_body = F_body; in.slip = slip; in.W = W;
  if ((rc = ens_enqueue_bd(c, w, in, seed, split_rand, delta, max_iter, rtol))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb;
  std::vector<double> Ft;
  if (mixed && !F_out) { Ft.resize((size_t)R * 6 * Nb); F_out = Ft.data(); }   // the masked read-back is chosen by F
  return ens_finish(c, w, R, iters, resid, true, nullptr, mixed ? F_out : nullptr);
}

// ---- the entry points with a mask: one worker per operation, per decided by the exported function (1: whole bodies, who's plain
// name; 6: velocity components, the _dof name) -------------------------------------------------------------------------------------------

static int ens_mx_solve(rbl_ctx *c, const char *who, int per, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter,
                 double rtol, double *lambda, double *U, double *F, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, who);
  const std::string no_out = std::string(who) + ": U or F is NULL";
  if (per == 6 && (!U || !F)) return rbl_fail(c, RBL_ERR_ARG, no_out);   // the _dof call refuses NULL outputs before it reads the mask,
  int rc = ens_mx_check(c, who, prescribed, body_in, max_iter, rtol, per); if (rc) return rc;
  if (!U || !F) return rbl_fail(c, RBL_ERR_ARG, no_out);                 // the whole-body call after: a caller sees the first refusal
  if ((rc = ens_ready(c))) return rc;
  return ens_step_det(c, prescribed, body_in, slip, max_iter, rtol, false, lambda, U, F, iters, resid, per);
}

static int ens_mx_step(rbl_ctx *c, const char *who, int per, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter,
                double rtol, double *F, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, who);
  int rc = ens_mx_check(c, who, prescribed, body_in, max_iter, rtol, per); if (rc) return rc;
  if ((rc = ens_flow_check(c))) return rc;
  if ((rc = ens_ready(c))) return rc;
  return ens_step_det(c, prescribed, body_in, slip, max_iter, rtol, true, nullptr, nullptr, F, iters, resid, per);
}

// the Brownian step: the deterministic one's checks and launch sequence plus the predictor's masked kernel.  A mask per velocity
// component must be in include/rbl.h section 7's admissible class, per replica
static int ens_mx_step_bd(rbl_ctx *c, const char *who, int per, const uint8_t *prescribed, const double *body_in, const double *slip,
                   const double *W, uint64_t seed, int split_rand, double delta, int max_iter, double rtol, double *F, int *iters,
                   double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, who);
  int rc = ens_mx_check(c, who, prescribed, body_in, max_iter, rtol, per); if (rc) return rc;
  if (per == 6 && (rc = rbl_bd_mask6_check(c, who, prescribed, c->ens_R, c->ens_Nb))) return rc;   // whole bodies: nothing to check
  if ((rc = ens_flow_check(c))) return rc;
  const RblBodyState &S = c->S;
  const bool brownian = S.kBT > 1e-10;                 // no Brownian terms: the deterministic mixed step (as rbl_step_brownian_mixed)
  if (brownian && (!(S.dt > 0.0) || !(delta > 0.0))) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": dt and delta must be positive");
  if ((rc = ens_ready(c))) return rc;
  if (!brownian) return ens_step_det(c, prescribed, body_in, slip, max_iter, rtol, true, nullptr, nullptr, F, iters, resid, per);
  return ens_step_bd(c, prescribed, body_in, slip, W, seed, split_rand, delta, max_iter, rtol, F, iters, resid, per);
}

// ---- hard joints (include/rbl.h sections 5 and 9): the jointed solve and step of every replica --------------------------------
// The joint set is the context's (rbl_set_joints / rbl_set_joint_kinds), shared by the replicas; the motor angles and rates are
// the replica's own and live here.  One launch of k_gmres_small_jt (rbl_small_joints.hip) solves every replica's jointed system.

// angles and rates of the stored set for the ensemble's R replicas of N_bod bodies: zeros, and the device table stale, when the
// set, R or N_bod changed since they were made
static void ens_jt_sync(rbl_ctx *c)
{
  const size_t n = (size_t)c->ens_R * (size_t)c->jt_n;
  if (c->ens_jt_gen == c->jt_gen && c->ens_jt_R == c->ens_R && c->ens_jt_Nb == c->ens_Nb && c->ens_jt_theta.size() == n) return;
  c->ens_jt_theta.assign(n, 0.0);
  c->ens_jt_rate.assign(n, 0.0);
  c->ens_jt_gen = c->jt_gen; c->ens_jt_R = c->ens_R; c->ens_jt_Nb = c->ens_Nb;   // (the device table's layout holds N_bod + 1 row starts)
  c->ens_jt_valid = false; c->ens_jt_phi_valid = false;
}

// what every jointed ensemble call asks before it touches a device (the style of ens_mx_check)
int ens_jt_check(rbl_ctx *c, const char *who, const double *F_body, int max_iter, double rtol)
{
  const std::string w(who);
  if (!F_body) return rbl_fail(c, RBL_ERR_ARG, w + ": F_body is NULL");
  if (max_iter < 1 || max_iter > 255) return rbl_fail(c, RBL_ERR_ARG, w + ": max_iter must lie in 1 .. 255 (no restart)");
  if (!(rtol >= 0.0)) return rbl_fail(c, RBL_ERR_ARG, w + ": rtol must be >= 0");
  int rc = need_params(c); if (rc) return rc;
  if ((rc = ens_state_check(c, w + ": "))) return rc;
  const bool on = ens_jt_active(c);
  if (on && c->jt_top >= c->ens_Nb)
    for (int j = 0; j < c->jt_n; ++j) {
      const int m = std::max(c->jt_body[2 * (size_t)j], c->jt_body[2 * (size_t)j + 1]);
      if (m >= c->ens_Nb)
        return rbl_fail(c, RBL_ERR_STATE, w + ": joint " + std::to_string(j) + " names body " + std::to_string(m) + ", a replica has " +
                                              std::to_string(c->ens_Nb) + " bodies (indices are local to a replica)");
    }
  if (!rbl_gmres_small_jt_fits(c->S.N_blb, c->ens_Nb, max_iter, on ? c->jt_n : 0))
    return rbl_fail(c, RBL_ERR_SIZE,
                    rbl_gmres_small_fits(c->S.N_blb, c->ens_Nb, max_iter, false)
                        ? w + ": this shape fits the one-kernel solver without joints, but not with the LDS of " + std::to_string(c->jt_n) +
                              " joints (" + std::to_string(rbl_gmres_small_jt_lds_bytes(c->S.N_blb, c->ens_Nb, max_iter, c->jt_n)) + " of 153600 bytes)"
                        : ens_beyond(w + ": "));
  return RBL_OK;
}

// the joint table on the device (RblEnsJoints): once per set, and again after every change of an angle or a rate
int ens_jt_upload(rbl_ctx *c, RblEnsJoints *T)
{
  ens_jt_sync(c);
  const int nj = c->jt_n, nb = c->ens_Nb;
  const size_t ne = c->jt_ends.size() / 2, Rn = (size_t)c->ens_R * nj;
  const size_t ndbl = 13 * (size_t)nj + 2 * Rn, nint = 5 * (size_t)nj + (size_t)nb + 1 + 2 * ne;
  int rc = rbl_dev_reserve(c, c->d_ens_jt, sizeof(double) * ndbl + sizeof(int) * nint); if (rc) return rc;
  double *d = (double *)c->d_ens_jt.p;
  int *di = (int *)(d + ndbl);
  T->anchor = d; T->ang = d + 6 * (size_t)nj; T->theta = d + 13 * (size_t)nj; T->rate = T->theta + Rn;
  T->body = di; T->mate = di + 2 * (size_t)nj; T->kind = di + 4 * (size_t)nj; T->ptr = di + 5 * (size_t)nj; T->ends = T->ptr + nb + 1;
  T->n = nj; T->n_ends = (int)ne;
  if (c->ens_jt_valid) return RBL_OK;
  std::vector<double> hd(ndbl);
  std::copy(c->jt_anchor.begin(), c->jt_anchor.end(), hd.begin());
  std::copy(c->jt_ang.begin(), c->jt_ang.end(), hd.begin() + 6 * (size_t)nj);
  std::copy(c->ens_jt_theta.begin(), c->ens_jt_theta.end(), hd.begin() + 13 * (size_t)nj);
  std::copy(c->ens_jt_rate.begin(), c->ens_jt_rate.end(), hd.begin() + 13 * (size_t)nj + Rn);
  std::vector<int> hi(nint);
  std::copy(c->jt_body.begin(), c->jt_body.end(), hi.begin());
  std::copy(c->jt_mate.begin(), c->jt_mate.end(), hi.begin() + 2 * (size_t)nj);
  std::copy(c->jt_kind.begin(), c->jt_kind.end(), hi.begin() + 4 * (size_t)nj);
  int *ptr = hi.data() + 5 * (size_t)nj;                // the CSR of joint ends with a row for EVERY body of a replica
  {                                                     // (jt_rows is in increasing body order: a body without a joint gets an empty row)
    std::vector<char> has((size_t)nb, 0);
    for (size_t i = 0; i < c->jt_rows.size(); ++i) { has[c->jt_rows[i]] = 1; ptr[c->jt_rows[i]] = c->jt_ptr[i]; }
    int next = (int)ne;
    ptr[nb] = next;
    for (int b = nb - 1; b >= 0; --b) {
      if (has[b]) next = ptr[b];
      else ptr[b] = next;
    }
  }
  std::copy(c->jt_ends.begin(), c->jt_ends.end(), hi.begin() + 5 * (size_t)nj + nb + 1);
  if ((rc = copy_h2d(c, d, hd.data(), sizeof(double) * ndbl))) return rc;
  if ((rc = copy_h2d(c, di, hi.data(), sizeof(int) * nint))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  c->ens_jt_valid = true;
  return RBL_OK;
}

// the jointed solve of every replica at the current configuration; move: a time step -- the force model's loads and the flow
// model's slip at q^n (ens_begin), c formed in the kernel from the gaps (coef = -gamma / dt), k_ens_evolve, and on success the
// commit and the motors' angles.  What it enqueues is ens_enqueue_det's sequence with the jointed variant (EnsJtStep)
static int ens_jt_solve(rbl_ctx *c, const char *who, const double *F_body, const double *slip, const double *jr, bool move, double coef, int max_iter,
                 double rtol, double *lambda, double *U, double *phi, int *iters, double *resid)
{
  const size_t nj3 = (size_t)3 * c->jt_n, Rz = (size_t)c->ens_R;
  c->ens_jt_phi_valid = false;
  EnsWork w;
  int rc;
  if ((rc = ens_work(c, max_iter, &w))) return rc;
  EnsJtStep jt = {who, {}, coef, jr != nullptr};
  if ((rc = ens_jt_upload(c, &jt.T))) return rc;
  if (jr && (rc = copy_h2d(c, w.jr, jr, sizeof(double) * Rz * nj3))) return rc;
  EnsStepIn in;
  in.F_body = F_body; in.slip = slip;
  if ((rc = ens_enqueue_det(c, w, in, max_iter, rtol, move, &jt))) return rc;
  // a redundant joint set: RBL_FLAG_REDUNDANT in the replica's word, which ens_finish turns into RBL_ERR_NOT_SPD with the replica named
  c->ens_jt_phi.resize(Rz * nj3);
  if ((rc = ens_finish_x(c, w, nj3, iters, resid, move, lambda, U, c->ens_jt_phi.data()))) return rc;
  if (phi) std::memcpy(phi, c->ens_jt_phi.data(), sizeof(double) * Rz * nj3);
  c->ens_jt_phi_valid = true;
  if (move) {                                            // the step committed: theta_j += rate_j dt, product and sum rounded one after the other
    bool moved = false;
    for (size_t i = 0; i < c->ens_jt_rate.size(); ++i)
      if (c->ens_jt_rate[i] != 0.0) {
        volatile double d = c->ens_jt_rate[i] * c->S.dt;
        c->ens_jt_theta[i] += d;
        moved = true;
      }
    if (moved) c->ens_jt_valid = false;
  }
  return RBL_OK;
}

// [sets n_joints] values, sets = 1 (every replica alike) or R, into the ensemble's [R n_joints]
static int ens_jt_set_values(rbl_ctx *c, const char *who, const double *v, int sets, bool rates)
{
  if (!c) return RBL_ERR_ARG;
  const std::string w(who);
  if (!c->ens_R) return ens_fail_state(c, w + ": ");
  if (c->jt_n < 1) return rbl_fail(c, RBL_ERR_STATE, w + ": no joints have been set (rbl_set_joint_kinds)");
  if (!v) return rbl_fail(c, RBL_ERR_ARG, w + ": the array is NULL");
  if (sets != 1 && sets != c->ens_R) return rbl_fail(c, RBL_ERR_ARG, w + ": sets must be 1 or R = " + std::to_string(c->ens_R));
  for (int s = 0; s < sets; ++s)
    for (int j = 0; j < c->jt_n; ++j) {
      const double x = v[(size_t)s * c->jt_n + j];
      const std::string at = w + ": set " + std::to_string(s) + ", joint " + std::to_string(j) + ": ";
      if (!std::isfinite(x)) return rbl_fail(c, RBL_ERR_ARG, at + "the value must be finite");
      if (rates && x != 0.0 && c->jt_kind[j] != RBL_JOINT_LOCK)
        return rbl_fail(c, RBL_ERR_ARG, at + "only a lock joint (RBL_JOINT_LOCK) takes a rate; it must be 0 here");
    }
  ens_jt_sync(c);
  std::vector<double> &dst = rates ? c->ens_jt_rate : c->ens_jt_theta;
  for (int r = 0; r < c->ens_R; ++r)
    std::copy(v + (size_t)(sets == 1 ? 0 : r) * c->jt_n, v + (size_t)(sets == 1 ? 0 : r) * c->jt_n + c->jt_n, dst.begin() + (size_t)r * c->jt_n);
  c->ens_jt_valid = false;
  return RBL_OK;
}


// ---- C ABI (include/rbl.h section 5) --------------------------------------------------------------------------------

int rbl_ensemble_set_config(rbl_ctx *c, int R, int N_bod, const double *X, const double *Q)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_set_config");
  int rc = need_params(c); if (rc) return rc;
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, "ensemble: not on a context with a communicator (run one ensemble per process)");
  if (R < 1 || R > ENS_R_MAX) return rbl_fail(c, RBL_ERR_SIZE, "ensemble: R must be 1 .. 65535");
  if (!rbl_gmres_small_fits(c->S.N_blb, N_bod, 1, false))
    return rbl_fail(c, RBL_ERR_SIZE, "ensemble: the system is beyond the one-kernel solver (N_bod * N_blb <= 256, N_bod <= 64 and its vectors within 150 KB of LDS: about 75 N_blobs + 60 N_bod doubles)");
  if (!X || !Q) return rbl_fail(c, RBL_ERR_ARG, "ensemble_set_config: null argument");
  // a shared cell holds for any R; a table of cells belongs to the R it was given for
  if (ens_cells_stored(c) && (size_t)R != c->ens_cells_L.size() / 2)
    return rbl_fail(c, RBL_ERR_STATE, "ensemble_set_config: R = " + std::to_string(R) + ", and cells are stored for " +
                                          std::to_string(c->ens_cells_L.size() / 2) + " replicas, which cannot be mapped to another R: call "
                                          "rbl_ensemble_set_cells or rbl_ensemble_set_periodic first");
  {                                                // K^T K of the structure (rotation invariant) must be invertible (:312-316)
    RblBodyState T = c->S;
    T.N_bod = 1; T.X.assign(3, 0.0); T.Q = {1.0, 0.0, 0.0, 0.0};
    if ((rc = rbl_body_set_K(T, c->last_error))) return rc;
  }
  if ((rc = rbl_dev_init(c))) return rc;
  const size_t nx = (size_t)3 * R * N_bod, nq = (size_t)4 * R * N_bod;
  std::vector<double> Qn(nq);
  for (size_t j = 0; j < nq / 4; ++j) {               // scalar-first, normalised, as rbl_set_config (:212-216)
    const double w = Q[4 * j], x = Q[4 * j + 1], y = Q[4 * j + 2], z = Q[4 * j + 3];
    const double nrm = std::sqrt(w * w + x * x + y * y + z * z);
    Qn[4 * j] = w / nrm; Qn[4 * j + 1] = x / nrm; Qn[4 * j + 2] = y / nrm; Qn[4 * j + 3] = z / nrm;
  }
  // two configuration sets (committed, written by a step) and the reference configuration
  if ((rc = rbl_dev_reserve(c, c->d_ens, sizeof(double) * (2 * (nx + nq) + 3 * (size_t)c->S.N_blb)))) return rc;
  c->ens_R = R; c->ens_Nb = N_bod; c->ens_Nblb = c->S.N_blb; c->ens_cur = 0;
  c->ens_jt_valid = false; c->ens_jt_phi_valid = false;  // a joint table on the device, and the last phi, belonged to the ensemble before
  c->ens_cfg_host.clear();
  if ((rc = copy_h2d(c, ens_X(c, 0), X, sizeof(double) * nx))) { c->ens_R = 0; return rc; }
  if ((rc = copy_h2d(c, ens_Q(c, 0), Qn.data(), sizeof(double) * nq))) { c->ens_R = 0; return rc; }
  if ((rc = ens_ready(c))) { c->ens_R = 0; return rc; }
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

int rbl_ensemble_get_config(rbl_ctx *c, double *X, double *Q)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_get_config");
  if (!c->ens_R) return ens_fail_state(c);
  if (!X || !Q) return rbl_fail(c, RBL_ERR_ARG, "ensemble_get_config: null argument");
  const size_t nb = (size_t)c->ens_R * c->ens_Nb;
  int rc = copy_d2h(c, X, ens_X(c, c->ens_cur), sizeof(double) * 3 * nb); if (rc) return rc;
  if ((rc = copy_d2h(c, Q, ens_Q(c, c->ens_cur), sizeof(double) * 4 * nb))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

int rbl_ensemble_info(const rbl_ctx *c, int *R, int *N_bod)
{
  if (!c) return RBL_ERR_ARG;
  if (R) *R = c->ens_R;
  if (N_bod) *N_bod = c->ens_Nb;
  return c->ens_R ? RBL_OK : RBL_ERR_STATE;
}

int rbl_ensemble_config_dev(rbl_ctx *c, const double **d_X, const double **d_Q)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_config_dev");
  if (!c->ens_R) return ens_fail_state(c);
  if (d_X) *d_X = ens_X(c, c->ens_cur);
  if (d_Q) *d_Q = ens_Q(c, c->ens_cur);
  return RBL_OK;
}

int rbl_ensemble_step_deterministic(rbl_ctx *c, const double *F_body, const double *slip, int max_iter, double rtol, int *iters,
                                    double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_step_deterministic");
  int rc = ens_flow_check(c); if (rc) return rc;
  if ((rc = ens_ready(c))) return rc;
  if (!F_body) return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_deterministic: F_body is NULL");
  if ((rc = ens_check_solver(c, max_iter))) return rc;
  return ens_step_det(c, nullptr, F_body, slip, max_iter, rtol, true, nullptr, nullptr, nullptr, iters, resid);
}

int rbl_ensemble_step_brownian(rbl_ctx *c, const double *F_body, const double *slip, const double *W, uint64_t seed,
                               int split_rand, double delta, int max_iter, double rtol, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_step_brownian");
  int rc = ens_flow_check(c); if (rc) return rc;
  if ((rc = ens_ready(c))) return rc;
  const RblBodyState &S = c->S;
  if (!(S.kBT > 1e-10))                                // no Brownian terms (:967-970): the deterministic midpoint
    return rbl_ensemble_step_deterministic(c, F_body, slip, max_iter, rtol, iters, resid);
  if (!F_body) return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_brownian: F_body is NULL");
  if (!(S.dt > 0.0) || !(delta > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_brownian: dt and delta must be positive");
  if ((rc = ens_check_solver(c, max_iter))) return rc;
  return ens_step_bd(c, nullptr, F_body, slip, W, seed, split_rand, delta, max_iter, rtol, nullptr, iters, resid);
}

// the masked entry points: a mask entry per body, or (the _dof forms; include/rbl.h section 7's _dof semantics, per replica) one per
// velocity component -- the same worker, the same enqueue sequence, the same kernels, told how many entries a body has
int rbl_ensemble_solve_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
                             double *lambda, double *U, double *F, int *iters, double *resid)
{
  return ens_mx_solve(c, "ensemble_solve_mixed", 1, prescribed, body_in, slip, max_iter, rtol, lambda, U, F, iters, resid);
}

int rbl_ensemble_solve_mixed_dof(rbl_ctx *c, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter,
                                 double rtol, double *lambda, double *U, double *F, int *iters, double *resid)
{
  return ens_mx_solve(c, "ensemble_solve_mixed_dof", 6, prescribed6, body_in, slip, max_iter, rtol, lambda, U, F, iters, resid);
}

int rbl_ensemble_step_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
                            double *F, int *iters, double *resid)
{
  return ens_mx_step(c, "ensemble_step_mixed", 1, prescribed, body_in, slip, max_iter, rtol, F, iters, resid);
}

int rbl_ensemble_step_mixed_dof(rbl_ctx *c, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter,
                                double rtol, double *F, int *iters, double *resid)
{
  return ens_mx_step(c, "ensemble_step_mixed_dof", 6, prescribed6, body_in, slip, max_iter, rtol, F, iters, resid);
}

int rbl_ensemble_step_brownian_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, const double *W,
                                     uint64_t seed, int split_rand, double delta, int max_iter, double rtol, double *F, int *iters,
                                     double *resid)
{
  return ens_mx_step_bd(c, "ensemble_step_brownian_mixed", 1, prescribed, body_in, slip, W, seed, split_rand, delta, max_iter, rtol, F,
                        iters, resid);
}

int rbl_ensemble_step_brownian_mixed_dof(rbl_ctx *c, const uint8_t *prescribed6, const double *body_in, const double *slip, const double *W,
                                         uint64_t seed, int split_rand, double delta, int max_iter, double rtol, double *F, int *iters,
                                         double *resid)
{
  return ens_mx_step_bd(c, "ensemble_step_brownian_mixed_dof", 6, prescribed6, body_in, slip, W, seed, split_rand, delta, max_iter, rtol, F,
                        iters, resid);
}

// ---- what rbl_ens_field.hip reads of the ensemble (rbl_api_internal.hpp) --------------------------------------------
int ens_view(rbl_ctx *c, RblEnsView *v)
{
  int rc = ens_ready(c); if (rc) return rc;
  v->cell = ens_cell_on(c);
  if ((rc = ens_cell_use(c))) return rc;
  v->C = ens_cell(c);
  v->cells = ens_cell_table(c);
  v->X = ens_X(c, c->ens_cur); v->Q = ens_Q(c, c->ens_cur); v->cfg = ens_cfg(c);
  v->R = c->ens_R; v->Nb = c->ens_Nb; v->nbl = c->S.N_blb;
  return RBL_OK;
}

int rbl_ensemble_interaction_forces(rbl_ctx *c, double *FT_body, double *energy)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_interaction_forces");
  int rc = ens_ready(c); if (rc) return rc;
  if (!ia_any(c)) return rbl_fail(c, RBL_ERR_STATE, "ensemble_interaction_forces: no force model is switched on (rbl_set_interactions)");
  EnsWork w;
  if ((rc = ens_work(c, 1, &w))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  const size_t N = (size_t)Nb * nbl, nb6 = (size_t)6 * Nb;
  RBL_HIP(c, hipMemsetAsync(w.resid, 0, w.rb_bytes, c->stream));
  const double *X = ens_X(c, c->ens_cur), *Q = ens_Q(c, c->ens_cur);
  rbl_launch_body_geom(c->stream, X, Q, ens_cfg(c), nbl, (int64_t)R * N, w.lever, w.pos);
  double *f = nullptr;
  if ((rc = ia_eval_batch(c, X, Q, w.pos, w.lever, Nb, R, w.ia, &f, w.FT, w.e, w.gerr))) return rc;
  std::vector<double> FT(nb6 * R), e(N * R);
  if ((rc = copy_d2h(c, FT.data(), w.FT, sizeof(double) * FT.size()))) return rc;
  if ((rc = copy_d2h(c, e.data(), w.e, sizeof(double) * e.size()))) return rc;
  if ((rc = ens_finish(c, w, R, nullptr, nullptr, false))) return rc;
  if (FT_body)
    for (size_t i = 0; i < FT.size(); ++i) FT_body[i] = -FT[i];             // reference convention: -K^T f_phys
  if (energy)
    for (int r = 0; r < R; ++r) {                                            // one order: blob index, as rbl_interaction_forces_dev
      double E = 0.0;
      for (size_t i = 0; i < N; ++i) E += e[(size_t)r * N + i];
      energy[r] = E;
    }
  return RBL_OK;
}

// the flow model's term at every replica's configuration (include/rbl.h section 8): R n3 doubles, zeros with both parts off
int rbl_ensemble_flow_slip(rbl_ctx *c, double *out)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_flow_slip");
  int rc = ens_flow_check(c); if (rc) return rc;
  if ((rc = ens_ready(c))) return rc;
  if (!out) return rbl_fail(c, RBL_ERR_ARG, "ensemble_flow_slip: out is NULL");
  EnsWork w;
  if ((rc = ens_work(c, 1, &w))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  const size_t vb = sizeof(double) * 3 * (size_t)R * Nb * nbl;
  const double *X = ens_X(c, c->ens_cur), *Q = ens_Q(c, c->ens_cur);
  rbl_launch_body_geom(c->stream, X, Q, ens_cfg(c), nbl, (int64_t)R * Nb * nbl, w.lever, w.pos);
  bool have = false;
  if ((rc = flow_add_batch(c, w.pos, Q, Nb, R, w.slip, &have))) return rc;
  if (!have) RBL_HIP(c, hipMemsetAsync(w.slip, 0, vb, c->stream));
  if ((rc = copy_d2h(c, out, w.slip, vb))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

// ---- hard joints of an ensemble (include/rbl.h section 5; the joint set is section 9's, rbl_set_joints / rbl_set_joint_kinds) ----

int rbl_ensemble_set_joint_rates(rbl_ctx *c, const double *rate, int sets)
{
  return ens_jt_set_values(c, "ensemble_set_joint_rates", rate, sets, true);
}

int rbl_ensemble_set_joint_angles(rbl_ctx *c, const double *theta, int sets)
{
  return ens_jt_set_values(c, "ensemble_set_joint_angles", theta, sets, false);
}

int rbl_ensemble_solve_jointed(rbl_ctx *c, const double *F_body, const double *slip, const double *joint_rhs, int max_iter, double rtol,
                               double *lambda, double *U, double *phi, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_solve_jointed");
  if (ens_cell_on(c)) return ens_cell_refuse(c, "ensemble_solve_jointed");
  int rc = ens_jt_check(c, "ensemble_solve_jointed", F_body, max_iter, rtol); if (rc) return rc;
  if ((rc = ens_ready(c))) return rc;
  if (!ens_jt_active(c))                               // switched off or never set: the unjointed solve on [slip ; -F]
    return ens_step_det(c, nullptr, F_body, slip, max_iter, rtol, false, lambda, U, nullptr, iters, resid);
  return ens_jt_solve(c, "ensemble_solve_jointed", F_body, slip, joint_rhs, false, 0.0, max_iter, rtol, lambda, U, phi, iters, resid);
}

int rbl_ensemble_step_jointed(rbl_ctx *c, const double *F_body, const double *slip, const double *joint_velocity, double gamma, int max_iter,
                              double rtol, double *phi, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_step_jointed");
  if (ens_cell_on(c)) return ens_cell_refuse(c, "ensemble_step_jointed");
  if (!F_body) return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_jointed: F_body is NULL");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_jointed: gamma must lie in [0, 1]");
  if (ens_jt_active(c) && !(c->S.dt > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_jointed: dt must be positive");
  int rc = ens_jt_check(c, "ensemble_step_jointed", F_body, max_iter, rtol); if (rc) return rc;
  if (!ens_jt_active(c)) return rbl_ensemble_step_deterministic(c, F_body, slip, max_iter, rtol, iters, resid);
  if ((rc = ens_flow_check(c))) return rc;
  if ((rc = ens_ready(c))) return rc;
  return ens_jt_solve(c, "ensemble_step_jointed", F_body, slip, joint_velocity, true, -gamma / c->S.dt, max_iter, rtol, nullptr, nullptr, phi,
                      iters, resid);
}

// gaps [R 3 n_joints] of the stored joints (on or off) at every replica's configuration -- an angular joint's rows hold e, or P e --,
// phi [R 3 n_joints] of the last jointed ensemble solve or step with this set, theta [R n_joints]; any may be NULL
int rbl_ensemble_joint_state(rbl_ctx *c, double *gap, double *phi, double *theta)
{
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "ensemble_joint_state");
  if (ens_cell_on(c)) return ens_cell_refuse(c, "ensemble_joint_state");
  if (!c->ens_R) return ens_fail_state(c);
  if (c->jt_n < 1) return rbl_fail(c, RBL_ERR_STATE, "ensemble_joint_state: no joints have been set (rbl_set_joint_kinds)");
  if (c->jt_top >= c->ens_Nb) return rbl_fail(c, RBL_ERR_STATE, "ensemble_joint_state: a joint names a body beyond the replica's " + std::to_string(c->ens_Nb));
  ens_jt_sync(c);
  if (phi && !c->ens_jt_phi_valid)
    return rbl_fail(c, RBL_ERR_STATE, "ensemble_joint_state: no jointed ensemble solve or step has succeeded with this joint set");
  const size_t Rn = (size_t)c->ens_R * c->jt_n;
  if (gap) {
    int rc = ens_ready(c); if (rc) return rc;
    RblEnsJoints T;
    if ((rc = ens_jt_upload(c, &T))) return rc;
    // the stored set, on or off: the gaps go where a jointed step's joint rows go, the lever arms (6 per joint) into the solver's
    // workspace, which holds more than two vectors of 3 N + 6 N_bod + 3 n_joints per replica
    EnsWork w;
    if ((rc = ens_work(c, 1, &w, c->jt_n))) return rc;
    double *d_lev = w.gm, *d_gap = w.jr;
    rbl_launch_ens_jt_geom(c->stream, ens_X(c, c->ens_cur), ens_Q(c, c->ens_cur), c->ens_Nb, c->ens_R, T, d_lev, d_gap);
    if ((rc = copy_d2h(c, gap, d_gap, sizeof(double) * 3 * Rn))) return rc;
    RBL_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (phi) std::memcpy(phi, c->ens_jt_phi.data(), sizeof(double) * 3 * Rn);
  if (theta) std::memcpy(theta, c->ens_jt_theta.data(), sizeof(double) * Rn);
  return RBL_OK;
}

// does a jointed ensemble of this shape fit the one-kernel solver?  1 or 0; *lds_bytes (may be NULL): what its vectors and joint
// data take of the solver's 153600 bytes (without the Krylov basis, which goes to global memory when it does not fit beside them).
// No context: a caller asks before it builds anything
int rbl_ensemble_joints_fit(int N_blb, int N_bod, int max_iter, int n_joints, int64_t *lds_bytes)
{
  if (lds_bytes) *lds_bytes = N_blb > 0 && N_bod > 0 && max_iter > 0 && n_joints >= 0 ? (int64_t)rbl_gmres_small_jt_lds_bytes(N_blb, N_bod, max_iter, n_joints) : 0;
  return rbl_gmres_small_jt_fits(N_blb, N_bod, max_iter, n_joints) ? 1 : 0;
}
