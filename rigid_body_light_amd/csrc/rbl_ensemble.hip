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
// With prescribed bodies (rbl_ensemble_solve_mixed / _step_mixed / _step_brownian_mixed; the semantics of include/rbl.h section 7
// per replica, the restatement of rbl_mixed.hip's mx_solve / mx_step and of rbl_steps.hip's rhs_and_midpoint_core): a 0/1 mask per
// body and replica travels with the call, and NULL for it is the unmasked step: ens_step_det and ens_step_bd serve both.
// The same launches with three differences: k_ens_midpoint is followed by k_ens_midpoint_prescribed (dq = 0 and the predictor
// (dt/2) U_p on a prescribed body; one more launch, so that a free body goes through the very same code), the solve is the
// masked k_gmres_small (it adds K_p U_p to the right-hand side with the lever arms of the configuration it solves at, zeroes
// the prescribed bodies' balance rows and splits the solution into U and F per body), and
// k_ens_evolve reads the U the solver wrote.  The right-hand-side kernels are the unmasked ones: body_in stands where F_body stood,
// so the model's K^T f reaches the bottom rows of the free bodies and what they write on a prescribed body's rows is overwritten
// by the solver.  U and F follow the error words in the ONE read-back.  A free body's arithmetic and its order are unchanged: with
// nobody prescribed the configurations and iteration counts are bitwise those of the unmasked steps.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_small_dev.hpp"

namespace {

constexpr int ET = 256;          // threads of the per-body / per-entry kernels
constexpr int EW = RBL_SG_THREADS / 64;
constexpr int ENS_R_MAX = 65535;

// update_X_Q of one body, c_rigid_obj.cpp:679-710 (the device restatement of rbl_body_update_X_Q): U displacement units
__device__ __forceinline__ void ens_update_body(const double *X, const double *Q, const double *U, double *Xo, double *Qo)
{
  const double *om = U + 3;
  const double nrm = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
  double qw = cos(nrm / 2.0), qx = 0.0, qy = 0.0, qz = 0.0;          // :681-683
  if (nrm > 1.0e-10) {                                                 // :684-686
    const double s = sin(nrm / 2.0) / nrm;
    qx = s * om[0]; qy = s * om[1]; qz = s * om[2];
  }
  double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);             // :687
  qw /= qn; qx /= qn; qy /= qn; qz /= qn;
  const double rw = qw * Q[0] - qx * Q[1] - qy * Q[2] - qz * Q[3];    // Q_rot * Q  (:704)
  const double rx = qw * Q[1] + qx * Q[0] + qy * Q[3] - qz * Q[2];
  const double ry = qw * Q[2] + qy * Q[0] + qz * Q[1] - qx * Q[3];
  const double rz = qw * Q[3] + qz * Q[0] + qx * Q[2] - qy * Q[1];
  qn = sqrt(rw * rw + rx * rx + ry * ry + rz * rz);                   // :705
  Qo[0] = rw / qn; Qo[1] = rx / qn; Qo[2] = ry / qn; Qo[3] = rz / qn;
  for (int c = 0; c < 3; ++c) Xo[c] = X[c] + U[c];                    // :706
}

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

// right-hand side of the deterministic step: [slip (or 0) ; -(F - FT)] per replica (FT: the model's K^T f_phys, or NULL)
__global__ __launch_bounds__(ET) void k_ens_rhs_det(int R, int n3, int nb6, const double *__restrict__ slip,
                                                    const double *__restrict__ F, const double *__restrict__ FT,
                                                    double *__restrict__ rhs)
{
  const long nsys = n3 + nb6, idx = (long)blockIdx.x * ET + threadIdx.x;
  if (idx >= (long)R * nsys) return;
  const long r = idx / nsys, e = idx - r * nsys;
  if (e < n3) { rhs[idx] = slip ? slip[r * n3 + e] : 0.0; return; }
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

// k_ens_midpoint with prescribed bodies (mask[nbod], body_in[6 nbod]) is k_ens_midpoint itself on every body, then this kernel
// on the prescribed ones: such a body takes no random displacement -- dq = 0 -- and sits at q^n + (dt/2) U_p in the predictor
// (k_mx_bd_sums, rbl_body_dev.hip, and the host loop of rhs_and_midpoint_core, rbl_steps.hip).  One kernel with the two cases as branches was tried: the
// compiler joins the branches' common tail (the update), scale * u of a free body then no longer fuses into X + u as it does
// in k_ens_midpoint, and a free body's configuration differs in the last bit from the unmasked step's.  Running the unmasked
// kernel gives the same bits by construction, for one more small launch per step
__global__ __launch_bounds__(ET) void k_ens_midpoint_prescribed(int nbod, const double *__restrict__ X, const double *__restrict__ Q,
                                                                const unsigned char *__restrict__ mask,
                                                                const double *__restrict__ body_in, double half_dt,
                                                                double *__restrict__ dq, double *__restrict__ Xh,
                                                                double *__restrict__ Qh)
{
  const int g = blockIdx.x * ET + threadIdx.x;
  if (g >= nbod || !mask[g]) return;
  double u[6];
  for (int p = 0; p < 6; ++p) { dq[6 * (size_t)g + p] = 0.0; u[p] = half_dt * body_in[6 * (size_t)g + p]; }
  ens_update_body(X + 3 * (size_t)g, Q + 4 * (size_t)g, u, Xh + 3 * (size_t)g, Qh + 4 * (size_t)g);
}

// One workgroup per replica: the random finite difference of the mobility along dq (m_rfd_dir: positions at q +- delta/2 dq,
// B M B W_rfd at each, (1/delta) difference) and the right-hand side of the stochastic step (rbl_RHS_and_Midpoint_dev):
//   top = slip - kBT M_RFD - c2 M^1/2 W1 (+ c2 M^1/2 W2 with split_rand),  bottom = -(F - FT).
// Also checks the replica's dense factor: a diagonal entry that is not positive and finite is RBL_FLAG_NOT_SPD.
template <bool WALL>
__global__ __launch_bounds__(RBL_SG_THREADS) void k_ens_rfd_rhs(RblParams P, int Nb, int nbl, const double *__restrict__ X,
                                                                const double *__restrict__ Q, const double *__restrict__ cfg,
                                                                const double *__restrict__ dq, double delta,
                                                                const double *__restrict__ W, const double *__restrict__ MW,
                                                                const double *__restrict__ Lm, const double *__restrict__ slip,
                                                                const double *__restrict__ F, const double *__restrict__ FT,
                                                                double kBT, double c2, int split, double *__restrict__ rhs,
                                                                unsigned *__restrict__ rerr)
{
  extern __shared__ double sm[];
  const int r = blockIdx.x, t = threadIdx.x;
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
      rbl_pair_accum<WALL, true, true>(Pu, pos[3 * t], pos[3 * t + 1], pos[3 * t + 2], pos[3 * t], pos[3 * t + 1], pos[3 * t + 2],
                                       di * vin[3 * t], di * vin[3 * t + 1], di * vin[3 * t + 2], true, ux, uy, uz, flags);
      su[3 * t] = ux; su[3 * t + 1] = uy; su[3 * t + 2] = uz;
    }
    rbl_small_pair_sweep<WALL>(Pu, pos, dmp, vin, N, part, flags);
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

// a bump allocator over one device buffer (256-byte aligned pieces)
struct Carve {
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
  void *ia;
  // read-back block: residuals | iterations | error word per replica | one error word for the batch
  double *resid; int *iters; unsigned *rerr, *gerr;
  size_t rb_bytes;
  // prescribed bodies: U and F of the masked solve follow the read-back block (rb_mx_bytes reaches their end) and stand in front
  // of x in one piece [U | F | x], as rbl_launch_gmres_small_ens_mixed wants them; body_in is uploaded where F_body goes (F)
  double *U, *Fo; unsigned char *mask;
  size_t rb_mx_bytes;
};

EnsWork ens_carve(void *base, int R, int Nb, int nbl, int max_iter, size_t *bytes)
{
  const size_t N = (size_t)Nb * nbl, n3 = 3 * N, nb6 = 6 * (size_t)Nb, nsys = n3 + nb6, Rz = (size_t)R;
  Carve C{(char *)base};
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
  w.mask = C.take<unsigned char>(Rz * Nb);
  w.gm = C.take<double>(Rz * rbl_gmres_small_work_doubles(nbl, Nb, max_iter));
  w.e = C.take<double>(Rz * N);
  w.ia = C.take<char>(ia_batch_bytes(Nb, nbl, R));
  *bytes = C.off;
  return w;
}

// the flow model's host-side refusals (wall consistency, n_scale) for the ensemble's body count, made by the step entry points
// and the query before ens_ready touches the device; without an ensemble there is nothing to check (ens_ready says so)
int ens_flow_check(rbl_ctx *c) { return c->ens_R ? flow_check(c, c->ens_Nb) : RBL_OK; }

int ens_fail_state(rbl_ctx *c) { return rbl_fail(c, RBL_ERR_STATE, "ensemble: no ensemble configuration (rbl_ensemble_set_config)"); }

double *ens_X(rbl_ctx *c, int which) { return (double *)c->d_ens.p + (size_t)which * 7 * c->ens_R * c->ens_Nb; }
double *ens_Q(rbl_ctx *c, int which) { return ens_X(c, which) + (size_t)3 * c->ens_R * c->ens_Nb; }
double *ens_cfg(rbl_ctx *c) { return ens_X(c, 2); }

// parameters set, ensemble set for the current structure, single GPU; uploads the reference configuration when it changed
int ens_ready(rbl_ctx *c)
{
  int rc = need_params(c); if (rc) return rc;
  if (!c->ens_R) return ens_fail_state(c);
  if (c->S.N_blb != c->ens_Nblb) return rbl_fail(c, RBL_ERR_STATE, "ensemble: the structure changed since rbl_ensemble_set_config");
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, "ensemble: not on a context with a communicator (run one ensemble per process)");
  if ((rc = rbl_dev_init(c))) return rc;
  if (c->ens_cfg_host != c->S.ref_cfg) {
    if ((rc = copy_h2d(c, ens_cfg(c), c->S.ref_cfg.data(), sizeof(double) * c->S.ref_cfg.size()))) return rc;
    c->ens_cfg_host = c->S.ref_cfg;
  }
  return RBL_OK;
}

// the step's flags: the first failing replica names the error; nothing is committed unless every replica succeeded
int ens_finish(rbl_ctx *c, const EnsWork &w, int R, int *iters, double *resid, bool commit, double *U = nullptr, double *F = nullptr)
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

// upload F (R 6 N_bod) and slip (R n3 or NULL), clear the read-back block, evaluate the force model at q^n when it is on and
// the caller wants its loads (model): *FT -> K^T f_phys of every replica (NULL otherwise).  The flow model (include/rbl.h
// section 8) goes the same way: one launch adds its term at q^n to every replica's slip.  *SL -> the slip the right-hand side
// takes: the caller's, the term, their sum, or NULL for zero
int ens_begin(rbl_ctx *c, const EnsWork &w, const double *F_body, const double *slip, const double **FT, const double **SL,
              bool model = true)
{
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  const size_t n3 = (size_t)3 * Nb * nbl, nb6 = (size_t)6 * Nb;
  int rc = copy_h2d(c, w.F, F_body, sizeof(double) * nb6 * R); if (rc) return rc;
  if (slip && (rc = copy_h2d(c, w.slip, slip, sizeof(double) * n3 * R))) return rc;
  RBL_HIP(c, hipMemsetAsync(w.resid, 0, w.rb_bytes, c->stream));
  const double *X = ens_X(c, c->ens_cur), *Q = ens_Q(c, c->ens_cur);
  rbl_launch_body_geom(c->stream, X, Q, ens_cfg(c), nbl, (int64_t)R * Nb * nbl, w.lever, w.pos);
  *FT = nullptr;
  if (model && c->ia_on) {
    double *f = nullptr;
    if ((rc = ia_eval_batch(c, X, w.pos, w.lever, Nb, R, w.ia, &f, w.FT, nullptr, w.gerr))) return rc;
    *FT = w.FT;
  }
  bool have_slip = slip != nullptr;
  if (model && (rc = flow_add_batch(c, w.pos, Q, Nb, R, w.slip, &have_slip))) return rc;
  *SL = have_slip ? w.slip : nullptr;
  return RBL_OK;
}

int ens_work(rbl_ctx *c, int max_iter, EnsWork *w)
{
  size_t bytes = 0;
  ens_carve(nullptr, c->ens_R, c->ens_Nb, c->S.N_blb, max_iter, &bytes);
  int rc = rbl_dev_reserve(c, c->d_ens_w, bytes); if (rc) return rc;
  *w = ens_carve(c->d_ens_w.p, c->ens_R, c->ens_Nb, c->S.N_blb, max_iter, &bytes);
  return RBL_OK;
}

int ens_check_solver(rbl_ctx *c, int max_iter)
{
  if (max_iter < 1) return rbl_fail(c, RBL_ERR_ARG, "ensemble step: max_iter must be >= 1");
  if (!rbl_gmres_small_fits(c->S.N_blb, c->ens_Nb, max_iter, false))
    return rbl_fail(c, RBL_ERR_SIZE, "ensemble step: the system is beyond the one-kernel solver (<= 256 blobs, <= 64 bodies, max_iter <= 255)");
  return RBL_OK;
}

// mixed: the masked solve (w.mask, body_in in w.F); the update then reads the U it wrote (a prescribed body: dt U_p exactly).
// evolve = false: the solve alone
int ens_solve_evolve(rbl_ctx *c, const EnsWork &w, const double *Xs, const double *Qs, int max_iter, double rtol, bool mixed = false,
                     bool evolve = true)
{
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  const long n3 = 3L * Nb * nbl, nsys = n3 + 6L * Nb;
  const RblParams P = rbl_make_params(c->S.a, c->S.eta);
  int rc = mixed ? rbl_launch_gmres_small_ens_mixed(c->stream, P, c->S.wall, Xs, Qs, ens_cfg(c), nbl, Nb, R, w.rhs, w.U, max_iter, rtol,
                                                    w.gm, w.iters, w.resid, w.rerr, w.mask, w.F)
                 : rbl_launch_gmres_small_ens(c->stream, P, c->S.wall, Xs, Qs, ens_cfg(c), nbl, Nb, R, w.rhs, w.x, max_iter, rtol, w.gm,
                                              w.iters, w.resid, w.rerr);
  if (rc) return rbl_fail(c, rc, "ensemble step: the one-kernel solver does not fit this device's LDS");
  if (!evolve) return RBL_OK;
  const int nbod = R * Nb;
  if (c->record_mom) {                                   // RBL_OPT_RECORD_MOMENTS: lambda is the top of every replica's x, the lever
    c->ens_mom_R = 0;                                    // arms those of the configuration solved at; valid once the step committed
    if ((rc = rbl_dev_reserve(c, c->d_ens_mom, sizeof(double) * 9 * (size_t)nbod))) return rc;
    flow_launch_moments(c, nullptr, Qs, ens_cfg(c), w.x, Nb, nbod, nsys, (double *)c->d_ens_mom.p);
  }
  hipLaunchKernelGGL(k_ens_evolve, dim3((unsigned)((nbod + ET - 1) / ET)), dim3(ET), 0, c->stream, nbod, Nb, mixed ? 6L * Nb : nsys,
                     mixed ? 0L : n3, c->S.dt, mixed ? (const double *)w.U : (const double *)w.x, (const double *)ens_X(c, c->ens_cur),
                     (const double *)ens_Q(c, c->ens_cur), ens_X(c, c->ens_cur ^ 1), ens_Q(c, c->ens_cur ^ 1), w.rerr);
  return RBL_OK;
}

// the checks of the entry points with prescribed bodies: none needs a device
int ens_mx_check(rbl_ctx *c, const char *who, const uint8_t *prescribed, const double *body_in, int max_iter, double rtol)
{
  int rc = need_params(c); if (rc) return rc;
  const std::string w(who);
  if (!prescribed || !body_in) return rbl_fail(c, RBL_ERR_ARG, w + ": prescribed or body_in is NULL");
  if (max_iter < 1 || !(rtol >= 0.0)) return rbl_fail(c, RBL_ERR_ARG, w + ": need max_iter >= 1 and rtol >= 0");
  if (max_iter > 255)
    return rbl_fail(c, RBL_ERR_SIZE, "ensemble step: the system is beyond the one-kernel solver (<= 256 blobs, <= 64 bodies, max_iter <= 255)");
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, "ensemble: not on a context with a communicator (run one ensemble per process)");
  if (!c->ens_R) return ens_fail_state(c);
  if (c->S.N_blb != c->ens_Nblb) return rbl_fail(c, RBL_ERR_STATE, "ensemble: the structure changed since rbl_ensemble_set_config");
  const size_t nbod = (size_t)c->ens_R * c->ens_Nb;
  for (size_t g = 0; g < nbod; ++g)
    if (prescribed[g] > 1) return rbl_fail(c, RBL_ERR_ARG, w + ": entries of prescribed must be 0 or 1 (replica " + std::to_string(g / c->ens_Nb) + ")");
  if (!rbl_gmres_small_fits(c->S.N_blb, c->ens_Nb, max_iter, false, true))
    return rbl_fail(c, RBL_ERR_SIZE, rbl_gmres_small_fits(c->S.N_blb, c->ens_Nb, max_iter, false)
                                         ? w + ": this shape fits the one-kernel solver without prescribed bodies, but not with the mask's 6 N_bod doubles of LDS"
                                         : std::string("ensemble step: the system is beyond the one-kernel solver (<= 256 blobs, <= 64 bodies, max_iter <= 255)"));
  return RBL_OK;
}

// the deterministic step of every replica (checks and ens_ready done by the caller).  prescribed == NULL:
// rbl_ensemble_step_deterministic -- the unmasked solver, lambda, U and F NULL; otherwise body_in stands where F_body stands and
// the solve is the masked one.  move = false: the solve alone, at the current configuration and without the model's loads
// (rbl_ensemble_solve_mixed)
int ens_step_det(rbl_ctx *c, const uint8_t *prescribed, const double *F_body, const double *slip, int max_iter, double rtol, bool move,
                 double *lambda, double *U, double *F, int *iters, double *resid)
{
  const bool mixed = prescribed != nullptr;
  EnsWork w;
  const double *FT, *SL;
  int rc;
  if ((rc = ens_work(c, max_iter, &w))) return rc;
  if (mixed && (rc = copy_h2d(c, w.mask, prescribed, (size_t)c->ens_R * c->ens_Nb))) return rc;
  if ((rc = ens_begin(c, w, F_body, slip, &FT, &SL, move))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb;
  const int n3 = 3 * Nb * c->S.N_blb, nb6 = 6 * Nb;
  const long tot = (long)R * (n3 + nb6);
  hipLaunchKernelGGL(k_ens_rhs_det, dim3((unsigned)((tot + ET - 1) / ET)), dim3(ET), 0, c->stream, R, n3, nb6, SL,
                     (const double *)w.F, FT, w.rhs);
  if ((rc = ens_solve_evolve(c, w, ens_X(c, c->ens_cur), ens_Q(c, c->ens_cur), max_iter, rtol, mixed, move))) return rc;
  std::vector<double> x;
  if (lambda) {                                          // the blob forces: the top of every replica's solution
    x.resize((size_t)R * (n3 + nb6));
    if ((rc = copy_d2h(c, x.data(), w.x, sizeof(double) * x.size()))) return rc;
  }
  std::vector<double> Ft;
  if (mixed && !F) { Ft.resize((size_t)R * nb6); F = Ft.data(); }         // the masked read-back is chosen by U or F
  if ((rc = ens_finish(c, w, R, iters, resid, move, mixed ? U : nullptr, mixed ? F : nullptr))) return rc;
  if (lambda)
    for (int r = 0; r < R; ++r) std::memcpy(lambda + (size_t)r * n3, x.data() + (size_t)r * (n3 + nb6), sizeof(double) * n3);
  return RBL_OK;
}

// the stochastic midpoint step of every replica (checks done by the caller).  prescribed == NULL: rbl_ensemble_step_brownian;
// otherwise body_in stands where F_body stands, the predictor and the solve are the masked ones and F_out takes the loads
int ens_step_bd(rbl_ctx *c, const uint8_t *prescribed, const double *F_body, const double *slip, const double *W, uint64_t seed,
                int split_rand, double delta, int max_iter, double rtol, double *F_out, int *iters, double *resid)
{
  const RblBodyState &S = c->S;
  const bool mixed = prescribed != nullptr;
  int rc;
  EnsWork w;
  if ((rc = ens_work(c, max_iter, &w))) return rc;
  if (mixed && (rc = copy_h2d(c, w.mask, prescribed, (size_t)c->ens_R * c->ens_Nb))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = S.N_blb, N = Nb * nbl;
  const int64_t n3 = 3 * (int64_t)N;
  if (W) { if ((rc = copy_h2d(c, w.W, W, sizeof(double) * 3 * (size_t)n3 * R))) return rc; }
  else rbl_launch_normal_batched(c->stream, seed, 3 * n3, R, w.W);            // rand_vector (:730-741), one draw per replica
  const double *FT, *SL;
  if ((rc = ens_begin(c, w, F_body, slip, &FT, &SL))) return rc;
  const double *X = ens_X(c, c->ens_cur), *Q = ens_Q(c, c->ens_cur);
  // dense root of every replica: B M B (:667-669), lower Cholesky (:670-671), L W1 and L W2 (:672)
  const RblParams P = rbl_make_params(S.a, S.eta);
  rbl_launch_build_M_batched(c->stream, P, S.wall, true, w.pos, N, R, w.Lm, n3 * n3, w.rerr, 0, 1);
  if ((rc = rbl_launch_cholesky_batched(c->stream, w.Lm, n3, R, n3 * n3, w.gerr, w.Linv)))
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
  if (mixed)                                             // the prescribed bodies: dq = 0, q^n + (dt/2) U_p
    hipLaunchKernelGGL(k_ens_midpoint_prescribed, dim3((unsigned)((nbod + ET - 1) / ET)), dim3(ET), 0, c->stream, nbod, X, Q,
                       (const unsigned char *)w.mask, (const double *)w.F, 0.5 * S.dt, w.dq, w.Xh, w.Qh);
  const size_t lds = rfd_lds_bytes(Nb, nbl);
  const void *fn = S.wall ? (const void *)k_ens_rfd_rhs<true> : (const void *)k_ens_rfd_rhs<false>;
  if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return rbl_fail(c, RBL_ERR_SIZE, "ensemble: the RFD product does not fit this device's LDS");
  }
  if (S.wall)
    hipLaunchKernelGGL(k_ens_rfd_rhs<true>, dim3((unsigned)R), dim3(RBL_SG_THREADS), lds, c->stream, P, Nb, nbl, X, Q, ens_cfg(c),
                       (const double *)w.dq, delta, (const double *)w.W, (const double *)w.MW, (const double *)w.Lm,
                       SL, (const double *)w.F, FT, S.kBT, c2, split, w.rhs, w.rerr);
  else
    hipLaunchKernelGGL(k_ens_rfd_rhs<false>, dim3((unsigned)R), dim3(RBL_SG_THREADS), lds, c->stream, P, Nb, nbl, X, Q, ens_cfg(c),
                       (const double *)w.dq, delta, (const double *)w.W, (const double *)w.MW, (const double *)w.Lm,
                       SL, (const double *)w.F, FT, S.kBT, c2, split, w.rhs, w.rerr);
  // saddle solve at q^{n+1/2}, update from q^n
  if ((rc = ens_solve_evolve(c, w, w.Xh, w.Qh, max_iter, rtol, mixed))) return rc;
  std::vector<double> Ft;
  if (mixed && !F_out) { Ft.resize((size_t)R * 6 * Nb); F_out = Ft.data(); }   // the masked read-back is chosen by F
  return ens_finish(c, w, R, iters, resid, true, nullptr, mixed ? F_out : nullptr);
}

}  // namespace

// ---- C ABI (include/rbl.h section 5) --------------------------------------------------------------------------------

int rbl_ensemble_set_config(rbl_ctx *c, int R, int N_bod, const double *X, const double *Q)
{
  if (!c) return RBL_ERR_ARG;
  int rc = need_params(c); if (rc) return rc;
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, "ensemble: not on a context with a communicator (run one ensemble per process)");
  if (R < 1 || R > ENS_R_MAX) return rbl_fail(c, RBL_ERR_SIZE, "ensemble: R must be 1 .. 65535");
  if (!rbl_gmres_small_fits(c->S.N_blb, N_bod, 1, false))
    return rbl_fail(c, RBL_ERR_SIZE, "ensemble: N_bod * N_blb must be <= 256 and N_bod <= 64 (the one-kernel solver)");
  if (!X || !Q) return rbl_fail(c, RBL_ERR_ARG, "ensemble_set_config: null argument");
  {                                                    // K^T K of the structure (rotation invariant) must be invertible (:312-316)
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
  if (!c->ens_R) return ens_fail_state(c);
  if (d_X) *d_X = ens_X(c, c->ens_cur);
  if (d_Q) *d_Q = ens_Q(c, c->ens_cur);
  return RBL_OK;
}

int rbl_ensemble_step_deterministic(rbl_ctx *c, const double *F_body, const double *slip, int max_iter, double rtol, int *iters,
                                    double *resid)
{
  if (!c) return RBL_ERR_ARG;
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

int rbl_ensemble_solve_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
                             double *lambda, double *U, double *F, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  int rc = ens_mx_check(c, "ensemble_solve_mixed", prescribed, body_in, max_iter, rtol); if (rc) return rc;
  if (!U || !F) return rbl_fail(c, RBL_ERR_ARG, "ensemble_solve_mixed: U or F is NULL");
  if ((rc = ens_ready(c))) return rc;
  return ens_step_det(c, prescribed, body_in, slip, max_iter, rtol, false, lambda, U, F, iters, resid);
}

int rbl_ensemble_step_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
                            double *F, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  int rc = ens_mx_check(c, "ensemble_step_mixed", prescribed, body_in, max_iter, rtol); if (rc) return rc;
  if ((rc = ens_flow_check(c))) return rc;
  if ((rc = ens_ready(c))) return rc;
  return ens_step_det(c, prescribed, body_in, slip, max_iter, rtol, true, nullptr, nullptr, F, iters, resid);
}

int rbl_ensemble_step_brownian_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, const double *W,
                                     uint64_t seed, int split_rand, double delta, int max_iter, double rtol, double *F, int *iters,
                                     double *resid)
{
  if (!c) return RBL_ERR_ARG;
  int rc = ens_mx_check(c, "ensemble_step_brownian_mixed", prescribed, body_in, max_iter, rtol); if (rc) return rc;
  if ((rc = ens_flow_check(c))) return rc;
  const RblBodyState &S = c->S;
  const bool brownian = S.kBT > 1e-10;                 // no Brownian terms: the deterministic mixed step (as rbl_step_brownian_mixed)
  if (brownian && (!(S.dt > 0.0) || !(delta > 0.0)))
    return rbl_fail(c, RBL_ERR_ARG, "ensemble_step_brownian_mixed: dt and delta must be positive");
  if ((rc = ens_ready(c))) return rc;
  if (!brownian) return ens_step_det(c, prescribed, body_in, slip, max_iter, rtol, true, nullptr, nullptr, F, iters, resid);
  return ens_step_bd(c, prescribed, body_in, slip, W, seed, split_rand, delta, max_iter, rtol, F, iters, resid);
}

int rbl_ensemble_interaction_forces(rbl_ctx *c, double *FT_body, double *energy)
{
  if (!c) return RBL_ERR_ARG;
  int rc = ens_ready(c); if (rc) return rc;
  if (!c->ia_on) return rbl_fail(c, RBL_ERR_STATE, "ensemble_interaction_forces: no force model is switched on (rbl_set_interactions)");
  EnsWork w;
  if ((rc = ens_work(c, 1, &w))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  const size_t N = (size_t)Nb * nbl, nb6 = (size_t)6 * Nb;
  RBL_HIP(c, hipMemsetAsync(w.resid, 0, w.rb_bytes, c->stream));
  const double *X = ens_X(c, c->ens_cur), *Q = ens_Q(c, c->ens_cur);
  rbl_launch_body_geom(c->stream, X, Q, ens_cfg(c), nbl, (int64_t)R * N, w.lever, w.pos);
  double *f = nullptr;
  if ((rc = ia_eval_batch(c, X, w.pos, w.lever, Nb, R, w.ia, &f, w.FT, w.e, w.gerr))) return rc;
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
