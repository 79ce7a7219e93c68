// rbl_joints.hip -- hard joints (include/rbl.h section 9): ball joints between anchor points fixed in two bodies, or in a body and
// the lab (a pivot), as constraint rows of the saddle system.  Shared internals are declared in rbl_api_internal.hpp.  Nothing here
// falls back to a CPU path.
//
// The system, in the convention of rbl_step_deterministic (rhs = [slip ; -F_body ; c]):
//     M lambda - K U            = slip
//     K^T lambda      + J^T phi = -F_body
//                   J U         = c
// (J U)_j = (u_A + w_A x l_A) - (u_B + w_B x l_B) with the lever arms l = R(Q) s of joint j's two anchors (no B term for a pivot),
// phi_j the joint's force, three unknowns behind the 3 N + 6 N_bod of the saddle system.  The Arnoldi recurrence, the Hessenberg
// solve and the convergence test are gmres_core's (gmres_core_with_ops with RblSolveOps::extra = 3 N_j); the operator is the
// library's own saddle product plus ONE tail launch (J^T phi into the body rows, J U into the joint rows).
//
// The right preconditioner is the exact inverse of the system with M replaced by the context's preconditioner M~ (apply_PC_dev
// with the force block's sign restored: P = [M~ -K ; K^T 0]^-1).  With P [0 ; h] = [. ; N^-1 h], N_b = K_b^T M~_b^-1 K_b = NL_b NL_b^T:
//     [lambda0 ; U0] = P [slip ; g],   phi = S^-1 (J U0 - c),   S = J N^-1 J^T,   [lambda ; U] = [lambda0 ; U0] - P [0 ; J^T phi]
// S (3 N_j rows, dense, couples only joints that share a body) is assembled from the per-body factors once per solve -- the
// configuration does not change inside one -- factored by the library's device Cholesky and inverted explicitly, so that an
// iteration applies it as one matrix-vector product.  The one redundant row of a closed hinge (two joints between one pair of
// bodies both hold the distance between their anchors) is expected: k_jt_geom finds it, k_jt_schur gives it an eigenvalue, so
// that S^-1 is the pseudo-inverse there -- the preconditioner stays bounded, the operator is untouched.  Any other joint set that
// leaves S singular (a loop of joints that constrains a relative coordinate twice) fails at the factorisation:
// RBL_ERR_NOT_SPD, "redundant" in the message, no answer.
//
// Kernels (all body- or joint-level and small; fixed-order sums, no floating-point atomics: results are bitwise reproducible):
//   k_jt_geom      one lane per joint: the lever arms of both ends, the gap g = p_A - p_B at the context's configuration and, for
//                  the joints of a closed hinge, their entries of its redundant row
//   k_jt_tail      the operator's tail and the preconditioner's two uses of J: one wave per jointed body over the CSR of joint
//                  ends for J^T phi (lanes stride the ends, LDS tree sum: any number of ends per body), one lane per joint for J U
//   k_jt_ninv      one lane per body: N_b^-1 (6 x 6, lab frame) from the body's Cholesky factor -- the context's per-body
//                  factors, or the ONE body-frame factor of the free-space tables rotated with the body
//   k_jt_schur     one work item per 3 x 3 block (j, k) of S: the one or two bodies the two joints share, found from the four
//                  body indices; every block is written by exactly one work item
//   k_jt_pivots    after the factorisation: a pivot that is not positive, not finite or lost to rounding latches RBL_FLAG_NOT_SPD
//   k_jt_mirror    L^T into the upper triangle, so that both substitution sweeps read columns
//   k_jt_inverse   one workgroup per column of S^-1: forward and backward substitution with the column in LDS, one barrier a step
//   k_jt_sinv      phi = S^-1 t: 64 rows a workgroup, four waves a quarter of the sum each, added in wave order
//   k_jt_step_rhs  c = -(gamma / dt) g + v of the time step
//
// Joint kinds (rbl_set_joint_kinds): every joint keeps three rows; the kind selects G of a joint end -- [I W] for a ball end, [0 I]
// for a lock end (w_A - w_B = c: a weld, or a motor), [0 P] for an axis end, P = I - ah ah^T (the relative rotation about ah =
// R(Q_A) a stays free).  k_jt_geom, k_jt_tail and k_jt_schur are templated on KINDS: a set without a lock or axis joint launches
// the <false> instantiations, the ball joint's code unchanged (the same bits whichever entry point stored the set), a set with
// one the <true> ones, which read the kind from the joint table.  An axis joint's row along ah constrains nothing: the operator's
// rows of that joint are P (w_A - w_B) - sigma ah (ah . phi_j) and S gets sigma ah ah^T on that diagonal block -- with the minus
// sign S = J N^-1 J^T + sigma ah ah^T is the exact Schur complement, so the preconditioner stays the exact inverse and no
// pseudo-inverse is involved.  The right-hand side's component along ah is projected out before the solve and phi's after it:
//   k_jt_across          x_j <- P x_j for every axis joint
//   k_jt_step_rhs_kinds  k_jt_step_rhs and a motor's - rate_j ah on its lock joint's rows
// The motor angles advance on the host after an accepted step and travel to the device with the rates (jt_upload).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"
#include "rbl_joints_dev.hpp"

namespace {

// one lane per joint: lev, gap and gau as jt_geom_joint (rbl_joints_dev.hpp) describes them.  The statements stand here a second
// time: called through that function the KINDS instantiation is scheduled differently, and this kernel keeps its code
template <bool KINDS>
__global__ __launch_bounds__(64) void k_jt_geom(const double *__restrict__ X, const double *__restrict__ Q, JtDev J,
                                                double *__restrict__ lev, double *__restrict__ gap, double *__restrict__ gau)
{
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= J.n) return;
  const int a = J.body[2 * (size_t)j], b = J.body[2 * (size_t)j + 1];
  const double *s = J.anchor + 6 * (size_t)j;
  double lA[3], lB[3], pB[3];
  if (KINDS && J.kind[j] != JT_BALL) {
    jt_angular(Q, J, j, a, b, lA, pB);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lev[6 * (size_t)j + c] = lA[c];
      lev[6 * (size_t)j + 3 + c] = 0.0;
      gap[3 * (size_t)j + c] = pB[c];
      if (gau) gau[3 * (size_t)j + c] = 0.0;
    }
    return;
  }
  jt_levers(Q, J, j, lA, lB);
#pragma unroll
  for (int c = 0; c < 3; ++c) pB[c] = b >= 0 ? X[3 * (size_t)b + c] + lB[c] : s[3 + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lev[6 * (size_t)j + c] = lA[c];
    lev[6 * (size_t)j + 3 + c] = lB[c];
    gap[3 * (size_t)j + c] = (X[3 * (size_t)a + c] + lA[c]) - pB[c];
  }
  if (!gau) return;
  double n[3] = {0.0, 0.0, 0.0};
  const int m = J.mate[2 * (size_t)j], swapped = J.mate[2 * (size_t)j + 1];
  if (m >= 0) {
    double mA[3], mB[3], dA[3], dB[3];
    jt_levers(Q, J, m, mA, mB);
    const bool lo = j < m;                               // dA, dB from the lower joint's point of view, on its bodies A and B
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double hA = swapped ? (lo ? mB[c] : lB[c]) : (lo ? mA[c] : lA[c]);
      const double hB = swapped ? (lo ? mA[c] : lA[c]) : (lo ? mB[c] : lB[c]);
      dA[c] = (lo ? lA[c] : mA[c]) - hA;
      dB[c] = (lo ? lB[c] : mB[c]) - hB;
    }
    const double nA = dA[0] * dA[0] + dA[1] * dA[1] + dA[2] * dA[2];
    double diff = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) diff += (dA[c] - dB[c]) * (dA[c] - dB[c]);
    const bool closed = b < 0 || diff <= JT_HINGE_CLOSED * JT_HINGE_CLOSED * nA;
    if (closed && nA > 0.0) {
      const double sc = ((lo || swapped) ? 1.0 : -1.0) / sqrt(nA);
#pragma unroll
      for (int c = 0; c < 3; ++c) n[c] = sc * dA[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) gau[3 * (size_t)j + c] = n[c];
}

// Workgroups [0, n_rows): body rows[w] takes J^T phi -- the force s phi_j and the torque l x (s phi_j) of every joint end on it,
// s = +1 at end A and -1 at end B -- added to body_out (add != 0) or stored there.  Workgroups behind them: one lane per joint,
// joint_out_j = (J U)_j - sub_j (sub NULL: zero).  Either half is skipped when its output is NULL.
// KINDS: a lock end loads its body with the torque s phi_j and no force, an axis end with s P phi_j, P = I - ah ah^T; their rows of
// J U are w_A - w_B and P (w_A - w_B), and with phi given an axis joint's rows are those of the operator, less sigma ah (ah . phi_j)
template <bool KINDS>
__global__ __launch_bounds__(64) void k_jt_tail(JtDev J, const double *__restrict__ lev, const double *__restrict__ phi, int add,
                                                double *__restrict__ body_out, const double *__restrict__ U,
                                                const double *__restrict__ sub, double *__restrict__ joint_out)
{
  __shared__ double red[6][64];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < J.n_rows) {
    if (!body_out) return;
    const int row = blockIdx.x, i = J.rows[row];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = J.ptr[row] + t; q < J.ptr[row + 1]; q += 64) {
      const int j = J.ends[2 * (size_t)q], end = J.ends[2 * (size_t)q + 1];
      const double s = end ? -1.0 : 1.0;
      const double *p = phi + 3 * (size_t)j;
      if (KINDS && J.kind[j] != JT_BALL) {
        double p0 = s * p[0], p1 = s * p[1], p2 = s * p[2];
        if (J.kind[j] == JT_AXIS) jt_across(lev + 6 * (size_t)j, p0, p1, p2);
        acc[3] += p0; acc[4] += p1; acc[5] += p2;
        continue;
      }
      rbl_KT_acc(lev + 6 * (size_t)j + 3 * end, s * p[0], s * p[1], s * p[2], acc);
    }
    rbl_block_sum<6, 64>(acc, red, t);
    if (t < 6) {
      double v = acc[0];
#pragma unroll
      for (int c = 1; c < 6; ++c) v = t == c ? acc[c] : v;   // (selects: a register array indexed by the lane would go to scratch)
      double *o = body_out + 6 * (size_t)i + t;
      *o = add ? *o + v : v;
    }
    return;
  }
  if (!joint_out) return;
  const int j = ((int)blockIdx.x - J.n_rows) * 64 + t;
  if (j >= J.n) return;
  const int a = J.body[2 * (size_t)j], b = J.body[2 * (size_t)j + 1];
  const double *l = lev + 6 * (size_t)j;
  double o0, o1, o2;
  if (KINDS && J.kind[j] != JT_BALL) {
    const double *wa = U + 6 * (size_t)a + 3;
    o0 = wa[0]; o1 = wa[1]; o2 = wa[2];
    if (b >= 0) {
      const double *wb = U + 6 * (size_t)b + 3;
      o0 -= wb[0]; o1 -= wb[1]; o2 -= wb[2];
    }
    if (J.kind[j] == JT_AXIS) {
      jt_across(l, o0, o1, o2);
      if (phi) {
        const double *p = phi + 3 * (size_t)j;
        const double d = jt_sigma(J.ninv, a) * (l[0] * p[0] + l[1] * p[1] + l[2] * p[2]);
        o0 -= l[0] * d; o1 -= l[1] * d; o2 -= l[2] * d;
      }
    }
  } else {
    rbl_KU(l, U + 6 * (size_t)a, o0, o1, o2);
    if (b >= 0) {
      double q0, q1, q2;
      rbl_KU(l + 3, U + 6 * (size_t)b, q0, q1, q2);
      o0 -= q0; o1 -= q1; o2 -= q2;
    }
  }
  if (sub) { o0 -= sub[3 * (size_t)j]; o1 -= sub[3 * (size_t)j + 1]; o2 -= sub[3 * (size_t)j + 2]; }
  joint_out[3 * (size_t)j] = o0; joint_out[3 * (size_t)j + 1] = o1; joint_out[3 * (size_t)j + 2] = o2;
}

// N_b^-1 = (L L^T)^-1 of every body, 6 x 6 row-major in the lab frame.  Q NULL: L = NL + 36 b, the body's own factor.  Q given:
// NL is the ONE body-frame factor of the free-space tables and N_b = (I2 x Rot_b) N_body (I2 x Rot_b)^T, so is its inverse.
// Every loop has compile-time bounds: the arrays stay in registers.
__global__ __launch_bounds__(64) void k_jt_ninv(const double *__restrict__ NL, const double *__restrict__ Q, int N_bod,
                                                double *__restrict__ Ninv)
{
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= N_bod) return;
  const double *L = Q ? NL : NL + 36 * (size_t)b;
  double X[6][6];                                        // L^-1, lower triangular
#pragma unroll
  for (int j = 0; j < 6; ++j) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i < j) { X[i][j] = 0.0; continue; }
      double v = i == j ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k >= j && k < i) v -= L[6 * i + k] * X[k][j];
      X[i][j] = v / L[6 * i + i];
    }
  }
  double A[6][6];                                        // L^-T L^-1
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k >= i && k >= j) v += X[k][i] * X[k][j];
      A[i][j] = v;
    }
  double *o = Ninv + 36 * (size_t)b;
  if (!Q) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) o[6 * i + j] = A[i][j];
    return;
  }
  double R[9];
  quat_rot(Q + 4 * (size_t)b, R);
#pragma unroll
  for (int hi = 0; hi < 2; ++hi)
#pragma unroll
    for (int hj = 0; hj < 2; ++hj) {                     // block (hi, hj): Rot A Rot^T
      double T[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          T[i][j] = R[3 * i] * A[3 * hi][3 * hj + j] + R[3 * i + 1] * A[3 * hi + 1][3 * hj + j] + R[3 * i + 2] * A[3 * hi + 2][3 * hj + j];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          o[6 * (3 * hi + i) + 3 * hj + j] = T[i][0] * R[3 * j] + T[i][1] * R[3 * j + 1] + T[i][2] * R[3 * j + 2];
    }
}

// S = J N^-1 J^T, dense column-major of order np >= 3 n (the rows behind 3 n: the identity), the caller has cleared it.  Work item
// g = j n + k owns the block of the joints j and k: for each pair of their ends that lies on ONE body b the term
// s_j s_k G_j N_b^-1 G_k^T with G = [I  W] of that end -- two ends of one joint lie on different bodies, so at most two terms.
// A closed hinge (gau != 0 on both its joints, k_jt_geom) adds sigma / 2 gau_j gau_k^T to its four blocks: its redundant row, which S
// annihilates, gets the eigenvalue sigma = the mean translational entry of N^-1 of the lower joint's body A, and S^-1 acts as the
// pseudo-inverse there.  diag0: the diagonal of S, kept for k_jt_pivots.
// KINDS: G = [0 I] for a lock end and [0 P] for an axis end, P = I - ah ah^T, and an axis joint's diagonal block gets
// sigma ah ah^T (jt_sigma): the row along its axis, which constrains nothing, has the eigenvalue the operator gives it
template <bool KINDS>
__global__ __launch_bounds__(256) void k_jt_schur(JtDev J, const double *__restrict__ lev, const double *__restrict__ gau,
                                                  const double *__restrict__ Ninv, long np, double *__restrict__ A,
                                                  double *__restrict__ diag0)
{
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)J.n;
  if (g < (size_t)np - 3 * n) {                          // the padding
    A[(3 * n + g) * (size_t)(np + 1)] = 1.0;
    diag0[3 * n + g] = 1.0;
  }
  if (g >= n * n) return;
  const int j = (int)(g / n), k = (int)(g - (size_t)j * n);
  double B[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int bj = J.body[2 * (size_t)j + e], bk = J.body[2 * (size_t)k + f];
      if (bj < 0 || bj != bk) continue;
      const double sgn = e == f ? 1.0 : -1.0;
      const double *Nb = Ninv + 36 * (size_t)bj;
      double Wj[3][3], Wk[3][3], T[6][3];
      double aj = 1.0, ak = 1.0;                         // G = [a I  W]
      if (KINDS) {
        aj = jt_G(J.kind[j], lev + 6 * (size_t)j, e, Wj);
        ak = jt_G(J.kind[k], lev + 6 * (size_t)k, f, Wk);
      } else {
        jt_W(lev + 6 * (size_t)j + 3 * e, Wj);
        jt_W(lev + 6 * (size_t)k + 3 * f, Wk);
      }
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c)                      // T = N_b^-1 G_k^T
          T[p][c] = (KINDS ? ak * Nb[6 * p + c] : Nb[6 * p + c]) + Nb[6 * p + 3] * Wk[c][0] + Nb[6 * p + 4] * Wk[c][1] + Nb[6 * p + 5] * Wk[c][2];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          B[r][c] += sgn * ((KINDS ? aj * T[r][c] : T[r][c]) + Wj[r][0] * T[3][c] + Wj[r][1] * T[4][c] + Wj[r][2] * T[5][c]);
    }
  if (KINDS && j == k && J.kind[j] == JT_AXIS) {
    const double sg = jt_sigma(Ninv, J.body[2 * (size_t)j]);
    const double *ah = lev + 6 * (size_t)j;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) B[r][c] += sg * ah[r] * ah[c];
  }
  const int mate = J.mate[2 * (size_t)j];
  if (mate >= 0 && (k == j || k == mate)) {
    const double *Nb = Ninv + 36 * (size_t)J.body[2 * (size_t)(j < mate ? j : mate)];
    const double half = (Nb[0] + Nb[7] + Nb[14]) * (0.5 / 3.0);
    const double *gj = gau + 3 * (size_t)j, *gk = gau + 3 * (size_t)k;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) B[r][c] += half * gj[r] * gk[c];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) A[(size_t)(3 * k + c) * (size_t)np + 3 * j + r] = B[r][c];
  if (j == k) {
#pragma unroll
    for (int r = 0; r < 3; ++r) diag0[3 * (size_t)j + r] = B[r][r];
  }
}

__global__ __launch_bounds__(256) void k_jt_pivots(const double *__restrict__ A, long np, const double *__restrict__ diag0, double tol,
                                                   unsigned *err)
{
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const double d = A[(size_t)i * (size_t)(np + 1)], s = diag0[i];
  if (!(d > 0.0) || !isfinite(d) || !(s > 0.0) || !(d * d > tol * s)) atomicOr(err, (unsigned)RBL_FLAG_NOT_SPD);
}

// A[r][c] = A[c][r] for r < c (column-major): the factor's transpose above the diagonal
__global__ __launch_bounds__(256) void k_jt_mirror(double *__restrict__ A, long np)
{
  const long c = blockIdx.y, r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < c) A[(size_t)c * (size_t)np + r] = A[(size_t)r * (size_t)np + c];
}

// Column col of S^-1 = L^-T L^-1 e_col, one workgroup a column, the column in LDS.  Thread t owns the rows r = t (mod 256): it alone
// updates x[r], so a step is: the owner of row i closes x[i], one barrier, every thread takes x[i] out of its own rows further
// on.  Forward (L y = e_col, rows from col on) reads column i of L below the diagonal, backward (L^T x = y) column i of the
// mirrored upper triangle above it: consecutive addresses across the workgroup both times.
__global__ __launch_bounds__(256) void k_jt_inverse(const double *__restrict__ A, int np, double *__restrict__ Sinv)
{
  extern __shared__ double x[];
  const int t = threadIdx.x, col = blockIdx.x;
  for (int r = t; r < np; r += 256) x[r] = r == col ? 1.0 : 0.0;
  __syncthreads();
  for (int i = col; i < np; ++i) {
    const double *Ai = A + (size_t)i * (size_t)np;
    if (t == (i & 255)) x[i] = x[i] / Ai[i];
    __syncthreads();
    const double xi = x[i];
    for (int r = i + 1 + ((t - (i + 1)) & 255); r < np; r += 256) x[r] -= Ai[r] * xi;
  }
  for (int i = np - 1; i >= 0; --i) {
    const double *Ai = A + (size_t)i * (size_t)np;
    if (t == (i & 255)) x[i] = x[i] / Ai[i];
    __syncthreads();
    const double xi = x[i];
    for (int r = t; r < i; r += 256) x[r] -= Ai[r] * xi;
  }
  __syncthreads();
  for (int r = t; r < np; r += 256) Sinv[(size_t)col * (size_t)np + r] = x[r];
}

// out = S^-1 in over the first m = 3 N_j rows and columns (S^-1 is symmetric: row r is read down column-major columns)
__global__ __launch_bounds__(256) void k_jt_sinv(const double *__restrict__ Sinv, long np, int m, const double *__restrict__ in,
                                                 double *__restrict__ out)
{
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = blockIdx.x * 64 + lane;
  double acc = 0.0;
  if (r < m)
    for (int c = w; c < m; c += 4) acc = __builtin_fma(Sinv[(size_t)c * (size_t)np + r], in[c], acc);
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && r < m) out[r] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// c = coef gap + v  (v NULL: zero)
__global__ __launch_bounds__(256) void k_jt_step_rhs(const double *__restrict__ gap, const double *__restrict__ v, double coef, int m,
                                                     double *__restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = coef * gap[i] + (v ? v[i] : 0.0);
}

// the same for a set with angular joints: a lock's row takes its motor's rate, - rate_j ah (body B turns at + rate_j about ah
// relative to body A); lev holds ah
__global__ __launch_bounds__(256) void k_jt_step_rhs_kinds(const double *__restrict__ gap, const double *__restrict__ v, double coef, int m,
                                                           JtDev J, const double *__restrict__ lev, double *__restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int j = i / 3, r = i - 3 * j;
  double o = coef * gap[i] + (v ? v[i] : 0.0);
  if (J.kind[j] == JT_LOCK) o -= J.rate[j] * lev[6 * (size_t)j + r];
  out[i] = o;
}

// x_j <- P x_j for every axis joint, one lane a joint: the right-hand side's rows before the solve (the component along the
// axis is ignored) and phi after it (its component along the axis is zero; GMRES leaves rounding there)
__global__ __launch_bounds__(64) void k_jt_across(JtDev J, const double *__restrict__ lev, double *__restrict__ x)
{
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= J.n || J.kind[j] != JT_AXIS) return;
  double v0 = x[3 * (size_t)j], v1 = x[3 * (size_t)j + 1], v2 = x[3 * (size_t)j + 2];
  jt_across(lev + 6 * (size_t)j, v0, v1, v2);
  x[3 * (size_t)j] = v0; x[3 * (size_t)j + 1] = v1; x[3 * (size_t)j + 2] = v2;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------

bool jt_active(const rbl_ctx *c) { return c->jt_on && c->jt_n > 0; }

long jt_np(const rbl_ctx *c) { return ((3L * c->jt_n + 31) / 32) * 32; }

struct JtBuf {             // the one workspace of a section 9 entry point (rbl_ctx::d_jtw)
  double *rhs, *x, *v, *w, *t, *lev, *gap, *c, *gau;
};

int jt_reserve(rbl_ctx *c, JtBuf &B)
{
  const size_t nj3 = 3 * (size_t)c->jt_n, nsys = sizes_of(c).nsys, n = nsys + nj3;
  const int rc = rbl_dev_reserve(c, c->d_jtw, sizeof(double) * (2 * n + 2 * nsys + 6 * nj3));
  if (rc) return rc;
  B.rhs = (double *)c->d_jtw.p; B.x = B.rhs + n; B.v = B.x + n; B.w = B.v + nsys; B.t = B.w + nsys; B.lev = B.t + nj3;
  B.gap = B.lev + 2 * nj3; B.c = B.gap + nj3; B.gau = B.c + nj3;
  return RBL_OK;
}

// the joints on the device, once per rbl_set_joints: anchors | bodies | rows | row starts | ends | mates.  A set with angular
// joints (jt_angular): anchors | axes and q_rel | theta | rates | the same integers | kinds, and again after every change of theta
// or of the rates
int jt_upload(rbl_ctx *c)
{
  if (c->jt_valid) return RBL_OK;
  const std::vector<double> *dpart[4] = {&c->jt_anchor, &c->jt_ang, &c->jt_theta, &c->jt_rate};
  const std::vector<int> *ipart[6] = {&c->jt_body, &c->jt_rows, &c->jt_ptr, &c->jt_ends, &c->jt_mate, &c->jt_kind};
  const int nd = c->jt_angular ? 4 : 1, nip = c->jt_angular ? 6 : 5;
  size_t ndbl = 0, ni = 0;
  for (int k = 0; k < nd; ++k) ndbl += dpart[k]->size();
  for (int k = 0; k < nip; ++k) ni += ipart[k]->size();
  int rc = rbl_dev_reserve(c, c->d_jt, sizeof(double) * ndbl + sizeof(int) * ni); if (rc) return rc;
  double *dq = (double *)c->d_jt.p;
  for (int k = 0; k < nd; ++k) {
    if ((rc = copy_h2d(c, dq, dpart[k]->data(), sizeof(double) * dpart[k]->size()))) return rc;
    dq += dpart[k]->size();
  }
  int *q = (int *)dq;
  for (int k = 0; k < nip; ++k) {
    const std::vector<int> *v = ipart[k];
    if ((rc = copy_h2d(c, q, v->data(), sizeof(int) * v->size()))) return rc;
    q += v->size();
  }
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  c->jt_valid = true;
  return RBL_OK;
}

JtDev jt_args(const rbl_ctx *c)
{
  JtDev J = {};
  J.anchor = (const double *)c->d_jt.p;
  const double *dend = J.anchor + c->jt_anchor.size();
  if (c->jt_angular) {
    J.ang = dend;
    J.theta = J.ang + c->jt_ang.size();
    J.rate = J.theta + c->jt_theta.size();
    dend = J.rate + c->jt_rate.size();
  }
  J.body = (const int *)dend;
  J.rows = J.body + c->jt_body.size();
  J.ptr = J.rows + c->jt_rows.size();
  J.ends = J.ptr + c->jt_ptr.size();
  J.mate = J.ends + c->jt_ends.size();
  if (c->jt_angular) J.kind = J.mate + c->jt_mate.size();
  J.n = c->jt_n; J.n_rows = (int)c->jt_rows.size();
  return J;
}

// what every jointed call asks of the context before it touches a device
int jt_check(rbl_ctx *c, const char *who, int max_iter, double rtol)
{
  if (max_iter < 1 || !(rtol >= 0.0)) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": need max_iter >= 1 and rtol >= 0");
  if (max_iter + 1 > rbl_gmres_max_vectors()) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": at most 255 iterations (no restart)");
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": not available on a context with a communicator");
  if (c->ens_R > 0) return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": not available on a context that holds an ensemble");
  return RBL_OK;
}

// ... and once the configuration is known to exist: every joint names a body of it
int jt_range(rbl_ctx *c, const char *who)
{
  if (c->jt_n > 0 && c->jt_top >= c->S.N_bod)
    for (int j = 0; j < c->jt_n; ++j) {
      const int m = std::max(c->jt_body[2 * (size_t)j], c->jt_body[2 * (size_t)j + 1]);
      if (m >= c->S.N_bod)
        return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": joint " + std::to_string(j) + " names body " + std::to_string(m) +
                                              ", the system has " + std::to_string(c->S.N_bod) + " bodies (rbl_set_joints)");
    }
  return RBL_OK;
}

// lever arms and gaps of the stored joints at the context's configuration
int jt_geom(rbl_ctx *c, double *lev, double *gap, double *gau)
{
  int rc = jt_upload(c); if (rc) return rc;
  if ((rc = ensure_xq_dev(c))) return rc;
  const double *dX = (const double *)c->d_XQ.p;
  const dim3 grid((unsigned)((c->jt_n + 63) / 64));
  if (c->jt_angular)
    hipLaunchKernelGGL(k_jt_geom<true>, grid, dim3(64), 0, c->stream, dX, dX + 3 * (size_t)c->S.N_bod, jt_args(c), lev, gap, gau);
  else
    hipLaunchKernelGGL(k_jt_geom<false>, grid, dim3(64), 0, c->stream, dX, dX + 3 * (size_t)c->S.N_bod, jt_args(c), lev, gap, gau);
  return RBL_OK;
}

struct JtSolve {
  const JtBuf *B;
  JtDev J;
  const double *Sinv;
  long np;
};

void jt_launch_tail(rbl_ctx *c, const JtSolve *m, const double *phi, int add, double *body_out, const double *U, const double *sub,
                    double *joint_out)
{
  const dim3 grid((unsigned)(m->J.n_rows + (m->J.n + 63) / 64));
  if (m->J.kind)
    hipLaunchKernelGGL(k_jt_tail<true>, grid, dim3(64), 0, c->stream, m->J, (const double *)m->B->lev, phi, add, body_out, U, sub, joint_out);
  else
    hipLaunchKernelGGL(k_jt_tail<false>, grid, dim3(64), 0, c->stream, m->J, (const double *)m->B->lev, phi, add, body_out, U, sub, joint_out);
}

int jt_op(rbl_ctx *c, void *user, const double *d_x, double *d_out)
{
  const JtSolve *m = (const JtSolve *)user;
  const long n3 = (long)sizes_of(c).n3, nsys = (long)sizes_of(c).nsys;
  const int rc = rbl_apply_saddle_dev(c, d_x, d_out); if (rc) return rc;
  jt_launch_tail(c, m, d_x + nsys, 1, d_out + n3, d_x + n3, nullptr, d_out + nsys);
  return RBL_OK;
}

int jt_pc(rbl_ctx *c, void *user, const double *d_in, double *d_out)
{
  const JtSolve *m = (const JtSolve *)user;
  const JtBuf &B = *m->B;
  const long n3 = (long)sizes_of(c).n3, nsys = (long)sizes_of(c).nsys;
  const int nj3 = 3 * m->J.n;
  RblPcReq rq;
  rq.fsign = 1.0;
  int rc = apply_PC_dev(c, d_in, d_out, rq); if (rc) return rc;                     // [lambda0 ; U0]
  jt_launch_tail(c, m, nullptr, 0, nullptr, d_out + n3, d_in + nsys, B.t);         // t = J U0 - c
  hipLaunchKernelGGL(k_jt_sinv, dim3((unsigned)((nj3 + 63) / 64)), dim3(256), 0, c->stream, m->Sinv, m->np, nj3, (const double *)B.t,
                     d_out + nsys);                                                  // phi = S^-1 t
  jt_launch_tail(c, m, d_out + nsys, 0, B.v + n3, nullptr, nullptr, nullptr);       // v = (0, J^T phi): the other rows stay zero
  RblPcReq rq2;
  rq2.fsign = 1.0;
  if ((rc = apply_PC_dev(c, B.v, B.w, rq2))) return rc;
  rbl_launch_axpby(c->stream, nsys, 1.0, d_out, -1.0, B.w, d_out);
  return RBL_OK;
}

// S of the context's configuration, its factor and its inverse; the preconditioner must be built (rbl_prepare_dev) and the latched
// flags clean.  A singular S: RBL_ERR_NOT_SPD with the message below
int jt_factor(rbl_ctx *c, const char *who, const JtBuf &B, const double **Sinv, const double **Ninv_out)
{
  const RblBodyState &S = c->S;
  const long np = jt_np(c);
  const size_t nb36 = 36 * (size_t)S.N_bod, sq = (size_t)np * (size_t)np;
  int rc = rbl_dev_reserve(c, c->d_jtS, sizeof(double) * (nb36 + 2 * sq + (size_t)np)); if (rc) return rc;
  double *Ninv = (double *)c->d_jtS.p, *A = Ninv + nb36, *Si = A + sq, *diag0 = Si + sq;
  const bool shared = S.block_pc && bf_on(c) && c->bf_tables;            // one body-frame factor for all bodies, behind the tables
  const size_t mb = 3 * (size_t)S.N_blb;
  const double *NL = shared ? (const double *)c->d_bfPC.p + mb * mb + 6 * mb : (const double *)c->d_NL.p;
  if (shared && (rc = ensure_xq_dev(c))) return rc;
  hipLaunchKernelGGL(k_jt_ninv, dim3((unsigned)((S.N_bod + 63) / 64)), dim3(64), 0, c->stream, NL,
                     shared ? (const double *)c->d_XQ.p + 3 * (size_t)S.N_bod : nullptr, S.N_bod, Ninv);
  RBL_HIP(c, hipMemsetAsync(A, 0, sizeof(double) * sq, c->stream));
  const JtDev J = jt_args(c);
  const size_t items = std::max((size_t)J.n * (size_t)J.n, (size_t)np);
  if (c->jt_angular)
    hipLaunchKernelGGL(k_jt_schur<true>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, c->stream, J, (const double *)B.lev,
                       (const double *)B.gau, (const double *)Ninv, np, A, diag0);
  else
    hipLaunchKernelGGL(k_jt_schur<false>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, c->stream, J, (const double *)B.lev,
                       (const double *)B.gau, (const double *)Ninv, np, A, diag0);
  if ((rc = rbl_dev_reserve(c, c->d_chol, rbl_cholesky_work_bytes(np)))) return rc;
  rc = rbl_launch_cholesky(c->stream, A, np, false, c->d_err, (double *)c->d_chol.p, c->d_chol.bytes, &c->chol_aux);
  if (rc) return rbl_fail(c, rc, std::string(who) + ": cholesky launch failed");
  hipLaunchKernelGGL(k_jt_pivots, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream, (const double *)A, np, (const double *)diag0,
                     JT_PIVOT_TOL, c->d_err);
  if ((rc = finish_and_check(c))) {
    if (rc == RBL_ERR_NOT_SPD)
      return rbl_fail(c, rc, std::string(who) + ": the joints are redundant: their Schur complement J N^-1 J^T is not positive definite "
                                                "(a loop of joints constrains a relative coordinate twice)");
    return rc;
  }
  hipLaunchKernelGGL(k_jt_mirror, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, c->stream, A, np);
  hipLaunchKernelGGL(k_jt_inverse, dim3((unsigned)np), dim3(256), sizeof(double) * (size_t)np, c->stream, (const double *)A, (int)np, Si);
  RBL_HIP(c, hipGetLastError());
  *Sinv = Si;
  *Ninv_out = Ninv;
  return RBL_OK;
}

// the solve on the buffers of B (rhs = [slip ; -F ; c], lever arms in place): leaves x = [lambda ; U ; phi] and the context's
// copy of phi; nothing is read back beyond the solver's convergence tests
int jt_solve(rbl_ctx *c, const char *who, const JtBuf &B, int max_iter, double rtol, int *iters, double *resid)
{
  RblPhase ph_total(c, RBL_T_TOTAL);
  c->jt_phi_valid = false;
  int rc = rbl_prepare_dev(c); if (rc) return rc;                        // resident geometry, the preconditioner of this configuration
  const size_t nsys = sizes_of(c).nsys, nj3 = 3 * (size_t)c->jt_n;
  JtSolve m{&B, jt_args(c), nullptr, jt_np(c)};
  if ((rc = jt_factor(c, who, B, &m.Sinv, &m.J.ninv))) return rc;
  RBL_HIP(c, hipMemsetAsync(B.v, 0, sizeof(double) * nsys, c->stream));
  const dim3 jgrid((unsigned)((c->jt_n + 63) / 64));
  if (c->jt_angular)                                     // an axis joint's right-hand side counts across its axis only
    hipLaunchKernelGGL(k_jt_across, jgrid, dim3(64), 0, c->stream, m.J, (const double *)B.lev, B.rhs + nsys);
  RblSolveOps ops{jt_op, jt_pc, &m};
  ops.extra = (int64_t)nj3;
  if ((rc = gmres_core_with_ops(c, &ops, B.rhs, max_iter, rtol, B.x, iters, resid))) return rc;
  if (c->jt_angular) hipLaunchKernelGGL(k_jt_across, jgrid, dim3(64), 0, c->stream, m.J, (const double *)B.lev, B.x + nsys);
  if ((rc = rbl_dev_reserve(c, c->d_jtphi, sizeof(double) * 4 * nj3))) return rc;
  RBL_HIP(c, hipMemcpyAsync(c->d_jtphi.p, B.x + nsys, sizeof(double) * nj3, hipMemcpyDeviceToDevice, c->stream));
  c->jt_phi_valid = true;
  return RBL_OK;
}

// rhs = [slip (or zero) ; -F ; c (or zero)] from device vectors; d_F may be B.v
int jt_rhs(rbl_ctx *c, const JtBuf &B, const double *d_F, bool have_slip, const double *d_c)
{
  const RblSizes z = sizes_of(c);
  const size_t nj3 = 3 * (size_t)c->jt_n;
  if (!have_slip) RBL_HIP(c, hipMemsetAsync(B.rhs, 0, sizeof(double) * z.n3, c->stream));
  rbl_launch_axpby(c->stream, (int64_t)z.nb6, -1.0, d_F, 0.0, nullptr, B.rhs + z.n3);
  if (d_c) RBL_HIP(c, hipMemcpyAsync(B.rhs + z.nsys, d_c, sizeof(double) * nj3, hipMemcpyDeviceToDevice, c->stream));
  else RBL_HIP(c, hipMemsetAsync(B.rhs + z.nsys, 0, sizeof(double) * nj3, c->stream));
  return RBL_OK;
}

// joints switched off or never set: the plain saddle solve on [slip ; -F], the caller's arrays on either side
int jt_plain_solve(rbl_ctx *c, RblSide side, const double *F_body, const double *slip, int max_iter, double rtol, double *lambda, double *U,
                   int *iters, double *resid)
{
  const RblSizes z = sizes_of(c);
  int rc = rbl_dev_reserve(c, c->d_jtw, sizeof(double) * (2 * z.nsys + z.nb6)); if (rc) return rc;
  double *x = (double *)c->d_jtw.p, *rhs = x + z.nsys, *f = rhs + z.nsys;
  if (slip && (rc = xfer_in(c, side, rhs, slip, sizeof(double) * z.n3))) return rc;
  if ((rc = xfer_in(c, side, f, F_body, sizeof(double) * z.nb6))) return rc;
  if (!slip) RBL_HIP(c, hipMemsetAsync(rhs, 0, sizeof(double) * z.n3, c->stream));
  rbl_launch_axpby(c->stream, (int64_t)z.nb6, -1.0, f, 0.0, nullptr, rhs + z.n3);
  if ((rc = rbl_gmres_saddle_dev(c, rhs, max_iter, rtol, x, 0, iters, resid))) return rc;
  if (lambda && (rc = xfer_out(c, side, lambda, x, sizeof(double) * z.n3))) return rc;
  if (U && (rc = xfer_out(c, side, U, x + z.n3, sizeof(double) * z.nb6))) return rc;
  return finish_and_check(c);
}

// The jointed solve, the checks done and the device up: the caller's arrays (either side) in, the solve, lambda, U and phi out
// where they are not NULL.  A host caller's loads and joint right-hand side go up into the workspace; a device caller's are read
// where they are.  Nothing is drained beyond the solver's convergence tests
int jt_solve_core(rbl_ctx *c, const char *who, RblSide side, const double *F_body, const double *slip, const double *joint_rhs, int max_iter,
                  double rtol, double *lambda, double *U, double *phi, int *iters, double *resid)
{
  const RblSizes z = sizes_of(c);
  const size_t nj3 = 3 * (size_t)c->jt_n;
  JtBuf B;
  int rc = jt_reserve(c, B); if (rc) return rc;
  if ((rc = jt_geom(c, B.lev, B.gap, B.gau))) return rc;
  if (slip && (rc = xfer_in(c, side, B.rhs, slip, sizeof(double) * z.n3))) return rc;
  if (side == RblSide::Host) {
    if ((rc = copy_h2d(c, B.v, F_body, sizeof(double) * z.nb6))) return rc;
    if (joint_rhs && (rc = copy_h2d(c, B.c, joint_rhs, sizeof(double) * nj3))) return rc;
    F_body = B.v;
    if (joint_rhs) joint_rhs = B.c;
  }
  if ((rc = jt_rhs(c, B, F_body, slip != nullptr, joint_rhs))) return rc;
  if ((rc = jt_solve(c, who, B, max_iter, rtol, iters, resid))) return rc;
  if (lambda && (rc = xfer_out(c, side, lambda, B.x, sizeof(double) * z.n3))) return rc;
  if (U && (rc = xfer_out(c, side, U, B.x + z.n3, sizeof(double) * z.nb6))) return rc;
  if (phi && (rc = xfer_out(c, side, phi, B.x + z.nsys, sizeof(double) * nj3))) return rc;
  return RBL_OK;
}

}   // namespace

// ---- the C ABI (include/rbl.h section 9) -------------------------------------------------------------------------------------------

static void jt_store(rbl_ctx *c, int n_joints, const int *body, const double *anchor, const int *kind, int on, int top);

// the joints: checks first, nothing is stored unless every one passes; then the CSR of joint ends by body
int rbl_set_joints(rbl_ctx *c, int n_joints, const int *body, const double *anchor, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!body && !anchor && !on) { c->jt_on = false; return RBL_OK; }
  if (!body) return rbl_fail(c, RBL_ERR_ARG, "set_joints: body must not be NULL");
  if (!anchor) return rbl_fail(c, RBL_ERR_ARG, "set_joints: anchor must not be NULL");
  if (n_joints < 1 || n_joints > JT_MAX) return rbl_fail(c, RBL_ERR_ARG, "set_joints: n_joints must lie in [1, " + std::to_string(JT_MAX) + "]");
  int top = -1;
  std::map<std::pair<int, int>, int> count;
  for (int j = 0; j < n_joints; ++j) {
    const int a = body[2 * (size_t)j], b = body[2 * (size_t)j + 1];
    const std::string at = "set_joints: joint " + std::to_string(j) + ": ";
    if (a == -1) return rbl_fail(c, RBL_ERR_ARG, at + "body[2 j] is -1: a pivot's lab point goes in the second slot, the body in the first");
    if (a < 0 || b < -1 || (c->S.cfg_set && std::max(a, b) >= c->S.N_bod))
      return rbl_fail(c, RBL_ERR_ARG, at + "body index out of range (the first >= 0, the second >= 0 or -1 for a lab point" +
                                          (c->S.cfg_set ? ", both below the " + std::to_string(c->S.N_bod) + " bodies of the configuration)" : ")"));
    if (a == b) return rbl_fail(c, RBL_ERR_ARG, at + "body: both ends lie on one body (a joint inside a rigid body constrains nothing)");
    for (int q = 0; q < 6; ++q)
      if (!std::isfinite(anchor[6 * (size_t)j + q])) return rbl_fail(c, RBL_ERR_ARG, at + "every value of anchor must be finite");
    if (++count[std::make_pair(std::min(a, b), std::max(a, b))] > 2)
      return rbl_fail(c, RBL_ERR_ARG, at + (b < 0 ? "a third pivot on body " + std::to_string(a)
                                                  : "a third joint between the bodies " + std::to_string(std::min(a, b)) + " and " + std::to_string(std::max(a, b))) +
                                          ": three ball joints would constrain nine of six relative coordinates");
    top = std::max(top, std::max(a, b));
  }
  jt_store(c, n_joints, body, anchor, nullptr, on, top);
  return RBL_OK;
}

// the checked joints into the context: the mates, the CSR of joint ends by body.  kind NULL: ball joints only
static void jt_store(rbl_ctx *c, int n_joints, const int *body, const double *anchor, const int *kind, int on, int top)
{
  c->jt_n = n_joints; c->jt_top = top;
  c->jt_by_kinds = kind != nullptr;
  c->jt_angular = false;
  c->jt_kind.assign((size_t)n_joints, JT_BALL);
  c->jt_ang.assign(7 * (size_t)n_joints, 0.0);
  c->jt_theta.assign((size_t)n_joints, 0.0);
  c->jt_rate.assign((size_t)n_joints, 0.0);
  for (int j = 0; j < n_joints; ++j) {
    c->jt_ang[7 * (size_t)j + 3] = 1.0;                  // q_rel of a ball joint reads back as the identity
    if (kind && kind[j] != JT_BALL) { c->jt_kind[j] = kind[j]; c->jt_angular = true; }
  }
  // the two ball joints of a pair of bodies name each other (at most two: checked by the caller)
  c->jt_mate.assign(2 * (size_t)n_joints, -1);
  std::map<std::pair<int, int>, int> first;
  for (int j = 0; j < n_joints; ++j) {
    if (c->jt_kind[j] != JT_BALL) continue;
    const int a = body[2 * (size_t)j], b = body[2 * (size_t)j + 1];
    const auto hit = first.emplace(std::make_pair(std::min(a, b), std::max(a, b)), j);
    if (hit.second) continue;
    const int m = hit.first->second, swapped = body[2 * (size_t)m] != a ? 1 : 0;
    c->jt_mate[2 * (size_t)j] = m; c->jt_mate[2 * (size_t)m] = j;
    c->jt_mate[2 * (size_t)j + 1] = c->jt_mate[2 * (size_t)m + 1] = swapped;
  }
  for (int j = 0; j < n_joints; ++j)
    if (c->jt_mate[2 * (size_t)j] < 0) c->jt_mate[2 * (size_t)j + 1] = 0;
  c->jt_body.assign(body, body + 2 * (size_t)n_joints);
  c->jt_anchor.assign(6 * (size_t)n_joints, 0.0);        // an angular joint has no anchors: zeros
  for (int j = 0; j < n_joints; ++j)
    if (c->jt_kind[j] == JT_BALL) std::copy(anchor + 6 * (size_t)j, anchor + 6 * (size_t)j + 6, c->jt_anchor.begin() + 6 * (size_t)j);
  // joint ends by body, in increasing joint index: the ends in joint order, sorted by body with a stable sort
  struct End { int body, joint, end; };
  std::vector<End> ends;
  ends.reserve(2 * (size_t)n_joints);
  for (int j = 0; j < n_joints; ++j)
    for (int q = 0; q < 2; ++q)
      if (body[2 * (size_t)j + q] >= 0) ends.push_back({body[2 * (size_t)j + q], j, q});
  std::stable_sort(ends.begin(), ends.end(), [](const End &x, const End &y) { return x.body < y.body; });
  c->jt_rows.clear(); c->jt_ptr.clear();
  c->jt_ends.resize(2 * ends.size());
  for (size_t q = 0; q < ends.size(); ++q) {
    if (!q || ends[q].body != ends[q - 1].body) {
      c->jt_rows.push_back(ends[q].body);
      c->jt_ptr.push_back((int)q);
    }
    c->jt_ends[2 * q] = ends[q].joint; c->jt_ends[2 * q + 1] = ends[q].end;
  }
  c->jt_ptr.push_back((int)ends.size());
  c->jt_on = on != 0;
  c->jt_valid = false;
  c->jt_phi_valid = false;
  ++c->jt_gen;                                           // an ensemble's angles and rates belonged to the set before (rbl_ensemble.hip)
}

int rbl_get_joints(const rbl_ctx *c, int *n_joints, int *on, int *body, double *anchor)
{
  if (!c) return RBL_ERR_ARG;
  if (n_joints) *n_joints = c->jt_n;
  if (on) *on = c->jt_on ? 1 : 0;
  if (body && c->jt_n) std::memcpy(body, c->jt_body.data(), sizeof(int) * c->jt_body.size());
  if (anchor && c->jt_n) std::memcpy(anchor, c->jt_anchor.data(), sizeof(double) * c->jt_anchor.size());
  return RBL_OK;
}

// joints of every kind: rbl_set_joints' checks and those of the angular joints, then the same storing
int rbl_set_joint_kinds(rbl_ctx *c, int n_joints, const int *body, const double *anchor, const int *kind, const double *axis,
                        const double *q_rel, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!body && !anchor && !kind && !axis && !q_rel && !on) { c->jt_on = false; return RBL_OK; }
  if (!body) return rbl_fail(c, RBL_ERR_ARG, "set_joint_kinds: body must not be NULL");
  if (!kind) return rbl_fail(c, RBL_ERR_ARG, "set_joint_kinds: kind must not be NULL");
  if (n_joints < 1 || n_joints > JT_MAX)
    return rbl_fail(c, RBL_ERR_ARG, "set_joint_kinds: n_joints must lie in [1, " + std::to_string(JT_MAX) + "]");
  int top = -1;
  std::map<std::pair<int, int>, std::pair<int, int>> count;        // balls, angular joints of a pair of bodies
  std::vector<double> ang(7 * (size_t)n_joints, 0.0);
  for (int j = 0; j < n_joints; ++j) {
    const int a = body[2 * (size_t)j], b = body[2 * (size_t)j + 1], k = kind[j];
    const std::string at = "set_joint_kinds: joint " + std::to_string(j) + ": ";
    if (k != JT_BALL && k != JT_LOCK && k != JT_AXIS)
      return rbl_fail(c, RBL_ERR_ARG, at + "unknown kind " + std::to_string(k) + " (RBL_JOINT_BALL 0, RBL_JOINT_LOCK 1, RBL_JOINT_AXIS 2)");
    if (a == -1) return rbl_fail(c, RBL_ERR_ARG, at + "body[2 j] is -1: the lab goes in the second slot, the body in the first");
    if (a < 0 || b < -1 || (c->S.cfg_set && std::max(a, b) >= c->S.N_bod))
      return rbl_fail(c, RBL_ERR_ARG, at + "body index out of range (the first >= 0, the second >= 0 or -1 for the lab" +
                                          (c->S.cfg_set ? ", both below the " + std::to_string(c->S.N_bod) + " bodies of the configuration)" : ")"));
    if (a == b) return rbl_fail(c, RBL_ERR_ARG, at + "body: both ends lie on one body (a joint inside a rigid body constrains nothing)");
    ang[7 * (size_t)j + 3] = 1.0;
    if (k == JT_BALL) {
      if (!anchor) return rbl_fail(c, RBL_ERR_ARG, at + "a ball joint needs anchor, which is NULL");
      for (int q = 0; q < 6; ++q)
        if (!std::isfinite(anchor[6 * (size_t)j + q])) return rbl_fail(c, RBL_ERR_ARG, at + "every value of anchor must be finite");
    } else {
      if (!axis || !q_rel) return rbl_fail(c, RBL_ERR_ARG, at + "a lock or axis joint needs axis and q_rel, one of which is NULL");
      double na = 0.0, nq = 0.0;
      for (int q = 0; q < 3; ++q) na += axis[3 * (size_t)j + q] * axis[3 * (size_t)j + q];
      for (int q = 0; q < 4; ++q) nq += q_rel[4 * (size_t)j + q] * q_rel[4 * (size_t)j + q];
      na = std::sqrt(na); nq = std::sqrt(nq);
      if (!std::isfinite(na) || na < 1e-12) return rbl_fail(c, RBL_ERR_ARG, at + "axis must be finite and of norm >= 1e-12");
      if (!std::isfinite(nq) || !(nq > 0.0)) return rbl_fail(c, RBL_ERR_ARG, at + "q_rel must be finite and of non-zero norm");
      for (int q = 0; q < 3; ++q) ang[7 * (size_t)j + q] = axis[3 * (size_t)j + q] / na;
      for (int q = 0; q < 4; ++q) ang[7 * (size_t)j + 3 + q] = q_rel[4 * (size_t)j + q] / nq;
    }
    std::pair<int, int> &n = count[std::make_pair(std::min(a, b), std::max(a, b))];
    const std::string pair = b < 0 ? "body " + std::to_string(a) + " and the lab"
                                   : "the bodies " + std::to_string(std::min(a, b)) + " and " + std::to_string(std::max(a, b));
    if (k == JT_BALL && ++n.first > 2)
      return rbl_fail(c, RBL_ERR_ARG, at + (b < 0 ? "a third pivot on body " + std::to_string(a) : "a third joint between " + pair) +
                                          ": three ball joints would constrain nine of six relative coordinates");
    if (k != JT_BALL && ++n.second > 1)
      return rbl_fail(c, RBL_ERR_ARG, at + "a second angular joint between " + pair + ": one lock or axis joint a pair");
    if (n.first > 1 && n.second > 0)
      return rbl_fail(c, RBL_ERR_ARG, at + "an angular joint together with two ball joints between " + pair +
                                          ": the second ball joint would constrain what the angular joint already holds");
    top = std::max(top, std::max(a, b));
  }
  jt_store(c, n_joints, body, anchor, kind, on, top);
  for (int j = 0; j < n_joints; ++j)
    if (kind[j] != JT_BALL) std::copy(ang.begin() + 7 * (size_t)j, ang.begin() + 7 * (size_t)j + 7, c->jt_ang.begin() + 7 * (size_t)j);
  return RBL_OK;
}

int rbl_get_joint_kinds(const rbl_ctx *c, int *n_joints, int *on, int *by_kinds, int *body, double *anchor, int *kind, double *axis,
                        double *q_rel, double *theta, double *rate)
{
  if (!c) return RBL_ERR_ARG;
  if (n_joints) *n_joints = c->jt_n;
  if (on) *on = c->jt_on ? 1 : 0;
  if (by_kinds) *by_kinds = c->jt_n > 0 && c->jt_by_kinds ? 1 : 0;
  if (!c->jt_n) return RBL_OK;
  if (body) std::memcpy(body, c->jt_body.data(), sizeof(int) * c->jt_body.size());
  if (anchor) std::memcpy(anchor, c->jt_anchor.data(), sizeof(double) * c->jt_anchor.size());
  if (kind) std::memcpy(kind, c->jt_kind.data(), sizeof(int) * c->jt_kind.size());
  for (int j = 0; j < c->jt_n; ++j) {
    if (axis) std::copy(c->jt_ang.begin() + 7 * (size_t)j, c->jt_ang.begin() + 7 * (size_t)j + 3, axis + 3 * (size_t)j);
    if (q_rel) std::copy(c->jt_ang.begin() + 7 * (size_t)j + 3, c->jt_ang.begin() + 7 * (size_t)j + 7, q_rel + 4 * (size_t)j);
  }
  if (theta) std::memcpy(theta, c->jt_theta.data(), sizeof(double) * c->jt_theta.size());
  if (rate) std::memcpy(rate, c->jt_rate.data(), sizeof(double) * c->jt_rate.size());
  return RBL_OK;
}

// the motors' rates: context state, read by rbl_step_jointed; nothing is stored unless every value passes
int rbl_set_joint_rates(rbl_ctx *c, const double *rate)
{
  if (!c) return RBL_ERR_ARG;
  if (c->jt_n < 1) return rbl_fail(c, RBL_ERR_STATE, "set_joint_rates: no joints have been set (rbl_set_joint_kinds)");
  if (!rate) return rbl_fail(c, RBL_ERR_ARG, "set_joint_rates: rate must not be NULL");
  for (int j = 0; j < c->jt_n; ++j) {
    const std::string at = "set_joint_rates: joint " + std::to_string(j) + ": ";
    if (!std::isfinite(rate[j])) return rbl_fail(c, RBL_ERR_ARG, at + "the rate must be finite");
    if (rate[j] != 0.0 && c->jt_kind[j] != JT_LOCK)
      return rbl_fail(c, RBL_ERR_ARG, at + "only a lock joint (RBL_JOINT_LOCK) takes a rate; it must be 0 here");
  }
  if (std::memcmp(c->jt_rate.data(), rate, sizeof(double) * (size_t)c->jt_n) == 0) return RBL_OK;
  c->jt_rate.assign(rate, rate + c->jt_n);
  c->jt_valid = false;
  return RBL_OK;
}

int rbl_solve_jointed(rbl_ctx *c, const double *F_body, const double *slip, const double *joint_rhs, int max_iter, double rtol,
                      double *lambda, double *U, double *phi, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (!F_body) return rbl_fail(c, RBL_ERR_ARG, "solve_jointed: F_body is NULL");
  int rc = jt_check(c, "solve_jointed", max_iter, rtol); if (rc) return rc;
  if ((rc = need_K(c))) return rc;
  if (jt_active(c) && (rc = jt_range(c, "solve_jointed"))) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!jt_active(c)) return jt_plain_solve(c, RblSide::Host, F_body, slip, max_iter, rtol, lambda, U, iters, resid);
  if ((rc = jt_solve_core(c, "solve_jointed", RblSide::Host, F_body, slip, joint_rhs, max_iter, rtol, lambda, U, phi, iters, resid))) return rc;
  return finish_and_check(c);
}

int rbl_solve_jointed_dev(rbl_ctx *c, const double *d_F_body, const double *d_slip, const double *d_joint_rhs, int max_iter, double rtol,
                          double *d_lambda, double *d_U, double *d_phi, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (!d_F_body || !d_U) return rbl_fail(c, RBL_ERR_ARG, "solve_jointed_dev: F_body or U is NULL");
  int rc = jt_check(c, "solve_jointed_dev", max_iter, rtol); if (rc) return rc;
  if ((rc = need_config(c))) return rc;
  if (jt_active(c) && (rc = jt_range(c, "solve_jointed_dev"))) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!jt_active(c)) return jt_plain_solve(c, RblSide::Device, d_F_body, d_slip, max_iter, rtol, d_lambda, d_U, iters, resid);
  if (!d_phi) return rbl_fail(c, RBL_ERR_ARG, "solve_jointed_dev: phi is NULL");
  return jt_solve_core(c, "solve_jointed_dev", RblSide::Device, d_F_body, d_slip, d_joint_rhs, max_iter, rtol, d_lambda, d_U, d_phi, iters,
                       resid);
}

// One deterministic time step with hard joints: the force model's loads and the flow model's slip at q^n as in
// rbl_step_deterministic, c = -(gamma / dt) g(q^n) + joint_velocity, the jointed solve, evolve_X_Q(U)
int rbl_step_jointed(rbl_ctx *c, const double *F_body, const double *slip, const double *joint_velocity, double gamma, int max_iter,
                     double rtol, double *phi, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  if (!F_body) return rbl_fail(c, RBL_ERR_ARG, "step_jointed: F_body is NULL");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return rbl_fail(c, RBL_ERR_ARG, "step_jointed: gamma must lie in [0, 1]");
  int rc = jt_check(c, "step_jointed", max_iter, rtol); if (rc) return rc;
  if ((rc = need_K(c))) return rc;
  if (jt_active(c) && (rc = jt_range(c, "step_jointed"))) return rc;
  if (!jt_active(c)) {                                   // the plain step, cold start; its history does not carry over either
    rc = rbl_step_deterministic(c, F_body, slip, max_iter, rtol, 0, iters, resid);
    c->step_hist_n = 0;
    return rc;
  }
  if (!(c->S.dt > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "step_jointed: dt must be positive");
  if ((rc = step_begin(c))) return rc;
  const RblSizes z = sizes_of(c);
  const size_t nj3 = 3 * (size_t)c->jt_n;
  JtBuf B;
  if ((rc = jt_reserve(c, B))) return rc;
  if ((rc = jt_geom(c, B.lev, B.gap, B.gau))) return rc;
  if ((rc = step_inputs(c, F_body, slip, B.v, B.rhs))) return rc;       // the models at q^n as in rbl_step_deterministic, bonds included
  if (joint_velocity && (rc = copy_h2d(c, B.t, joint_velocity, sizeof(double) * nj3))) return rc;
  if (c->jt_angular)
    hipLaunchKernelGGL(k_jt_step_rhs_kinds, dim3((unsigned)((nj3 + 255) / 256)), dim3(256), 0, c->stream, (const double *)B.gap,
                       joint_velocity ? (const double *)B.t : nullptr, -gamma / c->S.dt, (int)nj3, jt_args(c), (const double *)B.lev, B.c);
  else
    hipLaunchKernelGGL(k_jt_step_rhs, dim3((unsigned)((nj3 + 255) / 256)), dim3(256), 0, c->stream, (const double *)B.gap,
                       joint_velocity ? (const double *)B.t : nullptr, -gamma / c->S.dt, (int)nj3, B.c);
  if ((rc = jt_rhs(c, B, B.v, true, B.c))) return rc;
  c->step_hist_n = 0;                                    // the warm starts of rbl_step_deterministic extrapolate over ITS steps only
  if ((rc = jt_solve(c, "step_jointed", B, max_iter, rtol, iters, resid))) return rc;
  std::vector<double> U(z.nb6);
  if ((rc = step_commit(c, B.x, B.x + z.n3, U.data(), B.x + z.nsys, phi, nj3, true))) return rc;   // moments: lever arms of q^n
  if ((rc = rbl_evolve_X_Q(c, U.data()))) return rc;
  // the step is accepted: every motor's angle advances, theta_j += rate_j dt (product and sum rounded one after the other)
  bool moved = false;
  for (int j = 0; j < c->jt_n && c->jt_angular; ++j)
    if (c->jt_rate[j] != 0.0) {
      volatile double d = c->jt_rate[j] * c->S.dt;
      c->jt_theta[j] += d;
      moved = true;
    }
  if (moved) c->jt_valid = false;
  return RBL_OK;
}

// the gaps g_j = p_A - p_B of the stored joints (on or off) at the context's configuration and the phi of the last jointed solve
// or step with this joint set; host arrays of 3 n_joints, either may be NULL
int rbl_joint_state(rbl_ctx *c, double *gap, double *phi)
{
  if (!c) return RBL_ERR_ARG;
  int rc = need_config(c); if (rc) return rc;
  if (c->jt_n < 1) return rbl_fail(c, RBL_ERR_STATE, "joint_state: no joints have been set (rbl_set_joints)");
  if (phi && !c->jt_phi_valid)
    return rbl_fail(c, RBL_ERR_STATE, "joint_state: no jointed solve or step has succeeded with this joint set");
  if ((rc = jt_range(c, "joint_state"))) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const size_t nj3 = 3 * (size_t)c->jt_n;
  if ((rc = rbl_dev_reserve(c, c->d_jtphi, sizeof(double) * 4 * nj3))) return rc;
  double *d_phi = (double *)c->d_jtphi.p, *d_gap = d_phi + nj3, *d_lev = d_gap + nj3;
  if (gap) {
    if ((rc = jt_geom(c, d_lev, d_gap, nullptr))) return rc;
    if ((rc = copy_d2h(c, gap, d_gap, sizeof(double) * nj3))) return rc;
  }
  if (phi && (rc = copy_d2h(c, phi, d_phi, sizeof(double) * nj3))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

// the same with the motor angles: gap rows of an angular joint hold e (P e for an axis joint); theta[n_joints] may be NULL
int rbl_joint_state_kinds(rbl_ctx *c, double *gap, double *phi, double *theta)
{
  const int rc = rbl_joint_state(c, gap, phi);
  if (rc) return rc;
  if (theta) std::memcpy(theta, c->jt_theta.data(), sizeof(double) * c->jt_theta.size());
  return RBL_OK;
}
