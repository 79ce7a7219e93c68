// rbl_mixed.hip -- prescribed kinematics (include/rbl.h section 7): any subset of the bodies moves as told, the others stay free;
// one GMRES solve of the saddle system's size returns the blob forces, the free velocities and the loads the prescribed bodies need.
// Shared internals are declared in rbl_api_internal.hpp.  Nothing here falls back to a CPU path.
//
// The system:  A x = [M lambda - K (D_f U) ; D_f K^T lambda + D_p U] = [slip + K_p U_p ; -F_f on free bodies, 0 on prescribed ones]
// (D_f, D_p: diagonal 0/1 on a body's six lab-frame velocity components.  The mask has one entry per body, or six in the _dof entry
// points: one kernel family serves both, a whole-body mask being the component mask with none or all six of a body's bits set; the
// body-row solves of a component mask go through 6 x 6 factors masked once per solve).  The body slots that are prescribed carry the
// identity, start at 0 and stay 0 through every Krylov vector, so |rhs| is the norm of the physical right-hand side alone.  The
// mobility product is the library's own (apply_M_enqueue, untouched); what is new around it -- the masked K / K^T tail, the masked
// preconditioner tails, the right-hand side and the split of the solution -- are the O(N) kernels below: one workgroup per body, the
// mask read once per workgroup (the branch on it is uniform), deterministic LDS tree sums, no atomics; the K / K^T formulas, the
// mask decoding (mx_bits), the workgroup sum and the 6 x 6 substitution are rbl_body_dev.hpp's, shared with rbl_body_dev.hip.  The Arnoldi recurrence, the
// Hessenberg solve and the convergence test are gmres_core's (gmres_core_with_ops).
//
// Many right-hand sides under ONE mask (the _multi entry points) advance in lock step through gmres_multi_with_ops: the same kernels
// with the column on the grid's second axis -- one workgroup per (body, column), the vectors of a batch `pitch` doubles apart, a bit
// set `live` of the columns still iterating (a converged column's workgroups return at once).  One vector is a grid of height 1 with
// pitch 0 and live = 1: the arithmetic per vector is the same either way.
//
// The Brownian midpoint step with prescribed bodies has its entry points here and nothing of the scheme: right-hand side, predictor
// and the sequence of the step are rbl_steps.hip's (rhs_and_midpoint_core, step_midpoint), which the all-free step goes through with
// no mask; this file hands them the mask and mx_solve.  With a mask per velocity component (the _dof forms of the three entry
// points) the mask must make the free components a subset of the coordinates: rbl_bd_mask6_check.
#include <cstring>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"

namespace {

constexpr int MT = 256;

// the workgroup's column of a lock-step batch; false: that column has converged, nothing to do
__device__ __forceinline__ bool mx_live(unsigned live, int &col)
{
  col = (int)blockIdx.y;
  return (live >> col) & 1u;
}

// a fully prescribed body (pm == 63) in the operator and the preconditioners: lambda_b = v_b, the six body slots pass through
__device__ __forceinline__ void mx_pass_through(const double *__restrict__ v, const double *g, int b, int t, int N_blb, long n3,
                                                double *__restrict__ out)
{
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
    out[idx] = v[idx]; out[idx + 1] = v[idx + 1]; out[idx + 2] = v[idx + 2];
  }
  if (t < 6) out[n3 + 6 * (size_t)b + t] = g[t];
}

// right-hand side: top = slip + K D_p U_in, bottom = -F_in on the free components, 0 on the prescribed ones
__global__ __launch_bounds__(MT) void k_mx_rhs(const double *__restrict__ lever, const uint8_t *__restrict__ mask, int per,
                                               const double *__restrict__ body_in, const double *__restrict__ slip, int N_blb,
                                               long n3, double *__restrict__ rhs, long pb, long ps, long pr)
{
  const int b = blockIdx.x, t = threadIdx.x;
  const size_t col = blockIdx.y;                         // column: body_in pb, slip ps, rhs pr doubles apart
  body_in += col * (size_t)pb; rhs += col * (size_t)pr;
  if (slip) slip += col * (size_t)ps;
  const unsigned pm = mx_bits(mask, per, b);
  const double *u = body_in + 6 * (size_t)b;
  double up[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) up[c] = (pm >> c & 1u) ? u[c] : 0.0;
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
    double r0 = slip ? slip[idx] : 0.0, r1 = slip ? slip[idx + 1] : 0.0, r2 = slip ? slip[idx + 2] : 0.0;
    if (pm) {
      double k0, k1, k2;
      rbl_KU(lever + idx, up, k0, k1, k2);
      r0 += k0; r1 += k1; r2 += k2;
    }
    rhs[idx] = r0; rhs[idx + 1] = r1; rhs[idx + 2] = r2;
  }
  if (t < 6) rhs[n3 + 6 * (size_t)b + t] = (pm >> t & 1u) ? 0.0 : -u[t];
}

// the operator's tail after sub = M lambda: out = [sub - K (D_f U) ; D_f K^T lambda + D_p U]
__global__ __launch_bounds__(MT) void k_mx_op_tail(const double *__restrict__ lever, const uint8_t *__restrict__ mask, int per,
                                                   const double *__restrict__ x, const double *__restrict__ sub, int N_blb, long n3,
                                                   double *__restrict__ out, long pitch, long spitch, unsigned live)
{
  __shared__ double s[6][MT];
  const int b = blockIdx.x, t = threadIdx.x;
  int col;
  if (!mx_live(live, col)) return;
  x += (size_t)col * (size_t)pitch; out += (size_t)col * (size_t)pitch; sub += (size_t)col * (size_t)spitch;
  const unsigned pm = mx_bits(mask, per, b);
  const double *u = x + n3 + 6 * (size_t)b;
  if (pm == 63u) { mx_pass_through(sub, u, b, t, N_blb, n3, out); return; }      // no velocity unknown, no balance row
  double uf[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) uf[c] = (pm >> c & 1u) ? 0.0 : u[c];
  double f[6] = {0, 0, 0, 0, 0, 0};
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
    const double *l = lever + idx;
    double k0, k1, k2;
    rbl_KU(l, uf, k0, k1, k2);
    out[idx] = sub[idx] - k0; out[idx + 1] = sub[idx + 1] - k1; out[idx + 2] = sub[idx + 2] - k2;
    rbl_KT_acc(l, x[idx], x[idx + 1], x[idx + 2], f);
  }
  rbl_block_sum<6, MT>(f, s, t);
  if (t < 6) {
    double ft = f[0];
#pragma unroll
    for (int c = 1; c < 6; ++c) ft = t == c ? f[c] : ft;   // (selects: a register array indexed by the lane goes to scratch here)
    out[n3 + 6 * (size_t)b + t] = (pm >> t & 1u) ? u[t] : ft;
  }
}

// The masked 6 x 6 factors of a solve with a mask per component, once per solve, one thread per body: R_b = L L^T from the context's
// factor (NL: per body, or with `Q` the ONE body-frame factor of the free-space tables, taken to the lab frame first: R_lab =
// (I2 x Rot) R_body (I2 x Rot)^T), rows and columns of the prescribed components replaced by the identity's, factored again -- a
// principal submatrix's Cholesky factor is not a sub-block of NL.  A body with no bit set copies its own factor (Q NULL); with the
// shared factor nothing is written for it, as no tail reads it there (the body-frame preconditioner's answer stands).  Not positive
// definite: the flag k_pc_block_ninv latches.  Whole-body masks need none of this: a free body's factor is the context's own, a
// prescribed body reads none.
__global__ void k_mx_factors(const double *__restrict__ NL, const double *__restrict__ Q, const uint8_t *__restrict__ mask6, int N_bod,
                             double *__restrict__ NLm, unsigned *err)
{
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= N_bod) return;
  unsigned pm = 0;
  for (int c = 0; c < 6; ++c) pm |= (mask6[6 * (size_t)b + c] != 0 ? 1u : 0u) << c;
  const double *L0 = Q ? NL : NL + 36 * (size_t)b;
  double *Lo = NLm + 36 * (size_t)b;
  if (pm == 0) {
    if (!Q)
      for (int e = 0; e < 36; ++e) Lo[e] = L0[e];
    return;
  }
  double A[36], L[36];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      double v = 0.0;
      for (int k = 0; k <= j; ++k) v += L0[6 * i + k] * L0[6 * j + k];
      A[6 * i + j] = v; A[6 * j + i] = v;
    }
  if (Q) {
    double R[9], T[9];
    quat_rot(Q + 4 * (size_t)b, R);
    for (int hi = 0; hi < 2; ++hi)
      for (int hj = 0; hj <= hi; ++hj) {                 // block (hi, hj): R A R^T; the upper block is the lower one's transpose
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += R[3 * i + k] * A[6 * (3 * hi + k) + 3 * hj + j];
            T[3 * i + j] = v;
          }
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += T[3 * i + k] * R[3 * j + k];
            L[6 * (3 * hi + i) + 3 * hj + j] = v;
          }
      }
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j <= i; ++j) {
        // the diagonal blocks are symmetric up to rounding: the lower triangle is what the factorisation reads
        A[6 * i + j] = L[6 * i + j];
      }
  }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      const bool cut = ((pm >> i) | (pm >> j)) & 1u;
      L[6 * i + j] = cut ? (i == j ? 1.0 : 0.0) : A[6 * i + j];
    }
  bool ok = true;
  for (int j = 0; j < 6; ++j) {
    double d = L[6 * j + j];
    for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
    if (!(d > 0.0)) ok = false;
    d = sqrt(d);
    L[6 * j + j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double v = L[6 * i + j];
      for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = v / d;
    }
    for (int i = 0; i < j; ++i) L[6 * i + j] = 0.0;
  }
  if (!ok) atomicOr(err, (unsigned)RBL_FLAG_NOT_SPD);
  for (int e = 0; e < 36; ++e) Lo[e] = L[e];
}

// the six body rows of a preconditioner application from f = K_b^T y1 and the masked factor: (D_f R_b D_f + D_p) u = D_f (g - f) +
// D_p g; the body slots take u (a prescribed slot: g, passed through), uf = D_f u goes on into lambda
__device__ __forceinline__ void mx_body_rows(const double *NLm_b, unsigned pm, const double *g, const double (&f)[6], double *out_b, double *uf)
{
  double r[6], u[6];
  for (int p = 0; p < 6; ++p) r[p] = (pm >> p & 1u) ? g[p] : g[p] - f[p];
  rbl_chol6_solve(NLm_b, r, u);
  for (int p = 0; p < 6; ++p) {
    const bool pres = pm >> p & 1u;
    out_b[p] = pres ? g[p] : u[p];
    uf[p] = pres ? 0.0 : u[p];
  }
}

// block preconditioner after y1 = invM slip (ONE pass over the per-body factors, all bodies).  A body with a free component: what
// k_pc_block_tail does with the force block's sign restored and the masked factor -- f = K^T y1, the body rows of mx_body_rows,
// lambda = y1 + (invM K) D_f u, the exact inverse of [M_b -K_b D_f; D_f K_b^T D_p] on [slip_b; g_b].  Fully prescribed body:
// lambda = y1, the six body slots pass through.  NLm: the masked factors, or with a whole-body mask the context's own.
__global__ __launch_bounds__(MT) void k_mx_pc_block_tail(const double *__restrict__ lever, const uint8_t *__restrict__ mask, int per,
                                                         const double *__restrict__ y1, const double *__restrict__ MK, long stride,
                                                         const double *__restrict__ NLm, const double *__restrict__ in, int N_blb,
                                                         long n3, double *__restrict__ out, long pitch, unsigned live)
{
  __shared__ double s[6][MT];
  __shared__ double us[6];
  const int b = blockIdx.x, t = threadIdx.x;
  int col;
  if (!mx_live(live, col)) return;
  y1 += (size_t)col * (size_t)pitch; in += (size_t)col * (size_t)pitch; out += (size_t)col * (size_t)pitch;
  const unsigned pm = mx_bits(mask, per, b);
  const double *g = in + n3 + 6 * (size_t)b;
  if (pm == 63u) { mx_pass_through(y1, g, b, t, N_blb, n3, out); return; }
  double f[6] = {0, 0, 0, 0, 0, 0};
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
    rbl_KT_acc(lever + idx, y1[idx], y1[idx + 1], y1[idx + 2], f);
  }
  rbl_block_sum<6, MT>(f, s, t);
  if (t == 0) mx_body_rows(NLm + 36 * (size_t)b, pm, g, f, out + n3 + 6 * (size_t)b, us);
  __syncthreads();
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      double acc = y1[idx + d];
#pragma unroll
      for (int c = 0; c < 6; ++c) acc = __builtin_fma(MK[(size_t)c * stride + idx + d], us[c], acc);
      out[idx + d] = acc;
    }
  }
}

// diagonal preconditioner (invM2: the self-block scaling per blob, x/y and z).  A body with a free component: k_pc_diag_apply with
// the force block's sign restored and the masked factor, lambda = invM (slip + K D_f u); fully prescribed body: lambda = invM slip,
// the six body slots pass through.  NLm as in k_mx_pc_block_tail.
__global__ __launch_bounds__(MT) void k_mx_pc_diag(const double *__restrict__ lever, const uint8_t *__restrict__ mask, int per,
                                                   const double *__restrict__ invM2, const double *__restrict__ NLm, int N_blb, long n3,
                                                   const double *__restrict__ in, double *__restrict__ out, long pitch, unsigned live)
{
  __shared__ double s[6][MT];
  __shared__ double us[6];
  const int b = blockIdx.x, t = threadIdx.x;
  int col;
  if (!mx_live(live, col)) return;
  in += (size_t)col * (size_t)pitch; out += (size_t)col * (size_t)pitch;
  const unsigned pm = mx_bits(mask, per, b);
  const double *g = in + n3 + 6 * (size_t)b;
  if (pm == 63u) {
    for (int k = t; k < N_blb; k += MT) {
      const size_t i = (size_t)b * N_blb + k;
      out[3 * i] = invM2[2 * i] * in[3 * i]; out[3 * i + 1] = invM2[2 * i] * in[3 * i + 1];
      out[3 * i + 2] = invM2[2 * i + 1] * in[3 * i + 2];
    }
    if (t < 6) out[n3 + 6 * (size_t)b + t] = g[t];
    return;
  }
  double f[6] = {0, 0, 0, 0, 0, 0};
  for (int k = t; k < N_blb; k += MT) {                  // K^T (invM slip)
    const size_t i = (size_t)b * N_blb + k;
    rbl_KT_acc(lever + 3 * i, invM2[2 * i] * in[3 * i], invM2[2 * i] * in[3 * i + 1], invM2[2 * i + 1] * in[3 * i + 2], f);
  }
  rbl_block_sum<6, MT>(f, s, t);
  if (t == 0) mx_body_rows(NLm + 36 * (size_t)b, pm, g, f, out + n3 + 6 * (size_t)b, us);
  __syncthreads();
  for (int k = t; k < N_blb; k += MT) {                  // lambda = invM (slip + K D_f u)
    const size_t i = (size_t)b * N_blb + k;
    double k0, k1, k2;
    rbl_KU(lever + 3 * i, us, k0, k1, k2);
    out[3 * i] = invM2[2 * i] * (in[3 * i] + k0);
    out[3 * i + 1] = invM2[2 * i] * (in[3 * i + 1] + k1);
    out[3 * i + 2] = invM2[2 * i + 1] * (in[3 * i + 2] + k2);
  }
}

// free-space body-frame tables: `out` holds the ordinary preconditioner's answer for every body, which stands for a body with no
// bit set; a fully prescribed body takes lambda = y1 = M_b^-1 slip_b (a second factor application, lab frame) and its six body
// slots from the input; a partly prescribed one is redone from y1 with the masked lab-frame factor.
// The table MKb = M_body^-1 K_body ([6][3 N_blb], one for all bodies) is in the body frame: M_b^-1 K_b D_f u = Rot MKb (I2 x Rot)^T D_f u.
// Only a partial mask reads lever, MKb, Q and NLm: with a whole-body mask (per == 1) Q and NLm are NULL.
__global__ __launch_bounds__(MT) void k_mx_pc_bodyframe_tail(const double *__restrict__ lever, const uint8_t *__restrict__ mask, int per,
                                                             const double *__restrict__ y1, const double *__restrict__ MKb,
                                                             const double *__restrict__ Q, const double *__restrict__ NLm,
                                                             const double *__restrict__ in, int N_blb, long n3, double *__restrict__ out,
                                                             long pitch, unsigned live)
{
  __shared__ double s[6][MT];
  __shared__ double us[6];
  const int b = blockIdx.x, t = threadIdx.x;
  int col;
  if (!mx_live(live, col)) return;
  y1 += (size_t)col * (size_t)pitch; in += (size_t)col * (size_t)pitch; out += (size_t)col * (size_t)pitch;
  const unsigned pm = mx_bits(mask, per, b);
  if (pm == 0u) return;
  const double *g = in + n3 + 6 * (size_t)b;
  if (pm == 63u) { mx_pass_through(y1, g, b, t, N_blb, n3, out); return; }
  double R[9];
  quat_rot(Q + 4 * (size_t)b, R);
  double f[6] = {0, 0, 0, 0, 0, 0};
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
    rbl_KT_acc(lever + idx, y1[idx], y1[idx + 1], y1[idx + 2], f);
  }
  rbl_block_sum<6, MT>(f, s, t);
  if (t == 0) {
    double uf[6];
    mx_body_rows(NLm + 36 * (size_t)b, pm, g, f, out + n3 + 6 * (size_t)b, uf);
    for (int h = 0; h < 2; ++h)                          // (I2 x Rot)^T D_f u
      for (int d = 0; d < 3; ++d) us[3 * h + d] = R[d] * uf[3 * h] + R[3 + d] * uf[3 * h + 1] + R[6 + d] * uf[3 * h + 2];
  }
  __syncthreads();
  const long n = 3L * N_blb;
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
    double w[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc = __builtin_fma(MKb[(size_t)c * n + 3 * k + d], us[c], acc);
      w[d] = acc;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) out[idx + d] = y1[idx + d] + (R[3 * d] * w[0] + R[3 * d + 1] * w[1] + R[3 * d + 2] * w[2]);
  }
}

// v += add on the free components (the force model's loads enter the free components only)
__global__ void k_mx_add_free(const uint8_t *__restrict__ mask, int per, const double *__restrict__ add, int nb6, double *__restrict__ v)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb6 && !mask[per == 6 ? i : i / 6]) v[i] += add[i];
}

// the solution split: U = D_f U_solved + D_p U_in (echoed), F = D_f F_in (echoed) + D_p (-K_b^T lambda)
__global__ __launch_bounds__(MT) void k_mx_split(const double *__restrict__ lever, const uint8_t *__restrict__ mask, int per,
                                                 const double *__restrict__ body_in, const double *__restrict__ x, int N_blb, long n3,
                                                 double *__restrict__ U, double *__restrict__ F, long pb, long px)
{
  __shared__ double s[6][MT];
  const int b = blockIdx.x, t = threadIdx.x;
  const size_t col = blockIdx.y;                         // column: body_in, U and F pb, x px doubles apart
  body_in += col * (size_t)pb; U += col * (size_t)pb; F += col * (size_t)pb; x += col * (size_t)px;
  const unsigned pm = mx_bits(mask, per, b);
  const size_t o = 6 * (size_t)b;
  if (pm == 0u) {
    if (t < 6) { U[o + t] = x[n3 + o + t]; F[o + t] = body_in[o + t]; }
    return;
  }
  double f[6] = {0, 0, 0, 0, 0, 0};
  for (int k = t; k < N_blb; k += MT) {
    const size_t idx = 3 * ((size_t)b * N_blb + k);
    rbl_KT_acc(lever + idx, x[idx], x[idx + 1], x[idx + 2], f);
  }
  rbl_block_sum<6, MT>(f, s, t);
  if (t < 6) {
    const bool pres = pm >> t & 1u;
    U[o + t] = pres ? body_in[o + t] : x[n3 + o + t];
    F[o + t] = pres ? -f[t] : body_in[o + t];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------

struct MxBuf {           // the one workspace of a section 7 entry point (rbl_ctx::d_mx)
  double *rhs, *x, *y1, *body_in, *slip, *U, *F, *model;
  double *NLm;           // the masked 6 x 6 factors of a solve with a mask per component (k_mx_factors); NULL with per == 1
  uint8_t *mask;         // per * N_bod entries
  int per = 1;           // mask entries per body: 1 (whole bodies) or 6 (velocity components, the _dof entry points)
  int k = 1;             // columns: rhs, x, slip, body_in, U and F hold k vectors one after the other (the _multi entry points: <= 16)
};

int mx_reserve(rbl_ctx *c, MxBuf &B)
{
  const size_t nb6 = sizes_of(c).nb6, n3 = sizes_of(c).n3, nsys = n3 + nb6;
  const size_t nlm = B.per == 6 ? 6 * nb6 : 0;           // the masked factors: solves with a mask per component only
  const size_t k = (size_t)B.k;                          // (y1, model, the factors and the mask are shared by the columns)
  const int rc = rbl_dev_reserve(c, c->d_mx, sizeof(double) * (k * (2 * nsys + n3 + 3 * nb6) + n3 + nb6 + nlm) + (size_t)B.per * (size_t)c->S.N_bod);
  if (rc) return rc;
  B.rhs = (double *)c->d_mx.p; B.x = B.rhs + k * nsys; B.y1 = B.x + k * nsys; B.slip = B.y1 + n3; B.body_in = B.slip + k * n3;
  B.U = B.body_in + k * nb6; B.F = B.U + k * nb6; B.model = B.F + k * nb6; B.NLm = nlm ? B.model + nb6 : nullptr;
  B.mask = (uint8_t *)(B.model + nb6 + nlm);
  return RBL_OK;
}

struct MxSolve {
  const MxBuf *B;
  bool any_prescribed;
};

int mx_op(rbl_ctx *c, void *user, const double *d_x, double *d_out)
{
  const MxSolve *m = (const MxSolve *)user;
  const RblBodyState &S = c->S;
  const int64_t N = (int64_t)sizes_of(c).N, n3 = 3 * N;
  int rc = rbl_dev_reserve(c, c->d_sad, sizeof(double) * (size_t)n3); if (rc) return rc;
  if ((rc = apply_M_enqueue(c, S.wall, d_x, (const double *)c->d_pos.p, N, 0, N, (double *)c->d_sad.p))) return rc;
  hipLaunchKernelGGL(k_mx_op_tail, dim3((unsigned)S.N_bod), dim3(MT), 0, c->stream, (const double *)c->d_lever.p,
                     (const uint8_t *)m->B->mask, m->B->per, d_x, (const double *)c->d_sad.p, S.N_blb, (long)n3, d_out, 0L, 0L, 1u);
  return RBL_OK;
}

// k columns `pitch` doubles apart: ONE multi-vector product (the fp64 matrix cores from 4 columns on), ONE masked tail for the live ones
int mx_op_multi(rbl_ctx *c, void *user, const double *d_x, double *d_out, int k, int64_t pitch, unsigned live)
{
  const MxSolve *m = (const MxSolve *)user;
  const RblBodyState &S = c->S;
  const int64_t N = (int64_t)sizes_of(c).N, n3 = 3 * N;
  int rc = rbl_dev_reserve(c, c->d_sad, sizeof(double) * (size_t)n3 * (size_t)k); if (rc) return rc;
  if ((rc = apply_M_multi_enqueue(c, S.wall, d_x, (const double *)c->d_pos.p, N, k, (double *)c->d_sad.p, pitch, n3))) return rc;
  hipLaunchKernelGGL(k_mx_op_tail, dim3((unsigned)S.N_bod, (unsigned)k), dim3(MT), 0, c->stream, (const double *)c->d_lever.p,
                     (const uint8_t *)m->B->mask, m->B->per, d_x, (const double *)c->d_sad.p, S.N_blb, (long)n3, d_out, (long)pitch, (long)n3,
                     live);
  return RBL_OK;
}

// the tables of the free-space body-frame preconditioner (bf_build: M_body^-1 | M_body^-1 K_body | the 6 x 6 factor)
const double *bf_table_MK(const rbl_ctx *c)
{
  const size_t m = 3 * (size_t)c->S.N_blb;
  return (const double *)c->d_bfPC.p + m * m;
}

// the masked preconditioner on k vectors `pitch` doubles apart (one vector: k = 1, pitch 0, live = 1); y1: room for invM slip of
// every vector, `pitch` apart too.  The per-body factor passes take all k vectors at once (three share a pass); a converged
// column rides along there on its zeroed slot and is skipped by the tails
int mx_pc_cols(rbl_ctx *c, const MxSolve *m, const double *d_in, double *d_out, double *y1, int k, int64_t pitch, unsigned live)
{
  const RblBodyState &S = c->S;
  const long n3 = (long)sizes_of(c).n3;
  const double *lev = (const double *)c->d_lever.p;
  const dim3 grid((unsigned)S.N_bod, (unsigned)k), block(MT);
  const int per = m->B->per;
  const uint8_t *mask = m->B->mask;
  // the 6 x 6 factors of the tails: masked once per solve for a mask per component; whole bodies read the context's own (a free
  // body) or none (a prescribed one)
  const double *NL = per == 6 ? (const double *)m->B->NLm : (const double *)c->d_NL.p;
  int rc;
  if (!S.block_pc) {
    hipLaunchKernelGGL(k_mx_pc_diag, grid, block, 0, c->stream, lev, mask, per, (const double *)c->d_invM2.p, NL, S.N_blb, n3, d_in, d_out,
                       (long)pitch, live);
    return RBL_OK;
  }
  if (bf_on(c) && c->bf_tables) {
    // free space, small bodies: the one-launch body-frame preconditioner serves the free bodies as it is; the prescribed ones cost
    // a second application of the shared factor.  Whole bodies: the tail reads neither the orientations nor a masked factor
    for (int col = 0; col < k; ++col) {
      if (!(live >> col & 1u)) continue;
      RblPcReq rq;
      rq.fsign = 1.0;
      if ((rc = apply_PC_dev(c, d_in + (size_t)col * (size_t)pitch, d_out + (size_t)col * (size_t)pitch, rq))) return rc;
    }
    if (!m->any_prescribed) return RBL_OK;
    if ((rc = blk_solve(c, 0, S.N_bod, d_in, y1, k, pitch, 0))) return rc;
    hipLaunchKernelGGL(k_mx_pc_bodyframe_tail, grid, block, 0, c->stream, lev, mask, per, (const double *)y1, bf_table_MK(c),
                       per == 6 ? (const double *)c->d_XQ.p + 3 * (size_t)S.N_bod : nullptr, (const double *)m->B->NLm, d_in, S.N_blb, n3,
                       d_out, (long)pitch, live);
    return RBL_OK;
  }
  if ((rc = blk_solve(c, 0, S.N_bod, d_in, y1, k, pitch, 0))) return rc;                     // invM slip, every body: ONE pass
  RblPhase ph(c, RBL_T_PERBODY);
  hipLaunchKernelGGL(k_mx_pc_block_tail, grid, block, 0, c->stream, lev, mask, per, (const double *)y1, (const double *)c->d_pcMK.p,
                     n3, NL, d_in, S.N_blb, n3, d_out, (long)pitch, live);
  return RBL_OK;
}

int mx_pc(rbl_ctx *c, void *user, const double *d_in, double *d_out)
{
  const MxSolve *m = (const MxSolve *)user;
  return mx_pc_cols(c, m, d_in, d_out, m->B->y1, 1, 0, 1u);
}

int mx_pc_multi(rbl_ctx *c, void *user, const double *d_in, double *d_out, double *d_scratch, int k, int64_t pitch, unsigned live)
{
  return mx_pc_cols(c, (const MxSolve *)user, d_in, d_out, d_scratch, k, pitch, live);
}

// argument checks that need no device
int mx_check(rbl_ctx *c, const char *who, const uint8_t *prescribed, const void *body_in, int max_iter, double rtol, bool host_form,
             int *n_prescribed, int per = 1, int nrhs = 1)
{
  if (!c) return RBL_ERR_ARG;
  if (!prescribed || !body_in) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": prescribed or body_in is NULL");
  if (nrhs < 1) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": need nrhs >= 1");
  if (max_iter < 1 || !(rtol >= 0.0)) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": need max_iter >= 1 and rtol >= 0");
  if (max_iter + 1 > rbl_gmres_max_vectors()) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": at most 255 iterations (no restart)");
  int rc = host_form ? need_K(c) : need_config(c); if (rc) return rc;
  int np = 0;
  for (size_t b = 0; b < (size_t)per * (size_t)c->S.N_bod; ++b) {
    if (prescribed[b] > 1) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": entries of prescribed must be 0 or 1");
    np += prescribed[b];
  }
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": not available on a context with a communicator");
  *n_prescribed = np;
  return RBL_OK;
}

// the solve on buffers of B (mask, body_in and slip in place): leaves x = [lambda ; U_f], B.U and B.F; nothing is read back
// beyond the solver's convergence tests
int mx_solve(rbl_ctx *c, const MxBuf &B, bool have_slip, int n_prescribed, int max_iter, double rtol, int *iters, double *resid)
{
  RblPhase ph_total(c, RBL_T_TOTAL);
  int rc = rbl_prepare_dev(c); if (rc) return rc;                        // resident geometry, the preconditioner of this configuration
  const RblBodyState &S = c->S;
  const long n3 = (long)sizes_of(c).n3;
  const double *lev = (const double *)c->d_lever.p;
  const dim3 grid((unsigned)S.N_bod), block(MT);
  hipLaunchKernelGGL(k_mx_rhs, grid, block, 0, c->stream, lev, (const uint8_t *)B.mask, B.per, (const double *)B.body_in,
                     have_slip ? (const double *)B.slip : nullptr, S.N_blb, n3, B.rhs, 0L, 0L, 0L);
  if (B.per == 6) {                                      // the masked 6 x 6 factors: once per solve (whole bodies need none: mx_pc)
    const bool shared = S.block_pc && bf_on(c) && c->bf_tables;          // one body-frame factor for all bodies, behind the tables
    if (shared && (rc = ensure_xq_dev(c))) return rc;
    hipLaunchKernelGGL(k_mx_factors, dim3((unsigned)((S.N_bod + 63) / 64)), dim3(64), 0, c->stream,
                       shared ? bf_table_MK(c) + 18 * (size_t)S.N_blb : (const double *)c->d_NL.p,
                       shared ? (const double *)c->d_XQ.p + 3 * (size_t)S.N_bod : nullptr, (const uint8_t *)B.mask, S.N_bod, B.NLm, c->d_err);
  }
  MxSolve m{&B, n_prescribed > 0};
  const RblSolveOps ops{mx_op, mx_pc, &m};
  if ((rc = gmres_core_with_ops(c, &ops, B.rhs, max_iter, rtol, B.x, iters, resid))) return rc;
  hipLaunchKernelGGL(k_mx_split, grid, block, 0, c->stream, lev, (const uint8_t *)B.mask, B.per, (const double *)B.body_in,
                     (const double *)B.x, S.N_blb, n3, B.U, B.F, 0L, 0L);
  RBL_HIP(c, hipGetLastError());
  return RBL_OK;
}

// what a _multi call does once, the mask (shared by all columns) in place: the resident geometry and the preconditioner of this
// configuration, the masked 6 x 6 factors
int mx_multi_prepare(rbl_ctx *c, const MxBuf &B)
{
  int rc = rbl_prepare_dev(c); if (rc) return rc;
  const RblBodyState &S = c->S;
  if (B.per == 6) {
    const bool shared = S.block_pc && bf_on(c) && c->bf_tables;
    if (shared && (rc = ensure_xq_dev(c))) return rc;
    hipLaunchKernelGGL(k_mx_factors, dim3((unsigned)((S.N_bod + 63) / 64)), dim3(64), 0, c->stream,
                       shared ? bf_table_MK(c) + 18 * (size_t)S.N_blb : (const double *)c->d_NL.p,
                       shared ? (const double *)c->d_XQ.p + 3 * (size_t)S.N_bod : nullptr, (const uint8_t *)B.mask, S.N_bod, B.NLm, c->d_err);
  }
  return RBL_OK;
}

// one batch of kb <= B.k columns in lock step on the buffers of B (body_in and slip of the batch in place): leaves x = [lambda ;
// U_f], B.U and B.F column by column
int mx_solve_batch(rbl_ctx *c, const MxBuf &B, bool have_slip, int n_prescribed, int kb, int max_iter, double rtol, int *iters, double *resid)
{
  const RblBodyState &S = c->S;
  const long nb6 = (long)sizes_of(c).nb6, n3 = (long)sizes_of(c).n3, nsys = n3 + nb6;
  const double *lev = (const double *)c->d_lever.p;
  const dim3 grid((unsigned)S.N_bod, (unsigned)kb), block(MT);
  hipLaunchKernelGGL(k_mx_rhs, grid, block, 0, c->stream, lev, (const uint8_t *)B.mask, B.per, (const double *)B.body_in,
                     have_slip ? (const double *)B.slip : nullptr, S.N_blb, n3, B.rhs, nb6, n3, nsys);
  MxSolve m{&B, n_prescribed > 0};
  const RblMultiOps ops{mx_op_multi, mx_pc_multi, &m};
  int rc;
  if ((rc = gmres_multi_with_ops(c, &ops, B.rhs, kb, max_iter, rtol, B.x, iters, resid))) return rc;
  hipLaunchKernelGGL(k_mx_split, grid, block, 0, c->stream, lev, (const uint8_t *)B.mask, B.per, (const double *)B.body_in,
                     (const double *)B.x, S.N_blb, n3, B.U, B.F, nb6, nsys);
  RBL_HIP(c, hipGetLastError());
  return RBL_OK;
}

// the host's mask into the workspace.  Host form: copy_h2d.  Device form: from the context's pinned buffer (idle between the
// solver's read-backs, which drain the stream): a true asynchronous copy, so the caller's array may go after the call and the
// stream is not drained for it
int mx_mask_in(rbl_ctx *c, RblSide side, const MxBuf &B, const uint8_t *prescribed)
{
  const size_t nmask = (size_t)B.per * (size_t)c->S.N_bod;
  if (side == RblSide::Host) return copy_h2d(c, B.mask, prescribed, nmask);
  void *pin;
  int rc = pin_buffer(c, nmask, &pin); if (rc) return rc;
  if (pin) std::memcpy(pin, prescribed, nmask);
  RBL_HIP(c, hipMemcpyAsync(B.mask, pin ? pin : prescribed, nmask, hipMemcpyHostToDevice, c->stream));
  if (!pin) RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

// the workspace with the host's mask (B.per entries per body) and the caller's body_in and slip (either side) in place; model: the
// force model's loads at the current configuration added to the free slots of body_in and the flow model's term added to the
// slip (the steps).  *have_slip: B.slip holds something (the caller's slip, the term, or their sum)
int mx_upload(rbl_ctx *c, RblSide side, MxBuf &B, const uint8_t *prescribed, const double *body_in, const double *slip, bool model, int np,
              bool *have_slip)
{
  const size_t nb6 = sizes_of(c).nb6;
  int rc = mx_reserve(c, B); if (rc) return rc;
  if ((rc = mx_mask_in(c, side, B, prescribed))) return rc;
  if ((rc = xfer_in(c, side, B.body_in, body_in, sizeof(double) * nb6))) return rc;
  if ((rc = step_slip(c, side, slip, B.slip, model, have_slip))) return rc;
  if (model && ia_any(c) && np < B.per * c->S.N_bod) {    // -K^T f_phys at q^n, free slots only (none free: nothing feels the model)
    RBL_HIP(c, hipMemsetAsync(B.model, 0, sizeof(double) * nb6, c->stream));
    if ((rc = ia_add_to_step_force(c, B.model))) return rc;
    hipLaunchKernelGGL(k_mx_add_free, dim3((unsigned)((nb6 + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)B.mask, B.per,
                       (const double *)B.model, (int)nb6, B.body_in);
  }
  return RBL_OK;
}

// One solve, the checks done and the device up: the caller's arrays (either side) in, the solve, lambda (may be NULL), U and F out.
// model (host arrays only): a step's solve -- the models at q^n go in, the moments are recorded, F may be NULL and lambda is not
// asked for.  The host form ends in a drain and a check of the latched flags; the device form drains where the solver drains
int mx_core(rbl_ctx *c, RblSide side, const uint8_t *prescribed, int np, const double *body_in, const double *slip, int max_iter,
            double rtol, bool model, double *lambda, double *U, double *F, int *iters, double *resid, int per)
{
  const RblSizes z = sizes_of(c);
  MxBuf B;
  B.per = per;
  bool have_slip;
  int rc = mx_upload(c, side, B, prescribed, body_in, slip, model, np, &have_slip); if (rc) return rc;
  if ((rc = mx_solve(c, B, have_slip, np, max_iter, rtol, iters, resid))) return rc;
  if (model) return step_commit(c, B.x, B.U, U, B.F, F, z.nb6, true);   // moments: lever arms of q^n
  if (lambda && (rc = xfer_out(c, side, lambda, B.x, sizeof(double) * z.n3))) return rc;
  if (U && (rc = xfer_out(c, side, U, B.U, sizeof(double) * z.nb6))) return rc;
  if (F && (rc = xfer_out(c, side, F, B.F, sizeof(double) * z.nb6))) return rc;
  return side == RblSide::Host ? finish_and_check(c) : RBL_OK;
}

// host arrays in, host arrays out; model: the step's solve (see mx_core)
int mx_host(rbl_ctx *c, const char *who, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
            bool model, double *lambda, double *U, double *F, int *iters, double *resid, int per = 1)
{
  int np = 0;
  int rc = mx_check(c, who, prescribed, body_in, max_iter, rtol, true, &np, per); if (rc) return rc;
  if ((rc = model ? step_begin(c) : rbl_dev_init(c))) return rc;
  return mx_core(c, RblSide::Host, prescribed, np, body_in, slip, max_iter, rtol, model, lambda, U, F, iters, resid, per);
}

// device arrays in, device arrays out, the mask (per entries per body) from the host
int mx_dev(rbl_ctx *c, const char *who, const uint8_t *prescribed, const double *d_body_in, const double *d_slip, int max_iter, double rtol,
           double *d_lambda, double *d_U, double *d_F, int *iters, double *resid, int per)
{
  if (c && (!d_U || !d_F)) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": U or F is NULL");
  int np = 0;
  int rc = mx_check(c, who, prescribed, d_body_in, max_iter, rtol, false, &np, per); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  return mx_core(c, RblSide::Device, prescribed, np, d_body_in, d_slip, max_iter, rtol, false, d_lambda, d_U, d_F, iters, resid, per);
}

// ---- nrhs right-hand sides under one mask, in lock step, 16 columns a batch (the workspace holds one batch) -------------------------
// body_in: nrhs vectors of 6 N_bod, slip: NULL or nrhs vectors of 3 N, one after the other; lambda (may be NULL), U, F likewise
int mx_multi(rbl_ctx *c, const char *who, RblSide side, const uint8_t *prescribed, int nrhs, const double *body_in, const double *slip,
             int max_iter, double rtol, double *lambda, double *U, double *F, int *iters, double *resid, int per)
{
  if (!c) return RBL_ERR_ARG;
  if (!U || !F) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": U or F is NULL");
  int np = 0;
  int rc = mx_check(c, who, prescribed, body_in, max_iter, rtol, side == RblSide::Host, &np, per, nrhs); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const RblSizes z = sizes_of(c);
  const size_t fb = sizeof(double) * z.nb6, vb = sizeof(double) * z.n3;
  MxBuf B;
  B.per = per;
  B.k = nrhs < 16 ? nrhs : 16;
  if ((rc = mx_reserve(c, B))) return rc;
  if ((rc = mx_mask_in(c, side, B, prescribed))) return rc;
  RblPhase ph_total(c, RBL_T_TOTAL);
  if ((rc = mx_multi_prepare(c, B))) return rc;
  for (int k0 = 0; k0 < nrhs; k0 += 16) {
    const size_t kb = nrhs - k0 < 16 ? nrhs - k0 : 16;
    if ((rc = xfer_in(c, side, B.body_in, body_in + (size_t)k0 * z.nb6, fb * kb))) return rc;
    if (slip && (rc = xfer_in(c, side, B.slip, slip + (size_t)k0 * z.n3, vb * kb))) return rc;
    if ((rc = mx_solve_batch(c, B, slip != nullptr, np, (int)kb, max_iter, rtol, iters ? iters + k0 : nullptr, resid ? resid + k0 : nullptr)))
      return rc;
    for (size_t col = 0; lambda && col < kb; ++col)
      if ((rc = xfer_out(c, side, lambda + ((size_t)k0 + col) * z.n3, B.x + col * z.nsys, vb))) return rc;
    if ((rc = xfer_out(c, side, U + (size_t)k0 * z.nb6, B.U, fb * kb))) return rc;
    if ((rc = xfer_out(c, side, F + (size_t)k0 * z.nb6, B.F, fb * kb))) return rc;
    if ((rc = finish_and_check(c))) return rc;           // the latched device flags, batch by batch
  }
  return RBL_OK;
}

int mx_step(rbl_ctx *c, const char *who, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
            double *F, int *iters, double *resid, int per = 1)
{
  std::vector<double> U((size_t)6 * (size_t)(c->S.N_bod > 0 ? c->S.N_bod : 1));
  const int rc = mx_host(c, who, prescribed, body_in, slip, max_iter, rtol, true, nullptr, U.data(), F, iters, resid, per);
  if (rc) return rc;
  c->step_hist_n = 0;                                    // the warm starts of rbl_step_deterministic extrapolate over ITS steps only
  return rbl_evolve_X_Q(c, U.data());
}

// ---- the Brownian midpoint step with prescribed bodies: the scheme is rbl_steps.hip's (rhs_and_midpoint_core, step_midpoint) ---------

// the checks of the two right-hand-side forms and of the step, none of which needs a device
int mx_bd_check(rbl_ctx *c, const char *who, const uint8_t *prescribed, const void *body_in, int max_iter, double rtol, double delta,
                int *n_prescribed, int per = 1)
{
  int rc = mx_check(c, who, prescribed, body_in, max_iter, rtol, true, n_prescribed, per); if (rc) return rc;
  if (per == 6 && (rc = rbl_bd_mask6_check(c, who, prescribed, 1, c->S.N_bod))) return rc;
  if (max_iter > 254) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": at most 254 iterations (no restart)");
  if (c->S.kBT > 1e-10 && (!(c->S.dt > 0.0) || !(delta > 0.0)))
    return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": dt and delta must be positive");
  return RBL_OK;
}

// right-hand side and predictor, device arrays in and out (who: the entry point's name; per: mask entries per body)
int mx_bd_rhs_dev(rbl_ctx *c, const char *who, const uint8_t *prescribed, int per, const double *d_body_in, const double *d_slip,
                  const double *d_W, uint64_t seed, int method, int split_rand, double delta, double *d_s, double *X_half, double *Q_half)
{
  if (c && (!d_s || !X_half || !Q_half)) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": s, X_half or Q_half is NULL");
  int np = 0;
  int rc = mx_bd_check(c, who, prescribed, d_body_in, 1, 0.0, delta, &np, per); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const uint8_t *d_mask = nullptr;
  if (c->S.kBT > 1e-10) {                                // without Brownian terms the mask is not read: no workspace for it
    MxBuf B;
    B.per = per;
    if ((rc = mx_reserve(c, B))) return rc;
    if ((rc = mx_mask_in(c, RblSide::Host, B, prescribed))) return rc;
    d_mask = B.mask;
  }
  return rhs_and_midpoint_core(c, prescribed, d_mask, d_body_in, d_slip, d_W, seed, method, split_rand, delta, d_s, X_half, Q_half, per);
}

// the same with host arrays (who: the host entry point's name; the refusals name it)
int mx_bd_rhs_host(rbl_ctx *c, const char *who, const uint8_t *prescribed, int per, const double *body_in, const double *slip,
                   const double *W, uint64_t seed, int method, int split_rand, double delta, double *s, double *X_half, double *Q_half)
{
  if (c && (!s || !X_half || !Q_half)) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": s, X_half or Q_half is NULL");
  int np = 0;
  int rc = mx_bd_check(c, who, prescribed, body_in, 1, 0.0, delta, &np, per); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const size_t nb6 = sizes_of(c).nb6, n3 = sizes_of(c).n3;
  const size_t vb = sizeof(double) * n3, fb = sizeof(double) * nb6;
  if ((rc = rbl_dev_reserve(c, c->d_bd2, (W ? 4 : 1) * vb + fb))) return rc;
  double *dS = (double *)c->d_bd2.p, *dBody = dS + n3, *dW = dBody + nb6;
  if (slip && (rc = copy_h2d(c, dS, slip, vb))) return rc;
  if ((rc = copy_h2d(c, dBody, body_in, fb))) return rc;
  if (W && (rc = copy_h2d(c, dW, W, 3 * vb))) return rc;
  if ((rc = mx_bd_rhs_dev(c, who, prescribed, per, dBody, slip ? dS : nullptr, W ? dW : nullptr, seed, method, split_rand, delta, dS, X_half,
                          Q_half))) return rc;
  if ((rc = copy_d2h(c, s, dS, vb))) return rc;
  return finish_and_check(c);
}

// the Brownian step with prescribed bodies (per = 1) or velocity components (per = 6), the checks done and kBT > 1e-10: the
// predictor picks per component (k_mx_bd_sums and rhs_and_midpoint_core's loop) and the solve at q^{n+1/2} is mx_step's solve
int mx_bd_step(rbl_ctx *c, const uint8_t *prescribed, int per, int np, const double *body_in, const double *slip, const double *W,
               uint64_t seed, int method, int split_rand, double delta, int max_iter, double rtol, double *F, int *iters, double *resid)
{
  int rc = step_begin(c); if (rc) return rc;
  MxBuf B;
  B.per = per;
  double *dW;
  bool have_slip;
  // the models at q^n; forces: free components only
  if ((rc = mx_upload(c, RblSide::Host, B, prescribed, body_in, slip, true, np, &have_slip))) return rc;
  if ((rc = step_upload_W(c, W, &dW))) return rc;
  return step_midpoint(
      c,
      [&](double *Xh, double *Qh) {                       // s takes the slip's place in the solve's workspace: it never leaves the device
        return rhs_and_midpoint_core(c, prescribed, B.mask, B.body_in, have_slip ? B.slip : nullptr, dW, seed, method, split_rand, delta, B.slip,
                                     Xh, Qh, per);
      },
      [&](double *U) {
        const int r = mx_solve(c, B, true, np, max_iter, rtol, iters, resid);
        return r ? r : step_commit(c, B.x, B.U, U, B.F, F, sizes_of(c).nb6, true);   // moments: lever arms of q^{n+1/2}
      });
}

// rbl_step_brownian_mixed (per = 1) and its _dof form (per = 6): checks, then the deterministic step, the all-free step or mx_bd_step
int mx_bd_step_entry(rbl_ctx *c, const char *who, int per, const uint8_t *prescribed, const double *body_in, const double *slip,
                     const double *W, uint64_t seed, int method, int split_rand, double delta, int max_iter, double rtol, double *F,
                     int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  int np = 0;
  const int rc = mx_bd_check(c, who, prescribed, body_in, max_iter, rtol, delta, &np, per); if (rc) return rc;
  if (!(c->S.kBT > 1e-10))                               // no Brownian terms: the deterministic step (as rbl_step_brownian, :967-970)
    return mx_step(c, who, prescribed, body_in, slip, max_iter, rtol, F, iters, resid, per);
  if (per == 6 && np == 0) {                             // the _dof step with nothing prescribed: rbl_step_brownian itself, hence its
    // bits (the masked solve goes through another GMRES driver and would differ from it in the last digits); F: the loads it solved
    // with, echoed.  The whole-body step with nobody prescribed goes through the masked solve, as it always has: its bits stay too
    int r = rbl_step_brownian(c, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol, iters, resid);
    if (!r && F && !(r = copy_d2h(c, F, step_force_dev(c), sizeof(double) * sizes_of(c).nb6))) r = finish_and_check(c);
    return r;
  }
  return mx_bd_step(c, prescribed, per, np, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol, F, iters, resid);
}

}  // namespace

// The masks the Brownian midpoint step takes per velocity component (include/rbl.h section 7): every body's three rotation entries
// all 0 or all 1, the translation entries as the caller likes -- then the free coordinates are a subset of the coordinates.
// prescribed6[R 6 N_bod] (R = 1: a single context; the replica is named otherwise).  No device is touched.
int rbl_bd_mask6_check(rbl_ctx *c, const char *who, const uint8_t *prescribed6, int R, int N_bod)
{
  for (size_t g = 0; g < (size_t)R * (size_t)N_bod; ++g) {
    const uint8_t *m = prescribed6 + 6 * g;
    const int nrot = (m[3] != 0) + (m[4] != 0) + (m[5] != 0);
    if (nrot == 0 || nrot == 3) continue;
    const std::string where = R > 1 ? "replica " + std::to_string(g / (size_t)N_bod) + ", body " + std::to_string(g % (size_t)N_bod)
                                    : "body " + std::to_string(g);
    return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": " + where + ": the rotation is partly prescribed (entries 3..5 of a body's row of "
                                    "prescribed6 must be all 0 or all 1 in the Brownian step: the drift of a partly prescribed rotation "
                                    "has not been derived)");
  }
  return RBL_OK;
}

// ============================================================================
// 7. prescribed kinematics (include/rbl.h)
// ============================================================================
int rbl_solve_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
                    double *lambda, double *U, double *F, int *iters, double *resid)
{
  if (c && (!U || !F)) return rbl_fail(c, RBL_ERR_ARG, "solve_mixed: U or F is NULL");
  return mx_host(c, "solve_mixed", prescribed, body_in, slip, max_iter, rtol, false, lambda, U, F, iters, resid);
}

int rbl_solve_mixed_dev(rbl_ctx *c, const uint8_t *prescribed, const double *d_body_in, const double *d_slip, int max_iter, double rtol,
                        double *d_lambda, double *d_U, double *d_F, int *iters, double *resid)
{
  return mx_dev(c, "solve_mixed_dev", prescribed, d_body_in, d_slip, max_iter, rtol, d_lambda, d_U, d_F, iters, resid, 1);
}

int rbl_step_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol, double *F,
                   int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  return mx_step(c, "step_mixed", prescribed, body_in, slip, max_iter, rtol, F, iters, resid);
}

// ---- a mask per velocity component: prescribed6[6 N_bod], the same workers with six mask entries per body ----------------------------
int rbl_solve_mixed_dof(rbl_ctx *c, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter, double rtol,
                        double *lambda, double *U, double *F, int *iters, double *resid)
{
  if (c && (!U || !F)) return rbl_fail(c, RBL_ERR_ARG, "solve_mixed_dof: U or F is NULL");
  return mx_host(c, "solve_mixed_dof", prescribed6, body_in, slip, max_iter, rtol, false, lambda, U, F, iters, resid, 6);
}

int rbl_solve_mixed_dof_dev(rbl_ctx *c, const uint8_t *prescribed6, const double *d_body_in, const double *d_slip, int max_iter,
                            double rtol, double *d_lambda, double *d_U, double *d_F, int *iters, double *resid)
{
  return mx_dev(c, "solve_mixed_dof_dev", prescribed6, d_body_in, d_slip, max_iter, rtol, d_lambda, d_U, d_F, iters, resid, 6);
}

int rbl_step_mixed_dof(rbl_ctx *c, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter, double rtol,
                       double *F, int *iters, double *resid)
{
  if (!c) return RBL_ERR_ARG;
  return mx_step(c, "step_mixed_dof", prescribed6, body_in, slip, max_iter, rtol, F, iters, resid, 6);
}

// ---- many right-hand sides under one mask, in lock step ------------------------------------------------------------------------------
int rbl_solve_mixed_multi(rbl_ctx *c, const uint8_t *prescribed, int nrhs, const double *body_in, const double *slip, int max_iter,
                          double rtol, double *lambda, double *U, double *F, int *iters, double *resid)
{
  return mx_multi(c, "solve_mixed_multi", RblSide::Host, prescribed, nrhs, body_in, slip, max_iter, rtol, lambda, U, F, iters, resid, 1);
}

int rbl_solve_mixed_multi_dev(rbl_ctx *c, const uint8_t *prescribed, int nrhs, const double *d_body_in, const double *d_slip, int max_iter,
                              double rtol, double *d_lambda, double *d_U, double *d_F, int *iters, double *resid)
{
  return mx_multi(c, "solve_mixed_multi_dev", RblSide::Device, prescribed, nrhs, d_body_in, d_slip, max_iter, rtol, d_lambda, d_U, d_F, iters, resid, 1);
}

int rbl_solve_mixed_dof_multi(rbl_ctx *c, const uint8_t *prescribed6, int nrhs, const double *body_in, const double *slip, int max_iter,
                              double rtol, double *lambda, double *U, double *F, int *iters, double *resid)
{
  return mx_multi(c, "solve_mixed_dof_multi", RblSide::Host, prescribed6, nrhs, body_in, slip, max_iter, rtol, lambda, U, F, iters, resid, 6);
}

int rbl_solve_mixed_dof_multi_dev(rbl_ctx *c, const uint8_t *prescribed6, int nrhs, const double *d_body_in, const double *d_slip,
                                  int max_iter, double rtol, double *d_lambda, double *d_U, double *d_F, int *iters, double *resid)
{
  return mx_multi(c, "solve_mixed_dof_multi_dev", RblSide::Device, prescribed6, nrhs, d_body_in, d_slip, max_iter, rtol, d_lambda, d_U, d_F, iters,
                  resid, 6);
}

int rbl_RHS_and_Midpoint_mixed_dev(rbl_ctx *c, const uint8_t *prescribed, const double *d_body_in, const double *d_slip,
                                   const double *d_W, uint64_t seed, int method, int split_rand, double delta, double *d_s,
                                   double *X_half, double *Q_half)
{
  return mx_bd_rhs_dev(c, "RHS_and_Midpoint_mixed_dev", prescribed, 1, d_body_in, d_slip, d_W, seed, method, split_rand, delta, d_s, X_half,
                       Q_half);
}

int rbl_RHS_and_Midpoint_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, const double *W,
                               uint64_t seed, int method, int split_rand, double delta, double *s, double *X_half, double *Q_half)
{
  return mx_bd_rhs_host(c, "RHS_and_Midpoint_mixed", prescribed, 1, body_in, slip, W, seed, method, split_rand, delta, s, X_half, Q_half);
}

int rbl_step_brownian_mixed(rbl_ctx *c, const uint8_t *prescribed, const double *body_in, const double *slip, const double *W,
                            uint64_t seed, int method, int split_rand, double delta, int max_iter, double rtol, double *F,
                            int *iters, double *resid)
{
  return mx_bd_step_entry(c, "step_brownian_mixed", 1, prescribed, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol, F, iters,
                          resid);
}

// ---- the Brownian midpoint step with a mask per velocity component: prescribed6[6 N_bod], every body's rotation entries all equal ----
int rbl_RHS_and_Midpoint_mixed_dof_dev(rbl_ctx *c, const uint8_t *prescribed6, const double *d_body_in, const double *d_slip,
                                       const double *d_W, uint64_t seed, int method, int split_rand, double delta, double *d_s,
                                       double *X_half, double *Q_half)
{
  return mx_bd_rhs_dev(c, "RHS_and_Midpoint_mixed_dof_dev", prescribed6, 6, d_body_in, d_slip, d_W, seed, method, split_rand, delta, d_s,
                       X_half, Q_half);
}

int rbl_RHS_and_Midpoint_mixed_dof(rbl_ctx *c, const uint8_t *prescribed6, const double *body_in, const double *slip, const double *W,
                                   uint64_t seed, int method, int split_rand, double delta, double *s, double *X_half, double *Q_half)
{
  return mx_bd_rhs_host(c, "RHS_and_Midpoint_mixed_dof", prescribed6, 6, body_in, slip, W, seed, method, split_rand, delta, s, X_half,
                        Q_half);
}

int rbl_step_brownian_mixed_dof(rbl_ctx *c, const uint8_t *prescribed6, const double *body_in, const double *slip, const double *W,
                                uint64_t seed, int method, int split_rand, double delta, int max_iter, double rtol, double *F,
                                int *iters, double *resid)
{
  return mx_bd_step_entry(c, "step_brownian_mixed_dof", 6, prescribed6, body_in, slip, W, seed, method, split_rand, delta, max_iter, rtol, F,
                          iters, resid);
}
