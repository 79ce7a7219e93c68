// rbl_small_solve.hpp -- the body of the one-kernel GMRES solve of a small system (rbl_small.hip has the description), as a device
// function template that the kernels of rbl_small.hip (JOINTS = false: the unmasked and the masked solve) and of
// rbl_small_joints.hip (JOINTS = true: the jointed solve of the ensembles, include/rbl.h sections 5 and 9) instantiate.  Every
// jointed statement is behind `if constexpr (JOINTS)` and the jointed arguments exist in SmallArgsJt only: with JOINTS = false
// the function is the kernel body rbl_small.hip had.  Behind it, the host side of every variant: the sizes and small_launch, the
// one launcher, which rbl_small.hip, rbl_small_per.hip and rbl_small_joints.hip call with their kernels.
#pragma once
#include <type_traits>

#include "rbl_joints_dev.hpp"
#include "rbl_small_dev.hpp"

namespace {


constexpr int SGT = RBL_SG_THREADS;  // threads of the one workgroup
constexpr int SG_MAXN = 256;       // blobs
constexpr int SG_MAXB = 64;        // bodies
constexpr int SG_MAXIT = 255;
constexpr int SG_RLDS = 64;        // up to this many iterations the triangular factor R stays in LDS (packed columns)
constexpr size_t SG_LDS_MAX = 150 * 1024;

struct SmallArgs {
  const double *X, *Q, *cfg;       // body state (device): 3 Nb, 4 Nb (scalar-first), N_blb x 3 (mean removed)
  const double *rhs;               // nsys
  const double *x0;                // initial guess or nullptr
  double *x;                       // nsys
  double *V, *H;                   // global workspace: (max_iter+1) nsys (unused when the basis is in LDS) | packed R columns (max_iter > 64)
  int *iters_out;                  // device scalars
  double *resid_out;
  unsigned *err;
  size_t work_stride;              // replica r (blockIdx.x) of an ensemble: its X, Q, rhs, x0, x, workspace, iters_out, resid_out
  int err_stride;                  // and error word lie r strides further (one replica: a grid of one, nothing moves)
  RblParams P;
  int N_blb, N_bod, max_iter;
  double rtol, fsign;
};
// The masked variant's outputs U and F (6 N_bod per replica: all body velocities, all body loads) lie in front of x, in ONE block
// [U of every replica | F of every replica | x of every replica]: their addresses follow from x and the grid, and no pointer of
// theirs has to stay in registers across the pair sweep (WALL sits at the 128-register ceiling of a 1024-thread workgroup).
struct SmallArgsMixed : SmallArgs {
  const unsigned char *mask;       // per N_bod per replica: 1 = prescribed -- the body (per = 1) or this velocity component of it (per = 6)
  const double *body_in;           // 6 N_bod per replica: U of a prescribed component (a free component's load is in rhs already)
  int reps;                        // the grid
  int per;                         // mask entries per body: 1 or 6 (read in the prologue only: the flags in LDS serve afterwards)
};
// PER: the cell, behind everything the open system's kernels take
struct SmallArgsPer : SmallArgs { RblSmallCell C; };
struct SmallArgsMixedPer : SmallArgsMixed { RblSmallCell C; };
// The jointed variant (JOINTS): rhs and x hold 3 n_joints more per replica, [slip ; -F ; c] and [lambda ; U ; phi].  The joint
// table is shared by the replicas; J.ptr holds the row starts of the joint ends BY BODY (N_bod + 1 entries: a body without a
// joint has an empty row; J.rows is unused), J.theta and J.rate hold n_joints values per replica, replica r's r n_joints further.
struct SmallArgsJt : SmallArgs {
  JtDev J;
  int n_ends;                      // entries of J.ends (pairs)
  int jstep;                       // a time step: the joint rows of rhs hold joint_velocity, c = jcoef gap + joint_velocity - rate ah (a lock's rows)
  double jcoef;                    // -gamma / dt
};

// The thread index behind an empty asm statement: what a jointed statement inside the iteration derives from it (addresses of
// the joint's LDS data, body and component of a slot) is computed where it is used and not hoisted out of the Krylov loop, where it
// would stay in registers across the pair sweep (WALL runs at the 128-register ceiling of a 1024-thread workgroup)
__device__ __forceinline__ int jt_thread(int t)
{
  asm volatile("" : "+v"(t));
  return t;
}

// One component of J^T phi on a body from one joint end: phi_j = (p0, p1, p2), s = +1 at end A, -1 at end B.  A ball end loads the
// force s phi_j (c < 3) and the torque l x (s phi_j) (rbl_KT_acc's formula), a lock end the torque s phi_j, an axis end s P phi_j
__device__ __forceinline__ double jt_JT_component(int kind, const double *lv, int end, int c, double p0, double p1, double p2)
{
  const double s = end ? -1.0 : 1.0;
  p0 *= s; p1 *= s; p2 *= s;
  if (kind == JT_BALL) {
    const double *l = lv + 3 * end;
    return c == 0 ? p0 : c == 1 ? p1 : c == 2 ? p2 : c == 3 ? l[1] * p2 - l[2] * p1 : c == 4 ? l[2] * p0 - l[0] * p2 : l[0] * p1 - l[1] * p0;
  }
  if (kind == JT_AXIS) jt_across(lv, p0, p1, p2);
  return c < 3 ? 0.0 : c == 3 ? p0 : c == 4 ? p1 : p2;
}

// (J U)_j of one joint (k_jt_tail's rows without phi): a ball joint (u_A + w_A x l_A) - (u_B + w_B x l_B), a lock joint w_A - w_B,
// an axis joint P (w_A - w_B); b < 0: the lab, no B term.  U: the 6 N_bod body velocities
__device__ __forceinline__ void jt_JU(int kind, const double *l, int a, int b, const double *U, double &o0, double &o1, double &o2)
{
  if (kind != JT_BALL) {
    const double *wa = U + 6 * a + 3;
    o0 = wa[0]; o1 = wa[1]; o2 = wa[2];
    if (b >= 0) {
      const double *wb = U + 6 * b + 3;
      o0 -= wb[0]; o1 -= wb[1]; o2 -= wb[2];
    }
    if (kind == JT_AXIS) jt_across(l, o0, o1, o2);
    return;
  }
  rbl_KU(l, U + 6 * a, o0, o1, o2);
  if (b >= 0) {
    double q0, q1, q2;
    rbl_KU(l + 3, U + 6 * b, q0, q1, q2);
    o0 -= q0; o1 -= q1; o2 -= q2;
  }
}

// sum over the wavefront, result in every lane, fixed order.  Inside the 16-lane rows by DPP moves (quad_perm, half-row
// and row mirrors: a few cycles each; the __shfl_xor butterfly is six dependent ds_bpermute round trips, ~800 cycles, and
// this kernel pays it on every dot product), across the four rows through v_readlane.
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v)
{
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value(double v, int lane)
{
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_sum(double v)
{
  v += dpp_move<0xB1>(v);      // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);      // quad_perm [2,3,0,1]
  v += dpp_move<0x141>(v);     // row_half_mirror
  v += dpp_move<0x140>(v);     // row_mirror: every lane holds its row's sum
  return ((lane_value(v, 0) + lane_value(v, 16)) + lane_value(v, 32)) + lane_value(v, 48);
}

// PER (the ensembles in a periodic cell, include/rbl.h sections 5 and 10): the operator's pair sweep sums every pair over the cell's
// images and takes in every blob's own images (rbl_small_pair_sweep<WALL, true>); the cell is A.C of SmallArgsPer / SmallArgsMixedPer,
// a kernel argument.  The self block, the preconditioner (image-free, diagonal) and everything else are the open system's: with
// PER = false the function is unchanged.
template <bool WALL, bool VLDS, bool MIXED, bool JOINTS, bool PER = false, class Args>
__device__ __forceinline__ void rbl_small_solve(Args A)
{
  static_assert(!(PER && JOINTS), "the jointed solve has no image sum");
  extern __shared__ double sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  constexpr int NW = SGT / 64;
  // JOINTS: nj joints, whose 3 nj rows stand behind the nsb = 3 N + 6 N_bod of the saddle system in every vector (nsys counts them)
  int nj_ = 0, ne_ = 0;
  if constexpr (JOINTS) { nj_ = A.J.n; ne_ = A.n_ends; }
  const int nbl = A.N_blb, nb = A.N_bod, N = nbl * nb, n3 = 3 * N, nb6 = 6 * nb, nsb = n3 + nb6;
  const int nj = nj_, nj3 = 3 * nj, ne = ne_, nsys = JOINTS ? nsb + nj3 : nsb;
  const int m = A.max_iter;
  {
    const int rep = blockIdx.x;
    A.X += (size_t)rep * 3 * nb; A.Q += (size_t)rep * 4 * nb;
    A.rhs += (size_t)rep * nsys; A.x += (size_t)rep * nsys;
    if constexpr (MIXED || JOINTS) A.x0 = nullptr;        // cold start only (the ensembles')
    else if (A.x0) A.x0 += (size_t)rep * nsys;
    A.V += (size_t)rep * A.work_stride; A.H += (size_t)rep * A.work_stride;
    A.iters_out += rep; A.resid_out += rep; A.err += (size_t)rep * A.err_stride;
    if constexpr (MIXED) {
      A.mask += (size_t)rep * nb * A.per; A.body_in += (size_t)rep * nb6;
    }
    if constexpr (JOINTS) { A.J.theta += (size_t)rep * nj; A.J.rate += (size_t)rep * nj; }
  }
  double *pos = sm;                             // 3N  positions / a
  double *lev = pos + n3;                       // 3N  lever arms
  double *iM = lev + n3;                        // 2N  diag_invM: (xx = yy, zz)
  double *dmp = iM + 2 * N;                     // N   wall damping d_i (1 without the wall term)
  // MIXED: the mask lives in LDS as a seventh entry of every row of NLs (1.0: the row's velocity component is prescribed), where the thread of a
  // body slot reads its row anyway: the flag costs no register and no address across the pair sweep
  constexpr int NS = MIXED ? 42 : 36, RS = MIXED ? 7 : 6;
  double *NLs = dmp + N;                        // NS Nb  (K^T invM K)^-1, row-major 6x6 per body (rows of RS)
  double *vz = NLs + NS * nb;                   // nsys   z = P^-1 v
  double *vw = vz + nsys;                       // nsys   w
  double *vv = vw + nsys;                       // nsys   current basis vector / scratch
  double *fb = vv + nsys;                       // 6 Nb   body sums
  double *hh = fb + nb6;                        // max_iter + 2: Gram-Schmidt coefficients of one pass, later y
  double *hc = hh + (m + 2);                    // max_iter + 2: the new Hessenberg column
  double *gg = hc + (m + 2);                    // max_iter + 2: rotated right-hand side
  double *cs = gg + (m + 2);                    // max_iter: Givens cosines
  double *sn = cs + m;                          // max_iter: Givens sines
  double *sc = sn + m;                          // 8 scalars: [1] stop flag, [2] residual estimate, [3] |w|^2 before Gram-Schmidt
  double *part = sc + 8;                        // NW x 3N: one accumulator set per wavefront for the symmetric pair sweep (also scratch)
  double *su = part + (size_t)NW * n3;          // 3N  self terms
  double *kt = su + n3;                         // 6N  per-blob terms of K^T lambda
  // JOINTS: the joint data, in LDS where the thread that needs it reads it anyway (small_lds_base_bytes counts the same pieces)
  double *jl = kt + 6 * N;                      // 6 nj   lever arms l_A | l_B of a ball joint, ah | 0 of an angular one (k_jt_geom's lev)
  double *jg = jl + 6 * nj;                     // 3 nj   a closed hinge's redundant row (gau)
  double *jt = jg + nj3;                        // 3 nj   the gaps (prologue), then t = J U0 - c of the preconditioner
  double *js = jt + nj3;                        // nj     sigma of an axis joint
  double *jd = js + nj;                         // 3 nj   the diagonal of S before it is factored
  double *Sm = jd + nj3;                        // (3 nj)^2  S, then its Cholesky factor (column-major, lower triangle)
  double *Si = Sm + (size_t)nj3 * nj3;          // (3 nj)^2  S^-1
  int *jbody = (int *)(Si + (size_t)nj3 * nj3); // 2 nj bodies | nj kinds | N_bod + 1 row starts by body | 2 ne (joint, end)
  int *jkind = jbody + 2 * nj, *jptr = jkind + nj, *jends = jptr + nb + 1;
  double *Rl = JOINTS ? (double *)jbody + (3 * nj + nb + 1 + 2 * ne + 1) / 2 : kt + 6 * N;   // packed upper-triangular R, column j at j (j+1) / 2 (max_iter <= SG_RLDS), else global
  const bool r_lds = m <= SG_RLDS;
  double *Rm = r_lds ? Rl : A.H;
  double *Vb = VLDS ? Rl + (r_lds ? (size_t)m * (m + 1) / 2 : 0) : A.V;   // Krylov basis
  // MIXED with the basis in global memory: 32-bit offsets from the (uniform) base -- the workspace of one replica is a few MB --
  // so that no 64-bit address per thread is held across the pair sweep
  constexpr bool V32 = (MIXED || JOINTS) && !VLDS;
  const RblParams P = A.P;
  const RblParams Pu = rbl_small_unit_params(P);
  unsigned flags = 0;

  // ---- geometry + diagonal preconditioner ---------------------------------------------------------------
  if (t < N) {
    const int b = t / nbl, k = t - b * nbl;
    double R[9];
    rbl_quat_rot9(A.Q + 4 * b, R);
    const double c0 = A.cfg[3 * k], c1 = A.cfg[3 * k + 1], c2 = A.cfg[3 * k + 2];
    double l0, l1, l2, p2;
    {
#pragma clang fp contract(off)
      l0 = c0 * R[0] + c1 * R[1] + c2 * R[2];
      l1 = c0 * R[3] + c1 * R[4] + c2 * R[5];
      l2 = c0 * R[6] + c1 * R[7] + c2 * R[8];
      lev[3 * t] = l0; lev[3 * t + 1] = l1; lev[3 * t + 2] = l2;
      p2 = l2 + A.X[3 * b + 2];
      pos[3 * t] = (l0 + A.X[3 * b]) * P.inv_a; pos[3 * t + 1] = (l1 + A.X[3 * b + 1]) * P.inv_a; pos[3 * t + 2] = p2 * P.inv_a;
    }
    double dxx = 4.0 / 3.0, dzz = 4.0 / 3.0, d = 1.0;
    if (WALL) {  // self wall term (:98-104), h = z/a; damping (:629-633)
      const double h = p2 / P.a;
      if (h < 0.0) flags |= RBL_FLAG_BELOW_WALL;
      const double iz = 1.0 / h, iz3 = iz * iz * iz, iz5 = iz3 * iz * iz;
      dxx += -(9 * iz - 2 * iz3 + iz5) / 12.0;
      dzz += -(9 * iz - 4 * iz3 + iz5) / 6.0;
      d = (p2 >= P.a) ? 1.0 : p2 / P.a;
    }
    const double scale = 1.0 / P.nf;
    iM[2 * t] = scale / dxx; iM[2 * t + 1] = scale / dzz;
    dmp[t] = d;
  }
  __syncthreads();
  if (t < nb) {   // Ninv_b = sum_k K_k^T D_k K_k (lower triangle), then its 6x6 Cholesky, row-major L
    double acc[21];
    for (int q = 0; q < 21; ++q) acc[q] = 0.0;
    for (int k = 0; k < nbl; ++k) {
      const int i = t * nbl + k;
      const double lx = lev[3 * i], ly = lev[3 * i + 1], lz = lev[3 * i + 2];
      const double Kk[3][6] = {{1, 0, 0, 0, lz, -ly}, {0, 1, 0, -lz, 0, lx}, {0, 0, 1, ly, -lx, 0}};
      const double D[3] = {iM[2 * i], iM[2 * i], iM[2 * i + 1]};
      int q = 0;
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) {
          acc[q] += Kk[0][r] * D[0] * Kk[0][c] + Kk[1][r] * D[1] * Kk[1][c] + Kk[2][r] * D[2] * Kk[2][c];
          ++q;
        }
    }
    double L[36];
    int q = 0;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c <= r; ++c) { L[6 * r + c] = acc[q]; if (c < r) L[6 * c + r] = 0.0; ++q; }
    if constexpr (MIXED) {
      // the flags (the seventh entry of every row of NLs; the inverse below writes the first six), from one mask entry per body
      // or six.  A partly prescribed body: the rows and columns of its prescribed components become the identity's BEFORE the
      // factorisation (k_mx_factors' rule: a principal submatrix's factor is no sub-block of the full one); the selects leave
      // a body with no bit set its matrix, factor and inverse bit for bit.  The inverse then has the identity's rows and columns
      // there too, so apply_PC's 6x6 product takes nothing from a prescribed slot into a free one
      unsigned pm = 0;                         // bit p = component p of this body is prescribed
      for (int p = 0; p < 6; ++p) pm |= (A.mask[A.per == 6 ? 6 * t + p : t] ? 1u : 0u) << p;
      for (int p = 0; p < 6; ++p) NLs[NS * t + RS * p + 6] = (pm >> p & 1u) ? 1.0 : 0.0;
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) {
          const bool cut = ((pm >> r) | (pm >> c)) & 1u;
          L[6 * r + c] = cut ? (r == c ? 1.0 : 0.0) : L[6 * r + c];
        }
    }
    bool ok = true;
    for (int j = 0; j < 6; ++j) {
      double dd = L[6 * j + j];
      for (int k = 0; k < j; ++k) dd -= L[6 * j + k] * L[6 * j + k];
      if (!(dd > 0.0)) ok = false;
      dd = sqrt(dd);
      L[6 * j + j] = dd;
      for (int i = j + 1; i < 6; ++i) {
        double v = L[6 * i + j];
        for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k];
        L[6 * i + j] = v / dd;
      }
    }
    if (!ok) flags |= RBL_FLAG_NOT_SPD;
    // the explicit inverse (L L^T)^-1, column by column: every application is then a 6x6 product spread over six
    // threads instead of one thread's chain of two triangular solves with twelve divisions
    for (int col = 0; col < 6; ++col) {
      double y[6], u[6];
      for (int p = 0; p < 6; ++p) {
        double v = (p == col) ? 1.0 : 0.0;
        for (int q2 = 0; q2 < p; ++q2) v -= L[6 * p + q2] * y[q2];
        y[p] = v / L[6 * p + p];
      }
      for (int p = 5; p >= 0; --p) {
        double v = y[p];
        for (int q2 = p + 1; q2 < 6; ++q2) v -= L[6 * q2 + p] * u[q2];
        u[p] = v / L[6 * p + p];
      }
      for (int p = 0; p < 6; ++p) NLs[NS * t + RS * p + col] = u[p];
    }
  }
  __syncthreads();

  // ---- JOINTS: the joints of this replica's configuration, S = J N~^-1 J^T, its factor and its inverse ------------------------
  // (what k_jt_geom, k_jt_schur, the Cholesky, k_jt_pivots and k_jt_inverse of rbl_joints.hip do in launches of their own)
  if constexpr (JOINTS) {
    for (int i = t; i < 2 * nj; i += SGT) jbody[i] = A.J.body[i];
    for (int i = t; i < nj; i += SGT) jkind[i] = A.J.kind[i];
    for (int i = t; i <= nb; i += SGT) jptr[i] = A.J.ptr[i];
    for (int i = t; i < 2 * ne; i += SGT) jends[i] = A.J.ends[i];
    if (t < nj) jt_geom_joint<true>(A.X, A.Q, A.J, t, jl, jt, jg);
    __syncthreads();
    if (t < nj) js[t] = jkind[t] == JT_AXIS ? jt_sigma(NLs, jbody[2 * t]) : 0.0;   // NLs: the lab-frame N~^-1 per body, rows of 6
    // one entry of S a work item: row r of joint j against row c of joint k, s_j s_k g_j^T N_b^-1 g_k over the bodies b their
    // ends share (at most two), an axis joint's sigma ah ah^T on its diagonal block, a closed hinge's (sigma_t / 2) gau gau^T
    for (int e = t; e < nj3 * nj3; e += SGT) {
      const int row = e / nj3, col = e - row * nj3, j = row / 3, r = row - 3 * j, k = col / 3, c = col - 3 * k;
      double v = 0.0;
      for (int ej = 0; ej < 2; ++ej)
        for (int ek = 0; ek < 2; ++ek) {
          const int bj = jbody[2 * j + ej], bk = jbody[2 * k + ek];
          if (bj < 0 || bj != bk) continue;
          double gj[6], gk[6];
          jt_G_row(jkind[j], jl + 6 * j, ej, r, gj);
          jt_G_row(jkind[k], jl + 6 * k, ek, c, gk);
          const double *Nb = NLs + 36 * bj;
          double s = 0.0;
#pragma unroll
          for (int p = 0; p < 6; ++p) {
            double w = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) w += Nb[6 * p + q] * gk[q];
            s += gj[p] * w;
          }
          v += ej == ek ? s : -s;
        }
      if (j == k && jkind[j] == JT_AXIS) v += js[j] * jl[6 * j + r] * jl[6 * j + c];
      const int mate = A.J.mate[2 * j];
      if (mate >= 0 && (k == j || k == mate)) {
        const double *Nb = NLs + 36 * jbody[2 * (j < mate ? j : mate)];
        v += (Nb[0] + Nb[7] + Nb[14]) * (0.5 / 3.0) * jg[3 * j + r] * jg[3 * k + c];
      }
      Sm[(size_t)col * nj3 + row] = v;
      if (row == col) jd[row] = v;
    }
    __syncthreads();
    // right-looking Cholesky by the workgroup, column by column; every entry is updated by one thread, in column order.  The
    // pivot test is k_jt_pivots'.  Every thread reads the same pivot and takes the same decision: a lost pivot (a redundant
    // joint set) latches RBL_FLAG_REDUNDANT and stands in as 1, so that what follows stays finite and no thread leaves a barrier out
    for (int j = 0; j < nj3; ++j) {
      const double djj = Sm[(size_t)j * nj3 + j], s0 = jd[j];
      double d = sqrt(djj);
      if (!(d > 0.0) || !isfinite(d) || !(s0 > 0.0) || !(d * d > JT_PIVOT_TOL * s0)) { flags |= RBL_FLAG_REDUNDANT; d = 1.0; }
      __syncthreads();
      for (int i = j + t; i < nj3; i += SGT) Sm[(size_t)j * nj3 + i] = i == j ? d : Sm[(size_t)j * nj3 + i] / d;
      __syncthreads();
      const int mr = nj3 - j - 1;
      for (int e = t; e < mr * mr; e += SGT) {
        const int kk = e / mr, ii = e - kk * mr;
        if (ii >= kk) Sm[(size_t)(j + 1 + kk) * nj3 + j + 1 + ii] -= Sm[(size_t)j * nj3 + j + 1 + ii] * Sm[(size_t)j * nj3 + j + 1 + kk];
      }
      __syncthreads();
    }
    // S^-1 = L^-T L^-1, one thread a column: forward and backward substitution with the column at Si[p nj3 + col] (neighbouring
    // threads, neighbouring words).  S^-1 is symmetric: an iteration reads row r down Si[c nj3 + r]
    if (t < nj3) {
      for (int p = 0; p < nj3; ++p) {
        double v = p == t ? 1.0 : 0.0;
        for (int q = t; q < p; ++q) v -= Sm[(size_t)q * nj3 + p] * Si[(size_t)q * nj3 + t];
        Si[(size_t)p * nj3 + t] = p < t ? 0.0 : v / Sm[(size_t)p * nj3 + p];
      }
      for (int p = nj3 - 1; p >= 0; --p) {
        double v = Si[(size_t)p * nj3 + t];
        for (int q = p + 1; q < nj3; ++q) v -= Sm[(size_t)p * nj3 + q] * Si[(size_t)q * nj3 + t];
        Si[(size_t)p * nj3 + t] = v / Sm[(size_t)p * nj3 + p];
      }
    }
    __syncthreads();
  }

  // J^T phi, component c of body b: the joint ends on the body in stored order (JOINTS)
  auto jt_body_sum = [&](const double *ph, int b, int c) -> double {
    double h = 0.0;
    for (int q = jptr[b]; q < jptr[b + 1]; ++q) {
      const int j = jends[2 * q];
      h += jt_JT_component(jkind[j], jl + 6 * j, jends[2 * q + 1], c, ph[3 * j], ph[3 * j + 1], ph[3 * j + 2]);
    }
    return h;
  };

  // ---- operators on LDS vectors (every thread calls them: they contain barriers) ----------------------------
  // out = P^-1 in   (apply_PC with the diagonal invM, :589-616; fsign: see rbl_ctx::gmres_pc_sign_fix)
  auto apply_PC = [&, tk = t](const double *in, double *out) {
    // JOINTS: what this operator derives from the thread index is made here, per call, and frees its registers across the pair
    // sweep (jt_thread); otherwise t is the kernel's
    const int t = JOINTS ? jt_thread(tk) : tk;
    if (t < N) {                             // per-blob terms of K^T (invM slip) -> part[c][blob]
      const double v0 = iM[2 * t] * in[3 * t], v1 = iM[2 * t] * in[3 * t + 1], v2 = iM[2 * t + 1] * in[3 * t + 2];
      const double l0 = lev[3 * t], l1 = lev[3 * t + 1], l2 = lev[3 * t + 2];
      part[t] = v0; part[N + t] = v1; part[2 * N + t] = v2;
      part[3 * N + t] = l1 * v2 - l2 * v1; part[4 * N + t] = l2 * v0 - l0 * v2; part[5 * N + t] = l0 * v1 - l1 * v0;
    }
    __syncthreads();
    if (t < nb6) {                           // fsign F - K^T (invM slip), component c of body b (blobs added in order)
      const int b = t / 6, c = t - 6 * b;
      const double *p = part + (size_t)c * N + (size_t)b * nbl;
      double f = 0.0;
      for (int k = 0; k < nbl; ++k) f += p[k];
      if constexpr (MIXED || JOINTS) fb[t] = in[n3 + t] - f;         // the force block's sign restored (fsign = +1), as the ensembles solve
      else fb[t] = A.fsign * in[n3 + t] - f;
    }
    __syncthreads();
    if (t < nb6) {                           // U = Ninv^-1 (fsign F - f)   (:601-608), explicit 6x6 inverse
      const int b = t / 6, c = t - 6 * b;
      const double *Nm = NLs + NS * b + RS * c, *rh = fb + 6 * b;
      double u = 0.0;
#pragma unroll
      for (int d = 0; d < 6; ++d) u = __builtin_fma(Nm[d], rh[d], u);
      if constexpr (MIXED) u = Nm[6] != 0.0 ? in[n3 + t] : u;   // a prescribed component's slot passes through
      out[n3 + t] = u;
    }
    __syncthreads();
    if (t < N) {                             // Lambda = invM (slip + K U)   (:610)
      const int b = t / nbl;
      const double *u = out + n3 + 6 * b;
      const double l0 = lev[3 * t], l1 = lev[3 * t + 1], l2 = lev[3 * t + 2];
      out[3 * t] = iM[2 * t] * (in[3 * t] + u[0] + l2 * u[4] - l1 * u[5]);       // MIXED, all six prescribed: u = 0 (see apply_A),
      out[3 * t + 1] = iM[2 * t] * (in[3 * t + 1] + u[1] + l0 * u[5] - l2 * u[3]);   // so this is lambda = invM slip
      out[3 * t + 2] = iM[2 * t + 1] * (in[3 * t + 2] + u[2] + l1 * u[3] - l0 * u[4]);
    }
    __syncthreads();
    if constexpr (JOINTS) {
      // the exact inverse with the joints (rbl_joints.hip's jt_pc): t = J U0 - c_in, phi = S^-1 t, h = J^T phi, and the second
      // pass in its collapsed form -- its input is [0 ; h], so U' = N~^-1 h and lambda' = invM (K U') -- out -= [lambda' ; U']
      const int tj = jt_thread(t);
      if (tj < nj) {
        double o0, o1, o2;
        jt_JU(jkind[tj], jl + 6 * tj, jbody[2 * tj], jbody[2 * tj + 1], out + n3, o0, o1, o2);
        jt[3 * tj] = o0 - in[nsb + 3 * tj]; jt[3 * tj + 1] = o1 - in[nsb + 3 * tj + 1]; jt[3 * tj + 2] = o2 - in[nsb + 3 * tj + 2];
      }
      __syncthreads();
      if (tj < nj3) {
        double a = 0.0;
        for (int c = 0; c < nj3; ++c) a = __builtin_fma(Si[c * nj3 + tj], jt[c], a);
        out[nsb + tj] = a;
      }
      __syncthreads();
      if (tj < nb6) fb[tj] = jt_body_sum(out + nsb, tj / 6, tj % 6);
      __syncthreads();
      if (tj < nb6) {
        const int b = tj / 6, c = tj - 6 * b;
        const double *Nm = NLs + NS * b + RS * c, *rh = fb + 6 * b;
        double u = 0.0;
#pragma unroll
        for (int d = 0; d < 6; ++d) u = __builtin_fma(Nm[d], rh[d], u);
        kt[tj] = u;
        out[n3 + tj] -= u;
      }
      __syncthreads();
      if (tj < N) {
        const double *u = kt + 6 * (tj / nbl);
        const double l0 = lev[3 * tj], l1 = lev[3 * tj + 1], l2 = lev[3 * tj + 2];
        out[3 * tj] -= iM[2 * tj] * (u[0] + l2 * u[4] - l1 * u[5]);
        out[3 * tj + 1] -= iM[2 * tj] * (u[1] + l0 * u[5] - l2 * u[3]);
        out[3 * tj + 2] -= iM[2 * tj + 1] * (u[2] + l1 * u[3] - l0 * u[4]);
      }
      __syncthreads();
    }
  };

  // MIXED: [M lambda - K (D_f U) ; D_f K^T lambda + D_p U].  The slots of prescribed components are 0 in the right-hand side, this
  // operator is the identity on them and apply_PC passes them through, so they are exactly 0 in every vector either is applied to
  // (cold start only): K U of such a body is exactly 0 and its rows need no select -- the two selects are on the body slots.
  // out = [M lambda - K U ; K^T lambda]   (src/Rigid.py:73-80; M = B Mob B with the wall term, :641-659): self blocks here,
  // every unordered pair once by rbl_small_pair_sweep, the waves' accumulator sets added in wave order afterwards
  auto apply_A = [&](const double *in, double *out) {
    if (t < N) {                             // self blocks (:40-46, :98-104) and the per-blob terms of K^T lambda
      const double di = WALL ? dmp[t] : 1.0;
      double ux = 0.0, uy = 0.0, uz = 0.0;
      rbl_pair_accum<WALL, true, RBL_UNIT_RADIUS>(Pu, pos[3 * t], pos[3 * t + 1], pos[3 * t + 2], pos[3 * t], pos[3 * t + 1], pos[3 * t + 2],
                                       di * in[3 * t], di * in[3 * t + 1], di * in[3 * t + 2], true, ux, uy, uz, flags);
      su[3 * t] = ux; su[3 * t + 1] = uy; su[3 * t + 2] = uz;
      const double v0 = in[3 * t], v1 = in[3 * t + 1], v2 = in[3 * t + 2];
      const double l0 = lev[3 * t], l1 = lev[3 * t + 1], l2 = lev[3 * t + 2];
      kt[t] = v0; kt[N + t] = v1; kt[2 * N + t] = v2;
      kt[3 * N + t] = l1 * v2 - l2 * v1; kt[4 * N + t] = l2 * v0 - l0 * v2; kt[5 * N + t] = l0 * v1 - l1 * v0;
    }
    if constexpr (PER) rbl_small_pair_sweep<WALL, true>(Pu, pos, dmp, in, N, part, flags, A.C);
    else rbl_small_pair_sweep<WALL>(Pu, pos, dmp, in, N, part, flags);   // one accumulator set per wave in part (rbl_small_dev.hpp)
    if (t < n3) {                            // U_i = nf d_i (self + sum over the waves' sets) - (K U)_i
      double s = su[t];
      for (int w = 0; w < NW; ++w) s += part[(size_t)w * n3 + t];
      const int i = t / 3, c = t - 3 * i, b = i / nbl;
      if (!isfinite(s)) flags |= RBL_FLAG_NONFINITE;
      const double *u = in + n3 + 6 * b;
      const double l0 = lev[3 * i], l1 = lev[3 * i + 1], l2 = lev[3 * i + 2];
      const double ku = c == 0 ? u[0] + l2 * u[4] - l1 * u[5] : c == 1 ? u[1] + l0 * u[5] - l2 * u[3] : u[2] + l1 * u[3] - l0 * u[4];
      out[t] = (WALL ? P.nf * dmp[i] : P.nf) * s - ku;
    }
    if (t < nb6) {                           // K^T lambda: blobs of the body added in order (3N + 6 N_bod may exceed the
      const int b = t / 6, c = t - 6 * b;    // thread count, so this is not an else-branch of the rows above)
      const double *p = kt + (size_t)c * N + (size_t)b * nbl;
      double f = 0.0;
      for (int k = 0; k < nbl; ++k) f += p[k];
      if constexpr (MIXED) f = NLs[NS * b + RS * c + 6] != 0.0 ? in[n3 + t] : f;   // D_p U: the identity on a prescribed component's slot
      if constexpr (JOINTS) {                                                      // + J^T phi
        const int tj = jt_thread(t);
        f += jt_body_sum(in + nsb, tj / 6, tj % 6);
      }
      out[n3 + t] = f;
    }
    if constexpr (JOINTS) {                    // the joint rows: J U, with P and less sigma ah (ah . phi_j) on an axis joint (k_jt_tail)
      const int tj = jt_thread(t);
      if (tj < nj) {
        double o0, o1, o2;
        const double *l = jl + 6 * tj;
        jt_JU(jkind[tj], l, jbody[2 * tj], jbody[2 * tj + 1], in + n3, o0, o1, o2);
        if (jkind[tj] == JT_AXIS) {
          const double *p = in + nsb + 3 * tj;
          const double d = js[tj] * (l[0] * p[0] + l[1] * p[1] + l[2] * p[2]);
          o0 -= l[0] * d; o1 -= l[1] * d; o2 -= l[2] * d;
        }
        out[nsb + 3 * tj] = o0; out[nsb + 3 * tj + 1] = o1; out[nsb + 3 * tj + 2] = o2;
      }
    }
    __syncthreads();
  };

  // squared norm of an LDS vector -> hh[m+1] (every thread gets it): wave partials added in wave order
  auto norm2 = [&](const double *v) -> double {
    double a = 0.0;
    for (int i = t; i < nsys; i += SGT) a = __builtin_fma(v[i], v[i], a);
    a = wave_sum(a);
    if (lane == 0) part[wave] = a;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += part[w];
    __syncthreads();
    return s;
  };

  // ---- r0 = b - A x0 (or b), beta, V_0 --------------------------------------------------------------------
  double bnorm;
  {
    if constexpr (!MIXED) {
      for (int i = t; i < nsys; i += SGT) vw[i] = A.rhs[i];
      if constexpr (JOINTS) {                  // c of a time step in place (k_jt_step_rhs_kinds), then an axis joint's rows across its axis
        __syncthreads();
        const int tj = jt_thread(t);
        if (tj < nj) {
          double c0 = vw[nsb + 3 * tj], c1 = vw[nsb + 3 * tj + 1], c2 = vw[nsb + 3 * tj + 2];
          const double *l = jl + 6 * tj;
          if (A.jstep) {
            c0 = A.jcoef * jt[3 * tj] + c0; c1 = A.jcoef * jt[3 * tj + 1] + c1; c2 = A.jcoef * jt[3 * tj + 2] + c2;
            if (jkind[tj] == JT_LOCK) {
              const double rate = A.J.rate[tj];
              c0 -= rate * l[0]; c1 -= rate * l[1]; c2 -= rate * l[2];
            }
          }
          if (jkind[tj] == JT_AXIS) jt_across(l, c0, c1, c2);
          vw[nsb + 3 * tj] = c0; vw[nsb + 3 * tj + 1] = c1; vw[nsb + 3 * tj + 2] = c2;
        }
      }
    } else for (int i = t; i < nsys; i += SGT) {
      double v = A.rhs[i];
      {                                      // top += K (D_p U_in) (the lever arms of this configuration), bottom = 0 on prescribed components
        if (i < n3) {
          const int bl = i / 3, c = i - 3 * bl, b = bl / nbl;
          const double *fl = NLs + NS * b + 6;         // the six flags of the body (filled above)
          bool any = false;
          for (int p = 0; p < 6; ++p) any = any || fl[RS * p] != 0.0;
          if (any) {                               // K (D_p U_in): the prescribed components only; all six: the whole-body sum
            double u[6];
            for (int p = 0; p < 6; ++p) u[p] = fl[RS * p] != 0.0 ? A.body_in[6 * b + p] : 0.0;
            const double l0 = lev[3 * bl], l1 = lev[3 * bl + 1], l2 = lev[3 * bl + 2];
            v += c == 0 ? u[0] + l2 * u[4] - l1 * u[5] : c == 1 ? u[1] + l0 * u[5] - l2 * u[3] : u[2] + l1 * u[3] - l0 * u[4];
          }
        } else {                             // what is echoed is written here: rhs and body_in are not needed again
          // U and F of this replica: the launcher's ONE block [U | F | x] (the masked rbl_launch_gmres_small_ens: reps x 6 N_bod,
          // then reps x nsys), found from A.x, which the prologue moved on by blockIdx.x * nsys; the split at the end forms the
          // same two addresses -- change the layout there and in both places here together
          double *Uo = A.x - (size_t)blockIdx.x * nsys - 2 * (size_t)A.reps * nb6 + (size_t)blockIdx.x * nb6, *Fo = Uo + (size_t)A.reps * nb6;
          const int j = i - n3;
          if (NLs[NS * (j / 6) + RS * (j % 6) + 6] != 0.0) { v = 0.0; Uo[j] = A.body_in[j]; }
          else Fo[j] = -v;
        }
      }
      vw[i] = v;
    }
    __syncthreads();
    bnorm = sqrt(norm2(vw));
    if (A.x0) {
      for (int i = t; i < nsys; i += SGT) vz[i] = A.x0[i];
      __syncthreads();
      apply_A(vz, vv);
      for (int i = t; i < nsys; i += SGT) vw[i] -= vv[i];
      __syncthreads();
    }
  }
  const double beta = A.x0 ? sqrt(norm2(vw)) : bnorm;
  int used = 0;
  const double ibn = (bnorm > 0.0) ? 1.0 / bnorm : 0.0;
  double resid = (bnorm > 0.0) ? beta / bnorm : 0.0;
  const bool trivial = !(beta > 0.0) || (A.rtol > 0.0 && resid < A.rtol);
  if constexpr (MIXED || JOINTS) {                       // 1/|b| and the residual wait in LDS, not in registers, across the iterations
    if (t == 0) { sc[4] = ibn; sc[2] = resid; }
  }
  if (!trivial) {
    const double ib = 1.0 / beta;
    if constexpr (V32) {
      for (int i = t; i < nsys; i += SGT) { const double v = vw[i] * ib; vv[i] = v; Vb[(unsigned)i] = v; }
    } else {
      for (int i = t; i < nsys; i += SGT) { const double v = vw[i] * ib; vv[i] = v; Vb[i] = v; }
    }
    if (t == 0) gg[0] = beta;
    __syncthreads();
#ifdef RBL_SMALL_PROF
    long long tp[6] = {0, 0, 0, 0, 0, 0}, t0 = clock64(), t1;
#define RBL_STAMP(k) do { t1 = clock64(); tp[k] += t1 - t0; t0 = t1; } while (0)
#else
#define RBL_STAMP(k) do { } while (0)
#endif
    for (int j = 0; j < m; ++j) {
      RBL_STAMP(5);
      apply_PC(vv, vz);
      RBL_STAMP(0);
      apply_A(vz, vw);
      RBL_STAMP(1);
      // Classical Gram-Schmidt against V_0..V_j (wave w takes the basis vectors w, w+NW, ...), repeated only when the
      // first pass cancelled more than a factor 10 of |w| (the "twice is enough" test of Daniel-Gragg-Kaufman-Stewart
      // with eta = 0.1: the orthogonality error of a single pass is ~eps |w_before| / |w_after|).  Every update sweep
      // also gathers |w|^2, wave 0's first dot-product sweep gathers |w_before|^2: no separate norm passes.
      double hn2 = 0.0;
      for (int pass = 0; pass < 2; ++pass) {
        for (int k = wave; k <= j; k += NW) {
          const double *vk = Vb + (size_t)k * nsys;
          double a = 0.0, w0 = 0.0;
          for (int i = lane; i < nsys; i += 64) {
            const double wi = vw[i];
            if constexpr (V32) a = __builtin_fma(Vb[(unsigned)(k * nsys + i)], wi, a);
            else a = __builtin_fma(vk[i], wi, a);
            if (k == 0 && pass == 0) w0 = __builtin_fma(wi, wi, w0);
          }
          a = wave_sum(a);
          if (k == 0 && pass == 0) w0 = wave_sum(w0);
          if (lane == 0) { hh[k] = a; if (k == 0 && pass == 0) sc[3] = w0; }
        }
        __syncthreads();
        double wsq = 0.0;
        for (int i = t; i < nsys; i += SGT) {
          double a = vw[i];
          if constexpr (V32) { for (int k = 0; k <= j; ++k) a = __builtin_fma(-hh[k], Vb[(unsigned)(k * nsys + i)], a); }
          else for (int k = 0; k <= j; ++k) a = __builtin_fma(-hh[k], Vb[(size_t)k * nsys + i], a);
          vw[i] = a;
          wsq = __builtin_fma(a, a, wsq);
        }
        if (t <= j) hc[t] = pass ? hc[t] + hh[t] : hh[t];
        wsq = wave_sum(wsq);
        if (lane == 0) part[wave] = wsq;
        __syncthreads();
        hn2 = 0.0;
        for (int w = 0; w < NW; ++w) hn2 += part[w];
        if (hn2 >= 0.01 * sc[3]) break;      // workgroup-uniform: every thread adds the same 16 numbers in the same order
        __syncthreads();                     // part / hh are rewritten by the second pass
      }
      RBL_STAMP(2);
      const double hn = sqrt(hn2);
      RBL_STAMP(3);
      const double ih = hn > 1e-300 ? 1.0 / hn : 0.0;
      double *vn = Vb + (size_t)(j + 1) * nsys;
      if constexpr (V32) {
        for (int i = t; i < nsys; i += SGT) { const double v = vw[i] * ih; vv[i] = v; Vb[(unsigned)((j + 1) * nsys + i)] = v; }
      } else {
        for (int i = t; i < nsys; i += SGT) { const double v = vw[i] * ih; vv[i] = v; vn[i] = v; }
      }
      if (t == 0) {   // Givens update of column j (in LDS) and of the rotated right-hand side; residual estimate
        double cur = hc[0];                  // the running entry stays in a register: the chain is two FMAs per rotation,
        for (int i = 0; i < j; ++i) {        // the LDS reads of cs, sn and the next entry do not depend on it
          const double nxt = hc[i + 1], ci = cs[i], si = sn[i];
          hc[i] = __builtin_fma(ci, cur, si * nxt);
          cur = __builtin_fma(-si, cur, ci * nxt);
        }
        hc[j] = cur; hc[j + 1] = hn;
        const double den = sqrt(__builtin_fma(hc[j], hc[j], hc[j + 1] * hc[j + 1]));   // entries are O(|A P^-1|): no scaling needed
        const double rden = den > 0.0 ? 1.0 / den : 0.0;
        cs[j] = den > 0.0 ? hc[j] * rden : 1.0;
        sn[j] = hc[j + 1] * rden;
        hc[j] = den;
        gg[j + 1] = -sn[j] * gg[j];
        gg[j] = cs[j] * gg[j];
        if constexpr (MIXED || JOINTS) sc[2] = fabs(gg[j + 1]) * sc[4];
        else sc[2] = fabs(gg[j + 1]) * ibn;
        sc[1] = (A.rtol > 0.0 && sc[2] < A.rtol) || !(hn > 1e-300) ? 1.0 : 0.0;
        double *rc = Rm + (size_t)j * (j + 1) / 2;         // column j of R, rows 0..j
        for (int i = 0; i <= j; ++i) rc[i] = hc[i];
      }
      __syncthreads();
      RBL_STAMP(4);
      used = j + 1;
      resid = sc[2];
      if (sc[1] != 0.0) break;               // workgroup-uniform
    }
#ifdef RBL_SMALL_PROF
    if (t == 0) printf("k_gmres_small cycles (s_memtime, 100 MHz ticks?) over %d iterations: PC %lld  A %lld  CGS2 %lld  norm %lld  normalise+Givens %lld  other %lld\n",
                       used, tp[0], tp[1], tp[2], tp[3], tp[4], tp[5]);
#endif
    // y = R^-1 g (thread 0), z = V y, x = P^-1 z (+ x0).  A factor kept in global memory (max_iter > 64) is first staged
    // into the idle partial-sum buffer: the substitution is a chain of dependent reads
    const double *Rs = Rm;
    const int nR = used * (used + 1) / 2;
    if (!r_lds && nR <= NW * n3) {
      if constexpr (V32) { for (int i = t; i < nR; i += SGT) part[i] = Rm[(unsigned)i]; }
      else for (int i = t; i < nR; i += SGT) part[i] = Rm[i];
      Rs = part;
      __syncthreads();
    }
    if (t == 0) {
      for (int i = used - 1; i >= 0; --i) {
        double v = gg[i];
        for (int k = i + 1; k < used; ++k) v -= Rs[(size_t)k * (k + 1) / 2 + i] * hh[k];
        const double d = Rs[(size_t)i * (i + 1) / 2 + i];
        hh[i] = d != 0.0 ? v / d : 0.0;
        if (!isfinite(hh[i])) flags |= RBL_FLAG_NONFINITE;
      }
    }
    __syncthreads();
    for (int i = t; i < nsys; i += SGT) {
      double a = 0.0;
      if constexpr (V32) { for (int k = 0; k < used; ++k) a = __builtin_fma(hh[k], Vb[(unsigned)(k * nsys + i)], a); }
      else for (int k = 0; k < used; ++k) a = __builtin_fma(hh[k], Vb[(size_t)k * nsys + i], a);
      vw[i] = a;
    }
    __syncthreads();
    apply_PC(vw, vz);
    if constexpr (JOINTS) {                    // phi's component along an axis joint's axis is zero; GMRES leaves rounding there (k_jt_across)
      if (t < nj && jkind[t] == JT_AXIS) jt_across(jl + 6 * t, vz[nsb + 3 * t], vz[nsb + 3 * t + 1], vz[nsb + 3 * t + 2]);
      __syncthreads();
    }
    if constexpr (MIXED) {
      for (int i = t; i < nsys; i += SGT) A.x[i] = vz[i];
    } else {
      for (int i = t; i < nsys; i += SGT) A.x[i] = A.x0 ? A.x0[i] + vz[i] : vz[i];
    }
  } else {
    if constexpr (MIXED) {
      for (int i = t; i < nsys; i += SGT) { A.x[i] = 0.0; vz[i] = 0.0; }
    } else {
      for (int i = t; i < nsys; i += SGT) A.x[i] = A.x0 ? A.x0[i] : 0.0;
    }
  }
  if constexpr (MIXED) {   // the split: U solved (free) or echoed (prescribed); F echoed (free: the load that entered the right-hand
    __syncthreads();       // side) or -K_b^T lambda (prescribed), the blobs of the body added in order
    if (t < N) {
      const double v0 = vz[3 * t], v1 = vz[3 * t + 1], v2 = vz[3 * t + 2];
      const double l0 = lev[3 * t], l1 = lev[3 * t + 1], l2 = lev[3 * t + 2];
      kt[t] = v0; kt[N + t] = v1; kt[2 * N + t] = v2;
      kt[3 * N + t] = l1 * v2 - l2 * v1; kt[4 * N + t] = l2 * v0 - l0 * v2; kt[5 * N + t] = l0 * v1 - l1 * v0;
    }
    __syncthreads();
    if (t < nb6) {
      const int b = t / 6, c = t - 6 * b;
      const double *p = kt + (size_t)c * N + (size_t)b * nbl;
      double f = 0.0;
      for (int k = 0; k < nbl; ++k) f += p[k];
      // [U | F | x] of the masked rbl_launch_gmres_small_ens, as where the right-hand side is loaded above
      double *Uo = A.x - (size_t)blockIdx.x * nsys - 2 * (size_t)A.reps * nb6 + (size_t)blockIdx.x * nb6, *Fo = Uo + (size_t)A.reps * nb6;
      if (NLs[NS * b + RS * c + 6] != 0.0) Fo[t] = -f;
      else Uo[t] = vz[n3 + t];
    }
  }
  if constexpr (MIXED || JOINTS) {
    if (t == 0) { *A.iters_out = used; *A.resid_out = sc[2]; }
  } else {
    if (t == 0) { *A.iters_out = used; *A.resid_out = resid; }
  }
  if (flags) atomicOr(A.err, flags);
}

}  // namespace

// LDS of the vectors beside the Krylov basis, and of the basis: what the launcher and the fits predicates add up (constexpr: the
// CPU tests hold them against their restatement at compile time)
// n_joints > 0 (the jointed solve): every vector is 3 n_joints longer, and the joint data stand behind them -- 16 n_joints doubles
// of lever arms, redundant rows, gaps, sigmas and the diagonal of S, 2 (3 n_joints)^2 for S's factor and S^-1, and the integers
// (2 + 1 per joint, N_bod + 1 row starts, at most 4 per joint for the joint ends) two to a double
constexpr size_t small_jt_doubles(int N_bod, int n_joints)
{
  const size_t nj = (size_t)n_joints;
  return n_joints > 0 ? 16 * nj + 18 * nj * nj + (7 * nj + (size_t)N_bod + 2) / 2 : 0;
}
constexpr size_t small_lds_base_bytes(int N_blb, int N_bod, int max_iter, bool mixed = false, int n_joints = 0)
{
  const size_t N = (size_t)N_blb * N_bod, n3 = 3 * N, nb6 = 6 * (size_t)N_bod, nsys = n3 + nb6 + 3 * (size_t)n_joints, m = (size_t)max_iter;
  return sizeof(double) * (2 * n3 + 2 * N + N + 36 * (size_t)N_bod + 3 * nsys + nb6 + 3 * (m + 2) + 2 * m + 8 + (SGT / 64) * n3 + n3 + 6 * N +
                           (max_iter <= SG_RLDS ? m * (m + 1) / 2 : 0) + (mixed ? nb6 : 0) +    // mixed: the mask, one flag per row of NLs
                           small_jt_doubles(N_bod, n_joints));
}
constexpr size_t small_basis_bytes(int N_blb, int N_bod, int max_iter, int n_joints = 0)
{
  return sizeof(double) * (size_t)(max_iter + 1) * ((size_t)3 * N_blb * N_bod + (size_t)6 * N_bod + 3 * (size_t)n_joints);
}
// the global workspace of one replica (rbl_gmres_small_work_doubles): the Krylov basis, the packed triangular factor behind it, 8 spare
constexpr size_t small_work_doubles(int N_blb, int N_bod, int max_iter, int n_joints = 0)
{
  return small_basis_bytes(N_blb, N_bod, max_iter, n_joints) / sizeof(double) + (size_t)max_iter * (max_iter + 1) / 2 + 8;
}

// ---- the launcher of every variant ---------------------------------------------------------------------------------------------
// One workgroup per replica: S.reps systems of the same shape, replica r's X, Q, rhs, x0, x, workspace, iterations, residual and
// error word r strides further (err_stride = 0, S.reps = 1: the grid of one).  A arrives with what is the variant's own (mask,
// body_in, reps, per; the cell; the joint table) and gets everything else here; row: the variant's kernels for this wall flag,
// [0] with the Krylov basis in global memory, [1] with it in LDS.  n_joints > 0 (the jointed variant): rhs, x and every vector of the
// workspace hold 3 n_joints more per replica.  mixed: S.x is the x of ONE block [U | F | x] (rbl_internal.hpp: RblSmallEns)
template <class Args>
static int small_launch(hipStream_t st, const RblParams &P, const RblSmallEns &S, Args A, void (*const *row)(Args), bool mixed = false,
                        int n_joints = 0, const double *d_x0 = nullptr, double fsign = 1.0, int err_stride = 1)
{
  size_t lds = small_lds_base_bytes(S.N_blb, S.N_bod, S.max_iter, mixed, n_joints);
  if (!rbl_gmres_small_fits(S.N_blb, S.N_bod, S.max_iter, false) || 3 * (size_t)n_joints > (size_t)SGT || lds > SG_LDS_MAX) return RBL_ERR_SIZE;
  const size_t basis = small_basis_bytes(S.N_blb, S.N_bod, S.max_iter, n_joints);
  bool vlds = lds + basis <= SG_LDS_MAX;                   // the Krylov basis beside the vectors in LDS?
  A.X = S.X; A.Q = S.Q; A.cfg = S.cfg; A.rhs = S.rhs; A.x0 = d_x0; A.x = S.x;
  A.V = S.work; A.H = S.work + basis / sizeof(double);
  A.iters_out = S.iters; A.resid_out = S.resid; A.err = S.err;
  A.work_stride = small_work_doubles(S.N_blb, S.N_bod, S.max_iter, n_joints); A.err_stride = err_stride;
  A.P = P; A.N_blb = S.N_blb; A.N_bod = S.N_bod; A.max_iter = S.max_iter; A.rtol = S.rtol; A.fsign = fsign;
  // more than 64 KB of dynamic LDS needs the attribute (gfx950: 160 KB per CU).  If the runtime refuses the basis goes to
  // global memory; if even the vectors do not fit the caller falls back to the general solver (RBL_ERR_SIZE).
  auto allow = [&](bool v, size_t bytes) {
    if (bytes <= 64 * 1024) return true;
    if (hipFuncSetAttribute((const void *)row[v], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  };
  if (vlds && allow(true, lds + basis)) lds += basis;
  else {
    vlds = false;
    if (!allow(false, lds)) return RBL_ERR_SIZE;
  }
  hipLaunchKernelGGL(row[vlds], dim3((unsigned)S.reps), dim3(SGT), lds, st, A);
  return RBL_OK;
}
