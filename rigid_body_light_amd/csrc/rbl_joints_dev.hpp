// rbl_joints_dev.hpp -- device pieces of the hard joints (include/rbl.h section 9) shared by the single-context kernels of
// rbl_joints.hip and the one-kernel jointed solve of the ensembles (rbl_small_joints.hip): the joint table as the kernels take
// it, the lever arms, the angular gap, the geometry of one joint and the rotation half of a joint end's rows.  Everything is
// inline and lives in an unnamed namespace: each translation unit gets its own copy, under the names rbl_joints.hip had for them.
#pragma once
#include "rbl_body_dev.hpp"
#include "rbl_internal.hpp"

namespace {

constexpr int JT_MAX = 2048;                             // joints a context takes: S is dense, a column of it lives in LDS (48 KB)
// a pivot d of the factor of S counts as lost when d^2 <= JT_PIVOT_TOL S_ii.  What an exactly redundant constraint leaves of its
// pivot is rounding, some 1e-16 S_ii (S couples a joint to the few that share its bodies: the sums are short), and as often
// positive as not; an independent constraint leaves the squared sine of the angle it makes with the others.  The two joints of a
// hinge are independent only through their gaps (sine ~ gap / distance of the anchors), and a step with gamma = 1 keeps those at
// O(dt^2): the bound sits two orders above rounding and no higher, so that such a hinge still solves
constexpr double JT_PIVOT_TOL = 1e-14;

// the joints as the kernels take them (by value).  anchor: s_A | s_B (or the lab point P) per joint; ends: (joint, which end) per
// entry of the CSR by body
struct JtDev {
  const double *anchor;
  const int *body, *rows, *ptr, *ends, *mate;            // mate: (the other joint of the same pair of bodies or -1, its ends swapped?)
  int n, n_rows;
  // a set with angular joints (the KINDS instantiations; NULL otherwise).  ang: axis a (unit, in A's frame) | q_rel per joint;
  // ninv: the per-body N^-1 of the solve under way (k_jt_ninv), for an axis joint's sigma
  const int *kind;
  const double *ang, *theta, *rate, *ninv;
};

constexpr int JT_BALL = RBL_JOINT_BALL, JT_LOCK = RBL_JOINT_LOCK, JT_AXIS = RBL_JOINT_AXIS;

// two joints between one pair of bodies (a hinge) count as closed when the two anchors are as far apart on one body as on the
// other to within this, relative: |dA - dB| <= JT_HINGE_CLOSED |dA|.  Their common row -- the distance between the anchors,
// fixed by either body alone -- is then redundant to 1e-12 of the others
constexpr double JT_HINGE_CLOSED = 1e-6;

// l = R(Q_b) s
__device__ __forceinline__ void jt_lab(const double *__restrict__ Q, const double *__restrict__ s, int b, double (&l)[3])
{
  double R[9];
  quat_rot(Q + 4 * (size_t)b, R);
#pragma unroll
  for (int c = 0; c < 3; ++c) l[c] = R[3 * c] * s[0] + R[3 * c + 1] * s[1] + R[3 * c + 2] * s[2];
}

// the lever arms of joint j's two ends (l_B = 0 for a pivot)
__device__ __forceinline__ void jt_levers(const double *__restrict__ Q, const JtDev &J, int j, double (&lA)[3], double (&lB)[3])
{
  const double *s = J.anchor + 6 * (size_t)j;
  const int b = J.body[2 * (size_t)j + 1];
  jt_lab(Q, s, J.body[2 * (size_t)j], lA);
  if (b >= 0) jt_lab(Q, s + 3, b, lB);
  else lB[0] = lB[1] = lB[2] = 0.0;
}

// Hamilton product of two quaternions (w, x, y, z): R(p q) = R(p) R(q)
__device__ __forceinline__ void jt_qmul(const double (&p)[4], const double (&q)[4], double (&o)[4])
{
  o[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3];
  o[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
  o[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1];
  o[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

// v -= ah (ah . v): the part of v across the unit vector ah
__device__ __forceinline__ void jt_across(const double *__restrict__ ah, double &v0, double &v1, double &v2)
{
  const double d = ah[0] * v0 + ah[1] * v1 + ah[2] * v2;
  v0 -= ah[0] * d; v1 -= ah[1] * d; v2 -= ah[2] * d;
}

// sigma of an axis joint: the eigenvalue its free row gets in the operator and in S -- the mean rotational entry of N^-1 of its body A
__device__ __forceinline__ double jt_sigma(const double *__restrict__ Ninv, int a)
{
  const double *Nb = Ninv + 36 * (size_t)a;
  return (Nb[21] + Nb[28] + Nb[35]) * (1.0 / 3.0);
}

// An angular joint (lock or axis): ah = R(Q_A) a, its axis in the lab frame, and the angular gap e, the lab-frame rotation vector
// of Q_B* Q_B^-1 with the target Q_B* = Q_A rot(theta a) q_rel (theta: a lock's motor angle, 0 for an axis joint), the short way
// round, so that de/dt = w_A - w_B to first order.  An axis joint keeps the part of e across ah.  Q_B = identity for the lab
__device__ __forceinline__ void jt_angular(const double *__restrict__ Q, const JtDev &J, int j, int a, int b, double (&ah)[3], double (&e)[3])
{
  const double *g = J.ang + 7 * (size_t)j;
  const int kind = J.kind[j];
  jt_lab(Q, g, a, ah);
  const double half = kind == JT_LOCK ? 0.5 * J.theta[j] : 0.0, sn = sin(half);
  const double r[4] = {cos(half), sn * g[0], sn * g[1], sn * g[2]};
  const double qa[4] = {Q[4 * (size_t)a], Q[4 * (size_t)a + 1], Q[4 * (size_t)a + 2], Q[4 * (size_t)a + 3]};
  const double qr[4] = {g[3], g[4], g[5], g[6]};
  double qbc[4] = {1.0, 0.0, 0.0, 0.0}, t1[4], t2[4], d[4];
  if (b >= 0) {
    qbc[0] = Q[4 * (size_t)b]; qbc[1] = -Q[4 * (size_t)b + 1]; qbc[2] = -Q[4 * (size_t)b + 2]; qbc[3] = -Q[4 * (size_t)b + 3];
  }
  jt_qmul(qa, r, t1);
  jt_qmul(t1, qr, t2);
  jt_qmul(t2, qbc, d);
  const double sg = d[0] < 0.0 ? -1.0 : 1.0;
  const double vn = sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
  const double sc = vn > 0.0 ? sg * 2.0 * atan2(vn, sg * d[0]) / vn : 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) e[c] = sc * d[1 + c];
  if (kind == JT_AXIS) jt_across(ah, e[0], e[1], e[2]);
}

// Joint j's geometry (the body of k_jt_geom, one lane per joint): lev = l_A | l_B per joint, gap = p_A - p_B, and gau = the
// joint's three entries of its hinge's redundant row (zero: none; gau NULL: not wanted).
// Two joints lo < hi between one pair of bodies hold the points A1, A2 of one body on the points B1, B2 of the other; when the
// hinge is closed (JT_HINGE_CLOSED; two pivots on one body: always, the lab points do not move) the combination
// d . (rows of lo) - d . (rows of hi), d the unit vector from A2 to A1, is the rate of |A1 - A2|^2 - |B1 - B2|^2: zero whatever
// the bodies do.  gau_lo = d, gau_hi = -d (+d when hi names the two bodies in the other order): k_jt_schur takes this direction
// out of the null space of S.
// KINDS (a set with angular joints): a lock or axis joint leaves lev = ah | 0, gap = e (jt_angular) and gau = 0
template <bool KINDS>
__device__ __forceinline__ void jt_geom_joint(const double *__restrict__ X, const double *__restrict__ Q, const JtDev &J, int j,
                                              double *__restrict__ lev, double *__restrict__ gap, double *__restrict__ gau)
{
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

// W = -[l]x, the rotation half of a joint end's three rows of J: (w x l)_r = sum_m W[r][m] w_m  (rbl_KU's formula)
__device__ __forceinline__ void jt_W(const double *__restrict__ l, double (&W)[3][3])
{
  W[0][0] = 0.0;   W[0][1] = l[2];  W[0][2] = -l[1];
  W[1][0] = -l[2]; W[1][1] = 0.0;   W[1][2] = l[0];
  W[2][0] = l[1];  W[2][1] = -l[0]; W[2][2] = 0.0;
}

// the rotation half W of G = [a I  W] of a joint's end (lv: the joint's six values of lev) -> a: a ball end 1 and -[l]x, a lock
// end 0 and I, an axis end 0 and P = I - ah ah^T
__device__ __forceinline__ double jt_G(int kind, const double *__restrict__ lv, int end, double (&W)[3][3])
{
  if (kind == JT_BALL) { jt_W(lv + 3 * end, W); return 1.0; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) W[r][c] = (r == c ? 1.0 : 0.0) - (kind == JT_AXIS ? lv[r] * lv[c] : 0.0);
  return 0.0;
}

// Row r of G = [a I  W] of a joint's end as six numbers, chosen by selects (no indexed register array): what a thread that owns
// ONE entry of J N^-1 J^T, or one component of J U or J^T phi, needs of jt_G
__device__ __forceinline__ void jt_G_row(int kind, const double *__restrict__ lv, int end, int r, double (&g)[6])
{
  const double e0 = r == 0 ? 1.0 : 0.0, e1 = r == 1 ? 1.0 : 0.0, e2 = r == 2 ? 1.0 : 0.0;
  if (kind == JT_BALL) {
    const double *l = lv + 3 * end;
    g[0] = e0; g[1] = e1; g[2] = e2;
    g[3] = r == 0 ? 0.0 : r == 1 ? -l[2] : l[1];
    g[4] = r == 0 ? l[2] : r == 1 ? 0.0 : -l[0];
    g[5] = r == 0 ? -l[1] : r == 1 ? l[0] : 0.0;
    return;
  }
  const double ar = kind == JT_AXIS ? (r == 0 ? lv[0] : r == 1 ? lv[1] : lv[2]) : 0.0;
  g[0] = g[1] = g[2] = 0.0;
  g[3] = e0 - ar * lv[0]; g[4] = e1 - ar * lv[1]; g[5] = e2 - ar * lv[2];
}

}   // namespace
