// rbl_body_dev.hpp -- device helpers shared by the per-body kernels (rbl_body_dev.hip, rbl_mixed.hip, rbl_ensemble.hip): ONE copy
// of the K / K^T formulas, of the prescribed-mask decoding, of the quaternion's rotation, of the ordered workgroup sum and of the
// 6 x 6 substitution, so the kernels that restate a body's operators cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// rotation matrix (row-major) of a unit quaternion (w, x, y, z): lab = R body
__device__ __forceinline__ void quat_rot(const double *q, double *R)
{
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// update_X_Q of one body, c_rigid_obj.cpp:679-710 (the device restatement of rbl_body_update_X_Q): U displacement units.  The
// ensembles' update kernels and the Metropolis proposal (rbl_ens_mc.hip) move a body with this one sequence of operations
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

// (K_b u)_k = u_lin + u_ang x l_k    (reference c_rigid_obj.cpp:368-383, :404)
__device__ __forceinline__ void rbl_KU(const double *l, const double *u, double &k0, double &k1, double &k2)
{
  const double *om = u + 3;
  k0 = u[0] + l[2] * om[1] - l[1] * om[2];
  k1 = u[1] + l[0] * om[2] - l[2] * om[0];
  k2 = u[2] + l[1] * om[0] - l[0] * om[1];
}

// K_b^T v blob by blob: f += (v, l_k x v)     (:410)
__device__ __forceinline__ void rbl_KT_acc(const double *l, double v0, double v1, double v2, double (&f)[6])
{
  f[0] += v0; f[1] += v1; f[2] += v2;
  f[3] += l[1] * v2 - l[2] * v1;
  f[4] += l[2] * v0 - l[0] * v2;
  f[5] += l[0] * v1 - l[1] * v0;
}

// sums of NV values over a workgroup of NT threads (NT a power of two) by an LDS tree in one fixed order; every thread gets them
template <int NV, int NT>
__device__ __forceinline__ void rbl_block_sum(double (&v)[NV], double (*s)[NT], int t)
{
#pragma unroll
  for (int q = 0; q < NV; ++q) s[q][t] = v[q];
  __syncthreads();
  for (int st = NT / 2; st > 0; st >>= 1) {
    if (t < st) {
#pragma unroll
      for (int q = 0; q < NV; ++q) s[q][t] += s[q][t + st];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = s[q][0];
  __syncthreads();
}

// A body's prescribed-mask as a bit set (bit c: velocity component c prescribed), the ONE decoding every kernel uses.
// per = mask entries per body: 6 (one per component), or 1 (whole bodies: no bit or all six).  This form is per lane: for the
// kernels with one thread per body, whose lanes hold different bodies (never broadcast its result)
__device__ __forceinline__ unsigned mx_lane_bits(const uint8_t *__restrict__ mask, int per, size_t b)
{
  unsigned pm = 0;
  if (per == 6) {
    const uint8_t *m = mask + 6 * b;
#pragma unroll
    for (int c = 0; c < 6; ++c) pm |= (m[c] != 0 ? 1u : 0u) << c;
  } else {
    pm = mask[b] != 0 ? 63u : 0u;
  }
  return pm;
}

// the same for the kernels with one workgroup per body b: one scalar, so every branch on it is uniform
__device__ __forceinline__ unsigned mx_bits(const uint8_t *__restrict__ mask, int per, int b)
{
  return (unsigned)__builtin_amdgcn_readfirstlane((int)mx_lane_bits(mask, per, (size_t)b));
}

// u = (L L^T)^-1 g for a 6 x 6 lower Cholesky factor L, row-major (the per-body N = K^T invM K of the preconditioners, :601-608)
__device__ __forceinline__ void rbl_chol6_solve(const double *L, const double *g, double *u)
{
  double y[6];
  for (int p = 0; p < 6; ++p) {
    double v = g[p];
    for (int q = 0; q < p; ++q) v -= L[6 * p + q] * y[q];
    y[p] = v / L[6 * p + p];
  }
  for (int p = 5; p >= 0; --p) {
    double v = y[p];
    for (int q = p + 1; q < 6; ++q) v -= L[6 * q + p] * u[q];
    u[p] = v / L[6 * p + p];
  }
}
