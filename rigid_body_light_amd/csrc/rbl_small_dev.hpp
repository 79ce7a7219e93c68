// rbl_small_dev.hpp -- device pieces shared by the one-workgroup kernels of small systems: the one-kernel GMRES solve
// (rbl_small.hip) and the ensemble's random-finite-difference product (rbl_ensemble.hip).  Both evaluate B M B v of at most
// 256 blobs held in LDS with one workgroup of RBL_SG_THREADS threads.
#pragma once
#include "rbl_internal.hpp"

constexpr int RBL_SG_THREADS = 1024;

// the pair kernels' constants for positions given in units of a (rbl_pair_accum / rbl_pair_symv, scaled by nf afterwards)
// (RBL_UNIT_RADIUS: the one-workgroup kernels keep the radius as their length unit -- their LDS positions and cell tables serve the
// joints, the forces and the damping in radii as well, and a kernel that waits on barriers and launch latency has no use for the
// instruction the shared unit of the large products saves)
__device__ __forceinline__ RblParams rbl_small_unit_params(const RblParams &P)
{
  return {1.0, 1.0, P.nf, 4.0, 1e-24, -0.375, 0.125, 0};
}

// unit quaternion (scalar-first) -> row-major rotation, the expansion of k_blob_positions / rbl_quat_to_rot
__device__ __forceinline__ void rbl_quat_rot9(const double *q, double *R)
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

// The off-diagonal part of the product with the damped vector d v: every unordered pair once (M_ji = M_ij^T, rbl_pair_symv).
// Step (s, rb) pairs the rows i = 64 rb + lane with the columns j = i + s (mod N), s = 1 .. N/2 (for even N the offset N/2
// only from the lower half), so the 64 lanes of a wavefront touch 64 different rows and 64 different columns per step; the
// steps are dealt round-robin to the wavefronts, each adding into its OWN accumulator set part[wave][3N] (fixed order inside
// a wave).  The caller adds the sets in wave order.  pos: positions / a (3N), dmp: wall damping per blob (WALL only), in: 3N.
// Every thread of the workgroup calls it (it contains barriers); part holds NW x 3N doubles and is zeroed here.
//
// PER (a periodic cell, include/rbl.h sections 5 and 10; wall only): every unordered pair once per image,
//     U_i += sum_{|p| <= nx} sum_{|q| <= ny} B(d0 + (p Lx, q Ly, 0); z_i, z_j) F_j      and the transpose into U_j,
// d0 the nearest-image displacement formed as sweep_tile_per forms it (rbl_kernels.hip): M_ji = M_ij^T holds image by image
// because the image set is symmetric and rint is odd.  The image is folded into the step index: a wave's step is (offset s, row
// block, image k = (p + nx)(2 ny + 1) + (q + ny)), dealt round-robin as before, so the (2 nx + 1)(2 ny + 1)-fold sweep spreads
// evenly over the waves and nothing but the step's three scalars is live across the pair call; the reduction is redone per step.
// A blob's own images (p, q) != (0, 0) are ordinary pairs of two different blobs at one height: the steps behind the pairs',
// offset 0, take the half set k > k(0, 0) -- (p, q) and (-p, -q) are each other's transpose, so ui + uj of one evaluation is both.
// The step index comes through readfirstlane: the decoding below is scalar arithmetic.  C arrives as a kernel argument or, with a
// cell per replica, from the workgroup's record of a table that is only read (rbl_small_cells.hip): scalar registers either way,
// and W, kc, NI, npair, nall are then the workgroup's own -- a replica with more images runs more steps.
template <bool WALL, bool PER = false>
__device__ __forceinline__ void rbl_small_pair_sweep(const RblParams &Pu, const double *pos, const double *dmp, const double *in,
                                                     int N, double *part, unsigned &flags, const RblSmallCell &C = RblSmallCell{})
{
  static_assert(WALL || !PER, "the free-space lattice sum diverges: a cell needs the wall");
  constexpr int NW = RBL_SG_THREADS / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n3 = 3 * N;
  for (int idx = t; idx < NW * n3; idx += RBL_SG_THREADS) part[idx] = 0.0;
  __syncthreads();
  const int RB = (N + 63) / 64, nsteps = (N / 2) * RB;
  double *acc = part + (size_t)wave * n3;
  if constexpr (PER) {
    const int W = 2 * C.ny + 1, kc = C.nx * W + C.ny, NI = 2 * kc + 1;
    const int npair = nsteps * NI, nall = npair + RB * kc;
    for (int q = __builtin_amdgcn_readfirstlane(wave); q < nall; q += NW) {
      int s_, rb, k;
      if (q < npair) {                                 // a pair's image: image innermost, then the row block, then the offset
        const int u = q / NI;
        k = q - u * NI;
        s_ = u / RB + 1;
        rb = u - (s_ - 1) * RB;
      } else {                                         // a blob's own image, k(0, 0) < k < NI
        const int u = q - npair, kk = u / RB;
        k = kc + 1 + kk;
        rb = u - kk * RB;
        s_ = 0;
      }
      const int kp = k / W;
      const double pd = (double)(kp - C.nx), qd = (double)(k - kp * W - C.ny);
      const int i = rb * 64 + lane;
      if (i < N && (2 * s_ != N || 2 * i < N)) {
        int j = i + s_;
        if (j >= N) j -= N;
        const double di = dmp[i], dj = dmp[j];
        const RblV3 Fi[1] = {{di * in[3 * i], di * in[3 * i + 1], di * in[3 * i + 2]}}, Fj[1] = {{dj * in[3 * j], dj * in[3 * j + 1], dj * in[3 * j + 2]}};
        RblV3 ui[1] = {{0.0, 0.0, 0.0}}, uj[1] = {{0.0, 0.0, 0.0}};
        double dx = pos[3 * i] - pos[3 * j], dy = pos[3 * i + 1] - pos[3 * j + 1];
        dx = __builtin_fma(-C.Lx, rint(dx * C.iLx), dx);   // 1 / L is 0 on an open axis: rint(0) = 0 leaves d alone
        dy = __builtin_fma(-C.Ly, rint(dy * C.iLy), dy);
        rbl_pair_symv<true, RBL_UNIT_RADIUS, true>(Pu, __builtin_fma(pd, C.Lx, dx), __builtin_fma(qd, C.Ly, dy), pos[3 * i + 2], Fi, 0.0, 0.0, pos[3 * j + 2], Fj, ui, uj, flags);
        if (s_ == 0) {                                 // wave-uniform: j = i, image and mirror image in one
          ui[0].x += uj[0].x; ui[0].y += uj[0].y; ui[0].z += uj[0].z;
        }
        __hip_atomic_fetch_add(&acc[3 * i], ui[0].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&acc[3 * i + 1], ui[0].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&acc[3 * i + 2], ui[0].z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (s_ != 0) {
          __hip_atomic_fetch_add(&acc[3 * j], uj[0].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(&acc[3 * j + 1], uj[0].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(&acc[3 * j + 2], uj[0].z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
    __syncthreads();
    return;
  }
  for (int q = wave; q < nsteps; q += NW) {
    const int s_ = q / RB + 1, i = (q - (s_ - 1) * RB) * 64 + lane;
    if (i < N && (2 * s_ != N || 2 * i < N)) {
      int j = i + s_;
      if (j >= N) j -= N;
      const double di = WALL ? dmp[i] : 1.0, dj = WALL ? dmp[j] : 1.0;
      const RblV3 Fi[1] = {{di * in[3 * i], di * in[3 * i + 1], di * in[3 * i + 2]}}, Fj[1] = {{dj * in[3 * j], dj * in[3 * j + 1], dj * in[3 * j + 2]}};
      RblV3 ui[1] = {{0.0, 0.0, 0.0}}, uj[1] = {{0.0, 0.0, 0.0}};
      rbl_pair_symv<WALL, RBL_UNIT_RADIUS, true>(Pu, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], Fi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], Fj, ui, uj, flags);
      __hip_atomic_fetch_add(&acc[3 * i], ui[0].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&acc[3 * i + 1], ui[0].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&acc[3 * i + 2], ui[0].z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&acc[3 * j], uj[0].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&acc[3 * j + 1], uj[0].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&acc[3 * j + 2], uj[0].z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
}
