// rbl_ens_mc.hip -- Metropolis sampling of the force model on an ensemble (include/rbl.h section 5, rbl_ensemble_mc).
//
// One kernel, k_ens_mc: one workgroup of 256 lanes per replica, the whole chain of a launch inside it.  In LDS: the replica's blob
// positions (<= 256; the type rides in the fourth slot, as in k_blob_interactions_typed), body centres and quaternions (the
// committed set and the set with the trial in place, which the bond evaluation reads), the reference shape, the 36 typed-table
// descriptors and the lists of a trial.  The replica's cell record is read once, at the workgroup-uniform index r.  A trial touches
// global memory only for table coefficients and bond data (through L1 / L2, as the force kernels do) and for trace and frame writes.
//
// Per trial of body b: every lane draws the proposal and updates the body redundantly (the same operations on the same numbers:
// one result); lane k < N_blb writes blob k's new position to LDS and votes on the wall; wave 0 compacts the bodies inside the
// exact body-level cull of k_body_neighbours (centre within 2 R_body + r_cut of the old OR the new centre of b) into a list in
// increasing body index; the (blob of b) x (blob of a listed body) pairs are dealt over the lanes by their flat index, lane t
// taking t, t + 256, ..., and each lane adds U(r_new) - U(r_old) of its pairs, then of its blob's single-blob terms, of the trap
// (lane 0) and of its bond ends in registers; rbl_block_sum adds the lanes in one fixed tree; every lane takes the same verdict
// and lane k commits blob k.  No atomics on doubles, one summation order, no scratch: a launch is bitwise reproducible, and since
// the running state (configuration, counters, energy) passes between launches in full, so is any split of a chain into launches.
// The energy expressions are the force kernels' own (rbl_forces_dev.hpp); Philox and the body update are k_normal's and the steps'.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"
#include "rbl_forces_dev.hpp"
#include "rbl_philox.hpp"

namespace {

constexpr int MT = 256;               // lanes of the workgroup
constexpr int MC_NMAX = 256;          // blobs of a replica (the one-kernel solver's bound, rbl_ensemble_set_config)
constexpr int MC_BMAX = 64;           // bodies of a replica
constexpr int MC_TRACE = 10;          // doubles per trace row

// one launch: sweeps s0 .. s0 + ns - 1 of the call (global index sweep_start + ...)
struct McArgs {
  const double *Xs, *Qs;              // the configuration the launch starts from
  double *Xd, *Qd;                    // ... and leaves (may be Xs, Qs: a workgroup reads all of its replica first)
  const double *cfg;
  const double *e_blob;               // first launch: the per-blob energies of the evaluation before the chain
  const double *kBT; const uint8_t *frozen;
  long long *cnt;                     // tried | accepted | wall_rejected, 3 per replica
  double *E;                          // energy_start | running energy, 2 per replica
  unsigned *rerr;
  double *fX, *fQ, *fE, *trace;
  uint64_t seed;
  long long sweep_start, s0;
  double step_x, step_t;
  int ns, first, R, Nb, nbl, wall, kBT_sets, frozen_sets, stride, n_trace, replica_base;
};

// energy of one blob pair at the displacement (dx, dy, dz): every pair term that is on, each inside its own cutoff (the tests of
// k_blob_interactions_typed); ti, tj: the two types (typed only)
__device__ __forceinline__ double mc_pair_U(const IaMcModel &M, const IaCell &C, const IaTabLds *sd, int ti, int tj, double dx, double dy,
                                            double dz)
{
  if (M.per) ia_min_image(C, dx, dy);
  const double r2 = dx * dx + dy * dy + dz * dz;
  if (r2 > M.Y.cmax2) return 0.0;                        // beyond every cutoff that is on
  const double r = sqrt(r2);
  double U = 0.0;
  if (r2 <= M.p.rc2) {
    double g;
    ia_steric(M.p, r, U, g);
  }
  if ((M.tab & 1) && r <= M.PT.hi) {
    double Ut, dUt;
    ia_tab_eval(M.PT, r, Ut, dUt);
    U += Ut;
  }
  if (M.typed) {
    const IaTab &TT = sd[ia_type_pair(ti, tj)].T;
    if (r <= TT.hi) {
      double Ut, dUt;
      ia_tab_eval(TT, r, Ut, dUt);
      U += Ut;
    }
  }
  return U;
}

// the single-blob terms at height z: weight, wall repulsion, height table
__device__ __forceinline__ double mc_blob_U(const IaMcModel &M, double z)
{
  double U = M.p.w * z;
  if (M.p.wall) {
    double Uw, Fw;
    ia_wall(M.p, z, Uw, Fw);
    U += Uw;
  }
  if ((M.tab & 2) && z <= M.HT.hi) {
    double Uh, dUh;
    ia_tab_eval(M.HT, z, Uh, dUh);
    U += Uh;
  }
  return U;
}

// the trap of global body i at the centre X (k_body_traps' expression)
__device__ __forceinline__ double mc_trap_U(const IaMcModel &M, int i, const double *X)
{
  const size_t j = (size_t)(i % M.tr_per);
  double E = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double k = M.tr_k[3 * j + c], d = X[c] - M.tr_X0[3 * j + c];
    if (k != 0.0) E += 0.5 * k * d * d;
  }
  return E;
}

// quat_rot's expressions with contraction off.  The kernel forms a body's rotation at two places -- when a launch loads a replica and
// when a trial proposes -- and a launch that continues a chain must rebuild, from the committed (X, Q), the very blob positions the
// trial committed: with contraction left to the compiler the two inlined copies may fuse differently and the split of a chain into
// launches would show in the last bits of the energies
__device__ __forceinline__ void mc_quat_rot(const double *q, double *R)
{
#pragma clang fp contract(off)
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// blob k of a body at (X, rotation Rm): k_body_geom's arithmetic (the lever arm with contraction off, then + X), so the heights the
// wall test sees are the ones the next step's kernels will see
__device__ __forceinline__ void mc_blob_pos(const double *X, const double *Rm, const double *c, double *p)
{
#pragma clang fp contract(off)
  const double l0 = c[0] * Rm[0] + c[1] * Rm[1] + c[2] * Rm[2];
  const double l1 = c[0] * Rm[3] + c[1] * Rm[4] + c[2] * Rm[5];
  const double l2 = c[0] * Rm[6] + c[1] * Rm[7] + c[2] * Rm[8];
  p[0] = l0 + X[0]; p[1] = l1 + X[1]; p[2] = l2 + X[2];
}

__global__ __launch_bounds__(MT) void k_ens_mc(McArgs A, IaMcModel M)
{
  __shared__ double s_pos[MC_NMAX][4];
  __shared__ double s_new[MC_NMAX][3];
  __shared__ double s_cfg[MC_NMAX][3];
  __shared__ double s_X[MC_BMAX * 3], s_Q[MC_BMAX * 4], s_Xn[MC_BMAX * 3], s_Qn[MC_BMAX * 4];
  __shared__ IaTabLds s_desc[IA_TY_PAIRS];
  __shared__ double s_red[1][MT];
  __shared__ int s_list[MC_BMAX], s_row[MC_BMAX];
  __shared__ int s_nact;
  __shared__ double s_E0;
  const int r = blockIdx.x, t = threadIdx.x;
  const int Nb = A.Nb, nbl = A.nbl, N = Nb * nbl;
  if (!A.first && A.rerr[r]) return;                     // the first launch refused this replica's start: nothing moves
  const size_t g0 = (size_t)r * Nb;
  for (int u = t; u < 3 * nbl; u += MT) s_cfg[u / 3][u % 3] = A.cfg[u];
  for (int u = t; u < 3 * Nb; u += MT) s_X[u] = s_Xn[u] = A.Xs[3 * g0 + u];
  for (int u = t; u < 4 * Nb; u += MT) s_Q[u] = s_Qn[u] = A.Qs[4 * g0 + u];
  if (M.typed)
    for (int u = t; u < IA_TY_PAIRS; u += MT) s_desc[u].T = M.Y.desc[u];
  if (t < MC_BMAX) s_row[t] = -1;
  __syncthreads();
  if (M.bonds)
    for (int u = t; u < M.B.n_rows; u += MT) {
      const int i = M.B.rows[u];
      if (i >= 0 && i < Nb) s_row[i] = u;
    }
  IaCell C = M.C;
  if (M.per == 2) C = ia_cell_of(M.cells, r);
  int below = 0;
  if (t < N) {
    const int b = t / nbl, k = t - b * nbl;
    double Rm[9];
    mc_quat_rot(&s_Q[4 * b], Rm);
    mc_blob_pos(&s_X[3 * b], Rm, s_cfg[k], s_pos[t]);
    const int ty = M.typed ? M.Y.type[(size_t)(M.Y.per_row ? b : 0) * nbl + k] : 0;
    s_pos[t][3] = __hiloint2double(0, ty);
    below = A.wall && s_pos[t][2] < 0.0;
  }
  if (A.first) {
    if (__syncthreads_or(below)) {                       // RBL_FLAG_BELOW_WALL at the start: the replica is refused
      if (t == 0) A.rerr[r] = (unsigned)RBL_FLAG_BELOW_WALL;
      return;
    }
    if (t == 0) {                                        // the evaluation's blob energies in blob order, as the host adds them
      double E = 0.0;
      for (int i = 0; i < N; ++i) E += A.e_blob[(size_t)r * N + i];
      s_E0 = E;
      A.E[2 * (size_t)r] = E;
    }
    for (int u = t; u < A.n_trace * MC_TRACE; u += MT) A.trace[(size_t)r * A.n_trace * MC_TRACE + u] = -1.0;
  }
  __syncthreads();
  double E_run = A.first ? s_E0 : A.E[2 * (size_t)r + 1];
  long long tried = A.cnt[3 * (size_t)r], accepted = A.cnt[3 * (size_t)r + 1], wall_rej = A.cnt[3 * (size_t)r + 2];
  const double kT = A.kBT[A.kBT_sets == 1 ? 0 : r];
  const uint8_t *frozen = A.frozen ? A.frozen + (size_t)(A.frozen_sets == 1 ? 0 : r) * Nb : nullptr;
  const int nn = nbl * nbl;
  const double u_scale = 1.0 / 4294967296.0;

  for (int s = 0; s < A.ns; ++s) {
    const long long sc = A.s0 + s;                       // the call's sweep
    const uint64_t S = (uint64_t)(A.sweep_start + sc);   // the global one
    for (int b = 0; b < Nb; ++b) {
      if (frozen && frozen[b]) continue;
      // the proposal, by every lane
      uint32_t c0[4] = {(uint32_t)S, (uint32_t)(S >> 32), (uint32_t)(A.replica_base + r), 0x4D430000u | (uint32_t)b};
      uint32_t c1[4] = {(uint32_t)S, (uint32_t)(S >> 32), (uint32_t)(A.replica_base + r), 0x4D430100u | (uint32_t)b};
      philox4x32_10(c0, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
      philox4x32_10(c1, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
      double d[6];
#pragma unroll
      for (int q = 0; q < 3; ++q) d[q] = A.step_x * (2.0 * (((double)c0[q] + 0.5) * u_scale) - 1.0);
      d[3] = A.step_t * (2.0 * (((double)c0[3] + 0.5) * u_scale) - 1.0);
      d[4] = A.step_t * (2.0 * (((double)c1[0] + 0.5) * u_scale) - 1.0);
      d[5] = A.step_t * (2.0 * (((double)c1[1] + 0.5) * u_scale) - 1.0);
      const double u6 = ((double)c1[2] + 0.5) * u_scale;
      double Xo[3] = {s_X[3 * b], s_X[3 * b + 1], s_X[3 * b + 2]};
      double Qo[4] = {s_Q[4 * b], s_Q[4 * b + 1], s_Q[4 * b + 2], s_Q[4 * b + 3]};
      double Xn[3], Qn[4], Rm[9];
      ens_update_body(Xo, Qo, d, Xn, Qn);
      mc_quat_rot(Qn, Rm);
      int bad = 0;
      if (t < nbl) {
        double p[3];
        mc_blob_pos(Xn, Rm, s_cfg[t], p);
        s_new[t][0] = p[0]; s_new[t][1] = p[1]; s_new[t][2] = p[2];
        bad = A.wall && p[2] < 0.0;
      }
      if (t == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) s_Xn[3 * b + q] = Xn[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) s_Qn[4 * b + q] = Qn[q];
      }
      // the bodies inside the cull, in increasing index (wave 0; Nb <= 64)
      if (t < 64) {
        bool take = false;
        if (t < Nb && t != b && M.Y.cmax2 >= 0.0) {
          take = true;
          if (M.cull) {
            double ax = s_X[3 * t] - Xo[0], ay = s_X[3 * t + 1] - Xo[1];
            double bx = s_X[3 * t] - Xn[0], by = s_X[3 * t + 1] - Xn[1];
            const double az = s_X[3 * t + 2] - Xo[2], bz = s_X[3 * t + 2] - Xn[2];
            if (M.per) { ia_min_image(C, ax, ay); ia_min_image(C, bx, by); }
            take = ax * ax + ay * ay + az * az <= M.cull2 || bx * bx + by * by + bz * bz <= M.cull2;
          }
        }
        const unsigned long long m = __ballot(take);
        if (take) s_list[__popcll(m & ((1ull << t) - 1ull))] = t;
        if (t == 0) s_nact = __popcll(m);
      }
      const int wall_hit = __syncthreads_or(bad);        // (the barrier that publishes s_new, s_Xn, s_Qn and the list)
      double dE = 0.0;
      int verdict = 2;
      if (!wall_hit) {
        double acc[1] = {0.0};
        const int total = s_nact * nn;
        for (int p = t; p < total; p += MT) {
          const int q = p / nn, rem = p - q * nn, m = rem / nbl, k = rem - m * nbl;
          const int gj = s_list[q] * nbl + m, gi = b * nbl + k;
          const double xj = s_pos[gj][0], yj = s_pos[gj][1], zj = s_pos[gj][2];
          const int tj = __double2loint(s_pos[gj][3]), ti = __double2loint(s_pos[gi][3]);
          const double Un = mc_pair_U(M, C, s_desc, ti, tj, s_new[k][0] - xj, s_new[k][1] - yj, s_new[k][2] - zj);
          const double Uo = mc_pair_U(M, C, s_desc, ti, tj, s_pos[gi][0] - xj, s_pos[gi][1] - yj, s_pos[gi][2] - zj);
          acc[0] += Un - Uo;
        }
        if (t < nbl) acc[0] += mc_blob_U(M, s_new[t][2]) - mc_blob_U(M, s_pos[b * nbl + t][2]);
        if (t == 0 && M.tr_per) acc[0] += mc_trap_U(M, (int)g0 + b, Xn) - mc_trap_U(M, (int)g0 + b, Xo);
        if (M.bonds && s_row[b] >= 0) {
          const int row = s_row[b];
          for (int q = M.B.ptr[row] + t; q < M.B.ptr[row + 1]; q += MT) {
            const int partner = M.B.ends[3 * (size_t)q], bond = M.B.ends[3 * (size_t)q + 1], end = M.B.ends[3 * (size_t)q + 2];
            const int ia = end ? partner : b, ib = end ? b : partner;
            double lA[3], lB[3], rr[3], dd, Uo, Un, dU;
            ia_bond_eval(M.B, s_X, s_Q, bond, r, ia, ib, lA, lB, rr, dd, Uo, dU);
            ia_bond_eval(M.B, s_Xn, s_Qn, bond, r, ia, ib, lA, lB, rr, dd, Un, dU);
            acc[0] += Un - Uo;
          }
        }
        rbl_block_sum<1, MT>(acc, s_red, t);
        dE = acc[0];
        verdict = (dE <= 0.0 || u6 < exp(-dE / kT)) ? 1 : 0;
      }
      if (t == 0 && tried < A.n_trace) {
        double *row = A.trace + ((size_t)r * A.n_trace + (size_t)tried) * MC_TRACE;
        row[0] = (double)b;
#pragma unroll
        for (int q = 0; q < 6; ++q) row[1 + q] = d[q];
        row[7] = dE; row[8] = u6; row[9] = (double)verdict;
      }
      ++tried;
      if (verdict == 1) {
        ++accepted;
        E_run += dE;
        if (t < nbl) {
          const int gi = b * nbl + t;
          s_pos[gi][0] = s_new[t][0]; s_pos[gi][1] = s_new[t][1]; s_pos[gi][2] = s_new[t][2];
        }
        if (t == 0) {
#pragma unroll
          for (int q = 0; q < 3; ++q) s_X[3 * b + q] = Xn[q];
#pragma unroll
          for (int q = 0; q < 4; ++q) s_Q[4 * b + q] = Qn[q];
        }
      } else {
        if (verdict == 2) ++wall_rej;
        if (t == 0) {
#pragma unroll
          for (int q = 0; q < 3; ++q) s_Xn[3 * b + q] = Xo[q];
#pragma unroll
          for (int q = 0; q < 4; ++q) s_Qn[4 * b + q] = Qo[q];
        }
      }
      __syncthreads();                                   // the commit is visible; s_new and the list may be written again
    }
    if (A.stride > 0 && (sc + 1) % A.stride == 0) {
      const size_t f = (size_t)((sc + 1) / A.stride - 1);
      double *fX = A.fX + (f * A.R + r) * 3 * Nb, *fQ = A.fQ + (f * A.R + r) * 4 * Nb;
      for (int u = t; u < 3 * Nb; u += MT) fX[u] = s_X[u];
      for (int u = t; u < 4 * Nb; u += MT) fQ[u] = s_Q[u];
      if (t == 0) A.fE[f * A.R + r] = E_run;
    }
  }
  for (int u = t; u < 3 * Nb; u += MT) A.Xd[3 * g0 + u] = s_X[u];
  for (int u = t; u < 4 * Nb; u += MT) A.Qd[4 * g0 + u] = s_Q[u];
  if (t == 0) {
    A.cnt[3 * (size_t)r] = tried; A.cnt[3 * (size_t)r + 1] = accepted; A.cnt[3 * (size_t)r + 2] = wall_rej;
    A.E[2 * (size_t)r + 1] = E_run;
  }
}

// the call's own device buffer: kBT | read-back block (counters, energies) | frozen mask | frames | trace
struct McBuf {
  double *kBT;
  long long *cnt; double *E;
  size_t rb_off, rb_bytes;
  uint8_t *frozen;
  double *fX, *fQ, *fE, *trace;
};

McBuf mc_carve(void *base, int R, int Nb, int kBT_sets, int frozen_sets, size_t n_frames, int n_trace, size_t *bytes)
{
  const size_t Rz = (size_t)R;
  RblCarve C{(char *)base};
  McBuf b;
  b.kBT = C.take<double>((size_t)kBT_sets);
  b.rb_off = C.off;
  b.cnt = C.take<long long>(3 * Rz);
  b.E = C.take<double>(2 * Rz);
  b.rb_bytes = C.off - b.rb_off;
  b.frozen = C.take<uint8_t>((size_t)frozen_sets * Nb);
  b.fX = C.take<double>(n_frames * Rz * 3 * Nb); b.fQ = C.take<double>(n_frames * Rz * 4 * Nb); b.fE = C.take<double>(n_frames * Rz);
  b.trace = C.take<double>(Rz * (size_t)n_trace * MC_TRACE);
  *bytes = C.off;
  return b;
}

}  // namespace

int rbl_ensemble_mc(rbl_ctx *c, const rbl_mc_opts *o, rbl_mc_out *out)
{
  if (!c) return RBL_ERR_ARG;
  const std::string who = "ensemble_mc: ";
  if (!o || !out) return rbl_fail(c, RBL_ERR_ARG, who + "opts and out must not be NULL");
  if (o->size != (int64_t)sizeof(rbl_mc_opts)) return rbl_fail(c, RBL_ERR_ARG, who + "opts.size is not sizeof(rbl_mc_opts)");
  if (out->size != (int64_t)sizeof(rbl_mc_out)) return rbl_fail(c, RBL_ERR_ARG, who + "out.size is not sizeof(rbl_mc_out)");
  if (o->n_sweeps < 1) return rbl_fail(c, RBL_ERR_ARG, who + "n_sweeps must be >= 1");
  if (o->sweep_start < 0) return rbl_fail(c, RBL_ERR_ARG, who + "sweep_start must be >= 0");
  if (!std::isfinite(o->step_x) || o->step_x < 0.0) return rbl_fail(c, RBL_ERR_ARG, who + "step_x must be finite and >= 0");
  if (!std::isfinite(o->step_theta) || o->step_theta < 0.0) return rbl_fail(c, RBL_ERR_ARG, who + "step_theta must be finite and >= 0");
  if (o->replica_base < 0) return rbl_fail(c, RBL_ERR_ARG, who + "replica_base must be >= 0");
  if (o->kBT_sets < 0) return rbl_fail(c, RBL_ERR_ARG, who + "kBT_sets must be 0, 1 or R");
  if (o->kBT_sets > 0 && !o->kBT) return rbl_fail(c, RBL_ERR_ARG, who + "kBT is NULL with kBT_sets > 0");
  // (the first entry now; the others once kBT_sets is known to be R, below: a wrong count is refused before it is read)
  if (o->kBT_sets > 0 && (!std::isfinite(o->kBT[0]) || !(o->kBT[0] > 0.0)))
    return rbl_fail(c, RBL_ERR_ARG, who + "kBT[0] must be finite and > 0");
  if (o->frozen_sets < 0) return rbl_fail(c, RBL_ERR_ARG, who + "frozen_sets must be 0, 1 or R");
  if (o->frozen_sets > 0 && !o->frozen) return rbl_fail(c, RBL_ERR_ARG, who + "frozen is NULL with frozen_sets > 0");
  if (o->stride < 0) return rbl_fail(c, RBL_ERR_ARG, who + "stride must be >= 0");
  if (o->n_trace < 0) return rbl_fail(c, RBL_ERR_ARG, who + "n_trace must be >= 0");
  const size_t n_frames = o->stride > 0 ? (size_t)(o->n_sweeps / o->stride) : 0;
  if (n_frames && (!out->frame_X || !out->frame_Q || !out->frame_E))
    return rbl_fail(c, RBL_ERR_ARG, who + "frame_X, frame_Q and frame_E must not be NULL while stride > 0 records frames");
  if (o->n_trace > 0 && !out->trace) return rbl_fail(c, RBL_ERR_ARG, who + "trace must not be NULL with n_trace > 0");
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, who + "ensemble: not on a context with a communicator (run one ensemble per process)");
  if (ens_jt_active(c))
    return rbl_fail(c, RBL_ERR_STATE, who + "hard joints are switched on: constrained sampling is not offered (switch the joints off first)");
  int mask = 0;
  rbl_interactions_active(c, &mask);
  if (mask & 16) return rbl_fail(c, RBL_ERR_STATE, who + "the dipole pair term is active and not offered here (rbl_set_dipoles)");
  if (mask & 32) return rbl_fail(c, RBL_ERR_STATE, who + "the field torque is active and not offered here (rbl_set_magnetic_field)");
  int rc;
  if (c->S.params_set && (rc = ens_state_check(c, who))) return rc;
  if (c->S.params_set && !(c->S.kBT > 0.0) && o->kBT_sets == 0)
    return rbl_fail(c, RBL_ERR_ARG, who + "the context's kBT must be > 0 (or give kBT)");
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = c->S.N_blb;
  if (c->S.params_set) {
    if (o->kBT_sets > 1 && o->kBT_sets != R) return rbl_fail(c, RBL_ERR_ARG, who + "kBT_sets must be 0, 1 or R = " + std::to_string(R));
    for (int k = 1; k < o->kBT_sets; ++k)
      if (!std::isfinite(o->kBT[k]) || !(o->kBT[k] > 0.0))
        return rbl_fail(c, RBL_ERR_ARG, who + "kBT[" + std::to_string(k) + "] must be finite and > 0");
    if (o->frozen_sets > 1 && o->frozen_sets != R) return rbl_fail(c, RBL_ERR_ARG, who + "frozen_sets must be 0, 1 or R = " + std::to_string(R));
    if ((int64_t)o->replica_base + R > ((int64_t)1 << 31)) return rbl_fail(c, RBL_ERR_ARG, who + "replica_base + R must not exceed 2^31");
    if (!mask) return rbl_fail(c, RBL_ERR_STATE, who + "no term of the force model is switched on (rbl_set_interactions)");
  }
  if ((rc = ens_ready(c))) return rc;                     // (parameters never set: its refusal)
  // the kernel's LDS arrays hold the layout's bound (256 blobs, 64 bodies); what an ensemble can hold is less, the one-kernel solver's
  // size rule that rbl_ensemble_set_config applied -- asked again here, so the kernel never meets a shape that rule has not passed
  if (Nb > MC_BMAX || Nb * nbl > MC_NMAX || !rbl_gmres_small_fits(nbl, Nb, 1, false)) return rbl_fail(c, RBL_ERR_SIZE, who + ens_beyond());
  // energy_start: the evaluation of rbl_ensemble_interaction_forces -- its checks (trap, bond, type and cell counts, the cells'
  // minimum-image bounds) and uploads are the chain's as well
  EnsWork w;
  if ((rc = ens_work(c, 1, &w))) return rc;
  const size_t Rz = (size_t)R, N = (size_t)Nb * nbl;
  RBL_HIP(c, hipMemsetAsync(w.resid, 0, w.rb_bytes, c->stream));
  const int cur = c->ens_cur;
  const double *X = ens_X(c, cur), *Q = ens_Q(c, cur);
  rbl_launch_body_geom(c->stream, X, Q, ens_cfg(c), nbl, (int64_t)(Rz * N), w.lever, w.pos);
  double *f = nullptr;
  if ((rc = ia_eval_batch(c, X, Q, w.pos, w.lever, Nb, R, w.ia, &f, nullptr, w.e, w.gerr))) return rc;
  const IaMcModel M = ia_mc_model(c, R);
  const int kBT_sets = o->kBT_sets ? o->kBT_sets : 1;
  size_t bytes = 0;
  mc_carve(nullptr, R, Nb, kBT_sets, o->frozen_sets, n_frames, o->n_trace, &bytes);
  if ((rc = rbl_dev_reserve(c, c->d_ens_mc, bytes))) return rc;
  const McBuf b = mc_carve(c->d_ens_mc.p, R, Nb, kBT_sets, o->frozen_sets, n_frames, o->n_trace, &bytes);
  if ((rc = copy_h2d(c, b.kBT, o->kBT_sets ? o->kBT : &c->S.kBT, sizeof(double) * (size_t)kBT_sets))) return rc;
  if (o->frozen_sets && (rc = copy_h2d(c, b.frozen, o->frozen, (size_t)o->frozen_sets * Nb))) return rc;
  RBL_HIP(c, hipMemsetAsync(b.cnt, 0, b.rb_bytes, c->stream));
  McArgs A = {};
  A.cfg = ens_cfg(c); A.e_blob = w.e; A.kBT = b.kBT; A.frozen = o->frozen_sets ? b.frozen : nullptr;
  A.cnt = b.cnt; A.E = b.E; A.rerr = w.rerr;
  A.fX = b.fX; A.fQ = b.fQ; A.fE = b.fE; A.trace = b.trace;
  A.seed = o->seed; A.sweep_start = o->sweep_start; A.step_x = o->step_x; A.step_t = o->step_theta;
  A.R = R; A.Nb = Nb; A.nbl = nbl; A.wall = c->S.wall ? 1 : 0; A.kBT_sets = kBT_sets; A.frozen_sets = o->frozen_sets;
  A.stride = o->stride; A.n_trace = o->n_trace; A.replica_base = o->replica_base;
  A.Xd = ens_X(c, cur ^ 1); A.Qd = ens_Q(c, cur ^ 1);
  {
    RblPhase ph(c, RBL_T_FORCES);
    const int64_t per = c->mc_sweeps_per_launch;
    for (int64_t s0 = 0; s0 < o->n_sweeps; s0 += per) {
      A.first = s0 == 0 ? 1 : 0;
      A.Xs = A.first ? X : A.Xd; A.Qs = A.first ? Q : A.Qd;
      A.s0 = s0; A.ns = (int)std::min<int64_t>(per, o->n_sweeps - s0);
      hipLaunchKernelGGL(k_ens_mc, dim3((unsigned)R), dim3(MT), 0, c->stream, A, M);
      RBL_HIP(c, hipGetLastError());
    }
  }
  // one read-back of the flags (the evaluation's and the start's), the counters and the energies; frames and trace follow once the
  // call is known to have succeeded, so a refused call leaves the caller's arrays alone
  std::vector<char> h(w.rb_bytes + b.rb_bytes);
  if ((rc = copy_d2h(c, h.data(), w.resid, w.rb_bytes))) return rc;
  if ((rc = copy_d2h(c, h.data() + w.rb_bytes, b.cnt, b.rb_bytes))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  const unsigned *hf = (const unsigned *)(h.data() + ((char *)w.rerr - (char *)w.resid));
  for (int r = 0; r <= R; ++r)
    if (hf[r]) {
      rc = rbl_flags_to_status(c, hf[r]);
      c->last_error = who + (r < R ? "ensemble replica " + std::to_string(r) + ": " : std::string("ensemble: ")) + c->last_error;
      return rc;
    }
  const long long *hc = (const long long *)(h.data() + w.rb_bytes);
  const double *hE = (const double *)(h.data() + w.rb_bytes + ((char *)b.E - (char *)b.cnt));   // (the pieces are 256-byte aligned)
  if (n_frames) {
    if ((rc = copy_d2h(c, out->frame_X, b.fX, sizeof(double) * n_frames * Rz * 3 * Nb))) return rc;
    if ((rc = copy_d2h(c, out->frame_Q, b.fQ, sizeof(double) * n_frames * Rz * 4 * Nb))) return rc;
    if ((rc = copy_d2h(c, out->frame_E, b.fE, sizeof(double) * n_frames * Rz))) return rc;
  }
  if (o->n_trace && (rc = copy_d2h(c, out->trace, b.trace, sizeof(double) * Rz * (size_t)o->n_trace * MC_TRACE))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  for (int r = 0; r < R; ++r) {
    if (out->tried) out->tried[r] = hc[3 * (size_t)r];
    if (out->accepted) out->accepted[r] = hc[3 * (size_t)r + 1];
    if (out->wall_rejected) out->wall_rejected[r] = hc[3 * (size_t)r + 2];
    if (out->energy_start) out->energy_start[r] = hE[2 * (size_t)r];
    if (out->energy_end) out->energy_end[r] = hE[2 * (size_t)r + 1];
  }
  c->ens_cur ^= 1;                                        // the existing flip: the chain's result is the committed configuration
  return RBL_OK;
}
