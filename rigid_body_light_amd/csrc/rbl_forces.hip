// rbl_forces.hip -- configuration-dependent forces on the blobs (include/rbl.h section 4): buoyant weight, a screened wall
// repulsion and a steric repulsion between blobs of different bodies, evaluated on the GPU at the context's configuration and
// reduced to body forces / torques with K^T.  The reference has no force model; what it would have needed is a host loop.
//
// Two kernels:
//   k_body_neighbours    one wave per body i: the bodies j != i of i's window (an ensemble's replica; one system: all bodies)
//                        with |X_i - X_j| <= 2 R_body + r_cut, written in increasing j
//                        by a ballot and a prefix count (no atomics: the lists are the same on every call and every rank).
//                        Exact cull: a blob lies within R_body of its body's centre, so two blobs of bodies further apart
//                        than 2 R_body + r_cut are further apart than r_cut.
//   k_blob_interactions  one workgroup per (body i, tile of i's blobs): the neighbours' blob positions are staged through LDS
//                        in list order, every lane accumulates the force on ITS blob in registers over the ordered pairs
//                        (i <- j; the pair j <- i is evaluated by j's workgroup), weight and wall are added in the epilogue.
//                        No fp64 atomics, one summation order: bitwise reproducible.  The software exp and the division are
//                        taken only inside r_cut.
//   k_blob_interactions_tab<TAB>  the same body compiled with the tabulated terms (bit 0 of TAB: pair table, bit 1: height
//                        table): per pair inside the table's cutoff one interval index, one 32-byte coefficient read and two
//                        Horner evaluations.  The coefficients stay in global memory and are read through L1 / L2: a lane's
//                        interval follows ITS pair distance, so the read is a gather either way; in LDS a gather of 32 bytes
//                        per lane at unrelated intervals pays bank conflicts, and only tables below a few thousand intervals
//                        would fit beside the position chunk at all (the largest table is 2 MB).  An LDS-staged variant has
//                        not been built.  k_blob_interactions itself is the TAB = 0 instantiation with the argument list it
//                        always had.
//   k_blob_interactions_typed<TAB, CELL>  the pair kernel with blob types and one table per unordered type pair, launched only while
//                        types and a usable type table are on: the same grid, chunking and summation order; the neighbour's type
//                        rides in the fourth slot of the staged position, the 36 table descriptors sit in LDS (see the kernel).
//   k_body_traps         harmonic traps on the body centres, after K^T f: one lane per body.
//   k_body_dipoles<NT>   permanent dipoles fixed in the bodies, after the traps: one workgroup of NT lanes per body i (one wave
//                        for windows of up to 512 bodies, four beyond).  Lane t takes the partners j = t, t + NT, ... of i's
//                        window by their window-local index, rotates the partner's body-frame moment with its quaternion and
//                        accumulates force, torque and pair energy on i in fp64 registers; rbl_block_sum adds the lanes in one
//                        fixed tree and lane 0 adds the result, and the torque and energy of the uniform field B(t), to
//                        FT[6 i ..] and to the energy entry of the body's first blob.  No atomics; the order depends on the
//                        window-local indices alone, so a replica of an ensemble is bitwise the single context.  Every
//                        partner is read once per workgroup, so nothing is staged: the only LDS is the reduction's.
//   k_body_bonds         bonds and tethers between anchor points fixed in the bodies, after the dipoles: one wave per (bonded
//                        body, window).  The host keeps a CSR of bond ENDS by body, in increasing bond index (built once per
//                        rbl_set_bonds); lane t takes the ends t, t + 64, ... of its body, rotates both anchors with the two
//                        quaternions, evaluates the bond (harmonic, or the bond table continued along its tangent at both ends
//                        of the grid) and accumulates force, torque and its share of the energy in fp64 registers;
//                        rbl_block_sum adds the lanes in one fixed tree and lane 0 adds to FT[6 i ..] and to the energy entry
//                        of the body's first blob.  Both ends of a bond evaluate the same r = p_A - p_B with the same
//                        operations, so the two forces are bitwise opposite.  No atomics; the order depends on replica-local
//                        indices alone.  The grid covers the compact list of bonded bodies, not all bodies.
//   k_bond_state         one lane per (window, bond): length, tension dU/dd and energy, for the state queries.
//   k_body_neighbours_per, k_blob_interactions_per<TAB>, k_body_dipoles_per<NT>   the same three with the pair displacement by
//                        minimum image in a periodic cell (include/rbl.h section 10), selected by ia_launch while the cell is on.
//                        The pair kernel shares its body with the open one through a template flag; the other two repeat theirs
//                        (see k_body_neighbours_per).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"
#include "rbl_forces_dev.hpp"   // the argument structs and the energy expressions, shared with the sampler (rbl_ens_mc.hip)

namespace {

constexpr int IA_CAP_MAX = 1024;      // neighbour-list length per body (beyond it: RBL_ERR_CAPACITY)
constexpr int IA_CHUNK = 512;         // neighbour blobs staged per pass (x, y, z, pad: 16 KB of LDS)
constexpr int IA_BT = 256;            // lanes per workgroup of the pair kernel for bodies of more than 128 blobs

// win: bodies per window -- body i only sees the bodies [i - i % win, i - i % win + win) (the replicas of an ensemble do not
// interact); win = N_bod: every body
__global__ __launch_bounds__(64) void k_body_neighbours(const double *__restrict__ X, int N_bod, int win, double cut2, int cull,
                                                        int cap, int *__restrict__ cnt, int *__restrict__ list, unsigned *__restrict__ err)
{
  const int i = blockIdx.x, t = threadIdx.x;
  const double xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
  const int jb = i - i % win, je = min(jb + win, N_bod);
  int base = 0;
  for (int j0 = jb; j0 < je; j0 += 64) {
    const int j = j0 + t;
    bool take = false;
    if (j < je && j != i) {
      if (!cull) take = true;
      else {
        const double dx = X[3 * (size_t)j] - xi, dy = X[3 * (size_t)j + 1] - yi, dz = X[3 * (size_t)j + 2] - zi;
        take = dx * dx + dy * dy + dz * dz <= cut2;
      }
    }
    const unsigned long long m = __ballot(take);
    const int below = __popcll(m & ((1ull << t) - 1ull));
    if (take && base + below < cap) list[(size_t)i * cap + base + below] = j;
    base += __popcll(m);
  }
  if (t == 0) {
    cnt[i] = base;                                       // may exceed cap: the pair kernel walks min(cnt, cap) and the overflow is reported
    if (base > cap) atomicOr(err, (unsigned)RBL_FLAG_CAPACITY);
  }
}

// the same with the centre distance by minimum image (a periodic cell).  Its own body, k_body_neighbours' repeated: that kernel
// as an instantiation of a shared template came out of the compiler with its registers permuted, and it keeps its code instruction
// for instruction.  The two periodic kernels -- the cell by value, or the cell of the body's window from a table -- share this one
__device__ __forceinline__ void ia_body_neighbours_per(const double *__restrict__ X, int N_bod, int win, double cut2, int cull, int cap,
                                                       const IaCell &C, int *__restrict__ cnt, int *__restrict__ list,
                                                       unsigned *__restrict__ err)
{
  const int i = blockIdx.x, t = threadIdx.x;
  const double xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
  const int jb = i - i % win, je = min(jb + win, N_bod);
  int base = 0;
  for (int j0 = jb; j0 < je; j0 += 64) {
    const int j = j0 + t;
    bool take = false;
    if (j < je && j != i) {
      if (!cull) take = true;
      else {
        double dx = X[3 * (size_t)j] - xi, dy = X[3 * (size_t)j + 1] - yi;
        const double dz = X[3 * (size_t)j + 2] - zi;
        ia_min_image(C, dx, dy);
        take = dx * dx + dy * dy + dz * dz <= cut2;
      }
    }
    const unsigned long long m = __ballot(take);
    const int below = __popcll(m & ((1ull << t) - 1ull));
    if (take && base + below < cap) list[(size_t)i * cap + base + below] = j;
    base += __popcll(m);
  }
  if (t == 0) {
    cnt[i] = base;                                       // may exceed cap: the pair kernel walks min(cnt, cap) and the overflow is reported
    if (base > cap) atomicOr(err, (unsigned)RBL_FLAG_CAPACITY);
  }
}

__global__ __launch_bounds__(64) void k_body_neighbours_per(const double *__restrict__ X, int N_bod, int win, double cut2, int cull,
                                                            int cap, IaCell C, int *__restrict__ cnt, int *__restrict__ list,
                                                            unsigned *__restrict__ err)
{
  ia_body_neighbours_per(X, N_bod, win, cut2, cull, cap, C, cnt, list, err);
}

// ... and in the cell of the body's window, one per replica
__global__ __launch_bounds__(64) void k_body_neighbours_cells(const double *__restrict__ X, int N_bod, int win, double cut2, int cull,
                                                              int cap, const RblEnsCellRec *__restrict__ cells, int *__restrict__ cnt,
                                                              int *__restrict__ list, unsigned *__restrict__ err)
{
  ia_body_neighbours_per(X, N_bod, win, cut2, cull, cap, ia_cell_of(cells, blockIdx.x / win), cnt, list, err);
}

// TAB: bit 0 pair table PT, bit 1 height table HT (both ignored in the TAB = 0 instantiation, the model of weight, wall and
// steric repulsion alone).  A pair is counted once when it lies inside the cutoff of a pair term that is on; the built-in
// term is switched off by p.rc2 < 0
// PER: the pair displacement by minimum image in the cell C (every blob pair on its own: the check at the evaluation makes
// the convention unique inside the cutoff)
template <int TAB, bool PER = false>
__device__ __forceinline__ void ia_blob_interactions(double (*s)[4], const double *__restrict__ pos, const int *__restrict__ cnt,
                                                     const int *__restrict__ list, int cap, int N_blb, int tiles, const IaParams &p,
                                                     const IaTab &PT, const IaTab &HT, double *__restrict__ f,
                                                     double *__restrict__ e, int *__restrict__ npairs, const IaCell &C = IaCell{})
{
  const int i = blockIdx.x / tiles, k = (blockIdx.x - i * tiles) * blockDim.x + threadIdx.x;
  const bool own = k < N_blb;
  const size_t gi = (size_t)i * N_blb + (own ? k : 0);
  const double xi = pos[3 * gi], yi = pos[3 * gi + 1], zi = pos[3 * gi + 2];
  double fx = 0.0, fy = 0.0, fz = 0.0, en = 0.0;
  int np = 0;
  const int nn = min(cnt[i], cap);
  for (int q = 0; q < nn; ++q) {
    const double *pj = pos + 3 * (size_t)list[(size_t)i * cap + q] * N_blb;
    for (int c0 = 0; c0 < N_blb; c0 += IA_CHUNK) {
      const int m = min(IA_CHUNK, N_blb - c0);
      __syncthreads();                                   // the previous chunk has been read by every lane
      for (int u = threadIdx.x; u < m; u += blockDim.x) {
        s[u][0] = pj[3 * (size_t)(c0 + u)];
        s[u][1] = pj[3 * (size_t)(c0 + u) + 1];
        s[u][2] = pj[3 * (size_t)(c0 + u) + 2];
      }
      __syncthreads();
      if (!own) continue;
      for (int u = 0; u < m; ++u) {
        double dx = xi - s[u][0], dy = yi - s[u][1];
        const double dz = zi - s[u][2];
        if constexpr (PER) ia_min_image(C, dx, dy);
        const double r2 = dx * dx + dy * dy + dz * dz;
        if constexpr (TAB & 1) {
          if (r2 > p.rc2 && r2 > PT.hi2) continue;       // beyond both cutoffs (hi2: a hair above hi^2, r <= hi decides)
        } else {
          if (r2 > p.rc2) continue;                      // beyond the cutoff: skipped, not multiplied by zero
        }
        const double r = sqrt(r2);
        const bool in_t = (TAB & 1) && r <= PT.hi;       // each term has its own cutoff
        double U, g;                                     // energy of the pair, -U'(r) / r
        if ((TAB & 1) && r2 > p.rc2) {                   // only the table can reach this far
          if (!in_t) continue;
          U = 0.0; g = 0.0;
        } else {
          ia_steric(p, r, U, g);
        }
        if constexpr (TAB & 1) {
          if (in_t) {
            double Ut, dUt;
            ia_tab_eval(PT, r, Ut, dUt);
            U += Ut;
            if (r > 0.0) g -= dUt / r;                   // coincident blobs exert no force
          }
        }
        fx += g * dx; fy += g * dy; fz += g * dz;
        en += 0.5 * U;
        ++np;
      }
    }
  }
  if (!own) return;
  fz -= p.w;                                             // weight
  en += p.w * zi;
  if (p.wall) {                                          // wall repulsion, tangent continued below h = a
    double Fw, Uw;
    ia_wall(p, zi, Uw, Fw);
    fz += Fw;
    en += Uw;
  }
  if constexpr (TAB & 2) {
    if (zi <= HT.hi) {                                   // with or without the wall; nothing above h_cut
      double Uh, dUh;
      ia_tab_eval(HT, zi, Uh, dUh);
      fz -= dUh;
      en += Uh;
    }
  }
  f[3 * gi] = fx; f[3 * gi + 1] = fy; f[3 * gi + 2] = fz;
  if (e) e[gi] = en;
  npairs[gi] = np;
}

__global__ __launch_bounds__(IA_BT) void k_blob_interactions(const double *__restrict__ pos, const int *__restrict__ cnt,
                                                             const int *__restrict__ list, int cap, int N_blb, int tiles,
                                                             IaParams p, double *__restrict__ f, double *__restrict__ e,
                                                             int *__restrict__ npairs)
{
  __shared__ double s[IA_CHUNK][4];
  const IaTab none = {};
  ia_blob_interactions<0>(s, pos, cnt, list, cap, N_blb, tiles, p, none, none, f, e, npairs);
}

template <int TAB>
__global__ __launch_bounds__(IA_BT) void k_blob_interactions_tab(const double *__restrict__ pos, const int *__restrict__ cnt,
                                                                 const int *__restrict__ list, int cap, int N_blb, int tiles,
                                                                 IaParams p, IaTab PT, IaTab HT, double *__restrict__ f,
                                                                 double *__restrict__ e, int *__restrict__ npairs)
{
  static_assert(TAB >= 1 && TAB <= 3, "bit 0: pair table, bit 1: height table");
  __shared__ double s[IA_CHUNK][4];
  ia_blob_interactions<TAB>(s, pos, cnt, list, cap, N_blb, tiles, p, PT, HT, f, e, npairs);
}

// the pair kernel of a periodic cell, TAB = 0 ... 3 as above
template <int TAB>
__global__ __launch_bounds__(IA_BT) void k_blob_interactions_per(const double *__restrict__ pos, const int *__restrict__ cnt,
                                                                 const int *__restrict__ list, int cap, int N_blb, int tiles,
                                                                 IaParams p, IaTab PT, IaTab HT, IaCell C, double *__restrict__ f,
                                                                 double *__restrict__ e, int *__restrict__ npairs)
{
  static_assert(TAB >= 0 && TAB <= 3, "bit 0: pair table, bit 1: height table");
  __shared__ double s[IA_CHUNK][4];
  ia_blob_interactions<TAB, true>(s, pos, cnt, list, cap, N_blb, tiles, p, PT, HT, f, e, npairs, C);
}

// ... with a cell per replica: the tile's body i = blockIdx.x / tiles lies in window i / win
template <int TAB>
__global__ __launch_bounds__(IA_BT) void k_blob_interactions_cells(const double *__restrict__ pos, const int *__restrict__ cnt,
                                                                   const int *__restrict__ list, int cap, int N_blb, int tiles, int win,
                                                                   IaParams p, IaTab PT, IaTab HT, const RblEnsCellRec *__restrict__ cells,
                                                                   double *__restrict__ f, double *__restrict__ e,
                                                                   int *__restrict__ npairs)
{
  static_assert(TAB >= 0 && TAB <= 3, "bit 0: pair table, bit 1: height table");
  __shared__ double s[IA_CHUNK][4];
  ia_blob_interactions<TAB, true>(s, pos, cnt, list, cap, N_blb, tiles, p, PT, HT, f, e, npairs, ia_cell_of(cells, blockIdx.x / tiles / win));
}

// ---- blob types: one pair table per unordered type pair (include/rbl.h section 4; IaTyped, IaTabLds: rbl_forces_dev.hpp) ------
// the pair kernel with blob types: the grid, the chunking and the summation order of ia_blob_interactions (its own body: that one's
// kernels keep their code instruction for instruction).  The fourth slot of a staged blob carries its type; the neighbour's type
// is the same for every lane at every step of the inner loop (an LDS broadcast), the lane's own type is not, so the descriptor of
// (own, neighbour) is read from LDS by a per-lane address, and only by the pairs inside the largest cutoff.
// CELL: 0 open, 1 the cell C, 2 the cell of the tile's window from the table
template <int TAB, int CELL>
__global__ __launch_bounds__(IA_BT) void k_blob_interactions_typed(const double *__restrict__ pos, const int *__restrict__ cnt,
                                                                   const int *__restrict__ list, int cap, int N_blb, int tiles, int win,
                                                                   IaParams p, IaTab PT, IaTab HT, IaTyped Y, IaCell Cv,
                                                                   const RblEnsCellRec *__restrict__ cells, double *__restrict__ f,
                                                                   double *__restrict__ e, int *__restrict__ npairs)
{
  static_assert(TAB >= 0 && TAB <= 3 && CELL >= 0 && CELL <= 2, "TAB bit 0: pair table, bit 1: height table; CELL 0 open, 1 by value, 2 table");
  __shared__ double s[IA_CHUNK][4];
  __shared__ IaTabLds sd[IA_TY_PAIRS];
  for (int u = threadIdx.x; u < IA_TY_PAIRS; u += blockDim.x) sd[u].T = Y.desc[u];   // (the first barrier of the loop orders it)
  const int i = blockIdx.x / tiles, k = (blockIdx.x - i * tiles) * blockDim.x + threadIdx.x;
  IaCell C = Cv;
  if constexpr (CELL == 2) C = ia_cell_of(cells, i / win);
  const bool own = k < N_blb;
  const size_t gi = (size_t)i * N_blb + (own ? k : 0);
  const double xi = pos[3 * gi], yi = pos[3 * gi + 1], zi = pos[3 * gi + 2];
  const int ti = Y.type[(size_t)(Y.per_row ? i % win : 0) * N_blb + (own ? k : 0)];
  double fx = 0.0, fy = 0.0, fz = 0.0, en = 0.0;
  int np = 0;
  const int nn = min(cnt[i], cap);
  for (int q = 0; q < nn; ++q) {
    const int j = list[(size_t)i * cap + q];
    const double *pj = pos + 3 * (size_t)j * N_blb;
    const int *tj = Y.type + (size_t)(Y.per_row ? j % win : 0) * N_blb;
    for (int c0 = 0; c0 < N_blb; c0 += IA_CHUNK) {
      const int m = min(IA_CHUNK, N_blb - c0);
      __syncthreads();                                   // the previous chunk has been read by every lane
      for (int u = threadIdx.x; u < m; u += blockDim.x) {
        s[u][0] = pj[3 * (size_t)(c0 + u)];
        s[u][1] = pj[3 * (size_t)(c0 + u) + 1];
        s[u][2] = pj[3 * (size_t)(c0 + u) + 2];
        s[u][3] = __hiloint2double(0, tj[c0 + u]);       // the type in the low word of the fourth slot
      }
      __syncthreads();
      if (!own) continue;
      for (int u = 0; u < m; ++u) {
        double dx = xi - s[u][0], dy = yi - s[u][1];
        const double dz = zi - s[u][2];
        if constexpr (CELL != 0) ia_min_image(C, dx, dy);
        const double r2 = dx * dx + dy * dy + dz * dz;
        if (r2 > Y.cmax2) continue;                      // beyond every cutoff that is on: skipped, not multiplied by zero
        const double r = sqrt(r2);
        const IaTab &TT = sd[ia_type_pair(ti, __double2loint(s[u][3]))].T;
        const bool in_b = r2 <= p.rc2;                   // each term has its own cutoff
        const bool in_t = (TAB & 1) && r <= PT.hi;
        const bool in_y = r <= TT.hi;
        if (!(in_b || in_t || in_y)) continue;
        double U = 0.0, g = 0.0;                         // energy of the pair, -U'(r) / r
        if (in_b) ia_steric(p, r, U, g);
        if constexpr (TAB & 1) {
          if (in_t) {
            double Ut, dUt;
            ia_tab_eval(PT, r, Ut, dUt);
            U += Ut;
            if (r > 0.0) g -= dUt / r;                   // coincident blobs exert no force
          }
        }
        if (in_y) {
          double Ut, dUt;
          ia_tab_eval(TT, r, Ut, dUt);
          U += Ut;
          if (r > 0.0) g -= dUt / r;
        }
        fx += g * dx; fy += g * dy; fz += g * dz;
        en += 0.5 * U;
        ++np;
      }
    }
  }
  if (!own) return;
  fz -= p.w;                                             // weight
  en += p.w * zi;
  if (p.wall) {                                          // wall repulsion, tangent continued below h = a
    double Fw, Uw;
    ia_wall(p, zi, Uw, Fw);
    fz += Fw;
    en += Uw;
  }
  if constexpr (TAB & 2) {
    if (zi <= HT.hi) {                                   // with or without the wall; nothing above h_cut
      double Uh, dUh;
      ia_tab_eval(HT, zi, Uh, dUh);
      fz -= dUh;
      en += Uh;
    }
  }
  f[3 * gi] = fx; f[3 * gi + 1] = fy; f[3 * gi + 2] = fz;
  if (e) e[gi] = en;
  npairs[gi] = np;
}

// harmonic traps on the body centres: FT[6 i + c] -= k_c (X_c - X0_c), the energy added to the entry of the body's first blob
// (after the pair kernel on the same stream: one order).  per: entries of k / X0 -- body i reads entry i % per (an ensemble's
// shared layout: per = bodies of a replica; one entry per body otherwise)
__global__ __launch_bounds__(256) void k_body_traps(const double *__restrict__ X, const double *__restrict__ k3,
                                                    const double *__restrict__ X0, int nbod, int per, int N_blb,
                                                    double *__restrict__ FT, double *__restrict__ e)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nbod) return;
  const size_t j = (size_t)(i % per);
  double E = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double k = k3[3 * j + c], d = X[3 * (size_t)i + c] - X0[3 * j + c];
    if (k != 0.0) {                                      // a component of 0: no trap along that axis
      if (FT) FT[6 * (size_t)i + c] -= k * d;
      E += 0.5 * k * d * d;
    }
  }
  if (e) e[(size_t)i * N_blb] += E;
}

// the dipole model as the kernel takes it (by value).  B: B0 | B1 | B2
struct IaMag {
  double B[9], omega, dt, c_dd, r_core, r_cut;
  int pairs, field;                                      // the pair term (c_dd > 0) / the field torque is on
  int per_m, per_t;                                      // entries of the moment array (body i reads i % per_m) and of the field times
};

// B at replica r's field time t = t0 + dt * n, n = the replica's accepted steps so far inside a run (accepted == NULL, the
// one-step calls: 0).  The product and the sum are rounded separately, as the host's t0 + dt * n is: a run is bitwise the loop.
// Contraction is switched off for the two statements: __dmul_rn and __dadd_rn are the plain operators here, and the compiler fused
// them into one fma, which rounds differently for some n (t0 = 0.37, dt = 0.01: first at n = 9)
__device__ __forceinline__ void ia_field_B(const IaMag &M, const double *__restrict__ tf, const int *__restrict__ accepted, int r,
                                           double (&B)[3])
{
  const double n = accepted ? (double)accepted[r] : 0.0;
  double t;
  {
#pragma clang fp contract(off)
    const double s = M.dt * n;
    t = tf[M.per_t == 1 ? 0 : r] + s;
  }
  double sn, cs;
  sincos(__dmul_rn(M.omega, t), &sn, &cs);
#pragma unroll
  for (int c = 0; c < 3; ++c) B[c] = M.B[c] + M.B[3 + c] * cs + M.B[6 + c] * sn;
}

// lab-frame moment of body j: R(Q_j) m_body
__device__ __forceinline__ void ia_lab_moment(const double *__restrict__ Q, const double *__restrict__ mb, int j, int per_m,
                                              double (&m)[3])
{
  double R[9];
  quat_rot(Q + 4 * (size_t)j, R);
  const double *b = mb + 3 * (size_t)(j % per_m);
#pragma unroll
  for (int c = 0; c < 3; ++c) m[c] = R[3 * c] * b[0] + R[3 * c + 1] * b[1] + R[3 * c + 2] * b[2];
}

// dipole pairs between the centres of the bodies of one window and the field torque (include/rbl.h section 4), added to FT and
// to the energy entry of the body's first blob after the traps on the same stream: one order
template <int NT>
__global__ __launch_bounds__(NT) void k_body_dipoles(const double *__restrict__ X, const double *__restrict__ Q,
                                                     const double *__restrict__ mb, const double *__restrict__ tf,
                                                     const int *__restrict__ accepted, int win, int N_blb, IaMag M,
                                                     double *__restrict__ FT, double *__restrict__ e)
{
  __shared__ double red[7][NT];
  const int i = blockIdx.x, t = threadIdx.x;
  const int jb = i - i % win;
  double mi[3];
  ia_lab_moment(Q, mb, i, M.per_m, mi);
  const double xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // force, torque, sum of the pair energies
  if (M.pairs) {
    for (int j = jb + t; j < jb + win; j += NT) {
      if (j == i) continue;
      const double rx = xi - X[3 * (size_t)j], ry = yi - X[3 * (size_t)j + 1], rz = zi - X[3 * (size_t)j + 2];
      const double d2 = rx * rx + ry * ry + rz * rz;
      const double d = sqrt(d2);
      if (d > M.r_cut) continue;                         // skipped, not multiplied by zero (r_cut = +inf: every pair)
      double mj[3];
      ia_lab_moment(Q, mb, j, M.per_m, mj);
      const bool core = d < M.r_core;                    // below the core s is the constant r_core: U is a quadratic form in r
      const double is = 1.0 / (core ? M.r_core : d), is2 = is * is, is3 = is2 * is, is5 = is3 * is2;
      const double a = mi[0] * rx + mi[1] * ry + mi[2] * rz, b = mj[0] * rx + mj[1] * ry + mj[2] * rz;
      const double mm = mi[0] * mj[0] + mi[1] * mj[1] + mi[2] * mj[2];
      const double k5 = 3.0 * M.c_dd * is5;
      const double kr = core ? 0.0 : mm - 5.0 * a * b * is2;       // d >= r_core > 0: 1 / d^2 = is2
      acc[0] += k5 * (a * mj[0] + b * mi[0] + kr * rx);
      acc[1] += k5 * (a * mj[1] + b * mi[1] + kr * ry);
      acc[2] += k5 * (a * mj[2] + b * mi[2] + kr * rz);
      const double gb = k5 * b, g3 = M.c_dd * is3;               // the partner's field at i: gb r - g3 m_j
      const double hx = gb * rx - g3 * mj[0], hy = gb * ry - g3 * mj[1], hz = gb * rz - g3 * mj[2];
      acc[3] += mi[1] * hz - mi[2] * hy;
      acc[4] += mi[2] * hx - mi[0] * hz;
      acc[5] += mi[0] * hy - mi[1] * hx;
      acc[6] += M.c_dd * (mm * is3 - 3.0 * a * b * is5);
    }
    rbl_block_sum<7, NT>(acc, red, t);
  }
  if (t != 0) return;
  double E = 0.5 * acc[6];                               // every body carries half of each of its pair energies
  if (M.field) {
    double B[3];
    ia_field_B(M, tf, accepted, i / win, B);
    acc[3] += mi[1] * B[2] - mi[2] * B[1];
    acc[4] += mi[2] * B[0] - mi[0] * B[2];
    acc[5] += mi[0] * B[1] - mi[1] * B[0];
    E -= mi[0] * B[0] + mi[1] * B[1] + mi[2] * B[2];
  }
  if (FT) {
#pragma unroll
    for (int c = 0; c < 6; ++c) FT[6 * (size_t)i + c] += acc[c];
  }
  if (e) e[(size_t)i * N_blb] += E;
}

// bonds and tethers (include/rbl.h section 4; IaBonds, ia_bond_eval: rbl_forces_dev.hpp), added to FT and to the energy entry of the body's first blob after the dipoles on
// the same stream: one order.  One wave per (bonded body, window): blockIdx.x = window * n_rows + row
__global__ __launch_bounds__(64) void k_body_bonds(const double *__restrict__ X, const double *__restrict__ Q, int win, int N_blb,
                                                   IaBonds B, double *__restrict__ FT, double *__restrict__ e)
{
  __shared__ double red[7][64];
  const int w = blockIdx.x / B.n_rows, row = blockIdx.x - w * B.n_rows, t = threadIdx.x;
  const int i = w * win + B.rows[row];
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // force, torque, the body's share of the energies
  for (int q = B.ptr[row] + t; q < B.ptr[row + 1]; q += 64) {
    const int partner = B.ends[3 * (size_t)q], b = B.ends[3 * (size_t)q + 1], end = B.ends[3 * (size_t)q + 2];
    const int other = partner >= 0 ? w * win + partner : -1;
    double lA[3], lB[3], r[3], d, U, dU;
    ia_bond_eval(B, X, Q, b, w, end ? other : i, end ? i : other, lA, lB, r, d, U, dU);
    const double g = d > 0.0 ? -dU / d : 0.0;              // coincident ends exert no force
    double f[3] = {g * r[0], g * r[1], g * r[2]};          // on end A
    const double *l = lA;
    if (end) {
      f[0] = -f[0]; f[1] = -f[1]; f[2] = -f[2];
      l = lB;
    }
    acc[0] += f[0]; acc[1] += f[1]; acc[2] += f[2];
    acc[3] += l[1] * f[2] - l[2] * f[1];
    acc[4] += l[2] * f[0] - l[0] * f[2];
    acc[5] += l[0] * f[1] - l[1] * f[0];
    acc[6] += partner >= 0 ? 0.5 * U : U;                  // half of a body-body bond, all of a tether
  }
  rbl_block_sum<7, 64>(acc, red, t);
  if (t != 0) return;
  if (FT) {
#pragma unroll
    for (int c = 0; c < 6; ++c) FT[6 * (size_t)i + c] += acc[c];
  }
  if (e) e[(size_t)i * N_blb] += acc[6];
}

// length, tension dU/dd and energy of every bond of every window: out = length [n_win n] | tension | energy
__global__ __launch_bounds__(256) void k_bond_state(const double *__restrict__ X, const double *__restrict__ Q, int win, int n_win,
                                                    IaBonds B, double *__restrict__ out)
{
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, tot = (size_t)n_win * B.n;
  if (g >= tot) return;
  const int w = (int)(g / B.n), b = (int)(g - (size_t)w * B.n);
  const int jb = B.body[2 * (size_t)b + 1];
  double lA[3], lB[3], r[3], d, U, dU;
  ia_bond_eval(B, X, Q, b, w, w * win + B.body[2 * (size_t)b], jb >= 0 ? w * win + jb : -1, lA, lB, r, d, U, dU);
  out[g] = d;
  out[tot + g] = dU;
  out[2 * tot + g] = U;
}

// the same with the pair displacement by minimum image (a periodic cell): its own body for the reason given at
// ia_body_neighbours_per, shared by the kernel that takes the cell by value and the one that reads it from a table
template <int NT>
__device__ __forceinline__ void ia_body_dipoles_per(double (*red)[NT], const double *__restrict__ X, const double *__restrict__ Q,
                                                    const double *__restrict__ mb, const double *__restrict__ tf,
                                                    const int *__restrict__ accepted, int win, int N_blb, const IaMag &M, const IaCell &C,
                                                    double *__restrict__ FT, double *__restrict__ e)
{
  const int i = blockIdx.x, t = threadIdx.x;
  const int jb = i - i % win;
  double mi[3];
  ia_lab_moment(Q, mb, i, M.per_m, mi);
  const double xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // force, torque, sum of the pair energies
  if (M.pairs) {
    for (int j = jb + t; j < jb + win; j += NT) {
      if (j == i) continue;
      double rx = xi - X[3 * (size_t)j], ry = yi - X[3 * (size_t)j + 1];
      const double rz = zi - X[3 * (size_t)j + 2];
      ia_min_image(C, rx, ry);
      const double d2 = rx * rx + ry * ry + rz * rz;
      const double d = sqrt(d2);
      if (d > M.r_cut) continue;                         // skipped, not multiplied by zero (r_cut = +inf: every pair)
      double mj[3];
      ia_lab_moment(Q, mb, j, M.per_m, mj);
      const bool core = d < M.r_core;                    // below the core s is the constant r_core: U is a quadratic form in r
      const double is = 1.0 / (core ? M.r_core : d), is2 = is * is, is3 = is2 * is, is5 = is3 * is2;
      const double a = mi[0] * rx + mi[1] * ry + mi[2] * rz, b = mj[0] * rx + mj[1] * ry + mj[2] * rz;
      const double mm = mi[0] * mj[0] + mi[1] * mj[1] + mi[2] * mj[2];
      const double k5 = 3.0 * M.c_dd * is5;
      const double kr = core ? 0.0 : mm - 5.0 * a * b * is2;       // d >= r_core > 0: 1 / d^2 = is2
      acc[0] += k5 * (a * mj[0] + b * mi[0] + kr * rx);
      acc[1] += k5 * (a * mj[1] + b * mi[1] + kr * ry);
      acc[2] += k5 * (a * mj[2] + b * mi[2] + kr * rz);
      const double gb = k5 * b, g3 = M.c_dd * is3;               // the partner's field at i: gb r - g3 m_j
      const double hx = gb * rx - g3 * mj[0], hy = gb * ry - g3 * mj[1], hz = gb * rz - g3 * mj[2];
      acc[3] += mi[1] * hz - mi[2] * hy;
      acc[4] += mi[2] * hx - mi[0] * hz;
      acc[5] += mi[0] * hy - mi[1] * hx;
      acc[6] += M.c_dd * (mm * is3 - 3.0 * a * b * is5);
    }
    rbl_block_sum<7, NT>(acc, red, t);
  }
  if (t != 0) return;
  double E = 0.5 * acc[6];                               // every body carries half of each of its pair energies
  if (M.field) {
    double B[3];
    ia_field_B(M, tf, accepted, i / win, B);
    acc[3] += mi[1] * B[2] - mi[2] * B[1];
    acc[4] += mi[2] * B[0] - mi[0] * B[2];
    acc[5] += mi[0] * B[1] - mi[1] * B[0];
    E -= mi[0] * B[0] + mi[1] * B[1] + mi[2] * B[2];
  }
  if (FT) {
#pragma unroll
    for (int c = 0; c < 6; ++c) FT[6 * (size_t)i + c] += acc[c];
  }
  if (e) e[(size_t)i * N_blb] += E;
}

template <int NT>
__global__ __launch_bounds__(NT) void k_body_dipoles_per(const double *__restrict__ X, const double *__restrict__ Q,
                                                     const double *__restrict__ mb, const double *__restrict__ tf,
                                                     const int *__restrict__ accepted, int win, int N_blb, IaMag M, IaCell C,
                                                     double *__restrict__ FT, double *__restrict__ e)
{
  __shared__ double red[7][NT];
  ia_body_dipoles_per<NT>(red, X, Q, mb, tf, accepted, win, N_blb, M, C, FT, e);
}

// ... and in the cell of the body's window, one per replica
template <int NT>
__global__ __launch_bounds__(NT) void k_body_dipoles_cells(const double *__restrict__ X, const double *__restrict__ Q,
                                                           const double *__restrict__ mb, const double *__restrict__ tf,
                                                           const int *__restrict__ accepted, int win, int N_blb, IaMag M,
                                                           const RblEnsCellRec *__restrict__ cells, double *__restrict__ FT,
                                                           double *__restrict__ e)
{
  __shared__ double red[7][NT];
  ia_body_dipoles_per<NT>(red, X, Q, mb, tf, accepted, win, N_blb, M, ia_cell_of(cells, blockIdx.x / win), FT, e);
}

struct IaLayout {
  double *f, *e, *ft;
  int *cnt, *list, *np;
};

int ia_cap(int N_bod) { return std::max(1, std::min(N_bod - 1, IA_CAP_MAX)); }

// d_ia = f_blob [3 N] | energy per blob [N] | K^T f [6 N_bod] | neighbour counts [N_bod] | lists [N_bod x cap] | pairs per blob [N]
size_t ia_bytes(int nb, int nblb, int cap)
{
  const size_t N = (size_t)nb * nblb;
  return sizeof(double) * (4 * N + 6 * (size_t)nb) + sizeof(int) * ((size_t)nb * (1 + (size_t)cap) + N);
}

IaLayout ia_layout(void *p, int nb, int nblb, int cap)
{
  const size_t N = (size_t)nb * nblb;
  IaLayout L;
  L.f = (double *)p;
  L.e = L.f + 3 * N;
  L.ft = L.e + N;
  L.cnt = (int *)(L.ft + 6 * (size_t)nb);
  L.list = L.cnt + nb;
  L.np = L.list + (size_t)nb * cap;
  return L;
}

int ia_reserve(rbl_ctx *c, IaLayout &L)
{
  const RblBodyState &S = c->S;
  const int cap = ia_cap(S.N_bod);
  int rc = rbl_dev_reserve(c, c->d_ia, ia_bytes(S.N_bod, S.N_blb, cap)); if (rc) return rc;
  L = ia_layout(c->d_ia.p, S.N_bod, S.N_blb, cap);
  return RBL_OK;
}

}  // namespace

static bool ia_dp_pairs(const rbl_ctx *c) { return c->ia_dp_on && c->ia_dp_c > 0.0; }
static bool ia_dp_field(const rbl_ctx *c) { return c->ia_dp_on && c->ia_mf_on; }
static bool ia_bonds(const rbl_ctx *c) { return c->ia_bd_on && c->ia_bd_n > 0; }
// the type tables that can be reached: both types below n_types (the entries of an unordered pair are ordered by the larger type)
static int ia_ty_usable(const rbl_ctx *c) { return c->ia_ty_nt * (c->ia_ty_nt + 1) / 2; }
// the largest cutoff of a usable type table that is on, 0: none -- the typed term is evaluated only while this is positive
static double ia_typed_rcut(const rbl_ctx *c)
{
  double rc = 0.0;
  if (c->ia_ty_on)
    for (int q = 0; q < ia_ty_usable(c); ++q)
      if (c->ia_tt[q].on) rc = std::max(rc, c->ia_tt[q].hi);
  return rc;
}
static bool ia_typed(const rbl_ctx *c) { return ia_typed_rcut(c) > 0.0; }

bool ia_any(const rbl_ctx *c)
{
  return c->ia_on || c->ia_pt.on || c->ia_ht.on || c->ia_tr_on || ia_dp_pairs(c) || ia_dp_field(c) || ia_bonds(c) || ia_typed(c);
}

// the tables' coefficients and the traps on the device (once per rbl_set_pair_table / rbl_set_height_table / rbl_set_bond_table /
// rbl_set_traps):
// pair coefficients | height coefficients | bond coefficients | trap k | trap X0.  4 (n - 1) doubles per table: every interval
// starts 32-byte aligned
static int ia_upload(rbl_ctx *c)
{
  if (c->ia_tab_valid) return RBL_OK;
  const std::vector<double> *part[5] = {&c->ia_pt.coef, &c->ia_ht.coef, &c->ia_bt.coef, &c->ia_tr_k, &c->ia_tr_X0};
  size_t n = 0;
  for (const std::vector<double> *v : part) n += v->size();
  if (n) {
    int rc = rbl_dev_reserve(c, c->d_iat, sizeof(double) * n); if (rc) return rc;
    double *d = (double *)c->d_iat.p;
    for (const std::vector<double> *v : part) {
      if (!v->empty() && (rc = copy_h2d(c, d, v->data(), sizeof(double) * v->size()))) return rc;
      d += v->size();
    }
    RBL_HIP(c, hipStreamSynchronize(c->stream));
  }
  c->ia_tab_valid = true;
  return RBL_OK;
}

// the body-frame moments and the field times on the device: moments | times.  rbl_set_dipoles invalidates both, rbl_set_field_time
// the times alone, so the loop that sets the time before every step uploads n doubles per step and not the moments again
static int ia_mag_upload(rbl_ctx *c)
{
  if (c->ia_mag_valid && c->ia_ft_valid) return RBL_OK;
  const size_t nm = c->ia_dp_m.size(), nt = c->ia_ft.size(), need = sizeof(double) * (nm + nt);
  const bool moments = !c->ia_mag_valid || need > c->d_iam.bytes;     // a buffer that has to grow loses what it held
  int rc = rbl_dev_reserve(c, c->d_iam, need); if (rc) return rc;
  double *d = (double *)c->d_iam.p;
  if (moments && nm && (rc = copy_h2d(c, d, c->ia_dp_m.data(), sizeof(double) * nm))) return rc;
  if ((rc = copy_h2d(c, d + nm, c->ia_ft.data(), sizeof(double) * nt))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  c->ia_mag_valid = c->ia_ft_valid = true;
  return RBL_OK;
}

static IaTab ia_tab_args(const rbl_ctx::IaTable &t, const double *d_coef)
{
  IaTab T = {};
  if (!t.on) return T;
  T.coef = (const double4 *)d_coef;
  T.lo = t.lo; T.hi = t.hi;
  T.inv_h = (double)(t.n - 1) / (t.hi - t.lo);
  T.U0 = t.coef[0]; T.dU0 = t.dU0;
  T.hi2 = t.hi * t.hi * (1.0 + 1e-15);
  T.last = t.n - 2;
  return T;
}

// the typed term on the device, once per rbl_set_blob_types / rbl_set_type_table / rbl_clear_type_tables: one descriptor per
// unordered type pair (no usable table that is on: hi = hi2 = -1, no distance is inside it) | the coefficients of the usable
// tables that are on | the types.  The descriptors hold device addresses of this buffer, so they are built here
static int ia_ty_upload(rbl_ctx *c)
{
  if (c->ia_ty_valid) return RBL_OK;
  size_t ncoef = 0;
  for (int q = 0; q < ia_ty_usable(c); ++q)
    if (c->ia_tt[q].on) ncoef += c->ia_tt[q].coef.size();
  int rc = rbl_dev_reserve(c, c->d_iaty, sizeof(IaTab) * IA_TY_PAIRS + sizeof(double) * ncoef + sizeof(int) * c->ia_ty.size());
  if (rc) return rc;
  IaTab desc[IA_TY_PAIRS];
  double *d = (double *)((IaTab *)c->d_iaty.p + IA_TY_PAIRS);
  for (int q = 0; q < IA_TY_PAIRS; ++q) {
    const rbl_ctx::IaTable &t = c->ia_tt[q];
    desc[q] = IaTab{};
    desc[q].hi = desc[q].hi2 = -1.0;
    if (q >= ia_ty_usable(c) || !t.on) continue;
    desc[q] = ia_tab_args(t, d);
    if ((rc = copy_h2d(c, d, t.coef.data(), sizeof(double) * t.coef.size()))) return rc;
    d += t.coef.size();
  }
  if ((rc = copy_h2d(c, c->d_iaty.p, desc, sizeof(desc)))) return rc;
  if (!c->ia_ty.empty() && (rc = copy_h2d(c, d, c->ia_ty.data(), sizeof(int) * c->ia_ty.size()))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  c->ia_ty_valid = true;
  return RBL_OK;
}

// after ia_ty_upload
static IaTyped ia_typed_args(const rbl_ctx *c, double cmax2, bool per_row)
{
  size_t ncoef = 0;
  for (int q = 0; q < ia_ty_usable(c); ++q)
    if (c->ia_tt[q].on) ncoef += c->ia_tt[q].coef.size();
  IaTyped Y;
  Y.desc = (const IaTab *)c->d_iaty.p;
  Y.type = (const int *)((const double *)(Y.desc + IA_TY_PAIRS) + ncoef);
  Y.cmax2 = cmax2;
  Y.per_row = per_row ? 1 : 0;
  return Y;
}

// what an evaluation over windows of `win` bodies needs of the bonds (no device touched)
static int ia_bond_check(rbl_ctx *c, const char *who, int win, int n_win)
{
  if (c->ia_bd_top >= win)
    for (int b = 0; b < c->ia_bd_n; ++b) {
      const int m = std::max(c->ia_bd_body[2 * (size_t)b], c->ia_bd_body[2 * (size_t)b + 1]);
      if (m >= win)
        return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": bond " + std::to_string(b) + " names body " + std::to_string(m) +
                                              ", the system has " + std::to_string(win) + " bodies (rbl_set_bonds)");
    }
  if (n_win > 1 && c->ia_bd_sets != 1 && c->ia_bd_sets != n_win)
    return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": the bonds hold neither one parameter set nor one per replica (rbl_set_bonds)");
  if (!c->ia_bt.on && c->ia_bd_tab >= 0)
    return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": bond " + std::to_string(c->ia_bd_tab) + " is tabulated (kind 1) and no bond table is on (rbl_set_bond_table)");
  return RBL_OK;
}

// the bonds on the device, once per rbl_set_bonds: anchors | parameters | kinds | bodies | rows | row starts | ends
static int ia_bond_upload(rbl_ctx *c)
{
  if (c->ia_bd_valid) return RBL_OK;
  const std::vector<double> *dpart[2] = {&c->ia_bd_anchor, &c->ia_bd_param};
  const std::vector<int> *ipart[5] = {&c->ia_bd_kind, &c->ia_bd_body, &c->ia_bd_rows, &c->ia_bd_ptr, &c->ia_bd_ends};
  size_t nd = 0, ni = 0;
  for (const std::vector<double> *v : dpart) nd += v->size();
  for (const std::vector<int> *v : ipart) ni += v->size();
  int rc = rbl_dev_reserve(c, c->d_iab, sizeof(double) * nd + sizeof(int) * ni); if (rc) return rc;
  double *d = (double *)c->d_iab.p;
  for (const std::vector<double> *v : dpart) {
    if (!v->empty() && (rc = copy_h2d(c, d, v->data(), sizeof(double) * v->size()))) return rc;
    d += v->size();
  }
  int *q = (int *)d;
  for (const std::vector<int> *v : ipart) {
    if (!v->empty() && (rc = copy_h2d(c, q, v->data(), sizeof(int) * v->size()))) return rc;
    q += v->size();
  }
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  c->ia_bd_valid = true;
  return RBL_OK;
}

// after ia_upload and ia_bond_upload
static IaBonds ia_bond_args(const rbl_ctx *c, int n_win)
{
  IaBonds B = {};
  B.anchor = (const double *)c->d_iab.p;
  B.param = B.anchor + c->ia_bd_anchor.size();
  B.kind = (const int *)(B.param + c->ia_bd_param.size());
  B.body = B.kind + c->ia_bd_kind.size();
  B.rows = B.body + c->ia_bd_body.size();
  B.ptr = B.rows + c->ia_bd_rows.size();
  B.ends = B.ptr + c->ia_bd_ptr.size();
  B.BT.T = ia_tab_args(c->ia_bt, (const double *)c->d_iat.p + c->ia_pt.coef.size() + c->ia_ht.coef.size());
  B.BT.U1 = c->ia_bt.U1; B.BT.dU1 = c->ia_bt.dU1;
  B.n = c->ia_bd_n; B.n_rows = (int)c->ia_bd_rows.size();
  B.per_set = n_win > 1 && c->ia_bd_sets != 1 ? 1 : 0;     // a single context uses set 0
  return B;
}

// ---- the pieces of the model's kernel arguments that ia_launch and ia_mc_model (the Metropolis sampler's) both take: ONE builder each
// the built-in terms (switched off: no weight, no wall term, no pair inside a negative cutoff)
static IaParams ia_params(const rbl_ctx *c)
{
  const RblBodyState &S = c->S;
  IaParams P;
  P.w = c->ia_w; P.a = S.a; P.eps_w = c->ia_eps_wall; P.inv_bw = 1.0 / c->ia_b_wall; P.eps_b = c->ia_eps_blob;
  P.inv_bb = 1.0 / c->ia_b_blob; P.two_a = 2.0 * S.a; P.rc2 = c->ia_r_cut * c->ia_r_cut; P.wall = S.wall ? 1 : 0;
  if (!c->ia_on) { P.w = 0.0; P.wall = 0; P.eps_b = 0.0; P.rc2 = -1.0; }   // no pair is inside a negative cutoff
  return P;
}
// R_body^2: largest blob distance from the centre, body frame (mean removed)
static double ia_body_R2(const rbl_ctx *c)
{
  double R2 = 0.0;
  for (int k = 0; k < c->S.N_blb; ++k) {
    const double *q = &c->S.ref_cfg[3 * (size_t)k];
    R2 = std::max(R2, q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  }
  return R2;
}
// the larger cutoff of the pair terms that are on
static double ia_rc_max(const rbl_ctx *c, double rc_typed)
{
  return std::max(std::max(c->ia_on ? c->ia_r_cut : 0.0, c->ia_pt.on ? c->ia_pt.hi : 0.0), rc_typed);
}
// the body-level cull's radius.  A hair of slack for the rounding of the rotated lever arms and of the distances: it can only add
// candidates, whose pairs beyond the cutoffs are then skipped one by one
static double ia_cull_cut(const rbl_ctx *c, double rc_typed)
{
  return (2.0 * std::sqrt(ia_body_R2(c)) + ia_rc_max(c, rc_typed)) * (1.0 + 1e-12) + 1e-12;
}
// the largest cutoff^2 of the pair terms that are on, each rounded as its own test takes it (rc2; hi^2 a hair up)
static double ia_cmax2(const rbl_ctx *c, const IaParams &P, const IaTab &PT, double rc_typed)
{
  return std::max(std::max(P.rc2, c->ia_pt.on ? PT.hi2 : -1.0), rc_typed > 0.0 ? rc_typed * rc_typed * (1.0 + 1e-15) : -1.0);
}
static IaCell ia_cell_value(const double *per_L)
{
  IaCell C = {};
  C.Lx = per_L[0]; C.Ly = per_L[1];
  C.px = C.Lx > 0.0 ? 1 : 0; C.py = C.Ly > 0.0 ? 1 : 0;
  C.iLx = C.px ? 1.0 / C.Lx : 0.0; C.iLy = C.py ? 1.0 / C.Ly : 0.0;
  return C;
}
// the tables in d_iat (ia_upload's order): pair | height | bond coefficients | trap k | trap X0
static const double *ia_height_coef(const rbl_ctx *c) { return (const double *)c->d_iat.p + c->ia_pt.coef.size(); }
static const double *ia_trap_k(const rbl_ctx *c) { return ia_height_coef(c) + c->ia_ht.coef.size() + c->ia_bt.coef.size(); }

// the model over n_win windows of win bodies each (resident X of the body centres, blob positions and lever arms): neighbour
// lists inside each window, the pair kernel, K^T f.  d_f (3 N) is required here; d_FT (6 N_bod total) and d_e may be NULL.
// d_Q: the orientations beside d_X (the dipoles); d_accepted: a run's per-replica step counters, the field's clock (NULL: the
// field time as set).  ens: called for an ensemble -- the cell is the ensemble's (rbl_ensemble_set_periodic), not the single context's
static int ia_launch(rbl_ctx *c, const double *d_X, const double *d_Q, const double *d_pos, const double *d_lever, int win, int n_win,
                     double *d_cl, double *d_f, double *d_FT, double *d_e, unsigned *d_err, const int *d_accepted = nullptr, bool ens = false)
{
  const RblBodyState &S = c->S;
  if (c->ia_on && !(c->ia_r_cut >= 2.0 * S.a))           // the built-in term's own check: a context with only a table on has r_cut = 0
    return rbl_fail(c, RBL_ERR_STATE, "interactions: r_cut is below 2a of the current parameters (call rbl_set_interactions again)");
  const int nbod = win * n_win, cap = ia_cap(win);
  const size_t ntr = c->ia_tr_k.size() / 3;
  if (c->ia_tr_on && ntr != (size_t)win && ntr != (size_t)nbod)
    return rbl_fail(c, RBL_ERR_STATE, "interactions: the traps hold neither one entry per body nor one per body of every replica (rbl_set_traps)");
  const bool dp_pairs = ia_dp_pairs(c), dp_field = ia_dp_field(c), dp = dp_pairs || dp_field;
  const size_t ndm = c->ia_dp_m.size() / 3, nft = c->ia_ft.size();
  if (dp && ndm != 1 && ndm != (size_t)win && ndm != (size_t)nbod)
    return rbl_fail(c, RBL_ERR_STATE, "interactions: the dipole moments hold neither one entry, nor one per body, nor one per body of every replica (rbl_set_dipoles)");
  if (dp_field && n_win > 1 && nft != 1 && nft != (size_t)n_win)
    return rbl_fail(c, RBL_ERR_STATE, "interactions: the field time holds neither one entry nor one per replica (rbl_set_field_time)");
  const bool bonds = ia_bonds(c);
  int rc;
  if (bonds && (rc = ia_bond_check(c, "interactions", win, n_win))) return rc;
  const double rc_typed = ia_typed_rcut(c);
  const bool typed = rc_typed > 0.0;
  const size_t nty = c->ia_ty.size();
  if (typed && nty != (size_t)S.N_blb && nty != (size_t)win * S.N_blb)
    return rbl_fail(c, RBL_ERR_STATE, "interactions: the blob types hold neither one entry per blob of a body nor one per blob of the system (rbl_set_blob_types)");
  // a periodic cell (include/rbl.h section 10): minimum image in the neighbour search, the blob pair terms and the dipole pairs.
  // The convention is unique only while no pair inside a cutoff has a second image inside it: blobs of two bodies lie within
  // 2 R_body + r_cut of each other's centres, dipoles sit on the centres themselves
  // An ensemble with a cell per replica (rbl_ensemble_set_cells): the bounds replica by replica, the first offending one named, and
  // the kernels read the cell of a body's window from the table
  IaCell C = {};
  const bool per = ens ? c->ens_per_on : periodic_on(c);
  const bool tab_cells = ens && per && ens_cells_stored(c);
  const int n_cells = tab_cells ? (int)(c->ens_cells_L.size() / 2) : 1;
  if (tab_cells && n_cells != n_win)
    return rbl_fail(c, RBL_ERR_STATE, "interactions: the cells are stored for " + std::to_string(n_cells) + " replicas, the evaluation has " +
                                          std::to_string(n_win) + " (rbl_ensemble_set_cells)");
  if (per) {
    const double R2b = ia_body_R2(c), rc_pair = ia_rc_max(c, rc_typed);
    const double need_pair = (c->ia_on || c->ia_pt.on || typed) ? 2.0 * std::sqrt(R2b) + rc_pair : 0.0;
    const double need_dp = dp_pairs ? c->ia_dp_rcut : 0.0;
    for (int r = 0; r < n_cells; ++r) {
      const double *per_L = tab_cells ? &c->ens_cells_L[2 * (size_t)r] : ens ? c->ens_per_L : c->per_L;
      for (int k = 0; k < 2; ++k) {
        const double Lk = per_L[k];
        if (!(Lk > 0.0) || (need_pair <= 0.5 * Lk && need_dp <= 0.5 * Lk)) continue;     // (a run checks R cells per step: no strings here)
        const std::string head = tab_cells ? "interactions: replica " + std::to_string(r) + ": periodic cell too small: "
                                           : std::string("interactions: periodic cell too small: ");
        const std::string Ln = std::string("L") + (k ? "y" : "x") + " = " + std::to_string(Lk);
        if (need_pair > 0.5 * Lk)
          return rbl_fail(c, RBL_ERR_ARG, head + Ln + " needs 2 R_body + r_cut = " + std::to_string(need_pair) +
                                              " <= L / 2 = " + std::to_string(0.5 * Lk) + " for a unique minimum image");
        if (need_dp > 0.5 * Lk)
          return rbl_fail(c, RBL_ERR_ARG, head + Ln + " needs the dipole r_cut = " + std::to_string(need_dp) +
                                              " <= L / 2 = " + std::to_string(0.5 * Lk) + " for a unique minimum image");
      }
      if (tab_cells) continue;
      C = ia_cell_value(per_L);
    }
  }
  if (tab_cells && (rc = ens_cells_upload(c))) return rc;   // (current already unless the parameters changed since the cells were set)
  const RblEnsCellRec *cells = tab_cells ? (const RblEnsCellRec *)c->d_ens_cells.p : nullptr;
  if ((rc = ia_upload(c))) return rc;
  if (dp && (rc = ia_mag_upload(c))) return rc;
  if (bonds && (rc = ia_bond_upload(c))) return rc;
  if (typed && (rc = ia_ty_upload(c))) return rc;
  RblPhase ph(c, RBL_T_FORCES);
  IaLayout L = ia_layout(d_cl, nbod, S.N_blb, cap);
  const double cut = ia_cull_cut(c, rc_typed);
  if (cells)
    hipLaunchKernelGGL(k_body_neighbours_cells, dim3(nbod), dim3(64), 0, c->stream, d_X, nbod, win, cut * cut, c->ia_cull ? 1 : 0, cap,
                       cells, L.cnt, L.list, d_err);
  else if (per)
    hipLaunchKernelGGL(k_body_neighbours_per, dim3(nbod), dim3(64), 0, c->stream, d_X, nbod, win, cut * cut, c->ia_cull ? 1 : 0, cap,
                       C, L.cnt, L.list, d_err);
  else
    hipLaunchKernelGGL(k_body_neighbours, dim3(nbod), dim3(64), 0, c->stream, d_X, nbod, win, cut * cut, c->ia_cull ? 1 : 0, cap,
                       L.cnt, L.list, d_err);
  const IaParams P = ia_params(c);
  const int bt = S.N_blb > 128 ? IA_BT : (S.N_blb + 63) / 64 * 64, tiles = (S.N_blb + bt - 1) / bt;
  const dim3 grid((unsigned)(tiles * nbod));
  const int tab = (c->ia_pt.on ? 1 : 0) | (c->ia_ht.on ? 2 : 0);
  const double *T = (const double *)c->d_iat.p;
  const IaTab PT = ia_tab_args(c->ia_pt, T), HT = ia_tab_args(c->ia_ht, ia_height_coef(c));
#define RBL_IA_TAB(K)                                                                                                              \
  hipLaunchKernelGGL(k_blob_interactions_tab<K>, grid, dim3(bt), 0, c->stream, d_pos, (const int *)L.cnt, (const int *)L.list, cap, \
                     S.N_blb, tiles, P, PT, HT, d_f, d_e, L.np)
#define RBL_IA_PER(K)                                                                                                              \
  hipLaunchKernelGGL(k_blob_interactions_per<K>, grid, dim3(bt), 0, c->stream, d_pos, (const int *)L.cnt, (const int *)L.list, cap, \
                     S.N_blb, tiles, P, PT, HT, C, d_f, d_e, L.np)
#define RBL_IA_CELLS(K)                                                                                                              \
  hipLaunchKernelGGL(k_blob_interactions_cells<K>, grid, dim3(bt), 0, c->stream, d_pos, (const int *)L.cnt, (const int *)L.list, cap, \
                     S.N_blb, tiles, win, P, PT, HT, cells, d_f, d_e, L.np)
  if (typed) {
    const double cmax2 = ia_cmax2(c, P, PT, rc_typed);
    const IaTyped Y = ia_typed_args(c, cmax2, nty != (size_t)S.N_blb);
#define RBL_IA_TYPED(K, CELL)                                                                                                        \
  hipLaunchKernelGGL((k_blob_interactions_typed<K, CELL>), grid, dim3(bt), 0, c->stream, d_pos, (const int *)L.cnt,                 \
                     (const int *)L.list, cap, S.N_blb, tiles, win, P, PT, HT, Y, C, cells, d_f, d_e, L.np)
#define RBL_IA_TYPED_TAB(CELL)                                                                                                       \
  do {                                                                                                                               \
    if (tab == 0) RBL_IA_TYPED(0, CELL);                                                                                             \
    else if (tab == 1) RBL_IA_TYPED(1, CELL);                                                                                        \
    else if (tab == 2) RBL_IA_TYPED(2, CELL);                                                                                        \
    else RBL_IA_TYPED(3, CELL);                                                                                                      \
  } while (0)
    if (cells) RBL_IA_TYPED_TAB(2);
    else if (per) RBL_IA_TYPED_TAB(1);
    else RBL_IA_TYPED_TAB(0);
#undef RBL_IA_TYPED_TAB
#undef RBL_IA_TYPED
  } else if (cells) {
    if (tab == 0) RBL_IA_CELLS(0);
    else if (tab == 1) RBL_IA_CELLS(1);
    else if (tab == 2) RBL_IA_CELLS(2);
    else RBL_IA_CELLS(3);
  } else if (per) {
    if (tab == 0) RBL_IA_PER(0);
    else if (tab == 1) RBL_IA_PER(1);
    else if (tab == 2) RBL_IA_PER(2);
    else RBL_IA_PER(3);
  } else if (tab == 0)
    hipLaunchKernelGGL(k_blob_interactions, grid, dim3(bt), 0, c->stream, d_pos, (const int *)L.cnt, (const int *)L.list, cap,
                       S.N_blb, tiles, P, d_f, d_e, L.np);
  else if (tab == 1) RBL_IA_TAB(1);
  else if (tab == 2) RBL_IA_TAB(2);
  else RBL_IA_TAB(3);
#undef RBL_IA_TAB
#undef RBL_IA_PER
#undef RBL_IA_CELLS
  if (d_FT) rbl_launch_KT_x_Lam(c->stream, d_lever, d_f, S.N_blb, nbod, d_FT);
  if (c->ia_tr_on && (d_FT || d_e)) {
    const double *k3 = ia_trap_k(c);
    hipLaunchKernelGGL(k_body_traps, dim3((unsigned)((nbod + 255) / 256)), dim3(256), 0, c->stream, d_X, k3, k3 + 3 * ntr, nbod,
                       (int)ntr, S.N_blb, d_FT, d_e);
  }
  if (dp && (d_FT || d_e)) {
    IaMag M;
    std::memcpy(M.B, c->ia_mf_B, sizeof(M.B));
    M.omega = c->ia_mf_omega; M.dt = S.dt; M.c_dd = c->ia_dp_c; M.r_core = c->ia_dp_rcore; M.r_cut = c->ia_dp_rcut;
    M.pairs = dp_pairs ? 1 : 0; M.field = dp_field ? 1 : 0;
    M.per_m = (int)ndm; M.per_t = n_win > 1 ? (int)nft : 1;  // a single context uses entry 0
    const double *mb = (const double *)c->d_iam.p, *tf = mb + 3 * ndm;
    if (!per && win > 512)
      hipLaunchKernelGGL(k_body_dipoles<256>, dim3((unsigned)nbod), dim3(256), 0, c->stream, d_X, d_Q, mb, tf, d_accepted, win,
                         S.N_blb, M, d_FT, d_e);
    else if (!per)
      hipLaunchKernelGGL(k_body_dipoles<64>, dim3((unsigned)nbod), dim3(64), 0, c->stream, d_X, d_Q, mb, tf, d_accepted, win,
                         S.N_blb, M, d_FT, d_e);
    else if (cells && win > 512)
      hipLaunchKernelGGL(k_body_dipoles_cells<256>, dim3((unsigned)nbod), dim3(256), 0, c->stream, d_X, d_Q, mb, tf, d_accepted, win,
                         S.N_blb, M, cells, d_FT, d_e);
    else if (cells)
      hipLaunchKernelGGL(k_body_dipoles_cells<64>, dim3((unsigned)nbod), dim3(64), 0, c->stream, d_X, d_Q, mb, tf, d_accepted, win,
                         S.N_blb, M, cells, d_FT, d_e);
    else if (win > 512)
      hipLaunchKernelGGL(k_body_dipoles_per<256>, dim3((unsigned)nbod), dim3(256), 0, c->stream, d_X, d_Q, mb, tf, d_accepted, win,
                         S.N_blb, M, C, d_FT, d_e);
    else
      hipLaunchKernelGGL(k_body_dipoles_per<64>, dim3((unsigned)nbod), dim3(64), 0, c->stream, d_X, d_Q, mb, tf, d_accepted, win,
                         S.N_blb, M, C, d_FT, d_e);
  }
  if (bonds && (d_FT || d_e)) {
    const IaBonds B = ia_bond_args(c, n_win);
    hipLaunchKernelGGL(k_body_bonds, dim3((unsigned)((size_t)B.n_rows * n_win)), dim3(64), 0, c->stream, d_X, d_Q, win, S.N_blb, B,
                       d_FT, d_e);
  }
  return RBL_OK;
}

int ia_eval(rbl_ctx *c, double *d_f, double *d_FT, double *d_e)
{
  int rc = sync_bodies(c); if (rc) return rc;            // resident positions and lever arms of the current configuration
  const RblBodyState &S = c->S;
  IaLayout L;
  if ((rc = ia_reserve(c, L))) return rc;
  const double *dX = (const double *)c->d_XQ.p;
  if ((rc = ia_launch(c, dX, dX + 3 * (size_t)S.N_bod, (const double *)c->d_pos.p, (const double *)c->d_lever.p, S.N_bod, 1,
                      (double *)c->d_ia.p, d_f ? d_f : L.f, d_FT, d_e, c->d_err))) return rc;
  c->ia_nb = S.N_bod; c->ia_nblb = S.N_blb; c->ia_cap = ia_cap(S.N_bod);
  return RBL_OK;
}

size_t ia_batch_bytes(int N_bod, int N_blb, int reps)
{
  return ia_bytes(N_bod * reps, N_blb, ia_cap(N_bod));
}

int ia_eval_batch(rbl_ctx *c, const double *d_X, const double *d_Q, const double *d_pos, const double *d_lever, int N_bod, int reps,
                  void *d_work, double **d_f, double *d_FT, double *d_e, unsigned *d_err, const int *d_accepted)
{
  IaLayout L = ia_layout(d_work, N_bod * reps, c->S.N_blb, ia_cap(N_bod));
  *d_f = L.f;
  return ia_launch(c, d_X, d_Q, d_pos, d_lever, N_bod, reps, (double *)d_work, L.f, d_FT, d_e, d_err, d_accepted, true);
}

// the model as the Metropolis kernel takes it (rbl_forces_dev.hpp): ia_launch's own arguments, from the same builders, for an
// ensemble of n_win replicas.  The caller has just evaluated the model on the same ensemble (ia_eval_batch), which made every check
// and upload; the dipole terms are the caller's to refuse
IaMcModel ia_mc_model(const rbl_ctx *c, int n_win)
{
  IaMcModel M = {};
  M.p = ia_params(c);
  M.tab = (c->ia_pt.on ? 1 : 0) | (c->ia_ht.on ? 2 : 0);
  M.PT = ia_tab_args(c->ia_pt, (const double *)c->d_iat.p);
  M.HT = ia_tab_args(c->ia_ht, ia_height_coef(c));
  const double rc_typed = ia_typed_rcut(c);
  M.typed = rc_typed > 0.0 ? 1 : 0;
  const double cmax2 = ia_cmax2(c, M.p, M.PT, rc_typed);
  if (M.typed) M.Y = ia_typed_args(c, cmax2, c->ia_ty.size() != (size_t)c->S.N_blb);
  M.Y.cmax2 = cmax2;
  M.bonds = ia_bonds(c) ? 1 : 0;
  if (M.bonds) M.B = ia_bond_args(c, n_win);
  M.per = !c->ens_per_on ? 0 : ens_cells_stored(c) ? 2 : 1;
  if (M.per == 1) M.C = ia_cell_value(c->ens_per_L);
  M.cells = M.per == 2 ? (const RblEnsCellRec *)c->d_ens_cells.p : nullptr;
  const size_t ntr = c->ia_tr_k.size() / 3;
  M.tr_per = c->ia_tr_on ? (int)ntr : 0;
  M.tr_k = ia_trap_k(c);
  M.tr_X0 = M.tr_k + 3 * ntr;
  const double cut = ia_cull_cut(c, rc_typed);
  M.cull2 = cut * cut;
  M.cull = c->ia_cull ? 1 : 0;
  return M;
}

int ia_add_to_step_force(rbl_ctx *c, double *d_force)
{
  if (!ia_any(c)) return RBL_OK;
  IaLayout L;
  int rc = ia_reserve(c, L); if (rc) return rc;
  if ((rc = ia_eval(c, nullptr, L.ft, nullptr))) return rc;
  rbl_launch_axpby(c->stream, 6 * (int64_t)c->S.N_bod, 1.0, d_force, -1.0, L.ft, d_force);   // reference convention: F_body - K^T f_phys
  return finish_and_check(c);
}

// ---- C ABI (include/rbl.h section 4) --------------------------------------------------------------------------------

int rbl_set_interactions(rbl_ctx *c, double w, double eps_wall, double b_wall, double eps_blob, double b_blob, double r_cut, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!c->S.params_set) return rbl_fail(c, RBL_ERR_STATE, "set_interactions: setParameters has not been called (r_cut is checked against 2a)");
  const double v[6] = {w, eps_wall, b_wall, eps_blob, b_blob, r_cut};
  for (double x : v)
    if (!std::isfinite(x)) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: every parameter must be finite");
  if (!(b_wall > 0.0) || !(b_blob > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: b_wall and b_blob must be positive");
  if (eps_wall < 0.0 || eps_blob < 0.0) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: eps_wall and eps_blob must be >= 0 (repulsions)");
  if (!(r_cut >= 2.0 * c->S.a)) return rbl_fail(c, RBL_ERR_ARG, "set_interactions: r_cut must be >= 2a");
  c->ia_w = w; c->ia_eps_wall = eps_wall; c->ia_b_wall = b_wall; c->ia_eps_blob = eps_blob; c->ia_b_blob = b_blob; c->ia_r_cut = r_cut;
  c->ia_on = on != 0;
  return RBL_OK;
}

int rbl_get_interactions(const rbl_ctx *c, double *params6, int *on)
{
  if (!c) return RBL_ERR_ARG;
  if (params6) {
    const double v[6] = {c->ia_w, c->ia_eps_wall, c->ia_b_wall, c->ia_eps_blob, c->ia_b_blob, c->ia_r_cut};
    std::memcpy(params6, v, sizeof(v));
  }
  if (on) *on = c->ia_on ? 1 : 0;
  return RBL_OK;
}

// one tabulated term: checks, then the four Hermite coefficients per interval (include/rbl.h section 4).  Nothing is stored
// unless every check passes.  U = dU = NULL with on = 0 only switches the term off and keeps its table
static int ia_set_table(rbl_ctx *c, const char *who, rbl_ctx::IaTable &t, const double *U, const double *dU, int n, double lo, double hi,
                        bool lo_nonneg, int on)
{
  if (!U && !dU && !on) { t.on = false; return RBL_OK; }
  if (!U || !dU) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": U and dU must not be NULL");
  if (n < 2 || n > 65537) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": n must lie in [2, 65537]");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || (lo_nonneg && lo < 0.0))
    return rbl_fail(c, RBL_ERR_ARG, std::string(who) + (lo_nonneg ? ": needs finite 0 <= r_min < r_cut" : ": needs finite h_min < h_cut"));
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(U[k]) || !std::isfinite(dU[k])) return rbl_fail(c, RBL_ERR_ARG, std::string(who) + ": every value of U and dU must be finite");
  const double h = (hi - lo) / (double)(n - 1);
  std::vector<double> coef(4 * (size_t)(n - 1));
  for (int k = 0; k + 1 < n; ++k) {
    const double D0 = h * dU[k], D1 = h * dU[k + 1];
    double *q = &coef[4 * (size_t)k];
    q[0] = U[k];
    q[1] = D0;
    q[2] = 3.0 * (U[k + 1] - U[k]) - 2.0 * D0 - D1;
    q[3] = 2.0 * (U[k] - U[k + 1]) + D0 + D1;
  }
  t.coef.swap(coef);
  t.n = n; t.lo = lo; t.hi = hi; t.dU0 = dU[0];
  t.U1 = U[n - 1]; t.dU1 = dU[n - 1];
  t.on = on != 0;
  c->ia_tab_valid = false;
  return RBL_OK;
}

static int ia_get_table(const rbl_ctx::IaTable &t, int *n, double *lo, double *hi, int *on, double *coef)
{
  if (n) *n = t.n;
  if (lo) *lo = t.lo;
  if (hi) *hi = t.hi;
  if (on) *on = t.on ? 1 : 0;
  if (coef && !t.coef.empty()) std::memcpy(coef, t.coef.data(), sizeof(double) * t.coef.size());
  return RBL_OK;
}

int rbl_set_pair_table(rbl_ctx *c, const double *U, const double *dU, int n, double r_min, double r_cut, int on)
{
  if (!c) return RBL_ERR_ARG;
  return ia_set_table(c, "set_pair_table", c->ia_pt, U, dU, n, r_min, r_cut, true, on);
}

int rbl_get_pair_table(const rbl_ctx *c, int *n, double *r_min, double *r_cut, int *on, double *coef)
{
  if (!c) return RBL_ERR_ARG;
  return ia_get_table(c->ia_pt, n, r_min, r_cut, on, coef);
}

int rbl_set_height_table(rbl_ctx *c, const double *U, const double *dU, int n, double h_min, double h_cut, int on)
{
  if (!c) return RBL_ERR_ARG;
  return ia_set_table(c, "set_height_table", c->ia_ht, U, dU, n, h_min, h_cut, false, on);
}

int rbl_get_height_table(const rbl_ctx *c, int *n, double *h_min, double *h_cut, int *on, double *coef)
{
  if (!c) return RBL_ERR_ARG;
  return ia_get_table(c->ia_ht, n, h_min, h_cut, on, coef);
}

// a type table's slot: the unordered pair (ta, tb); NULL outside [0, 8)
static rbl_ctx::IaTable *ia_type_slot(rbl_ctx *c, int ta, int tb)
{
  if (ta < 0 || ta >= rbl_ctx::IA_TY_MAX || tb < 0 || tb >= rbl_ctx::IA_TY_MAX) return nullptr;
  const int hi = std::max(ta, tb);
  return &c->ia_tt[hi * (hi + 1) / 2 + std::min(ta, tb)];
}

int rbl_set_type_table(rbl_ctx *c, int ta, int tb, const double *U, const double *dU, int n, double r_min, double r_cut, int on)
{
  if (!c) return RBL_ERR_ARG;
  rbl_ctx::IaTable *t = ia_type_slot(c, ta, tb);
  if (!t)
    return rbl_fail(c, RBL_ERR_ARG, "set_type_table: ta = " + std::to_string(ta) + ", tb = " + std::to_string(tb) + ": both types must lie in [0, " +
                                        std::to_string(rbl_ctx::IA_TY_MAX) + ")");
  const bool untyped_valid = c->ia_tab_valid;            // (ia_set_table speaks for the buffer of the untyped tables)
  const int rc = ia_set_table(c, "set_type_table", *t, U, dU, n, r_min, r_cut, true, on);
  c->ia_tab_valid = untyped_valid;
  if (rc == RBL_OK) c->ia_ty_valid = false;
  return rc;
}

int rbl_get_type_table(const rbl_ctx *c, int ta, int tb, int *n, double *r_min, double *r_cut, int *on, double *coef)
{
  if (!c) return RBL_ERR_ARG;
  const rbl_ctx::IaTable *t = ia_type_slot(const_cast<rbl_ctx *>(c), ta, tb);
  if (!t) return RBL_ERR_ARG;
  return ia_get_table(*t, n, r_min, r_cut, on, coef);
}

int rbl_clear_type_tables(rbl_ctx *c)
{
  if (!c) return RBL_ERR_ARG;
  for (rbl_ctx::IaTable &t : c->ia_tt) t = rbl_ctx::IaTable{};
  c->ia_ty_valid = false;
  return RBL_OK;
}

// the blob types: checks first, nothing is stored unless every one passes (include/rbl.h section 4)
int rbl_set_blob_types(rbl_ctx *c, const int *type, int n, int n_types, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!type && !on) { c->ia_ty_on = false; return RBL_OK; }
  if (!type) return rbl_fail(c, RBL_ERR_ARG, "set_blob_types: type must not be NULL");
  if (n < 1) return rbl_fail(c, RBL_ERR_ARG, "set_blob_types: n must be >= 1");
  if (n_types < 1 || n_types > rbl_ctx::IA_TY_MAX)
    return rbl_fail(c, RBL_ERR_ARG, "set_blob_types: n_types = " + std::to_string(n_types) + " must lie in [1, " + std::to_string(rbl_ctx::IA_TY_MAX) + "]");
  for (int k = 0; k < n; ++k)
    if (type[k] < 0 || type[k] >= n_types)
      return rbl_fail(c, RBL_ERR_ARG, "set_blob_types: type[" + std::to_string(k) + "] = " + std::to_string(type[k]) + " must lie in [0, " +
                                          std::to_string(n_types) + ")");
  c->ia_ty.assign(type, type + n);
  c->ia_ty_nt = n_types;
  c->ia_ty_on = on != 0;
  c->ia_ty_valid = false;
  return RBL_OK;
}

int rbl_get_blob_types(const rbl_ctx *c, int *n, int *n_types, int *on, int *type)
{
  if (!c) return RBL_ERR_ARG;
  if (n) *n = (int)c->ia_ty.size();
  if (n_types) *n_types = c->ia_ty_nt;
  if (on) *on = c->ia_ty_on ? 1 : 0;
  if (type && !c->ia_ty.empty()) std::memcpy(type, c->ia_ty.data(), sizeof(int) * c->ia_ty.size());
  return RBL_OK;
}

int rbl_set_traps(rbl_ctx *c, const double *k3, const double *X0, int n_bodies, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!k3 && !X0 && !on) { c->ia_tr_on = false; return RBL_OK; }
  if (!k3 || !X0) return rbl_fail(c, RBL_ERR_ARG, "set_traps: k and X0 must not be NULL");
  if (n_bodies < 1) return rbl_fail(c, RBL_ERR_ARG, "set_traps: n_bodies must be >= 1");
  for (size_t i = 0; i < 3 * (size_t)n_bodies; ++i)
    if (!std::isfinite(k3[i]) || !std::isfinite(X0[i])) return rbl_fail(c, RBL_ERR_ARG, "set_traps: every value of k and X0 must be finite");
  c->ia_tr_k.assign(k3, k3 + 3 * (size_t)n_bodies);
  c->ia_tr_X0.assign(X0, X0 + 3 * (size_t)n_bodies);
  c->ia_tr_on = on != 0;
  c->ia_tab_valid = false;
  return RBL_OK;
}

int rbl_get_traps(const rbl_ctx *c, int *n_bodies, int *on, double *k3, double *X0)
{
  if (!c) return RBL_ERR_ARG;
  if (n_bodies) *n_bodies = (int)(c->ia_tr_k.size() / 3);
  if (on) *on = c->ia_tr_on ? 1 : 0;
  if (k3 && !c->ia_tr_k.empty()) std::memcpy(k3, c->ia_tr_k.data(), sizeof(double) * c->ia_tr_k.size());
  if (X0 && !c->ia_tr_X0.empty()) std::memcpy(X0, c->ia_tr_X0.data(), sizeof(double) * c->ia_tr_X0.size());
  return RBL_OK;
}

// the dipoles: checks first, nothing is stored unless every one passes (include/rbl.h section 4)
int rbl_set_dipoles(rbl_ctx *c, const double *m_body, int n_bodies, double c_dd, double r_core, double r_cut, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!m_body && !on) { c->ia_dp_on = false; return RBL_OK; }
  if (!m_body) return rbl_fail(c, RBL_ERR_ARG, "set_dipoles: m_body must not be NULL");
  if (n_bodies < 1) return rbl_fail(c, RBL_ERR_ARG, "set_dipoles: n_bodies must be >= 1");
  for (size_t i = 0; i < 3 * (size_t)n_bodies; ++i)
    if (!std::isfinite(m_body[i])) return rbl_fail(c, RBL_ERR_ARG, "set_dipoles: every value of m_body must be finite");
  if (!std::isfinite(c_dd) || c_dd < 0.0) return rbl_fail(c, RBL_ERR_ARG, "set_dipoles: c_dd must be finite and >= 0");
  if (c_dd > 0.0) {
    if (!std::isfinite(r_core) || !(r_core > 0.0)) return rbl_fail(c, RBL_ERR_ARG, "set_dipoles: r_core must be finite and positive while c_dd > 0");
    if (std::isnan(r_cut) || !(r_cut > r_core)) return rbl_fail(c, RBL_ERR_ARG, "set_dipoles: r_cut must be larger than r_core (+inf: every pair) while c_dd > 0");
  }
  c->ia_dp_m.assign(m_body, m_body + 3 * (size_t)n_bodies);
  c->ia_dp_c = c_dd; c->ia_dp_rcore = r_core; c->ia_dp_rcut = r_cut;
  c->ia_dp_on = on != 0;
  c->ia_mag_valid = c->ia_ft_valid = false;
  return RBL_OK;
}

int rbl_get_dipoles(const rbl_ctx *c, int *n_bodies, double *c_dd, double *r_core, double *r_cut, int *on, double *m_body)
{
  if (!c) return RBL_ERR_ARG;
  if (n_bodies) *n_bodies = (int)(c->ia_dp_m.size() / 3);
  if (c_dd) *c_dd = c->ia_dp_c;
  if (r_core) *r_core = c->ia_dp_rcore;
  if (r_cut) *r_cut = c->ia_dp_rcut;
  if (on) *on = c->ia_dp_on ? 1 : 0;
  if (m_body && !c->ia_dp_m.empty()) std::memcpy(m_body, c->ia_dp_m.data(), sizeof(double) * c->ia_dp_m.size());
  return RBL_OK;
}

int rbl_set_bond_table(rbl_ctx *c, const double *U, const double *dU, int n, double r_min, double r_cut, int on)
{
  if (!c) return RBL_ERR_ARG;
  return ia_set_table(c, "set_bond_table", c->ia_bt, U, dU, n, r_min, r_cut, true, on);
}

int rbl_get_bond_table(const rbl_ctx *c, int *n, double *r_min, double *r_cut, int *on, double *coef)
{
  if (!c) return RBL_ERR_ARG;
  return ia_get_table(c->ia_bt, n, r_min, r_cut, on, coef);
}

// the bonds: checks first, nothing is stored unless every one passes; then the CSR of bond ends by body (include/rbl.h section 4)
int rbl_set_bonds(rbl_ctx *c, int n_bonds, const int *body, const double *anchor, const int *kind, const double *param, int n_sets, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!body && !anchor && !param && !on) { c->ia_bd_on = false; return RBL_OK; }
  if (!body) return rbl_fail(c, RBL_ERR_ARG, "set_bonds: body must not be NULL");
  if (!anchor) return rbl_fail(c, RBL_ERR_ARG, "set_bonds: anchor must not be NULL");
  if (!param) return rbl_fail(c, RBL_ERR_ARG, "set_bonds: param must not be NULL");
  if (n_bonds < 1 || n_bonds > (1 << 24)) return rbl_fail(c, RBL_ERR_ARG, "set_bonds: n_bonds must lie in [1, 2^24]");
  if (n_sets < 1) return rbl_fail(c, RBL_ERR_ARG, "set_bonds: n_sets must be >= 1");
  if ((size_t)n_sets * (size_t)n_bonds > ((size_t)1 << 30)) return rbl_fail(c, RBL_ERR_ARG, "set_bonds: n_sets * n_bonds must not exceed 2^30");
  int top = -1;
  for (int b = 0; b < n_bonds; ++b) {
    const int i = body[2 * (size_t)b], j = body[2 * (size_t)b + 1];
    const std::string at = "set_bonds: bond " + std::to_string(b) + ": ";
    if (i < 0) return rbl_fail(c, RBL_ERR_ARG, at + "body[2 b], the first body index, must be >= 0");
    if (j < -1) return rbl_fail(c, RBL_ERR_ARG, at + "body[2 b + 1], the second body index, must be >= 0 or -1 (a lab point)");
    if (i == j) return rbl_fail(c, RBL_ERR_ARG, at + "body: both ends lie on one body (a bond inside a rigid body does nothing)");
    if (kind && kind[b] != 0 && kind[b] != 1) return rbl_fail(c, RBL_ERR_ARG, at + "kind must be 0 (harmonic) or 1 (tabulated)");
    for (int q = 0; q < 6; ++q)
      if (!std::isfinite(anchor[6 * (size_t)b + q])) return rbl_fail(c, RBL_ERR_ARG, at + "every value of anchor must be finite");
    top = std::max(top, std::max(i, j));
  }
  for (int s = 0; s < n_sets; ++s)
    for (int b = 0; b < n_bonds; ++b) {
      const double k = param[2 * ((size_t)s * n_bonds + b)], l0 = param[2 * ((size_t)s * n_bonds + b) + 1];
      const std::string at = "set_bonds: bond " + std::to_string(b) + ", set " + std::to_string(s) + ": ";
      if (!std::isfinite(k) || !std::isfinite(l0)) return rbl_fail(c, RBL_ERR_ARG, at + "every value of param (k, l0) must be finite");
      if (k < 0.0) return rbl_fail(c, RBL_ERR_ARG, at + "param: k must be >= 0");
      if (l0 < 0.0) return rbl_fail(c, RBL_ERR_ARG, at + "param: l0 must be >= 0");
    }
  c->ia_bd_n = n_bonds; c->ia_bd_sets = n_sets; c->ia_bd_top = top;
  c->ia_bd_body.assign(body, body + 2 * (size_t)n_bonds);
  c->ia_bd_anchor.assign(anchor, anchor + 6 * (size_t)n_bonds);
  if (kind) c->ia_bd_kind.assign(kind, kind + n_bonds);
  else c->ia_bd_kind.assign((size_t)n_bonds, 0);
  const auto tab = std::find(c->ia_bd_kind.begin(), c->ia_bd_kind.end(), 1);
  c->ia_bd_tab = tab == c->ia_bd_kind.end() ? -1 : (int)(tab - c->ia_bd_kind.begin());
  c->ia_bd_param.assign(param, param + 2 * (size_t)n_sets * n_bonds);
  // bond ends by body, in increasing bond index: the ends in bond order, sorted by body with a stable sort (a body index may
  // be anything up to INT_MAX here, so nothing is sized by it)
  struct End { int body, partner, bond, end; };
  std::vector<End> ends;
  ends.reserve(2 * (size_t)n_bonds);
  for (int b = 0; b < n_bonds; ++b)
    for (int q = 0; q < 2; ++q)
      if (body[2 * (size_t)b + q] >= 0) ends.push_back({body[2 * (size_t)b + q], body[2 * (size_t)b + 1 - q], b, q});
  std::stable_sort(ends.begin(), ends.end(), [](const End &x, const End &y) { return x.body < y.body; });
  c->ia_bd_rows.clear(); c->ia_bd_ptr.clear();
  c->ia_bd_ends.resize(3 * ends.size());
  for (size_t q = 0; q < ends.size(); ++q) {
    if (!q || ends[q].body != ends[q - 1].body) {
      c->ia_bd_rows.push_back(ends[q].body);
      c->ia_bd_ptr.push_back((int)q);
    }
    c->ia_bd_ends[3 * q] = ends[q].partner; c->ia_bd_ends[3 * q + 1] = ends[q].bond; c->ia_bd_ends[3 * q + 2] = ends[q].end;
  }
  c->ia_bd_ptr.push_back((int)ends.size());
  c->ia_bd_on = on != 0;
  c->ia_bd_valid = false;
  return RBL_OK;
}

int rbl_get_bonds(const rbl_ctx *c, int *n_bonds, int *n_sets, int *on, int *body, double *anchor, int *kind, double *param)
{
  if (!c) return RBL_ERR_ARG;
  if (n_bonds) *n_bonds = c->ia_bd_n;
  if (n_sets) *n_sets = c->ia_bd_sets;
  if (on) *on = c->ia_bd_on ? 1 : 0;
  if (body && c->ia_bd_n) std::memcpy(body, c->ia_bd_body.data(), sizeof(int) * c->ia_bd_body.size());
  if (anchor && c->ia_bd_n) std::memcpy(anchor, c->ia_bd_anchor.data(), sizeof(double) * c->ia_bd_anchor.size());
  if (kind && c->ia_bd_n) std::memcpy(kind, c->ia_bd_kind.data(), sizeof(int) * c->ia_bd_kind.size());
  if (param && c->ia_bd_n) std::memcpy(param, c->ia_bd_param.data(), sizeof(double) * c->ia_bd_param.size());
  return RBL_OK;
}

// length | tension | energy of the stored bonds (on or off) over n_win windows of win bodies into host arrays (any may be NULL)
static int ia_bond_state(rbl_ctx *c, const char *who, const double *d_X, const double *d_Q, int win, int n_win, double *length,
                         double *tension, double *energy)
{
  if (c->ia_bd_n < 1) return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": no bonds have been set (rbl_set_bonds)");
  int rc = ia_bond_check(c, who, win, n_win); if (rc) return rc;
  if ((rc = ia_upload(c))) return rc;
  if ((rc = ia_bond_upload(c))) return rc;
  const size_t tot = (size_t)n_win * c->ia_bd_n;
  if ((rc = rbl_dev_reserve(c, c->d_iabs, sizeof(double) * 3 * tot))) return rc;
  double *out = (double *)c->d_iabs.p;
  hipLaunchKernelGGL(k_bond_state, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, d_X, d_Q, win, n_win,
                     ia_bond_args(c, n_win), out);
  double *host[3] = {length, tension, energy};
  for (int q = 0; q < 3; ++q)
    if (host[q] && (rc = copy_d2h(c, host[q], out + q * tot, sizeof(double) * tot))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

int rbl_bond_state(rbl_ctx *c, double *length, double *tension, double *energy)
{
  int rc = need_config(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if ((rc = sync_bodies(c))) return rc;
  const double *dX = (const double *)c->d_XQ.p;
  return ia_bond_state(c, "bond_state", dX, dX + 3 * (size_t)c->S.N_bod, c->S.N_bod, 1, length, tension, energy);
}

int rbl_ensemble_bond_state(rbl_ctx *c, double *length, double *tension, double *energy)
{
  if (!c) return RBL_ERR_ARG;
  const double *dX = nullptr, *dQ = nullptr;
  int rc = rbl_ensemble_config_dev(c, &dX, &dQ); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  return ia_bond_state(c, "ensemble_bond_state", dX, dQ, c->ens_Nb, c->ens_R, length, tension, energy);
}

int rbl_set_magnetic_field(rbl_ctx *c, const double B0[3], const double B1[3], const double B2[3], double omega, int on)
{
  if (!c) return RBL_ERR_ARG;
  if (!B0 && !B1 && !B2 && !on) { c->ia_mf_on = false; return RBL_OK; }
  if (!B0 || !B1 || !B2) return rbl_fail(c, RBL_ERR_ARG, "set_magnetic_field: B0, B1 and B2 must not be NULL");
  const double *B[3] = {B0, B1, B2};
  static const char *const name[3] = {"B0", "B1", "B2"};
  for (int k = 0; k < 3; ++k)
    for (int q = 0; q < 3; ++q)
      if (!std::isfinite(B[k][q])) return rbl_fail(c, RBL_ERR_ARG, std::string("set_magnetic_field: every value of ") + name[k] + " must be finite");
  if (!std::isfinite(omega)) return rbl_fail(c, RBL_ERR_ARG, "set_magnetic_field: omega must be finite");
  for (int k = 0; k < 3; ++k) std::memcpy(c->ia_mf_B + 3 * k, B[k], 3 * sizeof(double));
  c->ia_mf_omega = omega;
  c->ia_mf_on = on != 0;
  return RBL_OK;
}

int rbl_get_magnetic_field(const rbl_ctx *c, double *B9, double *omega, int *on)
{
  if (!c) return RBL_ERR_ARG;
  if (B9) std::memcpy(B9, c->ia_mf_B, sizeof(c->ia_mf_B));
  if (omega) *omega = c->ia_mf_omega;
  if (on) *on = c->ia_mf_on ? 1 : 0;
  return RBL_OK;
}

int rbl_set_field_time(rbl_ctx *c, const double *t, int n)
{
  if (!c) return RBL_ERR_ARG;
  if (!t) return rbl_fail(c, RBL_ERR_ARG, "set_field_time: t must not be NULL");
  if (n < 1) return rbl_fail(c, RBL_ERR_ARG, "set_field_time: n must be >= 1");
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(t[i])) return rbl_fail(c, RBL_ERR_ARG, "set_field_time: every value of t must be finite");
  c->ia_ft.assign(t, t + n);
  c->ia_ft_valid = false;
  return RBL_OK;
}

int rbl_get_field_time(const rbl_ctx *c, int *n, double *t)
{
  if (!c) return RBL_ERR_ARG;
  if (n) *n = (int)c->ia_ft.size();
  if (t) std::memcpy(t, c->ia_ft.data(), sizeof(double) * c->ia_ft.size());
  return RBL_OK;
}

int rbl_interactions_active(const rbl_ctx *c, int *mask)
{
  if (!c || !mask) return RBL_ERR_ARG;
  *mask = (c->ia_on ? 1 : 0) | (c->ia_pt.on ? 2 : 0) | (c->ia_ht.on ? 4 : 0) | (c->ia_tr_on ? 8 : 0) |
          (ia_dp_pairs(c) ? 16 : 0) | (ia_dp_field(c) ? 32 : 0) | (ia_bonds(c) ? 64 : 0) | (ia_typed(c) ? 128 : 0);
  return RBL_OK;
}

int rbl_interaction_forces_dev(rbl_ctx *c, double *d_f_blob, double *d_FT_body, double *energy)
{
  int rc = need_config(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!ia_any(c)) return rbl_fail(c, RBL_ERR_STATE, "interaction_forces: no force model is switched on (rbl_set_interactions)");
  if (!energy) return ia_eval(c, d_f_blob, d_FT_body, nullptr);
  IaLayout L;
  if ((rc = ia_reserve(c, L))) return rc;
  if ((rc = ia_eval(c, d_f_blob, d_FT_body, L.e))) return rc;
  const size_t N = (size_t)c->S.N_bod * c->S.N_blb;
  std::vector<double> e(N);
  if ((rc = copy_d2h(c, e.data(), L.e, sizeof(double) * N))) return rc;
  if ((rc = finish_and_check(c))) return rc;
  double E = 0.0;                                        // one order: blob index
  for (double x : e) E += x;
  *energy = E;
  return RBL_OK;
}

int rbl_interaction_forces(rbl_ctx *c, double *f_blob, double *FT_body, double *energy)
{
  int rc = need_config(c); if (rc) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  if (!ia_any(c)) return rbl_fail(c, RBL_ERR_STATE, "interaction_forces: no force model is switched on (rbl_set_interactions)");
  const size_t N = (size_t)c->S.N_bod * c->S.N_blb, nb6 = (size_t)6 * c->S.N_bod;
  IaLayout L;
  if ((rc = ia_reserve(c, L))) return rc;
  if ((rc = rbl_interaction_forces_dev(c, nullptr, L.ft, energy))) return rc;
  if (f_blob && (rc = copy_d2h(c, f_blob, L.f, sizeof(double) * 3 * N))) return rc;
  if (FT_body && (rc = copy_d2h(c, FT_body, L.ft, sizeof(double) * nb6))) return rc;
  return finish_and_check(c);
}

int rbl_interaction_stats(rbl_ctx *c, int64_t *body_pairs, int64_t *blob_pairs)
{
  if (!c) return RBL_ERR_ARG;
  if (!c->ia_nb) return rbl_fail(c, RBL_ERR_STATE, "interaction_stats: nothing has been evaluated yet");
  const size_t N = (size_t)c->ia_nb * c->ia_nblb;
  std::vector<int> cnt((size_t)c->ia_nb), np(N);
  const IaLayout L = ia_layout(c->d_ia.p, c->ia_nb, c->ia_nblb, c->ia_cap);
  int rc = copy_d2h(c, cnt.data(), L.cnt, sizeof(int) * cnt.size()); if (rc) return rc;
  if ((rc = copy_d2h(c, np.data(), L.np, sizeof(int) * N))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  int64_t bp = 0, pp = 0;
  for (int x : cnt) bp += std::min(x, c->ia_cap);
  for (int x : np) pp += x;
  if (body_pairs) *body_pairs = bp;
  if (blob_pairs) *blob_pairs = pp;
  return RBL_OK;
}
