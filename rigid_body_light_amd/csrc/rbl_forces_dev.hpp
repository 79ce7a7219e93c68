// rbl_forces_dev.hpp -- the force model of include/rbl.h section 4 as its kernels take it: the by-value argument structs and the
// ONE copy of every energy expression (steric term, wall repulsion, tabulated potentials, bonds, minimum image), shared by the force
// kernels (rbl_forces.hip) and the Metropolis sampler (rbl_ens_mc.hip), so that what is sampled is the energy the forces derive from.
#pragma once
#include <hip/hip_runtime.h>

#include "rbl_body_dev.hpp"
#include "rbl_internal.hpp"

struct IaParams {
  double w, a, eps_w, inv_bw, eps_b, inv_bb, two_a, rc2;
  int wall;
};

// the periodic cell of include/rbl.h section 10 as the minimum-image kernels take it (by value): lengths and reciprocals, 0 on an
// open axis, whose reduction is then skipped (no 1 / 0)
struct IaCell {
  double Lx, Ly, iLx, iLy;
  int px, py;
};

// replica w's cell from the table of an ensemble with a cell per replica (rbl_ensemble_set_cells): every kernel that takes
// the table reads the record of its body's or tile's window first, a workgroup-uniform index into a table that is only read
__device__ __forceinline__ IaCell ia_cell_of(const RblEnsCellRec *__restrict__ cells, int w)
{
  const RblEnsCellRec &R = cells[w];
  return {R.Lx, R.Ly, R.iLx, R.iLy, R.Lx > 0.0 ? 1 : 0, R.Ly > 0.0 ? 1 : 0};
}

// minimum-image convention on a displacement: d - L rint(d / L) on every periodic axis
__device__ __forceinline__ void ia_min_image(const IaCell &C, double &dx, double &dy)
{
  if (C.px) dx = __builtin_fma(-C.Lx, rint(dx * C.iLx), dx);
  if (C.py) dy = __builtin_fma(-C.Ly, rint(dy * C.iLy), dy);
}

// a tabulated potential on the device: coef[k] = (c0, c1, c2, c3) of interval k, U = c0 + t (c1 + t (c2 + t c3)),
// dU/dx = (c1 + t (2 c2 + 3 c3 t)) / h with t = (x - lo) / h - k
struct IaTab {
  const double4 *coef;
  double lo, hi, inv_h, U0, dU0, hi2;                    // U0, dU0: value and slope at lo (the tangent below it); hi2: hi^2 rounded up
  int last;                                              // n - 2, the last interval
};

// (U, dU/dx) at x <= T.hi
__device__ __forceinline__ void ia_tab_eval(const IaTab &T, double x, double &U, double &dU)
{
  if (x >= T.lo) {
    const double sx = (x - T.lo) * T.inv_h;
    const int k = min((int)sx, T.last);
    const double t = sx - (double)k;
    const double4 c = T.coef[k];
    U = c.x + t * (c.y + t * (c.z + t * c.w));
    dU = (c.y + t * (2.0 * c.z + 3.0 * c.w * t)) * T.inv_h;
  } else {                                               // the tangent at lo continued downwards
    U = T.U0 + T.dU0 * (x - T.lo);
    dU = T.dU0;
  }
}

// the built-in steric term at distance r: energy of the pair and g = -U'(r) / r, the tangent at r = 2a continued inwards
__device__ __forceinline__ void ia_steric(const IaParams &p, double r, double &U, double &g)
{
  if (r >= p.two_a) {
    U = p.eps_b * (p.two_a / r) * exp(-(r - p.two_a) * p.inv_bb);
    g = U * (1.0 / r + p.inv_bb) / r;
  } else {                                               // the tangent at r = 2a continued inwards
    const double slope = p.eps_b * (1.0 / p.two_a + p.inv_bb);
    U = p.eps_b + slope * (p.two_a - r);
    g = r > 0.0 ? slope / r : 0.0;
  }
}

// the wall repulsion at height z: energy and force along +z, the tangent continued below h = a
__device__ __forceinline__ void ia_wall(const IaParams &p, double z, double &Uw, double &Fw)
{
  if (z >= p.a) { Uw = p.eps_w * exp(-(z - p.a) * p.inv_bw); Fw = Uw * p.inv_bw; }
  else { Fw = p.eps_w * p.inv_bw; Uw = p.eps_w + Fw * (p.a - z); }
}

// ---- blob types: one pair table per unordered type pair (include/rbl.h section 4) --------------------------------------------
constexpr int IA_TY_PAIRS = rbl_ctx::IA_TY_PAIRS;

// the typed term as the kernel takes it (by value).  desc: one IaTab per unordered type pair (hi = hi2 = -1: no table, nothing is
// inside it); type: rows of N_blb entries -- body i reads row 0 (per_row = 0: every body alike) or row i % win
struct IaTyped {
  const IaTab *desc;
  const int *type;
  double cmax2;                                          // the largest cutoff^2 of every pair term that is on (built-in, untyped, typed)
  int per_row;
};

// a descriptor in LDS, padded to 72 bytes: a lane's descriptor follows ITS type, so the 32 lanes of a ds_read_b64 group read
// up to 8 different descriptors.  At 64 bytes the descriptors 4 apart share their banks ((a / 4) % 64); at 18 dwords the first
// 32 all start on different even banks
struct IaTabLds {
  IaTab T;
  double pad;
};

__device__ __forceinline__ int ia_type_pair(int s, int t) { const int hi = max(s, t); return hi * (hi + 1) / 2 + min(s, t); }

// ---- bonds ---------------------------------------------------------------------------------------------------------------------
// the bond table on the device: the pair table's construction, continued along its tangent above hi as well as below lo
struct IaBondTab {
  IaTab T;
  double U1, dU1;                                        // value and slope at hi
};

// the bonds as the kernels take them (by value).  anchor: s_A | s_B (or the lab point P) per bond; param: (k, l0) per bond,
// set-major; ends: (partner or -1, bond, which end) per entry of the CSR
struct IaBonds {
  const double *anchor, *param;
  const int *kind, *body, *rows, *ptr, *ends;
  IaBondTab BT;
  int n, n_rows, per_set;                                // per_set: window w reads parameter set w (0: every window reads set 0)
};

// R(Q_b) s
__device__ __forceinline__ void ia_lab_anchor(const double *__restrict__ Q, const double *__restrict__ s, int b, double (&l)[3])
{
  double R[9];
  quat_rot(Q + 4 * (size_t)b, R);
#pragma unroll
  for (int c = 0; c < 3; ++c) l[c] = R[3 * c] * s[0] + R[3 * c + 1] * s[1] + R[3 * c + 2] * s[2];
}

// bond b of window w between the bodies ia and ib (global indices; ib < 0: the lab point): the lever arms of both ends,
// r = p_A - p_B, its length, the energy U(d) and the tension dU/dd.  ONE sequence of operations for both ends of a bond, for
// the state query and for the sampler (which hands it a replica's own X and Q, indices local to the replica)
__device__ __forceinline__ void ia_bond_eval(const IaBonds &B, const double *__restrict__ X, const double *__restrict__ Q, int b,
                                             int w, int ia, int ib, double (&lA)[3], double (&lB)[3], double (&r)[3], double &d,
                                             double &U, double &dU)
{
  const double *s = B.anchor + 6 * (size_t)b;
  ia_lab_anchor(Q, s, ia, lA);
  double pB[3];
  if (ib >= 0) {
    ia_lab_anchor(Q, s + 3, ib, lB);
#pragma unroll
    for (int c = 0; c < 3; ++c) pB[c] = X[3 * (size_t)ib + c] + lB[c];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { lB[c] = 0.0; pB[c] = s[3 + c]; }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = (X[3 * (size_t)ia + c] + lA[c]) - pB[c];
  d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  const double *q = B.param + 2 * ((size_t)(B.per_set ? w : 0) * B.n + b);
  const double k = q[0], l0 = q[1];
  if (B.kind[b] == 0) {
    const double x = d - l0;
    dU = k * x;
    U = 0.5 * k * x * x;
  } else {
    double Ut, dUt;
    if (d > B.BT.T.hi) {                                 // a bond never breaks: the tangent at hi continued upwards
      Ut = B.BT.U1 + B.BT.dU1 * (d - B.BT.T.hi);
      dUt = B.BT.dU1;
    } else {
      ia_tab_eval(B.BT.T, d, Ut, dUt);
    }
    U = k * Ut;
    dU = k * dUt;
  }
}

// ---- the model as the Metropolis kernel takes it (rbl_ens_mc.hip), built by ia_mc_model (rbl_forces.hip) after an evaluation of
// the same ensemble has made its checks and uploads: every term of bits 0, 1, 2, 3, 6 and 7 of rbl_interactions_active
struct IaMcModel {
  IaParams p;                                            // as the pair kernels take it (built-in terms off: w = 0, wall = 0, rc2 = -1)
  IaTab PT, HT;
  IaTyped Y;                                             // cmax2: the largest pair cutoff^2 that is on, typed or not (< 0: no pair term)
  IaBonds B;
  IaCell C;
  const RblEnsCellRec *cells;                            // per == 2
  const double *tr_k, *tr_X0;                            // traps: 3 per entry
  double cull2;                                          // (2 R_body + the largest cutoff)^2 with k_body_neighbours' slack
  int tab;                                               // bit 0 pair table, bit 1 height table
  int typed, bonds, cull;
  int per;                                               // 0 open, 1 the shared cell C, 2 a cell per replica
  int tr_per;                                            // trap entries (N_bod or R N_bod), 0: off
};
// after ia_eval_batch of the same ensemble on the same stream
#pragma GCC visibility push(hidden)
IaMcModel ia_mc_model(const rbl_ctx *c, int n_win);
#pragma GCC visibility pop
