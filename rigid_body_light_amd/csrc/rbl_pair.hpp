// rbl_pair.hpp -- device pair arithmetic for the blob mobility (gfx950, fp64).
//
// Two formulations of the same physics:
//
//  * rbl_block_ref():   the 3x3 block exactly as the reference assembles it
//    (c_rigid_obj.cpp:31-142 and :432-447): same expressions, IEEE division and
//    sqrt, FMA contraction OFF -> entries come out bit-identical to the CPU
//    oracle.  Used by the dense-build kernel, which is HBM-write bound, so the
//    extra ALU work is free.
//
//  * rbl_pair_accum() / rbl_pair_symv() / rbl_pair_block_fast():  the fast form used by the matvec
//    kernels, which are fp64-VALU bound: ONE v_rsq_f64 + a 3rd-order Newton step per distance, no
//    division, h_hat eliminated algebraically ( h_hat ez = z_j/R, (1-h_hat) ez = z_i/R ), the wall
//    "facts" as Horner polynomials (rbl_wall_coeffs) and the block applied in vector form
//        M F = cF F + dl [beta (dl.F) + gxz Fz] + z^ [gzx (dl.F) + (mzz - cF) Fz],   dl = (dx, dy, 0).
//    Agrees with the reference to ~1e-15 relative per pair (tests pin <=1e-12 on apply_M).
#pragma once
#include <hip/hip_runtime.h>

#define RBL_FLAG_OVERLAP 1
#define RBL_FLAG_BELOW_WALL 2
#define RBL_FLAG_NONFINITE 4
#define RBL_FLAG_NOT_SPD 8
#define RBL_FLAG_INTERNAL 16   // a bounded wait between workgroups ran out (rbl_tilechol.hip): never expected, never a hang
#define RBL_FLAG_CAPACITY 32   // an interaction neighbour list overflowed its cap (rbl_forces.hip): reported, never truncated silently
#define RBL_FLAG_REDUNDANT 64  // a pivot of the joints' Schur complement was lost inside the one-kernel jointed solve (rbl_small_solve.hpp): a redundant joint set

struct RblParams {
  double a;        // blob radius
  double inv_a;    // 1/a
  double nf;       // 1/(8 pi eta a)            c_rigid_obj.cpp:415
  double four_a2;  // (2a)^2, far/overlap switch c_rigid_obj.cpp:62
  double tiny2;    // (1e-12 a)^2, overlap abort c_rigid_obj.cpp:53
  double c_near_A; // -(3/8)/a   : 4/3 (1 - 9/32 r/a) = 4/3 + c_near_A r
  double c_near_B; // (1/8)/a    : 4/3 * 3/32 (a/r) / a^2 = c_near_B / r
  int no_damp;     // 1: the matvec kernels skip the damping B (plain wall-corrected M), used by the preconditioned square root
};

// ---------------------------------------------------------------------------
// 1/sqrt(x), full double precision: v_rsq_f64 seed (measured max rel. error 5.2e-8 on
// gfx950, tools/peak_fp64) + one 3rd-order correction -> error ~ e^3 ~ 1e-22 + rounding.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double rbl_rsqrt(double x)
{
  double y = __builtin_amdgcn_rsq(x);
  double h = x * y;
  double e = __builtin_fma(-h, y, 1.0);            // 1 - x y^2
  double p = __builtin_fma(e, 0.375, 0.5);         // 1/2 + 3/8 e
  double ye = y * e;
  y = __builtin_fma(ye, p, y);                     // y (1 + e/2 + 3 e^2/8)
  return y;
}

// ---------------------------------------------------------------------------
// Wall-corrected block of one pair (i <- j, h = z_j) as five scalars:
//     M_ij = cF I + beta dl dl^T + gxz dl z^T + gzx z dl^T + (mzz - cF) z z^T,    dl = (dx, dy, 0)
// (A, Bc: the free-space RPY coefficients; q = dx^2 + dy^2).  With e = (dx, dy, Rz)/R, Rz = z_i + z_j,
// w = a/R, u = w^2, v = e_z^2, g = z_j/R (= h_hat e_z), k = z_i/R (= (1 - h_hat) e_z) every "fact" of the
// reference (c_rigid_obj.cpp:108-130) is  w x (polynomial in u), evaluated in Horner form:
//   fact1 = w b1,  b1 = -1 - 2gk + u[(2v - 2/3) + u(2/3 - 10/3 v)]
//   fact2 = w b2,  b2 = -1 + 6gk + u[(2 - 10v) + u(70/3 v - 10/3)]
//   fact5 = w b5,  b5 = -4g^2 + u[-4v + u(20v - 8/3)]
//   fact2 ez + fact3 = w (T0 - T1),  fact2 ez + fact4 = w (T0 + T1)     with
//   T0 = 2g - ez,  T1 = ez { 6gk + u[(2 - 10v) + u(70/3 v - 10)] }
// Swapping the roles of i and j swaps g <-> k, i.e. T1 -> -T1 only: M_ji = M_ij^T exactly.
// ---------------------------------------------------------------------------
// UNIT: the length unit of the coordinates the caller hands in.
//   RBL_UNIT_PHYS   (0, = false)  physical lengths; the pair multiplies by a/R and a/r itself
//   RBL_UNIT_RADIUS (1, = true)   coordinates already divided by the blob radius (a = 1): those multiplications are gone.  The
//                                 one-workgroup kernels of small systems (rbl_small_dev.hpp) and the host checks of tests/host_pair
//   RBL_UNIT_SHARED (2)           coordinates divided by a / lambda, lambda^2 = RBL_UNIT_L2 = 3, and every coefficient DIVIDED by
//                                 lambda: the block the five scalars describe, applied to lambda-scaled displacements, is M / lambda
//                                 (the epilogues multiply by lambda nf instead of nf: rbl_unit_out_scale).  Every coefficient is
//                                 w = a/R or s = a/r times a polynomial in w^2, s^2 and ratios of lengths, so the unit only changes
//                                 the polynomials' constants -- with w' = w / lambda, u' = u / 3:
//     b1  = -1 - 2gk + u'[(6v - 2)   + u'(6 - 30v)]
//     b2p =      6gk + u'[(6 - 30v)  + u'(210v - 30)]            Q = 6 - 30v serves both: one instruction less per pair
//     and, u' being 1 / R'^2 itself, gk = z_i z_j / R^2 = z_i' z_j' u' joins the brackets (no (r/R)^2, no separate constant parts):
//     b1  = -1 + u'[(6v - 2 - 2 z_i' z_j') + u' Q],    b2p = u'[(Q + 6 z_i' z_j') + u'(210v - 30)]      a second instruction less:
//     -2 z_i' and 6 z_i' are the row's, formed outside the sweep's loop
//     T1p = b2p - 60 u'^2,   zz bracket  u'^2 (180v - 24) - v (b2p + 12u'),   A' = s' + 2 s'^3,   Bc' = (s' - 6 s'^3) / r'^2
//                                 (the brackets coincide because 3 (2 - 10v) = 9 (2/3 - 10/3 v): lambda^2 = 3 and nothing else)
//     and, w' u' being w'^3, the brackets X = (6v - 2 - 2 z_i' z_j') + u' Q and Y = (Q + 6 z_i' z_j') + u'(210v - 30) are used as they
//     stand (b1 = -1 + u' X, b2p = u' Y are never formed): their factor u' rides on the odd powers w'^3, w'^5 = w'^3 u' that the five
//     scalars are multiplied by anyway --
//     cF = (A - w') + w'^3 X,  beta = Bw + w'^5 Y,  gxz, gzx = gm -+ (Y - 60u') Rz w'^5,  mzz = cF + gm dz + w'^3 [u'(180v - 24) - v (Y + 12)]
//     u'^2 and u' Y go, w'^5 comes: a third instruction less (70 fp64 per unordered pair, 62 per ordered one; profiles/wall_brackets.md)
// A gfx9 VOP3 instruction reads at most one SGPR/constant, so of a bracket's two non-inline constants the compiler re-materialises the
// second one into a VGPR with a v_mov_b64 on EVERY evaluation.  A caller with registers to spare passes them in as
// opaque register-resident values (RblWallK from rbl_wall_k_resident()) and saves those issue slots (-30 serves Q and, as the addend,
// the 210v - 30 bracket).
#define RBL_UNIT_PHYS 0
#define RBL_UNIT_RADIUS 1
#define RBL_UNIT_SHARED 2
#define RBL_UNIT_L2 3.0                       // lambda^2: the ONE place the shared unit is chosen (the polynomials above assert it)
#define RBL_UNIT_L 1.7320508075688772         // lambda = sqrt(3)
#define RBL_UNIT_INV_L 0.57735026918962576    // 1 / lambda

constexpr double rbl_unit_l2(int unit) { return unit == RBL_UNIT_SHARED ? RBL_UNIT_L2 : 1.0; }
constexpr double rbl_unit_inv_l(int unit) { return unit == RBL_UNIT_SHARED ? RBL_UNIT_INV_L : 1.0; }

constexpr double rbl_unit_l(int unit) { return unit == RBL_UNIT_SHARED ? RBL_UNIT_L : 1.0; }
// The wall polynomials are what the shared unit pays for; in free space it saves nothing and its -6 (for the -2 of Bc, an inline
// constant) costs the wave-unit kernels a copy per pair and three instances a few bytes of scratch: free-space kernels keep the radius.
constexpr int rbl_unit_of(bool wall) { return wall ? RBL_UNIT_SHARED : RBL_UNIT_RADIUS; }

// the kernels' side of a unit (UNIT = RBL_UNIT_RADIUS or RBL_UNIT_SHARED): positions times rbl_unit_pos_scale when loaded, sums times
// rbl_unit_out_scale when they leave, the pair routines called with rbl_unit_params (the parameter set of a blob of radius 1 or
// lambda: switch distances and near-branch constants)
template <int UNIT>
__host__ __device__ __forceinline__ double rbl_unit_pos_scale(const RblParams &P) { return UNIT == RBL_UNIT_SHARED ? P.inv_a * RBL_UNIT_L : P.inv_a; }
template <int UNIT>
__host__ __device__ __forceinline__ double rbl_unit_out_scale(const RblParams &P) { return UNIT == RBL_UNIT_SHARED ? P.nf * RBL_UNIT_L : P.nf; }
template <int UNIT>
__host__ __device__ __forceinline__ RblParams rbl_unit_params(const RblParams &P)
{
  constexpr double L2 = rbl_unit_l2(UNIT);
  RblParams Pu = P;
  Pu.a = rbl_unit_l(UNIT); Pu.inv_a = rbl_unit_inv_l(UNIT);   // the blob radius in the unit
  Pu.four_a2 = 4.0 * L2; Pu.tiny2 = 1e-24 * L2;
  Pu.c_near_A = -0.375 / L2; Pu.c_near_B = 0.125 / L2;       // shared: (4/3 - 3/8 r) / lambda = 4/(3 lambda) - r'/8,  1/(8 lambda^2 r') = (1/24) / r'
  return Pu;
}

// The shared unit's constants are small integers, and gfx950 encodes such a double (low word zero) as the 32-bit literal of a VOP2
// v_fmac_f64 -- whose addend is its destination.  Where the addend lives on (fma(v, 210, -30): the resident -30;  fma(u', -60, Y): Y)
// the compiler takes that form anyway and copies the addend first, a v_mov_b64 per pair each.  So these multipliers are
// opaque as well, in SCALAR register pairs (a VOP3 v_fma_f64 reads one): 210 (k2), -60 (s1) and the 6 of Q and of 6v - 2 (s2, which the
// compiler otherwise keeps in a vector pair).  -30 and 180 stay in vector pairs: they share an instruction with 210 and -24.
// The 12 of Y + 12 (k4) is a scalar pair too: v_add_f64 exists as VOP3 only and takes no literal at all.
// (All of them in vector registers: the same instructions, and k_apply_M_symw<true,2,4,1> spills 12 bytes at its 168 VGPRs.)
struct RblWallK {
  double k1, k2, k3, k4;   // physical / radius units: -10/3, 70/3, 20, 3/2;  shared unit: -30, 210, 180, 12
  double s1, s2;           // shared unit: -60, 6
};
template <int UNIT = RBL_UNIT_PHYS>
__device__ __forceinline__ RblWallK rbl_wall_k_literal()
{
  if constexpr (UNIT == RBL_UNIT_SHARED) return RblWallK{-30.0, 210.0, 180.0, 12.0, -60.0, 6.0};
  else return RblWallK{-10.0 / 3.0, 70.0 / 3.0, 20.0, 1.5, 0.0, 0.0};
}
template <int UNIT>
__device__ __forceinline__ RblWallK rbl_wall_k_resident()
{
  RblWallK K = rbl_wall_k_literal<UNIT>();
  // opaque to the optimiser: the values stay in the registers they are given
  if constexpr (UNIT == RBL_UNIT_SHARED) asm volatile("" : "+v"(K.k1), "+v"(K.k3), "+s"(K.k2), "+s"(K.k4), "+s"(K.s1), "+s"(K.s2));
  else asm volatile("" : "+v"(K.k1), "+v"(K.k2), "+v"(K.k3), "+v"(K.k4));
  return K;
}

template <int UNIT = RBL_UNIT_PHYS>
__device__ __forceinline__ void rbl_wall_coeffs(const RblParams &P, double dz, double zi, double zj, double q,
                                                double r2, double A, double Bc, double &cF, double &beta, double &gxz,
                                                double &gzx, double &mzz, const RblWallK &K = rbl_wall_k_literal<UNIT>())
{
  // Further identities that take instructions out (84 -> 75 fp64 instructions per unordered pair when they came in; 70 today, see the
  // header comment):
  //   T0 = 2g - ez = (z_j - z_i)/R = -dz/R             (g never formed)
  //   gk = z_i z_j / R^2 = (1 - r^2/R^2) / 4           (R^2 - r^2 = 4 z_i z_j)
  //   v = ez^2 = 1 - q/R^2                             (ez itself is only needed as Rz/R inside Rz w/R^2)
  //   gk and v only enter O(1) polynomials, so the cancellation when z_i z_j << R^2 or Rz^2 << R^2 costs an
  //   absolute ~1e-16 there, nothing relative to the block
  //   2 ez T0 - 4 g^2 = -T0^2 - v                      (the zz bracket: -T0^2 - v (b2 + 1) + u d1), and its -w T0^2 =
  //   -dz^2 w/R^2 cancels the same term of Bc dz^2 = (Bc - w/R^2) dz^2 + dz^2 w/R^2:  mzz = cF + gm dz + w (u d1 - v b2p)
  //   T1 = ez (b2 + 1 - 20/3 u^2),  b2 + 1 = 6 gk + u t2 =: b2p
  //   fact2 ez -+ T1 enter as  gm -+ T1' (Rz w / R^2):  two FMAs on the shared product, no separate add/sub
  //   Bc dz + T0 w / R = dz (Bc - w / R^2) = gm,  and  Bc + b2 w / R^2 = (Bc - w/R^2) + b2p w / R^2
  const double Rz = zi + zj;
  const double R2 = __builtin_fma(Rz, Rz, q);
  const double invR = rbl_rsqrt(R2);
  const double w = UNIT ? invR : P.a * invR;
  const double iR2 = invR * invR;
  const double u = w * w;
  const double v = __builtin_fma(-q, iR2, 1.0);
  if constexpr (UNIT == RBL_UNIT_SHARED) {
    constexpr double L2 = rbl_unit_l2(UNIT);
    static_assert(L2 * 2.0 == L2 * L2 * 2.0 / 3.0 && L2 * -10.0 == L2 * L2 * -10.0 / 3.0, "Q is shared only where lambda^2 = 3");
    // gk = z_i z_j / R^2 = z_i z_j u here (u = 1 / R^2 in the unit), so the constant parts join the Horner brackets:
    //   b1 = -1 + u X,  X = (6v - 2 - 2 z_i z_j) + u Q;      b2p = u Y,  Y = (Q + 6 z_i z_j) + u (210v - 30)
    // -2 z_i and 6 z_i belong to the row: a sweep forms them once, outside its loop.
    // The brackets stay un-multiplied: every use of b1 and b2p goes on to a multiplication by w or w^3 = w u (u is 1 / R^2 here), so
    // the factor u moves into the odd powers w^3, w^5 = w^3 u, which all uses share:
    //   cF   = A + w b1         = (A - w) + w^3 X
    //   beta = Bw + w^3 b2p     = Bw + w^5 Y
    //   T1p  = b2p - 60 u^2     = u (Y - 60 u) =: u T1Y,      gxz, gzx = gm -+ T1p Rz w^3 = gm -+ T1Y Rz w^5
    //   mzz  = ... + w [u^2 (180v - 24) - v (b2p + 12 u)] = ... + w^3 [u (180v - 24) - v (Y + 12)]
    // u^2 and the product u Y are never formed, w^5 is: one instruction less per pair.  (12: an opaque scalar pair where the caller
    // keeps its constants resident -- v_add_f64 takes no literal.)
    const double Q = __builtin_fma(v, K.k1, K.s2);                                   // 6 - 30 v
    const double m = __builtin_fma(-2.0 * zi, zj, -2.0);
    const double X = __builtin_fma(u, Q, __builtin_fma(v, K.s2, m));
    const double Y = __builtin_fma(u, __builtin_fma(v, K.k2, K.k1), __builtin_fma(6.0 * zi, zj, Q));
    const double w3 = w * u, w5 = w3 * u;
    const double Bw = Bc - w3;
    cF = __builtin_fma(w3, X, A - w);
    beta = __builtin_fma(Y, w5, Bw);                                                 // lateral dyad: (Bc + fact2/R^2) dl dl^T
    const double T1Y = __builtin_fma(u, K.s1, Y);                                    // T1 / (ez u)
    const double gm = dz * Bw, gd5 = Rz * w5;
    gxz = __builtin_fma(-T1Y, gd5, gm);                                              // M_xz = dx gxz, M_yz = dy gxz
    gzx = __builtin_fma(T1Y, gd5, gm);                                               // M_zx = dx gzx, M_zy = dy gzx
    const double c = __builtin_fma(u, __builtin_fma(v, K.k3, -24.0), -(v * (Y + K.k4)));
    mzz = __builtin_fma(w3, c, __builtin_fma(gm, dz, cF));
  } else {
    // physical lengths and radii (w^3 = w / R^2 is not w u in physical lengths): the header comment's first form
    const double rr = r2 * iR2;                                                      // (r/R)^2 = 1 - 4 gk
    const double t1 = __builtin_fma(u, __builtin_fma(v, K.k1, 2.0 / 3.0), __builtin_fma(v, 2.0, -2.0 / 3.0));
    const double t2 = __builtin_fma(u, __builtin_fma(v, K.k2, -10.0 / 3.0), __builtin_fma(v, -10.0, 2.0));
    const double b1 = __builtin_fma(u, t1, __builtin_fma(0.5, rr, -K.k4));           // -1 - 2 gk + u t1
    const double b2p = __builtin_fma(u, t2, __builtin_fma(-rr, K.k4, K.k4));         // b2 + 1 = 6 gk + u t2
    const double uu = u * u;
    const double T1p = __builtin_fma(uu, -20.0 / 3.0, b2p);                          // T1 / ez
    const double w3 = w * iR2;                                                       // w / R^2
    const double Bw = Bc - w3;
    cF = __builtin_fma(w, b1, A);
    beta = __builtin_fma(b2p, w3, Bw);                                               // lateral dyad: (Bc + fact2/R^2) dl dl^T
    const double gm = dz * Bw, gdw = Rz * w3;
    gxz = __builtin_fma(-T1p, gdw, gm);                                              // M_xz = dx gxz, M_yz = dy gxz
    gzx = __builtin_fma(T1p, gdw, gm);                                               // M_zx = dx gzx, M_zy = dy gzx
    // zz bracket  u d1 - v b2p,  d1 = u (20 v - 8/3) - 4 v:   u^2 (20 v - 8/3) - v (b2p + 4 u)
    const double c = __builtin_fma(uu, __builtin_fma(v, K.k3, -8.0 / 3.0), -(v * __builtin_fma(4.0, u, b2p)));
    mzz = __builtin_fma(w, c, __builtin_fma(gm, dz, cF));
  }
}

// ---------------------------------------------------------------------------
// Fast matrix-free accumulation of one ordered pair (i <- j).
//   dx,dy,dz = r_i - r_j ;  zi, zj heights ; (Fx,Fy,Fz) = (damped) force on j
//   SELF: compile-time "this j-tile may contain i" (index-equality self term)
// Accumulates UNSCALED (units 1/(8 pi eta a)) into ux,uy,uz.
// ---------------------------------------------------------------------------
template <bool WALL, bool SELF, int UNIT = RBL_UNIT_PHYS>
__device__ __forceinline__ void rbl_pair_accum(const RblParams &P, double xi, double yi,
                                               double zi, double xj, double yj, double zj,
                                               double Fx, double Fy, double Fz, bool is_self,
                                               double &ux, double &uy, double &uz,
                                               unsigned &flags, const RblWallK &K = rbl_wall_k_literal<UNIT>())
{
  const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
  const double q = __builtin_fma(dy, dy, dx * dx);
  const double r2 = __builtin_fma(dz, dz, q);

  // ---- free-space RPY (c_rigid_obj.cpp:48-79) in physical units ----------
  const double invr = rbl_rsqrt(r2);
  const double invr2 = invr * invr;
  const double s = UNIT ? invr : P.a * invr;         // a/r
  const double t = s * s;                            // (a/r)^2
  // far:  A = (a/r)(1 + 2/3 (a/r)^2),  Bc = (a/r)(1 - 2 (a/r)^2)/r^2      (shared unit: s + 2 s^3, (s - 6 s^3)/r^2, all / lambda)
  constexpr double L2 = rbl_unit_l2(UNIT), iL = rbl_unit_inv_l(UNIT), four3 = (4.0 / 3.0) * iL;
  double A = __builtin_fma(s * t, 2.0 * L2 / 3.0, s);
  double Bc = (s * invr2) * __builtin_fma(-2.0 * L2, t, 1.0);
  if (__builtin_expect(__any(r2 < P.four_a2), 0)) {  // wave-uniform: the overlap branch (and i == j) is rare
    // overlap: A = 4/3 - 3/8 r/a,  Bc = (1/8) / (a r)
    const double rr = r2 * invr;                     // r
    const bool far = r2 >= P.four_a2;
    A = far ? A : __builtin_fma(rr, P.c_near_A, four3);
    Bc = far ? Bc : invr * P.c_near_B;
    if (r2 < P.tiny2 && !(SELF && is_self)) flags |= RBL_FLAG_OVERLAP;   // :53-58
  }
  if (SELF) {                                        // index equality, :40-46
    A = is_self ? four3 : A;
    Bc = is_self ? 0.0 : Bc;
  }
  const double q2 = __builtin_fma(dy, Fy, dx * Fx);

  if (!WALL) {
    const double tB = Bc * __builtin_fma(dz, Fz, q2);
    ux = __builtin_fma(A, Fx, __builtin_fma(tB, dx, ux));
    uy = __builtin_fma(A, Fy, __builtin_fma(tB, dy, uy));
    uz = __builtin_fma(A, Fz, __builtin_fma(tB, dz, uz));
    return;
  }

  // ---- single-wall correction (c_rigid_obj.cpp:98-140), ordered pair, h = z_j
  if (SELF && is_self) {
    // self wall term (:98-104): diag only, args (0,0,2h; h = z_i/a)
    const double iz = (UNIT == RBL_UNIT_SHARED ? RBL_UNIT_L : UNIT ? 1.0 : P.a) / zi;   // 1/h in radii (true division kept: rare path)
    const double iz3 = iz * iz * iz;
    const double iz5 = iz3 * iz * iz;
    const double dpar = -(9.0 * iz - 2.0 * iz3 + iz5) / 12.0 * iL;
    const double dper = -(9.0 * iz - 4.0 * iz3 + iz5) / 6.0 * iL;
    ux = __builtin_fma(A + dpar, Fx, ux);
    uy = __builtin_fma(A + dpar, Fy, uy);
    uz = __builtin_fma(A + dper, Fz, uz);
    return;
  }
  double cF, beta, gxz, gzx, mzz;
  rbl_wall_coeffs<UNIT>(P, dz, zi, zj, q, r2, A, Bc, cF, beta, gxz, gzx, mzz, K);
  const double lat = __builtin_fma(beta, q2, gxz * Fz);
  ux = __builtin_fma(cF, Fx, __builtin_fma(lat, dx, ux));
  uy = __builtin_fma(cF, Fy, __builtin_fma(lat, dy, uy));
  uz = __builtin_fma(mzz, Fz, __builtin_fma(gzx, q2, uz));
}

// ---------------------------------------------------------------------------
// Symmetric pair (i != j) for NV force vectors at once: evaluates the scalar coefficients ONCE and applies the
// block in both directions to every vector,
//     U_i[v] += M_ij F_j[v]      (accumulated into ui[v])
//     U_j[v] += M_ji F_i[v]      (accumulated into uj[v]; caller adds it to j)
// M_ji = M_ij^T holds exactly for the RPY part and, for the wall part, through the
// role swap g <-> k (h = z_i instead of z_j): fact1, fact2, the e_z-part of fact3
// and the h-free part of fact5 are shared.  70 fp64 instructions per unordered wall pair in the shared unit
// (the far sweep of k_apply_M_sym<true,4> and <true,2>, librbl.isa.json) vs 2 x 62 for two ordered evaluations (k_apply_M<true>).
// NV = 2: the coefficients (50 of the 70) are shared, only the 20-FMA application is repeated: 90 per pair.
// Used for the two Brownian increments of the stochastic step (lock-step Lanczos) and for 2-3 simultaneous vectors in general.
// ---------------------------------------------------------------------------
// NEARCHK = false: the caller has proved (tile bounding boxes) that no pair of this sweep is closer than 2a,
// the overlap branch and its per-pair compare are compiled out.
struct RblV3 {
  double x, y, z;
};

template <bool WALL, int UNIT = RBL_UNIT_PHYS, bool NEARCHK = true, int NV = 1>
__device__ __forceinline__ void rbl_pair_symv(const RblParams &P, double xi, double yi, double zi, const RblV3 (&Fi)[NV],
                                              double xj, double yj, double zj, const RblV3 (&Fj)[NV], RblV3 (&ui)[NV],
                                              RblV3 (&uj)[NV], unsigned &flags, const RblWallK &K = rbl_wall_k_literal<UNIT>())
{
  const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
  const double q = __builtin_fma(dy, dy, dx * dx);
  const double r2 = __builtin_fma(dz, dz, q);
  const double invr = rbl_rsqrt(r2);
  const double invr2 = invr * invr;
  const double s = UNIT ? invr : P.a * invr;
  const double s3 = (s * s) * s;
  constexpr double L2 = rbl_unit_l2(UNIT), four3 = (4.0 / 3.0) * rbl_unit_inv_l(UNIT);
  double A = __builtin_fma(s3, 2.0 * L2 / 3.0, s);         // (a/r)(1 + 2/3 (a/r)^2)            shared unit: s + 2 s^3
  double Bc = __builtin_fma(s3, -2.0 * L2, s) * invr2;     // (a/r)(1 - 2 (a/r)^2) / r^2                     (s - 6 s^3) / r^2
  if (NEARCHK && __builtin_expect(__any(r2 < P.four_a2), 0)) {   // wave-uniform: overlap branch is rare
    const double rr = r2 * invr;
    const double A_near = __builtin_fma(rr, P.c_near_A, four3);
    const double B_near = invr * P.c_near_B;
    const bool far = r2 >= P.four_a2;
    A = far ? A : A_near;
    Bc = far ? Bc : B_near;
    if (r2 < P.tiny2) flags |= RBL_FLAG_OVERLAP;
  }
  if (!WALL) {   // free space: the vector form A F + Bc (d.F) d is cheaper than forming the block
    auto app = [&](const RblV3 &F, RblV3 &u) {
      const double tB = Bc * __builtin_fma(dz, F.z, __builtin_fma(dy, F.y, dx * F.x));
      u.x = __builtin_fma(A, F.x, __builtin_fma(tB, dx, u.x));
      u.y = __builtin_fma(A, F.y, __builtin_fma(tB, dy, u.y));
      u.z = __builtin_fma(A, F.z, __builtin_fma(tB, dz, u.z));
    };
#pragma unroll
    for (int v = 0; v < NV; ++v) app(Fj[v], ui[v]);
#pragma unroll
    for (int v = 0; v < NV; ++v) app(Fi[v], uj[v]);
    return;
  }

  // Wall: coefficients for ONE direction (h = z_j); M_ji = M_ij^T exactly, so U_j += M_ij^T F_i reuses
  // them.  Vector form: 20 FMAs per vector for both directions instead of forming nine entries.
  double cF, beta, gxz, gzx, mzz;
  rbl_wall_coeffs<UNIT>(P, dz, zi, zj, q, r2, A, Bc, cF, beta, gxz, gzx, mzz, K);
  auto app = [&](const RblV3 &F, RblV3 &u, double g_lat, double g_z) {   // M F (g_lat = gxz, g_z = gzx) or M^T F (swapped)
    const double p = __builtin_fma(dy, F.y, dx * F.x);
    const double l = __builtin_fma(beta, p, g_lat * F.z);
    u.x = __builtin_fma(cF, F.x, __builtin_fma(l, dx, u.x));
    u.y = __builtin_fma(cF, F.y, __builtin_fma(l, dy, u.y));
    u.z = __builtin_fma(mzz, F.z, __builtin_fma(g_z, p, u.z));
  };
#pragma unroll
  for (int v = 0; v < NV; ++v) app(Fj[v], ui[v], gxz, gzx);      // U_i += M F_j
#pragma unroll
  for (int v = 0; v < NV; ++v) app(Fi[v], uj[v], gzx, gxz);      // U_j += M^T F_i
}

// ---------------------------------------------------------------------------
// Full 3x3 block of one ORDERED pair (i <- j, h = z_j) from the fast coefficient
// arithmetic, row-major m[9], unscaled.  Used by the multi-RHS kernel, where the
// block is the A-operand of fp64 MFMAs:  M = cF I + Bc d d^T + f2 e e^T + f3 e z^T
// + f4 z e^T + f5 z z^T.
// ---------------------------------------------------------------------------
template <bool WALL, bool SELF, int UNIT = RBL_UNIT_PHYS>
__device__ __forceinline__ void rbl_pair_block_fast(const RblParams &P, double xi, double yi,
                                                    double zi, double xj, double yj, double zj,
                                                    bool is_self, double *m, unsigned &flags,
                                                    const RblWallK &K = rbl_wall_k_literal<UNIT>())
{
  const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
  const double q = __builtin_fma(dy, dy, dx * dx);
  const double r2 = __builtin_fma(dz, dz, q);
  const double invr = rbl_rsqrt(r2);
  const double invr2 = invr * invr;
  const double s = UNIT ? invr : P.a * invr;
  const double t = s * s;
  constexpr double L2 = rbl_unit_l2(UNIT), iL = rbl_unit_inv_l(UNIT), four3 = (4.0 / 3.0) * iL;
  double A = __builtin_fma(s * t, 2.0 * L2 / 3.0, s);
  double Bc = (s * invr2) * __builtin_fma(-2.0 * L2, t, 1.0);
  if (__builtin_expect(__any(r2 < P.four_a2), 0)) {
    const double rr = r2 * invr;
    const bool far = r2 >= P.four_a2;
    A = far ? A : __builtin_fma(rr, P.c_near_A, four3);
    Bc = far ? Bc : invr * P.c_near_B;
    if (r2 < P.tiny2 && !(SELF && is_self)) flags |= RBL_FLAG_OVERLAP;
  }
  if (SELF) {
    A = is_self ? four3 : A;
    Bc = is_self ? 0.0 : Bc;
  }
  if (!WALL) {
    const double Bdx = Bc * dx, Bdy = Bc * dy, Bdz = Bc * dz;
    m[0] = __builtin_fma(Bdx, dx, A); m[1] = Bdx * dy; m[2] = Bdx * dz;
    m[3] = m[1]; m[4] = __builtin_fma(Bdy, dy, A); m[5] = Bdy * dz;
    m[6] = m[2]; m[7] = m[5]; m[8] = __builtin_fma(Bdz, dz, A);
    return;
  }
  if (SELF && is_self) {  // self wall term (:98-104): diagonal only
    const double iz = (UNIT == RBL_UNIT_SHARED ? RBL_UNIT_L : UNIT ? 1.0 : P.a) / zi;
    const double iz3 = iz * iz * iz;
    const double iz5 = iz3 * iz * iz;
    const double dpar = -(9.0 * iz - 2.0 * iz3 + iz5) / 12.0 * iL;
    const double dper = -(9.0 * iz - 4.0 * iz3 + iz5) / 6.0 * iL;
    m[0] = A + dpar; m[1] = 0.0; m[2] = 0.0;
    m[3] = 0.0; m[4] = A + dpar; m[5] = 0.0;
    m[6] = 0.0; m[7] = 0.0; m[8] = A + dper;
    return;
  }
  double cF, beta, gxz, gzx, mzz;
  rbl_wall_coeffs<UNIT>(P, dz, zi, zj, q, r2, A, Bc, cF, beta, gxz, gzx, mzz, K);
  const double bx = beta * dx, by = beta * dy;
  m[0] = __builtin_fma(bx, dx, cF); m[1] = bx * dy; m[2] = dx * gxz;
  m[3] = m[1]; m[4] = __builtin_fma(by, dy, cF); m[5] = dy * gxz;
  m[6] = dx * gzx; m[7] = dy * gzx; m[8] = mzz;
}

// ---------------------------------------------------------------------------
// Reference-order block (bit-compatible with the oracle).  b: row-major 3x3,
// NOT yet scaled by nf.  lo/hi are the (i<=j) roles of c_rigid_obj.cpp:430-447.
// ---------------------------------------------------------------------------
#pragma clang fp contract(off)
__device__ __forceinline__ void rbl_rpy_ref(double rx, double ry, double rz, bool self,
                                            double inv_a, double *o, unsigned &flags)
{
  const double four3 = 4.0 / 3.0;
  if (self) {
    o[0] = four3; o[1] = 0.0; o[2] = 0.0; o[3] = four3; o[4] = 0.0; o[5] = four3;
    return;
  }
  rx = rx * inv_a; ry = ry * inv_a; rz = rz * inv_a;
  const double r2 = rx * rx + ry * ry + rz * rz;
  const double r = __builtin_sqrt(r2);
  if (r < 1e-12) flags |= RBL_FLAG_OVERLAP;
  const double invr = 1.0 / r;
  const double invr2 = invr * invr;
  if (r >= 2.0) {
    const double c1 = 1.0 + 2.0 / (3.0 * r2);
    const double c2 = (1.0 - 2.0 * invr2) * invr2;
    o[0] = (c1 + c2 * rx * rx) * invr;
    o[1] = (c2 * rx * ry) * invr;
    o[2] = (c2 * rx * rz) * invr;
    o[3] = (c1 + c2 * ry * ry) * invr;
    o[4] = (c2 * ry * rz) * invr;
    o[5] = (c1 + c2 * rz * rz) * invr;
  } else {
    const double c1 = four3 * (1.0 - 0.28125 * r);
    const double c2 = four3 * 0.09375 * invr;
    o[0] = c1 + c2 * rx * rx;
    o[1] = c2 * rx * ry;
    o[2] = c2 * rx * rz;
    o[3] = c1 + c2 * ry * ry;
    o[4] = c2 * ry * rz;
    o[5] = c1 + c2 * rz * rz;
  }
}

__device__ __forceinline__ void rbl_wall_ref(double rx, double ry, double rz, double *M,
                                             bool self, double hj, unsigned &flags)
{
  if (hj < 0.0) { flags |= RBL_FLAG_BELOW_WALL; }
  if (self) {
    const double iz = 1.0 / hj;
    const double iz3 = iz * iz * iz;
    const double iz5 = iz3 * iz * iz;
    M[0] += -(9 * iz - 2 * iz3 + iz5) / 12.0;
    M[4] += -(9 * iz - 2 * iz3 + iz5) / 12.0;
    M[8] += -(9 * iz - 4 * iz3 + iz5) / 6.0;
    return;
  }
  const double hh = hj / rz;
  const double iR = 1.0 / __builtin_sqrt(rx * rx + ry * ry + rz * rz);
  const double ex = rx * iR, ey = ry * iR, ez = rz * iR;
  const double iR3 = iR * iR * iR;
  const double iR5 = iR3 * iR * iR;
  const double f1 = -(3 * (1 + 2 * hh * (1 - hh) * ez * ez) * iR +
                      2 * (1 - 3 * ez * ez) * iR3 - 2 * (1 - 5 * ez * ez) * iR5) / 3.0;
  const double f2 = -(3 * (1 - 6 * hh * (1 - hh) * ez * ez) * iR -
                      6 * (1 - 5 * ez * ez) * iR3 + 10 * (1 - 7 * ez * ez) * iR5) / 3.0;
  const double f3 = ez *
                    (3 * hh * (1 - 6 * (1 - hh) * ez * ez) * iR -
                     6 * (1 - 5 * ez * ez) * iR3 + 10 * (2 - 7 * ez * ez) * iR5) *
                    2.0 / 3.0;
  const double f4 = ez * (3 * hh * iR - 10 * iR5) * 2.0 / 3.0;
  const double f5 = -(3 * hh * hh * ez * ez * iR + 3 * ez * ez * iR3 +
                      (2 - 15 * ez * ez) * iR5) * 4.0 / 3.0;
  M[0] += f1 + f2 * ex * ex;
  M[1] += f2 * ex * ey;
  M[2] += f2 * ex * ez + f3 * ex;
  M[3] += f2 * ey * ex;
  M[4] += f1 + f2 * ey * ey;
  M[5] += f2 * ey * ez + f3 * ey;
  M[6] += f2 * ez * ex + f4 * ex;
  M[7] += f2 * ez * ey + f4 * ey;
  M[8] += f1 + f2 * ez * ez + f3 * ez + f4 * ez + f5;
}

// block for the ordered roles (lo <= hi):  r_lo - r_hi,  h = z_hi / a
__device__ __forceinline__ void rbl_block_ref(const RblParams &P, bool wall, double xl,
                                              double yl, double zl, double xh, double yh,
                                              double zh, bool self, double *b, unsigned &flags)
{
  const double rx = xl - xh, ry = yl - yh, rz = zl - zh;
  double s[6];
  rbl_rpy_ref(rx, ry, rz, self, P.inv_a, s, flags);
  b[0] = s[0]; b[1] = s[1]; b[2] = s[2];
  b[3] = s[1]; b[4] = s[3]; b[5] = s[4];
  b[6] = s[2]; b[7] = s[4]; b[8] = s[5];
  if (wall) rbl_wall_ref(rx / P.a, ry / P.a, (rz + 2 * zh) / P.a, b, self, zh / P.a, flags);
}
#pragma clang fp contract(fast)
