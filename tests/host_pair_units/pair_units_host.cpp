// Host build of the device pair arithmetic (rbl_pair.hpp) in the SHARED length unit (a / lambda, lambda^2 = 3: what every product
// kernel runs) for tests/test_pair_units_cpu.py -- the stand-in <hip/hip_runtime.h> is the one of tests/host_pair.
//   g++ -O2 -ffp-contract=fast -mfma -std=c++17 -shared -fPIC -Itests/host_pair -o libpair_units.so tests/host_pair_units/pair_units_host.cpp
// -DPAIR_UNITS_HEADER='"..."' -DPAIR_UNITS_RADIUS builds the same entry points over another copy of the header in radius units (the
// form before the shared unit: how the figure the test compares with was measured).
#ifndef PAIR_UNITS_HEADER
#define PAIR_UNITS_HEADER "../../rigid_body_light_amd/csrc/rbl_pair.hpp"
#endif
#include PAIR_UNITS_HEADER

namespace {
#ifdef PAIR_UNITS_RADIUS
constexpr auto U = true;
struct Frame {
  RblParams P;
  double in, out;
  explicit Frame(double a) : in(1.0 / a), out(1.0)
  {
    P.a = 1.0; P.inv_a = 1.0; P.nf = 1.0; P.four_a2 = 4.0; P.tiny2 = 1e-24; P.c_near_A = -0.375; P.c_near_B = 0.125; P.no_damp = 0;
  }
};
#else
constexpr int U = RBL_UNIT_SHARED;
// what a kernel does: positions times rbl_unit_pos_scale, the pair routines with rbl_unit_params, sums times rbl_unit_out_scale (nf = 1)
struct Frame {
  RblParams P;
  double in, out;
  explicit Frame(double a)
  {
    RblParams Q;
    Q.a = a; Q.inv_a = 1.0 / a; Q.nf = 1.0; Q.four_a2 = 4.0 * a * a; Q.tiny2 = (1e-12 * a) * (1e-12 * a);
    Q.c_near_A = -0.375 / a; Q.c_near_B = 0.125 / a; Q.no_damp = 0;
    in = rbl_unit_pos_scale<U>(Q); out = rbl_unit_out_scale<U>(Q);
    P = rbl_unit_params<U>(Q);
  }
};
#endif
}   // namespace

extern "C" {
// the nine entries of the ordered block (i <- j, h = z_j) formed from the five scalars (rbl_pair_block_fast), row-major, in units of
// 1 / (8 pi eta a); returns the flags
unsigned units_block(const double *ri, const double *rj, int i, int j, double a, int wall, double *out9)
{
  const Frame f(a);
  const double xi = ri[0] * f.in, yi = ri[1] * f.in, zi = ri[2] * f.in, xj = rj[0] * f.in, yj = rj[1] * f.in, zj = rj[2] * f.in;
  unsigned flags = 0;
  if (wall) rbl_pair_block_fast<true, true, U>(f.P, xi, yi, zi, xj, yj, zj, i == j, out9, flags);
  else rbl_pair_block_fast<false, true, U>(f.P, xi, yi, zi, xj, yj, zj, i == j, out9, flags);
  for (int k = 0; k < 9; ++k) out9[k] *= f.out;
  return flags;
}
// the same block through the ordered accumulation (rbl_pair_accum applied to the unit vectors)
unsigned units_accum(const double *ri, const double *rj, int i, int j, double a, int wall, double *out9)
{
  const Frame f(a);
  const double xi = ri[0] * f.in, yi = ri[1] * f.in, zi = ri[2] * f.in, xj = rj[0] * f.in, yj = rj[1] * f.in, zj = rj[2] * f.in;
  unsigned flags = 0;
  for (int c = 0; c < 3; ++c) {
    double ux = 0, uy = 0, uz = 0;
    const double fx = c == 0, fy = c == 1, fz = c == 2;
    if (wall) rbl_pair_accum<true, true, U>(f.P, xi, yi, zi, xj, yj, zj, fx, fy, fz, i == j, ux, uy, uz, flags);
    else rbl_pair_accum<false, true, U>(f.P, xi, yi, zi, xj, yj, zj, fx, fy, fz, i == j, ux, uy, uz, flags);
    out9[c] = ux * f.out; out9[3 + c] = uy * f.out; out9[6 + c] = uz * f.out;
  }
  return flags;
}
// the symmetric form (i != j): M_ij from U_i += M F_j and M_ji from U_j += M^T F_i, with or without the overlap test
unsigned units_sym(const double *ri, const double *rj, double a, int wall, int nearchk, double *Mij, double *Mji)
{
  const Frame f(a);
  const double xi = ri[0] * f.in, yi = ri[1] * f.in, zi = ri[2] * f.in, xj = rj[0] * f.in, yj = rj[1] * f.in, zj = rj[2] * f.in;
  unsigned flags = 0;
  for (int c = 0; c < 3; ++c) {
    const RblV3 F[1] = {{(double)(c == 0), (double)(c == 1), (double)(c == 2)}};
    RblV3 ui[1] = {{0, 0, 0}}, uj[1] = {{0, 0, 0}};
    if (wall) {
      if (nearchk) rbl_pair_symv<true, U, true>(f.P, xi, yi, zi, F, xj, yj, zj, F, ui, uj, flags);
      else rbl_pair_symv<true, U, false>(f.P, xi, yi, zi, F, xj, yj, zj, F, ui, uj, flags);
    } else {
      if (nearchk) rbl_pair_symv<false, U, true>(f.P, xi, yi, zi, F, xj, yj, zj, F, ui, uj, flags);
      else rbl_pair_symv<false, U, false>(f.P, xi, yi, zi, F, xj, yj, zj, F, ui, uj, flags);
    }
    const double ui3[3] = {ui[0].x, ui[0].y, ui[0].z}, uj3[3] = {uj[0].x, uj[0].y, uj[0].z};
    for (int p = 0; p < 3; ++p) { Mij[3 * p + c] = ui3[p] * f.out; Mji[3 * p + c] = uj3[p] * f.out; }
  }
  return flags;
}
}
