// Host build of the device pair arithmetic (rbl_pair.hpp) for CPU-side algebra checks -- see hip/hip_runtime.h here.
//   g++ -O2 -ffp-contract=fast -mfma -shared -fPIC -Itests/host_pair -o /tmp/libpair_host.so tests/host_pair/pair_host.cpp
#include "../../rigid_body_light_amd/csrc/rbl_pair.hpp"

static RblParams make_params(double a)
{
  RblParams P;
  P.a = a; P.inv_a = 1.0 / a; P.nf = 1.0; P.four_a2 = 4.0 * a * a; P.tiny2 = (1e-12 * a) * (1e-12 * a);
  P.c_near_A = -0.375 / a; P.c_near_B = 0.125 / a; P.no_damp = 0;
  return P;
}

extern "C" {
// ordered block (i <- j, h = z_j) by the fast accumulation form, unscaled, row-major
void fast_block(const double *ri, const double *rj, int i, int j, double a, int wall, double *out9)
{
  const RblParams P = make_params(a);
  unsigned flags = 0;
  for (int c = 0; c < 3; ++c) {
    double ux = 0, uy = 0, uz = 0;
    const double fx = c == 0, fy = c == 1, fz = c == 2;
    if (wall) rbl_pair_accum<true, true>(P, ri[0], ri[1], ri[2], rj[0], rj[1], rj[2], fx, fy, fz, i == j, ux, uy, uz, flags);
    else rbl_pair_accum<false, true>(P, ri[0], ri[1], ri[2], rj[0], rj[1], rj[2], fx, fy, fz, i == j, ux, uy, uz, flags);
    out9[c] = ux; out9[3 + c] = uy; out9[6 + c] = uz;
  }
}
// the same form in radius-scaled coordinates (UNIT = true: what k_apply_M and the velocity-field kernel run)
void fast_block_unit(const double *ri, const double *rj, int i, int j, double a, int wall, double *out9)
{
  const RblParams P = make_params(1.0);
  const double inv_a = 1.0 / a;
  const double xi = ri[0] * inv_a, yi = ri[1] * inv_a, zi = ri[2] * inv_a, xj = rj[0] * inv_a, yj = rj[1] * inv_a, zj = rj[2] * inv_a;
  unsigned flags = 0;
  for (int c = 0; c < 3; ++c) {
    double ux = 0, uy = 0, uz = 0;
    const double fx = c == 0, fy = c == 1, fz = c == 2;
    if (wall) rbl_pair_accum<true, true, true>(P, xi, yi, zi, xj, yj, zj, fx, fy, fz, i == j, ux, uy, uz, flags);
    else rbl_pair_accum<false, true, true>(P, xi, yi, zi, xj, yj, zj, fx, fy, fz, i == j, ux, uy, uz, flags);
    out9[c] = ux; out9[3 + c] = uy; out9[6 + c] = uz;
  }
}
// full ordered block (i <- j, h = z_j) in radius-scaled coordinates (what the MFMA kernel k_apply_M_mrhs forms), row-major, unscaled
void block_fast_unit(const double *ri, const double *rj, int i, int j, double a, int wall, double *out9)
{
  const RblParams P = make_params(1.0);
  const double inv_a = 1.0 / a;
  const double xi = ri[0] * inv_a, yi = ri[1] * inv_a, zi = ri[2] * inv_a, xj = rj[0] * inv_a, yj = rj[1] * inv_a, zj = rj[2] * inv_a;
  unsigned flags = 0;
  if (wall) rbl_pair_block_fast<true, true, true>(P, xi, yi, zi, xj, yj, zj, i == j, out9, flags);
  else rbl_pair_block_fast<false, true, true>(P, xi, yi, zi, xj, yj, zj, i == j, out9, flags);
}
// symmetric form in radius-scaled coordinates (what k_apply_M_sym runs): M_ij (from U_i += M F_j) and M_ji
// (from U_j += M^T F_i), both row-major, unscaled
void sym_blocks(const double *ri, const double *rj, double a, int wall, int nearchk, double *Mij, double *Mji)
{
  RblParams P = make_params(1.0);
  const double inv_a = 1.0 / a;   // the kernels multiply by P.inv_a
  const double xi = ri[0] * inv_a, yi = ri[1] * inv_a, zi = ri[2] * inv_a, xj = rj[0] * inv_a, yj = rj[1] * inv_a, zj = rj[2] * inv_a;
  unsigned flags = 0;
  for (int c = 0; c < 3; ++c) {
    const double fx = c == 0, fy = c == 1, fz = c == 2;
    const RblV3 f[1] = {{fx, fy, fz}};
    RblV3 ui[1] = {{0, 0, 0}}, uj[1] = {{0, 0, 0}};
    if (wall) {
      if (nearchk) rbl_pair_symv<true, true, true>(P, xi, yi, zi, f, xj, yj, zj, f, ui, uj, flags);
      else rbl_pair_symv<true, true, false>(P, xi, yi, zi, f, xj, yj, zj, f, ui, uj, flags);
    } else {
      if (nearchk) rbl_pair_symv<false, true, true>(P, xi, yi, zi, f, xj, yj, zj, f, ui, uj, flags);
      else rbl_pair_symv<false, true, false>(P, xi, yi, zi, f, xj, yj, zj, f, ui, uj, flags);
    }
    const double ui3[3] = {ui[0].x, ui[0].y, ui[0].z}, uj3[3] = {uj[0].x, uj[0].y, uj[0].z};
    for (int p = 0; p < 3; ++p) { Mij[3 * p + c] = ui3[p]; Mji[3 * p + c] = uj3[p]; }
  }
}
}
