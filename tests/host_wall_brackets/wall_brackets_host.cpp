// Host build of rbl_wall_coeffs (rbl_pair.hpp) in the SHARED length unit for tests/test_wall_brackets_cpu.py: the five scalars of the
// header's form (brackets X, Y kept un-multiplied, the factor u carried by w^3 and w^5) next to the form it replaced, restated here
// (b1 = -1 + u X and b2p = u Y formed, u^2 formed, multiplied by w and w^3).  The stand-in <hip/hip_runtime.h> is the one of tests/host_pair.
//   g++ -O2 -ffp-contract=fast -mfma -std=c++17 -shared -fPIC -Itests/host_pair -o libwall_brackets.so tests/host_wall_brackets/wall_brackets_host.cpp
#include "../../rigid_body_light_amd/csrc/rbl_pair.hpp"

namespace {
constexpr int U = RBL_UNIT_SHARED;

// the form before the brackets were kept: same inputs, same root, same constants
void wall_coeffs_before(double dz, double zi, double zj, double q, double A, double Bc, double *five)
{
  const double Rz = zi + zj;
  const double R2 = __builtin_fma(Rz, Rz, q);
  const double w = rbl_rsqrt(R2);
  const double u = w * w;
  const double v = __builtin_fma(-q, u, 1.0);
  const double Q = __builtin_fma(v, -30.0, 6.0);
  const double m = __builtin_fma(-2.0 * zi, zj, -2.0);
  const double b1 = __builtin_fma(u, __builtin_fma(u, Q, __builtin_fma(v, 6.0, m)), -1.0);
  const double b2p = u * __builtin_fma(u, __builtin_fma(v, 210.0, -30.0), __builtin_fma(6.0 * zi, zj, Q));
  const double uu = u * u;
  const double T1p = __builtin_fma(uu, -60.0, b2p);
  const double w3 = w * u;
  const double Bw = Bc - w3;
  const double cF = __builtin_fma(w, b1, A);
  const double beta = __builtin_fma(b2p, w3, Bw);
  const double gm = dz * Bw, gdw = Rz * w3;
  const double gxz = __builtin_fma(-T1p, gdw, gm);
  const double gzx = __builtin_fma(T1p, gdw, gm);
  const double c = __builtin_fma(uu, __builtin_fma(v, 180.0, -24.0), -(v * __builtin_fma(12.0, u, b2p)));
  const double mzz = __builtin_fma(w, c, __builtin_fma(gm, dz, cF));
  five[0] = cF; five[1] = beta; five[2] = gxz; five[3] = gzx; five[4] = mzz;
}
}   // namespace

extern "C" {
// One pair (i <- j, i != j), positions in physical lengths, blob radius a.  now5 / before5: cF, beta r'^2, gxz r', gzx r', mzz of the header's
// form and of the restated one, each times lambda: the size of the block entries they make, in units of 1 / (8 pi eta a) (r': the separation
// in the unit; the lateral scalars multiply dl, |dl| <= r').  scale2: A times lambda (the free-space coefficient, near or far formula as the kernels choose) and a / r.
void wall_brackets_pair(const double *ri, const double *rj, double a, double *now5, double *before5, double *scale2)
{
  RblParams Q;
  Q.a = a; Q.inv_a = 1.0 / a; Q.nf = 1.0; Q.four_a2 = 4.0 * a * a; Q.tiny2 = (1e-12 * a) * (1e-12 * a);
  Q.c_near_A = -0.375 / a; Q.c_near_B = 0.125 / a; Q.no_damp = 0;
  const double in = rbl_unit_pos_scale<U>(Q), out = rbl_unit_out_scale<U>(Q);
  const RblParams P = rbl_unit_params<U>(Q);
  const double xi = ri[0] * in, yi = ri[1] * in, zi = ri[2] * in, xj = rj[0] * in, yj = rj[1] * in, zj = rj[2] * in;
  // the free-space part as rbl_pair_symv forms it
  const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
  const double q = __builtin_fma(dy, dy, dx * dx);
  const double r2 = __builtin_fma(dz, dz, q);
  const double invr = rbl_rsqrt(r2);
  const double s3 = (invr * invr) * invr;
  double A = __builtin_fma(s3, 2.0, invr);
  double Bc = __builtin_fma(s3, -6.0, invr) * (invr * invr);
  if (r2 < P.four_a2) {
    A = __builtin_fma(r2 * invr, P.c_near_A, (4.0 / 3.0) * RBL_UNIT_INV_L);
    Bc = invr * P.c_near_B;
  }
  double f[5], g[5];
  rbl_wall_coeffs<U>(P, dz, zi, zj, q, r2, A, Bc, f[0], f[1], f[2], f[3], f[4]);
  wall_coeffs_before(dz, zi, zj, q, A, Bc, g);
  const double r = std::sqrt(r2);
  const double dim[5] = {1.0, r2, r, r, 1.0};
  for (int k = 0; k < 5; ++k) { now5[k] = f[k] * dim[k] * out; before5[k] = g[k] * dim[k] * out; }
  scale2[0] = A * out; scale2[1] = RBL_UNIT_L * invr;     // a / r = lambda / r'
}
}
