/*
 * interaction_oracle.c -- CPU restatement of the force model of include/rbl.h section 4 (test infrastructure, NOT the
 * product; the reference has no force model, so this is the project's own statement of it, not a pin to the reference).
 *
 * A plain all-pairs double loop over the blobs: every ordered pair (i, j) of blobs of DIFFERENT bodies with
 * |r_i - r_j|^2 <= r_cut^2, no neighbour lists, no cull.  OpenMP over i only; each i sums its j in increasing order.
 *
 *   r[3N]       blob positions, body-major (N = N_bod * N_blb)
 *   X[3 N_bod]  body centres (torques are taken about them)
 *   f[3N]       physical force on every blob;  FT[6 N_bod] = sum over the body's blobs of (f, (r - X) x f)
 *   returns the total energy  sum_i (w z_i + U_w(z_i)) + sum_{i<j, different bodies} U_b(|r_i - r_j|)
 */
#include <math.h>
#include <stdlib.h>

static void pair(double r, double a, double eps_b, double b_b, double *U, double *g)   /* g = -U'(r) / r */
{
  const double two_a = 2.0 * a;
  if (r >= two_a) {
    *U = eps_b * (two_a / r) * exp(-(r - two_a) / b_b);
    *g = *U * (1.0 / r + 1.0 / b_b) / r;
  } else {
    const double slope = eps_b * (1.0 / two_a + 1.0 / b_b);
    *U = eps_b + slope * (two_a - r);
    *g = r > 0.0 ? slope / r : 0.0;
  }
}

double orc_interactions(const double *r, const double *X, int N_bod, int N_blb, double a, int wall, double w, double eps_wall,
                        double b_wall, double eps_blob, double b_blob, double r_cut, double *f, double *FT)
{
  const long N = (long)N_bod * N_blb;
  double *e = (double *)malloc(sizeof(double) * (size_t)(N > 0 ? N : 1));
  const double rc2 = r_cut * r_cut;
#pragma omp parallel for schedule(dynamic, 64)
  for (long i = 0; i < N; ++i) {
    const long bi = i / N_blb;
    double fx = 0.0, fy = 0.0, fz = 0.0, en = 0.0;
    for (long bj = 0; bj < N_bod; ++bj) {
      if (bj == bi) continue;                                  /* pairs inside one body are left out */
      for (long j = bj * N_blb; j < (bj + 1) * N_blb; ++j) {
        const double dx = r[3 * i] - r[3 * j], dy = r[3 * i + 1] - r[3 * j + 1], dz = r[3 * i + 2] - r[3 * j + 2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 > rc2) continue;                                /* beyond r_cut: nothing */
        double U, g;
        pair(sqrt(d2), a, eps_blob, b_blob, &U, &g);
        fx += g * dx; fy += g * dy; fz += g * dz;
        en += 0.5 * U;
      }
    }
    const double h = r[3 * i + 2];
    fz -= w;
    en += w * h;
    if (wall) {
      if (h >= a) { const double U = eps_wall * exp(-(h - a) / b_wall); fz += U / b_wall; en += U; }
      else { fz += eps_wall / b_wall; en += eps_wall + eps_wall / b_wall * (a - h); }
    }
    f[3 * i] = fx; f[3 * i + 1] = fy; f[3 * i + 2] = fz;
    e[i] = en;
  }
  double E = 0.0;
  for (long i = 0; i < N; ++i) E += e[i];
  free(e);
  for (int b = 0; b < N_bod; ++b) {
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < N_blb; ++k) {
      const long i = (long)b * N_blb + k;
      const double lx = r[3 * i] - X[3 * b], ly = r[3 * i + 1] - X[3 * b + 1], lz = r[3 * i + 2] - X[3 * b + 2];
      const double *v = f + 3 * i;
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
      s[3] += ly * v[2] - lz * v[1]; s[4] += lz * v[0] - lx * v[2]; s[5] += lx * v[1] - ly * v[0];
    }
    for (int d = 0; d < 6; ++d) FT[6 * b + d] = s[d];
  }
  return E;
}
