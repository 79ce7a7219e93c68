// rbl_ens_drive.hip -- the time-dependent body input of a driven ensemble run and its lock-in sums (include/rbl.h section 5,
// rbl_ensemble_run_driven / rbl_ensemble_drive_eval).
//
// A run keeps its inputs constant; a driven run evaluates ONE of them, the body input (F_body, or body_in of a masked run), anew
// before every step and per replica:
//     in_r = ((A0_r + P_r[phase(p_r)]) + C_r cos(w_r t_r)) + S_r sin(w_r t_r),     t_r = t0_r + dt accepted[r]
// with the replica's own clock (the field clock of rbl_forces.hip's ia_field_B: product and sum rounded separately) and its own
// position p_r in a periodic piecewise-constant schedule (rbl_schedule.hpp, the motor schedule's map).  Two kernels:
//   k_ens_drive          before the step's sequence, one thread per entry of [R 6 N_bod]: the evaluated input into the buffer the
//                        step reads (EnsWork::F; A0 stays in a buffer of the drive's own), cs and sn of the replica into a table
//   k_ens_drive_commit   after k_ens_commit (and k_ens_obs_commit), one thread per entry: the commit's decision again from the
//                        run's status and the replica's verdict word; where the replica committed its cycle position moves on
//                        and, with lockin, the step's X(q^n), U and F times the table's cs / sn are added to the sums
// Every entry of every sum belongs to one thread and is added to in step order, product and sum rounded one after the other: no
// atomics on doubles, no scratch, two runs agree bitwise, replica r of R is the R = 1 run.  rbl_ensemble_drive_eval is
// k_ens_drive alone with a read-back: the device's sincos is not the host's, so this is what a loop of one-step calls
// reproduces a run with.  The run loop itself is ens_run's (rbl_ens_run.hip); nothing here is context state.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_schedule.hpp"

namespace {

constexpr int DT = 256;          // threads of both kernels: one entry each

// what k_ens_drive reads and writes (device pointers).  C, S: NULL for zeros; P: read while n_phases > 0
struct EnsDriveDev {
  const double *A0, *C, *S, *P, *om, *t0;
  const int *cum, *pos, *accepted;
  int n_phases, amp_sets, phase_sets;
  double dt;
  double *in, *cs_sn;
};

// One thread per entry e of replica r.  Every thread of a replica evaluates the same clock and the same sincos -- cheaper than a
// second launch or a wait --, thread e = 0 writes them into the table k_ens_drive_commit reads.  Contraction is off for the
// clock (ia_field_B's two statements) and for the three additions: every product is rounded before it is added
__global__ __launch_bounds__(DT) void k_ens_drive(int R, int nb6, EnsDriveDev D)
{
  const long idx = (long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long)R * nb6) return;
  const int r = (int)(idx / nb6), e = (int)(idx - (long)r * nb6);
  const double n = (double)D.accepted[r];
  double t;
  {
#pragma clang fp contract(off)
    const double s = D.dt * n;
    t = D.t0[r] + s;
  }
  double sn, cs;
  sincos(__dmul_rn(D.om[r], t), &sn, &cs);
  double p = 0.0;
  if (D.n_phases) {
    const int k = rbl_schedule_phase(D.cum, D.n_phases, D.pos[r]);
    p = D.P[((size_t)k * D.phase_sets + (D.phase_sets == 1 ? 0 : r)) * nb6 + e];
  }
  const size_t ia = (size_t)(D.amp_sets == 1 ? 0 : r) * nb6 + e;
  const double cc = D.C ? D.C[ia] : 0.0, ss = D.S ? D.S[ia] : 0.0;
  double v;
  {
#pragma clang fp contract(off)
    const double a = D.A0[idx] + p;
    const double hc = cc * cs;
    const double hs = ss * sn;
    v = (a + hc) + hs;
  }
  D.in[idx] = v;
  if (e == 0) { D.cs_sn[2 * (size_t)r] = cs; D.cs_sn[2 * (size_t)r + 1] = sn; }
}

// what k_ens_drive_commit reads and writes.  sums: X_c | X_s (R 3 N_bod each) | U_c | U_s | F_c | F_s (R 6 N_bod each) | norm (R 5)
struct EnsDriveCommitDev {
  const int *stopped; const unsigned *vflag; const int *accepted;
  const double *Xo, *U, *Fo, *cs_sn, *t0;
  const int *cum;
  long u_stride;
  int n_phases, lockin;
  double dt;
  int *pos;
  double *sums, *t_end;
};

// One thread per entry e of replica r, after k_ens_commit (the status and the verdict words are final for this step, accepted[r]
// counts this step where it committed).  pos[r] and t_end[r] belong to thread e = 0; entry e of U_c, U_s, F_c, F_s, entry
// e < 3 N_bod of X_c, X_s and entry e < 5 of norm to thread e (6 N_bod >= 6)
__global__ __launch_bounds__(DT) void k_ens_drive_commit(int R, int nb6, EnsDriveCommitDev D)
{
  const long idx = (long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long)R * nb6) return;
  const int r = (int)(idx / nb6), e = (int)(idx - (long)r * nb6);
  const bool ok = D.stopped[0] == 0 && D.vflag[r] == 0;    // k_ens_commit's decision
  if (e == 0) {
    if (ok && D.n_phases) D.pos[r] = rbl_schedule_next(D.cum, D.n_phases, D.pos[r]);
    const double n = (double)D.accepted[r];
    {
#pragma clang fp contract(off)
      const double s = D.dt * n;
      D.t_end[r] = D.t0[r] + s;
    }
  }
  if (!ok || !D.lockin) return;
  const double cs = D.cs_sn[2 * (size_t)r], sn = D.cs_sn[2 * (size_t)r + 1];
  const int nb3 = nb6 / 2;
  const size_t Rz = (size_t)R, nx = Rz * nb3, nu = Rz * nb6;
  double *X_c = D.sums, *X_s = X_c + nx, *U_c = X_s + nx, *U_s = U_c + nu, *F_c = U_s + nu, *F_s = F_c + nu, *norm = F_s + nu;
  {
#pragma clang fp contract(off)
    const double u = D.U[(size_t)r * D.u_stride + e];
    const double uc = u * cs, us = u * sn;
    U_c[idx] = U_c[idx] + uc;
    U_s[idx] = U_s[idx] + us;
    if (D.Fo) {
      const double f = D.Fo[idx];
      const double fc = f * cs, fs = f * sn;
      F_c[idx] = F_c[idx] + fc;
      F_s[idx] = F_s[idx] + fs;
    }
    if (e < nb3) {
      const size_t i = (size_t)r * nb3 + e;
      const double x = D.Xo[i];
      const double xc = x * cs, xs = x * sn;
      X_c[i] = X_c[i] + xc;
      X_s[i] = X_s[i] + xs;
    }
    if (e < 5) {
      const double q = e == 0 ? cs : e == 1 ? sn : e == 2 ? cs * cs : e == 3 ? sn * sn : cs * sn;
      const size_t i = 5 * (size_t)r + e;
      norm[i] = norm[i] + q;
    }
  }
}

size_t drive_sum_doubles(int R, int Nb) { return (size_t)R * (30 * (size_t)Nb + 5); }

// (R == 0, no ensemble: nothing to compare with)
bool set_count_ok(int sets, int R, bool zero) { return !R || (zero && sets == 0) || sets == 1 || sets == R; }

}  // namespace

int ens_drive_check(rbl_ctx *c, const char *who, const rbl_run_drive_opts *d, int R, int Nb, bool *empty, RblEnsDriveRun *D)
{
  const std::string w(who);
  if (d->size != (int64_t)sizeof(rbl_run_drive_opts)) return rbl_fail(c, RBL_ERR_ARG, w + ": drive.size is not sizeof(rbl_run_drive_opts)");
  const bool harmonic = d->cos_amp || d->sin_amp, lockin = d->lockin != 0;
  if (d->n_phases < 0) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: n_phases must be >= 0");
  *empty = !harmonic && d->n_phases == 0 && !lockin;
  D->o = d;
  // the set counts (no ensemble, R == 0: a count of 1 is the only one whose array has a known length; what needs R is left to the
  // underlying call's RBL_ERR_STATE)
  const std::string sR = R ? std::to_string(R) : std::string("the ensemble's replica count");
  if (harmonic && !set_count_ok(d->amp_sets, R, false)) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: amp_sets must be 1 or R = " + sR);
  if ((harmonic || lockin || d->omega) && !set_count_ok(d->omega_sets, R, false))
    return rbl_fail(c, RBL_ERR_ARG, w + ": drive: omega_sets must be 1 or R = " + sR);
  if (!set_count_ok(d->t0_sets, R, true)) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: t0_sets must be 0, 1 or R = " + sR);
  if (d->n_phases && !set_count_ok(d->phase_sets, R, false)) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: phase_sets must be 1 or R = " + sR);
  if (!set_count_ok(d->start_sets, R, true)) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: start_sets must be 0, 1 or R = " + sR);
  // arrays a count says are read
  if ((harmonic || lockin) && !d->omega) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: omega is NULL while a harmonic part or lockin is given");
  if (d->t0_sets && !d->t0) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: t0 is NULL while t0_sets > 0");
  if (d->n_phases && (!d->phase_steps || !d->phase_in))
    return rbl_fail(c, RBL_ERR_ARG, w + ": drive: phase_steps or phase_in is NULL while n_phases > 0");
  if (d->start_sets && !d->cycle_start) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: cycle_start is NULL while start_sets > 0");
  // finite values
  const size_t nb6 = 6 * (size_t)Nb;
  auto finite = [&](const double *a, size_t sets, size_t per, const std::string &name) {
    if (!R && sets != 1) return (int)RBL_OK;
    for (size_t i = 0; a && i < sets * per; ++i)
      if (!std::isfinite(a[i]))
        return rbl_fail(c, RBL_ERR_ARG, w + ": drive: " + name + ": set " + std::to_string(i / per) + ", entry " + std::to_string(i % per) +
                                            ": the value must be finite");
    return (int)RBL_OK;
  };
  int rc;
  if ((rc = finite(d->cos_amp, (size_t)d->amp_sets, nb6, "cos_amp"))) return rc;
  if ((rc = finite(d->sin_amp, (size_t)d->amp_sets, nb6, "sin_amp"))) return rc;
  if ((rc = finite(d->omega, (size_t)d->omega_sets, 1, "omega"))) return rc;
  if ((rc = finite(d->t0_sets ? d->t0 : nullptr, (size_t)d->t0_sets, 1, "t0"))) return rc;
  for (int k = 0; k < d->n_phases; ++k)
    if ((rc = finite(d->phase_in + (size_t)k * d->phase_sets * nb6, (size_t)d->phase_sets, nb6, "phase_in: phase " + std::to_string(k)))) return rc;
  // the schedule
  D->cum.clear();
  long long len = 0;
  if (d->n_phases) {
    D->cum.push_back(0);
    for (int k = 0; k < d->n_phases; ++k) {
      if (d->phase_steps[k] < 1)
        return rbl_fail(c, RBL_ERR_ARG, w + ": drive: phase_steps[" + std::to_string(k) + "] = " + std::to_string(d->phase_steps[k]) +
                                            ": every phase lasts at least one step");
      len += d->phase_steps[k];
      if (len > 0x7fffffffLL) return rbl_fail(c, RBL_ERR_ARG, w + ": drive: the cycle's length (the sum of phase_steps) must fit 31 bits");
      D->cum.push_back((int)len);
    }
  }
  D->start.assign((size_t)R, 0);
  for (int s = 0; s < (R ? d->start_sets : std::min(d->start_sets, 1)); ++s) {
    const long long p = d->cycle_start[s];
    if (p < 0 || p >= std::max(len, 1LL))
      return rbl_fail(c, RBL_ERR_ARG, w + ": drive: cycle_start[" + std::to_string(s) + "] = " + std::to_string(p) +
                                          " lies outside the cycle, 0 <= value < " + std::to_string(std::max(len, 1LL)) +
                                          (len ? "" : " (no phases: only 0)"));
    if (d->start_sets == 1) D->start.assign((size_t)R, (int)p);
    else if (R) D->start[(size_t)s] = (int)p;
  }
  if ((harmonic || lockin) && c->S.params_set && !(c->S.dt > 0.0))
    return rbl_fail(c, RBL_ERR_ARG, w + ": drive: dt must be positive with a harmonic part or lockin");
  D->omega.assign((size_t)R, 0.0);
  D->t0.assign((size_t)R, 0.0);
  for (int r = 0; r < R; ++r) {
    if (d->omega) D->omega[(size_t)r] = d->omega[d->omega_sets == 1 ? 0 : r];
    if (d->t0_sets) D->t0[(size_t)r] = d->t0[d->t0_sets == 1 ? 0 : r];
  }
  return RBL_OK;
}

size_t ens_drive_carve(RblEnsDriveRun &D, void *base, int R, int Nb)
{
  const size_t Rz = (size_t)R, nb6 = 6 * (size_t)Nb, np = (size_t)D.o->n_phases;
  RblCarve C{(char *)base};
  D.A0 = C.take<double>(Rz * nb6);
  D.C = C.take<double>(D.o->cos_amp ? (size_t)D.o->amp_sets * nb6 : 0);
  D.S = C.take<double>(D.o->sin_amp ? (size_t)D.o->amp_sets * nb6 : 0);
  D.P = C.take<double>(np ? np * (size_t)D.o->phase_sets * nb6 : 0);
  D.om = C.take<double>(Rz); D.t0d = C.take<double>(Rz); D.cs_sn = C.take<double>(2 * Rz);
  D.sums = C.take<double>(drive_sum_doubles(R, Nb));
  D.t_end = C.take<double>(Rz);
  D.cum_d = C.take<int>(np + 1); D.pos = C.take<int>(Rz);
  if (!D.o->cos_amp) D.C = nullptr;
  if (!D.o->sin_amp) D.S = nullptr;
  return C.off;
}

int ens_drive_begin(rbl_ctx *c, RblEnsDriveRun &D, void *base, int R, int Nb, const double *A0)
{
  const size_t Rz = (size_t)R, nb6 = 6 * (size_t)Nb, np = (size_t)D.o->n_phases;
  ens_drive_carve(D, base, R, Nb);
  int rc;
  if ((rc = copy_h2d(c, D.A0, A0, sizeof(double) * Rz * nb6))) return rc;
  if (D.C && (rc = copy_h2d(c, D.C, D.o->cos_amp, sizeof(double) * (size_t)D.o->amp_sets * nb6))) return rc;
  if (D.S && (rc = copy_h2d(c, D.S, D.o->sin_amp, sizeof(double) * (size_t)D.o->amp_sets * nb6))) return rc;
  if ((rc = copy_h2d(c, D.om, D.omega.data(), sizeof(double) * Rz))) return rc;
  if ((rc = copy_h2d(c, D.t0d, D.t0.data(), sizeof(double) * Rz))) return rc;
  if ((rc = copy_h2d(c, D.pos, D.start.data(), sizeof(int) * Rz))) return rc;
  if (np) {
    if ((rc = copy_h2d(c, D.cum_d, D.cum.data(), sizeof(int) * (np + 1)))) return rc;
    if ((rc = copy_h2d(c, D.P, D.o->phase_in, sizeof(double) * np * (size_t)D.o->phase_sets * nb6))) return rc;
  }
  RBL_HIP(c, hipMemsetAsync(D.sums, 0, sizeof(double) * drive_sum_doubles(R, Nb), c->stream));
  return RBL_OK;
}

void ens_drive_step(rbl_ctx *c, const RblEnsDriveRun &D, int R, int Nb, const int *d_accepted, double *d_in)
{
  const int nb6 = 6 * Nb;
  const long n = (long)R * nb6;
  const EnsDriveDev A = {D.A0, D.C, D.S, D.P, D.om, D.t0d, D.cum_d, D.pos, d_accepted, (int)D.o->n_phases, D.C || D.S ? (int)D.o->amp_sets : 1,
                         D.o->n_phases ? (int)D.o->phase_sets : 1, c->S.dt, d_in, D.cs_sn};
  hipLaunchKernelGGL(k_ens_drive, dim3((unsigned)((n + DT - 1) / DT)), dim3(DT), 0, c->stream, R, nb6, A);
}

void ens_drive_after(rbl_ctx *c, const RblEnsDriveRun &D, int R, int Nb, const int *d_stopped, const unsigned *d_vflag,
                     const int *d_accepted, const double *d_Xo, const double *d_U, long u_stride, const double *d_Fo)
{
  const int nb6 = 6 * Nb;
  const long n = (long)R * nb6;
  const EnsDriveCommitDev A = {d_stopped, d_vflag, d_accepted, d_Xo, d_U, D.masked ? d_Fo : nullptr, D.cs_sn, D.t0d, D.cum_d, u_stride,
                               (int)D.o->n_phases, D.o->lockin ? 1 : 0, c->S.dt, D.pos, D.sums, D.t_end};
  hipLaunchKernelGGL(k_ens_drive_commit, dim3((unsigned)((n + DT - 1) / DT)), dim3(DT), 0, c->stream, R, nb6, A);
}

int ens_drive_end(rbl_ctx *c, const RblEnsDriveRun &D, int R, int Nb)
{
  const size_t Rz = (size_t)R, nx = Rz * 3 * Nb, nu = Rz * 6 * Nb;
  const rbl_run_drive_out *q = D.out;
  int rc;
  if (q->cycle_pos && (rc = copy_d2h(c, q->cycle_pos, D.pos, sizeof(int32_t) * Rz))) return rc;
  if (q->t_end && (rc = copy_d2h(c, q->t_end, D.t_end, sizeof(double) * Rz))) return rc;
  if (D.o->lockin) {
    const double *X_c = D.sums, *X_s = X_c + nx, *U_c = X_s + nx, *U_s = U_c + nu, *F_c = U_s + nu, *F_s = F_c + nu, *norm = F_s + nu;
    if (q->X_c && (rc = copy_d2h(c, q->X_c, X_c, sizeof(double) * nx))) return rc;
    if (q->X_s && (rc = copy_d2h(c, q->X_s, X_s, sizeof(double) * nx))) return rc;
    if (q->U_c && (rc = copy_d2h(c, q->U_c, U_c, sizeof(double) * nu))) return rc;
    if (q->U_s && (rc = copy_d2h(c, q->U_s, U_s, sizeof(double) * nu))) return rc;
    if (D.masked && q->F_c && (rc = copy_d2h(c, q->F_c, F_c, sizeof(double) * nu))) return rc;
    if (D.masked && q->F_s && (rc = copy_d2h(c, q->F_s, F_s, sizeof(double) * nu))) return rc;
    if (q->norm && (rc = copy_d2h(c, q->norm, norm, sizeof(double) * 5 * Rz))) return rc;
  }
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}

void ens_drive_empty_out(const rbl_ctx *c, const RblEnsDriveRun &D, int R, const int *accepted)
{
  rbl_run_drive_out *q = D.out;
  if (!q) return;
  if (q->cycle_pos) std::memset(q->cycle_pos, 0, sizeof(int32_t) * (size_t)R);
  for (int r = 0; q->t_end && r < R; ++r) {
#pragma clang fp contract(off)
    const double s = c->S.dt * (double)accepted[r];
    q->t_end[r] = D.t0[(size_t)r] + s;
  }
}

// ---- C ABI (include/rbl.h section 5, driven runs) -------------------------------------------------------------------

int rbl_ensemble_drive_eval(rbl_ctx *c, const rbl_run_drive_opts *d, const double *base, const int32_t *accepted, const int32_t *cycle_pos,
                            double *in_out, double *cs_sn)
{
  const char *who = "ensemble_drive_eval";
  const std::string w(who);
  if (!c) return RBL_ERR_ARG;
  if (!d || !base || !in_out) return rbl_fail(c, RBL_ERR_ARG, w + ": drive, base or in_out is NULL");
  int rc = need_params(c); if (rc) return rc;
  if ((rc = ens_state_check(c, w + ": "))) return rc;
  const int R = c->ens_R, Nb = c->ens_Nb;
  RblEnsDriveRun D;
  bool empty;
  if ((rc = ens_drive_check(c, who, d, R, Nb, &empty, &D))) return rc;
  const long long len = D.cum.empty() ? 1 : D.cum.back();
  for (int r = 0; r < R; ++r) {
    if (accepted && accepted[r] < 0) return rbl_fail(c, RBL_ERR_ARG, w + ": accepted[" + std::to_string(r) + "] must be >= 0");
    if (cycle_pos && (cycle_pos[r] < 0 || cycle_pos[r] >= len))
      return rbl_fail(c, RBL_ERR_ARG, w + ": cycle_pos[" + std::to_string(r) + "] = " + std::to_string(cycle_pos[r]) +
                                          " lies outside the cycle, 0 <= value < " + std::to_string(len));
    if (cycle_pos) D.start[(size_t)r] = cycle_pos[r];
  }
  RblEnsView v;
  if ((rc = ens_view(c, &v))) return rc;
  const size_t Rz = (size_t)R, nb6 = 6 * (size_t)Nb, dbytes = ens_drive_carve(D, nullptr, R, Nb);
  if ((rc = rbl_dev_reserve(c, c->d_ens_obs, dbytes + sizeof(double) * Rz * nb6 + sizeof(int) * Rz))) return rc;
  double *d_in = (double *)((char *)c->d_ens_obs.p + dbytes);
  int *d_acc = (int *)(d_in + Rz * nb6);
  if ((rc = ens_drive_begin(c, D, c->d_ens_obs.p, R, Nb, base))) return rc;
  if (accepted) { if ((rc = copy_h2d(c, d_acc, accepted, sizeof(int) * Rz))) return rc; }
  else RBL_HIP(c, hipMemsetAsync(d_acc, 0, sizeof(int) * Rz, c->stream));
  ens_drive_step(c, D, R, Nb, d_acc, d_in);
  RBL_HIP(c, hipGetLastError());
  if ((rc = copy_d2h(c, in_out, d_in, sizeof(double) * Rz * nb6))) return rc;
  if (cs_sn && (rc = copy_d2h(c, cs_sn, D.cs_sn, sizeof(double) * 2 * Rz))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  return RBL_OK;
}
