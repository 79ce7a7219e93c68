// rbl_ens_run.hip -- runs of ensemble steps (include/rbl.h section 5): n steps of every replica in one call.
//
// The four exported calls -- rbl_ensemble_run, _run_jointed, _run_observed, _run_driven -- fill one request (EnsRunReq) and hand it to
// ens_run_request, which makes every check, in the order and with the words each entry point has always had, and writes a plan
// (EnsRunPlan): how a step is taken, and which parts are active -- joints when they are switched on (off or never set: the plain
// deterministic run, cycle_pos zeroed afterwards), observers when n_probes > 0 or moments is set, the drive when it is not empty (an
// empty one: t_end and cycle_pos follow from the accepted counts the run reads back anyway).  ens_run takes the plan; nothing
// re-enters the chain.
//
// The loop.  Each step function of rbl_ensemble.hip is an enqueueing part (ens_enqueue_det / ens_enqueue_bd) and a finish (the
// read-back, the host's verdict, the swap).  A run uploads its inputs once, enqueues the first part per step with them resident, and
// lets two kernels of its own stand where the finish stood:
//   k_ens_verdict             per replica (one workgroup): its error word, and under the reject policy the wall check of q^{n+1};
//                             one compare-and-swap latches the step that stops the run
//   k_ens_commit              per replica, a second launch (so `stopped` is final without any wait between workgroups): commit, or
//                             q^n copied into the new buffer; counters, sums over accepted steps, the frame
// The host swaps the two configuration buffers after every step without a synchronisation and reads back once at the end.
//
// The parts have one shape -- carve (their bytes behind the run's own buffer), begin (uploads, once), after (the part's launches
// behind the commit, handed the step's frame index), end (its share of the read-back):
//   joints      (here) the loop goes around the jointed step (an EnsJtStep); after the commit and the flip k_ens_jt_run, per replica and
//               joint: theta += rate dt where the replica committed, its position in the motor schedule, the sum of phi, the next step's
//               rates, the frame's theta and phi (k_ens_jt_rates before the first step, k_ens_jt_geom for a recording step's gaps)
//   observers   (rbl_ens_field.hip) in the step, on its lambda: k_first_moments, k_ens_probe, k_ens_obs_flags; after the commit k_ens_obs_commit
//   drive       (rbl_ens_drive.hip) one hook more, k_ens_drive before the step's sequence (the body input into EnsWork::F); after the
//               commit and the observers' k_ens_drive_commit
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rbl_api_internal.hpp"
#include "rbl_body_dev.hpp"
#include "rbl_schedule.hpp"
#include "rbl_small_dev.hpp"

namespace {

constexpr int ET = 256;          // threads of the per-replica kernels

// ---- a run of steps (rbl_ensemble_run): the verdict and the commit of every step, per replica, on the device ----------------
// The few bytes the host polls.  stopped: 1 + the step that stopped the run (0: never; written once, by the first verdict that
// finds a reason); stop_rep: R - r of the first failing replica r of that step (0: none, a batch-level failure); batch: the batch
// word of that step
struct EnsRunStatus { int stopped, stop_rep; unsigned batch; int pad; };

// what the commit kernel reads and writes (device pointers; the frame slots are NULL in a step that records none)
struct EnsRunDev {
  const double *Xo, *Qo;                 // q^n
  double *Xn, *Qn;                       // q^{n+1} as k_ens_evolve left it; q^n again where the replica does not commit
  const unsigned *vflag, *gerr;
  const int *iters; const double *resid;
  const double *Fo;                      // the masked solve's loads (NULL: nobody prescribed)
  EnsRunStatus *st;
  int *accepted, *rejected; unsigned *first_flags; long long *iters_sum; double *resid_max, *F_sum, *F_last;
  double *fX, *fQ; int *fA; double *fF;
};

// One workgroup per replica: the replica's verdict on step `step`, vflag[r] = its error word as the step's kernels left it and,
// with reject, the validation of q^{n+1} (Xn, Qn) BEFORE it commits: a blob of the new configuration below the wall is
// RBL_FLAG_BELOW_WALL, its height computed term for term as k_body_geom does (lever arm with contraction off, then + X), so this
// is the verdict the next step's k_build_M or pair sweep would reach.  Non-finite components of Xn, Qn are in the word already
// (k_ens_evolve).  Lanes that find something OR it into one LDS word.  Then the run-level decision: the batch word, or under
// the stop policy any replica's word, stops the run at this step unless it stopped before -- one compare-and-swap, nobody waits
template <bool WALL>
__global__ __launch_bounds__(ET) void k_ens_verdict(int Nb, int nbl, int step, int reject, const double *__restrict__ Xn,
                                                    const double *__restrict__ Qn, const double *__restrict__ cfg,
                                                    const unsigned *__restrict__ rerr, const unsigned *__restrict__ gerr,
                                                    unsigned *__restrict__ vflag, EnsRunStatus *st)
{
  __shared__ unsigned s_flags;
  const int r = blockIdx.x, t = threadIdx.x;
  if (t == 0) s_flags = rerr[r];
  __syncthreads();
  if (WALL && reject && t < Nb * nbl) {
    const int b = t / nbl, k = t - b * nbl;
    const size_t g = (size_t)r * Nb + b;
    double Rm[9];
    rbl_quat_rot9(Qn + 4 * g, Rm);
    const double c0 = cfg[3 * k], c1 = cfg[3 * k + 1], c2 = cfg[3 * k + 2];
    double p2;
    {
#pragma clang fp contract(off)
      const double l2 = c0 * Rm[6] + c1 * Rm[7] + c2 * Rm[8];
      p2 = l2 + Xn[3 * g + 2];
    }
    if (p2 < 0.0) atomicOr(&s_flags, (unsigned)RBL_FLAG_BELOW_WALL);
  }
  __syncthreads();
  if (t == 0) {
    const unsigned f = s_flags;
    vflag[r] = f;
    if (gerr[0] || (!reject && f)) atomicCAS(&st->stopped, 0, step + 1);
  }
}

// One workgroup per replica, after k_ens_verdict has finished for all of them (st->stopped is final for this step): the replica
// commits when the run has not stopped and its word is clear; otherwise q^n is copied into the new buffer, which the host
// makes the current one without looking.  Counters, the sums over accepted steps and the frame follow the same decision; every
// entry of F_sum is added to by one thread, in step order.  Nothing counts after the stopping step
__global__ __launch_bounds__(ET) void k_ens_commit(int R, int Nb, int step, EnsRunDev D)
{
  const int r = blockIdx.x, t = threadIdx.x;
  const int stopped = D.st->stopped;
  const unsigned f = D.vflag[r];
  const bool ok = stopped == 0 && f == 0;
  const int acc = D.accepted[r] + (ok ? 1 : 0);
  __syncthreads();                                     // every thread has read accepted[r]
  if (t == 0) {
    if (ok) {
      D.accepted[r] = acc;
      D.iters_sum[r] += D.iters[r];
      if (D.resid[r] > D.resid_max[r]) D.resid_max[r] = D.resid[r];
    } else if (f && (stopped == 0 || stopped == step + 1)) {
      if (D.rejected[r] == 0) D.first_flags[r] = f;
      D.rejected[r] += 1;
    }
    if (stopped == step + 1) {                         // the stopping step names its first failing replica and keeps the batch word
      if (f) atomicMax(&D.st->stop_rep, R - r);
      if (r == 0) D.st->batch = D.gerr[0];
    }
    if (D.fA) D.fA[r] = acc;
  }
  const int nx = 3 * Nb, nq = 4 * Nb, nf = 6 * Nb;
  for (int j = t; j < nx; j += ET) {
    const size_t i = (size_t)r * nx + j;
    double v = D.Xn[i];
    if (!ok) { v = D.Xo[i]; D.Xn[i] = v; }
    if (D.fX) D.fX[i] = v;
  }
  for (int j = t; j < nq; j += ET) {
    const size_t i = (size_t)r * nq + j;
    double v = D.Qn[i];
    if (!ok) { v = D.Qo[i]; D.Qn[i] = v; }
    if (D.fQ) D.fQ[i] = v;
  }
  if (D.Fo)
    for (int j = t; j < nf; j += ET) {
      const size_t i = (size_t)r * nf + j;
      double v = D.F_last[i];
      if (ok) { v = D.Fo[i]; D.F_last[i] = v; D.F_sum[i] += v; }
      if (D.fF) D.fF[i] = v;
    }
}

// ---- a run with hard joints (rbl_ensemble_run_jointed): ens_run's loop with the jointed step, and the joints' own launch ----
// What moves during such a run besides the configurations lives on the device: the angles and rates in the joint table
// (RblEnsJoints::theta / rate, which the solver and k_ens_jt_geom read per replica), every replica's position in the motor
// schedule, the sums and the last accepted value of phi.

// what k_ens_jt_run reads and writes (device pointers; the frame slots are NULL in a step that records none)
struct EnsJtRunDev {
  const EnsRunStatus *st; const unsigned *vflag;   // the run's status and this step's verdicts, as k_ens_commit read them
  double *theta, *rate;                            // the joint table's [R n_joints] arrays
  const double *x; long nsys, off;                 // this step's solutions: phi of replica r at x + r nsys + off
  const int *pos_in; int *pos_out;                 // cycle positions [R], read and written: two buffers, since a replica's threads
                                                   // may sit in two workgroups and nobody waits for anybody
  const int *cum; const double *rates;             // the schedule: prefix sums (n_phases + 1), rates [n_phases rate_sets n_joints]
  int n_phases, rate_sets;
  double dt;
  double *phi_sum, *phi_last;                      // [R 3 n_joints]
  double *fT, *fP;                                 // the frame's theta [R n_joints] and phi [R 3 n_joints]
};

// the scheduled rate of joint j of replica r at cycle position p
__device__ __forceinline__ double ens_jt_sched_rate(const int *cum, const double *rates, int n_phases, int rate_sets, int nj, int r, int j,
                                                    int p)
{
  const int k = rbl_schedule_phase(cum, n_phases, p);
  return rates[((size_t)k * rate_sets + (rate_sets == 1 ? 0 : r)) * nj + j];
}

// One thread per replica and joint, after k_ens_commit (st->stopped and vflag are final for this step): where the replica
// committed, theta += rate dt with the product and the sum rounded one after the other and only where rate != 0 -- the statements
// of the one-step call's host loop, so its bits --, the cycle position moves on by one and the step's phi is kept and added to
// phi_sum (every entry by one thread, in step order).  Then, committed or not, the rates of the replica's next step go into the
// table, and the frame is written: the angles as they stand, the last accepted phi
__global__ __launch_bounds__(64) void k_ens_jt_run(int R, int nj, EnsJtRunDev D)
{
  const long g = (long)blockIdx.x * 64 + threadIdx.x;
  if (g >= (long)R * nj) return;
  const int r = (int)(g / nj), j = (int)(g - (long)r * nj);
  const bool ok = D.st->stopped == 0 && D.vflag[r] == 0;
  const size_t e = 3 * (size_t)g;
  int p = D.n_phases ? D.pos_in[r] : 0;
  double th = D.theta[g], ph[3] = {D.phi_last[e], D.phi_last[e + 1], D.phi_last[e + 2]};
  if (ok) {
    const double rate = D.rate[g];
    if (rate != 0.0) {
#pragma clang fp contract(off)
      const double d = rate * D.dt;
      th = th + d;
      D.theta[g] = th;
    }
    if (D.n_phases) p = rbl_schedule_next(D.cum, D.n_phases, p);
    const double *phi = D.x + (size_t)r * D.nsys + D.off + 3 * j;
    for (int q = 0; q < 3; ++q) {
      ph[q] = phi[q];
      D.phi_last[e + q] = ph[q];
      D.phi_sum[e + q] += ph[q];
    }
  }
  if (D.n_phases) {
    D.rate[g] = ens_jt_sched_rate(D.cum, D.rates, D.n_phases, D.rate_sets, nj, r, j, p);
    if (j == 0) D.pos_out[r] = p;
  }
  if (D.fT) {
    D.fT[g] = th;
    for (int q = 0; q < 3; ++q) D.fP[e + q] = ph[q];
  }
}

// before the first step: the rates of every replica's starting position into the table
__global__ __launch_bounds__(64) void k_ens_jt_rates(int R, int nj, const int *__restrict__ pos, const int *__restrict__ cum,
                                                     const double *__restrict__ rates, int n_phases, int rate_sets, double *__restrict__ rate)
{
  const long g = (long)blockIdx.x * 64 + threadIdx.x;
  if (g >= (long)R * nj) return;
  const int r = (int)(g / nj), j = (int)(g - (long)r * nj);
  rate[g] = ens_jt_sched_rate(cum, rates, n_phases, rate_sets, nj, r, j, pos[r]);
}

struct EnsJtRun {
  const rbl_run_joint_opts *o; rbl_run_joint_out *out;
  std::vector<int> cum, start;                     // host: the prefix sums (n_phases + 1, or empty), the starting positions [R]
  EnsJtStep step;                                  // the jointed variant of every step: the joint table, -gamma / dt
  const double *x;                                 // the solutions of a step (EnsWork::x)
  const EnsRunStatus *st; const unsigned *vflag;
  int *pos[2]; int cur;                            // device: positions, which of the two is current
  int *cum_d; double *rates_d, *phi_sum, *phi_last, *lev, *fT, *fP, *fG;
};

size_t ens_jt_run_carve(EnsJtRun &J, void *base, int R, int nj, size_t n_frames)
{
  const size_t Rn = (size_t)R * nj, np = (size_t)J.o->n_phases;
  RblCarve C{(char *)base};
  J.pos[0] = C.take<int>(R); J.pos[1] = C.take<int>(R);
  J.cum_d = C.take<int>(np + 1);
  J.rates_d = C.take<double>(np * (size_t)J.o->rate_sets * nj);
  J.phi_sum = C.take<double>(6 * Rn);              // phi_sum | phi_last, cleared in one piece
  J.phi_last = J.phi_sum ? J.phi_sum + 3 * Rn : nullptr;
  J.lev = C.take<double>(6 * Rn);
  J.fT = C.take<double>(n_frames * Rn); J.fP = C.take<double>(n_frames * 3 * Rn); J.fG = C.take<double>(n_frames * 3 * Rn);
  return C.off;
}

// the joint table (with the stored angles and rates), joint_velocity and the schedule go up, once; the first step's rates are
// written.  From here on the device table is ahead of the host's copy: it is marked stale whatever follows.  st, vflag: the run's
// status and verdict words
int ens_jt_run_begin(rbl_ctx *c, EnsJtRun &J, void *base, size_t n_frames, const EnsWork &w, const EnsRunStatus *st, const unsigned *vflag)
{
  const int R = c->ens_R, nj = c->jt_n, np = J.o->n_phases;
  const size_t Rn = (size_t)R * nj;
  int rc;
  if ((rc = ens_jt_upload(c, &J.step.T))) return rc;
  ens_jt_run_carve(J, base, R, nj, n_frames);
  J.st = st; J.vflag = vflag; J.x = w.x; J.cur = 0;
  c->ens_jt_valid = false; c->ens_jt_phi_valid = false;
  if (J.o->joint_velocity && (rc = copy_h2d(c, w.jr, J.o->joint_velocity, sizeof(double) * 3 * Rn))) return rc;
  RBL_HIP(c, hipMemsetAsync(J.phi_sum, 0, sizeof(double) * 6 * Rn, c->stream));
  if (np) {
    if ((rc = copy_h2d(c, J.cum_d, J.cum.data(), sizeof(int) * ((size_t)np + 1)))) return rc;
    if ((rc = copy_h2d(c, J.rates_d, J.o->phase_rates, sizeof(double) * (size_t)np * J.o->rate_sets * nj))) return rc;
    if ((rc = copy_h2d(c, J.pos[0], J.start.data(), sizeof(int) * (size_t)R))) return rc;
    hipLaunchKernelGGL(k_ens_jt_rates, dim3((unsigned)((Rn + 63) / 64)), dim3(64), 0, c->stream, R, nj, (const int *)J.pos[0],
                       (const int *)J.cum_d, (const double *)J.rates_d, np, (int)J.o->rate_sets, (double *)J.step.T.rate);
  }
  return RBL_OK;
}

// after the step's commit and the host's flip: the joints' launch and, in a recording step (frame >= 0), the gaps at the committed
// configuration and angles by k_ens_jt_geom itself
void ens_jt_run_after(rbl_ctx *c, EnsJtRun &J, long frame)
{
  const int R = c->ens_R, Nb = c->ens_Nb, nj = c->jt_n, np = J.o->n_phases;
  const size_t Rn = (size_t)R * nj, n3 = (size_t)3 * Nb * c->S.N_blb, nb6 = (size_t)6 * Nb;
  EnsJtRunDev D;
  D.st = J.st; D.vflag = J.vflag;
  D.theta = (double *)J.step.T.theta; D.rate = (double *)J.step.T.rate;
  D.x = J.x; D.nsys = (long)(n3 + nb6 + 3 * (size_t)nj); D.off = (long)(n3 + nb6);
  D.pos_in = J.pos[J.cur]; D.pos_out = J.pos[J.cur ^ 1];
  D.cum = J.cum_d; D.rates = J.rates_d; D.n_phases = np; D.rate_sets = J.o->rate_sets;
  D.dt = c->S.dt;
  D.phi_sum = J.phi_sum; D.phi_last = J.phi_last;
  D.fT = D.fP = nullptr;
  if (frame >= 0) { D.fT = J.fT + (size_t)frame * Rn; D.fP = J.fP + (size_t)frame * 3 * Rn; }
  hipLaunchKernelGGL(k_ens_jt_run, dim3((unsigned)((Rn + 63) / 64)), dim3(64), 0, c->stream, R, nj, D);
  if (np) J.cur ^= 1;
  if (frame >= 0)
    rbl_launch_ens_jt_geom(c->stream, ens_X(c, c->ens_cur), ens_Q(c, c->ens_cur), Nb, R, J.step.T, J.lev, J.fG + (size_t)frame * 3 * Rn);
}

// the joints' share of the read-back: the angles become the ensemble's, the last accepted phi the one rbl_ensemble_joint_state
// returns (not after a stop: that phi is invalid, as after a failed step); nfr: the frames of the steps that were enqueued
int ens_jt_run_end(rbl_ctx *c, EnsJtRun &J, size_t nfr, bool stopped)
{
  const int R = c->ens_R, nj = c->jt_n;
  const size_t Rn = (size_t)R * nj;
  rbl_run_joint_out *out = J.out;
  int rc;
  c->ens_jt_phi.resize(3 * Rn);
  if ((rc = copy_d2h(c, c->ens_jt_theta.data(), J.step.T.theta, sizeof(double) * Rn))) return rc;
  if ((rc = copy_d2h(c, c->ens_jt_phi.data(), J.phi_last, sizeof(double) * 3 * Rn))) return rc;
  if (out->phi_sum && (rc = copy_d2h(c, out->phi_sum, J.phi_sum, sizeof(double) * 3 * Rn))) return rc;
  if (out->cycle_pos) {
    if (!J.o->n_phases) std::memset(out->cycle_pos, 0, sizeof(int32_t) * (size_t)R);
    else if ((rc = copy_d2h(c, out->cycle_pos, J.pos[J.cur], sizeof(int32_t) * (size_t)R))) return rc;
  }
  if (nfr) {
    if (out->frame_theta && (rc = copy_d2h(c, out->frame_theta, J.fT, sizeof(double) * nfr * Rn))) return rc;
    if (out->frame_phi && (rc = copy_d2h(c, out->frame_phi, J.fP, sizeof(double) * nfr * 3 * Rn))) return rc;
    if (out->frame_gap && (rc = copy_d2h(c, out->frame_gap, J.fG, sizeof(double) * nfr * 3 * Rn))) return rc;
  }
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  if (out->theta) std::memcpy(out->theta, c->ens_jt_theta.data(), sizeof(double) * Rn);
  c->ens_jt_phi_valid = !stopped;
  return RBL_OK;
}

// the run's own device buffer: [slip copy] | read-back block (status, counters, sums) | verdict words, last loads | frames; the
// active parts follow it (observers, then the joints or the drive)
struct EnsRunBuf {
  double *slip;
  EnsRunStatus *st; int *accepted, *rejected; unsigned *first_flags; long long *iters_sum; double *resid_max, *F_sum;
  size_t rb_off, rb_bytes;                 // the read-back block: from st to the end of F_sum
  unsigned *vflag; double *F_last;
  double *fX, *fQ; int *fA; double *fF;
};

EnsRunBuf ens_run_carve(void *base, int R, int Nb, int nbl, bool slip, bool mixed, size_t n_frames, size_t *bytes)
{
  const size_t Rz = (size_t)R, nb6 = 6 * (size_t)Nb, n3 = (size_t)3 * Nb * nbl;
  RblCarve C{(char *)base};
  EnsRunBuf b;
  b.slip = C.take<double>(slip ? Rz * n3 : 0);
  b.rb_off = C.off;
  b.st = C.take<EnsRunStatus>(1);
  b.accepted = C.take<int>(Rz); b.rejected = C.take<int>(Rz); b.first_flags = C.take<unsigned>(Rz);
  b.iters_sum = C.take<long long>(Rz); b.resid_max = C.take<double>(Rz);
  b.F_sum = C.take<double>(mixed ? Rz * nb6 : 0);
  b.rb_bytes = C.off - b.rb_off;
  b.vflag = C.take<unsigned>(Rz);
  b.F_last = C.take<double>(mixed ? Rz * nb6 : 0);
  b.fX = C.take<double>(n_frames * Rz * 3 * Nb); b.fQ = C.take<double>(n_frames * Rz * 4 * Nb);
  b.fA = C.take<int>(n_frames * Rz);
  b.fF = C.take<double>(mixed ? n_frames * Rz * nb6 : 0);
  *bytes = C.off;
  return b;
}

// What the checks made of a request: how every step is taken, and the parts that are active.  per: the mask's entries per body
struct EnsRunPlan {
  int per = 1;
  bool brownian = false, masked = false;
  size_t n_frames = 0;
  bool joints = false, observers = false, drive = false;
  bool joints_off = false;                 // a jointed request with the joints off or never set: jout->cycle_pos is zeroed afterwards
  bool drive_empty = false;                // a drive that drives nothing, with a dout: t_end and cycle_pos from the accepted counts
  EnsJtRun J = {};
  RblEnsObsRun O;
  RblEnsDriveRun D;
};

// n_steps steps of every replica (checks and ens_ready done by ens_run_request): the inputs go up once, every step is the one-step
// calls' enqueue sequence followed by the verdict and the commit, the buffers flip on the host, ONE read-back ends it
int ens_run(rbl_ctx *c, const rbl_run_opts &o, EnsRunPlan &P, rbl_run_out *out)
{
  const RblBodyState &S = c->S;
  const bool mixed = P.masked, reject = o.on_error == RBL_RUN_REJECT;
  const int R = c->ens_R, Nb = c->ens_Nb, nbl = S.N_blb;
  const size_t Rz = (size_t)R, nb6 = 6 * (size_t)Nb, n3 = (size_t)3 * Nb * nbl;
  int rc;
  EnsWork w;
  if ((rc = ens_work(c, o.max_iter, &w))) return rc;
  size_t at_obs = 0;
  ens_run_carve(nullptr, R, Nb, nbl, o.slip != nullptr, mixed, P.n_frames, &at_obs);
  // the parts behind: the observers, then the joints' or the drive's (never both: a drive with joints on is refused)
  const size_t at_part = at_obs + (P.observers ? ens_obs_carve(P.O, nullptr, R, Nb, P.n_frames) : 0);
  if ((rc = rbl_dev_reserve(c, c->d_ens_run, at_part + (P.joints  ? ens_jt_run_carve(P.J, nullptr, R, c->jt_n, P.n_frames)
                                                        : P.drive ? ens_drive_carve(P.D, nullptr, R, Nb) : 0))))
    return rc;
  char *base = (char *)c->d_ens_run.p;
  const EnsRunBuf b = ens_run_carve(base, R, Nb, nbl, o.slip != nullptr, mixed, P.n_frames, &at_obs);
  // the uploads, once
  if (mixed && (rc = ens_upload_mask(c, w, o.prescribed, P.per))) return rc;
  // (a driven run: the body input goes into the drive's own buffer, and k_ens_drive writes w.F before every step)
  if (P.drive) { if ((rc = ens_drive_begin(c, P.D, base + at_part, R, Nb, mixed ? o.body_in : o.F_body))) return rc; }
  else if ((rc = copy_h2d(c, w.F, mixed ? o.body_in : o.F_body, sizeof(double) * nb6 * Rz))) return rc;
  if (o.slip && (rc = copy_h2d(c, b.slip, o.slip, sizeof(double) * n3 * Rz))) return rc;
  RBL_HIP(c, hipMemsetAsync(b.st, 0, b.rb_bytes, c->stream));
  if (mixed) RBL_HIP(c, hipMemsetAsync(b.F_last, 0, sizeof(double) * nb6 * Rz, c->stream));
  if (P.joints && (rc = ens_jt_run_begin(c, P.J, base + at_part, P.n_frames, w, b.st, b.vflag))) return rc;
  if (P.observers && (rc = ens_obs_begin(c, P.O, base + at_obs, R, Nb, P.n_frames))) return rc;
  EnsStepIn in;
  in.obs = P.observers ? &P.O.step : nullptr;
  in.prescribed = o.prescribed; in.per = P.per;
  in.slip = o.slip ? b.slip : nullptr; in.resident = true; in.chol_err = 1;
  in.accepted = b.accepted;
  EnsRunStatus hs = {0, 0, 0u, 0};
  int enq = 0;
  const auto verdict = S.wall ? k_ens_verdict<true> : k_ens_verdict<false>;
  for (int n = 0; n < o.n_steps; ++n) {
    if (P.drive) ens_drive_step(c, P.D, R, Nb, b.accepted, w.F);   // the step's body input, from the replicas' clocks and cycle positions
    rc = P.brownian ? ens_enqueue_bd(c, w, in, o.seed + (uint64_t)n, o.split_rand, o.delta, o.max_iter, o.rtol)
                    : ens_enqueue_det(c, w, in, o.max_iter, o.rtol, true, P.joints ? &P.J.step : nullptr);
    if (rc) return rc;
    const int cur = c->ens_cur;
    hipLaunchKernelGGL(verdict, dim3((unsigned)R), dim3(ET), 0, c->stream, Nb, nbl, n, reject ? 1 : 0,
                       (const double *)ens_X(c, cur ^ 1), (const double *)ens_Q(c, cur ^ 1), (const double *)ens_cfg(c),
                       (const unsigned *)w.rerr, (const unsigned *)w.gerr, b.vflag, b.st);
    const long frame = o.stride > 0 && (n + 1) % o.stride == 0 ? (long)((n + 1) / o.stride - 1) : -1L;   // the frame this step records
    EnsRunDev D;
    D.Xo = ens_X(c, cur); D.Qo = ens_Q(c, cur); D.Xn = ens_X(c, cur ^ 1); D.Qn = ens_Q(c, cur ^ 1);
    D.vflag = b.vflag; D.gerr = w.gerr; D.iters = w.iters; D.resid = w.resid; D.Fo = mixed ? w.Fo : nullptr; D.st = b.st;
    D.accepted = b.accepted; D.rejected = b.rejected; D.first_flags = b.first_flags; D.iters_sum = b.iters_sum;
    D.resid_max = b.resid_max; D.F_sum = b.F_sum; D.F_last = b.F_last;
    D.fX = D.fQ = D.fF = nullptr; D.fA = nullptr;
    if (frame >= 0) {
      const size_t k = (size_t)frame;
      D.fX = b.fX + k * Rz * 3 * Nb; D.fQ = b.fQ + k * Rz * 4 * Nb; D.fA = b.fA + k * Rz;
      if (mixed) D.fF = b.fF + k * Rz * nb6;
    }
    hipLaunchKernelGGL(k_ens_commit, dim3((unsigned)R), dim3(ET), 0, c->stream, R, Nb, n, D);
    // the parts follow the commit's decision, replica by replica: the observers, the drive (q^n, the U the update read) ...
    if (P.observers) ens_obs_after(c, P.O, R, &b.st->stopped, b.vflag, frame);
    if (P.drive)
      ens_drive_after(c, P.D, R, Nb, &b.st->stopped, b.vflag, b.accepted, D.Xo, mixed ? (const double *)w.U : (const double *)w.x + n3,
                      mixed ? (long)nb6 : (long)(n3 + nb6), D.Fo);
    c->ens_cur ^= 1;                                     // the new buffer holds every replica's configuration, moved or not
    if (P.joints) ens_jt_run_after(c, P.J, frame);       // ... and the joints, at the committed configuration
    ++enq;
    if (o.check_every > 0 && enq % o.check_every == 0 && n + 1 < o.n_steps) {
      if ((rc = read_back(c, &hs, b.st, sizeof(hs)))) return rc;
      if (hs.stopped) break;
    }
  }
  RBL_HIP(c, hipGetLastError());
  // the one read-back: status, counters, sums; then the frames the run completed, straight into the caller's arrays
  std::vector<char> h(b.rb_bytes);
  if ((rc = copy_d2h(c, h.data(), b.st, b.rb_bytes))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));
  auto at = [&](const void *p) { return h.data() + ((const char *)p - (const char *)b.st); };
  std::memcpy(&hs, at(b.st), sizeof(hs));
  const int *hacc = (const int *)at(b.accepted), *hrej = (const int *)at(b.rejected);
  const unsigned *hff = (const unsigned *)at(b.first_flags);
  if (out->accepted) std::memcpy(out->accepted, hacc, sizeof(int) * Rz);
  if (out->rejected) std::memcpy(out->rejected, hrej, sizeof(int) * Rz);
  if (out->first_flags) std::memcpy(out->first_flags, hff, sizeof(unsigned) * Rz);
  if (out->first_status)
    for (int r = 0; r < R; ++r) out->first_status[r] = hrej[r] ? rbl_flags_to_status(c, hff[r]) : RBL_OK;
  if (out->iters_sum) std::memcpy(out->iters_sum, at(b.iters_sum), sizeof(int64_t) * Rz);
  if (out->resid_max) std::memcpy(out->resid_max, at(b.resid_max), sizeof(double) * Rz);
  if (mixed && out->F_sum) std::memcpy(out->F_sum, at(b.F_sum), sizeof(double) * nb6 * Rz);
  const size_t nfr = o.stride > 0 ? (size_t)(enq / o.stride) : 0;   // frames of the steps that were enqueued (a polled stop: fewer)
  if (nfr) {
    if ((rc = copy_d2h(c, out->frame_X, b.fX, sizeof(double) * nfr * Rz * 3 * Nb))) return rc;
    if ((rc = copy_d2h(c, out->frame_Q, b.fQ, sizeof(double) * nfr * Rz * 4 * Nb))) return rc;
    if ((rc = copy_d2h(c, out->frame_accepted_at, b.fA, sizeof(int) * nfr * Rz))) return rc;
    if (mixed && (rc = copy_d2h(c, out->frame_F, b.fF, sizeof(double) * nfr * Rz * nb6))) return rc;
    RBL_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (P.observers && (rc = ens_obs_end(c, P.O, nfr))) return rc;
  if (P.joints && (rc = ens_jt_run_end(c, P.J, nfr, hs.stopped != 0))) return rc;
  if (P.drive && (rc = ens_drive_end(c, P.D, R, Nb))) return rc;
  if (P.drive_empty) ens_drive_empty_out(c, P.D, R, hacc);
  out->stopped_at = hs.stopped ? hs.stopped - 1 : -1;
  out->steps_done = hs.stopped ? hs.stopped - 1 : o.n_steps;
  out->stop_replica = hs.stopped && hs.stop_rep ? R - hs.stop_rep : -1;
  if (!hs.stopped) return RBL_OK;
  const std::string at_step = "ensemble_run step " + std::to_string(hs.stopped - 1);
  if (hs.stop_rep) {
    rc = rbl_flags_to_status(c, hff[R - hs.stop_rep]);
    c->last_error = at_step + ", replica " + std::to_string(R - hs.stop_rep) + ": " + c->last_error;
  } else {
    rc = rbl_flags_to_status(c, hs.batch);
    c->last_error = at_step + ": " + c->last_error;
  }
  return rc;
}

// the schedule's own refusals (include/rbl.h section 5), none needing a device; fills J.cum and J.start
int ens_jt_schedule_check(rbl_ctx *c, const char *who, const rbl_run_joint_opts &jo, EnsJtRun &J)
{
  const std::string w(who);
  const int R = c->ens_R, nj = c->jt_n;
  if (jo.n_phases < 0) return rbl_fail(c, RBL_ERR_ARG, w + ": n_phases must be >= 0");
  if (jo.start_sets != 0 && jo.start_sets != 1 && jo.start_sets != R)
    return rbl_fail(c, RBL_ERR_ARG, w + ": start_sets must be 0, 1 or R = " + std::to_string(R));
  if (jo.start_sets && !jo.cycle_start) return rbl_fail(c, RBL_ERR_ARG, w + ": cycle_start is NULL while start_sets > 0");
  J.cum.clear();
  long long len = 0;
  if (jo.n_phases) {
    if (!ens_jt_active(c))
      return rbl_fail(c, RBL_ERR_STATE, w + ": a motor schedule was given, but the joints are switched off or were never set (rbl_set_joint_kinds)");
    if (!jo.phase_steps || !jo.phase_rates) return rbl_fail(c, RBL_ERR_ARG, w + ": phase_steps or phase_rates is NULL while n_phases > 0");
    if (jo.rate_sets != 1 && jo.rate_sets != R) return rbl_fail(c, RBL_ERR_ARG, w + ": rate_sets must be 1 or R = " + std::to_string(R));
    J.cum.push_back(0);
    for (int k = 0; k < jo.n_phases; ++k) {
      if (jo.phase_steps[k] < 1)
        return rbl_fail(c, RBL_ERR_ARG, w + ": phase_steps[" + std::to_string(k) + "] = " + std::to_string(jo.phase_steps[k]) + ": every phase lasts at least one step");
      len += jo.phase_steps[k];
      if (len > 0x7fffffffLL) return rbl_fail(c, RBL_ERR_ARG, w + ": the cycle's length (the sum of phase_steps) must fit 31 bits");
      J.cum.push_back((int)len);
    }
    for (int k = 0; k < jo.n_phases; ++k)
      for (int s = 0; s < jo.rate_sets; ++s)
        for (int j = 0; j < nj; ++j) {
          const double x = jo.phase_rates[((size_t)k * jo.rate_sets + s) * nj + j];
          const std::string at = w + ": phase " + std::to_string(k) + ", set " + std::to_string(s) + ", joint " + std::to_string(j) + ": ";
          if (!std::isfinite(x)) return rbl_fail(c, RBL_ERR_ARG, at + "the value must be finite");
          if (x != 0.0 && c->jt_kind[j] != RBL_JOINT_LOCK)
            return rbl_fail(c, RBL_ERR_ARG, at + "only a lock joint (RBL_JOINT_LOCK) takes a rate; it must be 0 here");
        }
  }
  J.start.assign((size_t)R, 0);
  for (int s = 0; s < jo.start_sets; ++s) {
    const long long p = jo.cycle_start[s];
    if (p < 0 || p >= std::max(len, 1LL))
      return rbl_fail(c, RBL_ERR_ARG, w + ": cycle_start[" + std::to_string(s) + "] = " + std::to_string(p) + " lies outside the cycle, 0 <= value < " +
                                          std::to_string(std::max(len, 1LL)) + (len ? "" : " (no schedule: only 0)"));
    if (jo.start_sets == 1) J.start.assign((size_t)R, (int)p);
    else J.start[(size_t)s] = (int)p;
  }
  return RBL_OK;
}

// the observers' own refusals, none needing a device.  They come before the run's: o has not been checked yet, and all that is
// read of it (guarded) is whether it records frames
int ens_obs_check(rbl_ctx *c, const rbl_run_opts *o, const rbl_run_obs_opts *obs, const rbl_run_obs_out *oout)
{
  const char *who = "ensemble_run_observed";
  const std::string w(who);
  if (!obs || !oout) return rbl_fail(c, RBL_ERR_ARG, w + ": obs or oout is NULL");
  if (obs->size != (int64_t)sizeof(rbl_run_obs_opts)) return rbl_fail(c, RBL_ERR_ARG, w + ": obs.size is not sizeof(rbl_run_obs_opts)");
  if (oout->size != (int64_t)sizeof(rbl_run_obs_out)) return rbl_fail(c, RBL_ERR_ARG, w + ": oout.size is not sizeof(rbl_run_obs_out)");
  if (obs->n_probes < 0) return rbl_fail(c, RBL_ERR_ARG, w + ": n_probes must be >= 0");
  if (obs->n_probes > 0) {
    if (!obs->points) return rbl_fail(c, RBL_ERR_ARG, w + ": points is NULL while n_probes > 0");
    if (obs->point_sets < 1) return rbl_fail(c, RBL_ERR_ARG, w + ": point_sets must be 1 or R");
    if (obs->probe_body < -1) return rbl_fail(c, RBL_ERR_ARG, w + ": probe_body must be -1 (lab points) or a body index");
    if (c->ens_R) {                                      // (no ensemble: the run's RBL_ERR_STATE, later)
      if (obs->point_sets != 1 && obs->point_sets != c->ens_R)
        return rbl_fail(c, RBL_ERR_ARG, w + ": point_sets must be 1 or R = " + std::to_string(c->ens_R));
      if (obs->probe_body >= c->ens_Nb)
        return rbl_fail(c, RBL_ERR_ARG, w + ": probe_body must be -1 (lab points) or a body index below N_bod = " + std::to_string(c->ens_Nb));
    }
    if (c->ens_R || obs->point_sets == 1) {              // (the sets are R sets or one: the array's length is known)
      int rc = ens_points_check(c, who, obs->points, obs->n_probes, obs->point_sets); if (rc) return rc;
    }
  }
  const bool frames = o && o->size == (int64_t)sizeof(rbl_run_opts) && o->stride > 0 && o->n_steps / o->stride > 0;
  if (frames && obs->n_probes > 0 && !oout->frame_u) return rbl_fail(c, RBL_ERR_ARG, w + ": frame_u must not be NULL while stride > 0 records frames of the probes");
  if (frames && obs->moments && !oout->frame_D) return rbl_fail(c, RBL_ERR_ARG, w + ": frame_D must not be NULL while stride > 0 records frames of the moments");
  return RBL_OK;
}

// One request: a run's options and outputs, the optional pairs (NULL: not given), the exported call it came from
enum EnsRunEntry { ENS_RUN, ENS_RUN_JOINTED, ENS_RUN_OBSERVED, ENS_RUN_DRIVEN };
struct EnsRunReq {
  const rbl_run_opts *o; rbl_run_out *out;
  const rbl_run_joint_opts *jo; rbl_run_joint_out *jout;
  const rbl_run_obs_opts *obs; rbl_run_obs_out *oout;
  const rbl_run_drive_opts *drive; rbl_run_drive_out *dout;
  EnsRunEntry entry;
};

// Every check of a run, then the run: the drive's own refusals (ens_drive_check), the observers' own, then the run's -- in the jointed
// flavour (rbl_ensemble_step_jointed's checks, the schedule's) for rbl_ensemble_run_jointed and for an observed run that brings jopts, in
// the plain one otherwise; the flavour's name leads the messages of the checks both have.  None needs a device before ens_ready
int ens_run_request(rbl_ctx *c, const EnsRunReq &q)
{
  if (!c) return RBL_ERR_ARG;
  const rbl_run_opts *o = q.o;
  rbl_run_out *out = q.out;
  EnsRunPlan P;
  int rc;
  if (q.entry == ENS_RUN_DRIVEN) {
    const std::string w("ensemble_run_driven");
    bool empty = true;
    if (q.dout && q.dout->size != (int64_t)sizeof(rbl_run_drive_out)) return rbl_fail(c, RBL_ERR_ARG, w + ": dout.size is not sizeof(rbl_run_drive_out)");
    if (q.drive) {
      if ((rc = ens_drive_check(c, "ensemble_run_driven", q.drive, c->ens_R, c->ens_Nb, &empty, &P.D))) return rc;
      if (!empty && !q.dout) return rbl_fail(c, RBL_ERR_ARG, w + ": dout is NULL while a drive is given");
      if (!empty && ens_jt_active(c))
        return rbl_fail(c, RBL_ERR_STATE, w + ": hard joints are switched on: a drive together with joints is not offered (run_jointed takes no "
                                              "drive; switch the joints off, or run without a drive)");
    }
    P.D.out = q.dout;
    P.drive = !empty;
    P.drive_empty = q.drive && empty && q.dout;          // nothing drives: the underlying run itself, whose accepted counts give t_end
  }
  if (q.entry == ENS_RUN_OBSERVED || (q.entry == ENS_RUN_DRIVEN && q.obs)) {
    if ((rc = ens_obs_check(c, o, q.obs, q.oout))) return rc;
    P.observers = q.obs->n_probes > 0 || q.obs->moments;   // (nothing asked for: the underlying run)
    P.O.o = q.obs; P.O.out = q.oout;
  }
  const bool jointed = q.entry == ENS_RUN_JOINTED || (q.entry == ENS_RUN_OBSERVED && q.jo);
  const char *who = jointed ? "ensemble_run_jointed" : "ensemble_run";
  const std::string w(who);
  if (jointed ? (!o || !q.jo || !out || !q.jout) : (!o || !out))
    return rbl_fail(c, RBL_ERR_ARG, w + (jointed ? ": opts, jopts, out or jout is NULL" : ": opts or out is NULL"));
  if (o->size != (int64_t)sizeof(rbl_run_opts)) return rbl_fail(c, RBL_ERR_ARG, w + ": opts.size is not sizeof(rbl_run_opts)");
  if (jointed && q.jo->size != (int64_t)sizeof(rbl_run_joint_opts)) return rbl_fail(c, RBL_ERR_ARG, w + ": jopts.size is not sizeof(rbl_run_joint_opts)");
  if (out->size != (int64_t)sizeof(rbl_run_out)) return rbl_fail(c, RBL_ERR_ARG, w + ": out.size is not sizeof(rbl_run_out)");
  if (jointed && q.jout->size != (int64_t)sizeof(rbl_run_joint_out)) return rbl_fail(c, RBL_ERR_ARG, w + ": jout.size is not sizeof(rbl_run_joint_out)");
  out->steps_done = 0; out->stopped_at = -1; out->stop_replica = -1; out->reserved = 0;   // what a refused call leaves
  if (periodic_on(c)) return periodic_refuse(c, who);
  if (jointed && ens_cell_on(c)) return ens_cell_refuse(c, who);
  if (o->n_steps < 1) return rbl_fail(c, RBL_ERR_ARG, w + ": n_steps must be >= 1");
  if (o->stride < 0) return rbl_fail(c, RBL_ERR_ARG, w + ": stride must be >= 0");
  if (o->check_every < 0) return rbl_fail(c, RBL_ERR_ARG, w + ": check_every must be >= 0");
  if (o->on_error != RBL_RUN_STOP && o->on_error != RBL_RUN_REJECT)
    return rbl_fail(c, RBL_ERR_ARG, w + ": on_error must be RBL_RUN_STOP (0) or RBL_RUN_REJECT (1)");
  P.n_frames = o->stride > 0 ? (size_t)(o->n_steps / o->stride) : 0;
  const bool no_frames = P.n_frames && (!out->frame_X || !out->frame_Q || !out->frame_accepted_at);
  if (!jointed) {
    if (o->prescribed_per != 0 && o->prescribed_per != 1 && o->prescribed_per != 6)
      return rbl_fail(c, RBL_ERR_ARG, w + ": prescribed_per must be 0 or 1 (a mask entry per body) or 6 (one per velocity component)");
    P.per = o->prescribed_per == 6 ? 6 : 1;
    const bool free_run = o->F_body != nullptr;
    P.masked = o->prescribed || o->body_in;
    if (free_run == P.masked)
      return rbl_fail(c, RBL_ERR_ARG, w + ": give either F_body or prescribed with body_in (both or neither were given)");
    if (P.masked && P.per == 6 && o->brownian && c->S.kBT > 1e-10)   // kBT <= 1e-10 runs the deterministic step, as elsewhere
      return rbl_fail(c, RBL_ERR_ARG, w + ": the Brownian step takes whole-body masks only (prescribed_per = 6 with brownian != 0 and "
                                          "kBT > 1e-10): the drift term of a partly prescribed body has not been derived");
    if (o->max_iter < 1) return rbl_fail(c, RBL_ERR_ARG, w + ": max_iter must be >= 1");
    if (!(o->rtol >= 0.0)) return rbl_fail(c, RBL_ERR_ARG, w + ": rtol must be >= 0");
    if (no_frames || (P.n_frames && P.masked && !out->frame_F))
      return rbl_fail(c, RBL_ERR_ARG, w + ": frame_X, frame_Q, frame_accepted_at (and frame_F with prescribed bodies) must not be NULL while stride > 0 records frames");
    if (P.masked) {                                      // NULL halves, max_iter > 255, communicator, state, entries, the LDS
      if ((rc = ens_mx_check(c, who, o->prescribed, o->body_in, o->max_iter, o->rtol, P.per))) return rc;
    } else {
      if ((rc = need_params(c))) return rc;
      if (o->max_iter > 255) return rbl_fail(c, RBL_ERR_SIZE, ens_beyond());
      if ((rc = ens_state_check(c, ""))) return rc;
      if ((rc = ens_check_solver(c, o->max_iter))) return rc;
    }
    P.brownian = o->brownian && c->S.kBT > 1e-10;        // no Brownian terms (:967-970): the deterministic step
    if (P.brownian && (!(c->S.dt > 0.0) || !(o->delta > 0.0))) return rbl_fail(c, RBL_ERR_ARG, w + ": dt and delta must be positive");
    P.D.masked = P.masked;
  } else {                                               // rbl_ensemble_step_jointed's checks, then the schedule's own
    if (o->prescribed || o->body_in)
      return rbl_fail(c, RBL_ERR_ARG, w + ": prescribed and body_in must be NULL: joints together with prescribed masks are not offered");
    if (o->prescribed_per != 0 && o->prescribed_per != 1)
      return rbl_fail(c, RBL_ERR_ARG, w + ": prescribed_per must be 0 or 1: joints together with prescribed masks are not offered");
    if (o->brownian && c->S.kBT > 1e-10)                   // kBT <= 1e-10: brownian is ignored, as in a plain run
      return rbl_fail(c, RBL_ERR_ARG, w + ": brownian != 0 with kBT > 1e-10: Brownian jointed steps are not offered, the drift of a constrained "
                                          "suspension has not been derived");
    if (!(q.jo->gamma >= 0.0 && q.jo->gamma <= 1.0)) return rbl_fail(c, RBL_ERR_ARG, w + ": gamma must lie in [0, 1]");
    P.joints = ens_jt_active(c);
    P.joints_off = !P.joints;                            // joints off or never set: the plain deterministic run
    if (P.joints && !(c->S.dt > 0.0)) return rbl_fail(c, RBL_ERR_ARG, w + ": dt must be positive");
    if ((rc = ens_jt_check(c, who, o->F_body, o->max_iter, o->rtol))) return rc;
    if (no_frames) return rbl_fail(c, RBL_ERR_ARG, w + ": frame_X, frame_Q and frame_accepted_at must not be NULL while stride > 0 records frames");
    P.J.o = q.jo; P.J.out = q.jout;
    if ((rc = ens_jt_schedule_check(c, who, *q.jo, P.J))) return rc;
    if (P.joints_off && (rc = ens_check_solver(c, o->max_iter))) return rc;   // (the plain run's own word on the shape)
    if (P.joints) P.J.step = {who, {}, -q.jo->gamma / c->S.dt, q.jo->joint_velocity != nullptr};
  }
  if ((rc = ens_flow_check(c))) return rc;
  if ((rc = ens_ready(c))) return rc;
  rc = ens_run(c, *o, P, out);
  if (P.joints_off && !(rc && out->stopped_at < 0) && q.jout->cycle_pos) std::memset(q.jout->cycle_pos, 0, sizeof(int32_t) * (size_t)c->ens_R);
  return rc;
}

}  // namespace

// ---- C ABI (include/rbl.h section 5, runs) ------------------------------------------------------------------------------------

int rbl_ensemble_run(rbl_ctx *c, const rbl_run_opts *o, rbl_run_out *out)
{
  return ens_run_request(c, {o, out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ENS_RUN});
}

int rbl_ensemble_run_jointed(rbl_ctx *c, const rbl_run_opts *o, const rbl_run_joint_opts *jo, rbl_run_out *out, rbl_run_joint_out *jout)
{
  return ens_run_request(c, {o, out, jo, jout, nullptr, nullptr, nullptr, nullptr, ENS_RUN_JOINTED});
}

int rbl_ensemble_run_observed(rbl_ctx *c, const rbl_run_opts *o, const rbl_run_joint_opts *jo, const rbl_run_obs_opts *obs, rbl_run_out *out,
                              rbl_run_joint_out *jout, rbl_run_obs_out *oout)
{
  return ens_run_request(c, {o, out, jo, jout, obs, oout, nullptr, nullptr, ENS_RUN_OBSERVED});
}

int rbl_ensemble_run_driven(rbl_ctx *c, const rbl_run_opts *o, const rbl_run_drive_opts *drive, const rbl_run_obs_opts *obs, rbl_run_out *out,
                            rbl_run_drive_out *dout, rbl_run_obs_out *oout)
{
  return ens_run_request(c, {o, out, nullptr, nullptr, obs, oout, drive, dout, ENS_RUN_DRIVEN});
}

int rbl_run_schedule_phase(const int32_t *phase_steps, int n_phases, int64_t pos)
{
  if (!phase_steps || n_phases < 1 || pos < 0) return -1;
  std::vector<int> cum(1, 0);
  for (int k = 0; k < n_phases; ++k) {
    if (phase_steps[k] < 1 || (int64_t)cum.back() + phase_steps[k] > 0x7fffffffLL) return -1;
    cum.push_back(cum.back() + phase_steps[k]);
  }
  return pos < cum.back() ? rbl_schedule_phase(cum.data(), n_phases, (int)pos) : -1;
}
