// rbl_small_joints.hip -- the jointed saddle solve of every replica of an ensemble in ONE kernel launch (include/rbl.h sections 5
// and 9): k_gmres_small_jt<WALL, VLDS>, the one-kernel solver of rbl_small.hip with the hard joints of rbl_joints.hip inside it.
//
//     M lambda - K U            = slip
//     K^T lambda      + J^T phi = -F
//                   J U         = c        (less sigma ah (ah . phi) on an axis joint's rows)
//
// One workgroup per replica.  The body of the solver is rbl_small_solve (rbl_small_solve.hpp) with JOINTS = true: after the
// geometry and the per-body N~^-1 of the diagonal preconditioner one thread per joint makes the joint's geometry
// (jt_geom_joint, rbl_joints_dev.hpp), the workgroup assembles S = J N~^-1 J^T in LDS, factors it, tests the pivots as
// k_jt_pivots does and inverts it; the operator gets J^T phi on the body rows and J U on the joint rows, the preconditioner is the
// exact inverse of the system with M~ for M (rbl_joints.hip's, its second pass collapsed to a 6 x 6 product per body and one blob
// pass), and phi is projected across the axis of every axis joint at the end.  Barriers stand where rbl_joints.hip has launches.
// Every sum has a fixed order, nothing is added atomically in floating point: replica r of R is bitwise the launch of that
// replica alone.  A redundant joint set latches RBL_FLAG_REDUNDANT in the replica's error word (a body's 6 x 6 block that fails its own Cholesky:
// RBL_FLAG_NOT_SPD, as in the unjointed solver).
//
// This kernel lives in a translation unit of its own so that rbl_small.hip keeps exactly its eight instantiations.
#include "rbl_small_solve.hpp"

namespace {

template <bool WALL, bool VLDS>
__global__ __launch_bounds__(SGT) void k_gmres_small_jt(SmallArgsJt A)
{
  rbl_small_solve<WALL, VLDS, false, true>(A);
}

// lever arms and gaps of every replica's joints (rbl_ensemble_joint_state): one lane per joint and replica
__global__ __launch_bounds__(64) void k_ens_jt_geom(const double *__restrict__ X, const double *__restrict__ Q, JtDev J, int N_bod, int reps,
                                                    double *__restrict__ lev, double *__restrict__ gap)
{
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= reps * J.n) return;
  const int r = g / J.n, j = g - r * J.n;
  J.theta += (size_t)r * J.n;
  jt_geom_joint<true>(X + (size_t)r * 3 * N_bod, Q + (size_t)r * 4 * N_bod, J, j, lev + (size_t)r * 6 * J.n, gap + (size_t)r * 3 * J.n, nullptr);
}

JtDev jt_table(const RblEnsJoints &T)
{
  JtDev J = {};
  J.anchor = T.anchor; J.body = T.body; J.rows = nullptr; J.ptr = T.ptr; J.ends = T.ends; J.mate = T.mate;
  J.n = T.n; J.n_rows = 0; J.kind = T.kind; J.ang = T.ang; J.theta = T.theta; J.rate = T.rate; J.ninv = nullptr;
  return J;
}

}  // namespace

// does the one-kernel jointed solver cover this system?  The plain predicate's limits, and the vectors with the joint data
// (small_lds_base_bytes) within SG_LDS_MAX.  n_joints = 0: the plain predicate's answer
bool rbl_gmres_small_jt_fits(int N_blb, int N_bod, int max_iter, int n_joints)
{
  if (n_joints < 0 || !rbl_gmres_small_fits(N_blb, N_bod, max_iter, false)) return false;
  return 3 * (size_t)n_joints <= (size_t)SGT && small_lds_base_bytes(N_blb, N_bod, max_iter, false, n_joints) <= SG_LDS_MAX;
}

size_t rbl_gmres_small_jt_lds_bytes(int N_blb, int N_bod, int max_iter, int n_joints)
{
  return small_lds_base_bytes(N_blb, N_bod, max_iter, false, n_joints);
}

// one workgroup per replica; S.rhs and S.x hold 3 N + 6 N_bod + 3 n_joints doubles per replica, S.work
// rbl_gmres_small_work_doubles(.., n_joints) per replica.  step: the joint rows of S.rhs hold joint_velocity and
// c = coef gap + them (- rate ah on a lock's rows) is formed in the kernel.  The launcher is small_launch (rbl_small_solve.hpp)
int rbl_launch_gmres_small_ens_jt(hipStream_t st, const RblParams &P, bool wall, const RblSmallEns &S, const RblEnsJoints &T, int step,
                                  double coef)
{
  static void (*const tab[2][2])(SmallArgsJt) = {{k_gmres_small_jt<false, false>, k_gmres_small_jt<false, true>},
                                                 {k_gmres_small_jt<true, false>, k_gmres_small_jt<true, true>}};
  SmallArgsJt A = {};
  A.J = jt_table(T); A.n_ends = T.n_ends; A.jstep = step; A.jcoef = coef;
  return small_launch(st, P, S, A, tab[wall], false, T.n);
}

// d_lev: reps x 6 n_joints, d_gap: reps x 3 n_joints
void rbl_launch_ens_jt_geom(hipStream_t st, const double *dX, const double *dQ, int N_bod, int reps, const RblEnsJoints &T, double *d_lev,
                            double *d_gap)
{
  const long tot = (long)reps * T.n;
  hipLaunchKernelGGL(k_ens_jt_geom, dim3((unsigned)((tot + 63) / 64)), dim3(64), 0, st, dX, dQ, jt_table(T), N_bod, reps, d_lev, d_gap);
}
