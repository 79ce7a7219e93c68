// rbl_small.hip -- the whole right-preconditioned GMRES solve of a SMALL system in ONE kernel launch.
//
// moving the Krylov loop onto the device "removes per-iteration latency at small N".  At
// BASELINE cfg 1 (10 x shell_N_12 = 120 blobs, 360 + 60 unknowns) one iteration of rbl_gmres_saddle_dev is ~6 kernel
// launches of a few microseconds each: the solve is launch-bound (1.0 ms for 21 products).  Here one workgroup of
// 1024 threads on one CU does everything between the right-hand side and the solution with workgroup barriers
// instead of kernel boundaries:
//
//   geometry (lever arms, positions: reference :257-265, :374) -> diagonal preconditioner (diag_invM :489-543,
//   Ninv = K^T invM K and its 6x6 Cholesky :593-594) -> [ z = P^-1 v_j  (:589-616) ; w = A z  (src/Rigid.py:73-80:
//   M lambda - K U | K^T lambda, M by ordered pair evaluation with rbl_pair_accum, reference :641-659) ;
//   classical Gram-Schmidt twice ; Givens update and convergence test ]* -> x = P^-1 V y.
//
// Vectors of the iteration, the new Hessenberg column, the Givens rotations and (up to 64 iterations) the triangular
// factor live in LDS; so does the Krylov basis when it fits beside them in the CU's 160 KB (cfg 1: 71 KB for 21 vectors),
// otherwise it goes to a global workspace (L2-resident).  A first version kept basis and Hessenberg matrix in global
// memory: thread 0's Givens recurrence then was a chain of dependent L2 round trips, ~10 us per iteration.
// Every sum has a fixed order: results are bitwise reproducible, like the rest of the library.
// Limits: N <= 256 blobs, N_bod <= 64, diagonal preconditioner, max_iter <= 255, AND the vectors below within SG_LDS_MAX = 150 KB
// (rbl_gmres_small_fits; checked by the launcher).  The LDS bound is the one that binds: the sixteen accumulator sets of the pair
// sweep alone are 384 N bytes, so about 75 N + 60 N_bod doubles in all -- one body of 238 blobs, 49 tetrahedra (196 blobs) or 62
// trimers at max_iter = 255; 64 x 4 and 1 x 256 blobs do NOT fit, and since the triangular factor is kept in LDS up to 64
// iterations the bound is not monotonic in max_iter (64 trimers fit at max_iter <= 38 and at 65 .. 189).
//
// MIXED (the ensembles with prescribed bodies, include/rbl.h sections 5 and 7): the same solve of
//   [M lambda - K (D_f U) ; D_f K^T lambda + D_p U] = [slip + K_p U_p ; -F_f | 0]
// with the replica's 0/1 mask per velocity component (six per body, lab frame; a whole body: none or all six set -- `per` says
// whether the mask holds one entry per body or six, and is read once, where the flags are filled).  ONE launch assembles the right-hand side, solves and splits: it takes the all-free
// right-hand side [slip ; -body_in], adds K (D_p U_in) with the lever arms it has just made and zeroes the bottom of the prescribed
// components (k_mx_rhs of rbl_mixed.hip); the operator and the preconditioner treat a prescribed slot as k_mx_op_tail /
// k_mx_pc_diag do, by selects on values outside the pair sweep, the 6 x 6 block of a partly prescribed body being factored with
// the identity's rows and columns on its prescribed components (k_mx_factors); the end is k_mx_split's: U, F per component, the
// K^T sums in blob order.  A free body's arithmetic and its order are those of the unmasked kernel, so with nobody prescribed the
// solution and the iteration count are bitwise the unmasked ones.  The four unmasked instantiations keep their code (every
// masked statement is behind `if constexpr (MIXED)`, the extra arguments exist in the masked ones only): 111-128 VGPRs, no
// scratch, WALL at the 128-register ceiling of a 1024-thread workgroup.  The masked ones fit under the same ceiling without
// scratch because nothing of theirs stays in a register across the pair sweep: the mask is in LDS where the thread that selects
// on it reads anyway, 1/|b| waits in LDS, U and F are addressed from x, and the basis in global memory is addressed with
// 32-bit offsets.
//
// The solver's body is rbl_small_solve (rbl_small_solve.hpp), shared with the jointed solve of the ensembles (rbl_small_joints.hip,
// JOINTS = true); here it is instantiated without joints, eight times.
#include "rbl_small_solve.hpp"

namespace {

template <bool WALL, bool VLDS, bool MIXED>
__global__ __launch_bounds__(SGT) void k_gmres_small(std::conditional_t<MIXED, SmallArgsMixed, SmallArgs> A)
{
  rbl_small_solve<WALL, VLDS, MIXED, false>(A);
}

}  // namespace

// does the one-kernel solver cover this system?
bool rbl_gmres_small_fits(int N_blb, int N_bod, int max_iter, bool block_pc, bool mixed)
{
  const long N = (long)N_blb * N_bod;
  if (block_pc || N < 1 || N > SG_MAXN || N_bod > SG_MAXB || max_iter < 1 || max_iter > SG_MAXIT) return false;
  return small_lds_base_bytes(N_blb, N_bod, max_iter, mixed) <= SG_LDS_MAX;
}

size_t rbl_gmres_small_work_doubles(int N_blb, int N_bod, int max_iter, int n_joints) { return small_work_doubles(N_blb, N_bod, max_iter, n_joints); }

// the launcher is small_launch (rbl_small_solve.hpp); the kernels of this file for one wall flag, [vlds]
template <bool MIXED>
static auto small_row(bool wall)
{
  static void (*const tab[2][2])(std::conditional_t<MIXED, SmallArgsMixed, SmallArgs>) = {
      {k_gmres_small<false, false, MIXED>, k_gmres_small<false, true, MIXED>}, {k_gmres_small<true, false, MIXED>, k_gmres_small<true, true, MIXED>}};
  return tab[wall];
}

// the grid of one.  d_work: rbl_gmres_small_work_doubles(...) doubles; d_scal: 2 doubles (iterations as an int in the first,
// residual in the second)
int rbl_launch_gmres_small(hipStream_t st, const RblParams &P, bool wall, const double *dX, const double *dQ, const double *dcfg,
                           int N_blb, int N_bod, const double *d_rhs, const double *d_x0, double *d_x, int max_iter, double rtol,
                           double fsign, double *d_work, double *d_scal, unsigned *d_err)
{
  const RblSmallEns S = {dX, dQ, dcfg, N_blb, N_bod, 1, d_rhs, d_x, max_iter, rtol, d_work, (int *)d_scal, d_scal + 1, d_err};
  return small_launch(st, P, S, SmallArgs{}, small_row<false>(wall), false, 0, d_x0, fsign, 0);
}

// every replica of an ensemble.  d_mask: the masked solve (MIXED above) -- S.rhs is the all-free right-hand side [slip ; -body_in]
// (the loads of the free components), d_mask reps x per N_bod bytes (per = 1: one per body, 6: one per velocity component),
// d_body_in reps x 6 N_bod (the prescribed components' velocities are read)
int rbl_launch_gmres_small_ens(hipStream_t st, const RblParams &P, bool wall, const RblSmallEns &S, const unsigned char *d_mask,
                               const double *d_body_in, int per)
{
  if (!d_mask) return small_launch(st, P, S, SmallArgs{}, small_row<false>(wall));
  SmallArgsMixed A = {};
  A.mask = d_mask; A.body_in = d_body_in; A.reps = S.reps; A.per = per;
  return small_launch(st, P, S, A, small_row<true>(wall), true);
}
