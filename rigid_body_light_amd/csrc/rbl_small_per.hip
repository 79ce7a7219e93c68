// rbl_small_per.hip -- the one-kernel GMRES solve of rbl_small.hip for the ensembles in a periodic cell (include/rbl.h sections 5
// and 10): k_gmres_small_per<VLDS, MIXED>, the body of the solver (rbl_small_solve, rbl_small_solve.hpp) with PER = true, so that the
// operator is [B M_per B lambda - K U ; K^T lambda]: the pair sweep evaluates every unordered pair once per image and takes in every
// blob's own images (rbl_small_pair_sweep<true, true>, rbl_small_dev.hpp, where the scheme is described).  Wall only -- the
// free-space lattice sum diverges --, unmasked and masked, the Krylov basis in LDS or in global memory: four instantiations.
// The cell travels as a kernel argument behind the open system's (SmallArgsPer / SmallArgsMixedPer): it sits in scalar
// registers and nothing of it is live in a vector register across the pair call: 116 - 122 VGPRs, no scratch.
// The self block, the image-free diagonal preconditioner, the masks and the LDS budget (rbl_gmres_small_fits) are the open system's.
// Every sum has a fixed order: replica r of R is bitwise the launch of that replica alone, and the basis in LDS or in global memory
// gives the same bits.
//
// These kernels live in a translation unit of their own so that rbl_small.hip keeps exactly its eight instantiations.
#include "rbl_small_solve.hpp"

namespace {

template <bool VLDS, bool MIXED>
__global__ __launch_bounds__(SGT) void k_gmres_small_per(std::conditional_t<MIXED, SmallArgsMixedPer, SmallArgsPer> A)
{
  rbl_small_solve<true, VLDS, MIXED, false, true>(A);
}

// one workgroup per replica, as rbl_small.hip's launch_small; A.C (and MIXED: mask, body_in, reps, per) set by the caller
template <bool MIXED>
int launch_small_per(hipStream_t st, const RblParams &P, const double *dX, const double *dQ, const double *dcfg, int N_blb, int N_bod,
                     const double *d_rhs, double *d_x, int max_iter, double rtol, double *d_work, int *d_iters, double *d_resid,
                     unsigned *d_err, int reps, std::conditional_t<MIXED, SmallArgsMixedPer, SmallArgsPer> A)
{
  if (!rbl_gmres_small_fits(N_blb, N_bod, max_iter, false, MIXED)) return RBL_ERR_SIZE;
  const size_t nsys = (size_t)3 * N_blb * N_bod + (size_t)6 * N_bod;
  size_t lds = small_lds_base_bytes(N_blb, N_bod, max_iter, MIXED);
  const size_t basis = small_basis_bytes(N_blb, N_bod, max_iter);
  bool vlds = lds + basis <= SG_LDS_MAX;                   // the Krylov basis beside the vectors in LDS?
  A.X = dX; A.Q = dQ; A.cfg = dcfg; A.rhs = d_rhs; A.x0 = nullptr; A.x = d_x;
  A.V = d_work; A.H = d_work + (size_t)(max_iter + 1) * nsys;
  A.iters_out = d_iters; A.resid_out = d_resid; A.err = d_err;
  A.work_stride = rbl_gmres_small_work_doubles(N_blb, N_bod, max_iter); A.err_stride = 1;
  A.P = P; A.N_blb = N_blb; A.N_bod = N_bod; A.max_iter = max_iter; A.rtol = rtol; A.fsign = 1.0;
  auto allow = [&](bool v, size_t bytes) {                 // as rbl_small.hip's launcher: beyond 64 KB the attribute is needed
    if (bytes <= 64 * 1024) return true;
    const void *fn = v ? (const void *)k_gmres_small_per<true, MIXED> : (const void *)k_gmres_small_per<false, MIXED>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  };
  if (vlds && allow(true, lds + basis)) lds += basis;
  else {
    vlds = false;
    if (!allow(false, lds)) return RBL_ERR_SIZE;
  }
  const dim3 grid((unsigned)reps);
  if (vlds) hipLaunchKernelGGL((k_gmres_small_per<true, MIXED>), grid, dim3(SGT), lds, st, A);
  else hipLaunchKernelGGL((k_gmres_small_per<false, MIXED>), grid, dim3(SGT), lds, st, A);
  return RBL_OK;
}

}  // namespace

// rbl_launch_gmres_small_ens in the cell C
int rbl_launch_gmres_small_ens_per(hipStream_t st, const RblParams &P, const RblSmallCell &C, const double *dX, const double *dQ,
                                   const double *dcfg, int N_blb, int N_bod, int reps, const double *d_rhs, double *d_x, int max_iter,
                                   double rtol, double *d_work, int *d_iters, double *d_resid, unsigned *d_rep_err)
{
  SmallArgsPer A = {};
  A.C = C;
  return launch_small_per<false>(st, P, dX, dQ, dcfg, N_blb, N_bod, d_rhs, d_x, max_iter, rtol, d_work, d_iters, d_resid, d_rep_err, reps, A);
}

// rbl_launch_gmres_small_ens_mixed in the cell C: d_UFx is the ONE block [U | F | x] of that launcher
int rbl_launch_gmres_small_ens_mixed_per(hipStream_t st, const RblParams &P, const RblSmallCell &C, const double *dX, const double *dQ,
                                         const double *dcfg, int N_blb, int N_bod, int reps, const double *d_rhs, double *d_UFx,
                                         int max_iter, double rtol, double *d_work, int *d_iters, double *d_resid, unsigned *d_rep_err,
                                         const unsigned char *d_mask, const double *d_body_in, int per)
{
  SmallArgsMixedPer A = {};
  A.mask = d_mask; A.body_in = d_body_in; A.reps = reps; A.per = per; A.C = C;
  return launch_small_per<true>(st, P, dX, dQ, dcfg, N_blb, N_bod, d_rhs, d_UFx + (size_t)2 * reps * 6 * N_bod, max_iter, rtol, d_work,
                                d_iters, d_resid, d_rep_err, reps, A);
}
