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

}  // namespace

// rbl_launch_gmres_small_ens in the cell C (d_mask, as there: the masked solve); the launcher is small_launch (rbl_small_solve.hpp)
int rbl_launch_gmres_small_ens_per(hipStream_t st, const RblParams &P, const RblSmallCell &C, const RblSmallEns &S,
                                   const unsigned char *d_mask, const double *d_body_in, int per)
{
  if (!d_mask) {
    static void (*const row[2])(SmallArgsPer) = {k_gmres_small_per<false, false>, k_gmres_small_per<true, false>};
    SmallArgsPer A = {};
    A.C = C;
    return small_launch(st, P, S, A, row);
  }
  static void (*const row[2])(SmallArgsMixedPer) = {k_gmres_small_per<false, true>, k_gmres_small_per<true, true>};
  SmallArgsMixedPer A = {};
  A.mask = d_mask; A.body_in = d_body_in; A.reps = S.reps; A.per = per; A.C = C;
  return small_launch(st, P, S, A, row, true);
}
