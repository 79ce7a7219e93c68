// rbl_small_cells.hip -- the one-kernel GMRES solve of rbl_small_per.hip for an ensemble with a periodic cell PER REPLICA
// (rbl_ensemble_set_cells; include/rbl.h section 5): k_gmres_small_cells<VLDS, MIXED>.  The kernel takes the table of the
// replicas' cells (RblEnsCellRec, R records) where k_gmres_small_per takes the one cell by value, reads record blockIdx.x --
// its radius-scaled form, the first 40 bytes -- before anything else and hands the solver's body (rbl_small_solve with PER = true)
// the very argument block k_gmres_small_per hands it.  The index is the workgroup's, the table is only read: the record arrives
// by scalar loads and stays in scalar registers as the by-value cell does, so W, kc, NI, npair and nall of the pair sweep
// (rbl_small_pair_sweep<true, true>, rbl_small_dev.hpp) are per-workgroup values and a replica with more images runs more steps.
// Arithmetic per pair and image is k_gmres_small_per's: replica r returns the bits of that kernel launched alone with cell r.
//
// Four instantiations in a translation unit of their own: rbl_small_per.hip keeps its four, instruction for instruction.
#include "rbl_small_solve.hpp"

namespace {

struct SmallArgsCells : SmallArgs { const RblEnsCellRec *cells; };
struct SmallArgsMixedCells : SmallArgsMixed { const RblEnsCellRec *cells; };

template <bool VLDS, bool MIXED>
__global__ __launch_bounds__(SGT) void k_gmres_small_cells(std::conditional_t<MIXED, SmallArgsMixedCells, SmallArgsCells> A)
{
  using Base = std::conditional_t<MIXED, SmallArgsMixed, SmallArgs>;
  std::conditional_t<MIXED, SmallArgsMixedPer, SmallArgsPer> B;
  static_cast<Base &>(B) = static_cast<const Base &>(A);
  B.C = A.cells[blockIdx.x].S;
  rbl_small_solve<true, VLDS, MIXED, false, true>(B);
}

}  // namespace

// rbl_launch_gmres_small_ens_per with replica r in the cell d_cells[r] (S.reps records on the device)
int rbl_launch_gmres_small_ens_cells(hipStream_t st, const RblParams &P, const RblEnsCellRec *d_cells, const RblSmallEns &S,
                                     const unsigned char *d_mask, const double *d_body_in, int per)
{
  if (!d_mask) {
    static void (*const row[2])(SmallArgsCells) = {k_gmres_small_cells<false, false>, k_gmres_small_cells<true, false>};
    SmallArgsCells A = {};
    A.cells = d_cells;
    return small_launch(st, P, S, A, row);
  }
  static void (*const row[2])(SmallArgsMixedCells) = {k_gmres_small_cells<false, true>, k_gmres_small_cells<true, true>};
  SmallArgsMixedCells A = {};
  A.mask = d_mask; A.body_in = d_body_in; A.reps = S.reps; A.per = per; A.cells = d_cells;
  return small_launch(st, P, S, A, row, true);
}
