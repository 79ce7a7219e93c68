// rbl_periodic.hip -- the periodic cell in x and y (include/rbl.h section 10): its state and the refusals of what it is not
// offered with.  The cell itself acts in two places: apply_M_enqueue / apply_M_multi_enqueue (rbl_products.hip) route every
// mobility product to k_apply_M_per (rbl_kernels.hip), and ia_launch (rbl_forces.hip) selects the minimum-image instantiations
// of the pair-force kernels.  Nothing here touches a device.
#include <cmath>
#include <string>

#include "rbl_api_internal.hpp"

bool periodic_on(const rbl_ctx *c) { return c->per_on; }

int periodic_refuse(rbl_ctx *c, const char *who)
{
  if (!c->per_on) return RBL_OK;
  return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": not offered with a periodic cell (rbl_set_periodic; switch the cell off first)");
}

// ---- the C ABI (include/rbl.h section 10) ------------------------------------------------------------------------------------------

// the cell: checks first, nothing is stored unless every one passes
int rbl_set_periodic(rbl_ctx *c, double Lx, double Ly, int nx, int ny, int on)
{
  if (!c) return RBL_ERR_ARG;
  const double L[2] = {Lx, Ly};
  int n[2] = {nx, ny};
  const char *axis[2] = {"x", "y"};
  for (int k = 0; k < 2; ++k) {
    const std::string Ln = std::string("L") + axis[k], nn = std::string("n") + axis[k];
    if (!std::isfinite(L[k]) || L[k] < 0.0)
      return rbl_fail(c, RBL_ERR_ARG, "set_periodic: " + Ln + " = " + std::to_string(L[k]) + " must be finite and >= 0 (0: that axis is open)");
    if (L[k] > 0.0 && c->S.params_set && !(L[k] > 4.0 * c->S.a))
      return rbl_fail(c, RBL_ERR_ARG, "set_periodic: " + Ln + " = " + std::to_string(L[k]) + " must exceed 4a = " + std::to_string(4.0 * c->S.a) +
                                          " (a blob must not overlap its own image)");
    if (L[k] > 0.0 && (n[k] < 1 || n[k] > 16))
      return rbl_fail(c, RBL_ERR_ARG, "set_periodic: " + nn + " = " + std::to_string(n[k]) + " must lie in [1, 16] on a periodic axis (the nearest image "
                                          "alone is not positive definite)");
    if (L[k] == 0.0) n[k] = 0;
  }
  if (on && L[0] == 0.0 && L[1] == 0.0)
    return rbl_fail(c, RBL_ERR_ARG, "set_periodic: Lx = 0 and Ly = 0 with on set: a cell that is switched on needs a periodic axis");
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, "set_periodic: not on a context with a communicator");
  if (c->ens_R) return rbl_fail(c, RBL_ERR_STATE, "set_periodic: not offered for ensembles (the context holds an ensemble configuration)");
  c->per_L[0] = L[0]; c->per_L[1] = L[1];
  c->per_n[0] = n[0]; c->per_n[1] = n[1];
  c->per_on = on != 0;
  c->step_hist_n = 0;                                    // a warm start belongs to the operator it was solved with
  return RBL_OK;
}

int rbl_get_periodic(const rbl_ctx *c, double *Lx, double *Ly, int *nx, int *ny, int *on)
{
  if (!c) return RBL_ERR_ARG;
  if (Lx) *Lx = c->per_L[0];
  if (Ly) *Ly = c->per_L[1];
  if (nx) *nx = c->per_n[0];
  if (ny) *ny = c->per_n[1];
  if (on) *on = c->per_on ? 1 : 0;
  return RBL_OK;
}
