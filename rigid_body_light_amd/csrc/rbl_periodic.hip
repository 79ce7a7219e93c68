// rbl_periodic.hip -- the periodic cell in x and y (include/rbl.h section 10): its state and the refusals of what it is not
// offered with.  The cell itself acts in two places: apply_M_enqueue / apply_M_multi_enqueue (rbl_products.hip) route every
// mobility product to k_apply_M_per (rbl_kernels.hip), and ia_launch (rbl_forces.hip) selects the minimum-image instantiations
// of the pair-force kernels.  The cell of an ensemble (rbl_ensemble_set_periodic, section 5) is state of its own beside it: it acts in
// the one-kernel solver's pair sweep, the drift kernel and the dense build of rbl_ensemble.hip, and ia_launch takes it when it is
// called for an ensemble.  That cell is either one shared by the replicas or one per replica (rbl_ensemble_set_cells): the later
// call replaces the earlier.  Nothing here touches a device but ens_cells_upload, which carries the table of the replicas' cells
// to the kernels that read it.
#include <cmath>
#include <string>

#include "rbl_api_internal.hpp"

bool periodic_on(const rbl_ctx *c) { return c->per_on; }

int periodic_refuse(rbl_ctx *c, const char *who)
{
  if (!c->per_on) return RBL_OK;
  return rbl_fail(c, RBL_ERR_STATE, std::string(who) + ": not offered with a periodic cell (rbl_set_periodic; switch the cell off first)");
}

// what a product or a step asks of a cell at use (the single context's and the ensembles'): the wall term, and lengths the current
// parameters have not outgrown.  L: the cell's two lengths; setter: the call that stores them, named in the message
int periodic_use_check(rbl_ctx *c, bool wall, const double *L, const char *setter, int replica)
{
  if (!wall) return rbl_fail(c, RBL_ERR_STATE, "periodic cell: the wall term is off, and the free-space lattice sum diverges (rbl_set_wall_pc)");
  for (int k = 0; k < 2; ++k)
    if (L[k] > 0.0 && !(L[k] > 4.0 * c->S.a))
      return rbl_fail(c, RBL_ERR_STATE, "periodic cell: " + (replica >= 0 ? "replica " + std::to_string(replica) + ": " : std::string()) +
                                            "L" + (k ? "y" : "x") + " = " + std::to_string(L[k]) +
                                            " no longer exceeds 4a of the current parameters (call " + setter + " again)");
  return RBL_OK;
}

// the argument checks of rbl_set_periodic, rbl_ensemble_set_periodic and -- replica by replica, the message naming it:
// "ensemble_set_cells: replica 3: Lx ..." -- rbl_ensemble_set_cells (who: the name in the messages); n of an open axis -> 0
static int cell_args(rbl_ctx *c, const std::string &who, const double *L, int *n, int on, int replica = -1)
{
  const char *axis[2] = {"x", "y"};
  const std::string rep = replica >= 0 ? "replica " + std::to_string(replica) + ": " : std::string();
  for (int k = 0; k < 2; ++k) {
    const std::string Ln = rep + "L" + axis[k], nn = rep + "n" + axis[k];
    if (!std::isfinite(L[k]) || L[k] < 0.0)
      return rbl_fail(c, RBL_ERR_ARG, who + ": " + Ln + " = " + std::to_string(L[k]) + " must be finite and >= 0 (0: that axis is open)");
    if (L[k] > 0.0 && c->S.params_set && !(L[k] > 4.0 * c->S.a))
      return rbl_fail(c, RBL_ERR_ARG, who + ": " + Ln + " = " + std::to_string(L[k]) + " must exceed 4a = " + std::to_string(4.0 * c->S.a) +
                                          " (a blob must not overlap its own image)");
    if (L[k] > 0.0 && (n[k] < 1 || n[k] > 16))
      return rbl_fail(c, RBL_ERR_ARG, who + ": " + nn + " = " + std::to_string(n[k]) + " must lie in [1, 16] on a periodic axis (the nearest image "
                                          "alone is not positive definite)");
    if (L[k] == 0.0) n[k] = 0;
  }
  if (on && L[0] == 0.0 && L[1] == 0.0)
    return rbl_fail(c, RBL_ERR_ARG, who + ": " + rep + "Lx = 0 and Ly = 0 with on set: a cell that is switched on needs a periodic axis");
  return RBL_OK;
}

// ---- the C ABI (include/rbl.h section 10) ------------------------------------------------------------------------------------------

// the cell: checks first, nothing is stored unless every one passes
int rbl_set_periodic(rbl_ctx *c, double Lx, double Ly, int nx, int ny, int on)
{
  if (!c) return RBL_ERR_ARG;
  const double L[2] = {Lx, Ly};
  int n[2] = {nx, ny};
  int rc = cell_args(c, "set_periodic", L, n, on); if (rc) return rc;
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

// ---- the cell of an ensemble (include/rbl.h section 5): state of its own, one cell shared by the replicas -----------------------------
// The argument checks stand first (they need no device and no ensemble), then the communicator, then the ensemble

int rbl_ensemble_set_periodic(rbl_ctx *c, double Lx, double Ly, int nx, int ny, int on)
{
  if (!c) return RBL_ERR_ARG;
  const double L[2] = {Lx, Ly};
  int n[2] = {nx, ny};
  int rc = cell_args(c, "ensemble_set_periodic", L, n, on); if (rc) return rc;
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, "ensemble_set_periodic: not on a context with a communicator");
  if (!c->ens_R)
    return rbl_fail(c, RBL_ERR_STATE, "ensemble_set_periodic: the context holds no ensemble configuration (rbl_ensemble_set_config; a single "
                                      "context's cell is rbl_set_periodic)");
  c->ens_per_L[0] = L[0]; c->ens_per_L[1] = L[1];
  c->ens_per_n[0] = n[0]; c->ens_per_n[1] = n[1];
  c->ens_per_on = on != 0;
  c->ens_cells_L.clear(); c->ens_cells_n.clear(); c->ens_cells_valid = false;   // the shared cell replaces a cell per replica
  return RBL_OK;
}

int rbl_ensemble_get_periodic(const rbl_ctx *c, double *Lx, double *Ly, int *nx, int *ny, int *on)
{
  if (!c) return RBL_ERR_ARG;
  if (ens_cells_stored(c))
    return rbl_fail(const_cast<rbl_ctx *>(c), RBL_ERR_STATE, "ensemble_get_periodic: the ensemble holds a cell per replica, there is no one cell to report "
                                                             "(rbl_ensemble_get_cells)");
  if (Lx) *Lx = c->ens_per_L[0];
  if (Ly) *Ly = c->ens_per_L[1];
  if (nx) *nx = c->ens_per_n[0];
  if (ny) *ny = c->ens_per_n[1];
  if (on) *on = c->ens_per_on ? 1 : 0;
  return RBL_OK;
}

// ---- a cell per replica (include/rbl.h section 5): replica r in (Lx[r], Ly[r]) with (nx[r], ny[r]) images -----------------------------
// The shared cell's checks in its order, replica by replica: the arguments, then the communicator, then the ensemble; nothing is
// stored unless every replica passes.  The shared cell's fields are cleared: the later call replaces the earlier

bool ens_cells_stored(const rbl_ctx *c) { return !c->ens_cells_L.empty(); }

int ens_cells_upload(rbl_ctx *c)
{
  if (!ens_cells_stored(c) || (c->ens_cells_valid && c->ens_cells_a == c->S.a)) return RBL_OK;
  const size_t R = c->ens_cells_L.size() / 2;
  std::vector<RblEnsCellRec> tab(R);
  for (size_t r = 0; r < R; ++r) tab[r] = rbl_ens_cell_rec(c->S.a, &c->ens_cells_L[2 * r], &c->ens_cells_n[2 * r]);
  int rc = rbl_dev_init(c); if (rc) return rc;
  if ((rc = rbl_dev_reserve(c, c->d_ens_cells, sizeof(RblEnsCellRec) * R))) return rc;
  if ((rc = copy_h2d(c, c->d_ens_cells.p, tab.data(), sizeof(RblEnsCellRec) * R))) return rc;
  RBL_HIP(c, hipStreamSynchronize(c->stream));         // tab leaves scope
  c->ens_cells_a = c->S.a; c->ens_cells_valid = true;
  return RBL_OK;
}

int rbl_ensemble_set_cells(rbl_ctx *c, int R, const double *Lx, const double *Ly, const int *nx, const int *ny, int on)
{
  if (!c) return RBL_ERR_ARG;
  const std::string who = "ensemble_set_cells";
  if (!Lx || !Ly || !nx || !ny) return rbl_fail(c, RBL_ERR_ARG, who + ": Lx, Ly, nx or ny is NULL");
  if (R < 1 || (c->ens_R && R != c->ens_R))
    return rbl_fail(c, RBL_ERR_ARG, who + ": R = " + std::to_string(R) + " must be the ensemble's R" +
                                        (c->ens_R ? " = " + std::to_string(c->ens_R) : std::string(" (>= 1)")));
  std::vector<double> L(2 * (size_t)R);
  std::vector<int> n(2 * (size_t)R);
  for (int r = 0; r < R; ++r) {
    L[2 * (size_t)r] = Lx[r]; L[2 * (size_t)r + 1] = Ly[r];
    n[2 * (size_t)r] = nx[r]; n[2 * (size_t)r + 1] = ny[r];
    int rc = cell_args(c, who, &L[2 * (size_t)r], &n[2 * (size_t)r], on, r); if (rc) return rc;
  }
  if (comm_on(c)) return rbl_fail(c, RBL_ERR_ARG, who + ": not on a context with a communicator");
  if (!c->ens_R)
    return rbl_fail(c, RBL_ERR_STATE, who + ": the context holds no ensemble configuration (rbl_ensemble_set_config; a single context's "
                                            "cell is rbl_set_periodic)");
  // the table first: a failed upload leaves the cell the context had
  std::vector<double> L0 = c->ens_cells_L;
  std::vector<int> n0 = c->ens_cells_n;
  c->ens_cells_L.swap(L); c->ens_cells_n.swap(n); c->ens_cells_valid = false;
  int rc = ens_cells_upload(c);
  if (rc) { c->ens_cells_L.swap(L0); c->ens_cells_n.swap(n0); return rc; }
  c->ens_per_L[0] = c->ens_per_L[1] = 0.0;
  c->ens_per_n[0] = c->ens_per_n[1] = 0;
  c->ens_per_on = on != 0;
  return RBL_OK;
}

// both states: a shared cell (or none: zeros) reads back as R equal rows
int rbl_ensemble_get_cells(const rbl_ctx *cc, double *Lx, double *Ly, int *nx, int *ny, int *on, int *per_replica)
{
  rbl_ctx *c = const_cast<rbl_ctx *>(cc);
  if (!c) return RBL_ERR_ARG;
  if (!c->ens_R)
    return rbl_fail(c, RBL_ERR_STATE, "ensemble_get_cells: the context holds no ensemble configuration (rbl_ensemble_set_config)");
  const bool per = ens_cells_stored(c);
  for (int r = 0; r < c->ens_R; ++r) {
    const double *L = per ? &c->ens_cells_L[2 * (size_t)r] : c->ens_per_L;
    const int *n = per ? &c->ens_cells_n[2 * (size_t)r] : c->ens_per_n;
    if (Lx) Lx[r] = L[0];
    if (Ly) Ly[r] = L[1];
    if (nx) nx[r] = n[0];
    if (ny) ny[r] = n[1];
  }
  if (on) *on = c->ens_per_on ? 1 : 0;
  if (per_replica) *per_replica = per ? 1 : 0;
  return RBL_OK;
}
