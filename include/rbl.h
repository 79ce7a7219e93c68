/*
 * rbl.h -- C ABI of the MI355X-native blob-mobility hot path (librbl.so).
 *
 * Drop-in boundary for brennansprinkle/Rigid_Body_Light: every entry point in
 * section 1 replaces ONE method the reference binds on `c_rigid.CManyBodies`
 * (reference src/c_rigid_obj.cpp:997-1027, nanobind).  The reference-side
 * binding a maintainer would write is in INTEGRATION.md; our own pybind11
 * shim (rigid_body_light_amd/csrc/c_rigid.cpp) calls nothing but this header.
 *
 * Conventions
 *   - plain pointers + sizes, double precision only, no C++/torch types;
 *   - host-pointer entry points (section 1,2) take caller-owned contiguous
 *     arrays, never modify inputs, and are synchronous;
 *   - device-pointer entry points (section 3) take HIP device pointers, enqueue
 *     on the context's stream (rbl_set_stream) and do NOT synchronise;
 *   - every function returns an int status (0 = RBL_OK) and never throws or
 *     exit()s; rbl_last_error(ctx) gives the message for the last failure;
 *   - vectors over blobs are xyz-interleaved, body-major (reference
 *     c_rigid_obj.cpp:281-293); quaternions are scalar-first (:212-215);
 *   - a context is not thread-safe (neither is the reference object, :151-154).
 */
#ifndef RBL_H
#define RBL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBL_OK 0
#define RBL_ERR_OVERLAP 1     /* two blobs closer than 1e-12 a; reference exit()s, :53-58 */
#define RBL_ERR_BELOW_WALL 2  /* blob centre below the wall; reference throws, :95-97    */
#define RBL_ERR_NOT_SPD 3     /* Cholesky met a non-positive pivot                        */
#define RBL_ERR_SIZE 4        /* bad length / shape                                       */
#define RBL_ERR_NO_DEVICE 5   /* no HIP device / HIP runtime failure at init              */
#define RBL_ERR_HIP 6         /* a HIP call failed                                        */
#define RBL_ERR_STATE 7       /* parameters or configuration not set                      */
#define RBL_ERR_SINGULAR 8    /* K^T K singular (reference exit()s, :313-316)             */
#define RBL_ERR_ALLOC 9
#define RBL_ERR_NONFINITE 10  /* result contains inf/nan                                  */
#define RBL_ERR_ARG 11
#define RBL_ERR_COMM 12       /* a collective failed (RCCL error, librccl not loadable, callback returned non-zero) */
#define RBL_ERR_CAPACITY 13   /* a bounded list overflowed (interaction neighbour lists); nothing was truncated silently */

typedef struct rbl_ctx rbl_ctx;

/* ===================================================================== */
/* 1. One entry point per method bound in the reference (file:line)       */
/* ===================================================================== */

/* CManyBodies()  -- nb::init<>(), c_rigid_obj.cpp:1001.  Host-only; the HIP
 * device is initialised lazily by the first compute call. */
rbl_ctx *rbl_create(void);
void rbl_destroy(rbl_ctx *ctx);

/* static `precision`, c_rigid_obj.cpp:170-174,1024-1026.  Always "double". */
const char *rbl_precision(void);

/* setParameters(a, dt, kBT, eta, cfg), c_rigid_obj.cpp:183-195.
 * cfg: N_blb x 3 row-major; its mean is removed in a private copy (:188). */
int rbl_set_parameters(rbl_ctx *ctx, double a, double dt, double kBT, double eta,
                       const double *cfg, int N_blb);

/* setBlkPC(bool) :197, setWallPC(bool) :199 */
int rbl_set_blk_pc(rbl_ctx *ctx, int block_diag_pc);
int rbl_set_wall_pc(rbl_ctx *ctx, int wall);

/* setConfig(X[3Nb], Q[4Nb]), c_rigid_obj.cpp:201-233 (Q normalised). */
int rbl_set_config(rbl_ctx *ctx, const double *X, const double *Q, int N_bod);

/* getConfig() -> (X[3Nb], Q[4Nb]), c_rigid_obj.cpp:235-255 */
int rbl_get_config(const rbl_ctx *ctx, double *X, double *Q);

/* set_K_mats(), c_rigid_obj.cpp:395-402 */
int rbl_set_K_mats(rbl_ctx *ctx);

/* K_x_U(U[6Nb]) -> [3N], :404 ; KT_x_Lam(lambda[3N]) -> [6Nb], :410 */
int rbl_K_x_U(rbl_ctx *ctx, const double *U, double *out);
int rbl_KT_x_Lam(rbl_ctx *ctx, const double *lambda, double *out);

/* multi_body_pos() -> [3N], c_rigid_obj.cpp:295-300 (computed on the GPU) */
int rbl_multi_body_pos(rbl_ctx *ctx, double *out);

/* apply_PC(IN[3N+6Nb]) -> [3N+6Nb], c_rigid_obj.cpp:589-616.  Diagonal PC (diag_invM :489): host
 * arithmetic, O(N).  Block-diagonal PC (Block_diag_invM :461): GPU -- batched per-body mobility,
 * batched Cholesky on the matrix cores, substitution instead of the reference's explicit inverse. */
int rbl_apply_PC(rbl_ctx *ctx, const double *in, double *out);

/* get_K() / get_Kinv(), c_rigid_obj.cpp:978-992: CSC arrays.  Call once with
 * NULL arrays to get nnz, then with arrays of that size (indptr: ncols+1). */
int rbl_get_K_csc(rbl_ctx *ctx, int64_t *nnz, int64_t *nrows, int64_t *ncols,
                  double *data, int32_t *indices, int32_t *indptr);
int rbl_get_Kinv_csc(rbl_ctx *ctx, int64_t *nnz, int64_t *nrows, int64_t *ncols,
                     double *data, int32_t *indices, int32_t *indptr);

/* evolve_X_Q(U[6Nb]), c_rigid_obj.cpp:865-878 (multiplies by dt internally,
 * rebuilds K, invalidates the preconditioner).  U is not modified. */
int rbl_evolve_X_Q(rbl_ctx *ctx, const double *U);

/* apply_M(F[n3], r_vecs[n3]) -> [n3], c_rigid_obj.cpp:641-659.
 * n3 = 3 * (number of blobs in r_vecs); it need not equal 3*N_bod*N_blb
 * (reference tests/test_interface.py:171-177).  U = M F, or B (M (B F)) with
 * the wall term when wall_PC is set.  Matrix-free on the GPU. */
int rbl_apply_M(rbl_ctx *ctx, const double *F, const double *r_vecs, int64_t n3,
                double *out);

/* ===================================================================== */
/* 2. Reference C++ members that are NOT bound to Python, + extensions    */
/* ===================================================================== */

/* Kinv_x_V :406, KTinv_x_F :408 */
int rbl_Kinv_x_V(rbl_ctx *ctx, const double *V, double *out);
int rbl_KTinv_x_F(rbl_ctx *ctx, const double *F, double *out);

/* apply_M for nrhs right-hand sides, F/out column-major n3 x nrhs. */
int rbl_apply_M_multi(rbl_ctx *ctx, const double *F, const double *r_vecs, int64_t n3,
                      int nrhs, double *out);

/* rotne_prager_tensor(r) -> dense column-major n3 x n3, c_rigid_obj.cpp:413-459
 * (wall term per wall_PC).  scale_damp != 0 returns B Mob B (:668-669). */
int rbl_rotne_prager_tensor(rbl_ctx *ctx, const double *r_vecs, int64_t n3,
                            int scale_damp, double *out);

/* M_half_W(), c_rigid_obj.cpp:661-675, on the object's own configuration.
 * W == NULL: standard normal noise from `seed` (counter-based, reproducible;
 * the reference seeds from the clock, :731).  method: RBL_MHALF_CHOLESKY is the
 * reference algorithm (dense B Mob B, lower Cholesky, L W);
 * RBL_MHALF_LANCZOS is matrix-free (a different square root of the same M). */
#define RBL_MHALF_CHOLESKY 0
#define RBL_MHALF_LANCZOS 1
/* Lanczos on the block-Jacobi preconditioned matrix S = L^-1 M L^-T (L L^T = per-body mobility), then
 * x = B L S^{1/2} W: covariance B M B exactly, a handful of iterations instead of ~30 (own configuration only) */
#define RBL_MHALF_LANCZOS_PC 2
int rbl_M_half_W(rbl_ctx *ctx, const double *W, uint64_t seed, int method, double *out);

/* same on caller-supplied positions (n3 free, like apply_M) */
int rbl_M_half_W_r(rbl_ctx *ctx, const double *r_vecs, int64_t n3, const double *W,
                   uint64_t seed, int method, double *out);

/* M_RFD(), c_rigid_obj.cpp:769-796 (C++ only in the reference): random finite difference of the
 * mobility, (1/delta)[M(q + delta/2 Kinv W) - M(q - delta/2 Kinv W)] W, out[3N].  W == NULL draws
 * N(0,1) from `seed`.  The reference hard-codes delta = 1e-4. */
int rbl_M_RFD(rbl_ctx *ctx, const double *W, uint64_t seed, double delta, double *out);

/* KTinv_RFD(), c_rigid_obj.cpp:743-767: K^T (1/delta)[Kinv(q+)^T - Kinv(q-)^T] W, W[6Nb] -> out[6Nb] */
int rbl_KTinv_RFD(rbl_ctx *ctx, const double *W, double delta, double *out);

/* M_RFD_cfgs(U, delta), c_rigid_obj.cpp:798-818: blob positions of the two configurations displaced by +-(delta/2) U
 * (U[6Nb], displacement units) -> r_plus[3N], r_minus[3N] (computed on the GPU; nothing is committed).  The reference
 * also draws a noise vector there that it never uses (:801). */
int rbl_M_RFD_cfgs(rbl_ctx *ctx, const double *U, double delta, double *r_plus, double *r_minus);

/* M_RFD_from_U(U, W), c_rigid_obj.cpp:820-842: (1/delta) [M(q + delta/2 U) - M(q - delta/2 U)] W with the caller's
 * displacement U[6Nb] and vector W[3N] -> out[3N].  The reference hard-codes delta = 1e-3 here (:822). */
int rbl_M_RFD_from_U(rbl_ctx *ctx, const double *U, const double *W, double delta, double *out);

/* KT_RFD_from_U(U, W), c_rigid_obj.cpp:844-863: (1/delta) [K(q + delta/2 U)^T - K(q - delta/2 U)^T] W, W[3N] -> out[6Nb]
 * (delta = 1e-3 in the reference, :846). */
int rbl_KT_RFD_from_U(rbl_ctx *ctx, const double *U, const double *W, double delta, double *out);

/* evolve_X_Q_RFD(U), c_rigid_obj.cpp:880-893: commit the configuration displaced by U[6Nb] (displacement units: NOT
 * multiplied by dt), rebuild K, and KEEP the preconditioner of the configuration it was built for (:892 sets
 * PC_mat_Set = true: an RFD displacement is of size delta, the factors of q serve q + delta U). */
int rbl_evolve_X_Q_RFD(rbl_ctx *ctx, const double *U);

/* The saddle operator a caller's Krylov solver applies, src/Rigid.py:73-80:  x = [lambda (3N) ; U (6Nb)]  ->
 * [M lambda - K U ; K^T lambda] on the object's own configuration, host vectors, ONE upload and ONE download (the
 * wrapper composes it from multi_body_pos + apply_M + K_x_U + KT_x_Lam: four round trips). */
int rbl_apply_saddle(rbl_ctx *ctx, const double *x, double *out);

/* update_X_Q(U), c_rigid_obj.cpp:798-863: the configuration displaced by U[6Nb] (translation and rotation
 * vector per body, displacement units) -> X_out[3Nb], Q_out[4Nb] (scalar-first); nothing is committed. */
int rbl_update_X_Q(rbl_ctx *ctx, const double *U, double *X_out, double *Q_out);

/* RHS_and_Midpoint(Slip, Force), c_rigid_obj.cpp:917-976 (C++ only in the reference): right-hand side and
 * predictor configuration of the stochastic midpoint step.
 *   in : Slip[n3], Force[6Nb] (NOT modified -- the reference mutates its arguments, :963,972);
 *        W = [W1 | W2 | W_rfd], 3*n3 standard normals, or NULL to draw them from `seed` (:730-741 seeds
 *        from the clock); method = RBL_MHALF_*; split_rand as the reference member (:150, default 1);
 *        delta = RFD step (the reference hard-codes 1e-4, :771)
 *   out: RHS[n3 + 6Nb] = [ Slip - (kBT*M_RFD + BI) ; -Force ],
 *        BI = c2 (M^1/2 W1 - M^1/2 W2), c1 = 2 sqrt(kBT/dt), c2 = sqrt(kBT/dt)   (split_rand)
 *        BI = c2  M^1/2 W1,             c1 = c2 = sqrt(2 kBT/dt)                 (otherwise)
 *        X_half[3Nb], Q_half[4Nb] = update_X_Q((dt/2) Kinv c1 M^1/2 W1)           (:955-959)
 *   kBT <= 1e-10: RHS = [Slip ; -Force], X_half/Q_half = current configuration     (:967-970)
 * With RBL_MHALF_CHOLESKY the dense factor is computed once and applied to W1 and W2. */
int rbl_RHS_and_Midpoint(rbl_ctx *ctx, const double *Slip, const double *Force, const double *W,
                         uint64_t seed, int method, int split_rand, double delta, double *RHS,
                         double *X_half, double *Q_half);

/* Lanczos controls / report.  max_iter: the basis is kept (max_iter + 1 vectors of 3 N doubles per recurrence).  tol: the recurrence stops when the ERROR ESTIMATE of the increment is below tol (relative):
 * the last correction d_m = |x_m - x_{m-1}| / |x_m| extrapolated geometrically, d_m rho / (1 - rho), rho = d_m / d_{m-1}.
 * For RBL_MHALF_LANCZOS_PC the estimate is taken in the Euclidean norm of the increment itself (RBL_OPT_LANCZOS_EUCLID_NORM = 0:
 * in its energy norm).  The report returns the iterations used by the last call and that estimate. */
int rbl_set_lanczos(rbl_ctx *ctx, int max_iter, double tol);
int rbl_get_lanczos_report(const rbl_ctx *ctx, int *iters, double *resid);

/* dense lower Cholesky of a caller matrix (column-major n x n, in place on the
 * device, result copied back; strict upper triangle zeroed). */
int rbl_cholesky_lower(rbl_ctx *ctx, double *M, int64_t n);

/* sizes / flags */
int rbl_get_sizes(const rbl_ctx *ctx, int *N_bod, int *N_blb);
const char *rbl_last_error(const rbl_ctx *ctx);

/* test hook: n independent 3x3 blocks (row-major, scaled by 1/(8 pi eta a)) of
 * pairs (ri[k], rj[k]) with indices (ii[k], jj[k]); mode 0 = reference-order
 * arithmetic (dense-build kernel), 1 = fast matvec arithmetic. */
int rbl_debug_pair_blocks(rbl_ctx *ctx, const double *ri, const double *rj,
                          const int32_t *ii, const int32_t *jj, int64_t n, int wall,
                          int mode, double *out9);

/* ===================================================================== */
/* 3. Device-pointer API (resident data, multi-GPU shards, benchmarks)    */
/* ===================================================================== */

/* Bind to the calling thread's current HIP device and a stream handle
 * (hipStream_t as void*; NULL = the default stream). */
int rbl_set_stream(rbl_ctx *ctx, void *hip_stream);

/* rows [row_begin,row_end) of apply_M over n_blobs blobs.  d_F, d_r: n_blobs*3
 * doubles on the device; d_out: 3*(row_end-row_begin).  Error conditions are
 * latched in a device word, read with rbl_sync_check. */
int rbl_apply_M_dev(rbl_ctx *ctx, const double *d_F, const double *d_r, int64_t n_blobs,
                    int64_t row_begin, int64_t row_end, double *d_out);

/* apply_M for nrhs right-hand sides resident on the device (d_F, d_out column-major
 * 3*n_blobs x nrhs).  Four or more vectors run on the fp64 matrix cores, 16 per pass. */
int rbl_apply_M_multi_dev(rbl_ctx *ctx, const double *d_F, const double *d_r, int64_t n_blobs,
                          int nrhs, double *d_out);

/* Symmetric-kernel shard of apply_M for multi-GPU strong scaling: this call evaluates the
 * unordered blob-tile pairs {I,J}, J >= I, of share i_first out of i_step: one row UNIT out of every i_step consecutive
 * ones (a unit = the rows one workgroup sweeps: 64 blobs, or 512 for large systems), at offset i_first in even blocks of
 * units and i_step - 1 - i_first in odd ones, so that the triangular work is the same for every share; it writes the PARTIAL sum of U = [B] M [B] F over all 3*n_blobs entries
 * to d_out; the sum of the i_step partial vectors (an all-reduce) is the full product.
 * i_first = 0, i_step = 1 is the whole product. */
int rbl_apply_M_sym_dev(rbl_ctx *ctx, const double *d_F, const double *d_r, int64_t n_blobs,
                        int i_first, int i_step, double *d_out);
/* the same for nrhs = 1 or 2 force vectors at once (d_F, d_out: [nrhs][3 n_blobs]); with two vectors the pair
 * coefficients are evaluated once for both (the two Brownian increments of the stochastic step) */
int rbl_apply_M_sym_multi_dev(rbl_ctx *ctx, const double *d_F, const double *d_r, int64_t n_blobs, int nrhs,
                              int i_first, int i_step, double *d_out);

/* launch geometry rbl_apply_M_sym[_multi]_dev would use (reporting: bench.py names the kernel instantiation it
 * times -- k_apply_M_sym<wall, rows_per_lane> -- and the slab workspace it needs) */
int rbl_apply_M_sym_info(rbl_ctx *ctx, int64_t n_blobs, int i_step, int nrhs, int *rows_per_lane, int *chunk_tiles,
                         int64_t *workspace_bytes);

/* the work units of that product on a GPU of n_cu compute units under the context's options, in the order they are handed out
 * (work queue: draw order), no device needed: nine numbers a unit -- index in that order, row group, chunk, first column tile,
 * column tiles, and the workspace ranges it writes for the first vector, in doubles: row sums (offset, length), column sums
 * (offset, length).  units holds the first `capacity` of the *n_units units.  info (8 ints, may be NULL): rows per lane, waves
 * per workgroup, chunk length, short chunk length, short chunks, chunks, 1 = work queue, 1 = that queue draws live units only */
int rbl_apply_M_sym_units(rbl_ctx *ctx, int64_t n_blobs, int n_cu, int i_step, int nrhs, int64_t *units, int64_t capacity,
                          int64_t *n_units, int *info, int64_t *workspace_bytes);

/* ... and the kernel instantiation a one- or two-vector symmetric product of that size launches under the context's options
 * ("k_apply_M_sym<true,2>", "k_apply_M_symw<false>", ...; name: >= 40 bytes) */
int rbl_apply_M_sym_kernel(rbl_ctx *ctx, int64_t n_blobs, int i_step, int nrhs, int wall, char *name, int name_len);

/* blob positions of bodies [body_begin, body_end) into d_out
 * (3*N_blb*(body_end-body_begin)); uses the host-side configuration. */
int rbl_blob_positions_dev(rbl_ctx *ctx, int body_begin, int body_end, double *d_out);

/* multi_body_pos() into a device vector d_out[3 N] according to the context's communicator: all bodies on this rank (single
 * GPU, tile-pair split), or -- RBL_OPT_COMM_SPLIT = 1 -- this rank's bodies followed by ONE all-gather over the ranks. */
int rbl_multi_body_pos_dev(rbl_ctx *ctx, double *d_out);

/* dense build on the device: d_out column-major n3 x n3 (ld = n3) */
int rbl_rotne_prager_tensor_dev(rbl_ctx *ctx, const double *d_r, int64_t n_blobs,
                                int scale_damp, double *d_out);

/* in-place lower Cholesky on the device (strict upper left untouched unless
 * zero_upper), then out = L W */
int rbl_cholesky_lower_dev(rbl_ctx *ctx, double *d_M, int64_t n, int zero_upper);
int rbl_trmv_lower_dev(rbl_ctx *ctx, const double *d_L, int64_t n, const double *d_W,
                       double *d_out);

/* M^{1/2} W on the device with positions d_r (n_blobs) and noise d_W (3 n_blobs) */
int rbl_M_half_W_dev(rbl_ctx *ctx, const double *d_r, int64_t n_blobs, const double *d_W,
                     int method, double *d_out);

/* ---- device-resident rigid-body operators: a Krylov iteration without host round trips ----
 * rbl_sync_bodies_dev uploads (X, Q, ref_cfg) and computes lever arms + blob positions on the
 * GPU; the functions below call it themselves when the configuration has changed.
 * Vectors: U/F 6*N_bod, lambda/slip 3*N, saddle/PC vectors 3*N + 6*N_bod (reference layout). */
int rbl_sync_bodies_dev(rbl_ctx *ctx);
/* uploads + workspace growth + preconditioner build for the current configuration, so that the
 * operator calls below are launch-only afterwards (capturable in a hipGraph) */
int rbl_prepare_dev(rbl_ctx *ctx);
int rbl_positions_dev(rbl_ctx *ctx, const double **d_pos, int64_t *n_blobs);  /* multi_body_pos, resident */
int rbl_K_x_U_dev(rbl_ctx *ctx, const double *d_U, double *d_out);            /* K_x_U    :404 */
int rbl_KT_x_Lam_dev(rbl_ctx *ctx, const double *d_lambda, double *d_out);    /* KT_x_Lam :410 */
int rbl_apply_PC_dev(rbl_ctx *ctx, const double *d_in, double *d_out);        /* apply_PC :589, diagonal PC */
int rbl_apply_saddle_dev(rbl_ctx *ctx, const double *d_x, double *d_out);     /* src/Rigid.py:73-80 */
/* Per-body factors L L^T = M_body of the object's own configuration (wall term per wall_PC, undamped; the
 * block-diagonal preconditioner's factors), applied to a blob vector d_in[n3] -> d_out[n3]:
 * mode 0: (L L^T)^-1 x, 1: L^-1 x, 2: L^-T x, 3: L x (mode 3 not in place).  With the wall term L is the lower Cholesky
 * factor of the body's block, rebuilt per configuration.  In free space every body's block is ONE body-frame matrix seen
 * through the body's rotation, M_b = (I x R_b) M_body (I x R_b)^T, so the factor is L = (I x R_b) chol(M_body): built once per
 * rbl_set_parameters, exact for every configuration, not triangular (mode 0 is the same operator either way;
 * RBL_OPT_BODYFRAME_FACTOR = 0 restores per-configuration Cholesky factors).  rbl_set_no_damp(ctx, 1) makes the matvec entry points
 * apply the plain wall-corrected M (no damping B) until switched off again: together they let a caller compose
 * the preconditioned square root  B L (L^-1 M L^-T)^{1/2} W  around its own (e.g. sharded) product.
 * Modes 5, 6, 7 (all bodies, not in place, single GPU) apply the WHOLE factor G the library's preconditioned Lanczos root
 * uses on this configuration -- G^-1 x, G^-T x, G x with G = L (I + Q (L_E - I) Q^T), the two-level factor (RBL_OPT_LANCZOS_TWO_LEVEL,
 * default), or G = L: what a test needs to check the root identities  s = G^-1 B^-1 x,  v = G^-T W,  |s|^2 = v^T M v,
 * root(s) = B M v  whatever the factor. */
int rbl_block_solve_dev(rbl_ctx *ctx, const double *d_in, double *d_out, int mode);
/* the same for the bodies [body_begin, body_end) only (body_end < 0: to the last body): d_in / d_out are still
 * full-length blob vectors, only the entries of those bodies are read and written, and only those bodies are
 * factored -- a multi-GPU driver gives every rank its own bodies and all-gathers the result. */
int rbl_block_solve_range_dev(rbl_ctx *ctx, const double *d_in, double *d_out, int mode, int body_begin, int body_end);
int rbl_set_no_damp(rbl_ctx *ctx, int on);
/* Keep the per-body Cholesky factors for `every` configuration changes (default 1: rebuilt after each change) before
 * they are rebuilt: both of their uses -- the block-diagonal preconditioner and the L of the preconditioned square
 * root -- stay exact with factors of a nearby configuration, only the iteration counts move.  M^-1 K and
 * (K^T M^-1 K)^-1 are still rebuilt for every configuration (with the kept factors). */
int rbl_set_block_refresh(rbl_ctx *ctx, int every);

/* Right-preconditioned GMRES(max_iter <= 255, no restart) on the saddle operator of the object's own
 * configuration (src/Rigid.py:73-80 is what a caller's Krylov solver applies; the reference ships no solver):
 * solves [M -K; K^T 0] x = rhs with P^-1 = apply_PC, all vectors in HBM.  rtol <= 0: exactly max_iter
 * iterations, no host round trip inside the loop; rtol > 0: stops at the first iteration whose residual
 * estimate is below rtol (tested every iteration, or every 4th for small launch-bound systems).  d_rhs, d_x: n3 + 6 N_bod doubles. */
int rbl_gmres_saddle_dev(rbl_ctx *ctx, const double *d_rhs, int max_iter, double rtol, double *d_x,
                         int use_x0 /* d_x holds an initial guess, e.g. the previous step's solution */,
                         int *iters, double *resid);
/* the same solve for host vectors (one upload of rhs [and x0], one download of x): what a caller of the wrapper's apply_saddle /
 * apply_PC would otherwise loop over from outside (src/Rigid.py:69-80) */
int rbl_gmres_saddle(rbl_ctx *ctx, const double *rhs, int max_iter, double rtol, double *x, int use_x0, int *iters, double *resid);
/* nrhs right-hand sides of the SAME configuration in lock step (rhs, x: nrhs vectors of n3 + 6 N_bod doubles, one after the other):
 * nrhs independent GMRES recurrences -- each column gets exactly the iterates rbl_gmres_saddle_dev would give it, its own iteration
 * count and residual (iters, resid: nrhs entries, either may be NULL) -- whose mobility products run 16 at a time on the fp64
 * matrix cores (the multi-vector kernel of rbl_apply_M_multi_dev) and whose block-preconditioner applications share passes over
 * the per-body factors.  The customer: the body mobility matrix (6 N_bod unit loads), several noise realisations of one
 * configuration.  The operator such loops iterate is the reference's src/Rigid.py:69-80. */
int rbl_gmres_saddle_multi_dev(rbl_ctx *ctx, const double *d_rhs, int nrhs, int max_iter, double rtol, double *d_x, int *iters,
                               double *resid);
int rbl_gmres_saddle_multi(rbl_ctx *ctx, const double *rhs, int nrhs, int max_iter, double rtol, double *x, int *iters, double *resid);
/* Whole time steps in one call, on the object's own configuration (the reference has no driver; these are what
 * rigid_body_light_amd/krylov.py's steppers do, for hosts without a Python loop).
 *   rbl_step_deterministic: solve [M -K; K^T 0][lambda; U] = [slip; -F_body] (rbl_gmres_saddle_dev; slip NULL = 0;
 *       warm_start: 0 cold, 1 begin from the previous call's solution, 2 / 3 from the linear / quadratic extrapolation
 *       of the last two / three solutions), then evolve_X_Q(U).
 *   rbl_step_brownian: stochastic midpoint step -- RHS_and_Midpoint at q^n (W = [W1|W2|W_rfd] host, or NULL for
 *       seeded device noise; method RBL_MHALF_*), saddle solve at q^{n+1/2}, update from q^n.
 * F_body: host, 6 N_bod; slip: host, 3 N_blobs.  iters / resid report the GMRES run.
 * Joints set with rbl_set_joints (section 9) are IGNORED by both, as by every entry point outside section 9: only
 * rbl_solve_jointed / rbl_step_jointed impose them. */
int rbl_step_deterministic(rbl_ctx *ctx, const double *F_body, const double *slip, int max_iter, double rtol,
                           int warm_start, int *iters, double *resid);
int rbl_step_brownian(rbl_ctx *ctx, const double *F_body, const double *slip, const double *W, uint64_t seed,
                      int method, int split_rand, double delta, int max_iter, double rtol, int *iters,
                      double *resid);

/* RHS_and_Midpoint on device vectors (d_Slip[n3], d_Force[6Nb], d_W[3 n3] or NULL, d_RHS[n3+6Nb]);
 * X_half / Q_half are host arrays (O(N_bod)). */
int rbl_RHS_and_Midpoint_dev(rbl_ctx *ctx, const double *d_Slip, const double *d_Force, const double *d_W,
                             uint64_t seed, int method, int split_rand, double delta, double *d_RHS,
                             double *X_half, double *Q_half);

/* ---- multi-GPU inside the library's own solvers --------------------------------------------------------------
 * One process per GPU, every rank holds the same (replicated) body state and calls the same entry points with the
 * same arguments.  Once a context has a communicator, every FULL mobility product the library evaluates for itself --
 * the iterations of rbl_gmres_saddle_dev, of the Lanczos square roots, M_RFD, rbl_apply_saddle_dev, the whole-step
 * entry points, and rbl_apply_M_dev over the full row range -- is this rank's share of the work followed by one
 * collective (RBL_OPT_COMM_SPLIT):
 *   0 (default)  unordered blob-tile pairs, dealt as rbl_apply_M_sym_dev(rank, world) deals them; the partial
 *                full-length U is completed by ONE sum all-reduce (24 N bytes);
 *   1            rows by body index (SURVEY.md 8e / north_star): each rank computes the geometry of ITS bodies, the blob
 *                positions are all-gathered once per configuration, a product is the ordered-pair kernel on the rank's own
 *                rows followed by ONE all-gather of U.
 * Per-body work (block factors, their applications) is done by the body's owner -- bodies are split contiguously by
 * index, sizes differing by at most one -- and completed by an in-place all-gather of the owners' segments.  All vectors
 * of the Krylov recurrences stay replicated and bitwise identical on every rank, so the ranks take the same convergence
 * decisions.
 *
 * (a) RCCL inside the library -- what a C / C++ host (the reference is one, c_rigid_obj.cpp:997-1027) uses: rank 0 calls
 *     rbl_comm_unique_id and hands the RBL_COMM_ID_BYTES bytes to the other ranks by whatever means the host has (MPI_Bcast,
 *     a file, torch.distributed); every rank then calls rbl_comm_init_rccl (collective: ncclCommInitRank on the context's
 *     device).  The collectives are ncclAllReduce / ncclAllGather / grouped ncclBroadcast enqueued on the context's stream;
 *     no host code runs between two products of a solve.  librccl is opened at run time (dlopen "librccl.so.1"): the copy
 *     already in the process (PyTorch's) or ROCm's.  world == 1 is allowed and keeps the multi-GPU code path on with one
 *     share: a one-GPU rehearsal of what N ranks run.
 * (b) the caller's callbacks (rbl_set_comm / rbl_set_comm_ops) -- rehearsals over other transports (gloo with host staging).
 *     `allreduce` must leave the sum over all ranks in d_buf[0..count) on every rank; `allgatherv` (optional) must leave
 *     rank r's segment d_buf[offsets[r] .. offsets[r] + counts[r]) on every rank, in place; both ordered after the work
 *     already enqueued on the context's stream and before whatever is enqueued next.  Without `allgatherv` the library
 *     zero-pads and sums instead.  allreduce == NULL switches back to single-GPU products.
 * rbl_comm_finalize destroys the communicator (rbl_destroy does it too). */
typedef int (*rbl_allreduce_fn)(void *user, double *d_buf, int64_t count);
typedef int (*rbl_allgatherv_fn)(void *user, double *d_buf, const int64_t *offsets, const int64_t *counts);
int rbl_set_comm(rbl_ctx *ctx, int rank, int world, rbl_allreduce_fn allreduce, void *user);
int rbl_set_comm_ops(rbl_ctx *ctx, int rank, int world, rbl_allreduce_fn allreduce, rbl_allgatherv_fn allgatherv, void *user);
#define RBL_COMM_ID_BYTES 128
int rbl_comm_unique_id(void *id_out /* RBL_COMM_ID_BYTES */);
int rbl_comm_init_rccl(rbl_ctx *ctx, const void *unique_id, int rank, int world);
int rbl_comm_finalize(rbl_ctx *ctx);
/* kind: 0 single GPU, 1 callbacks, 2 RCCL inside the library */
int rbl_comm_info(const rbl_ctx *ctx, int *rank, int *world, int *kind);
/* the context's collectives themselves on a device buffer (tests, benchmarks): sum all-reduce; in-place all-gather of the
 * per-rank segments d_buf[offsets[r] .. + counts[r]) */
int rbl_comm_allreduce_dev(rbl_ctx *ctx, double *d_buf, int64_t count);
int rbl_comm_allgatherv_dev(rbl_ctx *ctx, double *d_buf, const int64_t *offsets, const int64_t *counts);

/* ---- per-phase timings of the library's own solvers (the reference has one gettimeofday helper,
 * c_rigid_obj.cpp:22-29, and one printf around M_half_W, :929-932) -----------------------------------------------------
 * rbl_set_timing(ctx, 1): from now on the phases below are bracketed by hipEvents on the context's stream (a few
 * microseconds of host time per bracket; off by default).  rbl_get_timings synchronises the stream and returns, per
 * phase, the GPU time in milliseconds and the number of brackets accumulated since the last rbl_reset_timings (arrays of
 * RBL_T_COUNT entries; either may be NULL).  RBL_T_TOTAL spans the solver entry points (rbl_gmres_saddle_dev, the
 * Lanczos square roots, M_RFD); what it holds beyond the other phases is Krylov vector work, K operators, launch gaps and
 * the host's convergence tests.  On a multi-GPU context (rbl_set_comm) RBL_T_COLLECTIVE is the time the stream spent in
 * the caller's all-reduce, including the wait for the slowest rank. */
#define RBL_T_PRODUCT 0     /* mobility products: pair kernels + their slab reduction                         */
#define RBL_T_PERBODY 1     /* applications of the per-body factors / inverses, preconditioner tail            */
#define RBL_T_FACTOR 2      /* per-body dense blocks, batched Cholesky, explicit inverses, M^-1 K, (K^T M^-1 K) */
#define RBL_T_COLLECTIVE 3  /* the all-reduce callback of rbl_set_comm                                          */
#define RBL_T_DENSE 4       /* dense B M B build, Cholesky, L W (RBL_MHALF_CHOLESKY)                            */
#define RBL_T_TOTAL 5       /* whole solver calls                                                               */
#define RBL_T_FORCES 6      /* configuration-dependent forces (section 4): neighbour lists, pair kernel, K^T f.  Nothing is
                               recorded while interactions are off, and the phase opens no RBL_T_TOTAL bracket           */
#define RBL_T_COUNT 7
int rbl_set_timing(rbl_ctx *ctx, int on);
int rbl_reset_timings(rbl_ctx *ctx);
int rbl_get_timings(rbl_ctx *ctx, double *ms, int64_t *calls);

/* stream-synchronise, read and clear the latched device error word */
int rbl_sync_check(rbl_ctx *ctx);

/* ---- named per-context options ---------------------------------------------------------------------------------
 * rbl_set_option(ctx, RBL_OPT_*, value) / rbl_get_option: an unknown key or a value outside the option's range returns
 * RBL_ERR_ARG and changes nothing.  rbl_option_info gives name, range and default of a key (tests enumerate
 * 1 .. RBL_OPT_COUNT - 1), rbl_option_key the key of a name (0: unknown).  All per context; defaults in brackets. */
enum {
  RBL_OPT_MATVEC_KERNEL = 1,       /* [0] 0 heuristic (symmetric kernel for full products, MFMA kernel for >= 4 vectors), 1 ordered-rows
                                      kernel, 2 symmetric kernel, 3 MFMA multi-RHS kernel also for few vectors                        */
  RBL_OPT_ORDERED_JSPLIT = 2,      /* [0] j-split of the ordered kernel (0 = heuristic)                                               */
  RBL_OPT_SYM_CHUNK = 3,           /* [0] column tiles per work unit of the symmetric kernels (0 = heuristic)                         */
  RBL_OPT_SYM_ROWS_PER_LANE = 4,   /* [0] rows per lane of the one-vector symmetric kernel: 0 heuristic, 1, 2, 4 (experiments)         */
  RBL_OPT_SYM2_ROWS_PER_LANE = 5,  /* [0] the same for the two-vector kernel                                                          */
  RBL_OPT_SYM_WAVES = 6,           /* [0] waves per workgroup of the symmetric kernels: 0 heuristic, 1 or 4 (4 needs two rows per lane; any other
                                      value, or a combination no kernel has, is RBL_ERR_ARG -- at the call or at the product)            */
  RBL_OPT_SYM_WORK_QUEUE = 7,      /* [1] large systems (four-wave workgroups): 1 a fixed set of resident workgroups draws work units
                                      from a counter (an XCD that runs faster takes more), 0 one unit per workgroup in launch order;
                                      the slabs are addressed by unit, so results are bitwise the same either way                   */
  RBL_OPT_GMRES_PC_SIGN_FIX = 8,   /* [1] rbl_gmres_saddle_dev applies apply_PC with the sign of its force block restored (one
                                      eigenvalue cluster at +1; fewer iterations, same solution); 0: the reference's sign (:601)    */
  RBL_OPT_GMRES_ONE_KERNEL = 9,    /* [1] small systems (<= 256 blobs, diagonal PC, <= 255 iterations): whole solve in ONE launch    */
  RBL_OPT_GMRES_PREDICT_CHECKS = 10, /* [1] launch-bound systems (<= 20 000 blobs): convergence tests placed by the previous solve's
                                      count and the residual's rate; 0: every 4th iteration                                         */
  RBL_OPT_GMRES_OVERLAP_CHECK = 11, /* [1] the host reads the Hessenberg columns of a convergence test while the GPU already applies the
                                      preconditioner of the next iteration (no idle stream at the test); 0: drain, then go on          */
  RBL_OPT_RELAXED_KRYLOV = 12,     /* [0] inexact Krylov: 1 = once GMRES's residual estimate is below rtol x 1e5 (and in Lanczos runs to
                                      tolerances >= 1e-4) far tile pairs are evaluated in packed single precision (relative product
                                      error <= 3e-6, ~1.8x faster); the solution still satisfies the fp64 system to rtol.  2 = in those
                                      Lanczos runs only (a root asked for to 1e-3 does not see a product error of 1e-6): every GMRES
                                      product stays fp64                                                                             */
  RBL_OPT_RELAXED_ALWAYS = 13,     /* [0] test hook: every full product through that relaxed kernel                                   */
  RBL_OPT_BLOCK_EXPLICIT_SMALL = 14, /* [1] per-body factors of bodies with <= 170 blobs applied through explicit inverses L^-1       */
  RBL_OPT_BLOCK_EXPLICIT_LARGE = 15, /* [2] explicit inverses of larger bodies (the reference's own form of Block_diag_invM,
                                      :461-487): 0 never, 1 always, 2 when it pays (multi-GPU contexts; the shared body-frame factor) */
  RBL_OPT_BLOCK_INVERSE_F32 = 16,  /* [0] keep (also) a single-precision copy of the large inverses: the preconditioner and Lanczos
                                      runs to tolerances >= 1e-5 read half the bytes (sums stay fp64)                               */
  RBL_OPT_BODYFRAME_FACTOR = 17,   /* [1] free space: ONE body-frame factor rotated with each body; 0: per-configuration factors     */
  RBL_OPT_BODYFRAME_WALL_APPROX = 18, /* [0] with the wall term: the free-space body-frame factor as an APPROXIMATE block factor      */
  RBL_OPT_BLOCK_REFRESH = 19,      /* [1] keep the per-body factors for this many configuration changes (rbl_set_block_refresh)      */
  RBL_OPT_LANCZOS_TWO_LEVEL = 20,  /* [1] preconditioned root: two-level factor L (I + Q (L_E - I) Q^T); 0: block-Jacobi factor L    */
  RBL_OPT_LANCZOS_EUCLID_NORM = 21, /* [1] preconditioned root stops on the error estimate of x itself (Euclidean norm);
                                      0: of z = (L^-1 M L^-T)^{1/2} W, i.e. of x in the energy norm x^T (B M B)^-1 x                 */
  RBL_OPT_LANCZOS_REORTH = 22,     /* [1] every new Lanczos vector re-orthogonalised against the whole basis; 0: three-term recurrence */
  RBL_OPT_NO_DAMP = 23,            /* [0] transient: the matvec entry points apply the plain wall-corrected M, no damping B          */
  RBL_OPT_COMM_SPLIT = 24,         /* [0] multi-GPU contexts: 0 unordered tile pairs + all-reduce(U), 1 rows by body index +
                                      all-gather(positions, U) -- see "multi-GPU" above                                             */
  RBL_OPT_FUSED_KRYLOV = 25,       /* [1] launch-bound systems: the product's slab reduction also writes the saddle tail and the partial
                                      sums of the Arnoldi step's first Gram-Schmidt pass, and (free-space body-frame preconditioner) the
                                      normalisation of the new basis vector is done by the preconditioner kernels that consume it
                                      (three launches fewer per GMRES iteration); 0: one kernel per operation                       */
  RBL_OPT_RELAXED_GAP_RATIO = 26,  /* [0] relaxed product: a far tile pair is swept in single precision when the extents of its boxes,
                                      d_I + 2 d_J, are at most this many times their gap (0 = the library's default); smaller = fewer
                                      pairs relaxed, smaller product error (6e-8 (1 + ratio) of a separation)                        */
  RBL_OPT_SYM_WAVE_UNITS = 27,     /* [1] mid-size systems (one row per lane, < 128 blob tiles): work units owned by single waves, four
                                      independent waves per workgroup, column sums rotating through the lanes in registers
                                      (k_apply_M_symw); 0: the round-3 kernel (one workgroup per unit, column sums by LDS atomics).
                                      Same slabs and reduction either way                                                          */
  RBL_OPT_SHARED_GEMM = 28,        /* [1] free space, bodies of <= 170 blobs: the ONE body-frame inverse / preconditioner table is applied to
                                      all bodies' vectors as a matrix-matrix product on the fp64 matrix cores (the table read once);
                                      0: batched matrix-vector products (every body re-reads it)                                    */
  RBL_OPT_TWO_LEVEL_REFRESH = 29,  /* [1] two-level factor of the preconditioned root: keep the factored coarse (body-centre) operator for this
                                      many configuration changes; the bodies' coarse basis Q follows every change.  The root stays exact
                                      for ANY coarse operator (H^-1 is the exact inverse of H whatever L_E is); a stale one costs at most
                                      a Lanczos iteration and saves its 3 N_bod-square Cholesky factor + inverse per step             */
  RBL_OPT_BLOCK_TILE_FACTOR = 30,  /* [1] per-body factors (and explicit inverses) of bodies with 3 N_blb > 512 built by ONE dataflow launch over
                                      128 x 128 tiles (rbl_tilechol.hip); 0: the batched panel kernels of rounds 1-4 (12 + 12 launches)      */
  RBL_OPT_COMM_FORCE_STAGED = 31,  /* [0] test hook: the in-place all-gathers of a native (RCCL) communicator take the STAGED form (segments
                                      padded to the largest share, one ncclAllGather, unpacked) even when the shares are equal -- what a job
                                      with N_bod % world != 0 runs, exercised with one rank                                                 */
  RBL_OPT_BLOCK_SOLVE_PIPE = 32,   /* [1] substitution through the factors of bodies with 3 N_blb > 512: ONE software pipeline per body (the
                                      dependent chain of diagonal solves in one wave, fifteen waves streaming the factor with the next
                                      step's loads already in flight, one barrier a step: k_block_solve_pipe); 0: the two-barrier kernel
                                      of rounds 1-4 (k_block_solve).  Same sums per row in another association                            */
  RBL_OPT_INTERACTION_CULL = 33,   /* [1] test hook: the interaction kernel walks only the bodies within 2 R_body + r_cut of each body;
                                      0: every other body is a neighbour (results are bitwise the same: the cull is exact and the pairs
                                      beyond r_cut are skipped either way)                                                          */
  RBL_OPT_POISON_WORKSPACE = 34,   /* [0; the environment variable RBL_POISON_WORKSPACE, read by every rbl_create, sets the starting value]
                                      test hook: every device workspace the library allocates is filled with the 32-bit pattern
                                      0x7FF87FF8 (NaN as fp64 and as fp32, a large positive int32), and scratch workspaces are
                                      refilled whenever an entry point reserves them, so a kernel that reads memory nobody wrote
                                      fails loudly instead of reading zeros.  Costs a fill and a stream synchronise per reserve */
  RBL_OPT_SYM_TAIL_CHUNK = 35,     /* [0] one GPU, four rows per lane: column tiles per work unit of the SHORT chunks the work queue ends on
                                      (0 = heuristic, 1 .. 16; the chunk length itself = no short chunks).  Chunk boundaries regroup the
                                      partial row sums: results differ in the last bits between settings, never run to run            */
  RBL_OPT_SYM_TAIL_SHARE = 36,     /* [0] per-mille of the column tiles swept at that length (0 = heuristic, 1 .. 1000).  The short length
                                      set to the chunk length together with 1000 here: the schedule of the one-length kernel, the whole
                                      (row group x chunk) rectangle in its old order                                                 */
  RBL_OPT_RECORD_MOMENTS = 37,     /* [0] every whole-step entry point also leaves the first moments D_b = sum (r_i - X_b) lambda_i^T of its
                                      solve's blob forces on the device (section 8: rbl_step_moments, rbl_ensemble_step_moments); one small
                                      launch per step.  Setting the option (to either value) discards what was recorded              */
  RBL_OPT_MC_SWEEPS_PER_LAUNCH = 38, /* [128] rbl_ensemble_mc (section 5): sweeps of one kernel launch, 1 .. 65536; a chain of n_sweeps is
                                      ceil(n_sweeps / this) launches.  Results do not depend on it.  The default keeps a launch in the tens of
                                      milliseconds at the measured 4.3 - 6.4 us per trial (profiles/ensemble_mc.jsonl): 12 ms for 19 shells,
                                      about 31 ms for 53 tetrahedra (53 trials a sweep; not timed)                                  */
  RBL_OPT_COUNT = 39
};
int rbl_set_option(rbl_ctx *ctx, int option, int64_t value);
int rbl_get_option(const rbl_ctx *ctx, int option, int64_t *value);
int rbl_option_info(int option, const char **name, int64_t *min_value, int64_t *max_value, int64_t *default_value);
int rbl_option_key(const char *name);

/* ===================================================================== */
/* 4. Configuration-dependent forces (rigid_body_light_amd/csrc/rbl_forces.hip) */
/* ===================================================================== */
/* A force model on the blobs, evaluated on the GPU at the context's configuration (the reference has none).  h = z of a
 * blob centre (wall at z = 0), a = the blob radius of rbl_set_parameters, r_ij = r_i - r_j, r = |r_ij|:
 *   weight          every blob gets -w z^ (w: buoyant weight per blob);
 *   wall repulsion  only with the wall (rbl_set_wall_pc): U_w(h) = eps_wall exp(-(h - a) / b_wall) for h >= a, continued by
 *                   its tangent below h = a (there the force is the constant eps_wall / b_wall along +z^);
 *   steric          between blobs of DIFFERENT bodies: U_b(r) = eps_blob (2a / r) exp(-(r - 2a) / b_blob) for r >= 2a,
 *                   continued by its tangent below r = 2a (bounded force; coincident blobs, r = 0, exert none); pairs
 *                   with r > r_cut are skipped.  Pairs inside one rigid body are left out (their central forces sum to
 *                   zero force and torque on the body).
 * Three further terms, each with its own switch (none changes anything while it is off); they add to the ones above:
 *   pair table      between blobs of DIFFERENT bodies: a radial potential given by its values U[k] and derivatives dU[k] =
 *                   dU/dr on the uniform grid r_k = r_min + k h, h = (r_cut - r_min) / (n - 1), 0 <= r_min < r_cut,
 *                   2 <= n <= 65537.  Inside the grid U is the cubic Hermite interpolant of (U, dU) and the force is the exact
 *                   derivative of that interpolant: with D_k = h dU_k and t = (r - r_k) / h in [0, 1],
 *                     c0 = U_k, c1 = D_k, c2 = 3 (U_{k+1} - U_k) - 2 D_k - D_{k+1}, c3 = 2 (U_k - U_{k+1}) + D_k + D_{k+1},
 *                     U = c0 + t (c1 + t (c2 + t c3)),   dU/dr = (c1 + t (2 c2 + 3 c3 t)) / h
 *                   (energy and force consistent by construction, the force continuous; the interval index is clamped to
 *                   [0, n - 2]).  Below r_min the potential continues along its tangent at r_min (the constant force -dU_0;
 *                   coincident blobs, r = 0, exert none, as in the steric term); pairs with r > r_cut are skipped.  The
 *                   table is NOT shifted: U(r_cut) != 0 is a jump in the energy (the force stays finite; tabulate a shifted
 *                   potential where the energy matters).  It adds to the steric term, each with its own cutoff; the
 *                   neighbour cull uses the larger cutoff of the pair terms that are on;
 *   height table    the same construction in the blob height z over (h_min, h_cut), any finite h_min < h_cut: tangent
 *                   continued below h_min, nothing above h_cut; applied WITH OR WITHOUT the wall of the mobility (a soft
 *                   confinement in free space), beside the wall repulsion;
 *   traps           on the body centres: stiffness k (3 lab-frame components per body, 0: no trap along that axis) and
 *                   centre X0 (3 per body), E = 1/2 sum_c k_c (X_c - X0_c)^2, force -k_c (X_c - X0_c), no torque.  The
 *                   traps enter the BODY forces and the energy; the blob-level array f_blob does not contain them.
 *                   n_bodies must be N_bod when the model is evaluated; in an ensemble (section 5) N_bod entries shared by
 *                   every replica or R N_bod entries, replica-major (anything else at evaluation time: RBL_ERR_STATE).
 * Permanent magnetic dipoles, fixed in the bodies, with two terms of their own (each with its own switch, nothing changes while
 * they are off).  Body i carries the body-frame moment m_body,i; its lab-frame moment is m_i = R(Q_i) m_body,i with the rotation
 * matrix of the blob positions (Q scalar-first, normalised):
 *   field           a uniform field B(t) = B0 + B1 cos(omega t) + B2 sin(omega t) (three lab-frame vectors: static, rotating,
 *                   oscillating, elliptical, precessing), t the context's FIELD TIME (below).  Energy -sum_i m_i . B, torque
 *                   m_i x B on body i, no force;
 *   dipole pairs    between the centres of DIFFERENT bodies of the same system (never between the replicas of an ensemble):
 *                   with r = X_i - X_j, d = |r|, s = max(d, r_core), a = m_i . r, b = m_j . r,
 *                     U_ij = c_dd [ m_i . m_j / s^3 - 3 a b / s^5 ]         (the caller puts mu_0 / 4 pi into c_dd),
 *                     force on i, d >= r_core:  3 c_dd [ a m_j + b m_i + (m_i . m_j) r - 5 a b r / d^2 ] / s^5,
 *                     force on i, d <  r_core:  3 c_dd [ a m_j + b m_i ] / s^5,
 *                     torque on i:              m_i x c_dd [ 3 b r / s^5 - m_j / s^3 ],
 *                   the exact derivatives of U: below the core s is constant and U a quadratic form in r, so the energy is
 *                   continuous and the force bounded (it jumps at r_core); d = 0 gives no force.  Pairs with d > r_cut are
 *                   skipped, r_cut = +inf takes every pair; the energy is NOT shifted at r_cut (as the tables are not).  All
 *                   pairs of a system are visited with the cutoff test: there is no neighbour list for this term.
 * Like the traps, both enter the BODY forces / torques and the energy (each body carries half of every pair energy); f_blob
 * does not contain them.  m_body: 3 n_bodies doubles, n_bodies = 1 (every body alike), N_bod, or in an ensemble R N_bod
 * replica-major, read as the traps are (entry i % n_bodies); a count that fits neither at evaluation time: RBL_ERR_STATE.
 * Bit 4 of rbl_interactions_active: dipole pairs (dipoles on and c_dd > 0); bit 5: field torque (dipoles on and field on).
 * Field time: rbl_set_field_time takes n = 1 entry (shared) or n = R (one per replica of an ensemble; a single context uses
 * entry 0; anything else at an ensemble evaluation: RBL_ERR_STATE); the default is t = 0.  NO call advances it: the one-step
 * entry points and the queries evaluate B at the time that was set.  Inside rbl_ensemble_run (section 5) replica r evaluates
 * step by step at t_r = t0_r + dt accepted[r], accepted[r] the run's own count of the replica's accepted steps at the start
 * of the step and dt the context's: under RBL_RUN_REJECT a rejected replica's field waits for it.  The run leaves the
 * context's field time as it was; continue with t0_r + dt accepted[r] from the returned counts.  The product and the sum are
 * rounded separately on the device, so a run is bitwise the loop of one-step calls with rbl_set_field_time(t0 + dt n) before
 * step n.
 * RBL_ERR_ARG, with the argument named, the previous model in place and no device touched: NULL where an array is needed
 * with on != 0; non-finite moments, field vectors, omega or t; c_dd < 0 or non-finite; with c_dd > 0: r_core <= 0 or
 * non-finite, r_cut <= r_core or NaN (+inf is accepted); n_bodies < 1 or n < 1.  on = 0 with NULL arrays only switches the
 * term off.  The getters take NULL for what is not wanted (m_body: 3 n_bodies doubles, B9: B0 | B1 | B2, t: n doubles).
 * Bonds and tethers between anchor points fixed in the bodies (their own switch, nothing changes while they are off).  Bond b
 * joins end A, the point p_A = X_i + R(Q_i) s_A of body i, to end B, the same kind of point of a DIFFERENT body j -- or, with
 * j = -1, the fixed lab-frame point P (a tether).  s is a body-frame vector relative to the body's tracking point, in the frame
 * of the structure after its mean was removed (s = 0: the centre; a blob's body-frame position: the bond ends on that blob).
 * With r = p_A - p_B and d = |r|:
 *   kind 0, harmonic    U = 1/2 k (d - l0)^2, k >= 0, l0 >= 0;
 *   kind 1, tabulated   U = k T(d), T the BOND TABLE of rbl_set_bond_table: the construction, limits and coefficient layout of
 *                       the pair table (0 <= r_min < r_cut, 2 <= n <= 65537, cubic Hermite in (U, dU)), but continued along
 *                       its tangent at BOTH ends of the grid -- below r_min with the slope dU_0, above r_cut with the slope
 *                       dU_{n-1}: a bond never breaks, nothing is skipped beyond r_cut.  FENE, worm-like chain, Morse, ...
 *                       Evaluating a kind-1 bond while no bond table is set, or while it is off: RBL_ERR_STATE.
 * Force on end A: f = -(dU/dd) r / d, on end B: -f; d = 0 exerts no force for either kind (as in the steric term) and has the
 * energy U(0).  Body i gets the force f and the torque (R(Q_i) s_A) x f, body j gets -f and (R(Q_j) s_B) x (-f), a lab point
 * nothing.  Each body carries half of a body-body bond's energy, the one body of a tether all of it.  Like the traps and the
 * dipoles the term enters the BODY forces / torques and the energy, not f_blob.  One bond is a ball joint, two are a hinge, three
 * non-collinear ones a stiff joint with bending and torsional stiffness: there are no angle or dihedral terms.  Bit 6 of
 * rbl_interactions_active: bonds on and n_bonds > 0.
 * rbl_set_bonds: body[2 n_bonds] (body[2b] >= 0; body[2b+1] >= 0 and different, or -1), anchor[6 n_bonds] (s_A, then s_B or
 * P), kind[n_bonds] or NULL (all harmonic), param[n_sets 2 n_bonds] ((k, l0) per bond, set-major), n_sets = 1, or R for a
 * stiffness or rest-length sweep with one set per replica of an ensemble (a single context uses set 0; any other count at an
 * ensemble evaluation: RBL_ERR_STATE).  In an ensemble the topology and the anchors are shared by all replicas, indices are
 * local to a replica and replicas never bond to each other.  It may be called before rbl_set_config: a body index >= N_bod is
 * found when the model is evaluated (RBL_ERR_STATE, the bond named).  RBL_ERR_ARG, with the argument named, the previous model
 * in place and no device touched: NULL where an array is needed; n_bonds < 1 or > 2^24; n_sets < 1 (or n_sets n_bonds >
 * 2^30); a first index < 0; a second index < -1; both ends on one body; a kind other than 0 or 1; non-finite anchors or
 * parameters; k < 0; l0 < 0.  on = 0 with NULL arrays only switches the term off; on = 0 with arrays stores them switched off.
 * rbl_get_bonds takes NULL for what is not wanted.  rbl_bond_state / rbl_ensemble_bond_state: length d, tension dU/dd and
 * energy U of every stored bond (on or off) at the context's / every replica's configuration, n_bonds / R n_bonds doubles
 * each (replica-major), host arrays, any may be NULL; synchronous.  RBL_ERR_STATE before any bonds were set.
 * Blob types with one pair table per unordered type pair (their own switch, nothing changes while they are off): every blob
 * carries a type in [0, n_types), 1 <= n_types <= 8, and the pair of types (s, t) may own a TYPE TABLE T_st = T_ts with the
 * construction, limits and coefficient layout of the pair table.  For blobs i (type s) and j (type t) of DIFFERENT bodies of
 * one system with r <= r_cut(s, t), and T_st set and on, the pair gets T_st(r) IN ADDITION to the built-in steric term and the
 * untyped pair table; each of the three keeps its own cutoff, a type pair without a table adds nothing, r = 0 exerts no force
 * and each blob carries half of a pair's energy.  The term enters f_blob.  A type on a patch of a body's surface makes a pair
 * potential depend on the bodies' orientations without any angular term (Janus and patchy particles, sticky caps, selective
 * binding).  In a periodic cell (section 10) the largest type cutoff that is on joins r_cut of the cell's check.
 * rbl_set_blob_types: type[n], n = N_blb (every body alike: blob k of any body has type[k]) or N_bod N_blb (one entry per
 * blob of the system, body-major; in an ensemble the system of ONE replica, shared by all replicas: body i reads row
 * i % N_bod).  An n that fits neither is found when the model is evaluated with the term active (RBL_ERR_STATE).  RBL_ERR_ARG,
 * the previous types in place: type = NULL with on != 0, n < 1, n_types outside [1, 8], a value outside [0, n_types) (the
 * message names the first offending index and its value).  type = NULL with on = 0 only switches the stored types off.
 * rbl_set_type_table(ta, tb, ...): the arguments and refusals of rbl_set_pair_table for the table of the unordered pair
 * (ta, tb) -- (tb, ta) names the same table --, and ta or tb outside [0, 8): RBL_ERR_ARG.  A table whose type is >= the current
 * n_types is stored and ignored.  rbl_clear_type_tables forgets every type table (the types stay).  Bit 7 of
 * rbl_interactions_active: types on and at least one table on whose two types are < n_types; only then is the term evaluated.
 * The cap of 8 types: the 36 table descriptors of 64 bytes sit in LDS beside the pair kernel's 16 KB position chunk.
 * Body force / torque about the body centre = K^T f_blob (+ the traps, the dipole pairs, the field torque and the bonds).  The
 * evaluation is deterministic (ordered pairs, no atomics): the same configuration gives bitwise the same forces on every
 * call and every rank (multi-GPU contexts evaluate the whole model, replicated -- the dipole terms included).
 *
 * rbl_set_interactions: on = 0 switches the built-in terms off (with every term off the steps are exactly what they are
 * without a model).  Needs rbl_set_parameters first (RBL_ERR_STATE); b_wall, b_blob > 0, eps_wall, eps_blob >= 0, 2a <= r_cut, all finite, or
 * RBL_ERR_ARG and the previous model stays in place.  rbl_get_interactions returns it (params: w, eps_wall, b_wall,
 * eps_blob, b_blob, r_cut; either pointer may be NULL).
 *
 * Inside rbl_step_deterministic and rbl_step_brownian, with any term on, the model's forces at q^n (the configuration the step
 * starts from -- for the Brownian step the one RHS_and_Midpoint is called on, reference c_rigid_obj.cpp:917-976) are added
 * to the caller's F_body in the REFERENCE convention before the right-hand side [slip; -F_body] is formed:
 * U = -N F_body, so physical forces enter as F_body - K^T f_phys.  No lower-level entry point (rbl_RHS_and_Midpoint_dev,
 * rbl_gmres_saddle_dev, ...) adds them.
 *
 * The queries return PHYSICAL forces (a force along +z^ pushes the body up, U = +N K^T f):
 *   rbl_interaction_forces_dev: d_f_blob[3 N_blobs] device or NULL, d_FT_body[6 N_bod] device (force, torque per body),
 *       energy: host scalar or NULL (the total potential energy; asking for it synchronises the stream).  Enqueued on the
 *       context's stream; a neighbour-list overflow is latched in the device error word (rbl_sync_check: RBL_ERR_CAPACITY).
 *   rbl_interaction_forces: the same into host arrays (synchronous). */
int rbl_set_interactions(rbl_ctx *ctx, double w, double eps_wall, double b_wall, double eps_blob, double b_blob,
                         double r_cut, int on);
int rbl_get_interactions(const rbl_ctx *ctx, double *params6, int *on);
/* The tabulated terms and the traps (host arrays, copied; the coefficients are built once here).  Invalid arguments return
 * RBL_ERR_ARG and leave the previous table / traps in place.  on = 0 stores the arguments and switches the term off; U = dU =
 * NULL (k = X0 = NULL) with on = 0 only switches it off.  rbl_set_parameters is not needed first.  The getters take NULL for
 * what is not wanted; coef: 4 (n - 1) doubles (c0 c1 c2 c3 per interval), k3 / X0: 3 n_bodies each; n = 0: never set.
 * rbl_get_interactions keeps reporting the built-in term only; rbl_interactions_active: bit 0 built-in term, bit 1 pair
 * table, bit 2 height table, bit 3 traps, bit 4 dipole pairs, bit 5 field torque, bit 6 bonds, bit 7 typed pair
 * tables.  The steps, the queries below and the ensembles evaluate every term that is on. */
int rbl_set_pair_table(rbl_ctx *ctx, const double *U, const double *dU, int n, double r_min, double r_cut, int on);
int rbl_get_pair_table(const rbl_ctx *ctx, int *n, double *r_min, double *r_cut, int *on, double *coef);
int rbl_set_height_table(rbl_ctx *ctx, const double *U, const double *dU, int n, double h_min, double h_cut, int on);
int rbl_get_height_table(const rbl_ctx *ctx, int *n, double *h_min, double *h_cut, int *on, double *coef);
int rbl_set_traps(rbl_ctx *ctx, const double *k3, const double *X0, int n_bodies, int on);
int rbl_get_traps(const rbl_ctx *ctx, int *n_bodies, int *on, double *k3, double *X0);
int rbl_set_dipoles(rbl_ctx *ctx, const double *m_body, int n_bodies, double c_dd, double r_core, double r_cut, int on);
int rbl_get_dipoles(const rbl_ctx *ctx, int *n_bodies, double *c_dd, double *r_core, double *r_cut, int *on, double *m_body);
int rbl_set_magnetic_field(rbl_ctx *ctx, const double B0[3], const double B1[3], const double B2[3], double omega, int on);
int rbl_get_magnetic_field(const rbl_ctx *ctx, double *B9, double *omega, int *on);
int rbl_set_field_time(rbl_ctx *ctx, const double *t, int n);
int rbl_get_field_time(const rbl_ctx *ctx, int *n, double *t);
int rbl_set_bonds(rbl_ctx *ctx, int n_bonds, const int *body, const double *anchor, const int *kind, const double *param,
                  int n_sets, int on);
int rbl_get_bonds(const rbl_ctx *ctx, int *n_bonds, int *n_sets, int *on, int *body, double *anchor, int *kind, double *param);
int rbl_set_bond_table(rbl_ctx *ctx, const double *U, const double *dU, int n, double r_min, double r_cut, int on);
int rbl_get_bond_table(const rbl_ctx *ctx, int *n, double *r_min, double *r_cut, int *on, double *coef);
int rbl_bond_state(rbl_ctx *ctx, double *length, double *tension, double *energy);
int rbl_ensemble_bond_state(rbl_ctx *ctx, double *length, double *tension, double *energy);
int rbl_set_blob_types(rbl_ctx *ctx, const int *type, int n, int n_types, int on);
int rbl_get_blob_types(const rbl_ctx *ctx, int *n, int *n_types, int *on, int *type);
int rbl_set_type_table(rbl_ctx *ctx, int ta, int tb, const double *U, const double *dU, int n, double r_min, double r_cut, int on);
int rbl_get_type_table(const rbl_ctx *ctx, int ta, int tb, int *n, double *r_min, double *r_cut, int *on, double *coef);
int rbl_clear_type_tables(rbl_ctx *ctx);
int rbl_interactions_active(const rbl_ctx *ctx, int *mask);
int rbl_interaction_forces_dev(rbl_ctx *ctx, double *d_f_blob, double *d_FT_body, double *energy);
int rbl_interaction_forces(rbl_ctx *ctx, double *f_blob, double *FT_body, double *energy);
/* what the last evaluation walked (reporting, tools/bench_interactions.py): candidate (ordered) body pairs in the neighbour
 * lists and ordered blob pairs inside the cutoff of a pair term that is on (a pair inside both counts once); synchronises the
 * stream */
int rbl_interaction_stats(rbl_ctx *ctx, int64_t *body_pairs, int64_t *blob_pairs);

/* ===================================================================== */
/* 5. Ensembles of independent replicas (rigid_body_light_amd/csrc/rbl_ensemble.hip; runs: rbl_ens_run.hip) */
/* ===================================================================== */
/* R independent replicas of one small system, resident on the device: every replica shares the context's structure,
 * parameters (a, eta, dt, kBT), wall flag and force model (section 4) and has its own X (3 N_bod) and Q (4 N_bod); arrays
 * over replicas are replica-major (replica r's X at X + 3 N_bod r).  The reference has no such object; its one-system
 * counterparts are cited per entry.  One step advances every replica with a fixed number of kernel launches whatever R is,
 * with the scheme of rbl_step_deterministic / rbl_step_brownian (reference c_rigid_obj.cpp:917-976 for the stochastic
 * midpoint step), and ends in ONE small read-back (iterations, residuals, an error word per replica).  Replicas never
 * interact, neither hydrodynamically nor through the force model.  Ensemble calls leave the context's own configuration
 * (rbl_set_config) alone.
 *
 * Limits: the sizes of the one-kernel solver (N_bod N_blb <= 256, N_bod <= 64, max_iter <= 255, the LDS must fit) and
 * 1 <= R <= 65535, else RBL_ERR_SIZE; a context with a communicator gives RBL_ERR_ARG (several GPUs run separate ensembles in
 * separate processes).  The ensemble's GMRES always uses the diagonal preconditioner (rbl_set_blk_pc is ignored: it changes
 * iteration counts, not the solution); its Brownian root is the dense Cholesky factor (RBL_MHALF_CHOLESKY).
 * Errors: RBL_ERR_STATE before rbl_set_parameters / rbl_ensemble_set_config (or after the structure changed), and the codes
 * of the one-system steps (RBL_ERR_OVERLAP, RBL_ERR_BELOW_WALL, RBL_ERR_NOT_SPD, RBL_ERR_NONFINITE, ...); rbl_last_error names
 * the first failing replica.  A step commits only if every replica succeeded: on any error no replica's X or Q changes.
 *
 *   rbl_ensemble_set_config   setConfig (:201-233) for all replicas: X[R 3 N_bod], Q[R 4 N_bod] (normalised)
 *   rbl_ensemble_get_config   getConfig (:235-255): X[R 3 N_bod], Q[R 4 N_bod]
 *   rbl_ensemble_info         R and N_bod (RBL_ERR_STATE, zeros, when none is set)
 *   rbl_ensemble_config_dev   the resident X and Q (device pointers, valid until the next ensemble call) for observables
 *                             computed on the device
 *   rbl_ensemble_step_deterministic  rbl_step_deterministic for every replica (cold start): F_body[R 6 N_bod],
 *                             slip[R n3] or NULL, iters[R], resid[R] (either may be NULL); n3 = 3 N_bod N_blb
 *   rbl_ensemble_step_brownian  rbl_step_brownian(method RBL_MHALF_CHOLESKY) for every replica: W = [W1 | W2 | W_rfd] per
 *                             replica (R 3 n3) or NULL: replica r then draws its 3 n3 normals as
 *                             rbl_launch_normal(seed, offset r ceil(3 n3 / 2)) would (Philox pairs; replica 0 sees exactly
 *                             what rbl_step_brownian draws from the same seed).  kBT <= 1e-10: the deterministic step (:967-970)
 *   rbl_ensemble_interaction_forces  the force model at every replica's configuration: FT_body[R 6 N_bod] in the REFERENCE
 *                             convention (-K^T f_phys, what the steps add to F_body), energy[R] (either may be NULL)
 * The force model enters the steps as in the one-system steps: the right-hand side's force is F_body - K^T f_phys at q^n.
 *
 * With prescribed bodies (the semantics of section 7, per replica): in every replica any subset of its bodies is held (U = 0) or
 * driven (U given) while the others stay free, deterministic or Brownian; each call returns, per replica, the loads it takes.
 * prescribed[R N_bod] (0 = free, 1 = prescribed; replica-major, it may differ from replica to replica and travels with each
 * call), body_in[R 6 N_bod] (the load of a free body, the velocity of a prescribed one), U[R 6 N_bod] (solved, or echoed for a
 * prescribed body), F[R 6 N_bod] (echoed for a free body -- with the model's share when a step added it -- or -K_b^T lambda for a
 * prescribed one: the TOTAL load everything but the fluid supplies, as in rbl_step_mixed), lambda[R n3] the blob forces.
 *   rbl_ensemble_solve_mixed          rbl_solve_mixed at every replica's configuration; nothing moves, the force model does not
 *                             enter.  lambda may be NULL; U and F must not.
 *   rbl_ensemble_step_mixed           rbl_step_mixed for every replica: the solve, then evolve_X_Q(U) -- a driven body advances by
 *                             exactly dt U_p, a held one does not move.  The force model's loads at q^n enter the free bodies only.
 *   rbl_ensemble_step_brownian_mixed  rbl_step_brownian_mixed(method RBL_MHALF_CHOLESKY) for every replica: the RFD direction and
 *                             the random part of the predictor masked to the free bodies, a prescribed body at q^n + (dt/2) U_p in
 *                             the predictor, s = slip - kBT M_RFD - BI, the masked solve at q^{n+1/2} (K_p U_p with the midpoint's
 *                             lever arms), the update from q^n by dt U.  W and seed as rbl_ensemble_step_brownian.  kBT <= 1e-10:
 *                             rbl_ensemble_step_mixed.  F (may be NULL): the instantaneous loads, thermal part included.
 * One launch of the one-kernel solver assembles K_p U_p, solves every replica's masked system and splits U and F; U and F come
 * back in the step's one read-back.  Refused before the device is touched: a NULL prescribed or body_in (or U, F of the solve),
 * max_iter < 1, rtol < 0, an entry of prescribed above 1 and a context with a communicator (RBL_ERR_ARG); max_iter > 255 and a
 * shape whose masked solve does not fit the LDS (RBL_ERR_SIZE); no ensemble configuration (RBL_ERR_STATE).  Errors during a step
 * follow the ensemble's policy: the first failing replica is named, nothing is committed unless every replica succeeded.
 * With nobody prescribed in any replica the configurations and iteration counts are bitwise those of
 * rbl_ensemble_step_deterministic / rbl_ensemble_step_brownian on the same inputs.
 *
 * With a mask per velocity component (the _dof semantics of section 7, per replica: a roller with its rotation imposed and its
 * translation free, a trapped probe free to turn, a layer with U_z = 0): prescribed6[R 6 N_bod], component by component in the lab
 * frame (translation x, y, z, then rotation x, y, z); body_in, U and F as above, read component by component.
 *   rbl_ensemble_solve_mixed_dof      rbl_solve_mixed_dof at every replica's configuration; lambda may be NULL, U and F must not.
 *   rbl_ensemble_step_mixed_dof       rbl_step_mixed_dof for every replica: the solve, then evolve_X_Q(U); a body with its three
 *                             translations held keeps X exactly while it turns.  The force model's loads and the flow model's
 *                             term enter at q^n as in rbl_ensemble_step_mixed; the model's load counts on the free components
 *                             only, so the F of a prescribed component is the TOTAL load along it.
 * The same launch of the same kernel family: a whole body is the mask with none or all six of its entries set, and the launch is
 * told whether its mask holds one entry per body or six.  A partly prescribed body's 6 x 6 preconditioner block is K^T invM K with the rows and columns of its prescribed components replaced
 * by the identity's, factored again inside the launch (RBL_ERR_NOT_SPD when that fails).  Masks whose six entries per body are
 * equal give bitwise the results, iteration counts and configurations of rbl_ensemble_solve_mixed / _step_mixed.  Refusals and the
 * error policy are those above, with prescribed6 for prescribed.
 *   rbl_ensemble_step_brownian_mixed_dof  rbl_step_brownian_mixed_dof(method RBL_MHALF_CHOLESKY) for every replica, for the masks
 *                             section 7 admits: in every body of every replica the three rotation entries are all 0 or all 1
 *                             (translation entries as the caller likes).  rbl_ensemble_step_brownian_mixed's launch sequence with
 *                             one kernel exchanged: after the unmasked predictor kernel a per-component companion sets dq = 0 and
 *                             the predictor displacement (dt/2) U_p on the prescribed components of the bodies that have any
 *                             (a partly prescribed body's scale Kinv M^{1/2}W1 is computed again there; free bodies are not
 *                             touched), and the solver is told that the mask has six entries per body.  Whole rows in every
 *                             replica give bitwise rbl_ensemble_step_brownian_mixed.  kBT <= 1e-10: rbl_ensemble_step_mixed_dof.
 *                             A mask with a partly prescribed rotation is RBL_ERR_ARG before the device is touched; the message
 *                             names the replica and the body.  The other refusals are rbl_ensemble_step_brownian_mixed's.
 * A Brownian RUN with prescribed_per = 6 stays refused (below): it is the follow-up and needs only this kernel in its sequence.
 *
 * With hard joints (section 9): the jointed saddle solve and the jointed deterministic step of every replica, ONE solver launch
 * whatever R is (k_gmres_small_jt: the one-kernel solver with the joints' rows, their Schur complement S = J N~^-1 J^T assembled,
 * factored, pivot-tested and inverted in LDS, and section 9's exact right preconditioner with the diagonal M~).  The joint set is
 * the one rbl_set_joints / rbl_set_joint_kinds stored: topology, kinds, anchors, axes and q_rel are shared by all replicas, body
 * indices are local to a replica (checked against the ensemble's N_bod at these calls); the motors' rates and angles are the
 * replica's own.
 *   rbl_ensemble_set_joint_rates   rate[sets n_joints], sets = 1 (every replica alike) or R; only a lock joint takes a non-zero rate.
 *   rbl_ensemble_set_joint_angles  theta[sets n_joints]: a sweep of stroke phases, or a restart.  Both are zero for a new joint set
 *                             and after rbl_ensemble_set_config with another R or another N_bod (a new ensemble: the joint table
 *                             on the device is made again for its shape, and the phi of the last solve is dropped); a call
 *                             with the same R and N_bod keeps them.
 *   rbl_ensemble_solve_jointed     rbl_solve_jointed at every replica's configuration; nothing moves, the force model is not
 *                             evaluated.  F_body[R 6 N_bod]; slip[R n3] or NULL; joint_rhs[R 3 n_joints] or NULL (zero);
 *                             lambda[R n3], U[R 6 N_bod], phi[R 3 n_joints] may be NULL; iters[R], resid[R].
 *   rbl_ensemble_step_jointed      rbl_step_jointed for every replica: the force model's loads and the flow model's term at q^n as
 *                             in rbl_ensemble_step_deterministic, c = -(gamma / dt) gap + joint_velocity - rate ah (a lock's
 *                             rows) formed inside the solver launch, the solve, evolve_X_Q(U).  The first failing replica names
 *                             the error and nothing commits; when the step commits, and only then, theta_j += rate_j dt per replica
 *                             (product and sum rounded one after the other).  A fixed number of launches whatever R is.
 *   rbl_ensemble_joint_state       gap[R 3 n_joints] at the current configurations (an angular joint's rows: e, or P e), phi of the
 *                             last jointed ensemble solve or step with this set, theta[R n_joints]; any may be NULL.
 * Joints switched off or never set: the step is bitwise rbl_ensemble_step_deterministic and the solve is the unjointed one-kernel
 * solve on [slip ; -F_body] at the current configuration (phi untouched).  Replica r of R is bitwise the R = 1 call on its data.
 * Capacity: rbl_gmres_small_fits' limits with, for n_j joints, 3 n_j more doubles in each of the three vectors and in every basis
 * vector kept in LDS, and 16 n_j + 18 n_j^2 + (7 n_j + N_bod + 2) / 2 doubles of joint data (lever arms, redundant rows, gaps,
 * sigmas and S's diagonal; S's factor and S^-1; the integer tables), all within the solver's 150 KB: 10 x 12 blobs with 11 joints
 * or 9 x 12 blobs with 16 joints at max_iter = 100; about 22 joints at the most.  A set that does not fit is RBL_ERR_SIZE, the
 * message telling a shape that is beyond the solver anyway from one that only the joints' LDS pushes out.
 * Refused before any device work: NULL F_body, gamma outside [0, 1], dt <= 0 (a step), max_iter outside 1 .. 255, rtol < 0
 * (RBL_ERR_ARG); sets other than 1 or R, a non-zero rate on a joint that is no lock, a non-finite value (RBL_ERR_ARG); a
 * communicator (RBL_ERR_ARG); no ensemble configuration, a joint that names a body >= N_bod (RBL_ERR_STATE); RBL_ERR_SIZE above.
 * A redundant loop of joints in some replica is RBL_ERR_NOT_SPD with "redundant" and the first failing replica in the message;
 * nothing moved, no motor's angle advanced, and the context serves a valid set afterwards.  (The lost pivot of S has an error
 * bit of its own: a body's 6 x 6 preconditioner block that fails its Cholesky is RBL_ERR_NOT_SPD with the unjointed solver's message.)
 * Not offered with joints: prescribed masks, Brownian steps, lock-step right-hand sides.  Many steps in one call are
 * rbl_ensemble_run_jointed (below, after rbl_ensemble_run), which advances the per-replica angles and a motor schedule on the
 * device.  Every other entry point of this section ignores the joints. */
int rbl_ensemble_set_joint_rates(rbl_ctx *ctx, const double *rate, int sets);
int rbl_ensemble_set_joint_angles(rbl_ctx *ctx, const double *theta, int sets);
int rbl_ensemble_solve_jointed(rbl_ctx *ctx, const double *F_body, const double *slip, const double *joint_rhs, int max_iter, double rtol,
                               double *lambda, double *U, double *phi, int *iters, double *resid);
int rbl_ensemble_step_jointed(rbl_ctx *ctx, const double *F_body, const double *slip, const double *joint_velocity, double gamma,
                              int max_iter, double rtol, double *phi, int *iters, double *resid);
int rbl_ensemble_joint_state(rbl_ctx *ctx, double *gap, double *phi, double *theta);
/* The capacity rule above as a query without a context: 1 when N_bod bodies of N_blb blobs with n_joints joints fit the jointed
 * one-kernel solver at max_iter, 0 otherwise; *lds_bytes (may be NULL) the bytes its vectors and joint data take of the 153600.
 * n_joints = 0: the rule of the unjointed ensembles. */
int rbl_ensemble_joints_fit(int N_blb, int N_bod, int max_iter, int n_joints, int64_t *lds_bytes);
/* In a periodic cell (section 10's cell for ensembles): ONE cell in x and y shared by all replicas, state of its own beside the
 * single context's -- rbl_set_periodic still refuses a context that holds an ensemble, rbl_get_periodic reports that cell, and the
 * refusals of section 10 keep their meaning.  With it on, the operator of the one-kernel solver is B M_per B of section 10: its
 * pair sweep evaluates every unordered pair once per image (the image folded into the sweep's step index, so the
 * (2 nx + 1)(2 ny + 1)-fold work spreads over the sixteen waves; d0 formed as the single context's kernel forms it) and takes in
 * every blob's own images; the drift kernel's two products are the same sweep, and the dense matrix of the Brownian root is
 * summed image by image in the reference's order (k_build_M_per).  The preconditioner stays the image-free diagonal one, so expect
 * more iterations than in the open system.  Fixed summation order: two calls agree bitwise, and replica r of R with the R = 1 call.
 * Everything of this section takes the cell -- the deterministic and Brownian steps, the masked solves and steps with their _dof
 * forms, rbl_ensemble_run with both policies and frames, rbl_ensemble_interaction_forces (the minimum-image kernels, with
 * section 10's bounds on the cutoffs; replicas still never interact), the resistance matrix through the masked solve -- except the
 * jointed calls: rbl_ensemble_solve_jointed, rbl_ensemble_step_jointed, rbl_ensemble_run_jointed and rbl_ensemble_joint_state are RBL_ERR_STATE with
 * "periodic" in the message, before any device work, while the cell is on.  Coordinates stay unwrapped (rbl_ensemble_get_config,
 * frames, bond states).  The truncated sum's positivity is observed, not proven: a replica whose dense factor fails is
 * RBL_ERR_NOT_SPD naming it.
 *   rbl_ensemble_set_periodic  the checks, in this order, and nothing stored unless all pass: the argument checks of
 *                              rbl_set_periodic (RBL_ERR_ARG: a non-finite or negative length; 0 < L <= 4a once the parameters
 *                              are set; n outside 1 .. 16 on a periodic axis, n stored as 0 on an open one; both lengths 0 with on
 *                              set); a communicator (RBL_ERR_ARG); a context that holds no ensemble configuration
 *                              (RBL_ERR_STATE).  rbl_ensemble_set_config with a new R keeps the cell.  At use: RBL_ERR_STATE when
 *                              the wall term is off ("periodic cell: the wall term is off") or the parameters have outgrown a
 *                              length ("no longer exceeds 4a").
 *   rbl_ensemble_get_periodic  reads it back; any pointer may be NULL.
 * With the cell off or never set every call of this section launches what it launched before and returns the same bits. */
int rbl_ensemble_set_periodic(rbl_ctx *ctx, double Lx, double Ly, int nx, int ny, int on);
int rbl_ensemble_get_periodic(const rbl_ctx *ctx, double *Lx, double *Ly, int *nx, int *ny, int *on);
/* A cell PER REPLICA -- an area-fraction sweep, or the truncated sum at several image counts, in one call.  The ensemble's cell is
 * either the shared one above or one per replica; the later of rbl_ensemble_set_periodic / rbl_ensemble_set_cells replaces the
 * earlier.  Replica r's cell is (Lx[r], Ly[r]) with (nx[r], ny[r]) images; a replica may keep an axis open (L = 0, its n stored as
 * 0) while another has it periodic.  The cells live on the device as one table of R records, uploaded when they are set and again
 * at use when the blob radius has changed since, never per step; every kernel that takes the shared cell by value has a form that
 * reads its replica's record (a workgroup-uniform index: the record sits in scalar registers as the argument does), with the same
 * arithmetic per pair and image.  So replica r returns the bits of an R = 1 ensemble with the shared cell (Lx[r], Ly[r], nx[r],
 * ny[r]), R equal rows return the bits of the shared cell, and everything said above of the shared cell holds per replica: every
 * step, masked solve, run (observed and driven ones with their probes), rbl_ensemble_interaction_forces and
 * rbl_ensemble_velocity_field take the cells, the jointed calls stay refused.  A replica with more images runs more steps of the
 * pair sweep: a launch lasts as long as its slowest replica.
 *   rbl_ensemble_set_cells     R entries of each array; RBL_ERR_ARG for a NULL array and for an R that is not the ensemble's (R < 1
 *                              without one), then rbl_ensemble_set_periodic's checks in its order, replica by replica -- the
 *                              message names the first offending replica, "replica 3: Lx ..." --, then the communicator
 *                              (RBL_ERR_ARG), then a context without an ensemble (RBL_ERR_STATE).  Nothing is stored unless every
 *                              replica passes.  on = 0 stores the cells switched off.  At use the checks of the shared cell run
 *                              per replica and name the first offending one, before any device work: RBL_ERR_STATE "periodic
 *                              cell: replica 0: Lx ... no longer exceeds 4a", and the force model's bounds for a unique minimum
 *                              image, RBL_ERR_ARG "interactions: replica 2: periodic cell too small ...".
 *   rbl_ensemble_get_cells     R entries into each array that is not NULL, in both states: a shared cell (or none: zeros) reads
 *                              back as R equal rows; *per_replica says which state holds.  RBL_ERR_STATE without an ensemble.
 *   rbl_ensemble_get_periodic  is RBL_ERR_STATE naming rbl_ensemble_get_cells while cells per replica are stored (on or off): there
 *                              is no one cell to report.
 *   rbl_ensemble_set_config    with the same R keeps the cells; with another R it is RBL_ERR_STATE and changes nothing while cells
 *                              per replica are stored, because the table cannot be mapped: call rbl_ensemble_set_cells or
 *                              rbl_ensemble_set_periodic first. */
int rbl_ensemble_set_cells(rbl_ctx *ctx, int R, const double *Lx, const double *Ly, const int *nx, const int *ny, int on);
int rbl_ensemble_get_cells(const rbl_ctx *ctx, double *Lx, double *Ly, int *nx, int *ny, int *on, int *per_replica);
int rbl_ensemble_set_config(rbl_ctx *ctx, int R, int N_bod, const double *X, const double *Q);
int rbl_ensemble_get_config(rbl_ctx *ctx, double *X, double *Q);
int rbl_ensemble_info(const rbl_ctx *ctx, int *R, int *N_bod);
int rbl_ensemble_config_dev(rbl_ctx *ctx, const double **d_X, const double **d_Q);
int rbl_ensemble_step_deterministic(rbl_ctx *ctx, const double *F_body, const double *slip, int max_iter, double rtol,
                                    int *iters, double *resid);
int rbl_ensemble_step_brownian(rbl_ctx *ctx, const double *F_body, const double *slip, const double *W, uint64_t seed,
                               int split_rand, double delta, int max_iter, double rtol, int *iters, double *resid);
int rbl_ensemble_interaction_forces(rbl_ctx *ctx, double *FT_body, double *energy);
int rbl_ensemble_solve_mixed(rbl_ctx *ctx, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter,
                             double rtol, double *lambda, double *U, double *F, int *iters, double *resid);
int rbl_ensemble_step_mixed(rbl_ctx *ctx, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter,
                            double rtol, double *F, int *iters, double *resid);
int rbl_ensemble_solve_mixed_dof(rbl_ctx *ctx, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter,
                                 double rtol, double *lambda, double *U, double *F, int *iters, double *resid);
int rbl_ensemble_step_mixed_dof(rbl_ctx *ctx, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter,
                                double rtol, double *F, int *iters, double *resid);
int rbl_ensemble_step_brownian_mixed(rbl_ctx *ctx, const uint8_t *prescribed, const double *body_in, const double *slip,
                                     const double *W, uint64_t seed, int split_rand, double delta, int max_iter, double rtol,
                                     double *F, int *iters, double *resid);
int rbl_ensemble_step_brownian_mixed_dof(rbl_ctx *ctx, const uint8_t *prescribed6, const double *body_in, const double *slip,
                                         const double *W, uint64_t seed, int split_rand, double delta, int max_iter, double rtol,
                                         double *F, int *iters, double *resid);

/* A run: n_steps ensemble steps in ONE call.  The inputs are uploaded once, every step's verdict and commit are taken per
 * replica on the device, the records accumulate there, and the host reads back once at the end (plus the optional status polls
 * of check_every).  The one-step calls above are unchanged; a run enqueues their very launch sequence once per step, followed by
 * two small launches (the verdict of every replica, then the commit), and flips the two configuration buffers on the host
 * without a synchronisation.  The four step families are chosen by the options: brownian 0/1, and either F_body (all bodies
 * free) or prescribed with body_in (held or driven bodies, as rbl_ensemble_step_[brownian_]mixed).  prescribed_per = 6 makes the
 * mask one entry per velocity component (prescribed[R 6 N_bod], the steps of rbl_ensemble_step_mixed_dof; 0 and 1: whole bodies);
 * such a run is deterministic only: with brownian != 0 and kBT > 1e-10 it is refused, that step's drift term is not derived.  Everything in the options is
 * constant over the run (rbl_ensemble_run_driven, below, is the run whose body input follows a drive); the force model (section 4) and the flow model (section 8) enter every step at that step's q^n.
 * The one input that moves is the magnetic field's clock (section 4): replica r evaluates B at its field time + dt accepted[r],
 * and the context's field time itself is left as it was.
 *
 * Noise: drawn on the device.  Step n of the run (n = 0, 1, ... counts the run's steps, rejected ones included) draws what
 * rbl_ensemble_step_brownian(W = NULL, seed + n) draws; injected noise is not offered.  kBT <= 1e-10: the deterministic step.
 *
 * on_error
 *   RBL_RUN_STOP (0, the default): the policy of the one-step calls.  At the first step s in which any replica's error word or
 *     the batch word is set no replica commits, and a sticky device flag makes every later step of the run commit nothing: the
 *     final configuration is bitwise what a loop of one-step calls leaves when it fails at step s.  The call returns that step's
 *     status code, rbl_last_error names the step and the first failing replica, and the outputs are still filled.
 *   RBL_RUN_REJECT (1): a replica whose error word is set at step n keeps q^n, its rejected count goes up, and it tries again at
 *     step n + 1 with that step's fresh noise; the others commit.  Here the NEW configuration is validated before it commits (a
 *     replica that landed below the wall would otherwise be accepted and fail every later step): every component of X and Q
 *     finite and, with the wall, every blob of q^{n+1} at z >= 0, the height computed with the arithmetic the next step's
 *     kernels use, so the verdict is the one they would reach.  A replica that fails validation is rejected like any other.  A
 *     non-SPD mobility of one replica is that replica's rejection (in a run the batched Cholesky reports per matrix).  What
 *     cannot be pinned to a replica -- a neighbour-list overflow of the force model -- stops the run as under RBL_RUN_STOP.
 *     A rejected Brownian move is REDRAWN.  That is the customary treatment in rigid-multiblob codes, not an unbiased one: the
 *     accepted moves are conditioned on staying valid.  rejected[] is returned so that the caller can see how much it matters.
 *     Under RBL_RUN_REJECT the replicas no longer share a clock: replica r's physical time is dt accepted[r].
 * STOP does not validate the new configuration, by design: it reproduces the loop, which meets a bad q^{n+1} one step later.
 *
 * stride > 0 records n_frames = n_steps / stride frames: frame k is the committed configuration after step (k + 1) stride - 1,
 * X[R 3 N_bod], Q[R 4 N_bod], accepted_at[R] (the replica's accepted count then) and, for runs with prescribed bodies, that
 * step's F[R 6 N_bod] (a replica rejected in that very step: its last accepted F, zeros before any).  The frames are written on
 * the device and downloaded once.  Frames after a stop repeat the stopped configuration where their steps were still enqueued;
 * where a status poll ended the enqueuing first, the caller's arrays are left as they were from there on.  Stresslet frames and the flow at probe points are recorded by
 * rbl_ensemble_run_observed (below), not here, and rbl_ensemble_step_moments is RBL_ERR_STATE after a run until a one-step call has
 * recorded again.
 *
 * check_every = k > 0: after every k steps the host reads the status block (a few bytes, one stream drain) and stops enqueuing
 * once the run has stopped; 0: never before the end -- a stopped run then still enqueues its remaining steps, which meet the
 * flagged configuration again, set flags and commit nothing.  RBL_RUN_CHECK_DEFAULT is 64: a drain every 64 steps is a fraction
 * of a percent of their time, and it bounds what a stopped run wastes to 64 steps; results do not depend on it.
 *
 * Outputs (any per-replica pointer may be NULL): accepted[R], rejected[R]; first_flags[R], the error word (internal bits) of the
 * replica's first rejected step, and first_status[R], the same as an RBL_ERR_* code (0: never rejected); iters_sum[R] and
 * resid_max[R] over the replica's accepted steps; F_sum[R 6 N_bod] (runs with prescribed bodies) the sum over the replica's
 * ACCEPTED steps of the load F the one-step call returns, added in step order by one thread per entry (bitwise reproducible): its
 * mean is the microrheology measurement.  steps_done: steps before the run stopped (n_steps if it never did); stopped_at: the
 * step that stopped it or -1; stop_replica: its first failing replica, -1 for a batch-level failure or none.  Under
 * RBL_RUN_STOP a replica whose word is set at the stopping step counts one rejection; nothing counts after a stop.
 *
 * Refused before the device is touched, rbl_last_error naming the argument -- RBL_ERR_ARG: NULL structs or a wrong size,
 * n_steps < 1, stride < 0, check_every < 0, on_error outside {0, 1}, both or neither of F_body and (prescribed, body_in),
 * entries of prescribed above 1, prescribed_per outside {0, 1, 6}, a Brownian run with prescribed_per = 6, max_iter < 1, rtol < 0, dt or delta not positive for a Brownian run, frame arrays NULL while
 * stride > 0 and n_frames > 0, a context with a communicator; RBL_ERR_SIZE: the solver's size refusals; RBL_ERR_STATE: no
 * ensemble configuration.  After a run rbl_ensemble_get_config and the one-step calls go on from its final configuration. */
#define RBL_RUN_STOP 0
#define RBL_RUN_REJECT 1
#define RBL_RUN_CHECK_DEFAULT 64
typedef struct rbl_run_opts {
  int64_t size;               /* sizeof(rbl_run_opts) */
  int32_t n_steps;            /* >= 1 */
  int32_t brownian;           /* 0: deterministic steps, else the stochastic midpoint step */
  int32_t split_rand;         /* as rbl_ensemble_step_brownian */
  int32_t max_iter;           /* >= 1 */
  int32_t stride;             /* >= 0; 0 records no frames */
  int32_t on_error;           /* RBL_RUN_STOP or RBL_RUN_REJECT */
  int32_t check_every;        /* >= 0 */
  int32_t prescribed_per;     /* mask entries per body: 0 or 1 whole bodies, 6 velocity components (deterministic runs only) */
  uint64_t seed;              /* step n draws from seed + n */
  double delta;               /* RFD step, as rbl_ensemble_step_brownian */
  double rtol;                /* >= 0 */
  const double *F_body;       /* [R 6 N_bod], or NULL with prescribed and body_in */
  const uint8_t *prescribed;  /* [R N_bod] 0/1 ([R 6 N_bod] with prescribed_per = 6), or NULL with F_body */
  const double *body_in;      /* [R 6 N_bod] */
  const double *slip;         /* [R n3] or NULL */
} rbl_run_opts;
typedef struct rbl_run_out {
  int64_t size;               /* sizeof(rbl_run_out) */
  int32_t *accepted, *rejected;          /* [R] */
  uint32_t *first_flags;                 /* [R] */
  int32_t *first_status;                 /* [R] */
  int64_t *iters_sum;                    /* [R] */
  double *resid_max;                     /* [R] */
  double *F_sum;                         /* [R 6 N_bod], runs with prescribed bodies */
  double *frame_X, *frame_Q;             /* [n_frames R 3 N_bod], [n_frames R 4 N_bod] */
  int32_t *frame_accepted_at;            /* [n_frames R] */
  double *frame_F;                       /* [n_frames R 6 N_bod], runs with prescribed bodies */
  int32_t steps_done, stopped_at, stop_replica, reserved;   /* written by the call */
} rbl_run_out;
int rbl_ensemble_run(rbl_ctx *ctx, const rbl_run_opts *opts, rbl_run_out *out);

/* A run with hard joints: n_steps steps of rbl_ensemble_step_jointed in ONE call.  Each step enqueues that call's launch sequence
 * (force and flow models at q^n, the right-hand side, one k_gmres_small_jt, the moments kernel while RBL_OPT_RECORD_MOMENTS is
 * on, the update), then the run's verdict and commit and ONE small launch for the joints (k_ens_jt_run, one thread per replica
 * and joint), which for the replicas that commit advances theta -- d = rate dt, theta += d, product and sum rounded one after
 * the other, only where rate != 0: the one-step call's bits --, advances the replica's position in the motor schedule, adds the
 * step's phi to phi_sum, and for every replica writes the rates of its next step into the joint table the solver reads.  The
 * joint table, F_body, slip, joint_velocity and the schedule go up once; the host synchronises at the check_every polls and at the
 * one read-back that ends the run.  A run that records frames launches k_ens_jt_geom once more on the recording steps.
 *
 * opts: n_steps, max_iter, rtol, stride, on_error, check_every, F_body and slip are read as rbl_ensemble_run reads them; both
 * error policies are that call's (RBL_RUN_STOP: the failing step commits nothing and turns no motor, nor does any later one;
 * RBL_RUN_REJECT: a failing replica keeps q^n, theta and its position in the cycle and tries again, and the new configuration is
 * validated before it commits).  prescribed, body_in and prescribed_per outside {0, 1} are RBL_ERR_ARG (joints with masks are
 * not offered); brownian != 0 while kBT > 1e-10 is RBL_ERR_ARG (the drift of a constrained suspension has not been derived;
 * brownian is ignored at kBT <= 1e-10); seed, split_rand and delta are not read.
 *
 * jopts: gamma and joint_velocity[R 3 n_joints] (or NULL) as in rbl_ensemble_step_jointed, constant over the run, and the motor
 * schedule, the one input that moves: a cycle of n_phases >= 0 phases, phase k lasting phase_steps[k] >= 1 steps with the rates
 * phase_rates[k][s][j] (s < rate_sets, 1: every replica alike, or R; finite, non-zero on RBL_JOINT_LOCK joints only:
 * rbl_ensemble_set_joint_rates' rule, the message naming phase, set and joint).  A replica at cycle position p steps with the
 * rates of the phase whose half-open range [cum_k, cum_k+1) of the prefix sums of phase_steps holds p; p advances by one, modulo
 * the cycle's length (which must fit 31 bits), when the replica commits -- a rejected replica's schedule waits for it, like its
 * field clock.  cycle_start[start_sets], start_sets 0 (every replica at 0), 1 or R: the positions at the run's first step,
 * 0 <= value < the cycle's length.  n_phases = 0: the rates rbl_ensemble_set_joint_rates stored, constant.  The schedule is an
 * argument, never state: after the run the stored rates are what rbl_ensemble_set_joint_rates last gave.
 *
 * jout (any pointer may be NULL): theta[R n_joints], the angles the run leaves (rbl_ensemble_joint_state returns the same);
 * cycle_pos[R], the positions at the run's end, so that a next run continues the stroke; phi_sum[R 3 n_joints], the sum over the
 * replica's ACCEPTED steps of the phi the one-step call returns, added in step order by one thread per entry: its mean over a
 * motor's lock rows is the motor's torque.  With stride > 0 the frames frame_theta[n_frames R n_joints], frame_phi and
 * frame_gap[n_frames R 3 n_joints]: phi is that step's, or the replica's last accepted one where it was rejected in that step
 * (zeros before any); the gap is k_ens_jt_geom's at the committed configuration and angles, the bits of rbl_ensemble_joint_state.
 * After a run that did not stop rbl_ensemble_joint_state returns every replica's last accepted phi; after a stopped run phi is
 * invalid, as after a failed step.  rbl_ensemble_step_moments is RBL_ERR_STATE after the run.
 *
 * Joints switched off or never set: the call is rbl_ensemble_run with brownian = 0, bit for bit; the schedule must then be empty
 * (RBL_ERR_STATE otherwise), cycle_pos is zeros and the other arrays of jout are left alone.
 * Refused before any device work: NULL structs or wrong sizes, the refusals above, those of rbl_ensemble_run for the fields that
 * are read, those of rbl_ensemble_step_jointed (gamma, dt, max_iter outside 1 .. 255, a joint naming a body >= N_bod, the size
 * refusals with the LDS message), n_phases < 0, rate_sets outside {1, R} or start_sets outside {0, 1, R}, NULL schedule arrays
 * while n_phases > 0, a phase_steps entry < 1, a cycle_start outside the cycle (RBL_ERR_ARG), a periodic cell that is on
 * (RBL_ERR_STATE, "periodic"), a communicator. */
typedef struct rbl_run_joint_opts {
  int64_t size;                 /* sizeof(rbl_run_joint_opts) */
  double gamma;                 /* in [0, 1] */
  const double *joint_velocity; /* [R 3 n_joints] or NULL */
  int32_t n_phases;             /* >= 0; 0: the stored rates, constant */
  int32_t rate_sets;            /* 1 or R (read while n_phases > 0) */
  int32_t start_sets;           /* 0, 1 or R */
  int32_t reserved;
  const int32_t *phase_steps;   /* [n_phases], each >= 1 */
  const double *phase_rates;    /* [n_phases rate_sets n_joints] */
  const int32_t *cycle_start;   /* [start_sets] */
} rbl_run_joint_opts;
typedef struct rbl_run_joint_out {
  int64_t size;                 /* sizeof(rbl_run_joint_out) */
  double *theta;                /* [R n_joints] */
  int32_t *cycle_pos;           /* [R] */
  double *phi_sum;              /* [R 3 n_joints] */
  double *frame_theta;          /* [n_frames R n_joints] */
  double *frame_phi, *frame_gap; /* [n_frames R 3 n_joints] */
} rbl_run_joint_out;
int rbl_ensemble_run_jointed(rbl_ctx *ctx, const rbl_run_opts *opts, const rbl_run_joint_opts *jopts, rbl_run_out *out,
                             rbl_run_joint_out *jout);
/* The schedule's map from a cycle position to its phase, as the run's kernel evaluates it (one __host__ __device__ function):
 * the k with cum_k <= pos < cum_k+1, or -1 for n_phases < 1, a NULL array, a phase_steps entry < 1 or pos outside the cycle.
 * No context. */
int rbl_run_schedule_phase(const int32_t *phase_steps, int n_phases, int64_t pos);

/* Observers: the flow at probe points and the first moments of lambda, for every replica (rigid_body_light_amd/csrc/rbl_ens_field.hip).
 *
 * The field.  For replica r and point p, section 6's definition with the replica's own blobs as sources,
 *     u_r(x_p) = nf d(z_p) sum_j sum_images M(x_p, r_j + image) d(z_j) lambda_{r,j},
 * the velocity apply_M would give a force-free blob of radius a at x_p: the same pair block and damping (rbl_set_no_damp is not
 * read: the ensemble's operator always damps), a point within 1e-12 a of a blob takes the self block, 0 < r < 2a the overlapping
 * form, with the wall a point at z_p <= 0 gets u = 0 and no error.  With the ensemble's cell on (rbl_ensemble_set_periodic) the
 * sum runs over the cell's images of every blob: the nearest-image displacement is formed once per (point, blob) as the solver
 * forms it, the (2 nx + 1)(2 ny + 1) images are the innermost loop, and only the (0, 0) image of a coincident blob is the self
 * block -- its other images are ordinary pairs.  This is the one flow field the library has in a periodic cell (section 6 refuses
 * its context's cell).  A blob below the wall is RBL_ERR_BELOW_WALL, a non-finite result RBL_ERR_NONFINITE, both latched in the
 * replica's own error word: the message names the first failing replica.
 * One kernel, k_ens_probe: grid (point tiles, R); the replica's N <= 256 blobs are placed from (X, Q, reference configuration)
 * term for term as k_body_geom places them and staged once per workgroup in LDS (48 B each); one point per lane and register set,
 * NI sets per lane; every point sums over the blobs in index order, then the images p, then q.  No atomics on doubles: two calls
 * agree bitwise, replica r of R returns the bits of the R = 1 call, and a point's bits do not depend on the launch geometry.
 *
 *   rbl_ensemble_velocity_field      at the ensemble's CURRENT configuration.  points[point_sets 3 P], point_sets 1 (one set for
 *                                    every replica) or R; lambda[R 3 N] (N = N_bod N_blb; e.g. rbl_ensemble_solve_jointed's);
 *                                    u[R 3 P].  probe_body = -1: lab points.  probe_body = b >= 0: points are offsets s_p fixed in
 *                                    body b, placed at X_b + R(Q_b) s_p of the replica's configuration; u stays in lab-frame
 *                                    components and nothing is subtracted.  Host arrays, synchronous.
 *   rbl_ensemble_velocity_field_dev  the same with device pointers; the kernel is enqueued on the context's stream and the call
 *                                    returns once the replicas' error words have been read.
 *   rbl_ensemble_probe_info          the launch geometry of n_points points on this context's ensemble: points per lane (1, 2 or
 *                                    4), waves per workgroup (1 .. 4), point tiles.  One function of (n_points, R, CU count).
 * n_points == 0 does nothing (RBL_OK).  RBL_ERR_ARG: NULL arrays, n_points < 0, point_sets outside {1, R}, probe_body outside
 * [-1, N_bod), a non-finite coordinate (host form; the message names set and point); RBL_ERR_STATE: no ensemble configuration.
 *
 * Observed runs.  rbl_ensemble_run_observed is rbl_ensemble_run (jopts == NULL; jout is then ignored) or rbl_ensemble_run_jointed
 * with up to two observers evaluated inside every step, on that step's lambda while it lies in the solver's workspace and at the
 * configuration the solve was taken at -- q^n for deterministic and jointed steps, q^{n+1/2} for the Brownian step, the convention
 * of RBL_OPT_RECORD_MOMENTS (section 8): the probe kernel when n_probes > 0 (points, point_sets, probe_body as above; body-frame
 * points follow the body from step to step) and section 8's moments kernel when moments != 0.  Both run just before the update;
 * the probe kernel's flags go into the replica's error word, so a step with a non-finite field is that replica's failed step.
 * They enter it (one small launch, k_ens_obs_flags, a thread per replica) only where the step has not failed already: a replica
 * whose solve has failed -- say, a blob below the wall at the midpoint, which leaves a non-finite lambda -- keeps the word, and
 * with it first_flags and first_status, that the unobserved run gives it.
 * One more launch per quantity, k_ens_obs_commit (one thread per entry, after the run's commit), follows the commit's decision
 * per replica: where the replica committed the step's u and D are added to u_sum / D_sum, in step order, and remembered; on a
 * recording step the frame takes this step's value, the last accepted one where the replica was rejected in that step, zeros
 * before any accepted step (frame_F's convention).  Nothing is added from the stopping step on.  The sums divide by accepted[].
 * A Brownian step's lambda holds the thermal part: u and D are instantaneous values whose MEAN is the measurement, and, as in
 * section 8, the drift's share of the stress is not added.  The symmetric traceless part of D_sum / accepted is the mean stresslet.
 * The observers are arguments, never state: rbl_ensemble_step_moments stays RBL_ERR_STATE after a plain run and is untouched
 * after a jointed one.  With n_probes == 0 and moments == 0 the call is the underlying run, bit for bit and launch for launch.
 * Refused before any device work, rbl_last_error naming the argument -- RBL_ERR_ARG: NULL obs or oout or a wrong size,
 * n_probes < 0, points NULL while n_probes > 0, point_sets outside {1, R}, probe_body outside [-1, N_bod), a non-finite
 * coordinate (set and point named), frame_u (n_probes > 0) or frame_D (moments) NULL while stride > 0 records frames; then
 * everything the underlying run refuses.  u_sum and D_sum may be NULL. */
typedef struct rbl_run_obs_opts {
  int64_t size;               /* sizeof(rbl_run_obs_opts) */
  int32_t n_probes;           /* P >= 0; 0: no field */
  int32_t point_sets;         /* 1 or R (read while n_probes > 0) */
  int32_t probe_body;         /* -1: lab points; b >= 0: offsets fixed in body b */
  int32_t moments;            /* != 0: first moments of every step's lambda */
  const double *points;       /* [point_sets 3 P] */
} rbl_run_obs_opts;
typedef struct rbl_run_obs_out {
  int64_t size;               /* sizeof(rbl_run_obs_out) */
  double *u_sum;              /* [R 3 P] */
  double *D_sum;              /* [R 9 N_bod] */
  double *frame_u;            /* [n_frames R 3 P] */
  double *frame_D;            /* [n_frames R 9 N_bod] */
} rbl_run_obs_out;
int rbl_ensemble_velocity_field(rbl_ctx *ctx, const double *points, int64_t n_points, int point_sets, int probe_body,
                                const double *lambda, double *u);
int rbl_ensemble_velocity_field_dev(rbl_ctx *ctx, const double *d_points, int64_t n_points, int point_sets, int probe_body,
                                    const double *d_lambda, double *d_u);
int rbl_ensemble_probe_info(const rbl_ctx *ctx, int64_t n_points, int *ni, int *waves, int64_t *tiles);
int rbl_ensemble_run_observed(rbl_ctx *ctx, const rbl_run_opts *opts, const rbl_run_joint_opts *jopts, const rbl_run_obs_opts *obs,
                              rbl_run_out *out, rbl_run_joint_out *jout, rbl_run_obs_out *oout);

/* Driven runs: the one body input of a run that moves with time (rigid_body_light_amd/csrc/rbl_ens_drive.hip).
 *
 * rbl_ensemble_run keeps everything it is given constant over the run.  rbl_ensemble_run_driven is that run (with observers
 * when obs is not NULL, as rbl_ensemble_run_observed without joints) whose body input -- F_body of a run with all bodies free,
 * body_in of a masked run: velocities on prescribed bodies or components, loads on free ones -- is evaluated anew before every
 * step, per replica.  For replica r at a step that starts with accepted[r] = n and cycle position p_r the 6 N_bod entries are
 *     in_r = ((A0_r + P_r[phase(p_r)]) + C_r cos(w_r t_r)) + S_r sin(w_r t_r),     t_r = t0_r + dt n.
 * A0: opts->F_body or opts->body_in, the array a plain run holds constant.  cos_amp (C) and sin_amp (S): [amp_sets 6 N_bod],
 * amp_sets 1 (every replica alike) or R; either may be NULL: zeros.  omega[omega_sets], omega_sets 1 or R: one frequency per
 * replica, so R replicas are R points of a spectrum in one call.  t0[t0_sets], t0_sets 0 (t0 = 0), 1 or R.  P: a periodic
 * piecewise-constant part, n_phases >= 0 phases, phase k lasting phase_steps[k] >= 1 steps with phase_in[k][s][6 N_bod]
 * (s < phase_sets, 1 or R), read through the schedule map of rbl_ensemble_run_jointed (rbl_run_schedule_phase): the position
 * starts at cycle_start[start_sets] (start_sets 0: every replica at 0, 1 or R) and moves on by one, modulo the cycle's length,
 * when the replica commits -- a rejected replica's schedule and clock wait for it.  n_phases = 0: P = 0.
 * The arithmetic is fixed: dt n and the sum with t0 are two separately rounded operations (the field clock's, section 4),
 * w t is one rounded product followed by ONE sincos, the products C cs and S sn are rounded, and the three additions are made
 * in the order written, nothing contracted; absent parts enter as zeros.  So omega = 0 with S = 0 gives the bits of
 * (A0 + P) + C.  The drive is an argument, never state; the mask, slip, force model and flow model stay constant as before.
 *
 * Two launches per step beside the run's own: k_ens_drive before the step's sequence (one thread per entry of [R 6 N_bod];
 * the evaluated input goes into the buffer the step reads, A0 stays in one of its own; cs, sn per replica into a small table)
 * and k_ens_drive_commit after the run's commit and the observers' (one thread per entry; it takes the commit's own decision
 * from the run's status and the replica's verdict word, advances the cycle position and adds the lock-in sums).
 *
 * Lock-in sums (lockin != 0): for every step a replica commits, with the step's own cs = cos(w_r t_r), sn = sin(w_r t_r) --
 * the values the drive was evaluated with --, each entry added by one thread, in step order, product and sum rounded one
 * after the other:  X_c, X_s [R 3 N_bod] = sum X(q^n) cs / sn with the body centres of the configuration the step started
 * from;  U_c, U_s [R 6 N_bod] the same of the step's body velocities (what the update reads);  F_c, F_s [R 6 N_bod] the same of
 * the masked solve's loads (masked runs; left alone otherwise);  norm [R 5] = sum cs, sum sn, sum cs^2, sum sn^2, sum cs sn,
 * with which amplitude and phase are fitted exactly in discrete time.  Nothing is added from a stopping step on.
 * cycle_pos[R] and t_end[R] = t0 + dt accepted come back, so that a second run (cycle_start = cycle_pos, t0 = t_end)
 * continues the first: bit for bit where the clock arithmetic is exact (a dyadic dt and t0), otherwise t_end + dt m and
 * t0 + dt (n + m) are two roundings of one number.  Any pointer of dout may be NULL.
 *
 * Contracts: a driven run is, bit for bit, the loop of rbl_ensemble_drive_eval followed by the one-step call; replica r of R
 * is the R = 1 run with that replica's inputs; drive == NULL, or a drive with neither C nor S, no phases and lockin == 0, is the
 * underlying run bit for bit and launch for launch (cycle_pos is then zeros, t_end = t0 + dt accepted, the sums are left alone).
 *
 * rbl_ensemble_drive_eval: the same kernel, one launch and a read-back.  base[R 6 N_bod] stands for A0, accepted[R] (NULL:
 * zeros) and cycle_pos[R] (NULL: cycle_start) for the replicas' counters; in_out[R 6 N_bod] takes the evaluated input and
 * cs_sn[R 2] (may be NULL) the pair the kernel evaluated it with.  The device's sincos is not the host's: this call is what
 * lets a loop of one-step calls reproduce a driven run.
 *
 * Refused before any device work, rbl_last_error naming the argument -- RBL_ERR_ARG: a wrong struct size, dout NULL with a
 * non-empty drive, amp_sets or omega_sets outside {1, R}, t0_sets or start_sets outside {0, 1, R}, phase_sets outside {1, R},
 * n_phases < 0, omega NULL with a harmonic part or lockin, t0, phase_steps, phase_in or cycle_start NULL where its count says
 * it is read, a non-finite entry of cos_amp, sin_amp, omega, t0 or phase_in (set and entry named), a phase_steps entry < 1, a
 * cycle longer than 31 bits, a cycle_start outside the cycle, a harmonic part or lockin while dt <= 0; then everything the
 * underlying run refuses, unchanged (a Brownian run with prescribed_per = 6 and a communicator among them); RBL_ERR_STATE: hard
 * joints are switched on and the drive is not empty (drives for rbl_ensemble_run_jointed are not offered). */
typedef struct rbl_run_drive_opts {
  int64_t size;                 /* sizeof(rbl_run_drive_opts) */
  int32_t amp_sets;             /* 1 or R (read while cos_amp or sin_amp is given) */
  int32_t omega_sets;           /* 1 or R (read while omega is given) */
  int32_t t0_sets;              /* 0, 1 or R */
  int32_t n_phases;             /* >= 0 */
  int32_t phase_sets;           /* 1 or R (read while n_phases > 0) */
  int32_t start_sets;           /* 0, 1 or R */
  int32_t lockin;               /* != 0: the lock-in sums */
  int32_t reserved;
  const double *cos_amp;        /* C [amp_sets 6 N_bod] or NULL */
  const double *sin_amp;        /* S [amp_sets 6 N_bod] or NULL */
  const double *omega;          /* [omega_sets]; NULL without a harmonic part and lockin: 0 */
  const double *t0;             /* [t0_sets] */
  const int32_t *phase_steps;   /* [n_phases], each >= 1 */
  const double *phase_in;       /* [n_phases phase_sets 6 N_bod] */
  const int32_t *cycle_start;   /* [start_sets] */
} rbl_run_drive_opts;
typedef struct rbl_run_drive_out {
  int64_t size;                 /* sizeof(rbl_run_drive_out) */
  double *X_c, *X_s;            /* [R 3 N_bod] */
  double *U_c, *U_s;            /* [R 6 N_bod] */
  double *F_c, *F_s;            /* [R 6 N_bod], masked runs */
  double *norm;                 /* [R 5] */
  int32_t *cycle_pos;           /* [R] */
  double *t_end;                /* [R] */
} rbl_run_drive_out;
int rbl_ensemble_run_driven(rbl_ctx *ctx, const rbl_run_opts *opts, const rbl_run_drive_opts *drive, const rbl_run_obs_opts *obs,
                            rbl_run_out *out, rbl_run_drive_out *dout, rbl_run_obs_out *oout);
int rbl_ensemble_drive_eval(rbl_ctx *ctx, const rbl_run_drive_opts *drive, const double *base, const int32_t *accepted,
                            const int32_t *cycle_pos, double *in_out, double *cs_sn);

/* Metropolis sampling of the force model (rigid_body_light_amd/csrc/rbl_ens_mc.hip): rbl_ensemble_mc runs n_sweeps Metropolis
 * sweeps on every replica of the ensemble's current configuration and leaves the result as the current configuration, from
 * which every step family continues as from rbl_ensemble_set_config of the same numbers -- up to that call's own normalisation of
 * the quaternions, which the chain's result does not go through again: where set_config would move the last bit of a quaternion
 * the chain left (it divides by a norm that is 1 only to rounding), the two continuations differ by that bit's consequence and are
 * bitwise equal otherwise.  No mobility is involved: the chain
 * samples exp(-E / kBT) of the total energy E that rbl_ensemble_interaction_forces reports, for equilibrated starting
 * configurations and as the reference of the stationary distribution of the Brownian steps.
 *
 * Sweeps and trials.  One sweep is N_bod trials, body b = 0 .. N_bod - 1 in that order.  A fixed order preserves the stationary
 * distribution (every trial does); it is NOT detailed balance of the sweep, nor a random-scan chain.  The trial of body b in
 * replica r at the global sweep index S = sweep_start + s draws 7 uniforms from Philox-4x32-10, the generator of the steps'
 * noise, with the key (k0, k1) = (low, high word of seed) and the two counters
 *     c = { low word of S, high word of S, replica_base + r, 0x4D430000 | j << 8 | b },  j = 0, 1
 * (b < 64; the steps' normals use c[3] = 0, so the streams never meet): block j = 0 gives the words w0..w3, block j = 1 the
 * words w4..w6 (its fourth word is unused).  A word becomes u = (w + 0.5) 2^-32, 0 < u < 1.  The counter depends on
 * (replica_base + r, S, b) and on nothing else -- not on R, on the launch split, or on what other bodies did.
 * Proposal: dX = step_x (2 u_{0,1,2} - 1), a rotation vector phi = step_theta (2 u_{3,4,5} - 1) in the lab frame, and
 * q' = update_X_Q(q, (dX, phi)): the library's own body update (the rotation quaternion of phi multiplied from the left, then
 * normalised).  The proposal density is symmetric under (dX, phi) -> -(dX, phi): no Hastings factor.  u_6 decides: the trial is
 * accepted iff dE <= 0 or u_6 < exp(-dE / kBT_r).  kBT: kBT_sets = 0 the context's, 1 one value, R one value per replica (a
 * temperature sweep in one call); every value finite and > 0.
 * Energy.  dE is the change of the total energy of section 4 restricted to what body b takes part in: weight, wall repulsion
 * and height table of b's blobs; steric term, pair table and type tables between b's blobs and the blobs of the replica's other
 * bodies, each inside its own cutoff; b's trap; the bonds and tethers that end on b -- bits 0, 1, 2, 3, 6 and 7 of
 * rbl_interactions_active, with the definitions of section 4 (tangent continuations, unshifted cutoffs, the r = 0 rules), the
 * kernels sharing the force kernels' expressions.  Replica-indexed inputs are read as the force evaluation reads them (trap
 * sets, bond parameter sets, a cell per replica).  With the ensemble's cell on, shared or per replica, pair displacements take
 * the minimum image and bonds stay unwrapped, as in the force kernels.  Dipole pairs and the field torque (bits 4, 5) are not
 * offered: RBL_ERR_STATE, the term named, while either is active.  Nor are hard joints (constrained sampling), moves of more
 * than one body, cluster or swap moves, replica exchange, or a single context without an ensemble.
 * Domain.  With the wall on (rbl_set_wall_pc) a trial that puts any blob of b at z < 0 is rejected without an energy
 * evaluation and counted in wall_rejected (the mobility is undefined there); a starting configuration with a blob below the
 * wall is RBL_ERR_BELOW_WALL, the replica named, and nothing moves.
 * frozen: an optional byte mask, frozen_sets = 1 (N_bod entries) or R (R N_bod): a frozen body is never tried, keeps its bits
 * and still acts on the others.
 * Sizes: a replica is what rbl_ensemble_set_config accepts, the one-kernel solver's size rule (about 75 N_blobs + 60 N_bod doubles
 * within 150 KB of LDS): at most 19 shells of 12 blobs, 53 tetrahedra, or one body of 238 blobs.  The kernel's arrays are sized for
 * the layout's bound of 256 blobs and 64 bodies, which no ensemble reaches; the call asks the size rule again (RBL_ERR_SIZE).
 * Outputs, host arrays, any may be NULL; the flags, counters and energies come back in one read-back, frames and trace follow
 * once the call has succeeded (a refused call leaves the caller's arrays alone): tried, accepted, wall_rejected [R] (int64);
 * energy_start [R], the energy of rbl_ensemble_interaction_forces at the start (that evaluation, summed in its order);
 * energy_end [R] = energy_start plus the accepted dE in trial order; with stride > 0 the n_sweeps / stride frames after every
 * stride-th sweep of the call, frame_X [n_frames R 3 N_bod], frame_Q [n_frames R 4 N_bod], frame_E [n_frames R] (all three
 * required then); with n_trace > 0 the first n_trace trials of every replica, trace [R n_trace 10]: body, dX (3), phi (3),
 * dE, u_6, verdict (0 rejected, 1 accepted, 2 rejected at the wall: dE = 0, not evaluated; rows beyond the trials made: -1).
 * Contracts: the call is bitwise reproducible (one workgroup per replica, one summation order, no atomics on doubles); n1 + n2
 * sweeps give the configuration and the counters of n1 sweeps followed by n2 sweeps with sweep_start = n1 (energy_end agrees to
 * rounding: the second call starts from its own evaluation); replica r of R is the R = 1 ensemble of that replica with
 * replica_base = r; the host splits a chain into ceil(n_sweeps / RBL_OPT_MC_SWEEPS_PER_LAUNCH) launches, invisible in every bit.
 * Refused before any device work, RBL_ERR_ARG with the argument named: NULL structs or a wrong size, n_sweeps < 1, step_x or
 * step_theta negative or non-finite, a kBT <= 0 or non-finite (kBT NULL with kBT_sets > 0), kBT_sets or frozen_sets negative
 * or neither 1 nor R, stride < 0, n_trace < 0, sweep_start < 0, replica_base < 0 or replica_base + R > 2^31, frame arrays NULL
 * with n_frames > 0, trace NULL with n_trace > 0, a context with a communicator; RBL_ERR_STATE: hard joints switched on, a
 * dipole term active, no term of the force model on, no ensemble configuration.  On any error nothing moves. */
typedef struct rbl_mc_opts {
  int64_t size;               /* sizeof(rbl_mc_opts) */
  int64_t n_sweeps;           /* >= 1 */
  int64_t sweep_start;        /* >= 0: the global index of the call's first sweep */
  uint64_t seed;
  double step_x, step_theta;  /* >= 0 */
  int32_t replica_base;       /* >= 0 */
  int32_t kBT_sets;           /* 0 (the context's kBT), 1 or R */
  int32_t frozen_sets;        /* 0 (none frozen), 1 or R */
  int32_t stride;             /* >= 0; 0 records no frames */
  int32_t n_trace;            /* >= 0 */
  int32_t reserved;
  const double *kBT;          /* [kBT_sets] */
  const uint8_t *frozen;      /* [frozen_sets N_bod] */
} rbl_mc_opts;
typedef struct rbl_mc_out {
  int64_t size;               /* sizeof(rbl_mc_out) */
  int64_t *tried, *accepted, *wall_rejected;   /* [R] */
  double *energy_start, *energy_end;           /* [R] */
  double *frame_X, *frame_Q, *frame_E;         /* [n_frames R 3 N_bod], [n_frames R 4 N_bod], [n_frames R] */
  double *trace;                               /* [R n_trace 10] */
} rbl_mc_out;
int rbl_ensemble_mc(rbl_ctx *ctx, const rbl_mc_opts *opts, rbl_mc_out *out);

/* ===================================================================== */
/* 6. Fluid velocity at arbitrary points (rigid_body_light_amd/csrc/rbl_field.hip) */
/* ===================================================================== */
/* The flow the blob forces lambda (e.g. the lambda of a saddle solve [M -K; K^T 0][lambda; U] = [slip; -F]) drive at P points
 * x_p: the velocity apply_M would give an extra force-free blob of the context's radius a placed at x_p,
 *     u(x_p) = nf d(z_p) sum_j M(x_p, r_j) d(z_j) lambda_j,     nf = 1 / (8 pi eta a),
 * with the pair block M of apply_M (free space, or wall-corrected per rbl_set_wall_pc) and its damping d (c_rigid_obj.cpp:618-639;
 * rbl_set_no_damp is honoured).  A point within 1e-12 a of a blob takes the self block (no RBL_ERR_OVERLAP): a point placed on a
 * blob returns that blob's apply_M row.  0 < r < 2a takes the overlapping RPY form, as apply_M.  With the wall, a point at z <= 0
 * gets u = 0 (the fluid is z > 0; the damping already takes u to 0 at z = 0) -- no error.  A blob below the wall is
 * RBL_ERR_BELOW_WALL as in apply_M; a non-finite result is RBL_ERR_NONFINITE.
 * The tracer radius is a.  Point probes (radius 0) and other tracer radii are not offered: the free-space RPY tensor of unequal
 * radii is textbook, but its single-wall correction has nothing in this library or the reference to be checked against.
 *
 *   rbl_velocity_field      host arrays: points[3 P], lambda[3 n_src], r_vecs[3 n_src] or NULL, u[3 P] (synchronous).
 *                           r_vecs == NULL: the context's own blobs at the current configuration (n_src must be N_bod N_blb).
 *   rbl_velocity_field_dev  the same arguments as device pointers, enqueued on the context's stream; u stays on the device
 *                           (errors latched in the device word: rbl_sync_check)
 *   rbl_velocity_field_info the split the product of (n_points, n_src) takes on this context: points per lane (2 or 4), chunks the
 *                           sources are cut into (their partial sums added in fixed order), device workspace in bytes
 * Null or negative arguments, or r_vecs == NULL with another n_src, are RBL_ERR_ARG; n_points == 0 does nothing (RBL_OK).
 * Bitwise reproducible (no float atomics).  Under a communicator every rank evaluates a contiguous share of the points and one
 * all-gather completes u on every rank; the source split depends on the total point count only, so u is bitwise the same at any
 * rank count. */
int rbl_velocity_field(rbl_ctx *ctx, const double *points, int64_t n_points, const double *lambda, const double *r_vecs,
                       int64_t n_src, double *u);
int rbl_velocity_field_dev(rbl_ctx *ctx, const double *d_points, int64_t n_points, const double *d_lambda, const double *d_r_vecs,
                           int64_t n_src, double *d_u);
int rbl_velocity_field_info(const rbl_ctx *ctx, int64_t n_points, int64_t n_src, int *ni, int *chunks, int64_t *workspace_bytes);

/* ===================================================================== */
/* 7. Prescribed kinematics (rigid_body_light_amd/csrc/rbl_mixed.hip)     */
/* ===================================================================== */
/* Every other solver answers "given the loads on all bodies, how do they move?".  Here any subset p of the bodies has its
 * velocity PRESCRIBED (held: U = 0; driven: U given) while the others (f) stay free; the reference has no such solver.  With
 * K = [K_f K_p] the blob forces lambda and the free velocities U_f solve
 *     M lambda - K_f U_f = slip + K_p U_p        (no slip on every blob, prescribed bodies moving as told)
 *     K_f^T lambda       = -F_f                  (force and torque balance of the free bodies only)
 * and the by-product is the load the prescribed bodies need, F_p = -K_p^T lambda, in the convention of the F_body argument of
 * rbl_step_deterministic (rhs = [slip; -F]): if a mobility solve with loads F gives velocities U, prescribing that U on a set p
 * and keeping F on the rest returns the same lambda, the same U_f and F_p = F on p.  M is what rbl_apply_saddle applies on the
 * context's configuration.  p empty: the saddle system; f empty: M lambda = slip + K U, the resistance problem.
 *
 * The set travels with each call (prescribed[N_bod], 0 = free, 1 = prescribed) and is never context state: no other entry point
 * changes meaning.  body_in[6 N_bod] holds, body by body, the load F_b of a free body or the velocity U_b (translation, rotation)
 * of a prescribed one.  Outputs: U[6 N_bod] all body velocities (prescribed ones echoed), F[6 N_bod] all body loads (free ones
 * echoed, prescribed ones = -K_b^T lambda), lambda[3 N_blobs] (may be NULL) the blob forces -- what rbl_velocity_field takes.
 *
 * Cost: an ITERATION costs what an iteration of the unconstrained solve costs; a solve needs more of them the more bodies are
 * prescribed (nothing but M_b^-1 preconditions M on a prescribed body): 17 / 33 / 60 iterations to 1e-8 for none / a quarter /
 * all of 200 x 642-blob bodies above the wall with the block preconditioner.
 * Solver: the right-preconditioned GMRES of rbl_gmres_saddle_dev (no restart, max_iter <= 255, cold start) on
 *     [M lambda - K (D_f U) ; D_f K^T lambda + D_p U]     (D_f, D_p: 0/1 per body; the slots of prescribed bodies solve to 0)
 * with the context's preconditioner body by body: a free body as rbl_apply_PC treats it with the force block's sign restored
 * (the exact inverse of [M_b -K_b; K_b^T 0]), a prescribed one lambda_b = M_b^-1 slip_b with its six body slots passed through.
 * The residual estimate is relative to |[slip + K_p U_p ; F_f]|.  One iteration costs what an ordinary one costs: one mobility
 * product, one pass over the per-body factors (two with the free-space body-frame tables when a body is prescribed).
 *
 *   rbl_solve_mixed      host arrays, synchronous.
 *   rbl_solve_mixed_dev  body_in, slip, lambda, U, F are device pointers; `prescribed` stays a HOST array (N_bod bytes, checked
 *                        before any device work and copied, so it may go after the call); enqueued on the context's stream.
 *                        The call drains the stream where rbl_gmres_saddle_dev does -- once while the preconditioner of the
 *                        configuration is made ready (rbl_prepare_dev), at the solver's convergence tests and at its end --
 *                        and nowhere else; the copies into d_lambda, d_U, d_F are enqueued behind the solve and not waited
 *                        for.  Errors are latched in the device word (rbl_sync_check).
 *   rbl_step_mixed       host arrays: the solve at the current configuration, then evolve_X_Q(U) -- prescribed bodies advance by
 *                        their own velocity (a held body does not move).  F (may be NULL) as above.  With the force model on
 *                        (section 4) the step adds the model's loads at q^n, -K^T f_phys, to the FREE bodies' slots only: a
 *                        prescribed body's motion does not depend on the loads on it and its slots hold velocities.  The F
 *                        returned for a prescribed body is therefore the TOTAL load that everything other than the fluid
 *                        supplies: the model already supplies its share (rbl_interaction_forces returns it as PHYSICAL forces,
 *                        i.e. with the opposite sign: share = -FT_body), the outside agent supplies F minus that share.
 *                        The step clears the warm-start history of rbl_step_deterministic.
 * slip: 3 N_blobs or NULL for zero.  Status codes as the other solvers.  A NULL prescribed / body_in / U / F (rbl_step_mixed: F
 * may be NULL), max_iter < 1, rtol < 0 and entries of `prescribed` other than 0 / 1 are RBL_ERR_ARG before any device work; so
 * is a context with a communicator (as for the ensembles) -- sharding the mixed solve is a follow-up.  Results are bitwise
 * reproducible call to call (no float atomics).
 *
 * The Brownian midpoint step with prescribed bodies (kBT > 0): rbl_step_brownian with K -> K_f.  With D_f, D_p the 0/1 selectors
 * of the free and prescribed bodies' six slots and Kinv = (K^T K)^-1 K^T per body, from q^n:
 *     M^{1/2}W1 (and M^{1/2}W2 with split_rand) at q^n: the blob mobility of ALL blobs, the mask does not enter;
 *     dq = D_f Kinv W_rfd (prescribed bodies are not displaced),  M_RFD = (1/delta)[M(q + delta/2 dq) - M(q - delta/2 dq)] W_rfd;
 *     s = slip - kBT M_RFD - BI,  c1, c2, BI as in rbl_RHS_and_Midpoint_dev;
 *     q^{n+1/2} = q^n displaced by D_f (dt/2) c1 Kinv M^{1/2}W1 + D_p (dt/2) U_p  (a driven body at its own half step, a held
 *     one stays);
 *     the mixed solve above at q^{n+1/2} with slip = s and the same body_in (K_p U_p with the midpoint lever arms);
 *     q^n restored (also on failure), evolve_X_Q(U): a prescribed body advances by exactly dt U_p.
 * Eliminating lambda, U_f = -Ntilde (F_f + K_f^T M^-1 rhs_top) with Ntilde = (K_f^T M^-1 K_f)^-1: the noise of U_f has covariance
 * (2 kBT / dt) Ntilde and the midpoint and RFD terms give the drift kBT div_{q_f} Ntilde (the argument of the all-free step with
 * K_f for K; K_b depends on q_b only); the masks keep the random displacements inside the free coordinates.
 *
 *   rbl_RHS_and_Midpoint_mixed      host arrays: s[3 N_blobs], X_half[3 N_bod], Q_half[4 N_bod]; nothing is committed.  Of body_in
 *                        only the prescribed bodies' velocities are read.  W = [W1 | W2 | W_rfd] (9 N_blobs) or NULL: drawn from
 *                        `seed` as rbl_step_brownian draws them.  kBT <= 1e-10: s = slip, q^{n+1/2} = q^n.
 *   rbl_RHS_and_Midpoint_mixed_dev  d_body_in, d_slip (may be NULL), d_W (may be NULL), d_s are device pointers; `prescribed`,
 *                        X_half and Q_half stay host arrays.  d_s may be d_slip.  One small read-back (12 numbers per body).
 *   rbl_step_brownian_mixed         host arrays: the whole step; F (may be NULL), iters, resid as rbl_step_mixed -- the F of a held
 *                        body is its instantaneous load, thermal part included (what a microrheology measurement averages).  The
 *                        force model enters as in rbl_step_mixed: at q^n, the free bodies only.  kBT <= 1e-10: rbl_step_mixed.
 *                        s never leaves the device; beyond rbl_step_brownian's and rbl_step_mixed's own traffic the host sees
 *                        the mask, body_in and 12 numbers per body.
 * Their refusals are those above plus max_iter > 254 and, when kBT > 1e-10, dt <= 0 or delta <= 0: RBL_ERR_ARG before any device
 * work.
 * Ensembles of replicas with prescribed bodies are section 5's rbl_ensemble_*_mixed.
 *
 * Prescribed kinematics per velocity component (per-component constraints: the _dof entry points).  A microroller has its
 * angular velocity about a lab axis imposed and translates freely; a trapped particle is held in place and rotates freely; a
 * quasi-2D suspension has U_z = 0.  Here D_p and D_f = I - D_p are diagonal 0/1 selectors on each body's six LAB-frame components, in the order of body_in (translation
 * x, y, z, then rotation x, y, z):
 *     M lambda - K D_f U    = slip + K D_p U_in
 *     D_f K^T lambda + D_p U = -D_f F_in          (a prescribed slot: the identity, right-hand side 0)
 * prescribed6[6 N_bod] (0 = free, 1 = prescribed, component by component); body_in[6 N_bod] holds the load of a free component or
 * the velocity of a prescribed one; U = D_f U_solved + D_p U_in (prescribed components echoed), F = D_f F_in + D_p (-K^T lambda)
 * (free components echoed; a prescribed component: the force or torque along it that holds the motion), lambda as above.  Signs,
 * the residual (relative to the physical right-hand side; prescribed slots stay 0 in every Krylov vector) and the solver are
 * those above, and with all six entries of every body equal the system, the iteration count and the results are rbl_solve_mixed's.
 * The preconditioner stays the exact inverse of a body's own block in all three modes: with y1 = M_b^-1 slip_b, f = K_b^T y1 and
 * R_b = K_b^T M_b^-1 K_b (its diagonal-mobility stand-in under the diagonal preconditioner),
 *     (D_f R_b D_f + D_p) u = D_f (g - f) + D_p g,    lambda_b = y1 + (M_b^-1 K_b) D_f u,    the body slots take u.
 * The masked 6 x 6 Cholesky factors are made once per solve by one small launch (from the context's own factors; with the
 * free-space body-frame tables the one shared factor is first taken to each body's lab frame) and an iteration launches what an
 * iteration of rbl_solve_mixed launches: one mobility product and one pass over the per-body factors, two with the free-space
 * body-frame tables when anything is prescribed.  Its time per iteration over rbl_solve_mixed's with every body
 * prescribed: 1.03-1.05 at cfg 2, 1.001-1.004 at cfg 3, wall (tools/bench_prescribed_dof.py, profiles/prescribed_dof.jsonl).
 *
 *   rbl_solve_mixed_dof      host arrays, synchronous.
 *   rbl_solve_mixed_dof_dev  device pointers as rbl_solve_mixed_dev; prescribed6 stays a HOST array (6 N_bod bytes, checked
 *                            before any device work and copied); stream drains and error latching as there.
 *   rbl_step_mixed_dof       the solve, then evolve_X_Q(U): a body with its three translations held keeps its position exactly
 *                            while it turns.  The force model's loads at q^n are added to the FREE COMPONENTS only, so the F of
 *                            a prescribed component is the TOTAL load along it, as in rbl_step_mixed.  Clears the warm-start
 *                            history.
 * Refused with RBL_ERR_ARG before any device work: a NULL prescribed6 / body_in / U / F (rbl_step_mixed_dof: F may be NULL),
 * max_iter < 1, rtol < 0, more than 255 iterations, an entry of prescribed6 above 1, a context with a communicator.
 *
 * The Brownian midpoint step with a mask per velocity component (kBT > 0), for the masks in which every body's three ROTATION
 * entries (3..5 of its row) are all 0 or all 1; the translation entries are free to choose.  That covers a quasi-2D layer
 * (U_z = 0), a trapped probe held in place and free to turn, and a roller with Omega imposed whose translation diffuses.  For such
 * a mask the free velocity components ARE a subset of the coordinates: translation components are Cartesian coordinates, and a
 * whole rotation is either untouched or treated as the all-free step treats it.  The reference configuration has its mean removed,
 * so each body's K^T K is block diagonal -- n I for the translation, no translation-rotation coupling -- and (K D_f)^+ = D_f Kinv:
 * the random displacements D_f Kinv W stay inside the free coordinates.  The whole-body argument above then carries over with
 * K_f = K D_f: the free components' velocity has covariance (2 kBT / dt) Ntilde, Ntilde = ((K D_f)^T M^-1 K D_f)^-1 on the free
 * slots, and the drift kBT div_{q_f} Ntilde.  The scheme is the one above with D_f, D_p diagonal over the 6 N_bod slots:
 *     dq = D_f Kinv W_rfd;  q^{n+1/2} = q^n displaced by D_f (dt/2) c1 Kinv M^{1/2}W1 + D_p (dt/2) U_p, component by component in ONE
 *     update_X_Q;  the rbl_solve_mixed_dof system at q^{n+1/2} with slip = s and the same body_in (K D_p U_in with the midpoint
 *     lever arms);  q^n restored (also on failure), evolve_X_Q(U): a prescribed component advances by exactly dt U_p.
 *   rbl_RHS_and_Midpoint_mixed_dof, rbl_RHS_and_Midpoint_mixed_dof_dev, rbl_step_brownian_mixed_dof
 *                        the argument lists and conventions of the three whole-body calls above with prescribed6[6 N_bod] for
 *                        prescribed; the _dev form reads back 18 numbers per body.  The force model and the flow model enter at
 *                        q^n as in rbl_step_mixed_dof (free components only), RBL_OPT_RECORD_MOMENTS as in rbl_step_brownian_mixed.
 *                        kBT <= 1e-10: rbl_step_mixed_dof.  Rows all 0 or all 1 give bitwise the whole-body calls' results.  With no
 *                        entry set the step IS rbl_step_brownian (the call is handed to it: its bits and its iteration count; F
 *                        echoes the loads it solved with), from which rbl_step_brownian_mixed with nobody prescribed differs in
 *                        the last digits, the masked solve being another GMRES driver.
 * Refused with RBL_ERR_ARG before any device work: what the whole-body Brownian calls and the _dof calls refuse, and a mask with a
 * partly prescribed rotation (one or two of a body's entries 3..5 set) -- the message names the entry point and the first such
 * body.  A partly prescribed rotation is not a subset of the coordinates and nobody has derived its drift; sampling cannot tell
 * either, a shell's rotational drift being below one standard error of any affordable sample.
 * Cost: tools/bench_brownian_dof.py, profiles/brownian_dof.jsonl.
 *
 * Many right-hand sides under ONE mask, in lock step (the _multi entry points): the 6 N_bod unit velocities of the body resistance
 * matrix, a handful of imposed rotations or trap displacements under one component mask, several noise realisations against fixed
 * obstacles.  nrhs independent recurrences of the solver above -- each column with its own Krylov basis, Hessenberg matrix and
 * stopping test, so its iterates are those of the one-vector call on it alone up to the rounding of the multi-vector product --
 * advance together, 16 columns a batch as rbl_gmres_saddle_multi_dev: ONE launch of the multi-vector mobility product per
 * iteration (the fp64 matrix cores from 4 columns on), the per-body factor passes shared by the columns (three vectors a pass),
 * and the masked tails above with the column on the grid's second axis: one launch per iteration for all live columns.  The masked
 * 6 x 6 factors are made once per call.  A column that has converged stops iterating; a column whose right-hand side is exactly
 * zero returns zeros after one iteration.
 *     prescribed / prescribed6     ONE mask for all columns (N_bod / 6 N_bod bytes, a HOST array in the _dev forms too)
 *     body_in[nrhs][6 N_bod], slip[nrhs][3 N_blobs] or NULL        one vector after the other
 *     lambda[nrhs][3 N_blobs] (may be NULL), U[nrhs][6 N_bod], F[nrhs][6 N_bod]      column by column, each as above
 *     iters[nrhs], resid[nrhs]     (may be NULL)
 *   rbl_solve_mixed_multi, rbl_solve_mixed_dof_multi          host arrays, synchronous.
 *   rbl_solve_mixed_multi_dev, rbl_solve_mixed_dof_multi_dev  device pointers, stream drains and error latching as
 *                        rbl_solve_mixed_dev (the lock-step solver tests convergence every iteration).
 * Refused with RBL_ERR_ARG before any device work: what the one-vector calls refuse, and nrhs < 1.  Results are bitwise reproducible
 * call to call.  16 unit-velocity columns at cfg 3 take 0.34 (every body prescribed) and 0.32 (the rotations of all bodies) of the
 * sequential loop's time (tools/bench_prescribed_multi.py, profiles/prescribed_multi.jsonl).
 *
 * Not offered: contexts with a communicator, a mask that changes within a step, lock-step solves whose mask differs from column to
 * column, the Brownian steps in lock step; and with masks per component:
 *   - the Brownian step with a partly prescribed rotation (one or two of a body's three rotation components): that is not a
 *     subset of the coordinates and nobody has derived the scheme for it; single contexts and ensembles refuse such a mask;
 *   - for ensembles, Brownian RUNS with component masks (rbl_ensemble_run with prescribed_per = 6, brownian != 0 and kBT > 1e-10
 *     stays refused: the follow-up, which needs only the per-component midpoint kernel in the run's step sequence; the one-step
 *     rbl_ensemble_step_brownian_mixed_dof and the deterministic runs with prescribed_per = 6 are in section 5);
 *   - constraint axes fixed in the body frame (the six components are the lab frame's). */
int rbl_solve_mixed(rbl_ctx *ctx, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
                    double *lambda, double *U, double *F, int *iters, double *resid);
int rbl_solve_mixed_dev(rbl_ctx *ctx, const uint8_t *prescribed, const double *d_body_in, const double *d_slip, int max_iter,
                        double rtol, double *d_lambda, double *d_U, double *d_F, int *iters, double *resid);
int rbl_step_mixed(rbl_ctx *ctx, const uint8_t *prescribed, const double *body_in, const double *slip, int max_iter, double rtol,
                   double *F, int *iters, double *resid);
int rbl_solve_mixed_dof(rbl_ctx *ctx, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter, double rtol,
                        double *lambda, double *U, double *F, int *iters, double *resid);
int rbl_solve_mixed_dof_dev(rbl_ctx *ctx, const uint8_t *prescribed6, const double *d_body_in, const double *d_slip, int max_iter,
                            double rtol, double *d_lambda, double *d_U, double *d_F, int *iters, double *resid);
int rbl_step_mixed_dof(rbl_ctx *ctx, const uint8_t *prescribed6, const double *body_in, const double *slip, int max_iter, double rtol,
                       double *F, int *iters, double *resid);
int rbl_solve_mixed_multi(rbl_ctx *ctx, const uint8_t *prescribed, int nrhs, const double *body_in, const double *slip, int max_iter,
                          double rtol, double *lambda, double *U, double *F, int *iters, double *resid);
int rbl_solve_mixed_multi_dev(rbl_ctx *ctx, const uint8_t *prescribed, int nrhs, const double *d_body_in, const double *d_slip,
                              int max_iter, double rtol, double *d_lambda, double *d_U, double *d_F, int *iters, double *resid);
int rbl_solve_mixed_dof_multi(rbl_ctx *ctx, const uint8_t *prescribed6, int nrhs, const double *body_in, const double *slip, int max_iter,
                              double rtol, double *lambda, double *U, double *F, int *iters, double *resid);
int rbl_solve_mixed_dof_multi_dev(rbl_ctx *ctx, const uint8_t *prescribed6, int nrhs, const double *d_body_in, const double *d_slip,
                                  int max_iter, double rtol, double *d_lambda, double *d_U, double *d_F, int *iters, double *resid);
int rbl_RHS_and_Midpoint_mixed(rbl_ctx *ctx, const uint8_t *prescribed, const double *body_in, const double *slip, const double *W,
                               uint64_t seed, int method, int split_rand, double delta, double *s, double *X_half, double *Q_half);
int rbl_RHS_and_Midpoint_mixed_dev(rbl_ctx *ctx, const uint8_t *prescribed, const double *d_body_in, const double *d_slip,
                                   const double *d_W, uint64_t seed, int method, int split_rand, double delta, double *d_s,
                                   double *X_half, double *Q_half);
int rbl_step_brownian_mixed(rbl_ctx *ctx, const uint8_t *prescribed, const double *body_in, const double *slip, const double *W,
                            uint64_t seed, int method, int split_rand, double delta, int max_iter, double rtol, double *F,
                            int *iters, double *resid);
int rbl_RHS_and_Midpoint_mixed_dof(rbl_ctx *ctx, const uint8_t *prescribed6, const double *body_in, const double *slip, const double *W,
                                   uint64_t seed, int method, int split_rand, double delta, double *s, double *X_half, double *Q_half);
int rbl_RHS_and_Midpoint_mixed_dof_dev(rbl_ctx *ctx, const uint8_t *prescribed6, const double *d_body_in, const double *d_slip,
                                       const double *d_W, uint64_t seed, int method, int split_rand, double delta, double *d_s,
                                       double *X_half, double *Q_half);
int rbl_step_brownian_mixed_dof(rbl_ctx *ctx, const uint8_t *prescribed6, const double *body_in, const double *slip, const double *W,
                                uint64_t seed, int method, int split_rand, double delta, int max_iter, double rtol, double *F,
                                int *iters, double *resid);

/* ===================================================================== */
/* 8. Imposed flow and active slip (rigid_body_light_amd/csrc/rbl_flow.hip) */
/* ===================================================================== */
/* The other half of the right-hand side, kept in the context and evaluated on the device as the force model (section 4) is: a
 * background flow that is linear in space and a slip pattern carried by the bodies (the reference has neither; its only handle
 * is a lab-frame slip vector per call).  Sign convention of the `slip` argument throughout: the saddle system is
 * M lambda - K U = slip, so a blob that must move with the fluid velocity u_inf gets slip = -u_inf(r_i).  Per blob i of body b:
 *     t_i = scale_b R(q_b) s_body,i - (u0 + G r_i)
 * with the blob positions r_i and rotations R(q_b) of the configuration (what rbl_multi_body_pos returns).  No sums over blobs, no
 * atomics: bitwise the same on every call, every rank (a context with a communicator evaluates the whole term, replicated) and
 * for every replica of an ensemble.
 *
 *   rbl_set_background_flow  u_inf(r) = u0 + G r, G row-major, G[3 i + j] = d u_i / d x_j.  on = 0 switches the flow off.  NULL or
 *                            non-finite entries: RBL_ERR_ARG, the previous model stays in place.
 *   rbl_set_body_slip        slip_body[3 N_blb]: a pattern in the BODY frame, one vector per blob of the shared structure, in the
 *                            units and the sign of the `slip` argument; slip_scale[n_scale]: a factor per body (NULL: 1 for every
 *                            body; 0: a passive body).  Needs rbl_set_parameters first (RBL_ERR_STATE).  n_scale must equal the
 *                            body count of whatever configuration later uses the model -- the context's, or an ensemble's, where
 *                            slip_scale[b] serves body b of every replica; a mismatch is RBL_ERR_ARG at that use, not here.  The
 *                            pattern belongs to the structure: after any later rbl_set_parameters call a pattern that is still
 *                            switched on is RBL_ERR_STATE at the use, until rbl_set_body_slip is called again.
 *   rbl_get_flow_model       u0G12 = [u0 (3) | G (9)], the two switches; any pointer may be NULL.
 *
 * With the wall (rbl_set_wall_pc) the mobility assumes no slip at z = 0, so a flow that does not vanish there is refused: u0 != 0
 * or any of G[.][0], G[.][1], G[2][2] non-zero -- only u = (G02 z, G12 z, 0) passes -- is RBL_ERR_ARG at every use, a step or a
 * query, before the device is touched.  In free space any G is accepted.
 *
 * Where it enters: the term is added to the slip at q^n -- the configuration the step starts from, where the force model is
 * evaluated; for the Brownian steps the one RHS_and_Midpoint is called on -- in every whole-step entry point and nowhere else:
 * rbl_step_deterministic, rbl_step_brownian, rbl_step_mixed, rbl_step_mixed_dof, rbl_step_brownian_mixed, rbl_step_jointed,
 * rbl_ensemble_step_deterministic, rbl_ensemble_step_brownian, rbl_ensemble_step_mixed, rbl_ensemble_step_brownian_mixed.  When
 * the caller also passes `slip` the right-hand side holds slip + t, added in that order.  No lower-level entry point adds it
 * (rbl_solve_mixed*, rbl_gmres_saddle*, rbl_RHS_and_Midpoint*, the ensemble solves): for those there are the queries.  With both
 * parts off every entry point does exactly what it does without this section: no launch, no allocation.
 * Left out on purpose: flows that are not linear in r, evaluation at q^{n+1/2}, a flow per replica.
 *
 *   rbl_flow_slip_dev        the term at the context's configuration into device memory, 3 N_blobs doubles (enqueued, not
 *                            synchronised); zeros with both parts off
 *   rbl_flow_slip            the same into a host array (synchronous)
 *   rbl_ensemble_flow_slip   the term at every replica's configuration, R n3 doubles, host
 *
 * First moments of the blob forces.  For each body b, with the lever arms l_i = r_i - X_b the K operators use,
 *     D_b = sum_{i in b} l_i lambda_i^T      (3 x 3 row-major, 9 N_bod doubles in all)
 * one workgroup per body, fixed-order reduction, no atomics: bitwise reproducible.  The antisymmetric part of D_b is the torque of
 * rbl_KT_x_Lam, its symmetric traceless part the stresslet.  Any 3 N_blobs vector may be passed: the lambda of a solve, or the
 * f_blob of rbl_interaction_forces for the interparticle contribution.
 *   rbl_first_moments_dev    device pointers, enqueued on the context's stream
 *   rbl_first_moments        host arrays, synchronous
 * With the option RBL_OPT_RECORD_MOMENTS switched on every whole-step entry point listed above also computes D_b from the lambda of its solve, with
 * the lever arms of the configuration it solved at (q^n for the deterministic steps, q^{n+1/2} for the midpoint steps), into a
 * device buffer: one small launch per step, one launch over R N_bod bodies for an ensemble.
 *   rbl_step_moments           the last recorded set, 9 N_bod doubles
 *   rbl_ensemble_step_moments  the same of the last ensemble step, R 9 N_bod doubles
 * Both return RBL_ERR_STATE when no step has recorded since the option was set or since the configuration's size changed.
 * What is recorded is the first moment of that step's lambda, thermal part included in a Brownian step.  The Brownian drift's
 * contribution to the stress is NOT added: the recorded moments of Brownian steps do not average to the full Brownian stress. */
int rbl_set_background_flow(rbl_ctx *ctx, const double u0[3], const double G[9], int on);
int rbl_set_body_slip(rbl_ctx *ctx, const double *slip_body, const double *slip_scale, int n_scale, int on);
int rbl_get_flow_model(const rbl_ctx *ctx, double *u0G12, int *flow_on, int *body_slip_on);
int rbl_flow_slip_dev(rbl_ctx *ctx, double *d_out);
int rbl_flow_slip(rbl_ctx *ctx, double *out);
int rbl_ensemble_flow_slip(rbl_ctx *ctx, double *out);
int rbl_first_moments_dev(rbl_ctx *ctx, const double *d_lambda, double *d_D);
int rbl_first_moments(rbl_ctx *ctx, const double *lambda, double *D);
int rbl_step_moments(rbl_ctx *ctx, double *D);
int rbl_ensemble_step_moments(rbl_ctx *ctx, double *D);

/* ===================================================================== */
/* 9. Hard joints (rigid_body_light_amd/csrc/rbl_joints.hip)             */
/* ===================================================================== */
/* Ball joints between anchor points fixed in two bodies, or in a body and the lab (a pivot), imposed as CONSTRAINTS of the saddle
 * solve: the joint forces are unknowns of the same linear system and the constraint holds to the solver's tolerance at any dt.
 * (The bonds of section 4 are springs: they hold two points together as well as their stiffness allows, and a stiff one limits
 * dt like any explicit spring.)  The reference has no counterpart.
 *
 * Joint j joins the point p_A = X_A + R(Q_A) s_A of body A to the point p_B = X_B + R(Q_B) s_B of body B, or to the lab point P:
 * the description rbl_set_bonds takes.  body[2 j] = A >= 0, body[2 j + 1] = B >= 0 and different, or -1 for a pivot;
 * anchor[6 j .. 6 j + 5] = s_A, then s_B or P; s = 0 is the body centre, a blob's body-frame position ends the joint on that
 * blob.  Each joint has
 *     its gap          g_j = p_A - p_B,
 *     three rows       (J U)_j = (u_A + w_A x l_A) - (u_B + w_B x l_B),   l = R(Q) s the lever arms, no B term for a pivot,
 *     one unknown      phi_j, three components: the joint's force.
 * In the convention of rbl_step_deterministic (rhs = [slip; -F_body]) the jointed solve is
 *     M lambda - K U             = slip
 *     K^T lambda       + J^T phi = -F_body
 *                    J U         = c
 * phi is reported in the convention of the F_body argument (that of the F rbl_solve_mixed returns): the load the joints put on
 * the bodies is J^T phi -- on body A of joint j the force phi_j and the torque l_A x phi_j, on body B the opposite force at l_B --
 * and rbl_gmres_saddle on [slip; -(F_body + J^T phi)] returns the same lambda and U.  That statement defines the sign.
 *
 * One ball joint leaves the two bodies their three relative rotations; two between the same bodies are a hinge about the line
 * through them, two pivots on one body a hinge to the lab.  A closed hinge carries one redundant row -- both joints hold the
 * distance between the two anchors, which either body fixes by itself -- and the solver expects it (see "redundant" below).
 *
 *   rbl_set_joints   context state, like the bonds: checks first, nothing is stored unless all pass, no device touched.
 *                    RBL_ERR_ARG with the joint named in rbl_last_error and the previous joints in place for: NULL where an array
 *                    is needed; n_joints < 1 or > 2048; a body index out of range (body[2 j] < 0, body[2 j + 1] < -1, or, once a
 *                    configuration is set, either >= N_bod; a set made before any configuration is checked at the solve,
 *                    RBL_ERR_STATE there); a pivot in the first slot (body[2 j] = -1); both ends on one body; non-finite
 *                    anchors; more than two joints between the same pair of bodies or more than two pivots on one body (three
 *                    would constrain nine of six relative coordinates).  on = 0 stores the joints switched off; body = anchor =
 *                    NULL with on = 0 only switches them off.
 *   rbl_get_joints   reads them back; any pointer may be NULL.
 *   rbl_solve_jointed      host arrays, synchronous.  F_body[6 N_bod]; slip[3 N_blobs] or NULL (zero); joint_rhs[3 n_joints], the
 *                    c above, or NULL (zero); lambda[3 N_blobs], U[6 N_bod], phi[3 n_joints], any may be NULL.  No-restart
 *                    right-preconditioned GMRES as rbl_gmres_saddle_dev (max_iter <= 255), the vectors longer by 3 n_joints;
 *                    iters / resid report the run, resid relative to |[slip; -F_body; c]|.
 *   rbl_solve_jointed_dev  the same with device vectors, on the conditions of rbl_solve_mixed_dev: enqueued on the context's
 *                    stream, which is drained where the solver drains it (its convergence tests, the check of the factorisation);
 *                    d_slip, d_joint_rhs and d_lambda may be NULL; no force or flow model is added.
 *   rbl_step_jointed one deterministic time step: the force model's loads (bonds included, section 4) and the flow model's slip
 *                    (section 8) at q^n exactly as rbl_step_deterministic adds them, the solve above with
 *                        c = -(gamma / dt) g(q^n) + joint_velocity,
 *                    then evolve_X_Q(U).  gamma in [0, 1] (RBL_ERR_ARG otherwise) relaxes the gap: with gamma = 1 the O(dt^2) gap
 *                    the explicit rotation update leaves is taken out by the next step and does not accumulate, with gamma = 0
 *                    only the velocities are constrained and the gaps drift.  joint_velocity[3 n_joints] or NULL (zero): the
 *                    rate at which p_A - p_B is to change -- a pivot that moves with velocity v takes -v, a joint that is pulled
 *                    apart its opening rate.  phi[3 n_joints] may be NULL.  The step clears the warm-start history of
 *                    rbl_step_deterministic, as rbl_step_mixed does.
 *   rbl_joint_state  gap[3 n_joints]: the gaps of the stored joints (on or off) at the context's configuration; phi[3 n_joints]:
 *                    the joint forces of the last rbl_solve_jointed* / rbl_step_jointed that succeeded with this joint set,
 *                    RBL_ERR_STATE if there is none.  Host arrays, either may be NULL; synchronous.
 *
 * The preconditioner is the exact inverse of the system with M replaced by the context's preconditioner M~ (diagonal or per-body
 * blocks, with the wall term or the free-space body-frame tables: whatever rbl_set_blk_pc / rbl_set_wall_pc select).  One
 * application: apply_PC on the (slip, body) part; phi from the joint Schur complement S = J N~^-1 J^T, N~_b^-1 = (NL_b NL_b^T)^-1
 * the per-body 6 x 6 blocks every preconditioner keeps; apply_PC a second time on (0, J^T phi); the difference.  S has
 * 3 n_joints rows and couples only joints that share a body; it is stored dense, assembled, factored (the device Cholesky of
 * rbl_cholesky_lower_dev) and inverted once per solve -- the configuration cannot change inside one -- and applied as one
 * matrix-vector product per iteration.  Cost beyond the plain solve, per iteration: the second preconditioner application and
 * three launches over the joints; per solve: O(n_joints^3) for the inverse (profiles/joints.jsonl has the times).
 * No floating-point atomics anywhere: two calls on the same input give the same bits.
 *
 * Redundant joints.  A loop of joints that constrains a relative coordinate twice leaves S singular.  One such row is expected
 * and dealt with: that of a hinge.  Of two joints between one pair of bodies the combination d . (J U)_1 - d . (J U)_2, d the
 * unit vector between the two anchors, is the rate of change of |A_1 - A_2|^2 - |B_1 - B_2|^2, which vanishes identically once the
 * hinge is closed (||A_1 - A_2| - |B_1 - B_2|| <= 1e-6 |A_1 - A_2| is taken as closed; two pivots on one body are always: the lab
 * points do not move).  For a closed hinge the preconditioner gives that direction of S an eigenvalue of the size of the
 * others, i.e. applies the pseudo-inverse there; the operator is untouched, GMRES solves the consistent singular system, lambda
 * and U are the constrained motion and the two phi are determined up to equal and opposite forces along the hinge's axis, which
 * load neither body (the step's gamma = 1 drives every hinge there: its gaps stay at the O(dt^2) of the rotation update).  A
 * hinge that is open takes part as it is: its S has an eigenvalue of the order (gap / distance between the anchors)^2 relative
 * to the others and phi along the axis is determined that badly; a joint_rhs that asks the two anchors' distances to change
 * differently on the two bodies has no bounded answer.
 * Any OTHER redundancy -- a closed ring of joints, a joint between two bodies that hinges to the lab already hold, two joints
 * on one point -- makes the factorisation fail: a pivot d with d^2 <= 1e-14 S_ii counts as lost (two orders above what rounding
 * leaves of an exactly redundant row), and the call returns RBL_ERR_NOT_SPD with "redundant" in rbl_last_error, no answer, the
 * configuration untouched (a step does not advance); the context serves a valid joint set afterwards.
 *
 * The joints act in the section 9 calls only.  No other entry point changes meaning, launches or results: on a context with
 * joints set rbl_step_deterministic, rbl_solve_mixed and the rest ignore them.  With the joints switched off, or never set,
 * rbl_solve_jointed is the plain solve (rbl_gmres_saddle_dev on [slip; -F_body], cold start; joint_rhs and phi are not touched)
 * and rbl_step_jointed is rbl_step_deterministic with a cold start.
 *
 * Not offered, each refused before any device work: contexts with a communicator (RBL_ERR_ARG); the calls of THIS section on a
 * context that holds an ensemble (RBL_ERR_STATE) -- an ensemble's jointed solve and step are section 5's
 * rbl_ensemble_solve_jointed / rbl_ensemble_step_jointed / rbl_ensemble_run_jointed, which read the joint set stored here; the
 * other ensemble entry points, rbl_ensemble_run among them, ignore the joints like every other --; and, having no entry point at
 * all: the jointed solve together with prescribed masks (section 7), lock-step right-hand sides, Brownian steps (the drift of a
 * constrained suspension has not been derived here), joint kinds other than those below (no slider, no universal joint).
 *
 * Joint kinds.  rbl_set_joint_kinds is a superset of rbl_set_joints: one kind per joint, every joint keeps three rows and three
 * unknowns, so every vector of this section keeps its length 3 n_joints.  With dw = w_A - w_B (w_B = 0 and Q_B = identity for
 * body B = -1, the lab) and ah = R(Q_A) a the lab-frame image of a unit axis a fixed in body A:
 *
 *     kind                 rows (J U)_j                          load J^T phi of joint j
 *     RBL_JOINT_BALL  0    (u_A + w_A x l_A) - (u_B + w_B x l_B)  as above
 *     RBL_JOINT_LOCK  1    dw                                    torque +phi_j on A, -phi_j on B, no force
 *     RBL_JOINT_AXIS  2    P dw,  P = I - ah ah^T                torque +P phi_j on A, -P phi_j on B, no force
 *
 * An axis joint leaves the relative rotation about ah free.  Its row along ah constrains nothing; so that the system stays
 * regular without a pseudo-inverse, the operator's rows of that joint are P dw - sigma ah (ah . phi_j) and S gets sigma ah ah^T
 * on that diagonal block (the minus sign makes the preconditioner's S = J N~^-1 J^T + sigma ah ah^T the exact Schur complement),
 * sigma = the mean rotational diagonal entry of N~_A^-1.  The component of joint_rhs / joint_velocity along ah is IGNORED (the
 * rows are projected with P before the solve) and the returned phi_j is P phi_j: its component along ah is zero to the rounding
 * of that one projection, exactly zero when ah is a coordinate axis.  The answer does not depend on sigma.
 * Compositions are the caller's: BALL + AXIS on one pair of bodies is a five-row hinge (no redundant row, unlike the two-ball
 * hinge, which stays as it is), BALL + LOCK a weld, BALL + LOCK with a rate a motor or driven hinge.
 *
 * Orientation gap.  An angular joint stores q_rel (scalar first, normalised on entry) and, a lock, the axis a and a motor angle
 * theta (0 when set).  The target orientation of body B is Q_B* = Q_A rot(theta a) q_rel (an axis joint: theta = 0), and the
 * angular gap e is the lab-frame rotation vector of Q_B* Q_B^-1, the short way round (the quaternion's sign is flipped on a
 * negative scalar part), so that de/dt = w_A - w_B to first order, as dg/dt = J U for a ball joint.  An axis joint uses P e.
 * rbl_step_jointed sets c = -(gamma / dt) e + w on those rows, w the caller's joint_velocity rows plus, for a lock with the rate
 * Omega_j, -Omega_j ah: body B turns relative to body A at +Omega_j about ah.  After an accepted step theta_j += Omega_j dt; a
 * refused step changes nothing.
 *
 *   rbl_set_joint_kinds   body and anchor as rbl_set_joints; kind[n_joints]; axis[3 n_joints] (read for LOCK and AXIS,
 *                    normalised); q_rel[4 n_joints] (read for LOCK and AXIS); anchor is read for BALL only (an angular joint's
 *                    anchors read back as zeros).  Checks first, nothing stored unless all pass, no device touched.  RBL_ERR_ARG
 *                    with the joint named for: an unknown kind; an axis that is not finite or of norm < 1e-12 where one is
 *                    read; a q_rel of zero norm; a second angular joint on a pair of bodies (or on a body and the lab); an
 *                    angular joint together with two ball joints on that pair; both ends on one body; and every refusal of
 *                    rbl_set_joints.  At most 2048 joints.  Every pointer NULL with on = 0 only switches the joints off.
 *   rbl_get_joint_kinds   reads everything back, theta and the rates included; any pointer may be NULL.  by_kinds: 1 when the
 *                    stored set came through rbl_set_joint_kinds.  A set from rbl_set_joints reads back as BALL throughout.
 *   rbl_set_joint_rates   rate[n_joints], context state read by rbl_step_jointed: a lock's Omega_j; must be 0 for every other
 *                    kind (RBL_ERR_ARG, the joint named) and is 0 after rbl_set_joint_kinds.  May change from step to step.
 *   rbl_joint_state_kinds rbl_joint_state and theta[n_joints] (may be NULL).  The gap rows of an angular joint hold e (P e for
 *                    an axis joint); rbl_joint_state returns the same rows.
 * rbl_solve_jointed[_dev], rbl_step_jointed and rbl_joint_state serve whichever joint set is stored.  A set without a lock or
 * axis joint launches the kernels of the ball joint unchanged: the same bits whichever entry point stored it. */
#define RBL_JOINT_BALL 0
#define RBL_JOINT_LOCK 1
#define RBL_JOINT_AXIS 2
int rbl_set_joints(rbl_ctx *ctx, int n_joints, const int *body, const double *anchor, int on);
int rbl_get_joints(const rbl_ctx *ctx, int *n_joints, int *on, int *body, double *anchor);
int rbl_solve_jointed(rbl_ctx *ctx, const double *F_body, const double *slip, const double *joint_rhs, int max_iter, double rtol,
                      double *lambda, double *U, double *phi, int *iters, double *resid);
int rbl_solve_jointed_dev(rbl_ctx *ctx, const double *d_F_body, const double *d_slip, const double *d_joint_rhs, int max_iter,
                          double rtol, double *d_lambda, double *d_U, double *d_phi, int *iters, double *resid);
int rbl_step_jointed(rbl_ctx *ctx, const double *F_body, const double *slip, const double *joint_velocity, double gamma, int max_iter,
                     double rtol, double *phi, int *iters, double *resid);
int rbl_joint_state(rbl_ctx *ctx, double *gap, double *phi);
int rbl_set_joint_kinds(rbl_ctx *ctx, int n_joints, const int *body, const double *anchor, const int *kind, const double *axis,
                        const double *q_rel, int on);
int rbl_get_joint_kinds(const rbl_ctx *ctx, int *n_joints, int *on, int *by_kinds, int *body, double *anchor, int *kind, double *axis,
                        double *q_rel, double *theta, double *rate);
int rbl_set_joint_rates(rbl_ctx *ctx, const double *rate);
int rbl_joint_state_kinds(rbl_ctx *ctx, double *gap, double *phi, double *theta);

/* ===================================================================== */
/* 10. Periodic cell in x and y (rigid_body_light_amd/csrc/rbl_periodic.hip) */
/* ===================================================================== */
/* A suspension above the wall at a fixed area fraction: the system repeats with the cell lengths Lx, Ly along x and y (a length
 * of 0: that axis is open), the wall stays at z = 0.  The reference has no counterpart.  The cell enters in its simplest form:
 * explicit sums over periodic images of the wall-corrected pair mobility, and the minimum-image convention in the pair forces.
 *
 * Mobility.  For blobs i and j with d = r_i - r_j,
 *     d0         = (dx - Lx rint(dx / Lx), dy - Ly rint(dy / Ly), dz)         the nearest image (rint: round half to even)
 *     M_per[i,j] = sum_{|p| <= nx} sum_{|q| <= ny}  B(d0 + (p Lx, q Ly, 0); z_i, z_j)
 * with B the wall-corrected pair block of rbl_apply_M (the wall term with h = z_j), and U = B M_per B F with the same damping and
 * the same scale 1 / (8 pi eta a).  The term p = q = 0 of i = j is the self block; the terms (p, q) != 0 of i = j are the blob's
 * own images, ordinary pairs of two blobs at equal height.  Coordinates are never wrapped: rbl_get_config, the steps and every
 * frame stay unwrapped, the product depends on displacements only.
 * The wall is what makes this legitimate: the wall-corrected far field decays like r^-3, so the lattice sum over a 2-D cell
 * converges; the free-space sum does not and is not offered (RBL_ERR_STATE with "periodic" in the message at use while the wall
 * term is off).  The sum is TRUNCATED at (nx, ny) images: the operator is pseudo-periodic, its convergence in n is slow -- the
 * remainder falls like 1 / n -- and its positivity is observed, not proven.  On make_config(4, 12, wall) in a cell of 7.0 x 7.5
 * (tests/test_periodic_cpu.py re-derives the figures): symmetric to 1e-17 for every n; the smallest eigenvalue of the damped
 * matrix is -0.0035 at n = 0 (the nearest image alone is NOT positive definite, hence n >= 1), 0.01397 at n = 1, 0.01439 at n = 4,
 * against 0.01441 of the open system; for one random F the relative change of U from n - 1 to n is 0.129, 0.026, 0.011, 0.006
 * for n = 1 ... 4 (increments like 1 / n^2, a remainder like 1 / n).
 *
 * With the cell on every mobility product inside the library -- rbl_apply_M*, the saddle operator and both GMRES solvers, the
 * lock-step solves, the Lanczos roots, M_RFD, every step, the masked solves (section 7), the jointed solve (section 9) -- is the
 * periodic one: one ordered-pair kernel (k_apply_M_per, fp64 only: a relaxed request is ignored; several vectors go one at a
 * time; a row range is honoured) that costs about (2 nx + 1)(2 ny + 1) ordered products.  The one-kernel small solver is not
 * chosen; the preconditioners stay as they are, without images (they precondition, they do not define the answer).  No fp64
 * atomics, one summation order: results are bitwise reproducible, and the flags for blobs below the wall, overlaps and
 * non-finite results are raised as by the plain product.
 *
 * Forces (section 4).  The minimum-image displacement is used in the neighbour search, in the blob pair terms (steric and pair
 * table) and in the dipole pair term.  The convention is unique only if 2 R_body + r_cut <= L / 2 on every periodic axis (R_body:
 * the largest blob distance from the body centre; r_cut: the larger cutoff of the pair terms that are on) and the dipole r_cut
 * <= L / 2 (dipoles sit on the body centres); otherwise the evaluation returns RBL_ERR_ARG naming the length and the bound.
 * Weight, wall repulsion, height table, traps and the field torque do not see the cell.  Bonds and tethers (section 4) and
 * joints (section 9) join named bodies at their UNWRAPPED positions: none acts across the boundary by minimum image.
 *
 *   rbl_set_periodic   context state, like rbl_set_joints: checks first, nothing is stored unless all pass, no device touched.
 *                      RBL_ERR_ARG with the offending value named in rbl_last_error for: a non-finite or negative length; both
 *                      lengths 0 with on set; 0 < L <= 4a once the parameters are set (above 4a a blob never overlaps its own
 *                      image and every image with (p, q) != 0 on that axis is at least L / 2 >= 2a away; checked again at use);
 *                      n < 1 or n > 16 on a periodic axis (n is ignored and stored as 0 on an open one); a context with a
 *                      communicator.  RBL_ERR_STATE for a context that holds an ensemble.  on = 0 stores the cell switched off.
 *   rbl_get_periodic   reads it back; any pointer may be NULL.
 *
 * With the cell off or never set every entry point launches what it launched before and returns the same bits.
 *
 * Not offered, each refused with RBL_ERR_STATE and "periodic" in rbl_last_error before any device work while the cell is on: the
 * dense build and the dense Cholesky root (rbl_rotne_prager_tensor[_dev], rbl_M_half_W* with RBL_MHALF_CHOLESKY); the
 * explicit-kernel products rbl_apply_M_sym_dev and rbl_apply_M_sym_multi_dev; rbl_velocity_field[_dev]; every rbl_ensemble_*
 * entry point (an ensemble's cell is its own: rbl_ensemble_set_periodic, section 5); attaching a communicator.  And, having no entry point at all: free-space periodicity; an analytic tail correction
 * or an Ewald split; the relaxed single-precision products; wrapped coordinates; bonds or joints across the boundary by minimum
 * image; a periodic z. */
int rbl_set_periodic(rbl_ctx *ctx, double Lx, double Ly, int nx, int ny, int on);
int rbl_get_periodic(const rbl_ctx *ctx, double *Lx, double *Ly, int *nx, int *ny, int *on);

#ifdef __cplusplus
}
#endif
#endif /* RBL_H */
