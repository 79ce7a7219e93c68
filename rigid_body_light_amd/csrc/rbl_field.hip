// rbl_field.hip -- fluid velocity at arbitrary points from blob forces (include/rbl.h section 6).
//
//   u(x_p) = nf d(z_p) sum_j M(x_p, r_j) d(z_j) lambda_j
//
// the velocity apply_M would give an extra force-free blob of radius a at x_p: the same pair block (rbl_pair_accum,
// free space or wall-corrected), the same damping d, a coincident point (|x_p - r_j| < 1e-12 a) takes the self block,
// and with the wall a point at z_p <= 0 gets u = 0.  A rectangular (target x source) product, O(P N):
//
//   k_vf_pack<WALL>        sources once: radius-scaled positions and damped forces, 48 B per source, padded to whole
//                          tiles of 64 with far-away zero-force sources; a source below the wall latches the reference's
//                          error, as apply_M does
//   k_vf_sweep<WALL,NI>    one wave = one work unit: a super-tile of 64 NI points (lane l holds points l, l + 64, ...)
//                          x one chunk of source tiles, each tile staged in LDS once and read as broadcasts by all
//                          lanes, its reads and loop overhead shared by NI pairs; one chunk: the final velocity,
//                          several chunks: raw partial sums to a slab
//   k_vf_reduce<WALL>      the chunks' partial sums added in chunk order, then nf d(z_p) and the z <= 0 rule
//
// Every point's sum runs over the sources in index order inside a chunk and over the chunks in chunk order, and the
// chunk boundaries depend on (total points, sources, CU count) only (vf_geometry): the result is bitwise reproducible
// and a point's value does not depend on which share of the points (rank) it was evaluated in.  No float atomics.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rbl_api_internal.hpp"

namespace {

constexpr int VF_TS = 64;   // source tile = wave width

struct __attribute__((aligned(16))) VfBlob {
  double x, y, z, fx, fy, fz;   // unit-scaled position, damped force: three 16-B LDS broadcasts per source
};

// the pair arithmetic runs in the length unit rbl_unit_of(WALL) of rbl_pair.hpp, as in rbl_kernels.hip: positions times
// rbl_unit_pos_scale where they are packed or loaded, rbl_unit_params, sums times rbl_unit_out_scale
// (restated from rbl_kernels.hip, where it is file-local)

__device__ __forceinline__ double vf_damp_of(const RblParams &P, double z)
{
  if (P.no_damp) return 1.0;
  return (z >= P.a) ? 1.0 : z / P.a;   // c_rigid_obj.cpp:629-633
}

__device__ __forceinline__ double vf_wave_min(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double vf_wave_max(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ double vf_uniform(double v)   // a value all lanes hold, moved to scalar registers
{
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// one thread per (padded) source; a wave = one source tile, whose bounding box of the real sources (unit-scaled) goes to
// box[tile][6] = (min x, y, z, max x, y, z) -- the sweep's test whether a point of a unit may coincide with a source of the tile
template <bool WALL>
__global__ __launch_bounds__(256) void k_vf_pack(const double *__restrict__ r, const double *__restrict__ lam, long N, long Npad,
                                                 RblParams P, VfBlob *__restrict__ src, double *__restrict__ box, unsigned *err)
{
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Npad) return;                // (Npad is a multiple of 64: whole waves leave)
  VfBlob b;
  double lo[3], hi[3];
  if (j < N) {
    const double z = r[3 * j + 2];
    double d = 1.0;
    if (WALL) {
      if (z < 0.0) atomicOr(err, (unsigned)RBL_FLAG_BELOW_WALL);
      d = vf_damp_of(P, z);
    }
    const double ps = rbl_unit_pos_scale<rbl_unit_of(WALL)>(P);
    b.x = r[3 * j] * ps; b.y = r[3 * j + 1] * ps; b.z = z * ps;
    b.fx = d * lam[3 * j]; b.fy = d * lam[3 * j + 1]; b.fz = d * lam[3 * j + 2];
    lo[0] = hi[0] = b.x; lo[1] = hi[1] = b.y; lo[2] = hi[2] = b.z;
  } else {   // padding: zero force, far away, above the wall; not part of the box
    b.x = 1.0e15; b.y = 1.0e15; b.z = 1.0; b.fx = 0.0; b.fy = 0.0; b.fz = 0.0;
    lo[0] = lo[1] = lo[2] = INFINITY; hi[0] = hi[1] = hi[2] = -INFINITY;
  }
  src[j] = b;
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = vf_wave_min(lo[k]); hi[k] = vf_wave_max(hi[k]); }
  if ((threadIdx.x & (VF_TS - 1)) == 0) {
    double *o = box + (j / VF_TS) * 6;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
  }
}

// one staged tile against the lane's NI points.  COINC: the tile's box touches the unit's, a point may coincide with a source
// (|x_p - r_j| < 1e-12 a): rbl_pair_accum's SELF form, with "coincident" in place of its index equality, gives that pair the
// self block.  Otherwise the sweep is k_apply_M's off-diagonal one.
template <bool WALL, bool COINC, int NI>
__device__ __forceinline__ void vf_sweep_tile(const RblParams &Pu, const VfBlob *sj, const double (&xi)[NI], const double (&yi)[NI],
                                              const double (&zi)[NI], double (&ux)[NI], double (&uy)[NI], double (&uz)[NI],
                                              unsigned &flags, const RblWallK &K)
{
#pragma unroll 1     // (NI pairs per source already; a second source in flight spills the four-point wall kernel)
  for (int jj = 0; jj < VF_TS; ++jj) {
    const VfBlob b = sj[jj];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      bool coinc = false;
      if (COINC) {
        const double dx = xi[k] - b.x, dy = yi[k] - b.y, dz = zi[k] - b.z;
        coinc = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)) < Pu.tiny2;
      }
      rbl_pair_accum<WALL, COINC, rbl_unit_of(WALL)>(Pu, xi[k], yi[k], zi[k], b.x, b.y, b.z, b.fx, b.fy, b.fz, coinc, ux[k], uy[k], uz[k],
                                        flags, K);
    }
  }
}

// grid = (point super-tiles of this launch, chunks).  Unit (bx, by): points bx 64 NI .. + 64 NI of this launch's Pl, source
// tiles [by tpc, min((by + 1) tpc, Ts)).  nch == 1: out = u (final); nch > 1: slab[by][3 Pl] = raw sums.
template <bool WALL, int NI>
__global__ __launch_bounds__(VF_TS, NI == 4 ? 2 : (WALL ? 3 : 4)) void k_vf_sweep(const VfBlob *__restrict__ src, const double *__restrict__ box, const double *__restrict__ pts,
                                                                   long Pl, int Ts, int tpc, int nch, RblParams P,
                                                                   double *__restrict__ out, double *__restrict__ slab, unsigned *err)
{
  __shared__ VfBlob sj[VF_TS];
  const int t = threadIdx.x;
  const long p0 = (long)blockIdx.x * (VF_TS * NI);
  constexpr int kUnit = rbl_unit_of(WALL);
  const RblParams Pu = rbl_unit_params<kUnit>(P);
  const RblWallK WK = rbl_wall_k_resident<kUnit>();
  const double ps = rbl_unit_pos_scale<kUnit>(P);
  double xi[NI], yi[NI], zi[NI], ux[NI], uy[NI], uz[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    long p = p0 + t + (long)k * VF_TS;
    if (p >= Pl) p = Pl - 1;          // masked lane: a copy of the last point, never written
    xi[k] = pts[3 * p] * ps; yi[k] = pts[3 * p + 1] * ps; zi[k] = pts[3 * p + 2] * ps;
    ux[k] = 0.0; uy[k] = 0.0; uz[k] = 0.0;
  }
  // the unit's box (all lanes agree on it: wave-uniform branch per tile below)
  double blo[3], bhi[3];
  {
    double lx = xi[0], ly = yi[0], lz = zi[0], hx = xi[0], hy = yi[0], hz = zi[0];
#pragma unroll
    for (int k = 1; k < NI; ++k) {
      lx = fmin(lx, xi[k]); ly = fmin(ly, yi[k]); lz = fmin(lz, zi[k]);
      hx = fmax(hx, xi[k]); hy = fmax(hy, yi[k]); hz = fmax(hz, zi[k]);
    }
    blo[0] = vf_uniform(vf_wave_min(lx)); blo[1] = vf_uniform(vf_wave_min(ly)); blo[2] = vf_uniform(vf_wave_min(lz));
    bhi[0] = vf_uniform(vf_wave_max(hx)); bhi[1] = vf_uniform(vf_wave_max(hy)); bhi[2] = vf_uniform(vf_wave_max(hz));
  }
  unsigned flags = 0;
  const int tile0 = blockIdx.y * tpc;
  const int tile1 = min(tile0 + tpc, Ts);
  // the next tile travels in registers while the current one is swept (as plain doubles: a struct copy would go through scratch)
  const double *sp = (const double *)(src + (long)tile0 * VF_TS + t);
  double n0 = sp[0], n1 = sp[1], n2 = sp[2], n3 = sp[3], n4 = sp[4], n5 = sp[5];
  for (int tile = tile0; tile < tile1; ++tile) {
    __syncthreads();                          // previous tile fully consumed
    sj[t].x = n0; sj[t].y = n1; sj[t].z = n2; sj[t].fx = n3; sj[t].fy = n4; sj[t].fz = n5;
    __syncthreads();
    if (tile + 1 < tile1) {
      sp += VF_TS * 6;
      n0 = sp[0]; n1 = sp[1]; n2 = sp[2]; n3 = sp[3]; n4 = sp[4]; n5 = sp[5];
    }
    const double *tb = box + (long)tile * 6;
    constexpr double eps = 1e-11 * rbl_unit_l(kUnit);     // (unit-scaled; 10 x the coincidence distance)
    const bool coinc = tb[0] <= bhi[0] + eps && blo[0] <= tb[3] + eps && tb[1] <= bhi[1] + eps && blo[1] <= tb[4] + eps &&
                       tb[2] <= bhi[2] + eps && blo[2] <= tb[5] + eps;
    if (__builtin_amdgcn_readfirstlane((int)coinc))
      vf_sweep_tile<WALL, true, NI>(Pu, sj, xi, yi, zi, ux, uy, uz, flags, WK);
    else
      vf_sweep_tile<WALL, false, NI>(Pu, sj, xi, yi, zi, ux, uy, uz, flags, WK);
  }
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const long p = p0 + t + (long)k * VF_TS;
    if (p >= Pl) continue;
    if (nch == 1) {
      const double zp = pts[3 * p + 2];   // (the physical height, as apply_M damps with)
      double sc = rbl_unit_out_scale<kUnit>(P);
      if (WALL) sc *= vf_damp_of(P, zp);
      double vx = sc * ux[k], vy = sc * uy[k], vz = sc * uz[k];
      if (WALL && !(zp > 0.0)) { vx = 0.0; vy = 0.0; vz = 0.0; }   // outside the fluid: u = 0 (d(0) = 0 already)
      if (!(isfinite(vx) && isfinite(vy) && isfinite(vz))) flags |= RBL_FLAG_NONFINITE;
      out[3 * p] = vx; out[3 * p + 1] = vy; out[3 * p + 2] = vz;
    } else {
      double *s = slab + (size_t)blockIdx.y * (size_t)(3 * Pl) + 3 * p;
      s[0] = ux[k]; s[1] = uy[k]; s[2] = uz[k];
    }
  }
  if (flags) atomicOr(err, flags);
}

template <bool WALL>
__global__ __launch_bounds__(256) void k_vf_reduce(const double *__restrict__ slab, const double *__restrict__ pts, long Pl, int nch,
                                                   RblParams P, double *__restrict__ out, unsigned *err)
{
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over 3 Pl
  if (idx >= 3 * Pl) return;
  double s = 0.0;
  for (int k = 0; k < nch; ++k) s += slab[(size_t)k * (size_t)(3 * Pl) + idx];
  double sc = rbl_unit_out_scale<rbl_unit_of(WALL)>(P);   // (the slabs hold sums of the sweep's unit)
  const double zp = pts[3 * (idx / 3) + 2];
  if (WALL) sc *= vf_damp_of(P, zp);
  double v = sc * s;
  if (WALL && !(zp > 0.0)) v = 0.0;
  if (!isfinite(v)) atomicOr(err, (unsigned)RBL_FLAG_NONFINITE);
  out[idx] = v;
}

// ---- the split: ONE function of (points, sources, CUs) --------------------------------------------------------------------------
struct VfGeom {
  int NI;        // points per lane
  int Ts;        // source tiles of 64
  int tpc;       // source tiles per chunk
  int nch;       // chunks
};

constexpr long VF_NI4_POINTS = 16384;   // four points per lane from here on: <= 255 idle slots of >= 16 384
constexpr int VF_UNITS_PER_CU = 32;     // work units wanted per CU (several rounds of resident waves: XCDs that run faster take more)
constexpr int VF_MIN_CHUNK = 2;         // source tiles per chunk at least (a unit's point loads and slab writes stay small beside it)

VfGeom vf_geometry(int64_t n_points, int64_t n_src, int n_cu)
{
  VfGeom g;
  g.NI = n_points >= VF_NI4_POINTS ? 4 : 2;
  g.Ts = (int)((n_src + VF_TS - 1) / VF_TS);
  const int64_t tp = (n_points + VF_TS * g.NI - 1) / (VF_TS * g.NI);
  const int64_t want = (int64_t)(n_cu > 0 ? n_cu : 256) * VF_UNITS_PER_CU;
  int64_t c = (want + tp - 1) / tp;
  const int64_t cmax = std::max<int64_t>(1, g.Ts / VF_MIN_CHUNK);
  c = std::min(c, cmax);
  if (c < 1) c = 1;
  g.tpc = (int)((g.Ts + c - 1) / c);
  g.nch = (g.Ts + g.tpc - 1) / g.tpc;        // (rounding the chunks up to whole tiles may leave fewer)
  return g;
}

size_t vf_src_bytes(const VfGeom &g) { return (size_t)g.Ts * (VF_TS * sizeof(VfBlob) + 6 * sizeof(double)); }   // sources + tile boxes
size_t vf_slab_bytes(const VfGeom &g, int64_t n_local) { return g.nch > 1 ? (size_t)g.nch * 3 * (size_t)n_local * sizeof(double) : 0; }

template <bool WALL>
void vf_launch(hipStream_t st, const RblParams &P, const VfGeom &g, const double *d_lam, const double *d_r, int64_t n_src,
               const double *d_pts, int64_t n_local, double *d_out, void *d_work, unsigned *d_err)
{
  VfBlob *src = (VfBlob *)d_work;
  double *box = (double *)(src + (size_t)g.Ts * VF_TS);
  double *slab = (double *)((char *)d_work + vf_src_bytes(g));
  const long Npad = (long)g.Ts * VF_TS;
  hipLaunchKernelGGL(k_vf_pack<WALL>, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, d_r, d_lam, (long)n_src, Npad, P, src,
                     box, d_err);
  if (n_local <= 0) return;
  const unsigned tp = (unsigned)((n_local + VF_TS * g.NI - 1) / (VF_TS * g.NI));
  dim3 grid(tp, (unsigned)g.nch), block(VF_TS);
  if (g.NI == 4)
    hipLaunchKernelGGL((k_vf_sweep<WALL, 4>), grid, block, 0, st, (const VfBlob *)src, (const double *)box, d_pts, (long)n_local, g.Ts, g.tpc, g.nch, P,
                       d_out, slab, d_err);
  else
    hipLaunchKernelGGL((k_vf_sweep<WALL, 2>), grid, block, 0, st, (const VfBlob *)src, (const double *)box, d_pts, (long)n_local, g.Ts, g.tpc, g.nch, P,
                       d_out, slab, d_err);
  if (g.nch > 1) {
    const int64_t n = 3 * n_local;
    hipLaunchKernelGGL(k_vf_reduce<WALL>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)slab, d_pts,
                       (long)n_local, g.nch, P, d_out, d_err);
  }
}

// the ranks' contiguous shares of the points, cut at whole point super-tiles: every unit (and so every sum) is the same unit
// whatever the rank count
void vf_shares(int64_t n_points, const VfGeom &g, int W, std::vector<int64_t> &bounds)
{
  const int64_t unit = (int64_t)VF_TS * g.NI, nu = (n_points + unit - 1) / unit;
  bounds.assign((size_t)W + 1, 0);
  for (int r = 0; r <= W; ++r) bounds[(size_t)r] = std::min(n_points, (nu * (int64_t)r / W) * unit);
}

// enqueue u for all n_points (device pointers) on the context's stream; under a communicator this rank evaluates its
// contiguous share and one all-gather completes u on every rank
int vf_enqueue(rbl_ctx *c, const double *d_pts, int64_t n_points, const double *d_lam, const double *d_r, int64_t n_src, double *d_u)
{
  const VfGeom g = vf_geometry(n_points, n_src, c->n_cu);   // of the TOTAL point count: the same chunks on every rank
  const bool comm = comm_on(c);
  const int W = comm ? c->comm_world : 1, rank = comm ? c->comm_rank : 0;
  std::vector<int64_t> bounds;
  vf_shares(n_points, g, W, bounds);
  const int64_t p0 = bounds[(size_t)rank], p1 = bounds[(size_t)rank + 1];
  int rc;
  if ((rc = rbl_dev_reserve(c, c->d_vfw, vf_src_bytes(g) + vf_slab_bytes(g, p1 - p0)))) return rc;
  if (comm && comm_gather_needs_zero(c)) RBL_HIP(c, hipMemsetAsync(d_u, 0, sizeof(double) * 3 * (size_t)n_points, c->stream));
  {
    RblPhase ph(c, RBL_T_PRODUCT);
    const RblParams P = ctx_params(c, false);
    if (c->S.wall)
      vf_launch<true>(c->stream, P, g, d_lam, d_r, n_src, d_pts + 3 * p0, p1 - p0, d_u + 3 * p0, c->d_vfw.p, c->d_err);
    else
      vf_launch<false>(c->stream, P, g, d_lam, d_r, n_src, d_pts + 3 * p0, p1 - p0, d_u + 3 * p0, c->d_vfw.p, c->d_err);
    RBL_HIP(c, hipGetLastError());
  }
  if (comm) return comm_allgather_rows(c, d_u, bounds.data(), 3);
  return RBL_OK;
}

// argument checks that need no device: null / negative / mismatched arguments are RBL_ERR_ARG, n_points == 0 is a no-op (*noop)
int vf_check_args(rbl_ctx *c, const double *points, int64_t n_points, const double *lambda, const double *r_vecs, int64_t n_src,
                  double *u, bool *noop)
{
  *noop = false;
  if (!c) return RBL_ERR_ARG;
  if (periodic_on(c)) return periodic_refuse(c, "velocity_field");
  if (n_points < 0 || n_src < 0) return rbl_fail(c, RBL_ERR_ARG, "velocity_field: negative size");
  if (n_points == 0) { *noop = true; return RBL_OK; }
  if (!points || !u || !lambda) return rbl_fail(c, RBL_ERR_ARG, "velocity_field: null points, lambda or output");
  if (n_src == 0) return rbl_fail(c, RBL_ERR_ARG, "velocity_field: no sources");
  int rc = need_params(c); if (rc) return rc;
  if (!r_vecs) {   // the context's own blobs at the current configuration
    if ((rc = need_config(c))) return rc;
    if (n_src != (int64_t)c->S.N_bod * c->S.N_blb)
      return rbl_fail(c, RBL_ERR_ARG, "velocity_field: r_vecs = NULL needs n_src = N_bod * N_blb (the context's own blobs)");
  }
  return RBL_OK;
}

}  // namespace

// ============================================================================
// 6. velocity field (include/rbl.h)
// ============================================================================
int rbl_velocity_field_dev(rbl_ctx *c, const double *d_points, int64_t n_points, const double *d_lambda, const double *d_r_vecs,
                           int64_t n_src, double *d_u)
{
  bool noop;
  int rc = vf_check_args(c, d_points, n_points, d_lambda, d_r_vecs, n_src, d_u, &noop);
  if (rc || noop) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const double *d_r = d_r_vecs;
  if (!d_r && (rc = rbl_positions_dev(c, &d_r, nullptr))) return rc;
  return vf_enqueue(c, d_points, n_points, d_lambda, d_r, n_src, d_u);
}

int rbl_velocity_field(rbl_ctx *c, const double *points, int64_t n_points, const double *lambda, const double *r_vecs, int64_t n_src,
                       double *u)
{
  bool noop;
  int rc = vf_check_args(c, points, n_points, lambda, r_vecs, n_src, u, &noop);
  if (rc || noop) return rc;
  if ((rc = rbl_dev_init(c))) return rc;
  const double *d_r = nullptr;
  if (!r_vecs && (rc = rbl_positions_dev(c, &d_r, nullptr))) return rc;
  // host staging: [points 3P | u 3P | lambda 3N | r 3N]
  const size_t pb = sizeof(double) * 3 * (size_t)n_points, nb = sizeof(double) * 3 * (size_t)n_src;
  if ((rc = rbl_dev_reserve(c, c->d_vf, 2 * pb + 2 * nb))) return rc;
  double *d_pts = (double *)c->d_vf.p, *d_u = d_pts + 3 * n_points, *d_lam = d_u + 3 * n_points, *d_rs = d_lam + 3 * n_src;
  if ((rc = copy_h2d(c, d_pts, points, pb))) return rc;
  if ((rc = copy_h2d(c, d_lam, lambda, nb))) return rc;
  if (r_vecs) {
    if ((rc = copy_h2d(c, d_rs, r_vecs, nb))) return rc;
    d_r = d_rs;
  }
  if ((rc = vf_enqueue(c, d_pts, n_points, d_lam, d_r, n_src, d_u))) return rc;
  if ((rc = copy_d2h(c, u, d_u, pb))) return rc;
  return finish_and_check(c);
}

int rbl_velocity_field_info(const rbl_ctx *cc, int64_t n_points, int64_t n_src, int *ni, int *chunks, int64_t *workspace_bytes)
{
  rbl_ctx *c = const_cast<rbl_ctx *>(cc);
  if (!c) return RBL_ERR_ARG;
  if (n_points < 0 || n_src <= 0) return rbl_fail(c, RBL_ERR_ARG, "velocity_field_info: need n_points >= 0, n_src > 0");
  int rc = rbl_dev_init(c); if (rc) return rc;
  const VfGeom g = vf_geometry(n_points, n_src, c->n_cu);
  const bool comm = comm_on(c);
  const int W = comm ? c->comm_world : 1, rank = comm ? c->comm_rank : 0;
  std::vector<int64_t> bounds;
  vf_shares(n_points, g, W, bounds);
  const int64_t nl = bounds[(size_t)rank + 1] - bounds[(size_t)rank];
  if (ni) *ni = g.NI;
  if (chunks) *chunks = g.nch;
  if (workspace_bytes) *workspace_bytes = (int64_t)(vf_src_bytes(g) + vf_slab_bytes(g, nl));
  return RBL_OK;
}
