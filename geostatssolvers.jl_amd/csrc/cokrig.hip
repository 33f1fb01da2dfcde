// Cokriging (gss.h, gss_cokrig_create): the kriging system of krig.hip over the stacked samples of
// nz variables under C_ab(h) = b1[a][b] rho(h) (+ b0[a][b] at a zero key), with the per-variable indicators as constraint
// columns.  The factorisation, K3 and the cross-validation identities are those of the single-variable handle (krig.hip,
// krig_cv.hip); this unit holds what is cokriging's own:
//   cokrig_system_kernel  the n x n block of the system, replacing the pairwise covariances of the fit
//   cokrig_rhs_kernel     the right-hand sides of all nz targets from one evaluation of rho per (sample, point)
// the two creators, the global predictor and the entry of the moving neighbourhood (gss_cokrig_predict_knn), whose
// kernel and driver are in cokrig_local.hip.
#include "krig_handle.h"
#include "mfma_f64.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace gss {

// M[i * ldw + j] = C_{var_i var_j}(x_i, x_j) for i, j < n (the block is symmetric: the table is, and so is the key).
// Lane = column sample j, the row sample i is wave-uniform (cov_pairwise_kernel's layout).
template <int DIM>
__global__ __launch_bounds__(256) void cokrig_system_kernel(VgDev vg, const double* __restrict__ xd,
                                                            const int* __restrict__ var,
                                                            const double* __restrict__ tab, int n,
                                                            double* __restrict__ M, int64_t ldw) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int i0 = blockIdx.y * 64;
  const int i1 = i0 + 64 < n ? i0 + 64 : n;
  if (j >= n) return;
  double c[DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k) c[k] = xd[(int64_t)j * DIM + k];
  const int vj = var[j];
  for (int i = i0; i < i1; ++i) {
    double x[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) x[k] = xd[(int64_t)i * DIM + k];
    bool zero;
    const double rho = co_rho<DIM, -1>(vg, x, c, &zero);
    const int e = var[i] * CO_MAXZ + vj;
    M[(int64_t)i * ldw + j] = zero ? tab[CO_C0 + e] : tab[e] * rho;
  }
}

// Fd[c * n + i] = [var_i == c]: the unbiasedness columns of ordinary cokriging
__global__ __launch_bounds__(256) void cokrig_indicator_kernel(const int* __restrict__ var, int n, int nc,
                                                               double* __restrict__ Fd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = var[i];
  for (int c = 0; c < nc; ++c) Fd[(int64_t)c * n + i] = v == c ? 1.0 : 0.0;
}

// z_i -= means[var_i] (simple cokriging kriges the residuals)
__global__ __launch_bounds__(256) void cokrig_center_kernel(double* __restrict__ z, const int* __restrict__ var,
                                                            const double* __restrict__ tab, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) z[i] -= tab[CO_MEANS + var[i]];
}

// Right-hand sides of all targets: block t of R (blk = N1pad * ldr doubles apart) gets, in row j < n,
// b1[var_j][t] rho(x_j, x0_p), or c0[var_j][t] when the key is zero.  The unit walk, the two adjacent points per thread
// and the 16-B stores are those of krig_rhs2_kernel; rho is evaluated once per (sample, point) and scaled nz times.  j is
// wave-uniform, so x_j, var_j and row var_j of the two tables come through the scalar cache and the scale is a scalar
// operand of the multiply.
// nz is a run-time loop bound: the loop body keeps two products and two selects live whatever nz is, so the kernel
// needs no more registers than krig_rhs2_kernel plus the two key flags (DESIGN.md section 4 has the counts), and one
// instantiation per (DIM, KIND) serves nz = 1 .. 8.  Unrolling over a compile-time nz would only let the compiler
// hoist the nz scalar loads in front of the shape, which the scalar cache already hides behind the sqrt / exp chain.
template <int DIM, int KIND>
__global__ __launch_bounds__(256) void cokrig_rhs_kernel(VgDev vg, const double* __restrict__ xd,
                                                         const int* __restrict__ var, const double* __restrict__ tab,
                                                         int nz, int n, const double* __restrict__ x0, int64_t m_valid,
                                                         double* __restrict__ R, int64_t ldr, int64_t blk, int seg_len,
                                                         int nblk, int64_t ncols) {
  for (int unit = blockIdx.x; unit < nblk * NSEG; unit += gridDim.x) {
    const int seg = unit % NSEG;
    const int64_t p = (int64_t)(unit / NSEG) * 512 + 2 * threadIdx.x;
    if (p >= ncols) continue;
    const int64_t pa = p < m_valid ? p : m_valid - 1, pb = p + 1 < m_valid ? p + 1 : m_valid - 1;
    double ca[DIM], cb[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      ca[k] = x0[pa * DIM + k];
      cb[k] = x0[pb * DIM + k];
    }
    const int j0 = seg * seg_len;
    const int j1 = j0 + seg_len < n ? j0 + seg_len : n;
    double2* rp = reinterpret_cast<double2*>(R + (int64_t)j0 * ldr + p);
    const int64_t ld2 = ldr >> 1, blk2 = blk >> 1;
#pragma unroll 2
    for (int j = j0; j < j1; ++j) {
      double x[DIM];
#pragma unroll
      for (int k = 0; k < DIM; ++k) x[k] = xd[j * DIM + k];
      bool za, zb;
      const double ra = co_rho<DIM, KIND>(vg, x, ca, &za);
      const double rb = co_rho<DIM, KIND>(vg, x, cb, &zb);
      const double* row = tab + var[j] * CO_MAXZ;
      double2* rt = rp;
      for (int t = 0; t < nz; ++t) {
        const double b = row[t], c = row[CO_C0 + t];
        double2 v;
        v.x = za ? c : b * ra;
        v.y = zb ? c : b * rb;
        *rt = v;
        rt += blk2;
      }
      rp += ld2;
    }
  }
}

// rows n .. n + nrows - 1 of every block: the indicator [c == t] in row n + c (c < nc), zero rows up to N1pad
__global__ __launch_bounds__(256) void cokrig_tail_rows_kernel(double* __restrict__ R, int64_t ldr, int64_t blk, int n,
                                                               int nc, int nrows, int nz, int64_t ncols) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= ncols) return;
  for (int t = 0; t < nz; ++t)
    for (int r = 0; r < nrows; ++r) R[t * blk + (int64_t)(n + r) * ldr + p] = (r < nc && r == t) ? 1.0 : 0.0;
}

template <int DIM>
static int32_t launch_cokrig_rhs(hipStream_t s, const VgDev& vg, const double* xd, const int* var, const double* tab,
                                 int nz, int n, const double* x0, int64_t m_valid, double* R, int64_t ldr, int64_t blk,
                                 int seg_len, int nblk) {
  GSS_REQUIRE((ldr & 1) == 0 && (blk & 1) == 0, "launch_cokrig_rhs: odd leading dimension %lld (16-B stores need an "
              "even one)", (long long)ldr);
  const int64_t ncols = (int64_t)nblk * 256;
  const int nblk2 = (int)((ncols + 511) / 512);
  const dim3 g2((unsigned)(nblk2 * NSEG));
#define GSS_CK_LAUNCH(KIND)                                                                                          \
  hipLaunchKernelGGL((cokrig_rhs_kernel<DIM, KIND>), g2, dim3(256), 0, s, vg, xd, var, tab, nz, n, x0, m_valid, R,   \
                     ldr, blk, seg_len, nblk2, ncols)
  switch (vg.kind) {
    case GSS_VG_GAUSSIAN: GSS_CK_LAUNCH(GSS_VG_GAUSSIAN); break;
    case GSS_VG_EXPONENTIAL: GSS_CK_LAUNCH(GSS_VG_EXPONENTIAL); break;
    case GSS_VG_SPHERICAL: GSS_CK_LAUNCH(GSS_VG_SPHERICAL); break;
    case VG_MATERN12: GSS_CK_LAUNCH(VG_MATERN12); break;
    case VG_MATERN32: GSS_CK_LAUNCH(VG_MATERN32); break;
    case VG_MATERN52: GSS_CK_LAUNCH(VG_MATERN52); break;
    default: GSS_CK_LAUNCH(-1); break;
  }
#undef GSS_CK_LAUNCH
  return GSS_OK;
}

}  // namespace gss

using namespace gss;

// ---- what the fit (krig.hip) launches for a cokriging handle ------------------------------------------------------------
int32_t gss::cokrig_fit_system(const gss_krig* h, double* M, hipStream_t s) {
  const int64_t n = h->n, ldw = h->ldw;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)((n + 63) / 64));
  switch (h->dim) {
    case 1: hipLaunchKernelGGL(cokrig_system_kernel<1>, grid, dim3(256), 0, s, h->vg, h->xdata.as<double>(), h->covar.as<int>(), h->cotab.as<double>(), (int)n, M, ldw); break;
    case 2: hipLaunchKernelGGL(cokrig_system_kernel<2>, grid, dim3(256), 0, s, h->vg, h->xdata.as<double>(), h->covar.as<int>(), h->cotab.as<double>(), (int)n, M, ldw); break;
    default: hipLaunchKernelGGL(cokrig_system_kernel<3>, grid, dim3(256), 0, s, h->vg, h->xdata.as<double>(), h->covar.as<int>(), h->cotab.as<double>(), (int)n, M, ldw); break;
  }
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

int32_t gss::cokrig_fit_indicators(const gss_krig* h, double* Fd, hipStream_t s) {
  hipLaunchKernelGGL(cokrig_indicator_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, s,
                     h->covar.as<int>(), (int)h->n, h->nc, Fd);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

void gss::cokrig_fit_center(const gss_krig* h, double* zz, hipStream_t s) {
  hipLaunchKernelGGL(cokrig_center_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, s, zz,
                     h->covar.as<int>(), h->cotab.as<double>(), (int)h->n);
}

// entry points that know one variable only
int32_t gss::krig_refuse_cokrig(const gss_krig* h, const char* who) {
  GSS_REQUIRE(h->nz == 0, "%s: the handle is a cokriging system over %d variables; its estimates come from "
              "gss_cokrig_predict_global and gss_cokrig_predict_knn (cross-validation: gss_krig_cv_global, "
              "gss_krig_cv_global_folds, gss_cokrig_cv_knn)", who, h->nz);
  return GSS_OK;
}

void gss::cokrig_grouped(const gss_krig* h, CoGrouped* g) {
  g->x = h->co_xg.as<double>();
  g->x_raw = h->co_xg_raw.as<double>();
  g->zres = h->co_zres.as<double>();
  g->row = h->co_row.as<int>();
  g->tab = h->cotab.as<double>();
  g->nz = h->nz;
  for (int a = 0; a <= CO_MAXZ; ++a) g->off[a] = h->co_off[a];
}

int32_t gss::cokrig_knn_counts(const gss_krig* h, const char* who, const char* clamp_note, const int32_t* k, int* ksum) {
  if (h->nz > COL_MAXZ) {
    set_error("%s: the handle holds %d variables, the moving neighbourhood takes at most %d", who, h->nz, COL_MAXZ);
    return GSS_ERR_UNSUPPORTED;
  }
  GSS_REQUIRE(k != nullptr, "%s: k is NULL (one neighbour count per variable)", who);
  *ksum = 0;
  for (int a = 0; a < h->nz; ++a) {
    const int64_t na = h->co_off[a + 1] - h->co_off[a];
    GSS_REQUIRE(k[a] >= 1 && k[a] <= na, "%s: k[%d] = %d outside 1 .. %lld, the sample count of variable %d (a front-end "
                "clamps it%s)", who, a, k[a], (long long)na, a, clamp_note);
    *ksum += k[a];
  }
  if (*ksum > 64) {
    set_error("%s: %d neighbours in total, the tile kernel holds at most 64", who, *ksum);
    return GSS_ERR_UNSUPPORTED;
  }
  return GSS_OK;
}

int32_t gss::cokrig_searchers(const gss_krig* h, const CoGrouped& g, Searcher* sr, int32_t metric, double metric_param,
                              double radius, const double* inv_radii, hipStream_t s) {
  const int dim = h->dim;
  for (int a = 0; a < h->nz; ++a) {
    GSS_TRY(sr[a].init(metric, metric_param, radius, inv_radii, dim, &h->fr));
    GSS_TRY(sr[a].samples(g.x + g.off[a] * dim, g.x_raw ? g.x_raw + g.off[a] * dim : nullptr, g.off[a + 1] - g.off[a], s));
  }
  return GSS_OK;
}

// The body of both creators.  factor: fit the global system (gss_cokrig_create) or keep the samples only
// (gss_cokrig_create_local); who: the entry point the messages name.
static int32_t cokrig_create_impl(const char* who, bool factor, gss_krig_t** out, const gss_variogram_t* structure,
                                  int32_t nz, const double* b0, const double* b1, int32_t variant, const double* means,
                                  const double* xdata, const double* z, const int32_t* var, int64_t n, int32_t flags,
                                  void* stream) {
  GSS_REQUIRE(out != nullptr, "%s: out is NULL", who);
  *out = nullptr;
  GSS_REQUIRE(structure != nullptr, "%s: structure is NULL", who);
  GSS_REQUIRE(nz >= 1 && nz <= CO_MAXZ, "%s: nz = %d outside 1 .. %d", who, nz, CO_MAXZ);
  GSS_REQUIRE(b0 != nullptr && b1 != nullptr, "%s: b0 or b1 is NULL", who);
  if (structure->kind == GSS_VG_POWER) {
    set_error("%s: a power structure has no sill, the coregionalisation model needs one", who);
    return GSS_ERR_UNSUPPORTED;
  }
  GSS_REQUIRE(structure->nextra == 0, "%s: one structure plus nugget (nextra = %d)", who, structure->nextra);
  if (variant == GSS_KRIG_UNIVERSAL || variant == GSS_KRIG_EXTDRIFT) {
    set_error("%s: cokriging with a drift is not available (simple and ordinary only)", who);
    return GSS_ERR_UNSUPPORTED;
  }
  GSS_REQUIRE(variant == GSS_KRIG_SIMPLE || variant == GSS_KRIG_ORDINARY, "unknown kriging variant %d", variant);
  GSS_REQUIRE((flags & GSS_KRIG_NO_FACTOR) == 0, "%s: GSS_KRIG_NO_FACTOR is refused: a handle without a factor, for the "
              "moving neighbourhood only, comes from gss_cokrig_create_local", who);
  if (!factor && nz > COL_MAXZ) {
    set_error("%s: nz = %d: the moving neighbourhood takes at most %d variables (2 nz + 1 right-hand-side columns ride "
              "along in one 16-column tile)", who, nz, COL_MAXZ);
    return GSS_ERR_UNSUPPORTED;
  }
  GSS_REQUIRE(variant != GSS_KRIG_SIMPLE || means != nullptr, "%s: simple cokriging needs means[nz]", who);
  GSS_REQUIRE(xdata != nullptr && z != nullptr && var != nullptr, "%s: NULL data", who);
  GSS_REQUIRE(n >= 1, "all samples are missing, aborting...");
  GSS_REQUIRE(n < (1 << 30), "too many samples");

  // the coefficient table: b1 symmetrised (so that the system block and the right-hand sides read the same numbers
  // whichever index comes first), c0 = b0 + b1, the means
  double tab[CO_TAB] = {};
  double big = 0.0;
  for (int e = 0; e < nz * nz; ++e) {
    GSS_REQUIRE(std::isfinite(b0[e]) && std::isfinite(b1[e]), "%s: b0 / b1 entry [%d][%d] is not finite", who,
                e / nz, e % nz);
    big = std::fmax(big, std::fmax(std::fabs(b0[e]), std::fabs(b1[e])));
  }
  for (int a = 0; a < nz; ++a)
    for (int b = 0; b < nz; ++b) {
      GSS_REQUIRE(std::fabs(b0[a * nz + b] - b0[b * nz + a]) <= 1e-12 * big,
                  "%s: b0 is not symmetric at [%d][%d]", who, a, b);
      GSS_REQUIRE(std::fabs(b1[a * nz + b] - b1[b * nz + a]) <= 1e-12 * big,
                  "%s: b1 is not symmetric at [%d][%d]", who, a, b);
      const double s1 = 0.5 * (b1[a * nz + b] + b1[b * nz + a]), s0 = 0.5 * (b0[a * nz + b] + b0[b * nz + a]);
      tab[a * CO_MAXZ + b] = s1;
      tab[CO_C0 + a * CO_MAXZ + b] = s0 + s1;
    }
  for (int a = 0; a < nz; ++a)
    GSS_REQUIRE(tab[CO_C0 + a * CO_MAXZ + a] > 0.0, "%s: variable %d has no positive sill "
                "b0[%d][%d] + b1[%d][%d]", who, a, a, a, a, a);
  if (variant == GSS_KRIG_SIMPLE)
    for (int a = 0; a < nz; ++a) {
      GSS_REQUIRE(std::isfinite(means[a]), "%s: means[%d] is not finite", who, a);
      tab[CO_MEANS + a] = means[a];
    }

  gss_krig* h = new (std::nothrow) gss_krig();
  if (!h) return GSS_ERR_ALLOC;
  struct Guard {
    gss_krig* h;
    ~Guard() { delete h; }
  } guard{h};
  gss_variogram_t unit = *structure, plain;   // rho: sill 1, no nugget
  unit.sill = 1.0;
  unit.nugget = 0.0;
  GSS_TRY(vg_frame_split(&unit, &plain, &h->fr));
  GSS_TRY(make_vgdev(&plain, &h->vg));
  const int dim = h->vg.dim;
  int64_t per[CO_MAXZ] = {};
  for (int64_t i = 0; i < n; ++i) {
    GSS_REQUIRE(var[i] >= 0 && var[i] < nz, "%s: variable id %d of sample %lld outside 0 .. %d", who, var[i],
                (long long)i, nz - 1);
    GSS_REQUIRE(std::isfinite(z[i]), "%s: value of sample %lld is not finite", who, (long long)i);
    for (int k = 0; k < dim; ++k)
      GSS_REQUIRE(std::isfinite(xdata[i * dim + k]), "%s: coordinate %d of sample %lld is not finite", who, k,
                  (long long)i);
    ++per[var[i]];
  }
  if (variant == GSS_KRIG_ORDINARY)
    for (int a = 0; a < nz; ++a)
      GSS_REQUIRE(per[a] >= 1, "%s: variable %d has no sample (ordinary cokriging needs one "
                  "unbiasedness row per variable)", who, a);

  GSS_TRY(frame_origin(&h->fr, xdata, GSS_MEM_HOST, nullptr));
  h->variant = variant;
  h->dim = dim;
  h->n = n;
  h->nz = nz;
  for (int a = 0; a < nz; ++a) {
    h->c00[a] = tab[CO_C0 + a * CO_MAXZ + a];
    h->means[a] = tab[CO_MEANS + a];
  }
  std::memset(&h->ds, 0, sizeof(h->ds));
  h->ds.variant = variant;
  h->ds.dim = dim;
  for (int k = 0; k < 3; ++k) h->ds.inv_scale[k] = 1.0;
  h->nc = variant == GSS_KRIG_ORDINARY ? nz : 0;
  h->ds.nc = h->nc;
  h->N1 = n + h->nc;
  h->N1pad = round_up(h->N1 + 1, BK);   // (the spare row of the dual weights: gss_krig_create)
  h->ldw = round_up(h->N1 + 1, BM);

  hipStream_t s = to_stream(stream);
  GSS_TRY(h->z.alloc(sizeof(double) * (size_t)n));
  GSS_TRY(h->covar.alloc(sizeof(int32_t) * (size_t)n));
  GSS_TRY(h->cotab.alloc(sizeof(tab)));
  GSS_TRY(krig_upload_samples(h->fr, xdata, n, dim, &h->xdata, &h->xraw, s));
  GSS_HIP(hipMemcpyAsync(h->z.p, z, sizeof(double) * n, hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(h->covar.p, var, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(h->cotab.p, tab, sizeof(tab), hipMemcpyHostToDevice, s));
  // grouped by variable, the caller's order inside a variable: what the per-variable searches index
  {
    std::vector<double> xg((size_t)(n * dim)), zr((size_t)n);
    std::vector<int32_t> row((size_t)n);
    int64_t at[CO_MAXZ];
    h->co_off[0] = 0;
    for (int a = 0; a < CO_MAXZ; ++a) {
      at[a] = h->co_off[a];
      h->co_off[a + 1] = h->co_off[a] + per[a];
    }
    for (int64_t i = 0; i < n; ++i) {
      const int64_t j = at[var[i]]++;
      for (int k = 0; k < dim; ++k) xg[(size_t)(j * dim + k)] = xdata[i * dim + k];
      zr[(size_t)j] = z[i] - tab[CO_MEANS + var[i]];
      row[(size_t)j] = (int32_t)i;
    }
    GSS_TRY(h->co_zres.alloc(sizeof(double) * (size_t)n));
    GSS_TRY(h->co_row.alloc(sizeof(int32_t) * (size_t)n));
    GSS_TRY(krig_upload_samples(h->fr, xg.data(), n, dim, &h->co_xg, &h->co_xg_raw, s));
    GSS_HIP(hipMemcpyAsync(h->co_zres.p, zr.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
    GSS_HIP(hipMemcpyAsync(h->co_row.p, row.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    GSS_HIP(hipStreamSynchronize(s));   // tab and the grouped copies live on this frame
  }
  if (factor) {
    const bool async = (flags & GSS_KRIG_ASYNC_FIT) != 0;
    GSS_TRY(krig_factorize(h, s, async));
    if (!async) GSS_TRY(krig_fit_wait(h));   // otherwise joined by the first call that needs the factor
  }
  guard.h = nullptr;
  *out = h;
  return GSS_OK;
}

extern "C" {

int32_t gss_cokrig_create(gss_krig_t** out, const gss_variogram_t* structure, int32_t nz, const double* b0,
                          const double* b1, int32_t variant, const double* means, const double* xdata,
                          const double* z, const int32_t* var, int64_t n, int32_t flags, void* stream) {
  GSS_ENTRY();
  return cokrig_create_impl("gss_cokrig_create", true, out, structure, nz, b0, b1, variant, means, xdata, z, var, n,
                            flags, stream);
}

int32_t gss_cokrig_create_local(gss_krig_t** out, const gss_variogram_t* structure, int32_t nz, const double* b0,
                                const double* b1, int32_t variant, const double* means, const double* xdata,
                                const double* z, const int32_t* var, int64_t n, void* stream) {
  GSS_ENTRY();
  return cokrig_create_impl("gss_cokrig_create_local", false, out, structure, nz, b0, b1, variant, means, xdata, z, var,
                            n, 0, stream);
}

int32_t gss_cokrig_predict_global(gss_krig_t* h, const double* xdom, int64_t m, double* mean, double* variance,
                                  uint8_t* status, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(h->nz > 0, "gss_cokrig_predict_global: the handle is not a cokriging system (gss_cokrig_create makes one)");
  GSS_REQUIRE(h->factored, "handle has no factor");
  GSS_REQUIRE(m >= 0 && (m == 0 || (xdom && mean && variance)), "gss_cokrig_predict_global: NULL array");
  if (m == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  const int dim = h->dim, nz = h->nz;
  GSS_TRY(krig_quadform_attrs());

  int64_t mc = cokrig_chunk_cap(krig_chunk_points(h->N1pad * nz, m));   // the workspace holds nz blocks of N1pad rows
  DomainCall dc;   // host arrays: pieces of the call overlap their transfers with the computation of their neighbours
  Staged& sx = *dc.in(xdom, sizeof(double) * dim);
  Staged& smean = *dc.out(mean, sizeof(double), nz);
  Staged& svar = *dc.out(variance, sizeof(double), nz);
  Staged& sstat = *dc.out(status, 1, nz);
  GSS_TRY(dc.begin(mem, m, s, true, &h->fr));
  if (dc.piped && mc > HostPipe::PIECE) mc = HostPipe::PIECE;
  double *Rws = nullptr, *mpart = nullptr;
  GSS_TRY(krig_workspace(h->N1pad * nz, mc, s, &Rws, &mpart));
  const int64_t ldr = mc, blk = h->N1pad * ldr;
  const int seg_len = (int)((h->n + NSEG - 1) / NSEG);

  for (int64_t off = 0; off < m; off += mc) {
    const int64_t mv = (m - off) < mc ? (m - off) : mc;
    const int64_t cols = round_up(mv, 256);  // multiple of BN as well
    const double* x0 = sx.as<double>() + off * dim;
    GSS_TRY(dc.pipe.fetch(off, mv, s));
    const int nblk = (int)(cols / 256);
    const int nrows = (int)(h->N1pad - h->n);
    {
      ProfScope ps("cokrig_rhs", s);
      const double* xd = h->xdata.as<double>();
      const int* cv = h->covar.as<int>();
      const double* tab = h->cotab.as<double>();
      switch (dim) {
        case 1: GSS_TRY(launch_cokrig_rhs<1>(s, h->vg, xd, cv, tab, nz, (int)h->n, x0, mv, Rws, ldr, blk, seg_len, nblk)); break;
        case 2: GSS_TRY(launch_cokrig_rhs<2>(s, h->vg, xd, cv, tab, nz, (int)h->n, x0, mv, Rws, ldr, blk, seg_len, nblk)); break;
        default: GSS_TRY(launch_cokrig_rhs<3>(s, h->vg, xd, cv, tab, nz, (int)h->n, x0, mv, Rws, ldr, blk, seg_len, nblk)); break;
      }
      hipLaunchKernelGGL(cokrig_tail_rows_kernel, dim3((unsigned)(cols / 256)), dim3(256), 0, s, Rws, ldr, blk,
                         (int)h->n, h->nc, nrows, nz, cols);
      GSS_HIP(hipGetLastError());
    }
    GSS_TRY(krig_join_device(h, s));   // an asynchronous fit ran beside the assembly; the quadratic form needs it
    {
      ProfScope pq("krig_quadform", s);
      for (int t = 0; t < nz; ++t) {
        uint8_t* stp = status ? sstat.as<uint8_t>() + t * m + off : nullptr;
        launch_krig_quadform(h, Rws + t * blk, ldr, h->c00[t], h->means[t], mv, cols,
                             smean.as<double>() + t * m + off, svar.as<double>() + t * m + off, stp, mpart, s);
      }
    }
    GSS_HIP(hipGetLastError());
    GSS_TRY(dc.pipe.deliver(off, mv, s));
  }
  GSS_TRY(dc.finish(s));
  return krig_fit_wait(h);   // status of an asynchronous fit (it finished while the assembly ran)
}

int32_t gss_cokrig_predict_knn(gss_krig_t* h, const double* xdom, int64_t m, const int32_t* k, int32_t minneighbors,
                               double radius, const double* inv_radii, int32_t metric, double metric_param,
                               double* mean, double* variance, uint8_t* status, int32_t* idx_out, int32_t* count_out,
                               int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(h->nz > 0, "gss_cokrig_predict_knn: the handle is not a cokriging system (gss_cokrig_create and "
              "gss_cokrig_create_local make one)");
  const int nz = h->nz, dim = h->dim;
  int ksum = 0;
  GSS_TRY(cokrig_knn_counts(h, "gss_cokrig_predict_knn", "; gss_cokrig_predict_global uses every sample", k, &ksum));
  GSS_REQUIRE(m >= 0 && (m == 0 || (xdom && mean && variance)), "gss_cokrig_predict_knn: NULL array");

  hipStream_t s = to_stream(stream);
  CoGrouped g;
  cokrig_grouped(h, &g);
  Searcher sr[COL_MAXZ];
  GSS_TRY(cokrig_searchers(h, g, sr, metric, metric_param, radius, inv_radii, s));
  if (m == 0) return GSS_OK;
  DomainCall dc;   // host arrays: in and out piece by piece beside the computation (gss_internal.h)
  dc.in(xdom, sizeof(double) * dim);
  Staged& smean = *dc.out(mean, sizeof(double), nz);
  Staged& svar = *dc.out(variance, sizeof(double), nz);
  Staged& sstat = *dc.out(status, 1, nz);
  Staged& sidx = *dc.out(idx_out, sizeof(int32_t) * (size_t)ksum);
  Staged& scnt = *dc.out(count_out, sizeof(int32_t) * (size_t)nz);
  GSS_TRY(dc.begin(mem, m, s, !sr[0].two_frames, &h->fr));   // two frames: the domain is needed twice, it comes in whole
  GSS_TRY(cokrig_local_dev(h->vg, h->variant, dim, g, sr, k, minneighbors, dc.x(), sr[0].two_frames ? dc.x_raw : nullptr,
                           m, smean.as<double>(), svar.as<double>(), sstat.as<uint8_t>(), m, sidx.as<int>(),
                           scnt.as<int>(), s, &dc.pipe));
  return dc.finish(s);   // (piped: cokrig_local_dev ended with pipe.finish, everything is home)
}

}  // extern "C"
