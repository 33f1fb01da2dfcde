// Cross-validation of a kriging or cokriging handle (gss.h): every sample predicted from samples outside its own fold.
// Global neighbourhood: leave-one-out off the factor (krig_loo_kernel) and folds off the factor (crossval_folds.hip);
// moving neighbourhood: the fold-aware search with the drivers of krig_local.hip and cokrig_cv.hip.
#include "cv_fold.h"
#include "krig_handle.h"

#include <vector>

namespace gss {

// Leave-one-out from the factor (gss_krig_cv_global; Dubrule 1983): K^-1 = W'^T D W' with D = +1 on the n data rows and
// -1 on the nc constraint rows, so B_ii = (K^-1)_ii = sum_{k=i}^{N1-1} D_k W'(k, i)^2 -- W' is lower triangular and its
// columns are contiguous.  Row N1 of W' holds the dual weights (wd_row_kernel): it is not part of the factor and the
// sum stops in front of it.  One wave per column; lane l adds rows i + l, i + l + 64, ... in that order, the 64 lane
// sums meet in a fixed butterfly: the same bits on every run.  pred_i = z_i - wd_i / B_ii (wd was formed from z - mean
// for simple kriging, so the mean cancels), var_i = max(0, 1 / B_ii) = the Schur complement of the system without i.
__global__ __launch_bounds__(256) void krig_loo_kernel(const double* __restrict__ Wp, int64_t ldw, int n, int N1,
                                                       const double* __restrict__ wd, const double* __restrict__ z,
                                                       double* __restrict__ pred, double* __restrict__ var,
                                                       uint8_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // whole wave
  const double* col = Wp + (int64_t)i * ldw;
  double acc = 0.0;
  for (int k = i + lane; k < N1; k += 64) {
    const double w = col[k];
    acc = k < n ? fma(w, w, acc) : fma(-w, w, acc);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane != 0) return;
  const double NaN = __longlong_as_double(0x7ff8000000000000LL);
  const bool ok = acc > 0.0 && acc < __builtin_huge_val();
  const double v = 1.0 / acc;
  pred[i] = ok ? z[i] - wd[i] * v : NaN;
  var[i] = ok ? (v > 0.0 ? v : 0.0) : NaN;
  if (status) status[i] = ok ? GSS_PT_OK : GSS_PT_SINGULAR;
}

}  // namespace gss

using namespace gss;

extern "C" {

// ---- cross-validation (gss.h): every sample predicted from samples outside its own fold ------------------------------
int32_t gss_krig_cv_global(gss_krig_t* h, double* pred, double* var, uint8_t* status, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(h->factored, "gss_krig_cv_global: the handle has no factor (created with GSS_KRIG_NO_FACTOR and never "
                           "adopted one); gss_krig_cv_knn works without");
  GSS_REQUIRE(h->block_nsub == 0, "cross-validation is at point support: the handle has block support set");
  GSS_REQUIRE(pred && var, "gss_krig_cv_global: NULL array");
  hipStream_t s = to_stream(stream);
  GSS_TRY(krig_join_device(h, s));
  GSS_TRY(krig_fit_wait(h));   // an asynchronous fit: its status (GSS_ERR_NOT_POSDEF) is reported here
  const int64_t n = h->n;
  DomainCall dc;   // the outputs over the n samples (whole: nothing is piped)
  Staged &sp = *dc.out(pred, sizeof(double)), &sv = *dc.out(var, sizeof(double)), &sst = *dc.out(status, 1);
  GSS_TRY(dc.begin(mem, n, s, false, nullptr));
  {
    ProfScope ps("krig_loo", s);
    hipLaunchKernelGGL(krig_loo_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, h->Wp(), h->ldw, (int)n,
                       (int)h->N1, h->wd(), h->z.as<double>(), sp.as<double>(), sv.as<double>(), sst.as<uint8_t>());
    GSS_HIP(hipGetLastError());
  }
  return dc.finish(s);
}

// Folds under the global neighbourhood: the block form of the identity above, e_F = (B_FF)^-1 wd_F (crossval_folds.hip)
int32_t gss_krig_cv_global_folds(gss_krig_t* h, const int32_t* fold, double* pred, double* var, uint8_t* status,
                                 int32_t mem, void* stream) {
  GSS_ENTRY();
  if (fold == nullptr) return gss_krig_cv_global(h, pred, var, status, mem, stream);
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(h->factored, "gss_krig_cv_global_folds: the handle has no factor (created with GSS_KRIG_NO_FACTOR and "
                           "never adopted one); gss_krig_cv_knn works without");
  GSS_REQUIRE(h->block_nsub == 0, "cross-validation is at point support: the handle has block support set");
  GSS_REQUIRE(pred && var, "gss_krig_cv_global_folds: NULL array");
  hipStream_t s = to_stream(stream);
  GSS_TRY(krig_join_device(h, s));
  GSS_TRY(krig_fit_wait(h));   // an asynchronous fit: its status (GSS_ERR_NOT_POSDEF) is reported here
  const int64_t n = h->n;
  std::vector<int32_t> fh;   // the samples are grouped by fold on the host
  GSS_TRY(fold_ids_host("gss_krig_cv_global_folds", fold, n, mem, s, &fh));
  const int32_t* fhost = mem != GSS_MEM_HOST ? fh.data() : fold;
  DomainCall dc;   // the outputs over the n samples (whole: nothing is piped)
  Staged &sp = *dc.out(pred, sizeof(double)), &sv = *dc.out(var, sizeof(double)), &sst = *dc.out(status, 1);
  GSS_TRY(dc.begin(mem, n, s, false, nullptr));
  GSS_TRY(cv_global_folds_dev(h->Wp(), h->ldw, n, h->N1, h->nc, h->variant == GSS_KRIG_SIMPLE, h->wd(),
                              h->z.as<double>(), fhost, sp.as<double>(), sv.as<double>(), sst.as<uint8_t>(), s));
  return dc.finish(s);
}

int32_t gss_krig_cv_knn(gss_krig_t* h, const int32_t* fold, double exclude_radius, int32_t k, int32_t minneighbors,
                        double radius, const double* inv_radii, int32_t metric, double metric_param, double* pred,
                        double* var, uint8_t* status, int32_t* idx_out, int32_t* count_out, int32_t mem,
                        void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_TRY(krig_refuse_cokrig(h, "gss_krig_cv_knn"));
  if (metric == GSS_METRIC_HAVERSINE) {
    set_error("cross-validation under the haversine distance is not available: the fold search runs on the k-d index, "
              "which that key has no box bounds for (DESIGN.md section 7)");
    return GSS_ERR_UNSUPPORTED;
  }
  Searcher sr;
  GSS_TRY(sr.init(metric, metric_param, radius, inv_radii, h->dim, &h->fr));
  GSS_REQUIRE(h->block_nsub == 0, "cross-validation is at point support: the handle has block support set");
  GSS_REQUIRE(pred && var, "gss_krig_cv_knn: NULL array");
  const int64_t n = h->n;
  GSS_REQUIRE(k >= 1 && k <= n - 1, "gss_krig_cv_knn: maxneighbors %d outside 1..n-1 = %lld (a sample is never its own "
                                    "neighbour)", k, (long long)(n - 1));
  GSS_REQUIRE(!(exclude_radius != exclude_radius), "gss_krig_cv_knn: exclude_radius is NaN");
  hipStream_t s = to_stream(stream);
  const int dim = h->dim;
  Staged sf;
  std::vector<int32_t> fh;
  if (fold) {
    GSS_TRY(fold_ids_host("gss_krig_cv_knn", fold, n, mem, s, &fh));
    GSS_TRY(sf.in(fold, sizeof(int32_t) * (size_t)n, mem, s));
  }
  DomainCall dc;   // the outputs over the n samples (whole: nothing is piped)
  Staged &smean = *dc.out(pred, sizeof(double)), &svar = *dc.out(var, sizeof(double)), &sstat = *dc.out(status, 1);
  Staged &sidx = *dc.out(idx_out, sizeof(int32_t) * (size_t)k), &scnt = *dc.out(count_out, sizeof(int32_t));
  GSS_TRY(dc.begin(mem, n, s, false, nullptr));
  GSS_TRY(sr.samples(h->xdata.as<double>(), h->xraw.as<double>(), n, s));
  const double ex = exclusion_key(exclude_radius, sr.metric);
  const int* fold_dev = fold ? sf.as<int>() : nullptr;   // the samples are the queries: one array serves both
  const KnnMask mask(KnnMask::Fold{fold_dev, fold_dev, 0, ex});
  // the queries are the samples themselves: covariance frame, raw frame for a search in a second one, own drift rows
  // (xraw only exists beside a rotated variogram; without one xdata holds the coordinates as given)
  const double* xq_raw = h->fr.on ? h->xraw.as<double>() : h->xdata.as<double>();
  GSS_TRY(krig_local_dev(h->vg, h->variant, h->nc, dim, &h->ds.e[0][0], h->ds.inv_scale[0], h->sk_mean, sr,
                         h->xdata.as<double>(), h->z.as<double>(), h->drift_data.as<double>(), h->xdata.as<double>(),
                         sr.two_frames ? xq_raw : nullptr, h->drift_data.as<double>(), n, k, minneighbors,
                         smean.as<double>(), svar.as<double>(), sstat.as<uint8_t>(), sidx.as<int>(), scnt.as<int>(), s,
                         nullptr, 0, nullptr, 0.0, &mask));
  return dc.finish(s);
}

int32_t gss_cokrig_cv_knn(gss_krig_t* h, const int32_t* fold, double exclude_radius, const int32_t* k,
                          int32_t minneighbors, double radius, const double* inv_radii, int32_t metric,
                          double metric_param, double* pred, double* var, uint8_t* status, int32_t* idx_out,
                          int32_t* count_out, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(h->nz > 0, "gss_cokrig_cv_knn: the handle is not a cokriging system (gss_cokrig_create and "
              "gss_cokrig_create_local make one; one variable: gss_krig_cv_knn)");
  const int nz = h->nz, dim = h->dim;
  int ksum = 0;
  GSS_TRY(cokrig_knn_counts(h, "gss_cokrig_cv_knn", "", k, &ksum));
  if (metric == GSS_METRIC_HAVERSINE) {
    set_error("gss_cokrig_cv_knn: cross-validation under the haversine distance is not available: the fold search runs "
              "on the k-d index, which that key has no box bounds for (DESIGN.md section 7)");
    return GSS_ERR_UNSUPPORTED;
  }
  GSS_REQUIRE(!(exclude_radius != exclude_radius), "gss_cokrig_cv_knn: exclude_radius is NaN");
  GSS_REQUIRE(pred && var, "gss_cokrig_cv_knn: NULL array");
  hipStream_t s = to_stream(stream);
  CoGrouped g;
  cokrig_grouped(h, &g);
  Searcher sr[COL_MAXZ];
  GSS_TRY(cokrig_searchers(h, g, sr, metric, metric_param, radius, inv_radii, s));
  const int64_t n = h->n;
  Staged sf;
  std::vector<int32_t> fh;
  if (fold) {
    GSS_TRY(fold_ids_host("gss_cokrig_cv_knn", fold, n, mem, s, &fh));
    GSS_TRY(sf.in(fold, sizeof(int32_t) * (size_t)n, mem, s));
  }
  DomainCall dc;   // the outputs over the n samples (whole: nothing is piped)
  Staged &smean = *dc.out(pred, sizeof(double)), &svar = *dc.out(var, sizeof(double)), &sstat = *dc.out(status, 1);
  Staged &sidx = *dc.out(idx_out, sizeof(int32_t) * (size_t)ksum), &scnt = *dc.out(count_out, sizeof(int32_t) * (size_t)nz);
  GSS_TRY(dc.begin(mem, n, s, false, nullptr));
  const double ex = exclusion_key(exclude_radius, sr[0].metric);
  GSS_TRY(cokrig_cv_dev(h->vg, h->variant, dim, g, sr, k, minneighbors, sf.as<int>(), ex, smean.as<double>(),
                        svar.as<double>(), sstat.as<uint8_t>(), sidx.as<int>(), scnt.as<int>(), s));
  return dc.finish(s);
}

}  // extern "C"
