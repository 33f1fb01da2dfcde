// Error summary of a cross-validation (gss.h, gss_cv_summary): one deterministic reduction over (z, pred, var, status,
// fold).  Every sum is formed in a fixed order -- a thread over its points in ascending order, the threads of a workgroup
// in a fixed tree, the workgroups one after the other in a single workgroup -- and nothing is added with floating-point
// atomics, so two runs on the same inputs give the same bits.
#include "gss_internal.h"

#include <cmath>
#include <cstring>

namespace gss {

constexpr int CV_NT = 256;        // threads per workgroup
constexpr int CV_NSUM = 9;        // n_ok, n_missing, n_singular, sum e, sum |e|, sum e^2, n_std, sum e / s, sum e^2 / s^2
constexpr int CV_MAX_GROUPS = 1024;

// sums of the CV_NT threads of a workgroup -> thread 0, fixed tree
__device__ __forceinline__ void cv_block_reduce(double (&v)[CV_NSUM], double (*sh)[CV_NT]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < CV_NSUM; ++q) sh[q][t] = v[q];
  __syncthreads();
  for (int half = CV_NT / 2; half >= 1; half >>= 1) {
    if (t < half) {
#pragma unroll
      for (int q = 0; q < CV_NSUM; ++q) sh[q][t] += sh[q][t + half];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < CV_NSUM; ++q) v[q] = sh[q][0];
}

// workgroup g sums the points [g * per, (g + 1) * per); partial[g * CV_NSUM + q]
__global__ __launch_bounds__(CV_NT) void cv_partial_kernel(const double* __restrict__ z, const double* __restrict__ pred,
                                                           const double* __restrict__ var,
                                                           const uint8_t* __restrict__ status, int64_t n, int64_t per,
                                                           double* __restrict__ partial) {
  __shared__ double sh[CV_NSUM][CV_NT];
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n ? lo + per : n;
  double v[CV_NSUM];
#pragma unroll
  for (int q = 0; q < CV_NSUM; ++q) v[q] = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += CV_NT) {
    const int st = status ? status[i] : GSS_PT_OK;
    if (st == GSS_PT_MISSING) v[1] += 1.0;
    else if (st != GSS_PT_OK) v[2] += 1.0;
    else {
      const double e = z[i] - pred[i];
      v[0] += 1.0;
      v[3] += e;
      v[4] += fabs(e);
      v[5] += e * e;
      const double s2 = var[i];
      if (s2 > 0.0) {
        v[6] += 1.0;
        v[7] += e / sqrt(s2);
        v[8] += e * e / s2;
      }
    }
  }
  cv_block_reduce(v, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < CV_NSUM; ++q) partial[(int64_t)blockIdx.x * CV_NSUM + q] = v[q];
  }
}

// one wave per fold: lane l visits the points l, l + 64, ... in that order and keeps those of its fold with GSS_PT_OK;
// the lane sums meet in a fixed butterfly.  fsum[f] = sum e^2, fcnt[f] = number of points.
__global__ __launch_bounds__(CV_NT) void cv_fold_kernel(const double* __restrict__ z, const double* __restrict__ pred,
                                                        const uint8_t* __restrict__ status,
                                                        const int* __restrict__ fold, int64_t n, int nfolds,
                                                        double* __restrict__ fsum, double* __restrict__ fcnt) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * (CV_NT / 64) + (threadIdx.x >> 6);
  if (f >= nfolds) return;  // whole wave
  double s = 0.0, c = 0.0;
  for (int64_t i = lane; i < n; i += 64) {
    if (fold[i] != f || (status && status[i] != GSS_PT_OK)) continue;
    const double e = z[i] - pred[i];
    s += e * e;
    c += 1.0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off);
    c += __shfl_xor(c, off);
  }
  if (lane == 0) {
    fsum[f] = s;
    fcnt[f] = c;
  }
}

// one workgroup: the partials in workgroup order, the folds in fold order; out = the ten doubles of gss_cv_summary_t
__global__ __launch_bounds__(CV_NT) void cv_final_kernel(const double* __restrict__ partial, int ngroups,
                                                         const double* __restrict__ fsum,
                                                         const double* __restrict__ fcnt, int nfolds,
                                                         double* __restrict__ fold_mse, double* __restrict__ out) {
  __shared__ double sh[CV_NSUM][CV_NT];
  const double NaN = __longlong_as_double(0x7ff8000000000000LL);
  double v[CV_NSUM];
#pragma unroll
  for (int q = 0; q < CV_NSUM; ++q) v[q] = 0.0;
  for (int g = threadIdx.x; g < ngroups; g += CV_NT) {
#pragma unroll
    for (int q = 0; q < CV_NSUM; ++q) v[q] += partial[(int64_t)g * CV_NSUM + q];
  }
  cv_block_reduce(v, sh);
  __syncthreads();
  // mean over the non-empty folds of the folds' mean squared errors (slots 0 and 1 of the same tree)
  double w[CV_NSUM];
#pragma unroll
  for (int q = 0; q < CV_NSUM; ++q) w[q] = 0.0;
  for (int f = threadIdx.x; f < nfolds; f += CV_NT) {
    const double c = fcnt[f];
    const double mse = c > 0.0 ? fsum[f] / c : NaN;
    if (fold_mse) fold_mse[f] = mse;
    if (c > 0.0) {
      w[0] += mse;
      w[1] += 1.0;
    }
  }
  cv_block_reduce(w, sh);
  if (threadIdx.x != 0) return;
  const double nok = v[0], nstd = v[6];
  out[0] = nok;
  out[1] = v[1];
  out[2] = v[2];
  out[3] = nok > 0.0 ? v[3] / nok : NaN;
  out[4] = nok > 0.0 ? v[4] / nok : NaN;
  out[5] = nok > 0.0 ? v[5] / nok : NaN;
  out[6] = nstd;
  out[7] = nstd > 0.0 ? v[7] / nstd : NaN;
  out[8] = nstd > 0.0 ? v[8] / nstd : NaN;
  out[9] = nfolds > 0 ? (w[1] > 0.0 ? w[0] / w[1] : NaN) : out[5];
}

}  // namespace gss

using namespace gss;

extern "C" int32_t gss_cv_summary(const double* z, const double* pred, const double* var, const uint8_t* status,
                                  const int32_t* fold, int64_t n, int32_t nfolds, gss_cv_summary_t* out,
                                  double* fold_mse, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(z && pred && var && out, "gss_cv_summary: NULL array");
  GSS_REQUIRE(n >= 1, "gss_cv_summary: n = %lld", (long long)n);
  GSS_REQUIRE(fold != nullptr || (nfolds == 0 && fold_mse == nullptr),
              "gss_cv_summary: nfolds = %d and fold_mse need fold ids (leave-one-out passes fold = NULL, nfolds = 0)", nfolds);
  GSS_REQUIRE(fold == nullptr || nfolds >= 1, "gss_cv_summary: fold ids need nfolds >= 1 (got %d)", nfolds);
  static_assert(sizeof(gss_cv_summary_t) == 10 * sizeof(double), "gss_cv_summary_t is ten doubles");
  hipStream_t s = to_stream(stream);
  Staged sz, sp, sv, sst, sf, sfm;
  GSS_TRY(sz.in(z, sizeof(double) * (size_t)n, mem, s));
  GSS_TRY(sp.in(pred, sizeof(double) * (size_t)n, mem, s));
  GSS_TRY(sv.in(var, sizeof(double) * (size_t)n, mem, s));
  GSS_TRY(sst.in(status, (size_t)n, mem, s));
  GSS_TRY(sf.in(fold, sizeof(int32_t) * (size_t)n, mem, s));
  GSS_TRY(sfm.out(fold_mse, sizeof(double) * (size_t)(nfolds > 0 ? nfolds : 1), mem));
  // a workgroup sums at least 4096 points; at most CV_MAX_GROUPS workgroups
  int64_t per = 4096;
  if ((n + per - 1) / per > CV_MAX_GROUPS) per = round_up((n + CV_MAX_GROUPS - 1) / CV_MAX_GROUPS, CV_NT);
  const int ngroups = (int)((n + per - 1) / per);
  const int nf = fold ? nfolds : 0;
  DevBuf work;
  GSS_TRY(work.alloc(sizeof(double) * (size_t)(ngroups * CV_NSUM + 2 * (nf > 0 ? nf : 1) + 10)));
  double* partial = work.as<double>();
  double* fsum = partial + (int64_t)ngroups * CV_NSUM;
  double* fcnt = fsum + (nf > 0 ? nf : 1);
  double* dout = fcnt + (nf > 0 ? nf : 1);
  {
    ProfScope ps("cv_summary", s);
    hipLaunchKernelGGL(cv_partial_kernel, dim3((unsigned)ngroups), dim3(CV_NT), 0, s, sz.as<double>(), sp.as<double>(),
                       sv.as<double>(), sst.as<uint8_t>(), n, per, partial);
    if (nf > 0)
      hipLaunchKernelGGL(cv_fold_kernel, dim3((unsigned)((nf + CV_NT / 64 - 1) / (CV_NT / 64))), dim3(CV_NT), 0, s,
                         sz.as<double>(), sp.as<double>(), sst.as<uint8_t>(), sf.as<int>(), n, nf, fsum, fcnt);
    hipLaunchKernelGGL(cv_final_kernel, dim3(1), dim3(CV_NT), 0, s, partial, ngroups, fsum, fcnt, nf,
                       nf > 0 ? sfm.as<double>() : nullptr, dout);
    GSS_HIP(hipGetLastError());
  }
  double host[10];
  GSS_HIP(hipMemcpyAsync(host, dout, sizeof(host), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  std::memcpy(out, host, sizeof(host));
  if (nf > 0) GSS_TRY(sfm.back(s));
  return GSS_OK;
}
