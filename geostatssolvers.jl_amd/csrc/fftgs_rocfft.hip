// FFTGS on rocFFT: the pipeline of every grid that the fused (fftgs_fused.hip) and the generic passes
// (fftgs_generic.hip) do not take, and of GSS_FFTGS_PATH=rocfft.
//   spectrum:     fftgs_cov_kernel (K6) -> R2C -> fftgs_amp_kernel
//   realisation:  noise kernel -> R2C -> fftgs_phase_kernel (K7) -> C2R, `batch` realisations per execution on small grids
// HBM traffic per realisation (FP64, N cells): noise 8N (w) + R2C + phase 8N+4N (r) 8N (w) + C2R; the algorithmic
// floor is 32 N bytes.
#include "fftgs_handle.h"

#include <sys/stat.h>
#include <cerrno>
#include <array>
#include <list>
#include <mutex>
#include <string>
#include <utility>

namespace gss {

// C[e] = cov(|lag|) with lag = (cell - centre) * spacing, written as a contiguous real array
__global__ __launch_bounds__(256) void fftgs_cov_kernel(VgDev vg, GridSpec g, double* __restrict__ C) {
  const int64_t N = g.n1 * g.n2 * g.n3;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (int64_t)gridDim.x * 256) {
    const int64_t i1 = e % g.n1, i2 = (e / g.n1) % g.n2, i3 = e / (g.n1 * g.n2);
    double a[3] = {(double)(i1 - g.c1) * g.s1, (double)(i2 - g.c2) * g.s2, (double)(i3 - g.c3) * g.s3};
    const double zero[3] = {0.0, 0.0, 0.0};
    C[e] = cov_pair<3>(vg, a, zero);
  }
}

// the same for a rotated variogram: lag := R^T lag (R row-major 3 x 3 in HBM)
__global__ __launch_bounds__(256) void fftgs_cov_rot_kernel(VgDev vg, GridSpec g, const double* __restrict__ R,
                                                            double* __restrict__ C) {
  const int64_t N = g.n1 * g.n2 * g.n3;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (int64_t)gridDim.x * 256) {
    const int64_t i1 = e % g.n1, i2 = (e / g.n1) % g.n2, i3 = e / (g.n1 * g.n2);
    double a[3] = {(double)(i1 - g.c1) * g.s1, (double)(i2 - g.c2) * g.s2, (double)(i3 - g.c3) * g.s3};
    rotate_lag(R, a);
    const double zero[3] = {0.0, 0.0, 0.0};
    C[e] = cov_pair<3>(vg, a, zero);
  }
}

// Fh[idx] = sqrt(|X[idx]|) (DC = 0); partial[b] = sum over this block's elements of w * F^2 where w
// counts how many full-spectrum entries the half-spectrum entry stands for
__global__ __launch_bounds__(256) void fftgs_amp_kernel(GridSpec g, const double2* __restrict__ X,
                                                        double* __restrict__ Fh, double* __restrict__ partial) {
  __shared__ double red[256];
  const int64_t NH = g.nh * g.n2 * g.n3;
  double acc = 0.0;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < NH; idx += (int64_t)gridDim.x * 256) {
    const int64_t k1 = idx % g.nh;
    const double2 x = X[idx];
    double f = sqrt(sqrt(x.x * x.x + x.y * x.y));
    if (idx == 0) f = 0.0;  // fft.jl:103
    Fh[idx] = f;
    const bool self = (k1 == 0) || (2 * k1 == g.n1);
    acc += (self ? 1.0 : 2.0) * f * f;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// K7: X <- Fh * X / |X| (phase of the noise spectrum, amplitude of the covariance); DC <- mean
// (blockIdx.y: member of a batch of realisations, half spectra NH apart)
__global__ __launch_bounds__(256) void fftgs_phase_kernel(double2* __restrict__ X, const double* __restrict__ Fh,
                                                          int64_t NH, double mean) {
  X += (int64_t)blockIdx.y * NH;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < NH; idx += (int64_t)gridDim.x * 256) {
    const double2 x = X[idx];
    const double f = Fh[idx];
    const double mag2 = x.x * x.x + x.y * x.y;
    double2 p;
    if (mag2 > 0.0) {
      const double inv = f / sqrt(mag2);
      p.x = x.x * inv;
      p.y = x.y * inv;
    } else {  // angle(0) = 0
      p.x = f;
      p.y = 0.0;
    }
    if (idx == 0) {
      p.x = mean;
      p.y = 0.0;
    }
    X[idx] = p;
  }
}

// The two rocFFT plans of a grid size.  A plan describes the transform and is executed with the execution info of the
// handle that runs it (its own work buffer and stream), so handles of the same size share one pair; the library keeps
// the pairs of the last eight sizes alive between handles -- creating a pair costs 2-3 ms even when rocFFT finds its
// compiled kernels, which is most of a `solve` on the 100 x 100 grids of the reference's tests
// (tools/small_problem_latency.py).
struct FftPlans {
  rocfft_plan fwd = nullptr, inv = nullptr;
  size_t work_bytes = 0;
  // the same transforms for `batch` realisations at a time (small grids: the pipeline is four to ten launches whatever
  // the grid, created on the first call with enough realisations)
  rocfft_plan fwdB = nullptr, invB = nullptr;
  int batch = 0;
  size_t work_bytesB = 0;
  ~FftPlans() {
    if (fwd) rocfft_plan_destroy(fwd);
    if (inv) rocfft_plan_destroy(inv);
    if (fwdB) rocfft_plan_destroy(fwdB);
    if (invB) rocfft_plan_destroy(invB);
  }
};

static int32_t fft_exec(gss_fftgs* h, rocfft_plan plan, void* in, void* out, hipStream_t s) {
  GSS_FFT(rocfft_execution_info_set_stream(h->info, s));
  void* ib[1] = {in};
  void* ob[1] = {out};
  GSS_FFT(rocfft_execute(plan, ib, ob, h->info));
  return GSS_OK;
}

// rocFFT compiles the kernels of a grid size at run time (0.5 - 1.7 s per new size) and, left alone, forgets them
// when the process ends.  Unless the user chose a place (ROCFFT_RTC_CACHE_PATH), the compiled kernels are kept in
// $XDG_CACHE_HOME or ~/.cache, gss_hip/rocfft_kernels.db: the first plan of a later process then costs 0.1 s and
// further sizes a few milliseconds (measured: 1 024 x 1 024 cells 1.7 s -> 0.11 s, 100 x 100 cells 1.2 s -> 4 ms).
static void rocfft_kernel_cache_default() {
  if (std::getenv("ROCFFT_RTC_CACHE_PATH")) return;
  std::string dir;
  if (const char* x = std::getenv("XDG_CACHE_HOME")) dir = x;
  else if (const char* hm = std::getenv("HOME")) dir = std::string(hm) + "/.cache";
  if (dir.empty()) return;
  (void)mkdir(dir.c_str(), 0700);            // an existing directory is fine; a failure leaves rocFFT on its own
  dir += "/gss_hip";
  if (mkdir(dir.c_str(), 0700) != 0 && errno != EEXIST) return;
  (void)setenv("ROCFFT_RTC_CACHE_PATH", (dir + "/rocfft_kernels.db").c_str(), 0);
}

// rocFFT plans (run-time compiled: ~1.5 s the first time a size is seen), their work buffer and the natural-layout
// buffers of this pipeline; the other pipelines never need them
static int32_t ensure_rocfft(gss_fftgs* h) {
  if (h->fwd) return GSS_OK;
  static std::once_flag once;
  std::call_once(once, [] {
    rocfft_kernel_cache_default();
    rocfft_setup();
  });
  using Key = std::array<size_t, 5>;   // rocFFT plans belong to the device that was current when they were made
  // most recent first; calls hold the library lock; never destroyed (at exit rocFFT's own statics may be gone first)
  static auto& cache = *new std::list<std::pair<Key, std::shared_ptr<FftPlans>>>();
  int dev = 0;
  GSS_HIP(hipGetDevice(&dev));
  const Key key = {(size_t)h->ndim, (size_t)h->g.n1, (size_t)h->g.n2, (size_t)h->g.n3, (size_t)dev};
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->first == key) {
      h->plans = it->second;
      cache.splice(cache.begin(), cache, it);
      break;
    }
  if (!h->plans) {
    auto pl = std::make_shared<FftPlans>();
    size_t lengths[3] = {(size_t)h->g.n1, (size_t)h->g.n2, (size_t)h->g.n3};
    GSS_FFT(rocfft_plan_create(&pl->fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                               rocfft_precision_double, (size_t)h->ndim, lengths, 1, nullptr));
    GSS_FFT(rocfft_plan_create(&pl->inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                               rocfft_precision_double, (size_t)h->ndim, lengths, 1, nullptr));
    size_t w1 = 0, w2 = 0;
    GSS_FFT(rocfft_plan_get_work_buffer_size(pl->fwd, &w1));
    GSS_FFT(rocfft_plan_get_work_buffer_size(pl->inv, &w2));
    pl->work_bytes = w1 > w2 ? w1 : w2;
    cache.emplace_front(key, pl);
    if (cache.size() > 8) cache.pop_back();   // handles that still use the pair keep it alive
    h->plans = std::move(pl);
  }
  h->fwd = h->plans->fwd;
  h->inv = h->plans->inv;
  const size_t wb = h->plans->work_bytes;
  GSS_FFT(rocfft_execution_info_create(&h->info));
  if (wb > 0) {
    GSS_TRY(h->work.alloc(wb));
    GSS_FFT(rocfft_execution_info_set_work_buffer(h->info, h->work.p, wb));
  }
  GSS_TRY(h->U.alloc(sizeof(double) * (size_t)h->N));
  GSS_TRY(h->Xn.alloc(sizeof(double) * 2 * (size_t)h->NH));
  return GSS_OK;
}

// Batched plans of the rocFFT pipeline: 64 realisations per execution when the call has that many and 64 noise arrays
// and half spectra fit 96 MiB, else 16, else none (0).  The plans live with the single ones (shared per grid size).
static int32_t ensure_rocfft_batch(gss_fftgs* h, int64_t nreals, int* batch_out) {
  *batch_out = 0;
  const int env_b = env_int("GSS_FFTGS_ROCFFT_BATCH", -1);   // 0: off; n: that batch size (read per call)
  const size_t per = sizeof(double) * ((size_t)h->N + 2 * (size_t)h->NH);
  int want = 0;
  for (int b : {64, 16})
    if (nreals >= b && per * (size_t)b <= ((size_t)96 << 20)) { want = b; break; }
  if (env_b == 0) want = 0;
  if (env_b > 0) want = nreals >= env_b ? env_b : 0;
  if (want == 0) return GSS_OK;
  FftPlans* pl = h->plans.get();
  if (pl->batch != want) {
    if (pl->fwdB) rocfft_plan_destroy(pl->fwdB);
    if (pl->invB) rocfft_plan_destroy(pl->invB);
    pl->fwdB = pl->invB = nullptr;
    pl->batch = 0;
    size_t lengths[3] = {(size_t)h->g.n1, (size_t)h->g.n2, (size_t)h->g.n3};
    GSS_FFT(rocfft_plan_create(&pl->fwdB, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                               rocfft_precision_double, (size_t)h->ndim, lengths, (size_t)want, nullptr));
    GSS_FFT(rocfft_plan_create(&pl->invB, rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                               rocfft_precision_double, (size_t)h->ndim, lengths, (size_t)want, nullptr));
    size_t w1 = 0, w2 = 0;
    GSS_FFT(rocfft_plan_get_work_buffer_size(pl->fwdB, &w1));
    GSS_FFT(rocfft_plan_get_work_buffer_size(pl->invB, &w2));
    pl->work_bytesB = w1 > w2 ? w1 : w2;
    pl->batch = want;
  }
  if (pl->work_bytesB > h->work.bytes) {
    GSS_TRY(h->work.alloc(pl->work_bytesB));
    GSS_FFT(rocfft_execution_info_set_work_buffer(h->info, h->work.p, pl->work_bytesB));
  }
  if (h->U.bytes < sizeof(double) * (size_t)h->N * (size_t)want) GSS_TRY(h->U.alloc(sizeof(double) * (size_t)h->N * (size_t)want));
  if (h->Xn.bytes < sizeof(double) * 2 * (size_t)h->NH * (size_t)want)
    GSS_TRY(h->Xn.alloc(sizeof(double) * 2 * (size_t)h->NH * (size_t)want));
  *batch_out = want;
  return GSS_OK;
}

// fft.jl:96-103: C -> R2C -> sqrt|.|
int32_t fftgs_spectrum_rocfft(gss_fftgs* h, double* partial, hipStream_t s) {
  GSS_TRY(ensure_rocfft(h));
  if (h->rotated)
    hipLaunchKernelGGL(fftgs_cov_rot_kernel, dim3(grid_blocks(h->N)), dim3(256), 0, s, h->vg, h->g, h->rot.as<double>(),
                       h->U.as<double>());
  else
    hipLaunchKernelGGL(fftgs_cov_kernel, dim3(grid_blocks(h->N)), dim3(256), 0, s, h->vg, h->g, h->U.as<double>());
  GSS_HIP(hipGetLastError());
  GSS_TRY(fft_exec(h, h->fwd, h->U.p, h->Xn.p, s));
  hipLaunchKernelGGL(fftgs_amp_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, h->g, h->Xn.as<double2>(), h->Fh(), partial);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

int32_t fftgs_begin_rocfft(gss_fftgs* h, int64_t total, int* batch) {
  *batch = 0;
  GSS_TRY(ensure_rocfft(h));
  return total > 0 ? ensure_rocfft_batch(h, total, batch) : GSS_OK;
}

// fft.jl:163-170 for nb consecutive realisations, N doubles apart: nb is 1 or the batch of fftgs_begin_rocfft
int32_t fftgs_fields_rocfft(gss_fftgs* h, uint64_t seed, int64_t real, int nb, const double* noise, double* z,
                            hipStream_t s) {
  const int64_t N = h->N;
  double* u = h->U.as<double>();
  if (noise) {
    u = const_cast<double*>(noise);  // the forward transform does not overwrite its input
  } else {
    ProfScope ps("fftgs_noise", s);
    GSS_TRY(philox_uniform_dev(seed, real, N, u, N, N, s, nb, N));
  }
  {
    ProfScope ps("fftgs_fwd", s);
    GSS_TRY(fft_exec(h, nb > 1 ? h->plans->fwdB : h->fwd, u, h->Xn.p, s));
  }
  {
    ProfScope ps("fftgs_phase", s);
    hipLaunchKernelGGL(fftgs_phase_kernel, dim3(grid_blocks(h->NH), (unsigned)nb), dim3(256), 0, s, h->Xn.as<double2>(),
                       h->Fh(), h->NH, h->mean);
    GSS_HIP(hipGetLastError());
  }
  {
    ProfScope ps("fftgs_inv", s);
    GSS_TRY(fft_exec(h, nb > 1 ? h->plans->invB : h->inv, h->Xn.p, z, s));
  }
  return GSS_OK;
}

}  // namespace gss
