// Normal-score transform (gss.h "normal-score transform"): the fit on the host, the knots and two
// guide tables in HBM, and one fused elementwise kernel that takes a value, finds its interval, interpolates or
// evaluates a tail, and stores.
//
// Interval search.  The abscissae X_0 < ... < X_{K-1} (v for the forward direction, y for the inverse) are quantile
// knots, so a uniform grid of G = 2 K cells over [X_0, X_{K-1}] holds a few knots per cell.  cell(x) = trunc((x - X_0) *
// G / (X_{K-1} - X_0)), capped at G - 1, is one subtraction, one product and one truncation: the host evaluates exactly
// these for every knot, the kernel for every value, and the function is monotone.  With cnt[c] the number of knots in
// cells below c, every knot counted by cnt[cell(x)] lies strictly below x and every knot not counted by
// cnt[cell(x) + 1] strictly above, so the interval of x -- the largest k <= K - 2 with X_k <= x, what a binary search
// over the whole table returns -- lies in [guide[c], guide[c + 1]], guide[c] = min(max(cnt[c] - 1, 0), K - 2).  The
// kernel bisects that range: no step for an empty cell, one or two where the table is quantile-spaced, and still
// log2 of the cell's population when skewed data crowd one cell of the forward table.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <vector>

#include "gss_internal.h"

using namespace gss;

struct gss_nscore {
  int64_t K = 0;
  int64_t G[2] = {1, 1};             // guide cells by direction (GSS_NSCORE_FORWARD: over v, _INVERSE: over y)
  double inv_h[2] = {0.0, 0.0};      // cells per unit of the abscissa (0: one cell)
  double v1 = 0.0, vK = 0.0, y1 = 0.0, yK = 0.0;
  double zmin = 0.0, zmax = 0.0, plo = 1.0, phi = 1.0;
  double qlo = 1.0, qhi = 1.0;       // erfc(-y_1 / sqrt 2), erfc(y_K / sqrt 2)
  int ncu = 256;
  DevBuf tab;                        // v[K] | y[K] | guide forward [G0 + 1] | guide inverse [G1 + 1] (int32)
  const double* v() const { return tab.as<double>(); }
  const double* y() const { return tab.as<double>() + K; }
  const int32_t* guide(int dir) const {
    const int32_t* g = reinterpret_cast<const int32_t*>(tab.as<double>() + 2 * K);
    return dir == GSS_NSCORE_FORWARD ? g : g + G[0] + 1;
  }
};

namespace {

constexpr int64_t NS_MAX_KNOTS = (int64_t)1 << 24;
// Knots, ordinates and the guide of one direction take 24 K + 4 bytes of LDS.  1 280 knots are 30 KiB: five blocks of
// 256 threads would share the 160 KiB of a CU, so the table never costs a kernel that waits on HBM and on a short
// dependent chain of LDS reads its occupancy; a larger table would buy its LDS residence with the waves that hide them.
// The inverse kernel, with erfc and pow inlined for its tails, takes 123 VGPRs: four waves per SIMD, i.e. four blocks
// per CU, which is what the launch asks for (a fifth block per CU would run alone after the others).
constexpr int64_t NS_LDS_KNOTS = 1280;
constexpr int64_t NS_LDS_KNOTS_CAP = 2048;   // 48 KiB: below the 64 KiB a launch may ask for without opting in
constexpr int NS_BLOCKS_PER_CU = 4;
constexpr int64_t NS_HOST_CHUNK = (int64_t)1 << 22;   // elements of a host array staged at a time (32 MiB)

// what the kernel needs besides the tables, by value
struct NsPar {
  int32_t K, G;
  double x0, xl;       // first and last abscissa
  double f0, fl;       // ordinates there
  double inv_h;
  // inverse only: tails
  double zmin, zmax, span_lo, span_hi, plo, phi, qlo, qhi;
};

// ---------------------------------------------------------------------------------------------------------------------
// host: Phi^-1 on (0, 1/2] -- Acklam's rational approximation (relative error 1.2e-9) and one Halley step on erfc in
// long double, which the two-sided formula of the fit only ever asks for a lower-tail probability
// ---------------------------------------------------------------------------------------------------------------------
double phi_inv_start(double p) {
  static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                              1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
  static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                              6.680131188771972e+01, -1.328068155288572e+01};
  static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                              -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
  static const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
                              3.754408661907416e+00};
  if (p < 0.02425) {
    const double q = std::sqrt(-2.0 * std::log(p));
    return (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
           ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
  }
  const double q = p - 0.5, r = q * q;
  return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
         (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
}

double phi_inv_lower(long double p) {
  long double x = (long double)phi_inv_start((double)p);
  const long double e = 0.5L * erfcl(-x * 0.70710678118654752440084436210484904L) - p;
  const long double u = e * 2.50662827463100050241576528481104525L * expl(0.5L * x * x);
  x = x - u / (1.0L + 0.5L * x * u);
  return (double)x;
}

// guide of one direction over the abscissae X (see the head of the file); the kernel's cell() below is this cell()
inline int64_t ns_cell(double x, double x0, double inv_h, int64_t G) {
  const double c = (x - x0) * inv_h;
  return c >= (double)G ? G - 1 : (int64_t)c;
}

void build_guide(const std::vector<double>& X, int64_t* G_out, double* inv_h_out, std::vector<int32_t>* guide) {
  const int64_t K = (int64_t)X.size();
  int64_t G = 1;
  double inv_h = 0.0;
  if (K >= 2) {
    G = std::min<int64_t>(2 * K, NS_MAX_KNOTS);
    inv_h = (double)G / (X[K - 1] - X[0]);
    if (!std::isfinite(inv_h) || !std::isfinite(X[K - 1] - X[0])) {   // a span that over- or underflows: one cell
      G = 1;
      inv_h = 0.0;
    }
  }
  std::vector<int64_t> cnt((size_t)G + 2, 0);   // cnt[c + 1]: knots in cell c, then the prefix sums
  for (int64_t k = 0; k < K; ++k) ++cnt[(size_t)ns_cell(X[k], X[0], inv_h, G) + 1];
  for (int64_t c = 0; c < G; ++c) cnt[(size_t)c + 1] += cnt[(size_t)c];
  guide->resize((size_t)G + 1);
  const int64_t top = K >= 2 ? K - 2 : 0;
  for (int64_t c = 0; c <= G; ++c) (*guide)[(size_t)c] = (int32_t)std::min(std::max<int64_t>(cnt[(size_t)c] - 1, 0), top);
  *G_out = G;
  *inv_h_out = inv_h;
}

// ---------------------------------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------------------------------
template <bool INV>
__device__ __forceinline__ double nscore_one(double x, const NsPar& P, const double* X, const double* F,
                                             const int32_t* gd) {
  if (x != x) return x;
  if (x <= P.x0) {
    if (!INV || x == P.x0) return P.f0;
    if (P.span_lo == 0.0) return P.zmin;
    double t = fmin(erfc(-x * 0.7071067811865476) / P.qlo, 1.0);
    if (P.plo != 1.0) t = pow(t, P.plo);
    return fmin(fma(P.span_lo, t, P.zmin), P.f0);
  }
  if (x >= P.xl) {
    if (!INV || x == P.xl) return P.fl;
    if (P.span_hi == 0.0) return P.zmax;
    double t = fmin(erfc(x * 0.7071067811865476) / P.qhi, 1.0);
    if (P.phi != 1.0) t = pow(t, P.phi);
    return fmax(fma(-P.span_hi, t, P.zmax), P.fl);
  }
  // X_0 < x < X_{K-1}, so K >= 2
  const double c = (x - P.x0) * P.inv_h;
  const int cell = c >= (double)P.G ? P.G - 1 : (int)c;
  int lo = gd[cell], hi = gd[cell + 1];
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (X[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  const double xa = X[lo], xb = X[lo + 1], fa = F[lo], fb = F[lo + 1];
  const double r = (x - xa) / (xb - xa);
  return fmin(fmax(fma(fb - fa, r, fa), fa), fb);
}

// One pass over nblocks runs of len doubles.  A run whose source and destination sit alike within 16 bytes is read and
// written two doubles at a time: an odd first element and an odd last one are done alone by thread 0 of the grid row.
template <bool INV, bool LDS>
__global__ __launch_bounds__(256) void nscore_apply_kernel(NsPar P, const double* __restrict__ Xg,
                                                           const double* __restrict__ Fg,
                                                           const int32_t* __restrict__ gg, const double* in, double* out,
                                                           int64_t nblocks, int64_t len, int64_t in_stride,
                                                           int64_t out_stride) {
  extern __shared__ double nscore_lds[];
  const double* X = Xg;
  const double* F = Fg;
  const int32_t* gd = gg;
  if (LDS) {
    double* Xs = nscore_lds;
    double* Fs = nscore_lds + P.K;
    int32_t* gs = reinterpret_cast<int32_t*>(nscore_lds + 2 * (int64_t)P.K);
    for (int i = threadIdx.x; i < P.K; i += 256) {
      Xs[i] = Xg[i];
      Fs[i] = Fg[i];
    }
    for (int i = threadIdx.x; i <= P.G; i += 256) gs[i] = gg[i];
    __syncthreads();
    X = Xs;
    F = Fs;
    gd = gs;
  }
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  for (int64_t b = blockIdx.y; b < nblocks; b += gridDim.y) {
    const double* src = in + b * in_stride;
    double* dst = out + b * out_stride;
    if ((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 8) {
      for (int64_t i = tid; i < len; i += nth) dst[i] = nscore_one<INV>(src[i], P, X, F, gd);
      continue;
    }
    const int64_t head = (reinterpret_cast<uintptr_t>(src) >> 3) & 1;   // (len >= 1)
    const int64_t npair = (len - head) >> 1;
    const int64_t last = head + 2 * npair;
    if (tid == 0) {
      if (head) dst[0] = nscore_one<INV>(src[0], P, X, F, gd);
      if (last < len) dst[last] = nscore_one<INV>(src[last], P, X, F, gd);
    }
    const double2* s2 = reinterpret_cast<const double2*>(src + head);
    double2* d2 = reinterpret_cast<double2*>(dst + head);
    for (int64_t p = tid; p < npair; p += 2 * nth) {   // two loads in flight per thread
      const bool more = p + nth < npair;
      double2 a = s2[p];
      double2 c = more ? s2[p + nth] : a;
      a.x = nscore_one<INV>(a.x, P, X, F, gd);
      a.y = nscore_one<INV>(a.y, P, X, F, gd);
      d2[p] = a;
      if (more) {
        c.x = nscore_one<INV>(c.x, P, X, F, gd);
        c.y = nscore_one<INV>(c.y, P, X, F, gd);
        d2[p + nth] = c;
      }
    }
  }
}

int64_t lds_knots() {
  int64_t t = NS_LDS_KNOTS;
  if (const char* e = std::getenv("GSS_NSCORE_LDS_KNOTS")) {   // tests: both variants at small K
    const long long v = std::atoll(e);
    if (v >= 0) t = std::min<int64_t>(v, NS_LDS_KNOTS_CAP);
  }
  return t;
}

// device pointers; the caller has checked the arguments
int32_t nscore_launch(const gss_nscore* h, int dir, const double* in, double* out, int64_t nblocks, int64_t len,
                      int64_t is, int64_t os, hipStream_t s) {
  const bool inv = dir == GSS_NSCORE_INVERSE;
  NsPar P;
  P.K = (int32_t)h->K;
  P.G = (int32_t)h->G[dir];
  P.inv_h = h->inv_h[dir];
  P.x0 = inv ? h->y1 : h->v1;
  P.xl = inv ? h->yK : h->vK;
  P.f0 = inv ? h->v1 : h->y1;
  P.fl = inv ? h->vK : h->yK;
  P.zmin = h->zmin;
  P.zmax = h->zmax;
  P.span_lo = h->v1 - h->zmin;
  P.span_hi = h->zmax - h->vK;
  P.plo = h->plo;
  P.phi = h->phi;
  P.qlo = h->qlo;
  P.qhi = h->qhi;
  const double* X = inv ? h->y() : h->v();
  const double* F = inv ? h->v() : h->y();
  const int32_t* gd = h->guide(dir);
  const bool lds = h->K <= lds_knots();
  const size_t shmem = lds ? sizeof(double) * 2 * (size_t)h->K + sizeof(int32_t) * (size_t)(h->G[dir] + 2) : 0;
  const int64_t gy = std::min<int64_t>(nblocks, 65535);
  const int64_t want = ((len + 1) / 2 + 511) / 512;   // two pairs per thread and trip
  const int64_t room = std::max<int64_t>(1, (int64_t)h->ncu * NS_BLOCKS_PER_CU / gy);
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min(want, room)), (unsigned)gy);
#define GSS_NS_LAUNCH(INV, LDS)                                                                                   \
  hipLaunchKernelGGL((nscore_apply_kernel<INV, LDS>), grid, dim3(256), shmem, s, P, X, F, gd, in, out, nblocks, len, \
                     is, os)
  ProfScope ps("nscore_apply", s);
  if (inv) {
    if (lds) GSS_NS_LAUNCH(true, true);
    else GSS_NS_LAUNCH(true, false);
  } else {
    if (lds) GSS_NS_LAUNCH(false, true);
    else GSS_NS_LAUNCH(false, false);
  }
#undef GSS_NS_LAUNCH
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

}  // namespace

extern "C" {

int32_t gss_nscore_create(gss_nscore_t** out, const double* z, const double* w, int64_t n, double zmin, double zmax,
                          double power_lo, double power_hi, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(out != nullptr, "gss_nscore_create: out is NULL");
  *out = nullptr;
  GSS_REQUIRE(n >= 1, "gss_nscore_create: n = %lld: at least one value is needed", (long long)n);
  GSS_REQUIRE(z != nullptr, "gss_nscore_create: z is NULL");
  GSS_REQUIRE(power_lo > 0.0 && std::isfinite(power_lo) && power_hi > 0.0 && std::isfinite(power_hi),
              "gss_nscore_create: tail powers (%g, %g) must be finite and > 0", power_lo, power_hi);
  for (int64_t i = 0; i < n; ++i) {
    GSS_REQUIRE(std::isfinite(z[i]), "gss_nscore_create: value %lld is not finite", (long long)i);
    GSS_REQUIRE(w == nullptr || (std::isfinite(w[i]) && w[i] > 0.0),
                "gss_nscore_create: weight %lld is not finite and positive", (long long)i);
  }
  std::vector<int64_t> order((size_t)n);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(), [z](int64_t a, int64_t b) { return z[a] < z[b]; });
  std::vector<double> v;
  std::vector<long double> W;
  for (int64_t i = 0; i < n; ++i) {
    const double zi = z[order[(size_t)i]];
    const long double wi = w ? (long double)w[order[(size_t)i]] : 1.0L;
    if (!v.empty() && zi == v.back()) W.back() += wi;
    else {
      v.push_back(zi);
      W.push_back(wi);
    }
  }
  const int64_t K = (int64_t)v.size();
  GSS_REQUIRE(K <= NS_MAX_KNOTS, "gss_nscore_create: %lld distinct values, at most %lld", (long long)K,
              (long long)NS_MAX_KNOTS);
  const double lo = std::isnan(zmin) ? v.front() : zmin, hi = std::isnan(zmax) ? v.back() : zmax;
  GSS_REQUIRE(std::isfinite(lo) && lo <= v.front(), "gss_nscore_create: zmin = %g lies above the smallest value %g", lo,
              v.front());
  GSS_REQUIRE(std::isfinite(hi) && hi >= v.back(), "gss_nscore_create: zmax = %g lies below the largest value %g", hi,
              v.back());
  // weight strictly below (from the bottom) and strictly above (from the top) every class, each summed on its own
  std::vector<long double> below((size_t)K), above((size_t)K);
  long double acc = 0.0L;
  for (int64_t k = 0; k < K; ++k) {
    below[(size_t)k] = acc;
    acc += W[(size_t)k];
  }
  const long double T = acc;
  acc = 0.0L;
  for (int64_t k = K - 1; k >= 0; --k) {
    above[(size_t)k] = acc;
    acc += W[(size_t)k];
  }
  std::vector<double> y((size_t)K);
  for (int64_t k = 0; k < K; ++k) {
    const bool lower = below[(size_t)k] <= above[(size_t)k];
    // The smaller side plus half the class is at most T / 2 in exact arithmetic only: the sums from the bottom (below, T)
    // and from the top (above) round on their own once a prefix outgrows 64 bits, and the median class of equal weights
    // that are not exact in binary (0.1, 1 / n) then comes out one unit in the last place above 1/2.
    const long double p = std::min(((lower ? below[(size_t)k] : above[(size_t)k]) + 0.5L * W[(size_t)k]) / T, 0.5L);
    GSS_REQUIRE(p > 0.0L, "gss_nscore_create: the weights are too uneven: knot %lld has no probability", (long long)k);
    const double q = phi_inv_lower(p);
    y[(size_t)k] = lower ? q : -q;
    GSS_REQUIRE(k == 0 || y[(size_t)k] > y[(size_t)k - 1], "gss_nscore_create: the weights are too uneven for FP64: the "
                "score of knot %lld does not exceed that of knot %lld", (long long)k, (long long)k - 1);
  }
  std::vector<int32_t> gf, gi;
  std::unique_ptr<gss_nscore> h(new gss_nscore);
  h->K = K;
  build_guide(v, &h->G[0], &h->inv_h[0], &gf);
  build_guide(y, &h->G[1], &h->inv_h[1], &gi);
  h->v1 = v.front();
  h->vK = v.back();
  h->y1 = y.front();
  h->yK = y.back();
  h->zmin = lo;
  h->zmax = hi;
  h->plo = power_lo;
  h->phi = power_hi;
  h->qlo = std::erfc(-h->y1 * 0.7071067811865476);
  h->qhi = std::erfc(h->yK * 0.7071067811865476);

  // ---- device ----
  hipStream_t s = to_stream(stream);
  const size_t kb = sizeof(double) * (size_t)K, gfb = sizeof(int32_t) * gf.size(), gib = sizeof(int32_t) * gi.size();
  int32_t st = h->tab.alloc(2 * kb + gfb + gib);
  if (st == GSS_OK) {
    char* base = h->tab.as<char>();
    hipError_t e = hipMemcpyAsync(base, v.data(), kb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base + kb, y.data(), kb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base + 2 * kb, gf.data(), gfb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base + 2 * kb + gfb, gi.data(), gib, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the host images go out of scope
    int dev = 0, ncu = 0;
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) {
      set_error("gss_nscore_create: %s", hipGetErrorString(e));
      st = GSS_ERR_HIP;
    } else if (ncu > 0) {
      h->ncu = ncu;
    }
  }
  if (st != GSS_OK) return st;
  *out = h.release();
  return GSS_OK;
}

int32_t gss_nscore_destroy(gss_nscore_t* h) {
  GSS_ENTRY();
  delete h;
  return GSS_OK;
}

int32_t gss_nscore_info(const gss_nscore_t* h, int64_t* nknots) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && nknots != nullptr, "gss_nscore_info: bad arguments");
  *nknots = h->K;
  return GSS_OK;
}

int32_t gss_nscore_table(gss_nscore_t* h, double* v, double* y, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && v != nullptr && y != nullptr, "gss_nscore_table: bad arguments");
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_nscore_table: mem = %d", mem);
  hipStream_t s = to_stream(stream);
  const size_t kb = sizeof(double) * (size_t)h->K;
  const hipMemcpyKind kind = mem == GSS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  GSS_HIP(hipMemcpyAsync(v, h->v(), kb, kind, s));
  GSS_HIP(hipMemcpyAsync(y, h->y(), kb, kind, s));
  if (mem == GSS_MEM_HOST) GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

int32_t gss_nscore_apply(gss_nscore_t* h, int32_t direction, const double* in, double* out, int64_t nblocks,
                         int64_t len, int64_t in_stride, int64_t out_stride, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "gss_nscore_apply: handle is NULL");
  GSS_REQUIRE(direction == GSS_NSCORE_FORWARD || direction == GSS_NSCORE_INVERSE, "gss_nscore_apply: direction = %d",
              direction);
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_nscore_apply: mem = %d", mem);
  GSS_REQUIRE(nblocks >= 0 && len >= 0, "gss_nscore_apply: nblocks = %lld, len = %lld", (long long)nblocks,
              (long long)len);
  if (nblocks == 0 || len == 0) return GSS_OK;
  GSS_REQUIRE(in != nullptr && out != nullptr, "gss_nscore_apply: in or out is NULL");
  GSS_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 7) == 0,
              "gss_nscore_apply: in and out must be aligned to 8 bytes");
  if (nblocks == 1) in_stride = out_stride = len;   // (not read)
  GSS_REQUIRE(in_stride >= len && out_stride >= len, "gss_nscore_apply: strides (%lld, %lld) are shorter than the "
              "blocks of %lld elements", (long long)in_stride, (long long)out_stride, (long long)len);
  GSS_REQUIRE(in_stride <= INT64_MAX / 8 / nblocks && out_stride <= INT64_MAX / 8 / nblocks,
              "gss_nscore_apply: nblocks x stride overflows");
  const double* in_end = in + (nblocks - 1) * in_stride + len;
  const double* out_end = out + (nblocks - 1) * out_stride + len;
  const bool identity = out == in && in_stride == out_stride;
  GSS_REQUIRE(identity || out_end <= in || in_end <= out, "gss_nscore_apply: in and out overlap without being the same "
              "blocks");
  hipStream_t s = to_stream(stream);
  if (mem == GSS_MEM_DEVICE) return nscore_launch(h, direction, in, out, nblocks, len, in_stride, out_stride, s);

  int64_t chunk = NS_HOST_CHUNK;
  if (const char* e = std::getenv("GSS_NSCORE_CHUNK_ELEMS")) {   // tests: a chunk loop that runs more than once
    const long long v = std::atoll(e);
    if (v > 0 && v < chunk) chunk = v;
  }
  chunk = std::min(chunk, len);
  // Each chunk goes through Staged like the host arrays of every other entry point: an image of the input, an image of
  // the output, the launch between them, and back() waits for the results (the blocks return to the pool, so the
  // second chunk allocates nothing).  Nothing overlaps: see DESIGN.md section 7.
  for (int64_t b = 0; b < nblocks; ++b)
    for (int64_t off = 0; off < len; off += chunk) {
      const int64_t m = std::min(chunk, len - off);
      Staged si, so;
      GSS_TRY(si.in(in + b * in_stride + off, sizeof(double) * (size_t)m, mem, s));
      GSS_TRY(so.out(out + b * out_stride + off, sizeof(double) * (size_t)m, mem));
      GSS_TRY(nscore_launch(h, direction, si.as<double>(), so.as<double>(), 1, m, m, m, s));
      GSS_TRY(so.back(s));
    }
  return GSS_OK;
}

}  // extern "C"
