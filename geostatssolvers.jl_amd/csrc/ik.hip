// Indicator kriging (gss.h, gss_ik_predict_knn / gss_ik_order_relations / gss_ik_post): the ccdf of a
// continuous variable at K cutoffs from a moving neighbourhood, GSLIB's order-relation correction, and the
// post-processing of a corrected ccdf (mean, variance, exceedance probabilities, quantiles).  This unit holds the
// drivers, the general instantiations of ik_local_kernel (any model, 1-D, the full form) and the two row kernels; the
// compile-time kinds of the median form in 2-D and 3-D have units of their own (ik_2d.hip, ik_3d.hip).
#include "ik_kernel.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace gss {

// ---- order relations on m x K rows: sixteen lanes per point, lane q = cutoff q (ik_order16) ----------------------
__global__ __launch_bounds__(256) void ik_order_kernel(double* __restrict__ ccdf, int64_t m, int K,
                                                       unsigned long long* __restrict__ acc) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = t >> 4;
  const int q = (int)(t & 15);
  const bool in = p < m && q < K;
  const double f = in ? ccdf[p * K + q] : 0.0;
  const double r = ik_order16(f, q, K);   // (every lane: shuffles)
  unsigned long long changed = 0;
  double dmax = 0.0;
  if (in) {
    ccdf[p * K + q] = r;
    if (f == f && r == r && r != f) {   // (a row that holds a NaN becomes all NaN and is not counted)
      changed = 1;
      dmax = fabs(r - f);
    }
  }
  // per wave: count and largest change (non-negative doubles order like their bit patterns)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    changed += __shfl_xor(changed, off);
    dmax = fmax(dmax, __shfl_xor(dmax, off));
  }
  if (acc && (threadIdx.x & 63) == 0 && changed) {
    atomicAdd(&acc[0], changed);
    atomicMax(&acc[1], (unsigned long long)__double_as_longlong(dmax));
  }
}

// ---- post-processing: one thread per point --------------------------------------------------------------------------
struct IkPostSpec {
  int K, nthr, nq;
  double zmin, zmax, wlo, whi;
  double cut[IK_MAXK], thr[16], prob[16];
};

__device__ __forceinline__ double ik_pow(double x, double w) { return w == 1.0 ? x : pow(x, w); }

// V2: rows of an even number of doubles read as 16-byte pairs.  A row starts 8 K p bytes after the base; with K even
// that is a multiple of 16, so every pair is aligned whenever the base is (the launcher checks the base address and
// takes the 8-byte form otherwise).
template <bool V2>
__global__ __launch_bounds__(256) void ik_post_kernel(IkPostSpec sp, const double* __restrict__ ccdf, int64_t m,
                                                      double* __restrict__ etype, double* __restrict__ cvar,
                                                      double* __restrict__ pabove, double* __restrict__ quant) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= m) return;
  const int K = sp.K;
  double F[IK_MAXK];
  bool nan = false;
  if (V2) {
    const double2* row = reinterpret_cast<const double2*>(ccdf + p * K);
#pragma unroll
    for (int q = 0; q < IK_MAXK / 2; ++q) {
      if (2 * q < K) {
        const double2 v = row[q];
        F[2 * q] = v.x;
        F[2 * q + 1] = v.y;
      } else {
        F[2 * q] = 1.0;
        F[2 * q + 1] = 1.0;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < IK_MAXK; ++q) F[q] = q < K ? ccdf[p * K + q] : 1.0;
  }
#pragma unroll
  for (int q = 0; q < IK_MAXK; ++q) nan = nan || (F[q] != F[q]);
  const double NaN = __longlong_as_double(0x7ff8000000000000LL);
  const double dlo = sp.cut[0] - sp.zmin, dhi = sp.zmax - sp.cut[K - 1];
  double Ftop = F[0];   // F_{K-1}
#pragma unroll
  for (int q = 1; q < IK_MAXK; ++q)
    if (q < K) Ftop = F[q];
  if (etype || cvar) {
    // class means and second moments about zero (closed forms)
    const double slo = dlo * (sp.wlo / (sp.wlo + 1.0)), s2lo = dlo * dlo * (sp.wlo / (sp.wlo + 2.0));
    const double shi = dhi * (sp.whi / (sp.whi + 1.0)), s2hi = dhi * dhi * (sp.whi / (sp.whi + 2.0));
    double m1 = F[0] * (sp.zmin + slo);
    double m2 = F[0] * (sp.zmin * sp.zmin + 2.0 * sp.zmin * slo + s2lo);
#pragma unroll
    for (int q = 1; q < IK_MAXK; ++q) {
      if (q < K) {
        const double pq = F[q] - F[q - 1], a = sp.cut[q - 1], b = sp.cut[q];
        m1 += pq * (0.5 * (a + b));
        m2 += pq * ((a * a + a * b + b * b) * (1.0 / 3.0));
      }
    }
    const double pt = 1.0 - Ftop;
    m1 += pt * (sp.zmax - shi);
    m2 += pt * (sp.zmax * sp.zmax - 2.0 * sp.zmax * shi + s2hi);
    const double v = m2 - m1 * m1;
    if (etype) etype[p] = nan ? NaN : m1;
    if (cvar) cvar[p] = nan ? NaN : (v > 0.0 ? v : 0.0);
  }
  if (pabove) {
    for (int i = 0; i < sp.nthr; ++i) {
      const double t = sp.thr[i];
      double Ft;
      if (t <= sp.cut[0]) {
        Ft = F[0] * ik_pow((t - sp.zmin) / dlo, sp.wlo);
      } else if (t > sp.cut[K - 1]) {
        Ft = 1.0 - (1.0 - Ftop) * ik_pow((sp.zmax - t) / dhi, sp.whi);
      } else {
        Ft = Ftop;
#pragma unroll
        for (int q = IK_MAXK - 1; q >= 1; --q)
          if (q < K && t <= sp.cut[q])
            Ft = F[q - 1] + (F[q] - F[q - 1]) * ((t - sp.cut[q - 1]) / (sp.cut[q] - sp.cut[q - 1]));
      }
      pabove[p * sp.nthr + i] = nan ? NaN : 1.0 - Ft;
    }
  }
  if (quant) {
    for (int i = 0; i < sp.nq; ++i) {
      const double pr = sp.prob[i];
      double z;
      if (pr <= F[0]) {
        z = sp.zmin + dlo * ik_pow(pr / F[0], 1.0 / sp.wlo);
      } else if (pr > Ftop) {
        z = sp.zmax - dhi * ik_pow((1.0 - pr) / (1.0 - Ftop), 1.0 / sp.whi);
      } else {
        z = sp.cut[K - 1];
#pragma unroll
        for (int q = IK_MAXK - 1; q >= 1; --q)   // the first class whose upper value reaches pr wins (descending loop)
          if (q < K && pr <= F[q])
            z = sp.cut[q - 1] + (sp.cut[q] - sp.cut[q - 1]) * ((pr - F[q - 1]) / (F[q] - F[q - 1]));
      }
      quant[p * sp.nq + i] = nan ? NaN : z;
    }
  }
}

static int32_t ik_check_cutoffs(const char* who, const double* cutoffs, int32_t K) {
  GSS_REQUIRE(K >= 1 && K <= IK_MAXK, "%s: %d cutoffs outside 1 .. %d", who, K, IK_MAXK);
  GSS_REQUIRE(cutoffs != nullptr, "%s: cutoffs is NULL", who);
  for (int q = 0; q < K; ++q) {
    GSS_REQUIRE(std::isfinite(cutoffs[q]), "%s: cutoff %d is not finite", who, q);
    GSS_REQUIRE(q == 0 || cutoffs[q] > cutoffs[q - 1], "%s: cutoffs must increase strictly (cutoff %d)", who, q);
  }
  return GSS_OK;
}

static int32_t ik_order_dev(double* ccdf, int64_t m, int K, unsigned long long* acc, hipStream_t s) {
  const int64_t nt = m * 16;
  hipLaunchKernelGGL(ik_order_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, ccdf, m, K, acc);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

static bool frame_free(const gss_variogram_t& v) {   // every structure a sphere: the same on any frame
  auto sphere = [&](int aniso, const double* ir) {
    if (aniso == 0) return true;
    for (int k = 1; k < v.dim; ++k)
      if (ir[k] != ir[0]) return false;
    return true;
  };
  bool ok = sphere(v.aniso, v.inv_radii);
  for (int e = 0; e < v.nextra; ++e) ok = ok && sphere(v.extra[e].aniso, v.extra[e].inv_radii);
  return ok;
}

// GSS_IK_CHUNK_POINTS caps the points per chunk of gss_ik_predict_knn (tests: a chunk loop that runs more than once at a
// small size).  Any positive count: a chunk is a launch of its own, so it need not be a multiple of IK_WAVES.
static int64_t ik_chunk_cap(int64_t chunk) {
  if (const char* e = std::getenv("GSS_IK_CHUNK_POINTS")) {
    const int64_t cap = std::atoll(e);
    if (cap > 0 && cap < chunk) chunk = cap;
  }
  return chunk;
}

// the kernel of one chunk by dimension, model and form
static int32_t ik_dispatch(int dim, int kind, bool full, const IkLaunch& a) {
  if (full) {
    if (dim == 3) return ik_local_launch<3, -1, true>(a);
    if (dim == 2) return ik_local_launch<2, -1, true>(a);
    return ik_local_launch<1, -1, true>(a);
  }
  const bool fixed = kind == GSS_VG_GAUSSIAN || kind == GSS_VG_EXPONENTIAL || kind == GSS_VG_SPHERICAL ||
                     kind == VG_MATERN12 || kind == VG_MATERN32 || kind == VG_MATERN52;
  if (dim == 3) return fixed ? ik_local_launch_3d(kind, a) : ik_local_launch<3, -1, false>(a);
  if (dim == 2) return fixed ? ik_local_launch_2d(kind, a) : ik_local_launch<2, -1, false>(a);
  return ik_local_launch<1, -1, false>(a);
}

}  // namespace gss

using namespace gss;

extern "C" {

int32_t gss_ik_predict_knn(const double* xdata, const double* z, int64_t n, int32_t dim, const double* cutoffs,
                           int32_t K, const gss_variogram_t* vgs, int32_t nvg, int32_t variant, const double* fstar,
                           int32_t k, int32_t minneighbors, double radius, const double* inv_radii, int32_t metric,
                           double metric_param, const double* xdom, int64_t m, double* ccdf, double* raw,
                           uint8_t* status, int32_t* idx_out, int32_t* count_out, int32_t mem, void* stream) {
  GSS_ENTRY();
  const char* who = "gss_ik_predict_knn";
  GSS_TRY(ik_check_cutoffs(who, cutoffs, K));
  GSS_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside 1..3", who, dim);
  GSS_REQUIRE(n >= 1 && n < (1 << 30), "%s: %lld samples", who, (long long)n);
  GSS_REQUIRE(variant == GSS_KRIG_ORDINARY || variant == GSS_KRIG_SIMPLE,
              "%s: variant %d: ordinary or simple (indicator kriging takes no drift)", who, variant);
  GSS_REQUIRE(vgs != nullptr && (nvg == 1 || nvg == K), "%s: %d variograms: one (median form) or one per cutoff (%d)",
              who, nvg, K);
  const bool ordinary = variant == GSS_KRIG_ORDINARY;
  if (!ordinary) {
    GSS_REQUIRE(fstar != nullptr, "%s: the simple variant needs the global proportions F*", who);
    for (int q = 0; q < K; ++q)
      GSS_REQUIRE(fstar[q] >= 0.0 && fstar[q] <= 1.0, "%s: F*[%d] = %g outside [0, 1]", who, q, fstar[q]);
  }
  if (k > LMAX_K) {
    set_error("%s: maxneighbors %d beyond %d, the limit of the moving-neighbourhood tile kernel", who, k, LMAX_K);
    return GSS_ERR_UNSUPPORTED;
  }
  GSS_REQUIRE(k >= 1 && k <= n, "%s: maxneighbors %d outside 1..%lld (a front-end clamps it)", who, k, (long long)n);
  GSS_REQUIRE(minneighbors <= k, "%s: invalid min/max number of neighbors", who);
  GSS_REQUIRE(m >= 0 && (m == 0 || (xdom && ccdf)), "%s: NULL array", who);
  GSS_REQUIRE(xdata && z, "%s: NULL data", who);

  // the models: stationary, of the call's dimension, and on ONE frame -- the rotation of the rotated ones, which the
  // others must not depend on
  const bool full = nvg == K && K > 1;
  std::vector<VgDev> vd((size_t)nvg);
  Frame fr;
  fr.dim = dim;
  for (int q = 0; q < nvg; ++q) {
    GSS_REQUIRE(vgs[q].dim == dim, "%s: variogram %d has dim %d, the samples %d", who, q, vgs[q].dim, dim);
    if (!vg_is_stationary(&vgs[q])) {
      set_error("%s: variogram %d is a power model: indicator kriging needs a sill", who, q);
      return GSS_ERR_UNSUPPORTED;
    }
    gss_variogram_t plain;
    Frame f;
    GSS_TRY(vg_frame_split(&vgs[q], &plain, &f));
    GSS_TRY(make_vgdev(&plain, &vd[q]));
    if (f.on) {
      if (fr.on && std::memcmp(fr.R, f.R, sizeof(fr.R)) != 0) {
        set_error("%s: the rotated variograms of a call must share one rotation (variogram %d differs)", who, q);
        return GSS_ERR_UNSUPPORTED;
      }
      fr = f;
    }
  }
  if (fr.on) {
    for (int q = 0; q < nvg; ++q) {
      Frame f;
      gss_variogram_t plain;
      GSS_TRY(vg_frame_split(&vgs[q], &plain, &f));
      if (!f.on && !frame_free(vgs[q])) {
        set_error("%s: variogram %d is axis-aligned anisotropic and cannot share the frame of a rotated one", who, q);
        return GSS_ERR_UNSUPPORTED;
      }
    }
  }
  if (m == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  GSS_TRY(frame_origin(&fr, xdata, mem, s));   // (also the origin of a rotated search ball, as in gss_krig_create)
  Searcher sr;
  GSS_TRY(sr.init(metric, metric_param, radius, inv_radii, dim, &fr));

  Staged sxd, sz, stab, svg;
  GSS_TRY(sxd.in(xdata, sizeof(double) * (size_t)(n * dim), mem, s));
  const double* xraw = sxd.as<double>();
  FrameCopy xfr;   // a rotated model: the samples in its frame
  GSS_TRY(xfr.of(fr, &sxd, n, s));
  GSS_TRY(sr.samples(sxd.as<double>(), fr.on ? xraw : nullptr, n, s, mem == GSS_MEM_HOST ? xdata : nullptr));
  GSS_TRY(sz.in(z, sizeof(double) * (size_t)n, mem, s));
  double tab[IK_TAB];
  for (int q = 0; q < IK_MAXK; ++q) {
    tab[q] = q < K ? cutoffs[q] : 0.0;
    tab[IK_MAXK + q] = (q < K && !ordinary) ? fstar[q] : 0.0;
  }
  GSS_TRY(stab.in(tab, sizeof(tab), GSS_MEM_HOST, s));
  if (full) GSS_TRY(svg.in(vd.data(), sizeof(VgDev) * (size_t)K, GSS_MEM_HOST, s));

  DomainCall dc;   // whole: the outputs are rows of K, nothing is piped
  dc.in(xdom, sizeof(double) * dim);
  Staged& sccdf = *dc.out(ccdf, sizeof(double) * (size_t)K);
  Staged& sraw = *dc.out(raw, sizeof(double) * (size_t)K);
  Staged& sstat = *dc.out(status, 1);
  Staged& sidx = *dc.out(idx_out, sizeof(int32_t) * (size_t)k);
  Staged& scnt = *dc.out(count_out, sizeof(int32_t));
  GSS_TRY(dc.begin(mem, m, s, false, &fr));

  const int64_t chunk = ik_chunk_cap(1 << 20);
  const int64_t mc = m < chunk ? m : chunk;
  DevBuf idx_s, cnt_s, st_s;
  if (!idx_out) GSS_TRY(idx_s.alloc(sizeof(int) * (size_t)(mc * k)));
  if (!count_out) GSS_TRY(cnt_s.alloc(sizeof(int) * (size_t)mc));
  if (!status) GSS_TRY(st_s.alloc((size_t)mc));
  const int kind = vd[0].nextra == 0 ? vd[0].kind : -1;
  for (int64_t off = 0; off < m; off += chunk) {
    const int64_t mv = (m - off) < chunk ? (m - off) : chunk;
    int* idx = idx_out ? sidx.as<int>() + off * k : idx_s.as<int>();
    int* cnt = count_out ? scnt.as<int>() + off : cnt_s.as<int>();
    {
      ProfScope ps("knn", s);
      GSS_TRY(sr.query(dc.x() + off * dim, sr.two_frames ? dc.x_raw + off * dim : nullptr, mv, k, idx, cnt, s));
    }
    ProfScope pl("ik_local", s);
    IkLaunch a;
    a.vg = &vd[0];
    a.vgtab = full ? svg.as<VgDev>() : nullptr;
    a.sp = IkSpec{K, ordinary ? 1 : 0, minneighbors, k};
    a.ctab = stab.as<double>();
    a.xg = sxd.as<double>();
    a.zg = sz.as<double>();
    a.x0 = dc.x() + off * dim;
    a.m = mv;
    a.idx = idx;
    a.cnt = cnt;
    a.ccdf = sccdf.as<double>() + off * K;
    a.raw = raw ? sraw.as<double>() + off * K : nullptr;
    a.status = status ? sstat.as<uint8_t>() + off : st_s.as<uint8_t>();
    a.s = s;
    GSS_TRY(ik_dispatch(dim, kind, full, a));
  }
  GSS_TRY(dc.finish(s));
  GSS_HIP(hipStreamSynchronize(s));   // the staged samples, tables and lists are released on return
  return GSS_OK;
}

int32_t gss_ik_order_relations(double* ccdf, int64_t m, int32_t K, int64_t* ncorrected, double* maxcorr, int32_t mem,
                               void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(K >= 1 && K <= IK_MAXK, "gss_ik_order_relations: %d cutoffs outside 1 .. %d", K, IK_MAXK);
  GSS_REQUIRE(m >= 0 && (m == 0 || ccdf), "gss_ik_order_relations: NULL array");
  if (ncorrected) *ncorrected = 0;
  if (maxcorr) *maxcorr = 0.0;
  if (m == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  const size_t bytes = sizeof(double) * (size_t)(m * K);
  DevBuf img;   // host rows: a device image of the call, copied back where it came from
  double* rows = ccdf;
  if (mem == GSS_MEM_HOST) {
    GSS_TRY(img.alloc(bytes));
    rows = img.as<double>();
    GSS_HIP(hipMemcpyAsync(rows, ccdf, bytes, hipMemcpyHostToDevice, s));
  }
  DevBuf acc;
  const bool want = ncorrected || maxcorr;
  if (want) {
    GSS_TRY(acc.alloc(2 * sizeof(unsigned long long)));
    GSS_HIP(hipMemsetAsync(acc.p, 0, 2 * sizeof(unsigned long long), s));
  }
  GSS_TRY(ik_order_dev(rows, m, K, want ? acc.as<unsigned long long>() : nullptr, s));
  if (mem == GSS_MEM_HOST) GSS_HIP(hipMemcpyAsync(ccdf, rows, bytes, hipMemcpyDeviceToHost, s));
  if (want) {
    unsigned long long h[2] = {0, 0};
    GSS_HIP(hipMemcpyAsync(h, acc.p, sizeof(h), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
    if (ncorrected) *ncorrected = (int64_t)h[0];
    if (maxcorr) std::memcpy(maxcorr, &h[1], sizeof(double));
  } else if (mem == GSS_MEM_HOST) {
    GSS_HIP(hipStreamSynchronize(s));
  }
  return GSS_OK;
}

int32_t gss_ik_post(const double* ccdf, int64_t m, int32_t K, const double* cutoffs, double zmin, double zmax,
                    double w_lo, double w_hi, const double* thresholds, int32_t nthr, const double* probs, int32_t nq,
                    double* etype, double* cvar, double* pabove, double* quant, int32_t mem, void* stream) {
  GSS_ENTRY();
  const char* who = "gss_ik_post";
  GSS_TRY(ik_check_cutoffs(who, cutoffs, K));
  GSS_REQUIRE(std::isfinite(zmin) && std::isfinite(zmax) && zmin < cutoffs[0] && zmax > cutoffs[K - 1],
              "%s: zmin %g / zmax %g must enclose the cutoffs strictly", who, zmin, zmax);
  GSS_REQUIRE(w_lo > 0.0 && w_hi > 0.0 && std::isfinite(w_lo) && std::isfinite(w_hi),
              "%s: tail exponents %g / %g must be positive", who, w_lo, w_hi);
  GSS_REQUIRE(nthr >= 0 && nthr <= 16 && nq >= 0 && nq <= 16, "%s: %d thresholds / %d probabilities: at most 16 each",
              who, nthr, nq);
  GSS_REQUIRE((nthr == 0 || thresholds) && (nq == 0 || probs), "%s: NULL thresholds / probs", who);
  GSS_REQUIRE((!pabove || nthr > 0) && (!quant || nq > 0), "%s: an output without thresholds / probabilities", who);
  IkPostSpec sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.K = K;
  sp.nthr = pabove ? nthr : 0;
  sp.nq = quant ? nq : 0;
  sp.zmin = zmin;
  sp.zmax = zmax;
  sp.wlo = w_lo;
  sp.whi = w_hi;
  for (int q = 0; q < K; ++q) sp.cut[q] = cutoffs[q];
  for (int i = 0; i < nthr; ++i) {
    GSS_REQUIRE(thresholds[i] >= zmin && thresholds[i] <= zmax, "%s: threshold %d = %g outside [zmin, zmax]", who, i,
                thresholds[i]);
    sp.thr[i] = thresholds[i];
  }
  for (int i = 0; i < nq; ++i) {
    GSS_REQUIRE(probs[i] > 0.0 && probs[i] < 1.0, "%s: probability %d = %g outside (0, 1)", who, i, probs[i]);
    sp.prob[i] = probs[i];
  }
  GSS_REQUIRE(m >= 0 && (m == 0 || ccdf), "%s: NULL array", who);
  if (m == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  Staged sc, se, sv, spa, sq;
  GSS_TRY(sc.in(ccdf, sizeof(double) * (size_t)(m * K), mem, s));
  GSS_TRY(se.out(etype, sizeof(double) * (size_t)m, mem));
  GSS_TRY(sv.out(cvar, sizeof(double) * (size_t)m, mem));
  GSS_TRY(spa.out(pabove, sizeof(double) * (size_t)(m * (nthr > 0 ? nthr : 1)), mem));
  GSS_TRY(sq.out(quant, sizeof(double) * (size_t)(m * (nq > 0 ? nq : 1)), mem));
  const dim3 grid((unsigned)((m + 255) / 256)), block(256);
  const bool v2 = (K & 1) == 0 && (reinterpret_cast<uintptr_t>(sc.p) & 15) == 0;
  {
    ProfScope ps("ik_post", s);
    if (v2)
      hipLaunchKernelGGL(ik_post_kernel<true>, grid, block, 0, s, sp, sc.as<double>(), m, se.as<double>(),
                         sv.as<double>(), spa.as<double>(), sq.as<double>());
    else
      hipLaunchKernelGGL(ik_post_kernel<false>, grid, block, 0, s, sp, sc.as<double>(), m, se.as<double>(),
                         sv.as<double>(), spa.as<double>(), sq.as<double>());
    GSS_HIP(hipGetLastError());
  }
  GSS_TRY(se.back(s));
  GSS_TRY(sv.back(s));
  GSS_TRY(spa.back(s));
  GSS_TRY(sq.back(s));
  if (mem == GSS_MEM_HOST) GSS_HIP(hipStreamSynchronize(s));   // the staged ccdf is released on return
  return GSS_OK;
}

}  // extern "C"
