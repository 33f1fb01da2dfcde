// IDW and LWR estimation on the exact k-NN kernel.
//
//   gss_idw_predict  <- /root/reference/src/estimation/idw.jl:111-142
//   gss_lwr_predict  <- /root/reference/src/estimation/lwr.jl:114-147
//
// Two device paths, chosen by the neighbour count the searcher would return (ui.jl:16-23):
//   * k <= 64     : K4 (k-d ordered exact k-NN) then one wave per estimation point, lane = neighbour;
//   * k == n > 64 : "all samples" (maxneighbors = nothing): no search at all, one thread per estimation
//                   point sweeping the samples staged through LDS (broadcast reads).
// Cross-validation (gss_idw_cv / gss_lwr_cv, gss.h): the same two paths with the samples as estimation points -- the
// fold-aware search in front of the list kernels, and for k == n a self-join with an eligibility test per pair.
// The masked and the unmasked all-sample kernels are one body each with the test as a compile-time choice:
// est_all_body<DIM, ZC, CV> behind est_all_kernel / est_cv_all_kernel, idw_all_fast_body<DIM, E1, CV> behind
// idw_all_fast_kernel / idw_cv_all_fast_kernel; the __global__ wrappers only load the query (and its fold).  Shared
// pieces: idw_recip (the rsq / rcp Newton steps), lwr_moments (the S1 / S2 / b update, est_list_kernel too),
// est_stage_tile (the LDS tile of the general sweep), sqdist_fma.  Host side: with_dim (gss_internal.h) turns dim into a
// template argument for every launch; idw_spec / lwr_spec build the EstSpec of the predict and the cv entry points.
// LWR solves its (d+1) x (d+1) normal equations about the estimation point (same predictor, better conditioned
// than the raw coordinates the reference uses) with an unpivoted Cholesky; a non-positive pivot is reported as
// GSS_PT_SINGULAR where the reference's `\` would throw.
#include "cv_fold.h"
#include "gss_internal.h"

#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace gss {

struct EstSpec {
  int method;       // 0 = IDW, 1 = LWR
  const double* wsup;   // LWR: weights supplied per (point, neighbour) instead of wkind (gss_lwr_predict_weights)
  int wkind;        // GSS_WEIGHT_*
  double exponent;  // IDW
  double wa, wp;    // LWR weight parameters
  int metric;       // GSS_METRIC_* of the search (distances entering the weights use it too)
  double mparam;
  // value columns that share the search and the weights (idw.jl:128-141 is generic over the value type: a composition's
  // log-parts, several variables on one sample set): column c of the data at z + c * ldz, of the estimates at
  // mean + c * ldm; distance / variance / status are per point
  int nz;
  int64_t ldz, ldm;
};

// ranking key of the search for a runtime metric
template <int DIM>
__device__ __forceinline__ double est_key(int metric, const double* a, const double* b, const double* ir, bool aniso) {
  switch (metric) {
    case GSS_METRIC_CITYBLOCK: return metric_key<DIM, GSS_METRIC_CITYBLOCK>(a, b, ir, aniso);
    case GSS_METRIC_CHEBYSHEV: return metric_key<DIM, GSS_METRIC_CHEBYSHEV>(a, b, ir, aniso);
    case GSS_METRIC_HAVERSINE: return metric_key<DIM, GSS_METRIC_HAVERSINE>(a, b, ir, aniso);
    default: return sqdist_nofma<DIM>(a, b, ir, aniso);
  }
}

__device__ __forceinline__ double idw_weight(double d, double d2, double e) {
  if (e == 1.0) return 1.0 / d;
  if (e == 2.0) return 1.0 / d2;
  return 1.0 / pow(d, e);
}

__device__ __forceinline__ double lwr_weight(int kind, double a, double p, double h) {
  if (kind == GSS_WEIGHT_TRICUBE) {
    const double t = 1.0 - h * h * h;
    return t * t * t;
  }
  const double hp = (p == 2.0) ? h * h : (p == 1.0 ? h : pow(h, p));
  return gss_exp(-a * hp);
}

// Weighted least squares about the estimation point.  S1 = X'WX, S2 = X'W^2 X (packed lower triangles, NP = DIM+1,
// u_0 = 1, u_a = x_a - x0_a), b = X'Wz.  mean = theta_0 with S1 theta = b; "variance" = |W X S1^-1 e_1| =
// sqrt(a' S2 a) with S1 a = e_1 (lwr.jl:139-145).  Returns false when S1 is not positive definite.
template <int NP>
__device__ __forceinline__ bool lwr_solve(const double* S1, const double* S2, const double* b, double* mean,
                                          double* var) {
  double L[NP][NP];
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) L[i][j] = S1[i * (i + 1) / 2 + j];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const double ajj = L[j][j];
    double d = ajj;
#pragma unroll
    for (int c = 0; c < j; ++c) d -= L[j][c] * L[j][c];
    if (!(d > 1e-13 * ajj) || !(ajj > 0.0)) ok = false;
    const double l = sqrt(d > 0.0 ? d : 1.0);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < NP; ++i) {
      double s = L[i][j];
#pragma unroll
      for (int c = 0; c < j; ++c) s -= L[i][c] * L[j][c];
      L[i][j] = s / l;
    }
  }
  if (!ok) return false;
  double t[NP], a[NP];
  // theta = S1^-1 b
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double s = b[i];
#pragma unroll
    for (int c = 0; c < i; ++c) s -= L[i][c] * t[c];
    t[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {
    double s = t[i];
#pragma unroll
    for (int c = i + 1; c < NP; ++c) s -= L[c][i] * t[c];
    t[i] = s / L[i][i];
  }
  *mean = t[0];
  // a = S1^-1 e_1
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double s = (i == 0) ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < i; ++c) s -= L[i][c] * a[c];
    a[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {
    double s = a[i];
#pragma unroll
    for (int c = i + 1; c < NP; ++c) s -= L[c][i] * a[c];
    a[i] = s / L[i][i];
  }
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int hi = i > j ? i : j, lo = i > j ? j : i;
      q += a[i] * S2[hi * (hi + 1) / 2 + lo] * a[j];
    }
  *var = sqrt(q > 0.0 ? q : 0.0);
  return true;
}

// One sample's term of the LWR moments: S1 += w u u', S2 += w^2 u u', b_c += w u z_c for the ncz live columns
// (zval(c): the sample's value in column c).  Shared by the all-sample sweep and est_list_kernel.
template <int NP, int ZC, class Z>
__device__ __forceinline__ void lwr_moments(double w, const double* u, int ncz, Z&& zval, double* S1, double* S2,
                                            double (*b)[NP]) {
#pragma unroll
  for (int r = 0; r < NP; ++r) {
    const double wu = w * u[r];
#pragma unroll
    for (int c = 0; c < ZC; ++c)
      if (c < ncz) b[c][r] += wu * zval(c);
#pragma unroll
    for (int q = 0; q <= r; ++q) {
      const double t = wu * u[q];
      S1[r * (r + 1) / 2 + q] += t;
      S2[r * (r + 1) / 2 + q] += w * t;
    }
  }
}

// 1 / d (E1) from v_rsq_f64 or 1 / d^2 from v_rcp_f64 of a squared distance, two Newton steps each.  d2 == 0 gives
// NaN (0 * inf inside the step): the callers select or detect it, they never multiply it away.
template <bool E1>
__device__ __forceinline__ double idw_recip(double d2) {
  double y;
  if (E1) {
    y = __builtin_amdgcn_rsq(d2);
    const double hh = 0.5 * d2;
    y = fma(y, fma(-hh * y, y, 0.5), y);
    y = fma(y, fma(-hh * y, y, 0.5), y);
  } else {
    y = __builtin_amdgcn_rcp(d2);
    y = fma(y, fma(-d2, y, 1.0), y);
    y = fma(y, fma(-d2, y, 1.0), y);
  }
  return y;
}

// squared Euclidean distance of the scalar-operand kernels: one fma per axis, in axis order
template <int DIM>
__device__ __forceinline__ double sqdist_fma(const double* xj, const double* qc) {
  double d2 = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const double t = xj[a] - qc[a];
    d2 = fma(t, t, d2);
  }
  return d2;
}

// ---------------------------------------------------------------------------------------------
// k <= 64: one wave per estimation point on the neighbour lists written by K4
// ---------------------------------------------------------------------------------------------
// GW = lanes per estimation point: 64 (one wave per point) or 16 when k <= 16 (four points per wave: the reductions
// are four shuffle steps instead of six and are shared by four points)
template <int GW>
__device__ __forceinline__ double grp_sum(double v) {
#pragma unroll
  for (int off = GW / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
template <int GW>
__device__ __forceinline__ double grp_max(double v) {
#pragma unroll
  for (int off = GW / 2; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}
template <int GW>
__device__ __forceinline__ double grp_min(double v) {
#pragma unroll
  for (int off = GW / 2; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}

template <int DIM, int GW>
__global__ __launch_bounds__(256) void est_knn_kernel(EstSpec sp, const double* __restrict__ xdata,
                                                      const double* __restrict__ z, const double* __restrict__ x0,
                                                      int64_t m, int k, int minneighbors,
                                                      const int* __restrict__ idx, const int* __restrict__ count,
                                                      int aniso, double ir0, double ir1, double ir2,
                                                      double* __restrict__ mean_out, double* __restrict__ aux_out,
                                                      uint8_t* __restrict__ status_out) {
  constexpr int PPW = 64 / GW;  // points per wave
  const int lane = threadIdx.x & 63;
  const int gl = lane % GW, grp = lane / GW;
  const int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * PPW + grp;
  const bool valid = p < m;
  const int64_t pc = valid ? p : m - 1;
  const double NaN = __builtin_nan("");
  const int cnt = count[pc];
  const bool missing = cnt < minneighbors || cnt < 1;  // idw.jl:123-124, lwr.jl:126-127
  const double ir[3] = {ir0, ir1, ir2};
  double qc[DIM], c[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) qc[a] = x0[pc * DIM + a];
  const bool act = !missing && gl < cnt;
  const int i = act ? idx[pc * k + gl] : 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) c[a] = xdata[(int64_t)i * DIM + a];
  const double d2 = est_key<DIM>(sp.metric, c, qc, ir, aniso != 0);  // the key the search ranked by
  const double d = metric_dist(sp.metric, d2, sp.mparam);
  double res_aux = NaN;
  int res_status = GSS_PT_MISSING;

  if (sp.method == 0) {
    const unsigned long long zb = __ballot(act && d2 == 0.0);
    unsigned long long gz = zb;
    if (GW < 64) gz = (zb >> (grp * (GW & 63))) & ((1ull << (GW & 63)) - 1ull);
    const bool haszero = gz != 0ull;  // idw.jl:131-134: some distance is zero -> copy the first such sample
    const int jz = haszero ? __builtin_ctzll(gz) + grp * GW : lane;
    const double w = (act && !haszero) ? idw_weight(d, sp.metric == GSS_METRIC_EUCLIDEAN ? d2 : d * d, sp.exponent) : 0.0;
    const double sw = grp_sum<GW>(w);
    const double dmin = grp_min<GW>(act ? d : __builtin_huge_val());
    for (int cz = 0; cz < sp.nz; ++cz) {   // one weight vector, every value column (idw.jl:138)
      const double zi = z[(int64_t)cz * sp.ldz + i];
      const double zj = __shfl(zi, jz);
      const double swz = grp_sum<GW>(w * zi);
      if (valid && gl == 0) mean_out[(int64_t)cz * sp.ldm + p] = missing ? NaN : (haszero ? zj : swz / sw);
    }
    if (!missing) {
      res_aux = haszero ? 0.0 : dmin;  // idw.jl:139
      res_status = GSS_PT_OK;
    }
  } else {
    constexpr int NP = DIM + 1, NT = NP * (NP + 1) / 2;
    const double dmax = grp_max<GW>(act ? d : 0.0);
    const double w = act ? lwr_weight(sp.wkind, sp.wa, sp.wp, d / dmax) : 0.0;  // lwr.jl:132,136
    double u[NP];
    u[0] = 1.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) u[a + 1] = c[a] - qc[a];
    double S1[NT], S2[NT];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
#pragma unroll
      for (int q = 0; q <= r; ++q) {
        const double t = w * u[r] * u[q];
        S1[r * (r + 1) / 2 + q] = grp_sum<GW>(t);
        S2[r * (r + 1) / 2 + q] = grp_sum<GW>(w * t);
      }
    }
    bool ok = !missing && (dmax > 0.0);
    double var = 0.0;
    for (int cz = 0; cz < sp.nz; ++cz) {   // the normal equations are the same for every value column
      const double zi = z[(int64_t)cz * sp.ldz + i];
      double b[NP];
#pragma unroll
      for (int r = 0; r < NP; ++r) b[r] = grp_sum<GW>(w * u[r] * zi);
      double mu = 0.0;
      ok = ok && lwr_solve<NP>(S1, S2, b, &mu, &var);
      if (valid && gl == 0) mean_out[(int64_t)cz * sp.ldm + p] = ok ? mu : NaN;
    }
    if (!missing) {
      res_aux = ok ? var : NaN;
      res_status = ok ? GSS_PT_OK : GSS_PT_SINGULAR;
    }
  }
  if (valid && gl == 0) {
    aux_out[p] = res_aux;
    status_out[p] = (uint8_t)res_status;
  }
}

// ---------------------------------------------------------------------------------------------
// k == n: every sample (inside the ball, if any) is a neighbour; one thread per estimation point
// ---------------------------------------------------------------------------------------------
constexpr int EST_TILE = 1024;

// The reference's default IDW -- every sample a neighbour (idw.jl:93), Euclidean distance, no ball, exponent 1 or 2 --
// as a dedicated kernel: thread = estimation point, and the sample index is wave-uniform, so coordinates and values
// arrive through the scalar cache into SGPRs (no LDS staging, no vector loads) and enter the VALU instructions as
// scalar operands.  Seventeen vector instructions per sample and point: three differences, the squared distance,
// its running minimum (idw.jl:137 returns the nearest distance), 1 / d from v_rsq_f64 (1 / d^2 from v_rcp_f64) with two
// Newton steps, and the two sums.  A coincident sample turns the weight into NaN (0 * inf inside the Newton step): that
// is detected once at the end, and only such points rescan the samples for the first zero distance (idw.jl:131-134).
//
// CV (the self-join of cross-validation, below): sample j counts iff fold[j] != myfold; the fold id arrives as a scalar
// operand like the rest.  The weight of an ineligible sample is selected to zero, never multiplied by it -- the query's
// own sample has d^2 = 0 and the NaN of the Newton step would pass through a product -- and its d^2 is kept out of the
// running minimum.  A NaN or infinite sum therefore means a coincident ELIGIBLE sample, and the rescan applies the
// same test.  Without CV there is no fold load, no count and no select.
template <int DIM, bool E1, bool CV>
__device__ __forceinline__ void idw_all_fast_body(const double* __restrict__ xdata, const double* __restrict__ z,
                                                  const int* __restrict__ fold, int n, const double* qc, int myfold,
                                                  bool live, int64_t p, int minneighbors,
                                                  double* __restrict__ mean_out, double* __restrict__ aux_out,
                                                  uint8_t* __restrict__ status_out) {
  double sw = 0.0, swz = 0.0, dmin2 = __builtin_huge_val();
  int cnt = 0;
#pragma unroll 8
  for (int j = 0; j < n; ++j) {
    const double d2 = sqdist_fma<DIM>(xdata + (int64_t)j * DIM, qc);
    const bool in = !CV || fold[j] != myfold;   // (without CV: true at compile time, the selects below fold away)
    cnt += in ? 1 : 0;
    dmin2 = fmin(dmin2, in ? d2 : __builtin_huge_val());
    const double y = idw_recip<E1>(d2);
    const double w = in ? y : 0.0;
    sw += w;
    swz = fma(w, z[j], swz);
  }
  if (!live) return;
  double mu = swz / sw, dist = gss_sqrt(dmin2);
  if (!(sw < __builtin_huge_val())) {  // NaN (coincident sample) or overflow: the estimate is the first coincident value
    for (int j = 0; j < n; ++j) {
      const double d2 = sqdist_fma<DIM>(xdata + (int64_t)j * DIM, qc);
      if ((!CV || fold[j] != myfold) && d2 == 0.0) {
        mu = z[j];
        dist = 0.0;
        break;
      }
    }
  }
  const bool enough = !CV || (cnt >= minneighbors && cnt >= 1);
  const double NaN = __builtin_nan("");
  mean_out[p] = enough ? mu : NaN;
  aux_out[p] = enough ? dist : NaN;
  status_out[p] = enough ? GSS_PT_OK : GSS_PT_MISSING;
}

template <int DIM, bool E1>
__global__ __launch_bounds__(256) void idw_all_fast_kernel(const double* __restrict__ xdata,
                                                           const double* __restrict__ z, int n,
                                                           const double* __restrict__ x0, int64_t m,
                                                           double* __restrict__ mean_out,
                                                           double* __restrict__ aux_out,
                                                           uint8_t* __restrict__ status_out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < m;
  double qc[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) qc[a] = live ? x0[p * DIM + a] : 0.0;
  idw_all_fast_body<DIM, E1, false>(xdata, z, nullptr, n, qc, 0, live, p, 0, mean_out, aux_out, status_out);
}

// The same for cross-validation (one column, no exclusion radius): query p of a launch is sample qoff + p.
template <int DIM, bool E1>
__global__ __launch_bounds__(256) void idw_cv_all_fast_kernel(const double* __restrict__ xdata,
                                                              const double* __restrict__ z,
                                                              const int* __restrict__ fold, int n, int64_t qoff,
                                                              int64_t m, int minneighbors,
                                                              double* __restrict__ mean_out,
                                                              double* __restrict__ aux_out,
                                                              uint8_t* __restrict__ status_out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < m;
  const int64_t g = live ? qoff + p : qoff;   // (qoff < n: a launch has at least one query)
  double qc[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) qc[a] = xdata[g * DIM + a];
  idw_all_fast_body<DIM, E1, true>(xdata, z, fold, n, qc, fold[g], live, p, minneighbors, mean_out, aux_out,
                                   status_out);
}

// ZC = value columns carried through one sweep (1, or up to 4 of a multi-column call: sp.nz columns are served in
// chunks of ZC, each chunk sweeping the samples again -- the weights of a sweep are shared by its columns).
// The samples pass through LDS in pieces of EST_TILE; the self-join of cross-validation (CV) keeps their fold ids
// beside them, the plain kernel has no such array.
template <int DIM, int ZC, bool CV>
struct EstTile {
  double x[EST_TILE * DIM];
  double z[ZC][EST_TILE];
};
template <int DIM, int ZC>
struct EstTile<DIM, ZC, true> : EstTile<DIM, ZC, false> {
  int f[EST_TILE];
};

// samples t0 .. t0 + tn of the ncz live columns into the tile (a barrier on either side)
template <int DIM, int ZC, bool CV>
__device__ __forceinline__ void est_stage_tile(EstTile<DIM, ZC, CV>& tile, const double* __restrict__ xdata,
                                               const double* __restrict__ zc, int64_t ldz,
                                               const int* __restrict__ fold, int t0, int tn, int ncz) {
  __syncthreads();
  for (int e = threadIdx.x; e < tn * DIM; e += 256) tile.x[e] = xdata[(int64_t)t0 * DIM + e];
  if constexpr (CV)
    for (int e = threadIdx.x; e < tn; e += 256) tile.f[e] = fold[t0 + e];
#pragma unroll
  for (int c = 0; c < ZC; ++c)
    if (c < ncz)
      for (int e = threadIdx.x; e < tn; e += 256) tile.z[c][e] = zc[(int64_t)c * ldz + t0 + e];
  __syncthreads();
}

// The general all-sample sweep of one estimation point qc (thread p of the launch).  Sample j is a neighbour iff it
// lies inside the ball, if any (key <= r2), and, for CV, fold[j] != myfold and key > ex (ex = -1: no exclusion ball;
// every key is >= 0): one predicate per pair, the same in every sweep.
template <int DIM, int ZC, bool CV>
__device__ __forceinline__ void est_all_body(EstTile<DIM, ZC, CV>& tile, const EstSpec& sp,
                                             const double* __restrict__ xdata, const double* __restrict__ z,
                                             const int* __restrict__ fold, int n, const double* qc, int myfold,
                                             bool live, int64_t p, int minneighbors, double ex, double r2, int use_ball,
                                             int aniso, const double* ir, double* __restrict__ mean_out,
                                             double* __restrict__ aux_out, uint8_t* __restrict__ status_out) {
  const double NaN = __builtin_nan("");
  constexpr int NP = DIM + 1, NT = NP * (NP + 1) / 2;
  const bool euclid = sp.metric == GSS_METRIC_EUCLIDEAN;
  auto neighbour = [&](int j, double d2) __attribute__((always_inline)) {
    if constexpr (CV) return tile.f[j] != myfold && d2 > ex && (!use_ball || d2 <= r2);
    else return !use_ball || d2 <= r2;
  };

  for (int c0 = 0; c0 < sp.nz; c0 += ZC) {
  const int ncz = (sp.nz - c0) < ZC ? (sp.nz - c0) : ZC;
  const double* zc = z + (int64_t)c0 * sp.ldz;
  double* mo = mean_out + (int64_t)c0 * sp.ldm;
  int cnt = 0;
  double dmax2 = 0.0, dmin2 = __builtin_huge_val();
  double sw = 0.0, swz[ZC], zzero[ZC];
#pragma unroll
  for (int c = 0; c < ZC; ++c) swz[c] = zzero[c] = 0.0;
  bool haszero = false;
  // sweep 1: IDW sums (complete) / LWR farthest neighbour
  for (int t0 = 0; t0 < n; t0 += EST_TILE) {
    const int tn = (n - t0) < EST_TILE ? (n - t0) : EST_TILE;
    est_stage_tile(tile, xdata, zc, sp.ldz, fold, t0, tn, ncz);
    if (sp.method == 0 && euclid && (sp.exponent == 1.0 || sp.exponent == 2.0)) {
      // the reference's default (all samples, exponent 1) and its square: branch-free, four samples in flight
      const bool e1 = sp.exponent == 1.0;
#pragma unroll 4
      for (int j = 0; j < tn; ++j) {
        const double d2 = sqdist_nofma<DIM>(&tile.x[j * DIM], qc, ir, aniso != 0);
        const bool in = neighbour(j, d2);
        const bool zero = in && d2 == 0.0;
        cnt += in ? 1 : 0;
        dmin2 = (in && d2 < dmin2) ? d2 : dmin2;
#pragma unroll
        for (int c = 0; c < ZC; ++c) zzero[c] = (zero && !haszero && c < ncz) ? tile.z[c][j] : zzero[c];
        haszero = haszero || zero;
        const double y = e1 ? idw_recip<true>(d2) : idw_recip<false>(d2);
        const double w = (in && !zero) ? y : 0.0;
        sw += w;
#pragma unroll
        for (int c = 0; c < ZC; ++c)
          if (c < ncz) swz[c] = fma(w, tile.z[c][j], swz[c]);
      }
      continue;
    }
    if (sp.method == 1 && euclid) {  // LWR, first sweep: farthest neighbour and count
#pragma unroll 4
      for (int j = 0; j < tn; ++j) {
        const double d2 = sqdist_nofma<DIM>(&tile.x[j * DIM], qc, ir, aniso != 0);
        const bool in = neighbour(j, d2);
        cnt += in ? 1 : 0;
        dmax2 = (in && d2 > dmax2) ? d2 : dmax2;
      }
      continue;
    }
    for (int j = 0; j < tn; ++j) {
      const double d2 = est_key<DIM>(sp.metric, &tile.x[j * DIM], qc, ir, aniso != 0);
      if (!neighbour(j, d2)) continue;
      ++cnt;
      dmax2 = d2 > dmax2 ? d2 : dmax2;
      dmin2 = d2 < dmin2 ? d2 : dmin2;
      if (sp.method == 0) {
        if (d2 == 0.0) {
          if (!haszero) {
#pragma unroll
            for (int c = 0; c < ZC; ++c)
              if (c < ncz) zzero[c] = tile.z[c][j];
          }
          haszero = true;
        } else {
          const double dd = metric_dist(sp.metric, d2, sp.mparam);
          const double w = idw_weight(dd, euclid ? d2 : dd * dd, sp.exponent);
          sw += w;
#pragma unroll
          for (int c = 0; c < ZC; ++c)
            if (c < ncz) swz[c] += w * tile.z[c][j];
        }
      }
    }
  }
  const bool enough = cnt >= minneighbors && cnt >= 1;
  if (sp.method == 0) {
    if (live) {
#pragma unroll
      for (int c = 0; c < ZC; ++c)
        if (c < ncz) mo[(int64_t)c * sp.ldm + p] = !enough ? NaN : (haszero ? zzero[c] : swz[c] / sw);
      if (c0 == 0) {
        aux_out[p] = !enough ? NaN : (haszero ? 0.0 : metric_dist(sp.metric, dmin2, sp.mparam));
        status_out[p] = enough ? GSS_PT_OK : GSS_PT_MISSING;
      }
    }
    continue;
  }
  // sweep 2 (LWR): moments with delta = d / dmax over the same neighbours
  const double dmax = metric_dist(sp.metric, dmax2, sp.mparam);
  double S1[NT] = {}, S2[NT] = {}, b[ZC][NP] = {};
  for (int t0 = 0; t0 < n; t0 += EST_TILE) {
    const int tn = (n - t0) < EST_TILE ? (n - t0) : EST_TILE;
    est_stage_tile(tile, xdata, zc, sp.ldz, fold, t0, tn, ncz);
    const bool gauss_w = sp.wkind == GSS_WEIGHT_EXP && sp.wp == 2.0;  // exp(-a delta^2): no square root needed
    const double inv_dmax2 = 1.0 / dmax2;
    for (int j = 0; j < tn; ++j) {
      const double d2 = euclid ? sqdist_nofma<DIM>(&tile.x[j * DIM], qc, ir, aniso != 0)
                               : est_key<DIM>(sp.metric, &tile.x[j * DIM], qc, ir, aniso != 0);
      if (!neighbour(j, d2)) continue;
      double w;
      if (euclid && gauss_w) w = gss_exp(-sp.wa * (d2 * inv_dmax2));
      else if (euclid) w = lwr_weight(sp.wkind, sp.wa, sp.wp, gss_sqrt(d2 * inv_dmax2));
      else w = lwr_weight(sp.wkind, sp.wa, sp.wp, metric_dist(sp.metric, d2, sp.mparam) / dmax);
      double u[NP];
      u[0] = 1.0;
#pragma unroll
      for (int a = 0; a < DIM; ++a) u[a + 1] = tile.x[j * DIM + a] - qc[a];
      lwr_moments<NP, ZC>(w, u, ncz, [&](int c) { return tile.z[c][j]; }, S1, S2, b);
    }
  }
  if (live) {
    bool ok = enough && ((!CV && sp.wsup != nullptr) || dmax > 0.0);   // (no supplied weights in cross-validation)
    double var = 0.0;
#pragma unroll
    for (int c = 0; c < ZC; ++c) {
      if (c < ncz) {
        double mu = 0.0;
        ok = ok && lwr_solve<NP>(S1, S2, b[c], &mu, &var);
        mo[(int64_t)c * sp.ldm + p] = ok ? mu : NaN;
      }
    }
    if (c0 == 0) {
      aux_out[p] = ok ? var : NaN;
      status_out[p] = !enough ? GSS_PT_MISSING : (ok ? GSS_PT_OK : GSS_PT_SINGULAR);
    }
  }
  }
}

template <int DIM, int ZC>
__global__ __launch_bounds__(256) void est_all_kernel(EstSpec sp, const double* __restrict__ xdata,
                                                      const double* __restrict__ z, int n,
                                                      const double* __restrict__ x0, int64_t m, int minneighbors,
                                                      double r2, int use_ball, int aniso, double ir0, double ir1,
                                                      double ir2, double* __restrict__ mean_out,
                                                      double* __restrict__ aux_out, uint8_t* __restrict__ status_out) {
  __shared__ EstTile<DIM, ZC, false> tile;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < m;
  const double ir[3] = {ir0, ir1, ir2};
  double qc[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) qc[a] = live ? x0[p * DIM + a] : 0.0;
  est_all_body<DIM, ZC, false>(tile, sp, xdata, z, nullptr, n, qc, 0, live, p, minneighbors, -1.0, r2, use_ball, aniso,
                               ir, mean_out, aux_out, status_out);
}

// The self-join of cross-validation (gss.h, gss_idw_cv / gss_lwr_cv): query p of a launch is sample qoff + p.  `fold`
// is never NULL here: for leave-one-out the driver passes the samples' indices (est_cv_iota_kernel).  Outputs are the
// launch's own slices (column c of the estimates at mean_out + c * sp.ldm).
template <int DIM, int ZC>
__global__ __launch_bounds__(256) void est_cv_all_kernel(EstSpec sp, const double* __restrict__ xdata,
                                                         const double* __restrict__ z,
                                                         const int* __restrict__ fold, int n, int64_t qoff, int64_t m,
                                                         int minneighbors, double ex, double r2, int use_ball,
                                                         int aniso, double ir0, double ir1, double ir2,
                                                         double* __restrict__ mean_out, double* __restrict__ aux_out,
                                                         uint8_t* __restrict__ status_out) {
  __shared__ EstTile<DIM, ZC, true> tile;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < m;
  const int64_t g = live ? qoff + p : qoff;   // (qoff < n: a launch has at least one query)
  const double ir[3] = {ir0, ir1, ir2};
  double qc[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) qc[a] = xdata[g * DIM + a];
  est_all_body<DIM, ZC, true>(tile, sp, xdata, z, fold, n, qc, fold[g], live, p, minneighbors, ex, r2, use_ball, aniso,
                              ir, mean_out, aux_out, status_out);
}

// The reference's default LWR -- every sample a neighbour (lwr.jl:96), Euclidean distance, no ball, weight
// exp(-a delta^2) (lwr.jl:58 has a = 3) -- with the samples as scalar operands like idw_all_fast_kernel.  Sweep 1: the
// farthest sample (lwr.jl:132 normalises by it); sweep 2: the weighted moments of lwr.jl:136-145; the weight needs no
// square root because delta^2 = d^2 / dmax^2.
template <int DIM>
__global__ __launch_bounds__(256) void lwr_all_fast_kernel(double wa, const double* __restrict__ xdata,
                                                           const double* __restrict__ z, int n,
                                                           const double* __restrict__ x0, int64_t m,
                                                           double* __restrict__ mean_out,
                                                           double* __restrict__ aux_out,
                                                           uint8_t* __restrict__ status_out) {
  constexpr int NP = DIM + 1, NT = NP * (NP + 1) / 2;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < m;
  double qc[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) qc[a] = live ? x0[p * DIM + a] : 0.0;
  double dmax2 = 0.0;
#pragma unroll 8
  for (int j = 0; j < n; ++j) dmax2 = fmax(dmax2, sqdist_fma<DIM>(xdata + (int64_t)j * DIM, qc));
  const double scale = -wa / dmax2;
  double S1[NT] = {}, S2[NT] = {}, b[NP] = {};
#pragma unroll 2
  for (int j = 0; j < n; ++j) {
    double u[NP];
    u[0] = 1.0;
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      u[a + 1] = xdata[(int64_t)j * DIM + a] - qc[a];
      d2 = fma(u[a + 1], u[a + 1], d2);
    }
    const double w = gss_exp_poly(scale * d2);
    const double w2 = w * w, wz = w * z[j];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
      b[r] = fma(wz, u[r], b[r]);
#pragma unroll
      for (int q = 0; q <= r; ++q) {
        const double t = u[r] * u[q];
        S1[r * (r + 1) / 2 + q] = fma(w, t, S1[r * (r + 1) / 2 + q]);
        S2[r * (r + 1) / 2 + q] = fma(w2, t, S2[r * (r + 1) / 2 + q]);
      }
    }
  }
  if (!live) return;
  const double NaN = __builtin_nan("");
  double mu, var;
  const bool ok = (dmax2 > 0.0) && lwr_solve<NP>(S1, S2, b, &mu, &var);
  mean_out[p] = ok ? mu : NaN;
  aux_out[p] = ok ? var : NaN;
  status_out[p] = ok ? GSS_PT_OK : GSS_PT_SINGULAR;
}

// leave-one-out through the self-join kernels: every sample its own fold
__global__ __launch_bounds__(256) void est_cv_iota_kernel(int* __restrict__ out, int n) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = j;
}

// ---------------------------------------------------------------------------------------------
// 64 < k < n: one thread per estimation point walks its neighbour list (m x k, ascending key, written by the
// passes of the search).  Same sums, in the same (ascending-distance) order, as est_knn_kernel.
// ---------------------------------------------------------------------------------------------
template <int DIM, int ZC>
__global__ __launch_bounds__(256) void est_list_kernel(EstSpec sp, const double* __restrict__ xdata,
                                                       const double* __restrict__ z, const double* __restrict__ x0,
                                                       int64_t m, int k, int minneighbors, const int* __restrict__ idx,
                                                       const int* __restrict__ count, int aniso, double ir0, double ir1,
                                                       double ir2, double* __restrict__ mean_out,
                                                       double* __restrict__ aux_out, uint8_t* __restrict__ status_out,
                                                       int ncheck) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= m) return;
  const double ir[3] = {ir0, ir1, ir2};
  const double NaN = __builtin_nan("");
  constexpr int NP = DIM + 1, NT = NP * (NP + 1) / 2;
  double qc[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) qc[a] = x0[p * DIM + a];
  int cnt = count[p];
  const int* nb = idx + p * k;
  bool bad = false;
  if (ncheck > 0) {   // lists that come from the caller (gss_lwr_predict_weights): never gather through a bad entry
    cnt = cnt > k ? k : cnt;
    for (int j = 0; j < cnt; ++j) bad |= (unsigned)nb[j] >= (unsigned)ncheck;
  }
  if (bad || cnt < minneighbors || cnt < 1) {
    for (int c = 0; c < sp.nz; ++c) mean_out[(int64_t)c * sp.ldm + p] = NaN;
    aux_out[p] = NaN;
    status_out[p] = bad ? GSS_PT_SINGULAR : GSS_PT_MISSING;
    return;
  }
  for (int c0 = 0; c0 < sp.nz; c0 += ZC) {   // the columns of a chunk share one walk along the list and its weights
    const int ncz = (sp.nz - c0) < ZC ? (sp.nz - c0) : ZC;
    const double* zc = z + (int64_t)c0 * sp.ldz;
    double* mo = mean_out + (int64_t)c0 * sp.ldm;
    if (sp.method == 0) {
      double sw = 0.0, swz[ZC], dmin2 = __builtin_huge_val();
#pragma unroll
      for (int c = 0; c < ZC; ++c) swz[c] = 0.0;
      int jz = -1;
      for (int j = 0; j < cnt; ++j) {
        const int nj = nb[j];
        double xj[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) xj[a] = xdata[(int64_t)nj * DIM + a];
        const double d2 = est_key<DIM>(sp.metric, xj, qc, ir, aniso != 0);
        if (d2 == 0.0) {  // neighbours are sorted: the first zero distance is the first neighbour (idw.jl:131-134)
          jz = nj;
          break;
        }
        dmin2 = d2 < dmin2 ? d2 : dmin2;
        const double dd = metric_dist(sp.metric, d2, sp.mparam);
        const double w = idw_weight(dd, sp.metric == GSS_METRIC_EUCLIDEAN ? d2 : dd * dd, sp.exponent);
        sw += w;
#pragma unroll
        for (int c = 0; c < ZC; ++c)
          if (c < ncz) swz[c] += w * zc[(int64_t)c * sp.ldz + nj];
      }
#pragma unroll
      for (int c = 0; c < ZC; ++c)
        if (c < ncz) mo[(int64_t)c * sp.ldm + p] = jz >= 0 ? zc[(int64_t)c * sp.ldz + jz] : swz[c] / sw;
      if (c0 == 0) {
        aux_out[p] = jz >= 0 ? 0.0 : metric_dist(sp.metric, dmin2, sp.mparam);
        status_out[p] = GSS_PT_OK;
      }
      continue;
    }
    // LWR: delta = d / d_max with d_max the distance of the last (farthest) neighbour (lwr.jl:132)
    double dmax2 = 0.0;
    {
      const int nl = nb[cnt - 1];
      double xl[DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a) xl[a] = xdata[(int64_t)nl * DIM + a];
      dmax2 = est_key<DIM>(sp.metric, xl, qc, ir, aniso != 0);
    }
    const double dmax = metric_dist(sp.metric, dmax2, sp.mparam);
    double S1[NT] = {}, S2[NT] = {}, b[ZC][NP] = {};
    for (int j = 0; j < cnt; ++j) {
      const int nj = nb[j];
      double xj[DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a) xj[a] = xdata[(int64_t)nj * DIM + a];
      const double d2 = est_key<DIM>(sp.metric, xj, qc, ir, aniso != 0);
      const double w = sp.wsup ? sp.wsup[p * k + j]
                               : lwr_weight(sp.wkind, sp.wa, sp.wp, metric_dist(sp.metric, d2, sp.mparam) / dmax);
      double u[NP];
      u[0] = 1.0;
#pragma unroll
      for (int a = 0; a < DIM; ++a) u[a + 1] = xj[a] - qc[a];
      lwr_moments<NP, ZC>(w, u, ncz, [&](int c) { return zc[(int64_t)c * sp.ldz + nj]; }, S1, S2, b);
    }
    bool ok = sp.wsup != nullptr || dmax > 0.0;
    double var = 0.0;
#pragma unroll
    for (int c = 0; c < ZC; ++c) {
      if (c < ncz) {
        double mu = 0.0;
        ok = ok && lwr_solve<NP>(S1, S2, b[c], &mu, &var);
        mo[(int64_t)c * sp.ldm + p] = ok ? mu : NaN;
      }
    }
    if (c0 == 0) {
      aux_out[p] = ok ? var : NaN;
      status_out[p] = ok ? GSS_PT_OK : GSS_PT_SINGULAR;
    }
  }
}

// Cross-validation on the list estimators (gss_idw_cv / gss_lwr_cv, k < n): the centres are the samples themselves
// (x0 = sr.xs, m = n) and the search of every chunk takes the fold mask of its queries.
struct EstCv {
  KnnMask mask;                // KnnMask::Fold over the samples
  int *idx_out, *count_out;    // the lists of the call (n x k, n) where the caller asked for them, else NULL
};

// GSS_EST_CV_CHUNK caps the samples per chunk of a cross-validation call (tests: a chunk loop that runs more than once
// at a small size)
static int64_t est_cv_chunk_cap(int64_t chunk) {
  if (const char* e = std::getenv("GSS_EST_CV_CHUNK")) {
    const int64_t cap = std::atoll(e);
    if (cap > 0 && cap < chunk) chunk = cap;
  }
  return chunk;
}

// xdata / x0: samples and domain on the Searcher's frame, which the weights are evaluated on as well
static int32_t est_local_dev(const EstSpec& sp, Searcher& sr, const double* z, const double* x0, int64_t m, int k,
                             int minneighbors, double* mean, double* aux, uint8_t* status, hipStream_t s,
                             HostPipe* pipe = nullptr /* k <= 64 only */, const EstCv* cv = nullptr /* k < n only */) {
  const double* xdata = sr.xs;
  const int64_t n = sr.n;
  const int dim = sr.dim, use_ball = sr.use_ball, aniso = sr.aniso;
  const double r2 = sr.r2;
  const double* ir = sr.ir;
  const char* pname = sp.method == 0 ? (cv ? "idw_cv" : "idw") : (cv ? "lwr_cv" : "lwr");
  int* const idx_out = cv ? cv->idx_out : nullptr;
  int* const count_out = cv ? cv->count_out : nullptr;
  if (k > 64 && (int64_t)k == n) {   // every sample: no search
    ProfScope ps(pname, s);
    const dim3 grid((unsigned)((m + 255) / 256));
    with_dim(dim, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      // (the two dedicated kernels carry one value column; several columns share the sweeps of the general kernel)
      auto fast = [&](auto kernel, auto... head) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, head..., xdata, z, (int)n, x0, m, mean, aux, status);
      };
      auto general = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, sp, xdata, z, (int)n, x0, m, minneighbors, r2, use_ball, aniso,
                           ir[0], ir[1], ir[2], mean, aux, status);
      };
      if (sp.nz == 1 && sp.method == 0 && sp.metric == GSS_METRIC_EUCLIDEAN && !use_ball &&
          (sp.exponent == 1.0 || sp.exponent == 2.0) && minneighbors <= n) {
        if (sp.exponent == 1.0) fast(idw_all_fast_kernel<DIM, true>);
        else fast(idw_all_fast_kernel<DIM, false>);
      } else if (sp.nz == 1 && sp.method == 1 && sp.metric == GSS_METRIC_EUCLIDEAN && !use_ball &&
                 sp.wkind == GSS_WEIGHT_EXP && sp.wp == 2.0 && minneighbors <= n) {
        fast(lwr_all_fast_kernel<DIM>, sp.wa);
      } else if (sp.nz > 1) {
        general(est_all_kernel<DIM, 4>);
      } else {
        general(est_all_kernel<DIM, 1>);
      }
    });
    GSS_HIP(hipGetLastError());
    return GSS_OK;
  }

  // k < n (or k = n <= 64): the search, chunk by chunk, in front of a list estimator.  k <= 64: one wave (k <= 16: a
  // quarter of one) per point; 65 .. n - 1 (ui.jl:16-23 accepts any count): the search runs in passes of 64 and the
  // estimator walks the lists with one thread per point
  const bool piped = k <= 64 && pipe && pipe->on;   // host arrays of the domain arrive and leave piece by piece
  int64_t chunk = k <= 64 ? (piped ? HostPipe::PIECE : (1 << 20)) : (k > 512 ? (1 << 16) : (1 << 19));
  if (cv) chunk = est_cv_chunk_cap(chunk);
  DevBuf idx_s, cnt_s;
  if (!idx_out) GSS_TRY(idx_s.alloc(sizeof(int) * (size_t)((m < chunk ? m : chunk) * k)));
  if (!count_out) GSS_TRY(cnt_s.alloc(sizeof(int) * (size_t)(m < chunk ? m : chunk)));
  for (int64_t off = 0; off < m; off += chunk) {
    const int64_t mv = (m - off) < chunk ? (m - off) : chunk;
    int* idx = idx_out ? idx_out + off * k : idx_s.as<int>();
    int* cnt = count_out ? count_out + off : cnt_s.as<int>();
    if (piped) GSS_TRY(pipe->fetch(off, mv, s));
    {
      ProfScope ps("knn", s);
      const KnnMask mk = cv ? cv->mask.from(off) : KnnMask();   // cross-validation: the query folds of this chunk
      GSS_TRY(sr.query(x0 + off * dim, nullptr, mv, k, idx, cnt, s, cv ? &mk : nullptr));
    }
    ProfScope pl(pname, s);
    with_dim(dim, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      auto launch = [&](auto kernel, int per_block, auto... ncheck) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((mv + per_block - 1) / per_block)), dim3(256), 0, s, sp, xdata, z,
                           x0 + off * dim, mv, k, minneighbors, idx, cnt, aniso, ir[0], ir[1], ir[2], mean + off,
                           aux + off, status + off, ncheck...);
      };
      if (k <= 16) launch(est_knn_kernel<DIM, 16>, 16);   // sixteen lanes per point, sixteen points per workgroup
      else if (k <= 64) launch(est_knn_kernel<DIM, 64>, 4);
      else if (sp.nz > 1) launch(est_list_kernel<DIM, 4>, 256, 0);
      else launch(est_list_kernel<DIM, 1>, 256, 0);
    });
    GSS_HIP(hipGetLastError());
    if (piped) GSS_TRY(pipe->deliver(off, mv, s));
  }
  if (piped) GSS_TRY(pipe->finish(s));
  GSS_HIP(hipStreamSynchronize(s));  // scratch and the search index are released on return
  return GSS_OK;
}

static int32_t est_predict(EstSpec sp, const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz,
                           const double* xdom, int64_t m, int32_t k, int32_t minneighbors, double radius,
                           const double* inv_radii, double* mean, double* aux, uint8_t* status, int32_t mem,
                           void* stream) {
  GSS_REQUIRE(nz >= 1 && nz <= 4096, "%d value columns: 1 .. 4096", nz);
  sp.nz = nz;
  sp.ldz = n;
  sp.ldm = m;
  GSS_REQUIRE(n >= 1 && n < INT_MAX, "estimation requires data");  // idw.jl:95
  GSS_REQUIRE(dim >= 1 && dim <= 3, "dim = %d outside 1..3", dim);
  GSS_REQUIRE(k >= 1 && k <= n, "maxneighbors %d outside 1..%lld (searcher_ui clamps it, ui.jl:18-20)", k,
              (long long)n);
  GSS_REQUIRE(minneighbors <= k, "invalid min/max number of neighbors");  // idw.jl:97, lwr.jl:99
  // GSS_METRIC_ROTATED_BALL: the axis-aligned ball on frame coordinates (origin xdata[0]); the weights then use the
  // ball-metric distances, and LWR's affine regression does not depend on the frame
  Searcher sr;
  GSS_TRY(sr.init(sp.metric, sp.mparam, radius, inv_radii, dim));
  sp.metric = sr.metric;
  GSS_REQUIRE(m >= 0 && (m == 0 || (xdata && z && xdom && mean && aux)), "NULL array");
  if (m == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  Staged sxd, sz;
  GSS_TRY(sxd.in(xdata, sizeof(double) * n * dim, mem, s));
  if (sr.frame.on) GSS_TRY(frame_origin(&sr.frame, xdata, mem, s));
  GSS_TRY(sr.samples(sxd.as<double>(), nullptr, n, s));
  GSS_TRY(sz.in(z, sizeof(double) * n * nz, mem, s));
  DomainCall dc;   // host arrays of the domain: in and out piece by piece beside the computation (k <= 64, one column)
  dc.in(xdom, sizeof(double) * dim);
  Staged& smean = *dc.out(mean, sizeof(double), nz);
  Staged& saux = *dc.out(aux, sizeof(double));
  Staged& sstat = *dc.out(status, 1);
  GSS_TRY(dc.begin(mem, m, s, k <= 64 && nz == 1, &sr.frame));
  DevBuf st_own;
  uint8_t* st = sstat.as<uint8_t>();
  if (!status) {
    GSS_TRY(st_own.alloc((size_t)m));
    st = st_own.as<uint8_t>();
  }
  GSS_TRY(est_local_dev(sp, sr, sz.as<double>(), dc.x(), m, k, minneighbors, smean.as<double>(), saux.as<double>(), st, s,
                        &dc.pipe));
  GSS_TRY(dc.finish(s));   // (piped: est_local_dev ended with pipe.finish and a synchronisation, everything is home)
  if (!status) GSS_HIP(hipStreamSynchronize(s));  // st_own is released on return
  return GSS_OK;
}

// Cross-validation with every eligible sample (k == n): the self-join kernels over the samples on the Searcher's frame.
// fold: the caller's ids on the device, or NULL for leave-one-out (the indices are written out once).
static int32_t est_cv_all_dev(const EstSpec& sp, const Searcher& sr, const double* z, const int* fold, double ex,
                              int minneighbors, double* mean, double* aux, uint8_t* status, hipStream_t s) {
  const double* xdata = sr.xs;
  const int64_t n = sr.n;
  const int dim = sr.dim, use_ball = sr.use_ball, aniso = sr.aniso;
  const double r2 = sr.r2;
  const double* ir = sr.ir;
  DevBuf own;
  if (!fold) {
    GSS_TRY(own.alloc(sizeof(int) * (size_t)n));
    hipLaunchKernelGGL(est_cv_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, own.as<int>(), (int)n);
    GSS_HIP(hipGetLastError());
    fold = own.as<int>();
  }
  ProfScope ps(sp.method == 0 ? "idw_cv" : "lwr_cv", s);   // the self-join alone, not the indices above
  const bool fast = sp.nz == 1 && sp.method == 0 && sp.metric == GSS_METRIC_EUCLIDEAN && !use_ball && ex < 0.0 &&
                    (sp.exponent == 1.0 || sp.exponent == 2.0);
  const int64_t chunk = est_cv_chunk_cap(n);
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t mv = (n - off) < chunk ? (n - off) : chunk;
    const dim3 grid((unsigned)((mv + 255) / 256));
    with_dim(dim, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      auto masked_fast = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, xdata, z, fold, (int)n, off, mv, minneighbors, mean + off,
                           aux + off, status + off);
      };
      auto general = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, sp, xdata, z, fold, (int)n, off, mv, minneighbors, ex, r2,
                           use_ball, aniso, ir[0], ir[1], ir[2], mean + off, aux + off, status + off);
      };
      if (fast && sp.exponent == 1.0) masked_fast(idw_cv_all_fast_kernel<DIM, true>);
      else if (fast) masked_fast(idw_cv_all_fast_kernel<DIM, false>);
      else if (sp.nz > 1) general(est_cv_all_kernel<DIM, 4>);
      else general(est_cv_all_kernel<DIM, 1>);
    });
    GSS_HIP(hipGetLastError());
  }
  if (own.p) GSS_HIP(hipStreamSynchronize(s));   // the indices are released on return
  return GSS_OK;
}

// gss_idw_cv / gss_lwr_cv (gss.h): every check that needs no device comes first
static int32_t est_cv(EstSpec sp, const char* who, const double* xdata, const double* z, int64_t n, int32_t dim,
                      int32_t nz, const int32_t* fold, double exclude_radius, int32_t k, int32_t minneighbors,
                      double radius, const double* inv_radii, double* pred, double* aux, uint8_t* status,
                      int32_t* idx_out, int32_t* count_out, int32_t mem, void* stream) {
  GSS_REQUIRE(nz >= 1 && nz <= 4096, "%s: %d value columns: 1 .. 4096", who, nz);
  sp.nz = nz;
  sp.ldz = n;
  sp.ldm = n;
  GSS_REQUIRE(n >= 2 && n < INT_MAX, "%s: cross-validation needs at least two samples", who);
  GSS_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside 1..3", who, dim);
  GSS_REQUIRE(k >= 1 && k <= n, "%s: maxneighbors %d outside 1..n = %lld (n: every eligible sample; a sample is never "
                                "its own neighbour)", who, k, (long long)n);
  GSS_REQUIRE(minneighbors <= k, "%s: invalid min/max number of neighbors", who);  // idw.jl:97, lwr.jl:99
  GSS_REQUIRE(!(exclude_radius != exclude_radius), "%s: exclude_radius is NaN", who);
  const bool all = (int64_t)k == n;
  GSS_REQUIRE(!all || (!idx_out && !count_out), "%s: maxneighbors = n runs no search: idx_out / count_out must be NULL",
              who);
  if (!all && sp.metric == GSS_METRIC_HAVERSINE) {
    set_error("cross-validation under the haversine distance is not available: the fold search runs on the k-d index, "
              "which that key has no box bounds for (DESIGN.md section 7)");
    return GSS_ERR_UNSUPPORTED;
  }
  Searcher sr;
  GSS_TRY(sr.init(sp.metric, sp.mparam, radius, inv_radii, dim));
  sp.metric = sr.metric;
  GSS_REQUIRE(xdata && z && pred && aux, "%s: NULL array", who);
  std::vector<int32_t> fh;
  if (fold && mem == GSS_MEM_HOST) GSS_TRY(fold_ids_host(who, fold, n, mem, nullptr, &fh));
  hipStream_t s = to_stream(stream);
  if (fold && mem != GSS_MEM_HOST) GSS_TRY(fold_ids_host(who, fold, n, mem, s, &fh));
  Staged sxd, sz, sf;
  GSS_TRY(sxd.in(xdata, sizeof(double) * n * dim, mem, s));
  if (sr.frame.on) GSS_TRY(frame_origin(&sr.frame, xdata, mem, s));   // a rotated ball: origin xdata[0]
  GSS_TRY(sr.samples(sxd.as<double>(), nullptr, n, s));
  GSS_TRY(sz.in(z, sizeof(double) * n * nz, mem, s));
  if (fold) GSS_TRY(sf.in(fold, sizeof(int32_t) * (size_t)n, mem, s));
  DomainCall dc;   // the outputs over the n samples (whole: nothing is piped)
  Staged& smean = *dc.out(pred, sizeof(double), nz);
  Staged &saux = *dc.out(aux, sizeof(double)), &sstat = *dc.out(status, 1);
  Staged &sidx = *dc.out(idx_out, sizeof(int32_t) * (size_t)k), &scnt = *dc.out(count_out, sizeof(int32_t));
  GSS_TRY(dc.begin(mem, n, s, false, nullptr));
  DevBuf st_own;
  uint8_t* st = sstat.as<uint8_t>();
  if (!status) {
    GSS_TRY(st_own.alloc((size_t)n));
    st = st_own.as<uint8_t>();
  }
  const double ex = exclusion_key(exclude_radius, sr.metric);
  const int* fold_dev = fold ? sf.as<int>() : nullptr;   // the samples are the queries: one array serves both
  if (all) {
    GSS_TRY(est_cv_all_dev(sp, sr, sz.as<double>(), fold_dev, ex, minneighbors, smean.as<double>(), saux.as<double>(),
                           st, s));
  } else {
    const EstCv cv{KnnMask(KnnMask::Fold{fold_dev, fold_dev, 0, ex}), sidx.as<int>(), scnt.as<int>()};
    GSS_TRY(est_local_dev(sp, sr, sz.as<double>(), sr.xs, n, k, minneighbors, smean.as<double>(), saux.as<double>(), st,
                          s, nullptr, &cv));
  }
  GSS_TRY(dc.finish(s));
  GSS_HIP(hipStreamSynchronize(s));  // the staged samples and st_own are released on return
  return GSS_OK;
}

// The estimator of a predict or cross-validation call, its parameters checked (columns and strides: est_predict / est_cv)
static int32_t idw_spec(EstSpec* sp, int32_t metric, double metric_param, double exponent) {
  GSS_REQUIRE(exponent > 0.0, "exponent must be positive");  // idw.jl:96
  std::memset(sp, 0, sizeof(*sp));
  sp->method = 0;
  sp->exponent = exponent;
  sp->metric = metric;
  sp->mparam = metric_param;
  return GSS_OK;
}

static int32_t lwr_spec(EstSpec* sp, int32_t metric, double metric_param, int32_t weight_kind, double weight_a,
                        double weight_p) {
  GSS_REQUIRE(weight_kind == GSS_WEIGHT_EXP || weight_kind == GSS_WEIGHT_TRICUBE, "unknown weight function %d",
              weight_kind);
  GSS_REQUIRE(weight_kind != GSS_WEIGHT_EXP || weight_p > 0.0, "weight exponent must be positive");
  std::memset(sp, 0, sizeof(*sp));
  sp->method = 1;
  sp->wkind = weight_kind;
  sp->wa = weight_a;
  sp->wp = weight_p;
  sp->metric = metric;
  sp->mparam = metric_param;
  return GSS_OK;
}

}  // namespace gss

using namespace gss;

extern "C" {

int32_t gss_idw_predict_cols(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz,
                             const double* xdom, int64_t m, int32_t k, int32_t minneighbors, double radius,
                             const double* inv_radii, int32_t metric, double metric_param, double exponent, double* mean,
                             double* dist, uint8_t* status, int32_t mem, void* stream) {
  GSS_ENTRY();
  EstSpec sp;
  GSS_TRY(idw_spec(&sp, metric, metric_param, exponent));
  return est_predict(sp, xdata, z, n, dim, nz, xdom, m, k, minneighbors, radius, inv_radii, mean, dist, status, mem,
                     stream);
}

int32_t gss_idw_predict(const double* xdata, const double* z, int64_t n, int32_t dim, const double* xdom, int64_t m,
                        int32_t k, int32_t minneighbors, double radius, const double* inv_radii, int32_t metric,
                        double metric_param, double exponent, double* mean, double* dist, uint8_t* status, int32_t mem,
                        void* stream) {
  return gss_idw_predict_cols(xdata, z, n, dim, 1, xdom, m, k, minneighbors, radius, inv_radii, metric, metric_param,
                              exponent, mean, dist, status, mem, stream);
}

int32_t gss_lwr_predict_weights(const double* xdata, const double* z, int64_t n, int32_t dim, const double* xdom, int64_t m,
                                int32_t k, int32_t minneighbors, const int32_t* idx, const int32_t* count,
                                const double* weights, double* mean, double* var, uint8_t* status, int32_t mem,
                                void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(n >= 1 && n < INT_MAX && dim >= 1 && dim <= 3 && k >= 1 && k <= n, "gss_lwr_predict_weights: bad sizes");
  GSS_REQUIRE(m >= 0 && (m == 0 || (xdata && z && xdom && idx && count && weights && mean && var)), "NULL array");
  if (m == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  Staged sxd, sz, sx, si, sc, sw, smean, svar, sstat;
  GSS_TRY(sxd.in(xdata, sizeof(double) * n * dim, mem, s));
  GSS_TRY(sz.in(z, sizeof(double) * n, mem, s));
  GSS_TRY(sx.in(xdom, sizeof(double) * m * dim, mem, s));
  GSS_TRY(si.in(idx, sizeof(int32_t) * (size_t)(m * k), mem, s));
  GSS_TRY(sc.in(count, sizeof(int32_t) * (size_t)m, mem, s));
  GSS_TRY(sw.in(weights, sizeof(double) * (size_t)(m * k), mem, s));
  GSS_TRY(smean.out(mean, sizeof(double) * m, mem));
  GSS_TRY(svar.out(var, sizeof(double) * m, mem));
  DevBuf st_own;
  uint8_t* st = nullptr;
  if (status) {
    GSS_TRY(sstat.out(status, (size_t)m, mem));
    st = sstat.as<uint8_t>();
  } else {
    GSS_TRY(st_own.alloc((size_t)m));
    st = st_own.as<uint8_t>();
  }
  EstSpec sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.method = 1;
  sp.wsup = sw.as<double>();
  sp.nz = 1;
  sp.ldz = n;
  sp.ldm = m;
  const dim3 grid((unsigned)((m + 255) / 256));
  with_dim(dim, [&](auto D) {   // (the lists are the caller's: the kernel checks every entry against n)
    hipLaunchKernelGGL((est_list_kernel<decltype(D)::value, 1>), grid, dim3(256), 0, s, sp, sxd.as<double>(),
                       sz.as<double>(), sx.as<double>(), m, (int)k, (int)minneighbors, si.as<int>(), sc.as<int>(), 0, 1.0,
                       1.0, 1.0, smean.as<double>(), svar.as<double>(), st, (int)n);
  });
  GSS_HIP(hipGetLastError());
  GSS_TRY(smean.back(s));
  GSS_TRY(svar.back(s));
  if (status) GSS_TRY(sstat.back(s));
  GSS_HIP(hipStreamSynchronize(s));   // the staged copies are released on return
  return GSS_OK;
}

int32_t gss_lwr_predict(const double* xdata, const double* z, int64_t n, int32_t dim, const double* xdom, int64_t m,
                        int32_t k, int32_t minneighbors, double radius, const double* inv_radii, int32_t metric,
                        double metric_param, int32_t weight_kind, double weight_a, double weight_p, double* mean,
                        double* var, uint8_t* status, int32_t mem, void* stream) {
  return gss_lwr_predict_cols(xdata, z, n, dim, 1, xdom, m, k, minneighbors, radius, inv_radii, metric, metric_param,
                              weight_kind, weight_a, weight_p, mean, var, status, mem, stream);
}

int32_t gss_lwr_predict_cols(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz,
                             const double* xdom, int64_t m, int32_t k, int32_t minneighbors, double radius,
                             const double* inv_radii, int32_t metric, double metric_param, int32_t weight_kind,
                             double weight_a, double weight_p, double* mean, double* var, uint8_t* status, int32_t mem,
                             void* stream) {
  GSS_ENTRY();
  EstSpec sp;
  GSS_TRY(lwr_spec(&sp, metric, metric_param, weight_kind, weight_a, weight_p));
  return est_predict(sp, xdata, z, n, dim, nz, xdom, m, k, minneighbors, radius, inv_radii, mean, var, status, mem,
                     stream);
}

// ---- cross-validation (gss.h): every sample predicted from samples outside its own fold ------------------------------
int32_t gss_idw_cv(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz, const int32_t* fold,
                   double exclude_radius, int32_t k, int32_t minneighbors, double radius, const double* inv_radii,
                   int32_t metric, double metric_param, double exponent, double* pred, double* dist, uint8_t* status,
                   int32_t* idx_out, int32_t* count_out, int32_t mem, void* stream) {
  GSS_ENTRY();
  EstSpec sp;
  GSS_TRY(idw_spec(&sp, metric, metric_param, exponent));
  return est_cv(sp, "gss_idw_cv", xdata, z, n, dim, nz, fold, exclude_radius, k, minneighbors, radius, inv_radii, pred,
                dist, status, idx_out, count_out, mem, stream);
}

int32_t gss_lwr_cv(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz, const int32_t* fold,
                   double exclude_radius, int32_t k, int32_t minneighbors, double radius, const double* inv_radii,
                   int32_t metric, double metric_param, int32_t weight_kind, double weight_a, double weight_p,
                   double* pred, double* var, uint8_t* status, int32_t* idx_out, int32_t* count_out, int32_t mem,
                   void* stream) {
  GSS_ENTRY();
  EstSpec sp;
  GSS_TRY(lwr_spec(&sp, metric, metric_param, weight_kind, weight_a, weight_p));
  return est_cv(sp, "gss_lwr_cv", xdata, z, n, dim, nz, fold, exclude_radius, k, minneighbors, radius, inv_radii, pred,
                var, status, idx_out, count_out, mem, stream);
}

}  // extern "C"
