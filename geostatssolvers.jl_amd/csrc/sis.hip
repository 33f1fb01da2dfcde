// SIS: sequential indicator simulation (GSLIB sisim, median form) on an SGS handle (gss.h, gss_sis_realize; DESIGN.md
// section 4).  The reference has no indicator simulator; its CookieCutter (src/simulation/cookie.jl) needs a facies
// simulator, and the categorical kind is one.
//
// Median indicator kriging has ONE variogram for all cutoffs, hence one simple-kriging weight vector per node, and those
// weights depend on the path, the data cells and the variogram only.  So stage A of SGS (sgs_create.hip: masked search,
// weights, levels), run with the indicator variogram, is the whole realisation-independent part.  This file is stage B:
//
//   F_q[node] = F*_q + sum_j lambda_j (i_q(z[nb_j]) - F*_q),   i_q(z) = (z <= c_q)  (continuous)  |  (z == q)  (categorical)
//   z[node]   = draw(F, u(seed, realisation, node))
//
// K accumulators per lane (KT = K rounded up to 4 / 8 / 16: registers, unrolled), the cutoffs and F* in a by-value
// argument (wave-uniform: scalar registers).  The sweeps mirror the SGS ones that read their lists from memory; the field
// holds a cell's uniform in the cell's own slot until the cell is simulated.
#include "sgs_internal.h"
#include "philox.h"

#include <climits>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <vector>

namespace gss {

constexpr int SIS_MAXK = 16;

// Entries beyond K are padding that changes nothing.  Continuous: cut = +inf, fs = 1: every term is w * (1 - 1), F = 1,
// which the order-relation passes leave alone and never change a value below it.  Categorical: cut = -1 (no code), fs = 0:
// p = 0, which adds nothing to the sum or to the cumulated probabilities.
struct SisSpec {
  int K;
  double zmin, zmax, ilo, ihi;   // ilo = 1 / w_lo, ihi = 1 / w_hi
  double cut[SIS_MAXK];          // cutoffs | category codes 0 .. K-1
  double fs[SIS_MAXK];           // F* | p*
};

// The recursion step: acc[q] = sum_j w_j (i_q(z[nb_j * stride + r]) - F*_q) over a node's c neighbours, each sum by fma
// in list order, G gathers in flight.
template <int KT, bool CAT, int G>
__device__ __forceinline__ void sis_step(const SisSpec& sp, const int* __restrict__ nb, const double* __restrict__ ww, int c,
                                         const double* z, int64_t stride, int64_t r, double (&acc)[KT]) {
#pragma unroll
  for (int q = 0; q < KT; ++q) acc[q] = 0.0;
  auto term = [&](double wj, double zj) {
#pragma unroll
    for (int q = 0; q < KT; ++q) {
      const bool in = CAT ? zj == sp.cut[q] : zj <= sp.cut[q];
      acc[q] = fma(wj, (in ? 1.0 : 0.0) - sp.fs[q], acc[q]);
    }
  };
  int j = 0;
  for (; j + G <= c; j += G) {
    double zz[G];
#pragma unroll
    for (int u = 0; u < G; ++u) zz[u] = z[(int64_t)nb[j + u] * stride + r];
#pragma unroll
    for (int u = 0; u < G; ++u) term(ww[j + u], zz[u]);
  }
  for (; j < c; ++j) term(ww[j], z[(int64_t)nb[j] * stride + r]);
}

__device__ __forceinline__ double sis_pow(double x, double w) { return w == 1.0 ? x : pow(x, w); }

// Continuous draw: F = F* + acc, the order-relation correction of gss.h (clip, upward max, downward min, mean of the two;
// sequential per lane, the doubles of ik_order16), then the smallest z with F(z) >= u under the ccdf model of gss_ik_post.
template <int KT>
__device__ __forceinline__ double sis_draw_continuous(const SisSpec& sp, const double (&acc)[KT], double u) {
  double U[KT], D[KT], F[KT];
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    const double f = sp.fs[q] + acc[q];
    F[q] = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
  }
  U[0] = F[0];
#pragma unroll
  for (int q = 1; q < KT; ++q) U[q] = fmax(U[q - 1], F[q]);
  D[KT - 1] = F[KT - 1];
#pragma unroll
  for (int q = KT - 2; q >= 0; --q) D[q] = fmin(D[q + 1], F[q]);
#pragma unroll
  for (int q = 0; q < KT; ++q) F[q] = (U[q] + D[q]) * 0.5;
  const int K = sp.K;
  double Ftop = F[0], ctop = sp.cut[0];
#pragma unroll
  for (int q = 1; q < KT; ++q) {
    if (q < K) {
      Ftop = F[q];
      ctop = sp.cut[q];
    }
  }
  if (u <= F[0]) return F[0] > 0.0 ? sp.zmin + (sp.cut[0] - sp.zmin) * sis_pow(u / F[0], sp.ilo) : sp.zmin;
  if (u > Ftop) return sp.zmax - (sp.zmax - ctop) * sis_pow((1.0 - u) / (1.0 - Ftop), sp.ihi);
  // F_0 < u <= F_{K-1}: the first class whose upper value reaches u (descending loop: the lowest one wins), which is not
  // flat because the value below it is smaller than u
  double a = sp.cut[0], b = sp.cut[0], Fa = 0.0, Fb = 1.0;
#pragma unroll
  for (int q = KT - 1; q >= 1; --q) {
    if (q < K && u <= F[q]) {
      a = sp.cut[q - 1];
      b = sp.cut[q];
      Fa = F[q - 1];
      Fb = F[q];
    }
  }
  return a + (b - a) * ((u - Fa) / (Fb - Fa));
}

// Categorical draw: p = p* + acc clipped to [0, 1]; divided by the clipped sum where that is positive, else p*; cumulated
// in category order; the first category with u < cum, else (rounding at the top) the last one with a positive probability.
template <int KT>
__device__ __forceinline__ double sis_draw_categorical(const SisSpec& sp, const double (&acc)[KT], double u) {
  double p[KT];
  double sum = 0.0;
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    const double f = sp.fs[q] + acc[q];
    p[q] = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
    sum += p[q];
  }
  const bool ok = sum > 0.0;
  double cum = 0.0;
  int pick = -1, lastpos = 0;
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    const double pq = ok ? p[q] / sum : sp.fs[q];
    cum += pq;
    if (pq > 0.0) lastpos = q;
    if (pick < 0 && u < cum) pick = q;
  }
  return (double)(pick < 0 ? lastpos : pick);
}

template <int KT, bool CAT>
__device__ __forceinline__ double sis_draw(const SisSpec& sp, const double (&acc)[KT], double u) {
  if constexpr (CAT) return sis_draw_categorical<KT>(sp, acc, u);
  else return sis_draw_continuous<KT>(sp, acc, u);
}

// ---- the sweeps (indexing: sgs_level_sweep_kernel, sgs_level_sweep_paths_kernel, sgs_sweep_big_kernel,
//      sgs_sweep_paths_kernel of sgs.hip) ---------------------------------------------------------------------------------

// one level of a shared order: wave = (node of the level, block of 64 realisations) on the node-major field
template <int KT, bool CAT>
__global__ __launch_bounds__(256) void sis_level_sweep_kernel(SisSpec sp, const int* __restrict__ order, int first, int count,
                                                              const int* __restrict__ idx, const int* __restrict__ ncond,
                                                              const double* __restrict__ w, int k, int R, int rb,
                                                              double* __restrict__ zt) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (int64_t)count * rb) return;   // whole wave
  const int64_t node = order[first + (int)(item / rb)];
  const int r = (int)(item % rb) * 64 + lane;
  const bool live = r < R;
  const int rr = live ? r : R - 1;
  const double u = zt[node * R + rr];   // the cell's own slot holds its uniform until it is simulated
  double acc[KT];
  sis_step<KT, CAT, 8>(sp, idx + node * k, w + node * k, ncond[node], zt, R, rr, acc);
  const double v = sis_draw<KT, CAT>(sp, acc, u);
  if (live) zt[node * R + r] = v;
}

// one level of every visiting order at once: thread = (path, node) of the level, realisation-major field
template <int KT, bool CAT>
__global__ __launch_bounds__(256) void sis_level_sweep_paths_kernel(SisSpec sp, const int* __restrict__ order, int first,
                                                                    int count, const int* __restrict__ idx,
                                                                    const int* __restrict__ ncond,
                                                                    const double* __restrict__ w, int k, int64_t N, int R,
                                                                    int64_t path0, double* __restrict__ zr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int64_t g = order[first + i];
  const int64_t pi = g / N, node = g - pi * N;
  const int64_t r = pi - path0;              // realisation r of this call walks path path0 + r
  if (r < 0 || r >= R) return;
  double* z = zr + r * N;
  double acc[KT];
  sis_step<KT, CAT, 4>(sp, idx + g * k, w + g * k, ncond[g], z, 1, 0, acc);
  z[node] = sis_draw<KT, CAT>(sp, acc, z[node]);
}

// along a shared path, one lane per realisation: lists and weights are wave-uniform loads, the gathers coalesce
template <int KT, bool CAT>
__global__ __launch_bounds__(64) void sis_sweep_kernel(SisSpec sp, const int64_t* __restrict__ path,
                                                       const int* __restrict__ rank, const int* __restrict__ idx,
                                                       const int* __restrict__ ncond, const double* __restrict__ w, int k,
                                                       int64_t N, int R, double* __restrict__ zt) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  const bool live = r < R;
  const int rr = live ? r : R - 1;   // idle lanes shadow the last realisation (no stores): the wave stays uniform
  for (int64_t t = 0; t < N; ++t) {
    const int64_t node = path[t];
    if (rank[node] < 0) continue;  // conditioning cell
    double acc[KT];
    sis_step<KT, CAT, 8>(sp, idx + node * k, w + node * k, ncond[node], zt, R, rr, acc);
    const double v = sis_draw<KT, CAT>(sp, acc, zt[node * R + rr]);
    if (live) zt[node * R + r] = v;
  }
}

// along its own path, one lane per realisation on the realisation-major field
template <int KT, bool CAT>
__global__ __launch_bounds__(64) void sis_sweep_paths_kernel(SisSpec sp, const int64_t* __restrict__ paths,
                                                             const int* __restrict__ ranks, const int* __restrict__ idx,
                                                             const int* __restrict__ ncond, const double* __restrict__ w,
                                                             int k, int64_t N, int R, int64_t path0,
                                                             double* __restrict__ zr) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int64_t pi = path0 + r;                 // realisation r of this call walks path path0 + r
  const int64_t* path = paths + pi * N;
  const int* rank = ranks + pi * N;
  const int* nbr = idx + pi * N * k;
  const int* nc = ncond + pi * N;
  const double* wt = w + pi * N * k;
  double* z = zr + (int64_t)r * N;
  for (int64_t t = 0; t < N; ++t) {
    const int64_t node = path[t];
    if (rank[node] < 0) continue;               // conditioning cell
    double acc[KT];
    sis_step<KT, CAT, 4>(sp, nbr + node * k, wt + node * k, nc[node], z, 1, 0, acc);
    z[node] = sis_draw<KT, CAT>(sp, acc, z[node]);
  }
}

// ---- the field around the sweep: NODE_MAJOR zt[cell][r] (shared order) | zr[r][cell] (one order per realisation) ------

// z(cell, r) = u(seed, realisation, cell), element cell of gss_philox_uniform(seed, first_real + r, N), or uniforms[r][cell]
template <bool NODE_MAJOR>
__global__ __launch_bounds__(256) void sis_fill_kernel(int64_t N, int R, uint64_t seed, int64_t first_real,
                                                       const double* __restrict__ uniforms, double* __restrict__ z) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * R) return;
  const int64_t q = NODE_MAJOR ? e / R : e / N;
  const int64_t cell = NODE_MAJOR ? q : e - q * N;
  const int r = (int)(NODE_MAJOR ? e - q * R : q);
  double v;
  if (uniforms) {
    v = uniforms[(int64_t)r * N + cell];
  } else {
    double ua, ub;
    philox_pair(seed, (uint32_t)(first_real + r), STREAM_UNIFORM, (uint64_t)(cell >> 1), ua, ub);
    v = (cell & 1) ? ub : ua;
  }
  z[e] = v;
}

// z(dloc, r) = zdata for the conditioning cells
template <bool NODE_MAJOR>
__global__ __launch_bounds__(256) void sis_seed_data_kernel(int64_t N, int R, const int64_t* __restrict__ dlocs,
                                                            const double* __restrict__ zd, int64_t nd,
                                                            double* __restrict__ z) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nd * R) return;
  const int64_t q = NODE_MAJOR ? e / R : e / nd;
  const int64_t j = NODE_MAJOR ? q : e - q * nd;
  const int64_t r = NODE_MAJOR ? e - q * R : q;
  z[NODE_MAJOR ? dlocs[j] * R + r : r * N + dlocs[j]] = zd[j];
}

// out[r][cell] = zt[cell][r] through a 64 x 64 LDS tile (both sides coalesced)
__global__ __launch_bounds__(256) void sis_transpose_kernel(const double* __restrict__ zt, int64_t N, int R,
                                                            double* __restrict__ out) {
  __shared__ double tile[64][65];
  const int64_t c0 = (int64_t)blockIdx.x * 64;
  const int r0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int64_t c = c0 + i;
    const int r = r0 + tx;
    if (c < N && r < R) tile[i][tx] = zt[c * R + r];
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i;
    const int64_t c = c0 + tx;
    if (c < N && r < R) out[(int64_t)r * N + c] = tile[tx][i];
  }
}

// Average simulated nodes per level below which a handle with levels is swept along the path instead: a launch per level
// costs a launch whatever the level holds (3.9 us measured), the walk a round trip per node (2.2 - 2.4 us; DESIGN.md
// section 4 has the measurement: the ratio lies between 1.6 and 2.5 over kinds and K).
// GSS_SIS_WALK_BELOW overrides it, read at every call (tools/sis_sweep.py: 0 = always level by level, a huge value = always
// along the path).
constexpr double SIS_WALK_BELOW = 2.0;

static double sis_walk_below() {
  if (const char* e = std::getenv("GSS_SIS_WALK_BELOW")) {
    char* end = nullptr;
    const double v = std::strtod(e, &end);
    if (end != e && v >= 0.0) return v;
  }
  return SIS_WALK_BELOW;
}

// Realisations first_real .. first_real + nreals - 1 (a range gss_sis_realize has checked) with every array in HBM,
// asynchronous on s: fill uniforms, seed data, sweep, copy out.
template <int KT, bool CAT>
static int32_t sis_realize_block(gss_sgs_t* h, const SisSpec& sp, uint64_t seed, int64_t first_real, int64_t nreals,
                                 const double* uniforms, double* out, hipStream_t s) {
  const int64_t N = h->N;
  const int R = (int)nreals;
  const bool per_order = h->npaths > 1;
  const int L = h->lvl_off.empty() ? 0 : (int)h->lvl_off.size() - 2;
  const bool levels = L > 0 && (double)(N - h->nd) / (double)L >= sis_walk_below();
  const size_t elements = (size_t)N * (size_t)R;
  double* z = out;   // one order per realisation works in the output itself
  if (!per_order) {
    if (h->field.bytes < sizeof(double) * elements) {
      h->field.release();
      GSS_TRY(h->field.alloc(sizeof(double) * elements));
    }
    z = h->field.as<double>();
  }
  {
    ProfScope ps("sis_fill", s);
    const dim3 grid((unsigned)((elements + 255) / 256)), dgrid((unsigned)((h->nd * R + 255) / 256));
    if (per_order) {
      hipLaunchKernelGGL(sis_fill_kernel<false>, grid, dim3(256), 0, s, N, R, seed, first_real, uniforms, z);
      if (h->nd > 0)
        hipLaunchKernelGGL(sis_seed_data_kernel<false>, dgrid, dim3(256), 0, s, N, R, h->dlocs.as<int64_t>(),
                           h->zd.as<double>(), h->nd, z);
    } else {
      hipLaunchKernelGGL(sis_fill_kernel<true>, grid, dim3(256), 0, s, N, R, seed, first_real, uniforms, z);
      if (h->nd > 0)
        hipLaunchKernelGGL(sis_seed_data_kernel<true>, dgrid, dim3(256), 0, s, N, R, h->dlocs.as<int64_t>(),
                           h->zd.as<double>(), h->nd, z);
    }
    GSS_HIP(hipGetLastError());
  }
  {
    ProfScope ps("sis_sweep", s);
    const int* idx = h->idx.as<int>();
    const int* nc = h->ncond.as<int>();
    const double* w = h->w.as<double>();
    const dim3 walkers((unsigned)((R + 63) / 64));   // a lane per realisation walks the path
    if (levels) {   // a launch per level; with one order per realisation every order's level at once
      const int rb = (R + 63) / 64;
      for (int l = 1; l <= L; ++l) {
        const int first = h->lvl_off[(size_t)l], count = h->lvl_off[(size_t)l + 1] - first;
        if (count <= 0) continue;
        if (per_order)
          hipLaunchKernelGGL((sis_level_sweep_paths_kernel<KT, CAT>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s,
                             sp, h->order.as<int>(), first, count, idx, nc, w, h->k, N, R, first_real - h->path_base, z);
        else
          hipLaunchKernelGGL((sis_level_sweep_kernel<KT, CAT>), dim3((unsigned)(((int64_t)count * rb + 3) / 4)), dim3(256), 0,
                             s, sp, h->order.as<int>(), first, count, idx, nc, w, h->k, R, rb, z);
      }
    } else if (per_order) {
      hipLaunchKernelGGL((sis_sweep_paths_kernel<KT, CAT>), walkers, dim3(64), 0, s, sp, h->path.as<int64_t>(),
                         h->rank.as<int>(), idx, nc, w, h->k, N, R, first_real - h->path_base, z);
    } else {
      hipLaunchKernelGGL((sis_sweep_kernel<KT, CAT>), walkers, dim3(64), 0, s, sp, h->path.as<int64_t>(), h->rank.as<int>(),
                         idx, nc, w, h->k, N, R, z);
    }
    GSS_HIP(hipGetLastError());
  }
  if (!per_order) {
    hipLaunchKernelGGL(sis_transpose_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((R + 63) / 64)), dim3(256), 0, s, z,
                       N, R, out);
    GSS_HIP(hipGetLastError());
  }
  return GSS_OK;
}

template <bool CAT>
static int32_t sis_realize_kinds(gss_sgs_t* h, const SisSpec& sp, uint64_t seed, int64_t first_real, int64_t nreals,
                                 const double* uniforms, double* out, hipStream_t s) {
  if (sp.K <= 4) return sis_realize_block<4, CAT>(h, sp, seed, first_real, nreals, uniforms, out, s);
  if (sp.K <= 8) return sis_realize_block<8, CAT>(h, sp, seed, first_real, nreals, uniforms, out, s);
  return sis_realize_block<16, CAT>(h, sp, seed, first_real, nreals, uniforms, out, s);
}

}  // namespace gss

using namespace gss;

extern "C" {

int32_t gss_sis_realize(gss_sgs_t* h, int32_t kind, const double* cutoffs, int32_t K, const double* fstar, double zmin,
                        double zmax, double w_lo, double w_hi, uint64_t seed, int64_t first_real, int64_t nreals,
                        const double* uniforms, double* out, int32_t mem, void* stream) {
  GSS_ENTRY();
  const char* who = "gss_sis_realize";
  GSS_REQUIRE(kind == GSS_SIS_CONTINUOUS || kind == GSS_SIS_CATEGORICAL, "%s: kind %d: continuous (0) or categorical (1)",
              who, kind);
  GSS_REQUIRE(h != nullptr, "%s: NULL handle", who);
  const bool cat = kind == GSS_SIS_CATEGORICAL;
  GSS_REQUIRE(K >= (cat ? 2 : 1) && K <= SIS_MAXK, "%s: K = %d outside %d .. %d", who, K, cat ? 2 : 1, SIS_MAXK);
  GSS_REQUIRE(fstar != nullptr, "%s: fstar is NULL", who);
  SisSpec sp;
  sp.K = K;
  sp.zmin = sp.zmax = 0.0;
  sp.ilo = sp.ihi = 1.0;
  for (int q = 0; q < SIS_MAXK; ++q) {
    sp.cut[q] = cat ? -1.0 : std::numeric_limits<double>::infinity();
    sp.fs[q] = cat ? 0.0 : 1.0;
  }
  double psum = 0.0;
  for (int q = 0; q < K; ++q) {
    GSS_REQUIRE(fstar[q] >= 0.0 && fstar[q] <= 1.0, "%s: fstar[%d] = %g outside [0, 1]", who, q, fstar[q]);
    sp.fs[q] = fstar[q];
    psum += fstar[q];
  }
  if (cat) {
    GSS_REQUIRE(cutoffs == nullptr, "%s: the categorical kind takes no cutoffs", who);
    GSS_REQUIRE(std::fabs(psum - 1.0) <= 1e-9, "%s: the proportions sum to %.17g, not 1", who, psum);
    for (int q = 0; q < K; ++q) sp.cut[q] = (double)q;
  } else {
    GSS_REQUIRE(cutoffs != nullptr, "%s: cutoffs is NULL", who);
    for (int q = 0; q < K; ++q) {
      GSS_REQUIRE(std::isfinite(cutoffs[q]), "%s: cutoff %d is not finite", who, q);
      GSS_REQUIRE(q == 0 || cutoffs[q] > cutoffs[q - 1], "%s: cutoffs must increase strictly (cutoff %d)", who, q);
      GSS_REQUIRE(q == 0 || fstar[q] >= fstar[q - 1], "%s: fstar must not decrease (entry %d)", who, q);
      sp.cut[q] = cutoffs[q];
    }
    GSS_REQUIRE(std::isfinite(zmin) && std::isfinite(zmax) && zmin < cutoffs[0] && zmax > cutoffs[K - 1],
                "%s: zmin %g / zmax %g must enclose the cutoffs strictly", who, zmin, zmax);
    GSS_REQUIRE(w_lo > 0.0 && w_hi > 0.0 && std::isfinite(w_lo) && std::isfinite(w_hi),
                "%s: tail exponents %g / %g must be positive", who, w_lo, w_hi);
    sp.zmin = zmin;
    sp.zmax = zmax;
    sp.ilo = 1.0 / w_lo;
    sp.ihi = 1.0 / w_hi;
  }
  GSS_REQUIRE(nreals >= 0 && first_real >= 0 && nreals < INT_MAX, "%s: bad realisation range", who);
  GSS_REQUIRE(nreals == 0 || out != nullptr, "%s: out is NULL", who);
  const int64_t N = h->N;
  if (h->npaths > 1) {   // one visiting order per realisation: the rule of gss_sgs_realize
    const int64_t p0 = first_real - h->path_base;
    GSS_REQUIRE(p0 >= 0 && p0 + nreals <= h->npaths, "%s: realisations %lld..%lld have no visiting order in this handle "
                "(paths cover %lld..%lld)", who, (long long)first_real, (long long)(first_real + nreals - 1),
                (long long)h->path_base, (long long)(h->path_base + h->npaths - 1));
  }
  hipStream_t s = to_stream(stream);
  if (cat && h->nd > 0) {   // the codes at the conditioning cells, on a host copy
    std::vector<double> zd((size_t)h->nd);
    GSS_HIP(hipMemcpyAsync(zd.data(), h->zd.p, sizeof(double) * zd.size(), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < h->nd; ++j)
      GSS_REQUIRE(zd[(size_t)j] >= 0.0 && zd[(size_t)j] <= (double)(K - 1) && zd[(size_t)j] == std::floor(zd[(size_t)j]),
                  "%s: zdata[%lld] = %g is no category code 0 .. %d", who, (long long)j, zd[(size_t)j], K - 1);
  }
  if (nreals == 0) return GSS_OK;
  auto block = [&](int64_t first, int64_t n, const double* u, double* o) {
    return cat ? sis_realize_kinds<true>(h, sp, seed, first, n, u, o, s)
               : sis_realize_kinds<false>(h, sp, seed, first, n, u, o, s);
  };
  if (mem == GSS_MEM_DEVICE) {
    GSS_TRY(block(first_real, nreals, uniforms, out));
    GSS_HIP(hipStreamSynchronize(s));
    return GSS_OK;
  }
  // Host arrays: blocks of realisations -- whole groups of 64 lanes for a shared visiting order -- through the output
  // ring, as gss_sgs_realize
  int64_t rb = OutStream::default_chunk(sizeof(double) * (size_t)N, nreals);
  if (h->npaths <= 1 && rb < nreals) rb = rb < 64 ? 64 : rb / 64 * 64;
  if (rb > nreals) rb = nreals;
  OutStream os;
  GSS_TRY(os.begin(out, sizeof(double) * (size_t)N, nreals, mem, s, rb));
  DevBuf ubuf;
  if (uniforms) GSS_TRY(ubuf.alloc(sizeof(double) * (size_t)(rb * N)));
  for (int64_t r0 = 0; r0 < nreals; r0 += rb) {
    const int64_t n = nreals - r0 < rb ? nreals - r0 : rb;
    if (uniforms)
      GSS_HIP(hipMemcpyAsync(ubuf.p, uniforms + r0 * N, sizeof(double) * (size_t)(n * N), hipMemcpyHostToDevice, s));
    double* dout = nullptr;
    GSS_TRY(os.slot(r0, s, &dout));
    GSS_TRY(block(first_real + r0, n, uniforms ? ubuf.as<double>() : nullptr, dout));
    GSS_TRY(os.done(r0 + n - 1, s));
  }
  return os.finish(s);
}

}  // extern "C"
