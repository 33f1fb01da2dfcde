// K7: empirical variograms on the device (gss_variogram_empirical, gss_variogram_plane, gss_variogram_cross).  The model
// fits to them (gss_variogram_fit and its kin) are host code in variography_fit.hip.  Replaces [DEP] Variography's
// EmpiricalVariogram / DirectionalVariogram -- the step that produces the `variogram=` parameter every solver takes.
// The conventions are the library's own (include/gss.h).
//
// Three kernels -- vario_window_kernel (lag bins), vario_plane_kernel (sector and lag), vario_cross_kernel (products of
// differences) -- each hold their own accumulation and nothing of the others'.  What they share is written once, as
// __forceinline__ pieces: the LDS set-up (vario_lds_init), the unit draw with the triangle skip (vario_next_unit), the
// box cull (vario_cull), the load of batch J (vario_load_j), the pair key and pair test (vario_pair) and the copy-out
// (vario_copy_out).  One loop around an accumulator object was tried and cost registers ("Cross-variograms").
//
// Layout.  The samples are put in a space-filling order -- the Searcher's k-d order (knn_build.hip) from 32 768 samples,
// one sort by Morton key below that, where the level-by-level build would cost as much as the pair pass: batches of 64
// consecutive points with a bounding box each.  A tile is a pair of batches (I, J), I <= J: 64 x 64 sample pairs, the lower triangle only when
// I == J.  One wave works on one tile at a time: lane = point of batch J (coordinates and values in registers), the
// points of batch I are wave uniform and arrive through the scalar cache -- the operand layout of K1 (cov_kernels.hip).
//
// Work units are (batch I, 16 consecutive batches J -- 4 for small sets); the waves of a persistent grid draw them from
// one counter (one global atomic per unit of up to 65 536 pairs, per run of up to 64 units on large sets), so no round of workgroups waits for a straggler and the empty half of
// the triangle costs a comparison per unit.  In a unit, lanes 0..15 each bound one tile: the box-to-box lower bound of
// the squared distance, accumulated with the rounded operations of the pair key itself, so it never exceeds a real
// pair's key; a tile whose bound lies beyond the last bin edge is never opened, and the results cannot depend on that.
//
// Accumulation (vario_window_kernel).  Pairs of one tile fall into few neighbouring bins, all of them at or above the
// bin of the tile's lower bound.  Every lane therefore keeps a window of VW consecutive bins, starting at that bin, in registers (count, sum of
// h, sums per value column: selected with an exact 0 / 1 factor); the rare pair beyond the window goes to the
// workgroup's histogram in LDS with one LDS atomic per quantity.  After the tile the window is flushed to the same
// histogram.  At the end each workgroup writes its histogram to its own slice of a scratch array and a second kernel adds
// the slices in workgroup order: no global atomic per pair, 64-bit integer counts that do not depend on the schedule.
//
// Varioplane (gss_variogram_plane).  vario_plane_kernel bins every kept pair by (direction sector, lag), without the
// direction test of the other two: the sector is found by bisection over the sector boundaries held in LDS (the truth
// pattern of the header's rule is a prefix, so the bisection returns its count).  The wave-uniform window of lag bins does not carry
// over -- a near tile scatters over every sector -- but a far tile subtends few sectors and few lags, so consecutive
// pairs of a lane often share a bin: every lane keeps its current run (bin, count, sums) in registers and sends it to
// the workgroup's nangles x nlags histogram in LDS, one atomic per quantity, when the bin changes and after the tile.
// Plain LDS atomics for every pair lost to this by up to 3 x ("Varioplane").
//
// Cross-variograms (gss_variogram_cross).  vario_cross_kernel bins every kept pair once and adds the NZ (NZ + 1) / 2
// products dz_a dz_b of its value differences.  A window of VW bins times 36 products does not fit the register file
// (288 VGPRs at VW = 4), so the kernel takes the run form of the plane path for every NZ: a lane keeps one current bin
// (count, sum of h, NP products: NP + 2 accumulators) and sends it to the workgroup's histogram in LDS when the bin
// changes.  The bin is a lag, the same for a lane's whole life, so a run is carried across tiles and units and flushed
// last at the end of the kernel.  The histogram is (2 + NP) nlags + 2 words (78 KiB at NZ = 8, 256 lags: room for two
// workgroups per compute unit; the registers of that instantiation admit one).  Registers and times: DESIGN.md,
// "Cross-variograms".
//
// Ordering, check, gather, batches, grid sizing and the reduction are one host path for the three calls (vario_run).
#include "gss_internal.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace gss {

namespace {

constexpr int VARIO_MAX_LAGS = 256;
constexpr int VARIO_MAX_NZ = 8;
constexpr int VARIO_JW_MAX = 16;   // tiles per work unit: 16, or 4 when there are few batches (more, smaller units)
constexpr int VARIO_THREADS = 256;
constexpr int VARIO_PLANE_MAX_NZ = 4;
constexpr int VARIO_PLANE_MAX_ANGLES = 180;
constexpr int VARIO_PLANE_MAX_WORDS = 8192;   // nangles nlags (2 + nz): 64 KiB of histogram, two workgroups per CU

struct VarioArgs {
  int64_t n;
  int nb;
  int jw;               // tiles per unit
  int nchunks;          // ceil(nb / jw)
  int grab;             // units a wave draws per atomic (large sets: the counter must not become the bottleneck)
  int nlags;
  int directional;
  int nocull;
  double delta, inv_delta;
  double u[3];
  double dtol2, cos2;
  // varioplane (vario_plane_kernel only)
  int nangles;          // sectors
  int nsteps;           // ceil(log2(nangles)): bisection steps
  double e[9];          // 3-D: in-plane axes e1, e2 and the normal
  double ptol2;         // 3-D: fl(ptol^2), the slab
};

// the pair key: ((D0 D0) + (D1 D1)) + (D2 D2), one rounding per operation
template <int DIM>
__device__ __forceinline__ double vario_d2(const double* a, const double* b, double* delta) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const double t = a[k] - b[k];
    delta[k] = t;
    const double tt = t * t;
    acc = k == 0 ? tt : acc + tt;
  }
  return acc;
}

// lower bound of vario_d2 over two boxes: per axis the gap max(loA - hiB, loB - hiA, 0) never exceeds |a - b| for
// points inside (rounded subtraction is monotone and antisymmetric), and squares and sums are accumulated as above
template <int DIM>
__device__ __forceinline__ double vario_box_d2(const double* loa, const double* hia, const double* lob,
                                               const double* hib) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const double g1 = loa[k] - hib[k], g2 = lob[k] - hia[k];
    double t = g1 > g2 ? g1 : g2;
    t = t > 0.0 ? t : 0.0;
    const double tt = t * t;
    acc = k == 0 ? tt : acc + tt;
  }
  return acc;
}

// bin k with edge2[k] < d2 <= edge2[k + 1], for 0 < d2 <= edge2[nlags]; h = sqrt(d2).  The quotient h / delta places
// the pair within one bin of the right one (its error is a few ulp, a bin is at least 1 / 256 of the range); the two
// comparisons on d2 decide.
__device__ __forceinline__ int vario_bin(const double* edge2, int nlags, double d2, double h, double inv_delta) {
  int k = (int)(h * inv_delta);
  k = k < 0 ? 0 : (k > nlags - 1 ? nlags - 1 : k);
  const double e0 = edge2[k], e1 = edge2[k + 1];
  k += (d2 > e1 ? 1 : 0) - (d2 <= e0 ? 1 : 0);   // both edges are read: no divergent branch around the second
  return k < 0 ? 0 : (k > nlags - 1 ? nlags - 1 : k);
}

__device__ __forceinline__ void lds_add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }

// (D0 e0 + D1 e1) + D2 e2, one rounding per operation
__device__ __forceinline__ double vario_project(const double* dl, const double* e) {
#pragma clang fp contract(off)
  const double t = dl[0] * e[0] + dl[1] * e[1];
  return t + dl[2] * e[2];
}

// Sector of the in-plane lag (a1, a2) by the rule of gss.h: p = c_0 a2, q = s_0 a1; p == q: sector 0; p < q: negate;
// then the number of s >= 1 with c_s a2 >= s_s a1.  Those s form a prefix 1 .. S (the boundaries turn one way through
// less than pi), so S is found by bisection: boundary `lo` holds (0 does after the negation), boundary `hi` does not
// (nangles: there is none).  dir: (c_s, s_s) pairs in LDS; nsteps = ceil(log2(nangles)), the same for every lane.
__device__ __forceinline__ int vario_sector(const double* dir, int nangles, int nsteps, double a1, double a2) {
#pragma clang fp contract(off)
  const double p = dir[0] * a2, q = dir[1] * a1;
  const bool flip = p < q;
  a1 = flip ? -a1 : a1;
  a2 = flip ? -a2 : a2;
  int lo = 0, hi = nangles;
  for (int it = 0; it < nsteps; ++it) {
    const int mid = (lo + hi) >> 1;   // == lo once hi - lo == 1: the comparison below then holds again
    const double l = dir[2 * mid] * a2, r = dir[2 * mid + 1] * a1;
    const bool ge = l >= r;
    lo = ge ? mid : lo;
    hi = ge ? hi : mid;
  }
  return p == q ? 0 : lo;
}

// ---- the pieces of the pair pass that the three kernels below share ------------------------------------------------
// Every kernel takes the same arguments and lays out its dynamic LDS the same way: nlags + 1 squared bin edges, then
// what is flushed -- cnt[nbins], ndup, opened, hsum[nbins], sums[rows nbins] -- then whatever else the kernel wants.

// squared bin edges edge2[k] = fl(fl(k delta)^2): two rounded products of exactly represented operands, the same
// doubles on every workgroup and on the host; the histogram is cleared; ends with the barrier
__device__ __forceinline__ void vario_lds_init(double* s_edge, unsigned long long* s_cnt, int nlags, int nwords,
                                               double delta) {
  for (int t = threadIdx.x; t <= nlags; t += VARIO_THREADS) {
    const double e = mul_rounded((double)t, delta);
    s_edge[t] = mul_rounded(e, e);
  }
  for (int t = threadIdx.x; t < nwords; t += VARIO_THREADS) s_cnt[t] = 0ull;   // +0.0 is all-zero bits
  __syncthreads();
}

// The next work unit (batch I, tiles J0 .. J0 + jw - 1) of this wave: drawn from the global counter, A.grab units per
// atomic; units in the empty half of the triangle are passed over.  false: the counter is exhausted.
__device__ __forceinline__ bool vario_next_unit(const VarioArgs& A, unsigned long long* unit_counter, int lane,
                                                unsigned long long& unext, unsigned long long& uend, int& I, int& J0) {
  const unsigned long long nunits = (unsigned long long)A.nb * (unsigned long long)A.nchunks;
  while (true) {
    if (unext == uend) {
      unsigned long long u0 = 0ull;
      if (lane == 0) u0 = atomicAdd(unit_counter, (unsigned long long)A.grab);
      unext = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u0 >> 32)) << 32) |
              (unsigned)__builtin_amdgcn_readfirstlane((int)u0);
      if (unext >= nunits) return false;
      uend = unext + (unsigned long long)A.grab < nunits ? unext + (unsigned long long)A.grab : nunits;
    }
    const unsigned long long u = unext++;
    I = (int)(u / (unsigned)A.nchunks);
    J0 = (int)(u % (unsigned)A.nchunks) * A.jw;
    if (J0 + A.jw - 1 >= I) return true;   // else: the empty half of the triangle
  }
}

// lanes 0..15: bound of tile (I, J0 + lane), kept in lb; -> the mask of the tiles to open
template <int DIM>
__device__ __forceinline__ unsigned long long vario_cull(const double* __restrict__ blo, const double* __restrict__ bhi,
                                                         const VarioArgs& A, int I, int J0, int lane, double emax2,
                                                         double& lb) {
  const int Jl = J0 + lane;
  bool cand = lane < A.jw && Jl >= I && Jl < A.nb;
  lb = 0.0;
  if (cand) {
    double loa[DIM], hia[DIM], lob[DIM], hib[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      loa[a] = blo[(int64_t)I * DIM + a];
      hia[a] = bhi[(int64_t)I * DIM + a];
      lob[a] = blo[(int64_t)Jl * DIM + a];
      hib[a] = bhi[(int64_t)Jl * DIM + a];
    }
    lb = vario_box_d2<DIM>(loa, hia, lob, hib);
    cand = A.nocull || lb <= emax2;
  }
  return __ballot(cand);
}

// batch J into registers: lane = point (a lane past the end holds a copy of the last point and vj = false)
template <int DIM, int NZ>
__device__ __forceinline__ bool vario_load_j(const double* __restrict__ xs, const double* __restrict__ zs, int64_t n,
                                             int J, int lane, double* xj, double* zj) {
  const int64_t j = (int64_t)J * 64 + lane;
  const bool vj = j < n;
  const int64_t jc = vj ? j : n - 1;
#pragma unroll
  for (int a = 0; a < DIM; ++a) xj[a] = xs[jc * DIM + a];
#pragma unroll
  for (int c = 0; c < NZ; ++c) zj[c] = zs[(int64_t)c * n + jc];
  return vj;
}

// The pair (sample i of batch I: wave uniform, scalar loads; the lane's point): key d2, delta vector dl, duplicates
// counted apart, -> keep.  DIRECTIONAL: with the direction test of gss_variogram_empirical (when A.directional).
template <int DIM, bool DIRECTIONAL>
__device__ __forceinline__ bool vario_pair(const double* __restrict__ xs, int64_t i, const double* xj, bool pairok,
                                           const VarioArgs& A, double emax2, double& d2, double* dl,
                                           unsigned long long& ndup) {
  double xi[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) xi[a] = xs[i * DIM + a];
  d2 = vario_d2<DIM>(xi, xj, dl);
  ndup += (pairok && d2 == 0.0) ? 1ull : 0ull;
  bool keep = pairok && d2 > 0.0 && d2 <= emax2;
  if (DIRECTIONAL && A.directional) {
#pragma clang fp contract(off)
    double t = dl[0] * A.u[0];
    if (DIM > 1) t = t + dl[1] * A.u[1];
    if (DIM > 2) t = t + dl[2] * A.u[2];
    const double tt = t * t;
    const double p2 = d2 - tt;
    const double cd = A.cos2 * d2;
    keep = keep && p2 <= A.dtol2 && tt >= cd;
  }
  return keep;
}

// the wave's counters into the histogram, the histogram into the workgroup's slice
__device__ __forceinline__ void vario_copy_out(unsigned long long* s_cnt, int nbins, int nwords, unsigned long long ndup,
                                               unsigned long long opened, int lane,
                                               unsigned long long* __restrict__ partial) {
  if (ndup) atomicAdd(&s_cnt[nbins], ndup);
  if (lane == 0 && opened) atomicAdd(&s_cnt[nbins + 1], opened);
  __syncthreads();
  unsigned long long* out = partial + (size_t)blockIdx.x * nwords;
  for (int t = threadIdx.x; t < nwords; t += VARIO_THREADS) out[t] = s_cnt[t];
}

// the increments of a pair that the direct estimators sum: dz^2 (Matheron), sqrt|dz| (Cressie-Hawkins)
template <int NZ, bool CRESSIE>
__device__ __forceinline__ void vario_increments(const double* __restrict__ zs, int64_t n, int64_t i, const double* zj,
                                                 double* val) {
#pragma unroll
  for (int c = 0; c < NZ; ++c) {
    const double dz = zs[(int64_t)c * n + i] - zj[c];
    val[c] = CRESSIE ? gss_sqrt(fabs(dz)) : mul_rounded(dz, dz);
  }
}

#define VARIO_KERNEL_ARGS                                                                                             \
  const double* __restrict__ xs,  /* n x DIM, k-d order */                                                            \
      const double* __restrict__ zs,  /* NZ columns of n, k-d order */                                                \
      const double* __restrict__ blo, /* nb x DIM batch boxes */                                                      \
      const double* __restrict__ bhi, VarioArgs A, unsigned long long* __restrict__ unit_counter,                     \
      unsigned long long* __restrict__ partial, /* per workgroup: what is flushed (above) */                          \
      const double* __restrict__ dirs           /* plane: (c_s, s_s), 2 nangles doubles; else unused */

// Lag bins: a register window of VW bins from the bin of the tile's lower bound, LDS atomics beyond it.
template <int DIM, int NZ, bool CRESSIE>
__global__ __launch_bounds__(VARIO_THREADS) void vario_window_kernel(VARIO_KERNEL_ARGS) {
  constexpr int VW = NZ <= 2 ? 6 : 4;   // bins of the register window
  extern __shared__ double smem[];
  const int nlags = A.nlags;
  double* s_edge = smem;                                                  // nlags + 1
  unsigned long long* s_cnt = reinterpret_cast<unsigned long long*>(smem + nlags + 1);   // nlags + 2 (ndup, opened)
  double* s_h = smem + nlags + 1 + nlags + 2;                             // nlags
  double* s_z = s_h + nlags;                                              // NZ * nlags
  const int nwords = (nlags + 2) + nlags + NZ * nlags;
  vario_lds_init(s_edge, s_cnt, nlags, nwords, A.delta);

  const int lane = threadIdx.x & 63;
  const double emax2 = s_edge[nlags];
  const int64_t n = A.n;
  unsigned long long ndup = 0ull, opened = 0ull;

  unsigned long long unext = 0ull, uend = 0ull;
  int I, J0;
  while (vario_next_unit(A, unit_counter, lane, unext, uend, I, J0)) {
    double lb;
    unsigned long long open = vario_cull<DIM>(blo, bhi, A, I, J0, lane, emax2, lb);
    opened += (unsigned long long)__popcll(open);

    const int ni = (int64_t)I * 64 + 64 <= n ? 64 : (int)(n - (int64_t)I * 64);
    while (open) {
      const int pick = __builtin_ctzll(open);
      open &= open - 1;
      const int J = J0 + pick;
      const double lbJ = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lb), pick),
                                          __builtin_amdgcn_readlane(__double2loint(lb), pick));
      // first bin any pair of this tile can fall into (wave uniform)
      int kb = 0;
      if (lbJ > 0.0 && lbJ <= emax2) kb = vario_bin(s_edge, nlags, lbJ, gss_sqrt(lbJ), A.inv_delta);
      kb = __builtin_amdgcn_readfirstlane(kb);
      const bool diag = I == J;
      double xj[DIM], zj[NZ];
      const bool vj = vario_load_j<DIM, NZ>(xs, zs, n, J, lane, xj, zj);

      unsigned int wc[VW];
      double wh[VW], wz[NZ][VW];
#pragma unroll
      for (int w = 0; w < VW; ++w) {
        wc[w] = 0u;
        wh[w] = 0.0;
#pragma unroll
        for (int c = 0; c < NZ; ++c) wz[c][w] = 0.0;
      }
#pragma unroll 2
      for (int ii = 0; ii < ni; ++ii) {
        const int64_t i = (int64_t)I * 64 + ii;
        double d2, dl[DIM];
        const bool keep = vario_pair<DIM, true>(xs, i, xj, vj && (!diag || ii < lane), A, emax2, d2, dl, ndup);
        const double h = gss_sqrt(d2);
        const int k = vario_bin(s_edge, nlags, d2, h, A.inv_delta);
        const int w = keep ? k - kb : -1;
        double val[NZ];
        vario_increments<NZ, CRESSIE>(zs, n, i, zj, val);
#pragma unroll
        for (int s = 0; s < VW; ++s) {
          const bool m = w == s;
          const double mf = m ? 1.0 : 0.0;   // exact selector: fma(1, v, acc) = acc + v rounded once, fma(0, v, acc) = acc
          wc[s] += m ? 1u : 0u;
          wh[s] = fma(mf, h, wh[s]);
#pragma unroll
          for (int c = 0; c < NZ; ++c) wz[c][s] = fma(mf, val[c], wz[c][s]);
        }
        if (keep && (unsigned)w >= (unsigned)VW) {   // beyond the window: straight to the workgroup's histogram
          atomicAdd(&s_cnt[k], 1ull);
          lds_add_f64(&s_h[k], h);
#pragma unroll
          for (int c = 0; c < NZ; ++c) lds_add_f64(&s_z[c * nlags + k], val[c]);
        }
      }
      // flush the window (bins kb .. kb + VW - 1, those that exist)
#pragma unroll
      for (int s = 0; s < VW; ++s) {
        if (wc[s] != 0u) {
          const int k = kb + s;   // wc > 0 only for a real bin
          atomicAdd(&s_cnt[k], (unsigned long long)wc[s]);
          lds_add_f64(&s_h[k], wh[s]);
#pragma unroll
          for (int c = 0; c < NZ; ++c) lds_add_f64(&s_z[c * nlags + k], wz[c][s]);
        }
      }
    }
  }
  vario_copy_out(s_cnt, nlags, nwords, ndup, opened, lane, partial);
}

// Varioplane: bins by (sector, lag).  Every lane keeps the run of consecutive kept pairs that fall into one bin in
// registers and sends it to the histogram when the bin changes and after the tile.  No direction test.
template <int DIM, int NZ, bool CRESSIE>
__global__ __launch_bounds__(VARIO_THREADS) void vario_plane_kernel(VARIO_KERNEL_ARGS) {
  extern __shared__ double smem[];
  const int nlags = A.nlags;
  const int nbins = A.nangles * nlags;                                    // bins of the histogram: (sector, lag)
  double* s_edge = smem;                                                  // nlags + 1
  unsigned long long* s_cnt = reinterpret_cast<unsigned long long*>(smem + nlags + 1);   // nbins + 2 (ndup, opened)
  double* s_h = smem + nlags + 1 + nbins + 2;                             // nbins
  double* s_z = s_h + nbins;                                              // NZ * nbins
  const int nwords = (nbins + 2) + nbins + NZ * nbins;
  double* s_dir = smem + nlags + 1 + nwords;                              // 2 nangles
  for (int t = threadIdx.x; t < 2 * A.nangles; t += VARIO_THREADS) s_dir[t] = dirs[t];
  vario_lds_init(s_edge, s_cnt, nlags, nwords, A.delta);

  const int lane = threadIdx.x & 63;
  const double emax2 = s_edge[nlags];
  const int64_t n = A.n;
  unsigned long long ndup = 0ull, opened = 0ull;

  unsigned long long unext = 0ull, uend = 0ull;
  int I, J0;
  while (vario_next_unit(A, unit_counter, lane, unext, uend, I, J0)) {
    double lb;
    unsigned long long open = vario_cull<DIM>(blo, bhi, A, I, J0, lane, emax2, lb);
    opened += (unsigned long long)__popcll(open);

    const int ni = (int64_t)I * 64 + 64 <= n ? 64 : (int)(n - (int64_t)I * 64);
    while (open) {
      const int pick = __builtin_ctzll(open);
      open &= open - 1;
      const int J = J0 + pick;
      const bool diag = I == J;
      double xj[DIM], zj[NZ];
      const bool vj = vario_load_j<DIM, NZ>(xs, zs, n, J, lane, xj, zj);

      int rb = -1;   // the lane's current run -- its bin, its pairs, its sums
      unsigned int rc = 0u;
      double rh = 0.0, rz[NZ];
#pragma unroll
      for (int c = 0; c < NZ; ++c) rz[c] = 0.0;
#pragma unroll 2
      for (int ii = 0; ii < ni; ++ii) {
        const int64_t i = (int64_t)I * 64 + ii;
        double d2, dl[DIM];
        bool keep = vario_pair<DIM, false>(xs, i, xj, vj && (!diag || ii < lane), A, emax2, d2, dl, ndup);
        const double h = gss_sqrt(d2);
        const int k = vario_bin(s_edge, nlags, d2, h, A.inv_delta);
        double val[NZ];
        vario_increments<NZ, CRESSIE>(zs, n, i, zj, val);
        double a1 = dl[0], a2 = dl[DIM > 1 ? 1 : 0];
        if (DIM == 3) {
          a1 = vario_project(dl, A.e);
          a2 = vario_project(dl, A.e + 3);
          const double wn = vario_project(dl, A.e + 6);
          keep = keep && mul_rounded(wn, wn) <= A.ptol2;
        }
        const int b = vario_sector(s_dir, A.nangles, A.nsteps, a1, a2) * nlags + k;   // < nbins for every pair
        if (keep && b != rb) {   // the bin changes: the run goes to the histogram
          if (rc != 0u) {
            atomicAdd(&s_cnt[rb], (unsigned long long)rc);
            lds_add_f64(&s_h[rb], rh);
#pragma unroll
            for (int c = 0; c < NZ; ++c) lds_add_f64(&s_z[c * nbins + rb], rz[c]);
          }
          rb = b;
          rc = 0u;
          rh = 0.0;
#pragma unroll
          for (int c = 0; c < NZ; ++c) rz[c] = 0.0;
        }
        if (keep) {
          rc += 1u;
          rh += h;
#pragma unroll
          for (int c = 0; c < NZ; ++c) rz[c] += val[c];
        }
      }
      if (rc != 0u) {   // the last run of the tile
        atomicAdd(&s_cnt[rb], (unsigned long long)rc);
        lds_add_f64(&s_h[rb], rh);
#pragma unroll
        for (int c = 0; c < NZ; ++c) lds_add_f64(&s_z[c * nbins + rb], rz[c]);
      }
    }
  }
  vario_copy_out(s_cnt, nbins, nwords, ndup, opened, lane, partial);
}

// Cross-variograms: bins by lag, sums mul_rounded(dz_a, dz_b) for every a <= b (row a NZ - a (a - 1) / 2 + (b - a)).
// Run form like the plane's; the bin is a lag, the same for a lane's whole life, so the run is carried across tiles and
// units and flushed last at the end of the kernel.
template <int DIM, int NZ>
__global__ __launch_bounds__(VARIO_THREADS) void vario_cross_kernel(VARIO_KERNEL_ARGS) {
  constexpr int NP = NZ * (NZ + 1) / 2;
  extern __shared__ double smem[];
  const int nlags = A.nlags;
  double* s_edge = smem;                                                  // nlags + 1
  unsigned long long* s_cnt = reinterpret_cast<unsigned long long*>(smem + nlags + 1);   // nlags + 2 (ndup, opened)
  double* s_h = smem + nlags + 1 + nlags + 2;                             // nlags
  double* s_z = s_h + nlags;                                              // NP * nlags
  const int nwords = (nlags + 2) + nlags + NP * nlags;
  vario_lds_init(s_edge, s_cnt, nlags, nwords, A.delta);

  const int lane = threadIdx.x & 63;
  const double emax2 = s_edge[nlags];
  const int64_t n = A.n;
  unsigned long long ndup = 0ull, opened = 0ull;

  int rb = 0;   // the lane's current run: its bin (valid while rc > 0), its pairs, its sums
  unsigned int rc = 0u;
  double rh = 0.0, rz[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) rz[p] = 0.0;

  unsigned long long unext = 0ull, uend = 0ull;
  int I, J0;
  while (vario_next_unit(A, unit_counter, lane, unext, uend, I, J0)) {
    double lb;
    unsigned long long open = vario_cull<DIM>(blo, bhi, A, I, J0, lane, emax2, lb);
    opened += (unsigned long long)__popcll(open);

    const int ni = (int64_t)I * 64 + 64 <= n ? 64 : (int)(n - (int64_t)I * 64);
    while (open) {
      const int pick = __builtin_ctzll(open);
      open &= open - 1;
      const int J = J0 + pick;
      const bool diag = I == J;
      double xj[DIM], zj[NZ];
      const bool vj = vario_load_j<DIM, NZ>(xs, zs, n, J, lane, xj, zj);

#pragma unroll 2
      for (int ii = 0; ii < ni; ++ii) {
        const int64_t i = (int64_t)I * 64 + ii;
        double d2, dl[DIM];
        const bool keep = vario_pair<DIM, true>(xs, i, xj, vj && (!diag || ii < lane), A, emax2, d2, dl, ndup);
        const double h = gss_sqrt(d2);
        const int k = vario_bin(s_edge, nlags, d2, h, A.inv_delta);   // in 0 .. nlags - 1 for every pair
        // The run is updated without a branch that writes registers (such a branch makes the compiler keep copies of
        // all NP sums): exact 0 / 1 factors select instead.  mf masks the pair: a dropped pair contributes products
        // that are exactly zero; fma(rz, 1, v) = rz + v rounded once.  kf clears the run after it has been sent.
        const bool flush = keep && k != rb && rc != 0u;
        if (flush) {   // the bin changes: the run goes to the histogram
          atomicAdd(&s_cnt[rb], (unsigned long long)rc);
          lds_add_f64(&s_h[rb], rh);
#pragma unroll
          for (int p = 0; p < NP; ++p) lds_add_f64(&s_z[p * nlags + rb], rz[p]);
        }
        const double mf = keep ? 1.0 : 0.0, kf = flush ? 0.0 : 1.0;
        double dz[NZ], dm[NZ];
#pragma unroll
        for (int c = 0; c < NZ; ++c) {
          dz[c] = zs[(int64_t)c * n + i] - zj[c];
          dm[c] = mul_rounded(dz[c], mf);
        }
        rb = keep ? k : rb;
        rc = (flush ? 0u : rc) + (keep ? 1u : 0u);
        rh = fma(rh, kf, keep ? h : 0.0);
        int p = 0;
#pragma unroll
        for (int a = 0; a < NZ; ++a) {
#pragma unroll
          for (int b = a; b < NZ; ++b) {
            rz[p] = fma(rz[p], kf, mul_rounded(dm[a], dz[b]));
            ++p;
          }
        }
      }
    }
  }
  if (rc != 0u) {   // the last run of the lane
    atomicAdd(&s_cnt[rb], (unsigned long long)rc);
    lds_add_f64(&s_h[rb], rh);
#pragma unroll
    for (int p = 0; p < NP; ++p) lds_add_f64(&s_z[p * nlags + rb], rz[p]);
  }
  vario_copy_out(s_cnt, nlags, nwords, ndup, opened, lane, partial);
}

#undef VARIO_KERNEL_ARGS

// Sum of the workgroup slices, one workgroup per output word: thread j adds the slices j, j + 256, ... in ascending
// order, then the 256 partial sums are folded pairwise in a fixed pattern -- the integer totals are exact and the
// floating-point ones depend only on which pairs each workgroup of the pair kernel drew.
__global__ __launch_bounds__(256) void vario_reduce_kernel(const unsigned long long* __restrict__ partial, int nwg,
                                                           int nlags, int nz, int64_t* __restrict__ count,
                                                           double* __restrict__ lagsum, double* __restrict__ zsum,
                                                           int64_t* __restrict__ ndup, int64_t* __restrict__ stats,
                                                           const int* __restrict__ bad) {
  __shared__ unsigned long long su[256];
  __shared__ double sd[256];
  const int nwords = (nlags + 2) + nlags + nz * nlags;
  const int t = blockIdx.x;   // < nwords
  const bool integer = t < nlags + 2;
  unsigned long long au = 0ull;
  double ad = 0.0;
  for (int g = threadIdx.x; g < nwg; g += 256) {
    const unsigned long long v = partial[(size_t)g * nwords + t];
    if (integer) au += v;
    else ad += __longlong_as_double((long long)v);
  }
  su[threadIdx.x] = au;
  sd[threadIdx.x] = ad;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      su[threadIdx.x] += su[threadIdx.x + w];
      sd[threadIdx.x] += sd[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const bool poisoned = *bad != 0;   // a non-finite input: counts and *ndup = -1, sums NaN (gss.h)
  if (integer) {
    if (t < nlags) count[t] = poisoned ? -1 : (int64_t)su[0];
    else if (t == nlags) *ndup = poisoned ? -1 : (int64_t)su[0];
    else stats[0] = (int64_t)su[0];
  } else {
    const double v = poisoned ? __longlong_as_double(0x7ff8000000000000LL) : sd[0];
    const int q = t - (nlags + 2);
    if (q < nlags) lagsum[q] = v;
    else zsum[q - nlags] = v;
  }
}

// *bad is set when a coordinate or a value is not finite (before anything is ordered by them)
__global__ __launch_bounds__(256) void vario_check_kernel(const double* __restrict__ x, const double* __restrict__ z,
                                                          int64_t nx, int64_t nzv, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = (i >= nx || isfinite(x[i])) && (i >= nzv || isfinite(z[i]));
  if (!ok) *bad = 1;
}

// values into the order of the index
__global__ __launch_bounds__(256) void vario_gather_kernel(const double* __restrict__ z, const int* __restrict__ perm,
                                                           int64_t n, int nz, double* __restrict__ zs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = perm[i];
  for (int c = 0; c < nz; ++c) zs[(int64_t)c * n + i] = z[(int64_t)c * n + p];
}

// ---- ordering of small sets: one sort by Morton key ------------------------------------------------------------------
// Below VARIO_KD_MIN samples the level-by-level k-d ordering of the search index (a radix sort and a bounding-box pass
// per level, and a wait for the stream) costs as much as the pair pass itself.  Such a set is ordered by ONE radix sort
// of 30-bit Morton keys on its bounding box instead; the batches of 64 and their boxes are formed from that order in the
// same arrays (KnnIndex xs / perm / lo / hi).  Any order gives the same counts; a compact one keeps a tile's pairs in
// few bins.  Everything is queued on the stream, nothing waits.
constexpr int64_t VARIO_KD_MIN = 32768;

__device__ __forceinline__ unsigned long long vario_f64_key(double v) {   // monotone image of a double
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double vario_key_f64(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// box[0..2] = min, box[3..5] = max as monotone keys; also clears the unit counter and the bad-value flag
__global__ void vario_init_kernel(unsigned long long* __restrict__ box, unsigned long long* __restrict__ flags) {
  if (threadIdx.x < 3) box[threadIdx.x] = ~0ull;
  else if (threadIdx.x < 6) box[threadIdx.x] = 0ull;
  else if (threadIdx.x < 8) flags[threadIdx.x - 6] = 0ull;
}

template <int DIM>
__global__ __launch_bounds__(256) void vario_bbox_kernel(const double* __restrict__ x, int64_t n,
                                                         unsigned long long* __restrict__ box) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ic = i < n ? i : n - 1;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    unsigned long long lo = vario_f64_key(x[ic * DIM + a]), hi = lo;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&box[a], lo);
      atomicMax(&box[3 + a], hi);
    }
  }
}

template <int DIM>
__global__ __launch_bounds__(256) void vario_morton_kernel(const double* __restrict__ x, int64_t n,
                                                           const unsigned long long* __restrict__ box,
                                                           unsigned int* __restrict__ key, int* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  constexpr int BITS = 30 / DIM;
  unsigned int q[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const double lo = vario_key_f64(box[a]), ext = vario_key_f64(box[3 + a]) - lo;
    const double t = ext > 0.0 ? (x[i * DIM + a] - lo) / ext * (double)(1u << BITS) : 0.0;
    q[a] = t >= (double)((1u << BITS) - 1u) ? (1u << BITS) - 1u : (t > 0.0 ? (unsigned int)t : 0u);
  }
  unsigned int k = 0u;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) k |= ((q[a] >> b) & 1u) << (b * DIM + a);
  }
  key[i] = k;
  val[i] = (int)i;
}

// ordered coordinates and the box of every batch of 64: one wave per batch
template <int DIM>
__global__ __launch_bounds__(256) void vario_batches_kernel(const double* __restrict__ x, const int* __restrict__ perm,
                                                            int64_t n, int nb, double* __restrict__ xs,
                                                            double* __restrict__ blo, double* __restrict__ bhi) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= nb) return;   // whole wave
  const int64_t j = (int64_t)b * 64 + lane;
  const int64_t jc = j < n ? j : n - 1;   // a clamped duplicate does not change the box
  const int p = perm[jc];
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const double v = x[(int64_t)p * DIM + a];
    if (j < n) xs[j * DIM + a] = v;
    double lo = v, hi = v;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) {
      blo[(int64_t)b * DIM + a] = lo;
      bhi[(int64_t)b * DIM + a] = hi;
    }
  }
}

template <int DIM>
int32_t vario_morton_index(const double* xdev, int64_t n, unsigned long long* box, KnnIndex* ix, hipStream_t s) {
  const int nb = (int)((n + 63) / 64);
  const dim3 gn((unsigned)((n + 255) / 256));
  DevBuf k0, k1, v0, tmp;
  GSS_TRY(k0.alloc(sizeof(unsigned int) * (size_t)n));
  GSS_TRY(k1.alloc(sizeof(unsigned int) * (size_t)n));
  GSS_TRY(v0.alloc(sizeof(int) * (size_t)n));
  GSS_TRY(ix->perm.alloc(sizeof(int) * (size_t)n));
  GSS_TRY(ix->xs.alloc(sizeof(double) * (size_t)n * DIM));
  GSS_TRY(ix->lo.alloc(sizeof(double) * (size_t)nb * DIM));
  GSS_TRY(ix->hi.alloc(sizeof(double) * (size_t)nb * DIM));
  hipLaunchKernelGGL(vario_bbox_kernel<DIM>, gn, dim3(256), 0, s, xdev, n, box);
  hipLaunchKernelGGL(vario_morton_kernel<DIM>, gn, dim3(256), 0, s, xdev, n, box, k0.as<unsigned int>(), v0.as<int>());
  GSS_HIP(hipGetLastError());
  size_t tb = 0;
  GSS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k0.as<unsigned int>(), k1.as<unsigned int>(), v0.as<int>(),
                                             ix->perm.as<int>(), (int)n, 0, 30, s));
  GSS_TRY(tmp.alloc(tb));
  GSS_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k0.as<unsigned int>(), k1.as<unsigned int>(), v0.as<int>(),
                                             ix->perm.as<int>(), (int)n, 0, 30, s));
  hipLaunchKernelGGL(vario_batches_kernel<DIM>, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, xdev, ix->perm.as<int>(),
                     n, nb, ix->xs.as<double>(), ix->lo.as<double>(), ix->hi.as<double>());
  GSS_HIP(hipGetLastError());
  ix->n = n;
  ix->nb = nb;
  ix->nb1 = 0;
  ix->dim = DIM;
  return GSS_OK;   // (the sort buffers return to the block cache: their re-use is ordered behind this stream)
}

struct VarioPtrs {
  const double *xs, *zs, *lo, *hi;
  unsigned long long *unit_counter, *partial;
  const double* dirs;   // varioplane: sector boundaries (device)
};

// What an entry point asks of the pass: which kernel family, the bins of the histogram (nlags, or nangles nlags), the
// rows of value sums per bin (nz, or nz (nz + 1) / 2 products) and the plane's sector boundaries (a host array), else NULL.
enum { VARIO_LAGS, VARIO_PLANE, VARIO_CROSS };
struct VarioForm {
  int form;
  int64_t nbins;
  int32_t nsum;
  const double* dirs;
};

using VarioKernel = void (*)(const double*, const double*, const double*, const double*, VarioArgs, unsigned long long*,
                             unsigned long long*, const double*);

// (form, dim, nz, estimator) -> the kernel.  Every instantiation: lag bins (dim 1 .. 3, nz 1 .. 8, both estimators),
// plane (dim 2, 3, nz 1 .. 4, both estimators), cross (dim 1 .. 3, nz 1 .. 8); the entry points have checked the ranges.
template <int DIM, int NZ>
VarioKernel vario_kernel_of(int form, bool cressie) {
  if (form == VARIO_CROSS) return vario_cross_kernel<DIM, NZ>;
  if constexpr (DIM >= 2 && NZ <= VARIO_PLANE_MAX_NZ) {
    if (form == VARIO_PLANE)
      return cressie ? vario_plane_kernel<DIM, NZ, true> : vario_plane_kernel<DIM, NZ, false>;
  }
  return cressie ? vario_window_kernel<DIM, NZ, true> : vario_window_kernel<DIM, NZ, false>;
}

template <int DIM>
VarioKernel vario_kernel_nz(int form, int nz, bool cressie) {
  switch (nz) {
    case 1: return vario_kernel_of<DIM, 1>(form, cressie);
    case 2: return vario_kernel_of<DIM, 2>(form, cressie);
    case 3: return vario_kernel_of<DIM, 3>(form, cressie);
    case 4: return vario_kernel_of<DIM, 4>(form, cressie);
    case 5: return vario_kernel_of<DIM, 5>(form, cressie);
    case 6: return vario_kernel_of<DIM, 6>(form, cressie);
    case 7: return vario_kernel_of<DIM, 7>(form, cressie);
    default: return vario_kernel_of<DIM, 8>(form, cressie);
  }
}

VarioKernel vario_kernel(int form, int dim, int nz, int estimator) {
  const bool cressie = estimator == GSS_VARIO_CRESSIE;
  switch (dim) {
    case 1: return vario_kernel_nz<1>(form, nz, cressie);
    case 2: return vario_kernel_nz<2>(form, nz, cressie);
    default: return vario_kernel_nz<3>(form, nz, cressie);
  }
}

// nwg == 0: *resident = workgroups of this kernel that fit one CU at a time (nothing is launched).  big: the histogram
// may pass the 64 KiB a kernel gets without asking (plane: up to VARIO_PLANE_MAX_WORDS; cross: from NP nlags > ~7 900;
// lag bins alone never: 22 KiB at most).
int32_t vario_launch(VarioKernel kernel, bool big, const VarioPtrs& P, const VarioArgs& A, int nwg, size_t lds,
                     hipStream_t s, int* resident) {
  if (nwg == 0) {
    if (big)
      GSS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
    GSS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(resident, kernel, VARIO_THREADS, lds));
    return GSS_OK;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)nwg), dim3(VARIO_THREADS), lds, s, P.xs, P.zs, P.lo, P.hi, A,
                     P.unit_counter, P.partial, P.dirs);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// tile counters of the last call: written by the reduction into page-locked memory, read after the event
int64_t* g_vario_stats = nullptr;   // [0] tiles opened
hipEvent_t g_vario_event = nullptr;
int64_t g_vario_tiles_total = 0;
bool g_vario_pending = false;

}  // namespace

int32_t vario_stat(const char* name, int64_t* value) {
  if (!std::strcmp(name, "vario_tiles_total")) {
    *value = g_vario_tiles_total;
    return GSS_OK;
  }
  if (!std::strcmp(name, "vario_tiles_opened")) {
    if (g_vario_pending) {
      GSS_HIP(hipEventSynchronize(g_vario_event));
      g_vario_pending = false;
    }
    *value = g_vario_stats ? g_vario_stats[0] : 0;
    return GSS_OK;
  }
  return -1;
}

}  // namespace gss

using namespace gss;

namespace {

// The pass over the pairs that gss_variogram_empirical, gss_variogram_plane and gss_variogram_cross share: checks of
// the common arguments, staging, the finite-input check, the ordering, the gather, the grid, the pair kernel, the
// reduction and the way home.  A: what the caller has filled in of the kernel's arguments (direction or sectors).
int32_t vario_run(const char* who, const double* x, int64_t n, int32_t dim, const double* z, int32_t nz,
                  int32_t nlags, double maxlag, int32_t estimator, VarioArgs& A, const VarioForm& F, int64_t* count,
                  double* lagsum, double* zsum, int64_t* nduplicates, int32_t mem, void* stream) {
  const int64_t nbins = F.nbins;
  const int32_t nsum = F.nsum;
  // squared bin edges edge2[k] = fl(fl(k delta)^2): the kernel forms the same doubles; only the ends are checked here
  const double delta = maxlag / (double)nlags;
  {
    volatile double e1 = delta * delta, en = (double)nlags * delta;
    volatile double en2 = en * en;
    GSS_REQUIRE(e1 > 0.0 && std::isfinite(en2), "%s: maxlag^2 leaves the range of a double", who);
  }

  hipStream_t s = to_stream(stream);
  Staged sx, sz, scount, slag, szsum, sdup, sdirs;
  GSS_TRY(sx.in(x, sizeof(double) * (size_t)n * dim, mem, s));
  GSS_TRY(sz.in(z, sizeof(double) * (size_t)n * nz, mem, s));
  DevBuf zs, flags, partial;
  GSS_TRY(zs.alloc(sizeof(double) * (size_t)n * nz));
  GSS_TRY(flags.alloc(sizeof(unsigned long long) * 8));   // [0] unit counter, [1] bad-value flag, [2..7] bounding box
  unsigned long long* d_flags = flags.as<unsigned long long>();
  int* d_bad = reinterpret_cast<int*>(d_flags + 1);
  hipLaunchKernelGGL(vario_init_kernel, dim3(1), dim3(64), 0, s, d_flags + 2, d_flags);
  {
    const int64_t nx = n * dim, nzv = n * nz, nmax = nx > nzv ? nx : nzv;
    hipLaunchKernelGGL(vario_check_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, sx.as<double>(),
                       sz.as<double>(), nx, nzv, d_bad);
  }
  GSS_HIP(hipGetLastError());
  KnnIndex ix;
  if (n >= VARIO_KD_MIN) {
    GSS_TRY(knn_index_build_device(sx.as<double>(), n, dim, &ix, s));   // the Searcher's k-d order; waits for s once
  } else {
    switch (dim) {
      case 1: GSS_TRY(vario_morton_index<1>(sx.as<double>(), n, d_flags + 2, &ix, s)); break;
      case 2: GSS_TRY(vario_morton_index<2>(sx.as<double>(), n, d_flags + 2, &ix, s)); break;
      default: GSS_TRY(vario_morton_index<3>(sx.as<double>(), n, d_flags + 2, &ix, s)); break;
    }
  }
  hipLaunchKernelGGL(vario_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sz.as<double>(),
                     ix.perm.as<int>(), n, (int)nz, zs.as<double>());
  GSS_HIP(hipGetLastError());

  int dev = 0, ncu = 0;
  GSS_HIP(hipGetDevice(&dev));
  GSS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  VarioPtrs P;
  P.xs = ix.xs.as<double>();
  P.zs = zs.as<double>();
  P.lo = ix.lo.as<double>();
  P.hi = ix.hi.as<double>();
  P.dirs = nullptr;
  if (F.dirs) {   // the sector boundaries: a host array in both memory modes
    GSS_TRY(sdirs.in(F.dirs, sizeof(double) * 2 * (size_t)A.nangles, GSS_MEM_HOST, s));
    P.dirs = sdirs.as<double>();
  }
  A.n = n;
  A.nb = ix.nb;
  A.jw = ix.nb < 512 ? 4 : VARIO_JW_MAX;   // below ~32 000 samples 16-tile units are too few to fill the device
  A.nchunks = (ix.nb + A.jw - 1) / A.jw;
  A.nlags = nlags;
  {
    const char* e = std::getenv("GSS_VARIO_CULL");   // "0": open every tile (tests: results do not depend on it)
    A.nocull = e && e[0] == '0';
  }
  A.delta = delta;
  A.inv_delta = 1.0 / delta;
  P.unit_counter = d_flags;
  const size_t nwords = (size_t)(nbins + 2) + nbins + (size_t)nsum * nbins;
  const size_t lds = sizeof(double) * ((size_t)nlags + 1 + nwords + (F.dirs ? 2 * (size_t)A.nangles : 0));
  const VarioKernel kernel = vario_kernel(F.form, dim, nz, estimator);
  // the grid: as many workgroups as are resident at a time for this instantiation (registers and LDS decide: 6 per CU
  // for one value column, 2 for eight), fewer when there are not two units per wave; a workgroup beyond that would only
  // start once the others have emptied the counter
  int resident = 0;
  GSS_TRY(vario_launch(kernel, F.form != VARIO_LAGS, P, A, 0, lds, s, &resident));
  if (resident < 1) resident = 1;
  const int64_t nunits = (int64_t)A.nb * A.nchunks;
  const int64_t want = (nunits + 7) / 8, cap = (int64_t)ncu * resident;
  const int nwg = (int)(want < 1 ? 1 : (want > cap ? cap : want));
  {
    const int64_t g = nunits / ((int64_t)nwg * 4 * 32);   // at least 32 draws per wave
    A.grab = (int)(g < 1 ? 1 : (g > 64 ? 64 : g));
  }
  GSS_TRY(partial.alloc(sizeof(unsigned long long) * nwords * (size_t)nwg));
  P.partial = partial.as<unsigned long long>();

  GSS_TRY(scount.out(count, sizeof(int64_t) * nbins, mem));
  GSS_TRY(slag.out(lagsum, sizeof(double) * nbins, mem));
  GSS_TRY(szsum.out(zsum, sizeof(double) * nbins * nsum, mem));
  GSS_TRY(sdup.out(nduplicates, sizeof(int64_t), mem));
  if (!g_vario_stats) {
    GSS_HIP(hipHostMalloc(reinterpret_cast<void**>(&g_vario_stats), 2 * sizeof(int64_t), hipHostMallocDefault));
    g_vario_stats[0] = g_vario_stats[1] = 0;
    GSS_HIP(hipEventCreateWithFlags(&g_vario_event, hipEventDisableTiming));
  }
  {
    static const char* const scope[] = {"vario_pairs", "vario_plane", "vario_cross"};   // by form
    ProfScope prof(scope[F.form], s);
    GSS_TRY(vario_launch(kernel, false, P, A, nwg, lds, s, nullptr));
  }
  // (a histogram of nbins bins is reduced as one of nbins lags: sector s of the plane at s * nlags)
  hipLaunchKernelGGL(vario_reduce_kernel, dim3((unsigned)nwords), dim3(256), 0, s, P.partial, nwg,
                     (int)nbins, (int)nsum, scount.as<int64_t>(), slag.as<double>(), szsum.as<double>(),
                     sdup.as<int64_t>(), g_vario_stats, d_bad);
  GSS_HIP(hipGetLastError());
  GSS_HIP(hipEventRecord(g_vario_event, s));
  g_vario_pending = true;
  g_vario_tiles_total = (int64_t)A.nb * ((int64_t)A.nb + 1) / 2;
  // (the index, the ordered values and the slices are scratch: released into the block cache, whose re-use is ordered
  //  behind this call by the stream chain)
  if (mem == GSS_MEM_HOST) {
    GSS_HIP(hipMemcpyAsync(count, scount.p, sizeof(int64_t) * nbins, hipMemcpyDeviceToHost, s));
    GSS_HIP(hipMemcpyAsync(lagsum, slag.p, sizeof(double) * nbins, hipMemcpyDeviceToHost, s));
    GSS_HIP(hipMemcpyAsync(zsum, szsum.p, sizeof(double) * nbins * nsum, hipMemcpyDeviceToHost, s));
    GSS_HIP(hipMemcpyAsync(nduplicates, sdup.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
    // a non-finite input is found on the device and reported through the outputs (gss.h); here they have arrived
    GSS_REQUIRE(*nduplicates >= 0, "%s: a coordinate or a value is NaN or infinite (missing values "
                "are dropped by the caller: a pair takes part only if both of its values exist)", who);
  }
  return GSS_OK;
}

// the arguments the two calls share, checked before anything touches the device
int32_t vario_check_args(const char* who, const double* x, int64_t n, int32_t dim, int32_t mindim, const double* z,
                         int32_t nz, int32_t maxnz, int32_t nlags, double maxlag, int32_t estimator,
                         const int64_t* count, const double* lagsum, const double* zsum, const int64_t* nduplicates,
                         int32_t mem) {
  GSS_REQUIRE(x != nullptr && z != nullptr && count != nullptr && lagsum != nullptr && zsum != nullptr &&
                  nduplicates != nullptr, "%s: NULL argument", who);
  GSS_REQUIRE(dim >= mindim && dim <= 3, "%s: dim %d outside %d..3", who, dim, mindim);
  GSS_REQUIRE(n >= 2 && n < (int64_t)INT32_MAX, "%s: n = %lld samples (2 .. 2^31 - 2)", who, (long long)n);
  GSS_REQUIRE(nz >= 1 && nz <= maxnz, "%s: nz %d outside 1..%d", who, nz, maxnz);
  GSS_REQUIRE(nlags >= 1 && nlags <= VARIO_MAX_LAGS, "%s: nlags %d outside 1..%d", who, nlags, VARIO_MAX_LAGS);
  GSS_REQUIRE(std::isfinite(maxlag) && maxlag > 0.0, "%s: maxlag must be positive and finite", who);
  GSS_REQUIRE(estimator == GSS_VARIO_MATHERON || estimator == GSS_VARIO_CRESSIE, "%s: unknown estimator %d", who,
              estimator);
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "%s: bad mem %d", who, mem);
  return GSS_OK;
}

// the direction test of gss_variogram_empirical and gss_variogram_cross into the kernel's arguments (A is cleared first)
int32_t vario_direction(const char* who, int32_t dim, const double* direction, double dtol, double cos_atol,
                        VarioArgs& A) {
  std::memset(&A, 0, sizeof(A));
  A.dtol2 = __builtin_huge_val();
  if (direction == nullptr) return GSS_OK;
  // the direction is a HOST array of `dim` doubles in both memory modes (it is a parameter, not data)
  double nn = 0.0;
  for (int a = 0; a < dim; ++a) {
    GSS_REQUIRE(std::isfinite(direction[a]), "%s: direction is not finite", who);
    nn += direction[a] * direction[a];
    A.u[a] = direction[a];
  }
  GSS_REQUIRE(std::fabs(std::sqrt(nn) - 1.0) <= 1e-12, "%s: direction is not a unit vector (norm %.17g)", who,
              std::sqrt(nn));
  GSS_REQUIRE(dtol > 0.0 && !std::isnan(dtol), "%s: dtol must be positive (+inf: no band)", who);
  GSS_REQUIRE(cos_atol >= 0.0 && cos_atol <= 1.0, "%s: cos_atol outside [0, 1]", who);
  A.directional = 1;
  A.dtol2 = dtol * dtol;
  A.cos2 = cos_atol * cos_atol;
  return GSS_OK;
}

}  // namespace

extern "C" int32_t gss_variogram_empirical(const double* x, int64_t n, int32_t dim, const double* z, int32_t nz,
                                           int32_t nlags, double maxlag, const double* direction, double dtol,
                                           double cos_atol, int32_t estimator, int64_t* count, double* lagsum,
                                           double* zsum, int64_t* nduplicates, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_TRY(vario_check_args("gss_variogram_empirical", x, n, dim, 1, z, nz, VARIO_MAX_NZ, nlags, maxlag, estimator, count,
                           lagsum, zsum, nduplicates, mem));
  VarioArgs A;
  GSS_TRY(vario_direction("gss_variogram_empirical", dim, direction, dtol, cos_atol, A));
  return vario_run("gss_variogram_empirical", x, n, dim, z, nz, nlags, maxlag, estimator, A,
                   VarioForm{VARIO_LAGS, nlags, nz, nullptr}, count, lagsum, zsum, nduplicates, mem, stream);
}

extern "C" int32_t gss_variogram_cross(const double* x, int64_t n, int32_t dim, const double* z, int32_t nz,
                                       int32_t nlags, double maxlag, const double* direction, double dtol,
                                       double cos_atol, int64_t* count, double* lagsum, double* csum,
                                       int64_t* nduplicates, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_TRY(vario_check_args("gss_variogram_cross", x, n, dim, 1, z, nz, VARIO_MAX_NZ, nlags, maxlag, GSS_VARIO_MATHERON,
                           count, lagsum, csum, nduplicates, mem));
  VarioArgs A;
  GSS_TRY(vario_direction("gss_variogram_cross", dim, direction, dtol, cos_atol, A));
  return vario_run("gss_variogram_cross", x, n, dim, z, nz, nlags, maxlag, GSS_VARIO_MATHERON, A,
                   VarioForm{VARIO_CROSS, nlags, nz * (nz + 1) / 2, nullptr}, count, lagsum, csum, nduplicates, mem,
                   stream);
}

extern "C" int32_t gss_variogram_plane(const double* x, int64_t n, int32_t dim, const double* z, int32_t nz,
                                       int32_t nlags, double maxlag, int32_t nangles, const double* dirs,
                                       const double* basis, double ptol, int32_t estimator, int64_t* count,
                                       double* lagsum, double* zsum, int64_t* nduplicates, int32_t mem, void* stream) {
  GSS_ENTRY();
  const char* who = "gss_variogram_plane";
  GSS_REQUIRE(dim != 1, "gss_variogram_plane: dim 1 has no directions (a plane needs dim 2 or 3)");
  GSS_TRY(vario_check_args(who, x, n, dim, 2, z, nz, VARIO_PLANE_MAX_NZ, nlags, maxlag, estimator, count, lagsum, zsum,
                           nduplicates, mem));
  GSS_REQUIRE(dirs != nullptr, "gss_variogram_plane: NULL argument (dirs)");
  GSS_REQUIRE(nangles >= 2 && nangles <= VARIO_PLANE_MAX_ANGLES, "gss_variogram_plane: nangles %d outside 2..%d", nangles,
              VARIO_PLANE_MAX_ANGLES);
  GSS_REQUIRE((int64_t)nangles * nlags * (2 + nz) <= VARIO_PLANE_MAX_WORDS,
              "gss_variogram_plane: nangles * nlags * (2 + nz) = %lld exceeds the limit of %d histogram words (split the "
              "value columns or the lags over several calls)", (long long)nangles * nlags * (2 + nz),
              VARIO_PLANE_MAX_WORDS);
  // sector boundaries: unit vectors whose angles increase strictly, each step and the whole span by less than pi
  // (cross and dot product of neighbours give the step's angle in (0, pi); the steps add up to the span)
  double span = 0.0;
  for (int a = 0; a < nangles; ++a) {
    const double c = dirs[2 * a], sn = dirs[2 * a + 1];
    GSS_REQUIRE(std::isfinite(c) && std::isfinite(sn) && std::fabs(std::sqrt(c * c + sn * sn) - 1.0) <= 1e-12,
                "gss_variogram_plane: dirs[%d] is not a unit vector", a);
    if (a == 0) continue;
    const double cross = dirs[2 * a - 2] * sn - dirs[2 * a - 1] * c, dot = dirs[2 * a - 2] * c + dirs[2 * a - 1] * sn;
    GSS_REQUIRE(cross > 0.0, "gss_variogram_plane: the angles of dirs are not strictly increasing (sector %d)", a);
    span += std::atan2(cross, dot);
  }
  GSS_REQUIRE(span < 3.14159265358979323846, "gss_variogram_plane: dirs span %.17g radians: the sectors partition a "
              "half-circle, theta_last - theta_0 < pi", span);
  VarioArgs A;
  std::memset(&A, 0, sizeof(A));
  A.dtol2 = __builtin_huge_val();
  A.nangles = nangles;
  A.nsteps = 0;
  while ((1 << A.nsteps) < nangles) ++A.nsteps;
  A.ptol2 = __builtin_huge_val();
  if (dim == 2) {
    GSS_REQUIRE(basis == nullptr, "gss_variogram_plane: basis must be NULL for dim 2 (the plane is the plane of the "
                "samples)");
  } else {
    GSS_REQUIRE(basis != nullptr, "gss_variogram_plane: dim 3 needs a basis (e1, e2 and the normal of the plane)");
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b <= a; ++b) {
        double d = 0.0;
        for (int k = 0; k < 3; ++k) d += basis[3 * a + k] * basis[3 * b + k];
        GSS_REQUIRE(std::isfinite(d) && std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-12,
                    "gss_variogram_plane: basis is not orthonormal (vectors %d and %d: %.17g)", b, a, d);
      }
    }
    for (int k = 0; k < 9; ++k) A.e[k] = basis[k];
    GSS_REQUIRE(ptol > 0.0 && !std::isnan(ptol), "gss_variogram_plane: ptol must be positive (+inf: no slab)");
    volatile double p2 = ptol * ptol;
    A.ptol2 = p2;
  }
  return vario_run(who, x, n, dim, z, nz, nlags, maxlag, estimator, A,
                   VarioForm{VARIO_PLANE, (int64_t)nangles * nlags, nz, dirs}, count, lagsum, zsum, nduplicates, mem,
                   stream);
}

// gss_shutdown: the page-locked tile counter and its event
void gss::vario_release() {
  if (g_vario_event) (void)hipEventDestroy(g_vario_event);
  if (g_vario_stats) (void)hipHostFree(g_vario_stats);
  g_vario_event = nullptr;
  g_vario_stats = nullptr;
  g_vario_pending = false;
}
