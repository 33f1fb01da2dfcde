// Declustering weights (gss.h "declustering"): cell declustering on one grid, the GSLIB sweep over
// cell sizes and origin offsets, and polygonal declustering by discretisation.
//
// Cell counts are sort-and-count work.  A batch of grids is done at once: every (grid, sample) pair gets the key
// (batch-local grid number, cell of the sample on that grid) and the sample index as value, one hipCUB radix sort brings
// equal cells of one grid together, and the rest is four thin kernels over the sorted array:
//   heads    h[p] = p where the key differs from the one before, 0 elsewhere; the heads of each grid are counted
//            (occupied cells; integer atomics, aggregated per wave)
//   scan     start[p] = max(h[0 .. p]): where the run of p begins (hipCUB inclusive scan)
//   runs     the last element of a run writes its length at the run's start
//   scatter  count[grid][sample] = length of the run the pair sits in
// The key only carries the bits it needs: per axis the width of the largest index any grid of the batch reaches, and
// above them the width of the batch's grid number; the sort runs over exactly those bits.  A batch never exceeds
// DECLUS_BATCH_ITEMS pairs (36 bytes of scratch each, from the block pool), so the working memory does not grow with
// the number of grids.  Everything that rounds happens per sample in an order fixed by (size, offset) alone -- the sum of
// a size's weights is carried from batch to batch in ascending offset -- so the batching changes no bit.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gss_internal.h"

#include <hipcub/hipcub.hpp>

using namespace gss;

namespace {

constexpr double DECLUS_MAX_INDEX = 2097152.0;                // 2^21: three axes fit 63 bits
constexpr int64_t DECLUS_BATCH_ITEMS = (int64_t)1 << 24;      // (grid, sample) pairs sorted at a time
constexpr int64_t DECLUS_QUERY_CHUNK = (int64_t)1 << 22;      // lattice points searched at a time (96 MiB of centres)
constexpr int DECLUS_SUM_ITEMS = 2048;                        // samples per block of the weighted-mean reduction

struct DeclusGrid {
  double o[3], s[3];
};

// The cell of x along one axis (gss.h): one subtraction, one IEEE division, floor.  Host and device evaluate exactly
// this; the host only at the two ends of the data's box, which bound every sample's index because each step is monotone.
__host__ __device__ __forceinline__ double declus_cell(double x, double o, double s) {
#pragma clang fp contract(off)
  const double d = x - o;
  const double q = d / s;
  return floor(q);
}

// order-preserving image of a double (a < b <=> key(a) < key(b); -0 below +0), the same on the host and the device
__host__ __device__ __forceinline__ unsigned long long declus_f64_key(double v) {
  unsigned long long b;
  __builtin_memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double declus_key_f64(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------------------------------
// out[0..2] = ~0, out[3..6] = 0: the box of declus_bounds_kernel before any sample
__global__ void declus_bounds_init_kernel(unsigned long long* out) {
  if (threadIdx.x < 7) out[threadIdx.x] = threadIdx.x < 3 ? ~0ull : 0ull;
}

// out[a] = key of the smallest coordinate along axis a, out[3 + a] of the largest, out[6] != 0: a non-finite value
template <int DIM>
__global__ __launch_bounds__(256) void declus_bounds_kernel(const double* __restrict__ x, int64_t n,
                                                            unsigned long long* __restrict__ out) {
  unsigned long long lo[DIM], hi[DIM];
  unsigned long long bad = 0ull;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    lo[a] = ~0ull;
    hi[a] = 0ull;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const double v = x[i * DIM + a];
      if (!(fabs(v) <= DBL_MAX)) bad = 1ull;
      const unsigned long long k = declus_f64_key(v);
      lo[a] = k < lo[a] ? k : lo[a];
      hi[a] = k > hi[a] ? k : hi[a];
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const unsigned long long l2 = __shfl_xor(lo[a], o), h2 = __shfl_xor(hi[a], o);
      lo[a] = l2 < lo[a] ? l2 : lo[a];
      hi[a] = h2 > hi[a] ? h2 : hi[a];
    }
    bad |= __shfl_xor(bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      atomicMin(&out[a], lo[a]);
      atomicMax(&out[3 + a], hi[a]);
    }
    if (bad) atomicMax(&out[6], 1ull);
  }
}

// key[g n + i] = (g, cell of sample i on grid g), val = i; blockIdx.y = g.  b0 / b1 / b2: key bits of the axes.  An index
// is masked to its width: the host has checked the widths against the box of the data, and the mask keeps a key's grid
// number intact whatever a coordinate holds.
template <int DIM>
__global__ __launch_bounds__(256) void declus_keys_kernel(const double* __restrict__ x, int64_t n,
                                                          const DeclusGrid* __restrict__ grids, int b0, int b1, int b2,
                                                          unsigned long long* __restrict__ key, int* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int g = blockIdx.y;
  const DeclusGrid G = grids[g];
  const int bits[3] = {b0, b1, b2};
  unsigned long long cell = 0ull;
  int shift = 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const unsigned long long ia = (unsigned long long)(long long)declus_cell(x[i * DIM + a], G.o[a], G.s[a]);
    cell |= (ia & ((1ull << bits[a]) - 1ull)) << shift;
    shift += bits[a];
  }
  const unsigned long long hi = shift < 64 ? ((unsigned long long)g << shift) : 0ull;   // (shift == 64 only with g == 0)
  key[(int64_t)g * n + i] = hi | cell;
  val[(int64_t)g * n + i] = (int)i;
}

// h[p] = p at the first element of a run of equal keys, 0 elsewhere; nocc[g] += heads of grid g = key >> cb
__global__ __launch_bounds__(256) void declus_heads_kernel(const unsigned long long* __restrict__ key, int64_t N, int cb,
                                                           int* __restrict__ h, unsigned int* __restrict__ nocc) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < N;
  const int64_t pc = live ? p : N - 1;
  const unsigned long long k = key[pc];
  const bool head = live && (pc == 0 || key[pc - 1] != k);
  if (live) h[p] = head ? (int)p : 0;
  const int g = cb < 64 ? (int)(k >> cb) : 0;
  const int g0 = __builtin_amdgcn_readfirstlane(g);
  if (__all(g == g0)) {   // all but the waves that straddle two grids: one atomic per wave
    const unsigned long long m = __ballot(head);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&nocc[g0], (unsigned int)__popcll(m));
  } else if (head) {
    atomicAdd(&nocc[g], 1u);
  }
}

// the last element of a run writes the run's length at the run's start (one writer per run)
__global__ __launch_bounds__(256) void declus_runs_kernel(const unsigned long long* __restrict__ key,
                                                          const int* __restrict__ start, int64_t N,
                                                          int* __restrict__ runlen) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  if (p == N - 1 || key[p + 1] != key[p]) {
    const int s0 = start[p];
    runlen[s0] = (int)(p - s0) + 1;
  }
}

// count[g n + sample] = length of the run the pair sits in
__global__ __launch_bounds__(256) void declus_scatter_kernel(const unsigned long long* __restrict__ key,
                                                             const int* __restrict__ val, const int* __restrict__ start,
                                                             const int* __restrict__ runlen, int64_t N, int cb, int64_t n,
                                                             int* __restrict__ count) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  const int64_t g = cb < 64 ? (int64_t)(key[p] >> cb) : 0;
  count[g * n + val[p]] = runlen[start[p]];
}

// The grids k0 .. k0 + ng - 1 of one size, in ascending offset: acc_i += n / (noccupied_k count_ik), the integer product
// exact in 64 bits.  first: the size begins here (acc starts at 0); last: it ends here and w_i = acc_i / noff.
__global__ __launch_bounds__(256) void declus_accum_kernel(const int* __restrict__ count,
                                                           const unsigned int* __restrict__ nocc, int ng, int64_t n,
                                                           int first, int last, int noff, double* __restrict__ acc,
                                                           double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double a = first ? 0.0 : acc[i];
  for (int g = 0; g < ng; ++g) {
    const long long prod = (long long)nocc[g] * (long long)count[(int64_t)g * n + i];
    a = a + (double)n / (double)prod;
  }
  if (last) w[i] = a / (double)noff;
  else acc[i] = a;
}

// sum over 256 threads in a fixed tree; the result in thread 0
__device__ __forceinline__ double declus_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) lds[threadIdx.x] = lds[threadIdx.x] + lds[threadIdx.x + o];
    __syncthreads();
  }
  return lds[0];
}

// partial[b] = sum of w_i z_i over samples b 2048 .. b 2048 + 2047: each thread its eight in ascending order, then the
// tree.  The shape depends on n alone, so the sum is the same bits from call to call and from batching to batching.
__global__ __launch_bounds__(256) void declus_wsum_kernel(const double* __restrict__ w, const double* __restrict__ z,
                                                          int64_t n, double* __restrict__ partial) {
  __shared__ double lds[256];
  const int64_t base = (int64_t)blockIdx.x * DECLUS_SUM_ITEMS;
  double a = 0.0;
  for (int j = 0; j < DECLUS_SUM_ITEMS / 256; ++j) {
    const int64_t i = base + threadIdx.x + 256 * j;
    if (i < n) a = a + mul_rounded(w[i], z[i]);
  }
  const double t = declus_block_sum(a, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// *out = (sum of the partial sums, thread t taking t, t + 256, ... in order, then the tree) / n; one block
__global__ __launch_bounds__(256) void declus_wsum_final_kernel(const double* __restrict__ partial, int64_t nblk,
                                                                int64_t n, double* __restrict__ out) {
  __shared__ double lds[256];
  double a = 0.0;
  for (int64_t b = threadIdx.x; b < nblk; b += 256) a = a + partial[b];
  const double t = declus_block_sum(a, lds);
  if (threadIdx.x == 0) *out = t / (double)n;
}

// centres j0 .. j0 + m - 1 of the lattice, axis 0 fastest: lo_a + (j_a + 1/2) step_a, product and sum rounded apart
template <int DIM>
__global__ __launch_bounds__(256) void declus_queries_kernel(double l0, double l1, double l2, double s0, double s1,
                                                             double s2, int64_t d0, int64_t d1, int64_t j0, int64_t m,
                                                             double* __restrict__ q) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  const double lo[3] = {l0, l1, l2}, st[3] = {s0, s1, s2};
  int64_t j = j0 + t, ja[3];
  ja[0] = DIM > 1 ? j % d0 : j;
  j = DIM > 1 ? j / d0 : 0;
  ja[1] = DIM > 2 ? j % d1 : j;
  ja[2] = DIM > 2 ? j / d1 : 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const double c = ((double)ja[a] + 0.5) * st[a];
    q[t * DIM + a] = lo[a] + c;
  }
}

__global__ __launch_bounds__(256) void declus_hits_kernel(const int* __restrict__ idx, int64_t m, int64_t n,
                                                          unsigned long long* __restrict__ hits) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  const int64_t i = idx[t];
  if (i >= 0 && i < n) atomicAdd(&hits[i], 1ull);   // (a plain nearest-neighbour query always names a sample)
}

// w_i = n hits_i / M (the product in FP64: exact below 2^53); *nzero += samples without a hit
__global__ __launch_bounds__(256) void declus_hit_weights_kernel(const unsigned long long* __restrict__ hits, int64_t n,
                                                                 double M, double* __restrict__ w,
                                                                 unsigned long long* __restrict__ nzero) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const unsigned long long h = live ? hits[i] : 1ull;
  if (live) w[i] = mul_rounded((double)n, (double)h) / M;
  const unsigned long long m = __ballot(h == 0ull);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(nzero, (unsigned long long)__popcll(m));
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

struct Box {
  double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
  bool bad = false;   // a non-finite value
};

void box_host(const double* x, int64_t n, int dim, Box* b) {
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < dim; ++a) {
      const double v = x[i * dim + a];
      if (!(std::fabs(v) <= DBL_MAX)) b->bad = true;
      const unsigned long long k = declus_f64_key(v);
      lo[a] = std::min(lo[a], k);
      hi[a] = std::max(hi[a], k);
    }
  for (int a = 0; a < dim; ++a) {
    b->lo[a] = declus_key_f64(lo[a]);
    b->hi[a] = declus_key_f64(hi[a]);
  }
}

// the same for a device array; waits for the stream
int32_t box_device(const double* x, int64_t n, int dim, Box* b, hipStream_t s) {
  DevBuf out;
  GSS_TRY(out.alloc(sizeof(unsigned long long) * 7));
  unsigned long long* o = out.as<unsigned long long>();
  hipLaunchKernelGGL(declus_bounds_init_kernel, dim3(1), dim3(64), 0, s, o);
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 4096));
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL(declus_bounds_kernel<decltype(D)::value>, grid, dim3(256), 0, s, x, n, o);
  });
  GSS_HIP(hipGetLastError());
  unsigned long long h[7];
  GSS_HIP(hipMemcpyAsync(h, o, sizeof(h), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  for (int a = 0; a < dim; ++a) {
    b->lo[a] = declus_key_f64(h[a]);
    b->hi[a] = declus_key_f64(h[3 + a]);
  }
  b->bad = h[6] != 0ull;
  return GSS_OK;
}

// The indices the box of the data reaches on grid g must lie in [0, 2^21); bits[a] is raised to the width of the largest.
// what: "size 3, offset 2" or "the grid"
int32_t grid_check(const char* fn, const char* what, const DeclusGrid& g, const Box& b, int dim, int* bits) {
  for (int a = 0; a < dim; ++a) {
    const double imin = declus_cell(b.lo[a], g.o[a], g.s[a]), imax = declus_cell(b.hi[a], g.o[a], g.s[a]);
    GSS_REQUIRE(imin >= 0.0 && imax < DECLUS_MAX_INDEX,
                "%s: the cell indices along axis %d run from %.17g to %.17g on %s (sides %g): they must lie in [0, 2^21)",
                fn, a, imin, imax, what, g.s[a]);
    int w = 0;
    while ((double)(1ll << w) <= imax) ++w;
    bits[a] = std::max(bits[a], w);
  }
  return GSS_OK;
}

int64_t chunk_grids_cap() {
  if (const char* e = std::getenv("GSS_DECLUS_CHUNK_GRIDS")) {   // tests: more than one batch at a small size
    const long long v = std::atoll(e);
    if (v > 0) return v;
  }
  return INT64_MAX;
}

int ceil_log2(int64_t v) {
  int b = 0;
  while (((int64_t)1 << b) < v) ++b;
  return b;
}

// scratch of the counting pipeline for up to `cap` pairs
struct CountWork {
  DevBuf key[2], val[2], h, start, tmp;
  size_t tmp_bytes = 0;
  int64_t cap = 0;
  int32_t alloc(int64_t N, hipStream_t s) {
    cap = N;
    for (int b = 0; b < 2; ++b) {
      GSS_TRY(key[b].alloc(sizeof(unsigned long long) * (size_t)N));
      GSS_TRY(val[b].alloc(sizeof(int) * (size_t)N));
    }
    GSS_TRY(h.alloc(sizeof(int) * (size_t)N));
    GSS_TRY(start.alloc(sizeof(int) * (size_t)N));
    hipcub::DoubleBuffer<unsigned long long> keys(key[0].as<unsigned long long>(), key[1].as<unsigned long long>());
    hipcub::DoubleBuffer<int> vals(val[0].as<int>(), val[1].as<int>());
    size_t sort_bytes = 0, scan_bytes = 0;
    GSS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, vals, (int)N, 0, 64, s));
    GSS_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, scan_bytes, h.as<int>(), start.as<int>(), hipcub::Max(), (int)N,
                                              s));
    tmp_bytes = std::max(sort_bytes, scan_bytes);
    GSS_TRY(tmp.alloc(tmp_bytes));
    return GSS_OK;
  }
};

// count[g n + i] and nocc[g] for the nb grids at `grids` (device); bits: key widths of the axes over these grids
int32_t count_batch(const double* x, int64_t n, int dim, const DeclusGrid* grids, int nb, const int* bits, CountWork* wk,
                    int* count, unsigned int* nocc, hipStream_t s) {
  const int64_t N = (int64_t)nb * n;
  const int cb = bits[0] + bits[1] + bits[2], gb = ceil_log2(nb);
  GSS_REQUIRE(N <= wk->cap && cb + gb <= 64, "declustering: a batch of %d grids does not fit its scratch", nb);
  hipcub::DoubleBuffer<unsigned long long> keys(wk->key[0].as<unsigned long long>(), wk->key[1].as<unsigned long long>());
  hipcub::DoubleBuffer<int> vals(wk->val[0].as<int>(), wk->val[1].as<int>());
  GSS_TRY(dev_zero_bytes(nocc, sizeof(unsigned int) * (size_t)nb, s));
  with_dim(dim, [&](auto D) {
    hipLaunchKernelGGL(declus_keys_kernel<decltype(D)::value>, dim3(blocks_of(n), (unsigned)nb), dim3(256), 0, s, x, n,
                       grids, bits[0], bits[1], bits[2], keys.Current(), vals.Current());
  });
  GSS_HIP(hipGetLastError());
  if (cb + gb > 0) {
    ProfScope ps("declus_sort", s);
    size_t tb = wk->tmp_bytes;
    GSS_HIP(hipcub::DeviceRadixSort::SortPairs(wk->tmp.p, tb, keys, vals, (int)N, 0, cb + gb, s));
  }
  const dim3 gN(blocks_of(N));
  int* h = wk->h.as<int>();
  int* start = wk->start.as<int>();
  hipLaunchKernelGGL(declus_heads_kernel, gN, dim3(256), 0, s, keys.Current(), N, cb, h, nocc);
  GSS_HIP(hipGetLastError());
  size_t tb = wk->tmp_bytes;
  GSS_HIP(hipcub::DeviceScan::InclusiveScan(wk->tmp.p, tb, h, start, hipcub::Max(), (int)N, s));
  // (h has been scanned: it now takes the run lengths, written at the run starts only)
  hipLaunchKernelGGL(declus_runs_kernel, gN, dim3(256), 0, s, keys.Current(), start, N, h);
  hipLaunchKernelGGL(declus_scatter_kernel, gN, dim3(256), 0, s, keys.Current(), vals.Current(), start, h, N, cb, n,
                     count);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

int32_t common_checks(const char* fn, const double* x, int64_t n, int32_t dim, int32_t mem) {
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "%s: mem = %d", fn, mem);
  GSS_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside 1 .. 3", fn, dim);
  GSS_REQUIRE(n >= 1 && n < (int64_t)INT32_MAX, "%s: n = %lld: between 1 and 2^31 - 2 samples", fn, (long long)n);
  GSS_REQUIRE(x != nullptr, "%s: x is NULL", fn);
  return GSS_OK;
}

int32_t sides_check(const char* fn, const double* sides, int64_t count, int dim) {
  for (int64_t c = 0; c < count; ++c)
    for (int a = 0; a < dim; ++a) {
      const double v = sides[c * dim + a];
      GSS_REQUIRE(v > 0.0 && v <= DBL_MAX, "%s: side %g of axis %d (size %lld) must be finite and > 0", fn, v, a,
                  (long long)c);
    }
  return GSS_OK;
}

// the box of x, on the host for a host array (no device is touched) and on the device otherwise
int32_t box_of(const char* fn, const double* x, int64_t n, int dim, int32_t mem, void* stream, Box* b) {
  if (mem == GSS_MEM_HOST) box_host(x, n, dim, b);
  else GSS_TRY(box_device(x, n, dim, b, to_stream(stream)));
  GSS_REQUIRE(!b->bad, "%s: a coordinate is not finite", fn);
  return GSS_OK;
}

// The sweep over grids [g_begin, g_end) (whole sizes) of `grids` (host; `gdev` on the device): the weights of the last
// size end up in w; with z the weighted mean of every size in wm[size].
struct Sweep {
  const double* x;
  const double* z;
  int64_t n;
  int dim, noff;
  const std::vector<DeclusGrid>* grids;
  const Box* box;
  const DeclusGrid* gdev;
  unsigned int* nocc;   // one word per grid of the call
  double *acc, *partial, *wm, *w;
  CountWork* wk;
  DevBuf* cnt;
  int64_t max_nb;
};

int32_t sweep_range(const Sweep& S, int64_t g_begin, int64_t g_end, bool means, hipStream_t s) {
  const int64_t n = S.n;
  const int64_t nblk = (n + DECLUS_SUM_ITEMS - 1) / DECLUS_SUM_ITEMS;
  int64_t g0 = g_begin;
  while (g0 < g_end) {
    int64_t nb = std::min(g_end - g0, S.max_nb);
    int bits[3];
    while (true) {   // the batch's grid number must fit beside the cell bits its grids need
      bits[0] = bits[1] = bits[2] = 0;
      for (int64_t g = g0; g < g0 + nb; ++g) GSS_TRY(grid_check("gss_decluster_cells", "a grid", (*S.grids)[(size_t)g], *S.box, S.dim, bits));
      if (bits[0] + bits[1] + bits[2] + ceil_log2(nb) <= 64 || nb == 1) break;
      nb = std::max<int64_t>(1, nb / 2);
    }
    GSS_TRY(count_batch(S.x, n, S.dim, S.gdev + g0, (int)nb, bits, S.wk, S.cnt->as<int>(), S.nocc + g0, s));
    for (int64_t g = g0; g < g0 + nb;) {   // the batch by size
      const int64_t c = g / S.noff, gend = std::min(g0 + nb, (c + 1) * S.noff);
      const bool first = g == c * S.noff, last = gend == (c + 1) * S.noff;
      hipLaunchKernelGGL(declus_accum_kernel, dim3(blocks_of(n)), dim3(256), 0, s, S.cnt->as<int>() + (g - g0) * n,
                         S.nocc + g, (int)(gend - g), n, first ? 1 : 0, last ? 1 : 0, S.noff, S.acc, S.w);
      if (last && means) {
        hipLaunchKernelGGL(declus_wsum_kernel, dim3((unsigned)nblk), dim3(256), 0, s, S.w, S.z, n, S.partial);
        hipLaunchKernelGGL(declus_wsum_final_kernel, dim3(1), dim3(256), 0, s, S.partial, nblk, n, S.wm + c);
      }
      GSS_HIP(hipGetLastError());
      g = gend;
    }
    g0 += nb;
  }
  return GSS_OK;
}

}  // namespace

extern "C" {

int32_t gss_decluster_cell_counts(const double* x, int64_t n, int32_t dim, const double* origin, const double* sides,
                                  int32_t* count, int64_t* noccupied, int32_t mem, void* stream) {
  GSS_ENTRY();
  const char* fn = "gss_decluster_cell_counts";
  GSS_TRY(common_checks(fn, x, n, dim, mem));
  GSS_REQUIRE(origin != nullptr && sides != nullptr && count != nullptr && noccupied != nullptr, "%s: NULL argument", fn);
  GSS_TRY(sides_check(fn, sides, 1, dim));
  DeclusGrid g{};
  for (int a = 0; a < dim; ++a) {
    GSS_REQUIRE(std::fabs(origin[a]) <= DBL_MAX, "%s: origin %g of axis %d is not finite", fn, origin[a], a);
    g.o[a] = origin[a];
    g.s[a] = sides[a];
  }
  Box box;
  GSS_TRY(box_of(fn, x, n, dim, mem, stream, &box));
  int bits[3] = {0, 0, 0};
  GSS_TRY(grid_check(fn, "the grid", g, box, dim, bits));

  hipStream_t s = to_stream(stream);
  ProfScope ps("declus_cell_counts", s);
  Staged sx, sc;
  GSS_TRY(sx.in(x, sizeof(double) * (size_t)(n * dim), mem, s));
  GSS_TRY(sc.out(count, sizeof(int32_t) * (size_t)n, mem));
  DevBuf gdev, nocc;
  GSS_TRY(gdev.alloc(sizeof(DeclusGrid)));
  GSS_TRY(nocc.alloc(sizeof(unsigned int)));
  GSS_HIP(hipMemcpyAsync(gdev.p, &g, sizeof(g), hipMemcpyHostToDevice, s));
  CountWork wk;
  GSS_TRY(wk.alloc(n, s));
  GSS_TRY(count_batch(sx.as<double>(), n, dim, gdev.as<DeclusGrid>(), 1, bits, &wk, sc.as<int>(), nocc.as<unsigned int>(),
                      s));
  unsigned int occ = 0;
  GSS_HIP(hipMemcpyAsync(&occ, nocc.p, sizeof(occ), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));   // noccupied is a host word; g and the scratch go out of scope
  *noccupied = (int64_t)occ;
  GSS_TRY(sc.back(s));
  return GSS_OK;
}

int32_t gss_decluster_cells(const double* x, const double* z, int64_t n, int32_t dim, const double* sides, int32_t ncs,
                            int32_t noff, int32_t criterion, double* w, double* wmean, int32_t* best, int32_t mem,
                            void* stream) {
  GSS_ENTRY();
  const char* fn = "gss_decluster_cells";
  GSS_TRY(common_checks(fn, x, n, dim, mem));
  GSS_REQUIRE(ncs >= 1 && ncs <= 256, "%s: ncs = %d outside 1 .. 256", fn, ncs);
  GSS_REQUIRE(noff >= 1 && noff <= 64, "%s: noff = %d outside 1 .. 64", fn, noff);
  GSS_REQUIRE(criterion == GSS_DECLUS_MIN || criterion == GSS_DECLUS_MAX, "%s: criterion = %d", fn, criterion);
  GSS_REQUIRE(sides != nullptr && w != nullptr && best != nullptr, "%s: NULL argument", fn);
  GSS_REQUIRE(z != nullptr || ncs == 1, "%s: z is NULL with ncs = %d: without values only one size can be weighted", fn,
              ncs);
  GSS_REQUIRE(z == nullptr || wmean != nullptr, "%s: wmean is NULL", fn);
  GSS_TRY(sides_check(fn, sides, ncs, dim));
  Box box, zbox;
  GSS_TRY(box_of(fn, x, n, dim, mem, stream, &box));
  if (z != nullptr) {
    if (mem == GSS_MEM_HOST) box_host(z, n, 1, &zbox);
    else GSS_TRY(box_device(z, n, 1, &zbox, to_stream(stream)));
    GSS_REQUIRE(!zbox.bad, "%s: a value of z is not finite", fn);
  }
  // every grid of the sweep: origin = lo - (side k) / noff, the product and the quotient rounded apart
  const int64_t G = (int64_t)ncs * noff;
  std::vector<DeclusGrid> grids((size_t)G);
  for (int c = 0; c < ncs; ++c)
    for (int k = 0; k < noff; ++k) {
      DeclusGrid& g = grids[(size_t)(c * noff + k)];
      g = DeclusGrid{};
      for (int a = 0; a < dim; ++a) {
#pragma clang fp contract(off)
        const double sa = sides[c * dim + a];
        const double shift = sa * (double)k;
        const double off = shift / (double)noff;
        g.s[a] = sa;
        g.o[a] = box.lo[a] - off;
      }
      int bits[3] = {0, 0, 0};
      char what[64];
      snprintf(what, sizeof(what), "size %d, offset %d", c, k);
      GSS_TRY(grid_check(fn, what, g, box, dim, bits));
    }

  hipStream_t s = to_stream(stream);
  ProfScope ps("declus_cells", s);
  Staged sx, sz, sw;
  GSS_TRY(sx.in(x, sizeof(double) * (size_t)(n * dim), mem, s));
  GSS_TRY(sz.in(z, sizeof(double) * (size_t)n, mem, s));
  GSS_TRY(sw.out(w, sizeof(double) * (size_t)n, mem));
  const int64_t nblk = (n + DECLUS_SUM_ITEMS - 1) / DECLUS_SUM_ITEMS;
  DevBuf gdev, nocc, acc, partial, wm, cnt;
  GSS_TRY(gdev.alloc(sizeof(DeclusGrid) * (size_t)G));
  GSS_TRY(nocc.alloc(sizeof(unsigned int) * (size_t)G));
  GSS_TRY(acc.alloc(sizeof(double) * (size_t)n));
  GSS_TRY(partial.alloc(sizeof(double) * (size_t)nblk));
  GSS_TRY(wm.alloc(sizeof(double) * (size_t)ncs));
  GSS_HIP(hipMemcpyAsync(gdev.p, grids.data(), sizeof(DeclusGrid) * (size_t)G, hipMemcpyHostToDevice, s));
  const int64_t max_nb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(G, DECLUS_BATCH_ITEMS / n),
                                                                chunk_grids_cap()));
  CountWork wk;
  GSS_TRY(wk.alloc(max_nb * n, s));
  GSS_TRY(cnt.alloc(sizeof(int) * (size_t)(max_nb * n)));
  Sweep S{sx.as<double>(), sz.as<double>(), n, dim, noff, &grids, &box, gdev.as<DeclusGrid>(), nocc.as<unsigned int>(),
          acc.as<double>(), partial.as<double>(), wm.as<double>(), sw.as<double>(), &wk, &cnt, max_nb};
  GSS_TRY(sweep_range(S, 0, G, z != nullptr, s));
  int32_t b = 0;
  if (z != nullptr) {
    GSS_HIP(hipMemcpyAsync(wmean, wm.p, sizeof(double) * (size_t)ncs, hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
    for (int c = 1; c < ncs; ++c)
      if (criterion == GSS_DECLUS_MIN ? wmean[c] < wmean[b] : wmean[c] > wmean[b]) b = c;
    // w holds the weights of the last size: those of another best size are formed once more, by the same arithmetic
    if (b != ncs - 1) GSS_TRY(sweep_range(S, (int64_t)b * noff, (int64_t)(b + 1) * noff, false, s));
  }
  *best = b;
  GSS_TRY(sw.back(s));
  GSS_HIP(hipStreamSynchronize(s));   // the grids and the scratch go out of scope
  return GSS_OK;
}

int32_t gss_decluster_nearest(const double* x, int64_t n, int32_t dim, const double* lo, const double* step,
                              const int64_t* dims, double* w, int64_t* nzero, int32_t mem, void* stream) {
  GSS_ENTRY();
  const char* fn = "gss_decluster_nearest";
  GSS_TRY(common_checks(fn, x, n, dim, mem));
  GSS_REQUIRE(lo != nullptr && step != nullptr && dims != nullptr && w != nullptr && nzero != nullptr,
              "%s: NULL argument", fn);
  int64_t M = 1;
  for (int a = 0; a < dim; ++a) {
    GSS_REQUIRE(std::fabs(lo[a]) <= DBL_MAX, "%s: lo %g of axis %d is not finite", fn, lo[a], a);
    GSS_REQUIRE(step[a] > 0.0 && step[a] <= DBL_MAX, "%s: step %g of axis %d must be finite and > 0", fn, step[a], a);
    GSS_REQUIRE(dims[a] >= 1, "%s: dims %lld of axis %d must be >= 1", fn, (long long)dims[a], a);
    GSS_REQUIRE(dims[a] <= ((int64_t)1 << 53) / M, "%s: the lattice has more than 2^53 points", fn);
    M *= dims[a];
  }
  Box box;
  GSS_TRY(box_of(fn, x, n, dim, mem, stream, &box));

  hipStream_t s = to_stream(stream);
  ProfScope ps("declus_nearest", s);
  int64_t chunk = DECLUS_QUERY_CHUNK;
  if (const char* e = std::getenv("GSS_DECLUS_CHUNK_QUERIES")) {   // tests: a chunk loop that runs more than once
    const long long v = std::atoll(e);
    if (v > 0 && v < chunk) chunk = v;
  }
  chunk = std::min(chunk, M);
  Staged sx, sw;
  GSS_TRY(sx.in(x, sizeof(double) * (size_t)(n * dim), mem, s));
  GSS_TRY(sw.out(w, sizeof(double) * (size_t)n, mem));
  DevBuf q, idx, hits;
  GSS_TRY(q.alloc(sizeof(double) * (size_t)(chunk * dim)));
  GSS_TRY(idx.alloc(sizeof(int) * (size_t)chunk));
  GSS_TRY(hits.alloc(sizeof(unsigned long long) * (size_t)(n + 1)));   // [n]: samples without a hit
  GSS_TRY(dev_zero_bytes(hits.p, sizeof(unsigned long long) * (size_t)(n + 1), s));
  unsigned long long nz = 0;
  {
    Searcher sr;   // (waits for the stream before it lets its index go)
    GSS_TRY(sr.init(GSS_METRIC_EUCLIDEAN, 0.0, -1.0, nullptr, dim));
    GSS_TRY(sr.samples(sx.as<double>(), nullptr, n, s, mem == GSS_MEM_HOST ? x : nullptr));
    const double l[3] = {lo[0], dim > 1 ? lo[1] : 0.0, dim > 2 ? lo[2] : 0.0};
    const double st[3] = {step[0], dim > 1 ? step[1] : 1.0, dim > 2 ? step[2] : 1.0};
    const int64_t d0 = dims[0], d1 = dim > 1 ? dims[1] : 1;
    for (int64_t j0 = 0; j0 < M; j0 += chunk) {
      const int64_t m = std::min(chunk, M - j0);
      with_dim(dim, [&](auto D) {
        hipLaunchKernelGGL(declus_queries_kernel<decltype(D)::value>, dim3(blocks_of(m)), dim3(256), 0, s, l[0], l[1],
                           l[2], st[0], st[1], st[2], d0, d1, j0, m, q.as<double>());
      });
      GSS_HIP(hipGetLastError());
      GSS_TRY(sr.query(q.as<double>(), nullptr, m, 1, idx.as<int>(), nullptr, s));
      hipLaunchKernelGGL(declus_hits_kernel, dim3(blocks_of(m)), dim3(256), 0, s, idx.as<int>(), m, n,
                         hits.as<unsigned long long>());
      GSS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(declus_hit_weights_kernel, dim3(blocks_of(n)), dim3(256), 0, s, hits.as<unsigned long long>(), n,
                       (double)M, sw.as<double>(), hits.as<unsigned long long>() + n);
    GSS_HIP(hipGetLastError());
    GSS_HIP(hipMemcpyAsync(&nz, hits.as<unsigned long long>() + n, sizeof(nz), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));   // nzero is a host word
  }
  *nzero = (int64_t)nz;
  GSS_TRY(sw.back(s));
  return GSS_OK;
}

}  // extern "C"
