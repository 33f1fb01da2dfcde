// Cross-validation by folds under the global neighbourhood (gss.h, gss_krig_cv_global_folds): the block form of
// Dubrule's identity, read off the factor a fitted handle already holds.  With B = K^-1 = W'^T D W' (D = +1 on the n
// data rows, -1 on the nc constraint rows) and wd = B [z - mean; 0], the errors of the samples of a fold F predicted
// from every sample outside F are e_F = (B_FF)^-1 wd_F and their kriging variances diag((B_FF)^-1).  Three steps:
//
//   1. cv_fold_gram_kernel   B_FF = W'[:, F]^T D W'[:, F] for every fold at once, FP64 MFMA, packed blocks
//   2. cv_fold_solve_kernel  folds of up to CVF_S samples: B_FF = L L^T, L^-1, e_F and the variances in LDS, one
//                            workgroup per fold
//      folds beyond CVF_S    one after the other through potrf_inverse_f64 (the routine of the fit), then
//                            cv_fold_u_kernel and cv_fold_finish_kernel
//   3. pred = z - e, var, status scattered through the permutation that groups the samples by fold
//
// Every sum is formed in a fixed order (k ascending in an MFMA accumulator; a thread over its terms in ascending
// order; the lanes of a wave in a fixed butterfly) and nothing is added with atomics: two runs give the same bits.
#include "gss_internal.h"
#include "mfma_f64.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace gss {

// ---- 1. signed Gram blocks ------------------------------------------------------------------------------------------
// One workgroup (4 waves) per 64 x 64 block of the lower triangle of a B_FF; wave w owns the 16 rows w of the block and
// its four 16 x 16 column tiles (4 accumulators of v_mfma_f64_16x16x4_f64, lane map of mfma_f64.h).  k runs over the
// rows of W' in stages of CVF_K = 16: a stage is the rows k .. k + 15 of the 64 gathered columns of either side.
//
// Loads: a column of W' is contiguous in k, the gathered columns are ldw apart.  Thread t fetches rows 4 (t >> 6) .. + 3
// of column t & 63 -- 32 aligned bytes, the four waves together one 128-byte line of every column -- and writes them
// k-major into LDS, As[k][column] with a row stride of CVF_LD = 80 doubles.  80 = 16 (mod 32): the two k rows that the
// 32 lanes of one ds_read_b64 group read for an MFMA operand fall on disjoint halves of the 64 banks.  A write goes the
// other way about: the row stride is a multiple of 32 dwords, so two k of one column share a bank and the 64 lanes of a
// write must differ in their column -- which is why a thread owns a column and not a quarter of a line.
// The next stage is fetched into registers while the MFMAs of this one run.
//
// W' is lower triangular and row N1 holds the dual weights: an element (k, c) counts for c <= k < N1 only, everything
// else is replaced by an exact zero, whatever the memory holds.  The columns of a fold are gathered in ascending order
// (stable grouping), so the first column of the row block bounds every column of both sides from below and k starts at
// its multiple of 16.  Columns past the end of the fold are zero-filled.  The sign of D is applied to the A side.
constexpr int CVF_T = 64;    // block of B_FF per workgroup
constexpr int CVF_K = 16;    // rows of W' per stage
constexpr int CVF_LD = 80;   // LDS row stride (doubles)

// fold descriptor: 4 ints per fold
enum { CVF_OFF = 0, CVF_SIZE = 1, CVF_FLAG = 2, CVF_DESC = 4 };

__device__ __forceinline__ void cvf_fetch(const double* __restrict__ col, int c, int k, int n, int N1, bool negate,
                                          double (&v)[4]) {
  if (c < 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = 0.0;
    return;
  }
  // k is a multiple of 4 below N1 and the leading dimension a multiple of 128 above N1: k + 3 is a row of the column
  const d2v lo = *reinterpret_cast<const d2v*>(col + k);
  const d2v hi = *reinterpret_cast<const d2v*>(col + k + 2);
  const double w[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kk = k + q;
    const double x = (kk >= c && kk < N1) ? w[q] : 0.0;
    v[q] = (negate && kk >= n) ? -x : x;
  }
}

__global__ __launch_bounds__(256) void cv_fold_gram_kernel(const double* __restrict__ Wp, int64_t ldw, int n, int N1,
                                                           const int* __restrict__ perm, const int* __restrict__ desc,
                                                           const long long* __restrict__ goff,
                                                           const int* __restrict__ tiles, double* __restrict__ G) {
  __shared__ double As[CVF_K * CVF_LD];
  __shared__ double Bs[CVF_K * CVF_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int f = tiles[3 * blockIdx.x], bi = tiles[3 * blockIdx.x + 1], bj = tiles[3 * blockIdx.x + 2];
  const int off = desc[CVF_DESC * f + CVF_OFF], s = desc[CVF_DESC * f + CVF_SIZE];
  const int ia = bi * CVF_T + lane, ib = bj * CVF_T + lane;
  const int ca = ia < s ? perm[off + ia] : -1;
  const int cb = ib < s ? perm[off + ib] : -1;
  const double* cola = Wp + (int64_t)(ca < 0 ? 0 : ca) * ldw;
  const double* colb = Wp + (int64_t)(cb < 0 ? 0 : cb) * ldw;
  const int k0 = perm[off + bi * CVF_T] & ~(CVF_K - 1);   // bi >= bj: the smallest column of either side
  // live 16-tiles of this block (the last block of a fold is ragged); on the diagonal only tiles tn <= wave
  const int rows_live = (min(s - bi * CVF_T, CVF_T) + 15) >> 4;
  int cols_live = (min(s - bj * CVF_T, CVF_T) + 15) >> 4;
  if (bi == bj && wave + 1 < cols_live) cols_live = wave + 1;
  const bool live = wave < rows_live;

  d4 acc[4];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) acc[tn] = d4{0.0, 0.0, 0.0, 0.0};
  double ra[4], rb[4];
  cvf_fetch(cola, ca, k0 + 4 * wave, n, N1, true, ra);
  cvf_fetch(colb, cb, k0 + 4 * wave, n, N1, false, rb);
  const int lr = lane & 15, lk = lane >> 4;
  for (int kb = k0; kb < N1; kb += CVF_K) {
    __syncthreads();   // the reads of the stage before
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      As[(4 * wave + q) * CVF_LD + lane] = ra[q];
      Bs[(4 * wave + q) * CVF_LD + lane] = rb[q];
    }
    __syncthreads();
    if (kb + CVF_K < N1) {
      cvf_fetch(cola, ca, kb + CVF_K + 4 * wave, n, N1, true, ra);
      cvf_fetch(colb, cb, kb + CVF_K + 4 * wave, n, N1, false, rb);
    }
    if (live) {
#pragma unroll
      for (int kk = 0; kk < CVF_K / 4; ++kk) {
        const double a = As[(kk * 4 + lk) * CVF_LD + wave * 16 + lr];
        const double* bp = Bs + (kk * 4 + lk) * CVF_LD + lr;
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
          if (tn < cols_live) acc[tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bp[tn * 16], acc[tn], 0, 0, 0);
      }
    }
  }
  if (!live) return;
  // the block and its mirror image: the factorisations read the lower triangle, the packed block is kept symmetric
  double* g = G + goff[f];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) {
    if (tn >= cols_live) continue;
    const int c = bj * CVF_T + tn * 16 + lr;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int r = bi * CVF_T + wave * 16 + lk + 4 * r4;
      if (r < s && c < s && r >= c) {
        g[r + (int64_t)c * s] = acc[tn][r4];
        g[c + (int64_t)r * s] = acc[tn][r4];
      }
    }
  }
}

// ---- 2. one workgroup per fold --------------------------------------------------------------------------------------
// CVF_S = 128: the lower triangle of B_FF sits in LDS as a square with an odd row stride (s | 1: threads that walk a
// row or a column of it meet distinct banks), L replaces it and L^-1 replaces L, so one square serves all three:
// 128 * 129 doubles + two vectors of 128 = 134 144 bytes of the 163 840 a workgroup may have.  (A second square for the
// inverse would halve the size; 140 is the largest s that fits this way, 128 is the multiple of the MFMA tile below it.)
// The kernel is launched with the LDS of the largest such fold of the call, so many small folds share a CU.
constexpr int CVF_S = 128;
constexpr size_t cvf_solve_lds(int s) { return sizeof(double) * ((size_t)s * (s | 1) + 2 * (size_t)s); }

__device__ __forceinline__ void cvf_put(int p, double a, double b, uint8_t st, double* __restrict__ pred,
                                        double* __restrict__ var, uint8_t* __restrict__ status) {
  pred[p] = a;
  var[p] = b;
  if (status) status[p] = st;
}

__global__ __launch_bounds__(256) void cv_fold_solve_kernel(const double* __restrict__ G,
                                                            const long long* __restrict__ goff,
                                                            const int* __restrict__ desc, const int* __restrict__ list,
                                                            const int* __restrict__ perm, const double* __restrict__ wd,
                                                            const double* __restrict__ z, double* __restrict__ pred,
                                                            double* __restrict__ var, uint8_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double cvf_sm[];
  const double NaN = __longlong_as_double(0x7ff8000000000000LL);
  const int t = threadIdx.x;
  const int f = list[blockIdx.x];
  const int off = desc[CVF_DESC * f + CVF_OFF], s = desc[CVF_DESC * f + CVF_SIZE];
  if (desc[CVF_DESC * f + CVF_FLAG]) {   // the samples outside the fold cannot determine the system
    for (int i = t; i < s; i += 256) cvf_put(perm[off + i], NaN, NaN, GSS_PT_SINGULAR, pred, var, status);
    return;
  }
  const int ld = s | 1;
  double* A = cvf_sm;
  double* y = A + s * ld;
  double* col = y + s;
  const double* g = G + goff[f];
  for (int c = t >> 4; c < s; c += 16)
    for (int r = c + (t & 15); r < s; r += 16) A[r + c * ld] = g[r + (int64_t)c * s];
  for (int i = t; i < s; i += 256) y[i] = wd[perm[off + i]];
  __syncthreads();

  // B_FF = L L^T, right-looking; every thread sees the same pivot, so all of them leave together
  bool bad = false;
  for (int j = 0; j < s; ++j) {
    const double d = A[j + j * ld];
    if (!(d > 0.0 && d < __builtin_huge_val())) {
      bad = true;
      break;
    }
    const double r = sqrt(d);
    __syncthreads();   // the pivot has been read
    for (int i = j + t; i < s; i += 256) A[i + j * ld] = i == j ? r : A[i + j * ld] / r;
    __syncthreads();
    for (int c = j + 1 + (t >> 4); c < s; c += 16) {
      const double lc = A[c + j * ld];
      for (int i = c + (t & 15); i < s; i += 16) A[i + c * ld] = fma(-A[i + j * ld], lc, A[i + c * ld]);
    }
    __syncthreads();
  }
  if (bad) {
    for (int i = t; i < s; i += 256) cvf_put(perm[off + i], NaN, NaN, GSS_PT_SINGULAR, pred, var, status);
    return;
  }

  // L <- L^-1 in place, last column first: X(i, j) = -(sum_{k = j+1..i} X(i, k) L(k, j)) / L(j, j)
  for (int j = s - 1; j >= 0; --j) {
    for (int i = j + 1 + t; i < s; i += 256) col[i] = A[i + j * ld];
    const double dj = 1.0 / A[j + j * ld];
    __syncthreads();
    for (int i = j + 1 + t; i < s; i += 256) {
      double a = 0.0;
      for (int k = j + 1; k <= i; ++k) a = fma(A[i + k * ld], col[k], a);
      A[i + j * ld] = -a * dj;
    }
    if (t == 0) A[j + j * ld] = dj;
    __syncthreads();
  }

  // u = L^-1 wd_F ; e = L^-T u ; var_i = sum_{k >= i} (L^-1)(k, i)^2
  for (int k = t; k < s; k += 256) {
    double a = 0.0;
    for (int i = 0; i <= k; ++i) a = fma(A[k + i * ld], y[i], a);
    col[k] = a;
  }
  __syncthreads();
  for (int i = t; i < s; i += 256) {
    double e = 0.0, v = 0.0;
    for (int k = i; k < s; ++k) {
      const double w = A[k + i * ld];
      e = fma(w, col[k], e);
      v = fma(w, w, v);
    }
    const int p = perm[off + i];
    cvf_put(p, z[p] - e, v > 0.0 ? v : 0.0, GSS_PT_OK, pred, var, status);
  }
}

// ---- folds beyond CVF_S: W = inv(L) of the fold (s x s, column-major, ld s) comes from potrf_inverse_f64 -------------
// u_k = sum_{i <= k} W(k, i) wd_F(i): one wave per row, lanes in a fixed butterfly
__global__ __launch_bounds__(256) void cv_fold_u_kernel(const double* __restrict__ W, int s,
                                                        const int* __restrict__ permf, const double* __restrict__ wd,
                                                        double* __restrict__ u) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= s) return;  // whole wave
  double acc = 0.0;
  for (int i = lane; i <= k; i += 64) acc = fma(W[k + (int64_t)i * s], wd[permf[i]], acc);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) u[k] = acc;
}

// e_i = sum_{k >= i} W(k, i) u_k, var_i = sum_{k >= i} W(k, i)^2: one wave per column, as krig_loo_kernel
__global__ __launch_bounds__(256) void cv_fold_finish_kernel(const double* __restrict__ W, int s,
                                                             const int* __restrict__ permf,
                                                             const double* __restrict__ u, const int* __restrict__ info,
                                                             const double* __restrict__ z, double* __restrict__ pred,
                                                             double* __restrict__ var, uint8_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= s) return;  // whole wave
  const double* col = W + (int64_t)i * s;
  double e = 0.0, v = 0.0;
  for (int k = i + lane; k < s; k += 64) {
    const double w = col[k];
    e = fma(w, u[k], e);
    v = fma(w, w, v);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    e += __shfl_xor(e, o);
    v += __shfl_xor(v, o);
  }
  if (lane != 0) return;
  const double NaN = __longlong_as_double(0x7ff8000000000000LL);
  const int p = permf[i];
  if (info[0] != 0) cvf_put(p, NaN, NaN, GSS_PT_SINGULAR, pred, var, status);   // a pivot of the fold's Cholesky
  else cvf_put(p, z[p] - e, v > 0.0 ? v : 0.0, GSS_PT_OK, pred, var, status);
}

// ---- host -----------------------------------------------------------------------------------------------------------
// fold: n ids >= 0 on the host (checked by the caller); Wp, wd, z, pred, var, status (nullable): device.  Returns when
// the results are complete (the host arrays of the grouping are read by asynchronous copies).
int32_t cv_global_folds_dev(const double* Wp, int64_t ldw, int64_t n, int64_t N1, int nc, bool simple,
                            const double* wd, const double* z, const int32_t* fold, double* pred, double* var,
                            uint8_t* status, hipStream_t s) {
  // samples grouped by fold, stable: ascending id, ascending sample index inside a fold
  std::vector<int> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [fold](int a, int b) { return fold[a] < fold[b]; });
  std::vector<int> desc, list, big, tiles;
  std::vector<long long> goff;
  const int64_t need = nc > 1 ? nc : 1;   // samples a remainder must at least hold (simple kriging: none)
  long long gtotal = 0;
  int small_max = 0;
  int64_t big_max = 0;
  for (int64_t a = 0; a < n;) {
    int64_t b = a + 1;
    while (b < n && fold[perm[(size_t)b]] == fold[perm[(size_t)a]]) ++b;
    const int f = (int)goff.size(), sf = (int)(b - a);
    const int undetermined = (!simple && n - sf < need) ? 1 : 0;
    desc.insert(desc.end(), {(int)a, sf, undetermined, 0});
    goff.push_back(gtotal);
    if (undetermined || sf <= CVF_S) {
      list.push_back(f);
      if (!undetermined && sf > small_max) small_max = sf;
    } else {
      big.push_back(f);
      if (sf > big_max) big_max = sf;
    }
    if (!undetermined) {
      gtotal += (long long)sf * sf;
      const int nb = (sf + CVF_T - 1) / CVF_T;
      for (int bi = 0; bi < nb; ++bi)
        for (int bj = 0; bj <= bi; ++bj) tiles.insert(tiles.end(), {f, bi, bj});
    }
    a = b;
  }
  const size_t nf = goff.size(), ntiles = tiles.size() / 3;

  // one device image of the grouping: goff | perm | desc | list | tiles
  const size_t ints = (size_t)n + desc.size() + list.size() + tiles.size();
  DevBuf meta, gram;
  GSS_TRY(meta.alloc(sizeof(long long) * nf + sizeof(int) * ints));
  long long* d_goff = meta.as<long long>();
  int* d_perm = reinterpret_cast<int*>(d_goff + nf);
  int* d_desc = d_perm + n;
  int* d_list = d_desc + desc.size();
  int* d_tiles = d_list + list.size();
  GSS_HIP(hipMemcpyAsync(d_goff, goff.data(), sizeof(long long) * nf, hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(d_perm, perm.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(d_desc, desc.data(), sizeof(int) * desc.size(), hipMemcpyHostToDevice, s));
  if (!list.empty()) GSS_HIP(hipMemcpyAsync(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, s));
  if (ntiles) GSS_HIP(hipMemcpyAsync(d_tiles, tiles.data(), sizeof(int) * tiles.size(), hipMemcpyHostToDevice, s));
  GSS_TRY(gram.alloc(sizeof(double) * (size_t)(gtotal > 0 ? gtotal : 1)));
  double* G = gram.as<double>();

  if (ntiles) {
    ProfScope ps("cv_fold_gram", s);
    hipLaunchKernelGGL(cv_fold_gram_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, Wp, ldw, (int)n, (int)N1, d_perm,
                       d_desc, d_goff, d_tiles, G);
    GSS_HIP(hipGetLastError());
  }
  if (!list.empty()) {
    const size_t lds = cvf_solve_lds(small_max);
    static uint64_t attr = 0;
    if (first_on_this_device(attr))
      GSS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cv_fold_solve_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)cvf_solve_lds(CVF_S)));
    ProfScope ps("cv_fold_solve", s);
    hipLaunchKernelGGL(cv_fold_solve_kernel, dim3((unsigned)list.size()), dim3(256), lds, s, G, d_goff, d_desc, d_list,
                       d_perm, wd, z, pred, var, status);
    GSS_HIP(hipGetLastError());
  }
  if (!big.empty()) {
    // at most n / CVF_S folds, one after the other on the factor-and-inverse of the fit
    int64_t wsz = big_max * big_max;
    for (int f : big)
      if (potrf_inverse_work_doubles(desc[CVF_DESC * f + CVF_SIZE]) > wsz)
        wsz = potrf_inverse_work_doubles(desc[CVF_DESC * f + CVF_SIZE]);
    DevBuf winv, scr, uvec, info;
    GSS_TRY(winv.alloc(sizeof(double) * (size_t)(big_max * big_max)));
    GSS_TRY(scr.alloc(sizeof(double) * (size_t)wsz));
    GSS_TRY(uvec.alloc(sizeof(double) * (size_t)big_max));
    GSS_TRY(info.alloc(sizeof(int) * big.size()));
    {
      ProfScope ps("cv_fold_large", s);
      for (size_t b = 0; b < big.size(); ++b) {
        const int f = big[b], off = desc[CVF_DESC * f + CVF_OFF], sf = desc[CVF_DESC * f + CVF_SIZE];
        GSS_TRY(dev_zero_bytes(winv.p, sizeof(double) * (size_t)sf * sf, s));
        GSS_TRY(potrf_inverse_f64(G + goff[(size_t)f], sf, sf, winv.as<double>(), sf, scr.as<double>(),
                                  info.as<int>() + b, false, s));
        const unsigned grid = (unsigned)((sf + 3) / 4);
        hipLaunchKernelGGL(cv_fold_u_kernel, dim3(grid), dim3(256), 0, s, winv.as<double>(), sf, d_perm + off, wd,
                           uvec.as<double>());
        hipLaunchKernelGGL(cv_fold_finish_kernel, dim3(grid), dim3(256), 0, s, winv.as<double>(), sf, d_perm + off,
                           uvec.as<double>(), info.as<int>() + b, z, pred, var, status);
        GSS_HIP(hipGetLastError());
      }
    }
    std::vector<int> hinfo(big.size());
    GSS_HIP(hipMemcpyAsync(hinfo.data(), info.p, sizeof(int) * big.size(), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
    for (int h : hinfo) {
      if (h < 0) {
        set_error("gss_krig_cv_global_folds: the factor-and-inverse kernel gave up waiting at a grid barrier");
        return GSS_ERR_HIP;
      }
    }
  }
  GSS_HIP(hipStreamSynchronize(s));   // perm, desc, ... leave scope
  return GSS_OK;
}

}  // namespace gss
