// SGS stage A (gss_sgs_create; the split of the work is described in sgs.hip): per node the masked exact k-NN
// (rank[neighbour] < rank[node]; knn.hip), then the k x k covariance, Cholesky, lambda = C^-1 c0 and
// sigma^2 = sill - |L^-1 c0|^2 -- a wave per node up to 64 neighbours, a workgroup per node beyond.
#include "sgs_internal.h"

#include <climits>
#include <cmath>
#include <memory>

namespace gss {

__device__ __forceinline__ int sgs_tri(int i) { return (i * (i + 1)) >> 1; }

// row i and column c of entry e of a packed lower triangle
__device__ __forceinline__ void sgs_tri_decode(int e, int* i, int* c) {
  int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while (sgs_tri(r + 1) <= e) ++r;
  while (sgs_tri(r) > e) --r;
  *i = r;
  *c = e - sgs_tri(r);
}

// A node without weights, written by one thread: a data cell (sigma 0, never simulated, seq.jl:103) or the marginal
// (sigma = sqrt(sill), sgs.jl:66: too few neighbours, seq.jl:107-109, or status(fitted) == false, seq.jl:124-128)
__device__ __forceinline__ void sgs_no_weights(bool first, int64_t p, double sg, int* __restrict__ ncond,
                                               double* __restrict__ sigma_out) {
  if (first) {
    ncond[p] = 0;
    sigma_out[p] = sg;
  }
}

// One pass of 64 of the ordered compaction (`mask=simulated` applied after the search): a lane keeps entry j of a raw
// list of cnt entries if that cell is simulated before the node (rank below rp; data cells: -1).  slot, total: of the pass.
struct SgsKept { bool keep; int nb, slot, total; };
__device__ __forceinline__ SgsKept sgs_keep_pass(const int* __restrict__ list, int j, int cnt,
                                                 const int* __restrict__ rank, int rp, int lane) {
  const bool in = j < cnt;
  const int nb = in ? list[j] : 0;
  const bool keep = in && rank[nb] < rp;
  const unsigned long long bm = __ballot(keep);
  return {keep, nb, (int)__popcll(bm & ((1ull << lane) - 1ull)), (int)__popcll(bm)};
}

// lowest visiting rank inside each batch of the search index
__global__ __launch_bounds__(256) void sgs_batch_minrank_kernel(const int* __restrict__ perm,
                                                                const int* __restrict__ rank, int n, int nb,
                                                                int* __restrict__ bmin) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= nb) return;
  const int j = b * 64 + lane;
  int r = j < n ? rank[perm[j]] : INT_MAX;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(r, off);
    r = o < r ? o : r;
  }
  if (lane == 0) bmin[b] = r;
}

// simple-kriging weights of one node per wave
template <int DIM>
__global__ __launch_bounds__(64) void sgs_weights_kernel(
    VgDev vg, const double* __restrict__ cent, const int* __restrict__ rank, int64_t N, int k, int minneighbors,
    const int* __restrict__ idx, const int* __restrict__ count, int* __restrict__ ncond, double* __restrict__ w_out,
    double* __restrict__ sigma_out, int* __restrict__ idx_rw, int filter_after) {
  __shared__ double Lp[SGS_MAX_K * (SGS_MAX_K + 1) / 2];
  __shared__ double nx[SGS_MAX_K][3];
  __shared__ int cidx[SGS_MAX_K];
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  if (rank[p] < 0) {  // data cell
    if (filter_after && lane < k) idx_rw[p * k + lane] = -1;   // its list is this kernel's to write: empty
    sgs_no_weights(lane == 0, p, 0.0, ncond, sigma_out);
    return;
  }
  int cnt = count[p];
  if (filter_after) {   // the search was NOT masked: of the k nearest cells (the node itself included) keep, in order
    const SgsKept kp = sgs_keep_pass(idx + p * k, lane, cnt, rank, rank[p], lane);
    if (kp.keep) cidx[kp.slot] = kp.nb;
    __syncthreads();
    cnt = kp.total;
    if (lane < k) idx_rw[p * k + lane] = lane < cnt ? cidx[lane] : -1;
    __syncthreads();
  }
  const double smarg = sqrt(vg.sill);
  if (cnt < minneighbors || cnt <= 0) {
    sgs_no_weights(lane == 0, p, smarg, ncond, sigma_out);
    return;
  }
  double c0[DIM], xj[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) c0[a] = cent[p * DIM + a];
  const bool act = lane < cnt;
  const int nj = act ? (filter_after ? cidx[lane] : idx[p * k + lane]) : 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    xj[a] = act ? cent[(int64_t)nj * DIM + a] : 0.0;
    nx[lane][a] = xj[a];
  }
  double b = act ? cov_pair<DIM>(vg, xj, c0) : 0.0;
  __syncthreads();
  const int nent = sgs_tri(cnt);
  for (int e = lane; e < nent; e += 64) {
    int i, c;
    sgs_tri_decode(e, &i, &c);
    double xi[DIM], xc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      xi[a] = nx[i][a];
      xc[a] = nx[c][a];
    }
    Lp[e] = cov_pair<DIM>(vg, xi, xc);
  }
  __syncthreads();
  // Cholesky, left-looking by columns: lane i owns row i
  bool bad = false;
  const double* rowi = Lp + sgs_tri(lane < cnt ? lane : 0);
  for (int j = 0; j < cnt; ++j) {
    double acc = 0.0;
    const bool mine = lane >= j && lane < cnt;
    if (mine) {
      const double* rowj = Lp + sgs_tri(j);
      acc = rowi[j];
      for (int c = 0; c < j; ++c) acc = fma(-rowi[c], rowj[c], acc);
    }
    const double d = __shfl(acc, j);
    if (!(d > 0.0)) {
      bad = true;
      break;
    }
    const double sq = sqrt(d);
    if (mine) Lp[sgs_tri(lane) + j] = (lane == j) ? sq : acc / sq;
    __syncthreads();
  }
  if (bad) {
    sgs_no_weights(lane == 0, p, smarg, ncond, sigma_out);
    return;
  }
  // y = L^-1 c0 (column sweep)
  for (int j = 0; j < cnt; ++j) {
    const double ljj = Lp[sgs_tri(j) + j];
    const double lij = (lane > j && lane < cnt) ? rowi[j] : 0.0;
    const double yj = __shfl(b, j) / ljj;
    if (lane == j) b = yj;
    else b = fma(-lij, yj, b);
  }
  const double q = wave_sum(act ? b * b : 0.0);
  // lambda = L^-T y (row j of L is contiguous: lane i < j reads L[j][i])
  for (int j = cnt - 1; j >= 0; --j) {
    const double ljj = Lp[sgs_tri(j) + j];
    const double lj = __shfl(b, j) / ljj;
    if (lane == j) b = lj;
    else if (lane < j) b = fma(-Lp[sgs_tri(j) + lane], lj, b);
  }
  if (act) w_out[p * k + lane] = b;
  if (lane == 0) {
    const double v = vg.sill - q;
    ncond[p] = cnt;
    sigma_out[p] = sqrt(v > 0.0 ? v : 0.0);
  }
}

// More than 64 neighbours (seq.jl:91-98 accepts any maxneighbors; the search runs in passes of 64, knn.hip).  One
// workgroup of 256 threads per node: the kept neighbours in order (wave 0: sgs_keep_pass by 64s), the packed covariance
// triangle in LDS while it fits (up to 180 neighbours) or in a slab of HBM, Cholesky by columns, forward and back
// substitution.  A functional path like krig_local_big_kernel: two barriers per column.
constexpr int SGS_BIG_NT = 256;
constexpr int SGS_BIG_LDS_DOUBLES = 16384 + 256;   // packed triangle + the right-hand side of <= 180 neighbours
constexpr int SGS_BIG_MAX_K = 1024;

template <int DIM>
__global__ __launch_bounds__(SGS_BIG_NT) void sgs_weights_big_kernel(
    VgDev vg, const double* __restrict__ cent, const int* __restrict__ rank, int64_t N, int k, int minneighbors,
    const int* __restrict__ idx, const int* __restrict__ count, int* __restrict__ ncond, double* __restrict__ w_out,
    double* __restrict__ sigma_out, int* __restrict__ idx_rw, double* __restrict__ scratch, int64_t slab, int use_lds) {
  extern __shared__ double sgs_big_sm[];
  __shared__ int s_cnt, s_bad;
  __shared__ double s_red[SGS_BIG_NT / 64];
  const int tid = threadIdx.x;
  const double smarg = sqrt(vg.sill);
  for (int64_t p = blockIdx.x; p < N; p += gridDim.x) {
    __syncthreads();  // the previous node's shared words have been read
    if (rank[p] < 0) {  // data cell; its list is empty
      for (int j = tid; j < k; j += SGS_BIG_NT) idx_rw[p * k + j] = -1;
      sgs_no_weights(tid == 0, p, 0.0, ncond, sigma_out);
      continue;
    }
    if (tid < 64) {  // keep, in order, the neighbours already simulated when the node is visited
      const int cnt0 = count[p];
      const int rp = rank[p];
      int off = 0;
      for (int base = 0; base < cnt0; base += 64) {
        const SgsKept kp = sgs_keep_pass(idx + p * k, base + tid, cnt0, rank, rp, tid);
        if (kp.keep) idx_rw[p * k + off + kp.slot] = kp.nb;
        off += kp.total;
      }
      for (int j = off + tid; j < k; j += 64) idx_rw[p * k + j] = -1;
      if (tid == 0) {
        s_cnt = off;
        s_bad = 0;
      }
    }
    __syncthreads();
    const int c = s_cnt;
    if (c < minneighbors || c <= 0) {
      sgs_no_weights(tid == 0, p, smarg, ncond, sigma_out);
      continue;
    }
    const int* nb = idx_rw + p * k;
    double* M = use_lds ? sgs_big_sm : scratch + (int64_t)blockIdx.x * slab;
    const int ntri = c * (c + 1) / 2;
    double* b = M + ntri;
    double c0[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) c0[a] = cent[p * DIM + a];
    for (int e = tid; e < ntri; e += SGS_BIG_NT) {
      int i, j;
      sgs_tri_decode(e, &i, &j);
      const int ni = nb[i], nj = nb[j];
      double xi[DIM], xj[DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        xi[a] = cent[(int64_t)ni * DIM + a];
        xj[a] = cent[(int64_t)nj * DIM + a];
      }
      M[e] = cov_pair<DIM>(vg, xi, xj);
    }
    for (int j = tid; j < c; j += SGS_BIG_NT) {
      double xj[DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a) xj[a] = cent[(int64_t)nb[j] * DIM + a];
      b[j] = cov_pair<DIM>(vg, xj, c0);
    }
    __syncthreads();
    // Cholesky, left-looking by columns; rows are dealt to the threads
    for (int j = 0; j < c; ++j) {
      const double* rowj = M + sgs_tri(j);
      for (int i = j + tid; i < c; i += SGS_BIG_NT) {
        double* rowi = M + sgs_tri(i);
        double acc = rowi[j];
        for (int q = 0; q < j; ++q) acc = fma(-rowi[q], rowj[q], acc);
        rowi[j] = acc;
      }
      __syncthreads();
      const double d = rowj[j];
      if (!(d > 0.0)) {
        if (tid == 0) s_bad = 1;
        break;   // d is read by every thread alike: the whole workgroup leaves the loop
      }
      __syncthreads();
      const double sq = sqrt(d);
      for (int i = j + tid; i < c; i += SGS_BIG_NT) {
        double* rowi = M + sgs_tri(i);
        rowi[j] = (i == j) ? sq : rowi[j] / sq;
      }
      __syncthreads();
    }
    __syncthreads();
    if (s_bad) {
      sgs_no_weights(tid == 0, p, smarg, ncond, sigma_out);
      continue;
    }
    // y = L^-1 c0 by columns
    for (int j = 0; j < c; ++j) {
      const double yj = b[j] / M[sgs_tri(j) + j];
      __syncthreads();
      if (tid == 0) b[j] = yj;
      for (int i = j + 1 + tid; i < c; i += SGS_BIG_NT) b[i] = fma(-M[sgs_tri(i) + j], yj, b[i]);
      __syncthreads();
    }
    double q = 0.0;
    for (int j = tid; j < c; j += SGS_BIG_NT) q = fma(b[j], b[j], q);
    q = wave_sum(q);
    if ((tid & 63) == 0) s_red[tid >> 6] = q;
    // lambda = L^-T y (row j of L is contiguous)
    for (int j = c - 1; j >= 0; --j) {
      const double lj = b[j] / M[sgs_tri(j) + j];
      __syncthreads();
      if (tid == 0) b[j] = lj;
      const double* rowj = M + sgs_tri(j);
      for (int i = tid; i < j; i += SGS_BIG_NT) b[i] = fma(-rowj[i], lj, b[i]);
      __syncthreads();
    }
    for (int j = tid; j < c; j += SGS_BIG_NT) w_out[p * k + j] = b[j];
    if (tid == 0) {
      double qq = 0.0;
      for (int wv = 0; wv < SGS_BIG_NT / 64; ++wv) qq += s_red[wv];
      const double v = vg.sill - qq;
      ncond[p] = c;
      sigma_out[p] = sqrt(v > 0.0 ? v : 0.0);
    }
  }
}

// what the steps of gss_sgs_create_paths hand to each other (the searcher leaves last: it waits for the stream)
struct SgsStageA {
  Frame fv;   // rotated variogram: covariances on frame coordinates, origin = the first centroid
  Searcher sr;
  const KnnIndex* ix = nullptr;   // NULL: exhaustive search (Haversine), which takes no mask
  int minneighbors = 0;
  // the variants, chosen once: a workgroup per node beyond 64 neighbours; the search writes raw lists (unmasked and
  // shared by every path, or masked in passes of 64) that the weights kernel compacts or moves into the handle's
  bool big = false, raw_lists = false;
  DevBuf cent, bmin, cnt;
  DevBuf rawidx;   // the lists as searched, where the weights kernel writes the handle's
  DevBuf bigscr;   // more than 180 neighbours: covariance triangles of the workgroups of sgs_weights_big_kernel
};

// visiting rank of every cell (-1 = conditioning cell) per path; each path must be a permutation of 0..N-1
static int32_t sgs_host_ranks(const int64_t* path, int64_t P, int64_t N, const int64_t* dlocs, int64_t nd,
                              std::vector<int64_t>* hpath, std::vector<int>* hrank) {
  hpath->assign((size_t)(N * P), 0);
  hrank->assign((size_t)(N * P), INT_MAX);
  int64_t* hp = hpath->data();   // (locals: the stores below then cannot move the vectors' own words)
  for (int64_t pp = 0; pp < P; ++pp) {
    int* rk = hrank->data() + pp * N;
    for (int64_t t = 0; t < N; ++t) {
      const int64_t c = path ? path[pp * N + t] : t;  // LinearPath (seq.jl:33)
      GSS_REQUIRE(c >= 0 && c < N && rk[c] == INT_MAX, "path %lld is not a permutation of the domain (step %lld)",
                  (long long)pp, (long long)t);
      hp[pp * N + t] = c;
      rk[c] = (int)t;
    }
    for (int64_t j = 0; j < nd; ++j) {
      GSS_REQUIRE(dlocs[j] >= 0 && dlocs[j] < N, "data location %lld outside the domain", (long long)dlocs[j]);
      GSS_REQUIRE(rk[dlocs[j]] >= 0, "data location %lld given twice", (long long)dlocs[j]);
      rk[dlocs[j]] = -1;
    }
  }
  return GSS_OK;
}

// the handle's arrays, the centroids on the covariance frame, the samples of the search and its index
static int32_t sgs_upload(gss_sgs* h, SgsStageA* a, const double* centroids, const std::vector<int64_t>& hpath,
                          const std::vector<int>& hrank, const int64_t* dlocs, const double* zdata, hipStream_t s) {
  const int64_t N = h->N, P = h->npaths;
  GSS_TRY(a->cent.alloc(sizeof(double) * (size_t)(N * h->dim)));
  GSS_TRY(h->path.alloc(sizeof(int64_t) * (size_t)(N * P)));
  GSS_TRY(h->rank.alloc(sizeof(int) * (size_t)(N * P)));
  GSS_TRY(h->idx.alloc(sizeof(int) * (size_t)(N * P * h->k)));
  GSS_TRY(h->ncond.alloc(sizeof(int) * (size_t)(N * P)));
  GSS_TRY(a->cnt.alloc(sizeof(int) * (size_t)N));
  GSS_TRY(h->w.alloc(sizeof(double) * (size_t)(N * P * h->k)));
  GSS_TRY(h->sigma.alloc(sizeof(double) * (size_t)(N * P)));
  GSS_HIP(hipMemcpyAsync(a->cent.p, centroids, a->cent.bytes, hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(h->path.p, hpath.data(), h->path.bytes, hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(h->rank.p, hrank.data(), h->rank.bytes, hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemsetAsync(h->w.p, 0, h->w.bytes, s));
  if (h->nd > 0) {
    GSS_TRY(h->dlocs.alloc(sizeof(int64_t) * (size_t)h->nd));
    GSS_TRY(h->zd.alloc(sizeof(double) * (size_t)h->nd));
    GSS_HIP(hipMemcpyAsync(h->dlocs.p, dlocs, h->dlocs.bytes, hipMemcpyHostToDevice, s));
    GSS_HIP(hipMemcpyAsync(h->zd.p, zdata, h->zd.bytes, hipMemcpyHostToDevice, s));
  }
  if (a->fv.on) GSS_TRY(frame_apply_dev(a->fv, a->cent.as<double>(), N, a->cent.as<double>(), s));
  GSS_TRY(a->sr.samples(a->cent.as<double>(), nullptr, N, s, centroids));
  GSS_TRY(a->sr.index(s, &a->ix));
  if (a->ix) GSS_TRY(a->bmin.alloc(sizeof(int) * (size_t)a->ix->nb));
  if (a->raw_lists) GSS_TRY(a->rawidx.alloc(sizeof(int) * (size_t)(N * h->k)));
  return GSS_OK;
}

// neighbour lists, then weights and sigma, of path pp
template <int DIM>
static int32_t sgs_path(gss_sgs* h, SgsStageA* a, int64_t pp, hipStream_t s) {
  const int64_t N = h->N;
  const int k = h->k;
  const int* rk = h->rank.as<int>() + pp * N;
  int* idxp = h->idx.as<int>() + pp * N * k;
  if (a->ix)
    hipLaunchKernelGGL(sgs_batch_minrank_kernel, dim3((unsigned)((a->ix->nb + 3) / 4)), dim3(256), 0, s,
                       a->ix->perm.as<int>(), rk, (int)N, a->ix->nb, a->bmin.as<int>());
  GSS_HIP(hipGetLastError());
  int* lists = a->raw_lists ? a->rawidx.as<int>() : idxp;
  {
    ProfScope ps("sgs_search", s);
    if (!h->filter_after) {
      const KnnMask mask(KnnMask::Rank{rk, rk, a->bmin.as<int>()});
      GSS_TRY(a->sr.query(nullptr, nullptr, N, k, lists, a->cnt.as<int>(), s, &mask));
    } else if (pp == 0) {   // one unmasked search serves every path: k nearest cells of the whole domain
      GSS_TRY(a->sr.query(nullptr, nullptr, N, k, lists, a->cnt.as<int>(), s));
    }
  }
  int* nc = h->ncond.as<int>() + pp * N;
  double* w = h->w.as<double>() + pp * N * k;
  double* sg = h->sigma.as<double>() + pp * N;
  ProfScope ps("sgs_weights", s);
  if (!a->big) {
    hipLaunchKernelGGL((sgs_weights_kernel<DIM>), dim3((unsigned)N), dim3(64), 0, s, h->vg, a->cent.as<double>(), rk, N, k,
                       a->minneighbors, lists, a->cnt.as<int>(), nc, w, sg, idxp, h->filter_after);
  } else {
    // one workgroup per node, grid-stride; the triangle in LDS when it fits, else a slab of HBM per workgroup
    const int64_t need = (int64_t)k * (k + 1) / 2 + k;
    const int use_lds = need <= SGS_BIG_LDS_DOUBLES ? 1 : 0;
    int64_t nwg = N < 1024 ? N : 1024;
    if (!use_lds) {
      const int64_t cap = ((int64_t)1 << 30) / (int64_t)(sizeof(double) * (size_t)need);   // 1 GiB of slabs
      if (nwg > cap) nwg = cap > 1 ? cap : 1;
      if (a->bigscr.bytes < sizeof(double) * (size_t)(need * nwg)) {
        a->bigscr.release();
        GSS_TRY(a->bigscr.alloc(sizeof(double) * (size_t)(need * nwg)));
      }
    }
    h->big = 1;
    h->big_lds = use_lds;
    const size_t lds = use_lds ? sizeof(double) * (size_t)need : 0;
    if (lds > 48 * 1024)
      GSS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sgs_weights_big_kernel<DIM>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((sgs_weights_big_kernel<DIM>), dim3((unsigned)nwg), dim3(SGS_BIG_NT), lds, s, h->vg,
                       a->cent.as<double>(), rk, N, k, a->minneighbors, a->rawidx.as<int>(), a->cnt.as<int>(), nc, w, sg,
                       idxp, a->bigscr.as<double>(), need, use_lds);
  }
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

}  // namespace gss

using namespace gss;

extern "C" {

int32_t gss_sgs_create_paths(gss_sgs_t** out, const gss_variogram_t* vg, double mean, const double* centroids,
                             int64_t N, int32_t dim, const int64_t* path, int64_t npaths, int64_t path_base,
                             const int64_t* dlocs, const double* zdata, int64_t nd, int32_t maxneighbors,
                             int32_t minneighbors, double radius, const double* inv_radii, int32_t flags,
                             void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(out != nullptr, "gss_sgs_create: out is NULL");
  GSS_REQUIRE(npaths >= 1 && path_base >= 0 && (npaths == 1 || path != nullptr), "gss_sgs_create_paths: bad path set");
  *out = nullptr;
  GSS_REQUIRE(vg && centroids, "gss_sgs_create: NULL argument");
  GSS_REQUIRE(N >= 1 && N < INT_MAX && dim >= 1 && dim <= 3, "gss_sgs_create: bad sizes");
  GSS_REQUIRE(nd >= 0 && nd <= N && (nd == 0 || (dlocs && zdata)), "gss_sgs_create: bad conditioning data");
  GSS_REQUIRE(maxneighbors >= 1 && maxneighbors <= N, "maxneighbors %d outside 1..%lld (searcher_ui clamps it, "
              "ui.jl:18-20)", maxneighbors, (long long)N);
  GSS_REQUIRE(maxneighbors <= SGS_BIG_MAX_K, "maxneighbors = %d: at most %d neighbours in SGS", maxneighbors,
              SGS_BIG_MAX_K);
  hipStream_t s = to_stream(stream);
  auto* h = new gss_sgs();
  std::unique_ptr<gss_sgs> guard(h);
  SgsStageA a;
  GSS_REQUIRE(vg_is_stationary(vg), "variogram model must be stationary");  // fft.jl:91, lu.jl:110
  gss_variogram_t plain;
  GSS_TRY(vg_frame_split(vg, &plain, &a.fv));
  GSS_TRY(make_vgdev(&plain, &h->vg));
  GSS_REQUIRE(h->vg.dim == dim, "variogram dimension %d != domain dimension %d", h->vg.dim, dim);
  h->dim = dim;
  h->k = maxneighbors;
  h->N = N;
  h->nd = nd;
  h->mean = mean;
  h->npaths = npaths;
  h->path_base = path_base;
  h->filter_after = (flags & GSS_SGS_MASK_AFTER_SEARCH) ? 1 : 0;
  a.minneighbors = minneighbors;
  a.big = h->k > SGS_MAX_K;
  a.raw_lists = h->filter_after || a.big;
  const int metric = (flags >> GSS_SGS_METRIC_SHIFT) & 7;
  // Haversine(r) (seq.jl:91-98 hands `distance` to the searcher): its ranking key does not depend on r and has no box
  // bounds, so it runs on the exhaustive search -- which exists unmasked only: available with the mask applied to the
  // search result (GSS_SGS_MASK_AFTER_SEARCH, the front-ends' default), not for the masked search
  GSS_REQUIRE(metric == GSS_METRIC_EUCLIDEAN || metric == GSS_METRIC_CITYBLOCK || metric == GSS_METRIC_CHEBYSHEV ||
                  metric == GSS_METRIC_ROTATED_BALL || (metric == GSS_METRIC_HAVERSINE && h->filter_after),
              "gss_sgs_create: search distance %d -- Euclidean, Cityblock or Chebyshev; Haversine only with "
              "GSS_SGS_MASK_AFTER_SEARCH (there is no masked exhaustive search)", metric);
  GSS_TRY(frame_origin(&a.fv, centroids, GSS_MEM_HOST, nullptr));
  GSS_TRY(a.sr.init(metric, 1.0, radius, inv_radii, dim, &a.fv));
  std::vector<int64_t> hpath;
  std::vector<int> hrank;
  GSS_TRY(sgs_host_ranks(path, npaths, N, dlocs, nd, &hpath, &hrank));

  GSS_TRY(sgs_upload(h, &a, centroids, hpath, hrank, dlocs, zdata, s));
  for (int64_t pp = 0; pp < npaths; ++pp) {   // stage A once per visiting order
    int32_t rc = GSS_OK;
    with_dim(dim, [&](auto D) { rc = sgs_path<decltype(D)::value>(h, &a, pp, s); });
    GSS_TRY(rc);
  }
  {
    ProfScope ps("sgs_levels", s);
    GSS_TRY(sgs_build_levels(h, s));
  }
  GSS_HIP(hipStreamSynchronize(s));  // host staging vectors and scratch are released on return
  *out = guard.release();
  return GSS_OK;
}

int32_t gss_sgs_create(gss_sgs_t** out, const gss_variogram_t* vg, double mean, const double* centroids, int64_t N,
                       int32_t dim, const int64_t* path, const int64_t* dlocs, const double* zdata, int64_t nd,
                       int32_t maxneighbors, int32_t minneighbors, double radius, const double* inv_radii,
                       int32_t flags, void* stream) {
  GSS_ENTRY();
  return gss_sgs_create_paths(out, vg, mean, centroids, N, dim, path, 1, 0, dlocs, zdata, nd, maxneighbors, minneighbors,
                              radius, inv_radii, flags, stream);
}

int32_t gss_sgs_destroy(gss_sgs_t* h) {
  GSS_ENTRY();
  delete h;
  return GSS_OK;
}

int32_t gss_sgs_weights(gss_sgs_t* h, int32_t* idx, int32_t* ncond, double* w, double* sigma, int32_t mem,
                        void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  hipStream_t s = to_stream(stream);
  const hipMemcpyKind kind = mem == GSS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  // (the first visiting order when the handle holds several)
  const size_t nk = (size_t)(h->N * h->k), n1 = (size_t)h->N;
  if (idx) GSS_HIP(hipMemcpyAsync(idx, h->idx.p, sizeof(int) * nk, kind, s));
  if (ncond) GSS_HIP(hipMemcpyAsync(ncond, h->ncond.p, sizeof(int) * n1, kind, s));
  if (w) GSS_HIP(hipMemcpyAsync(w, h->w.p, sizeof(double) * nk, kind, s));
  if (sigma) GSS_HIP(hipMemcpyAsync(sigma, h->sigma.p, sizeof(double) * n1, kind, s));
  if (mem == GSS_MEM_HOST) GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

int32_t gss_sgs_schedule(gss_sgs_t* h, int32_t* out, int32_t n) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && out != nullptr, "NULL argument");
  GSS_REQUIRE(n >= GSS_SGS_SCHEDULE_WORDS, "gss_sgs_schedule: room for %d words, %d needed", n, GSS_SGS_SCHEDULE_WORDS);
  const bool team = h->team_chunks > 0;   // (team_rl is chosen before the chunks: it only counts where they exist)
  out[0] = (int32_t)h->npaths;
  out[1] = h->lvl_off.empty() ? 0 : (int32_t)h->lvl_off.size() - 2;
  out[2] = h->team_chunks;
  out[3] = team ? h->team_rl : 0;
  out[4] = team ? h->team_cap : 0;
  out[5] = h->big;
  out[6] = h->big_lds;
  return GSS_OK;
}

}  // extern "C"
