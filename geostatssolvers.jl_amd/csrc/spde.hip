// SPDEGS: Gaussian simulation on a triangle mesh (Lindgren et al. 2011), src/simulation/spde.jl of the reference.
//
//   spde.jl:37-39   B = laplacematrix, M = measurematrix, Delta = inv(M) B     spde_emit_kernel + sort + spde_reduce_kernel
//   spde.jl:56-64   A = kappa^2 I - Delta, Q = A'A / tau^2                      never formed: S = kappa^2 M - B = M A (CSR)
//   spde.jl:67-68   cholesky(Array(Q)), L = inv(U)                             --
//   spde.jl:98-99   z = L w                                                     S z = tau M w by Jacobi-CG (same covariance
//                                                                              tau^2 inv(A) inv(A)'), NB columns interleaved
//   spde.jl:108-109 integrate(vdata) -> element values                          spde_epilogue_kernel: mean of the 3 vertices
//
// Operators: gss.h, "SPDEGS".  Assembly without floating-point atomics: every triangle emits its twelve contributions
// to B under the key row * nv + col, a stable radix sort over the bits the keys use brings equal entries together in
// triangle order, and one thread per distinct entry sums its run in that order.  The vertex masses ride along: slot
// 4k + 2 of a triangle is the diagonal contribution of its vertex k + 1, each vertex of the triangle exactly once.
//
// The solve.  x, r, p, Ap are vertex-major with the NB columns of a block interleaved, so a matrix entry is read once
// per block and a neighbour's NB values are one contiguous segment.  One iteration is two launches in stream order:
//   spde_spmv_kernel    every workgroup sums the r.z and r.r slabs of the previous update in the same order and so
//                       arrives at the same beta, done flag and iteration count per column (workgroup 0 keeps them);
//                       then p = z + beta p is formed on the fly for the row and its neighbours (z = r / diag S),
//                       Ap = S p, and the p.Ap partials go into their slab
//   spde_update_kernel  alpha = (r.z) / (p.Ap) from the slab, x += alpha p, r -= alpha Ap, partials of r.z and r.r
// Every column has its own scalars; one that has converged is skipped by both kernels from then on.  The host reads
// one page-locked word ("all columns done") every SPDE_POLL iterations and nothing else.
#include "gss_internal.h"

#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "philox.h"

namespace gss {

constexpr int SPDE_THREADS = 256;
constexpr int SPDE_GROUPS = 256;   // most workgroups of a CG kernel = rows of a dot-product slab
constexpr int SPDE_POLL = 32;      // iterations between two looks at the "all done" word
constexpr int SPDE_NB_MAX = 32;

// what a check found, packed as (index << 3 | code) and kept by atomicMin: the first offender in index order
enum { SPDE_BAD_INDEX = 1, SPDE_BAD_REPEAT = 2, SPDE_BAD_AREA = 3, SPDE_BAD_COORD = 4, SPDE_BAD_ORPHAN = 5 };
constexpr unsigned long long SPDE_CLEAN = ~0ull;

// Area and the three half cotangents of a triangle with corners P[0..2] (3-vectors, z = 0 in 2-D); w[k] belongs to the
// corner k, opposite the edge (k + 1, k + 2).  Every product and sum is rounded on its own, on the host as on the device.
__host__ __device__ __forceinline__ double tri_geom(const double (*P)[3], double* w) {
#pragma clang fp contract(off)
  const double u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
  const double v[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
  const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
  const double T = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
  for (int k = 0; k < 3; ++k) {
    const double* c = P[k];
    const double* a = P[(k + 1) % 3];
    const double* b = P[(k + 2) % 3];
    const double dot = ((a[0] - c[0]) * (b[0] - c[0]) + (a[1] - c[1]) * (b[1] - c[1])) + (a[2] - c[2]) * (b[2] - c[2]);
    w[k] = 0.5 * (dot / (2.0 * T));
  }
  return T;
}

__global__ __launch_bounds__(256) void spde_coord_check_kernel(const double* __restrict__ x, int64_t n, int dim,
                                                               unsigned long long* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && !(fabs(x[i]) <= DBL_MAX)) atomicMin(err, ((unsigned long long)(i / dim) << 3) | SPDE_BAD_COORD);
}

// triangle t: checks, its 32-bit indices, its area, and the twelve contributions to B (keys, positions, values)
__global__ __launch_bounds__(256) void spde_emit_kernel(const double* __restrict__ x, int dim, int64_t nv,
                                                        const int64_t* __restrict__ tri, int64_t nt,
                                                        int32_t* __restrict__ tri32, double* __restrict__ area,
                                                        unsigned long long* __restrict__ keys, int* __restrict__ pos,
                                                        double* __restrict__ bval,
                                                        unsigned long long* __restrict__ err) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  int bad = 0;
  double w[3] = {0.0, 0.0, 0.0}, T = 0.0;
  if (id[0] < 0 || id[0] >= nv || id[1] < 0 || id[1] >= nv || id[2] < 0 || id[2] >= nv) bad = SPDE_BAD_INDEX;
  else if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) bad = SPDE_BAD_REPEAT;
  else {
    double P[3][3];
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) P[k][a] = a < dim ? x[id[k] * dim + a] : 0.0;
    T = tri_geom(P, w);
    if (!(T > 0.0 && T <= DBL_MAX)) bad = SPDE_BAD_AREA;
  }
  if (bad) atomicMin(err, ((unsigned long long)t << 3) | (unsigned long long)bad);
  area[t] = T;
  for (int k = 0; k < 3; ++k) {
    const unsigned long long a = bad ? 0ull : (unsigned long long)id[(k + 1) % 3];
    const unsigned long long b = bad ? 0ull : (unsigned long long)id[(k + 2) % 3];
    const unsigned long long n = (unsigned long long)nv;
    const int64_t o = 12 * t + 4 * k;
    tri32[3 * t + k] = bad ? 0 : (int32_t)id[k];
    keys[o] = a * n + b;
    keys[o + 1] = b * n + a;
    keys[o + 2] = a * n + a;
    keys[o + 3] = b * n + b;
    bval[o] = bval[o + 1] = bad ? 0.0 : w[k];
    bval[o + 2] = bval[o + 3] = bad ? 0.0 : -w[k];
    for (int j = 0; j < 4; ++j) pos[o + j] = (int)(o + j);
  }
}

__global__ __launch_bounds__(256) void spde_heads_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                         int* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// one thread per distinct (row, col): the run of equal keys summed in sorted (= triangle) order -> CSR entry `rank - 1`
__global__ __launch_bounds__(256) void spde_reduce_kernel(const unsigned long long* __restrict__ keys,
                                                          const int* __restrict__ pos, const int* __restrict__ rank,
                                                          const double* __restrict__ bval,
                                                          const double* __restrict__ area, int64_t n, int64_t nv,
                                                          double kappa2, double tau, int lumped,
                                                          int64_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                          double* __restrict__ val, double* __restrict__ mass,
                                                          double* __restrict__ dinv, double* __restrict__ bscale) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  if (i > 0 && keys[i - 1] == key) return;
  const int64_t row = (int64_t)(key / (unsigned long long)nv), c = (int64_t)(key % (unsigned long long)nv);
  double acc = 0.0, m = 0.0;
  for (int64_t j = i; j < n && keys[j] == key; ++j) {
    const int q = pos[j];
    acc += bval[q];
    if (row == c && (q & 3) == 2) m += area[q / 12] / 3.0;
  }
  const int64_t e = rank[i] - 1;
  col[e] = (int32_t)c;
  if (row == c) {
    const double s = kappa2 * m - acc;
    val[e] = s;
    mass[row] = m;
    dinv[row] = 1.0 / s;
    bscale[row] = lumped ? tau * sqrt(m) : tau * m;
  } else {
    val[e] = -acc;
  }
  if (i == 0 || (int64_t)(keys[i - 1] / (unsigned long long)nv) != row) rowptr[row] = e;
}

__global__ __launch_bounds__(256) void spde_orphan_kernel(const int64_t* __restrict__ rowptr, int64_t nv,
                                                          unsigned long long* __restrict__ err) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < nv && rowptr[v] < 0) atomicMin(err, ((unsigned long long)v << 3) | SPDE_BAD_ORPHAN);
}

// ---------------------------------------------------------------------------------------------
// conjugate gradients on NB interleaved columns
// ---------------------------------------------------------------------------------------------
struct CgCol {
  double rho;    // r.z of the current residual
  double beta;   // for the direction this iteration forms
  double bn2;    // ||b||^2
  double rr;     // ||r||^2, frozen when the column is done
  int done;
  int iters;     // updates the column has had when it was found converged (or when the solve gave up)
};

// the direction a column takes at vertex v: p = z + beta p_old with z = r / diag(S)
__device__ __forceinline__ double cg_direction(double dinv, double r, double beta, double p_old) {
  return fma(beta, p_old, dinv * r);
}

// Sum of one slab column: thread (g, c) adds the partials g, g + G, .. in order, lane c < NB adds the G sums in order.
// Every workgroup of every kernel that needs a dot product calls this and gets the same bits.
template <int NB>
__device__ __forceinline__ void slab_partial(const double* __restrict__ slab, int ngroups, double* sh) {
  constexpr int G = SPDE_THREADS / NB;
  const int c = threadIdx.x % NB, g = threadIdx.x / NB;
  double a = 0.0;
  for (int q = g; q < ngroups; q += G) a += slab[q * NB + c];
  sh[threadIdx.x] = a;
}
template <int NB>
__device__ __forceinline__ double slab_total(const double* sh) {   // threadIdx.x < NB, after a barrier
  constexpr int G = SPDE_THREADS / NB;
  double a = 0.0;
  for (int q = 0; q < G; ++q) a += sh[q * NB + threadIdx.x];
  return a;
}

// The per-column decisions of iteration k (k updates done so far), into mine[0 .. NB).
template <int NB>
__device__ __forceinline__ void cg_head(const double* __restrict__ slab_rz, const double* __restrict__ slab_rr,
                                        int ngroups, const CgCol* __restrict__ prev, int k, double tol2, double* sh,
                                        CgCol* mine) {
  slab_partial<NB>(slab_rz, ngroups, sh);
  slab_partial<NB>(slab_rr, ngroups, sh + SPDE_THREADS);
  __syncthreads();
  if (threadIdx.x < NB) {
    const double rz = slab_total<NB>(sh), rr = slab_total<NB>(sh + SPDE_THREADS);
    CgCol o;
    if (k == 0) {
      o.rho = 1.0; o.beta = 0.0; o.bn2 = rr; o.rr = rr; o.done = 0; o.iters = 0;
    } else {
      o = prev[threadIdx.x];
    }
    if (!o.done) {
      o.beta = k == 0 ? 0.0 : rz / o.rho;
      o.rho = rz;
      o.rr = rr;
      o.iters = k;
      if (rr <= tol2 * o.bn2) o.done = 1;
    }
    mine[threadIdx.x] = o;
  }
  __syncthreads();
}

template <int NB>
__global__ __launch_bounds__(SPDE_THREADS) void spde_spmv_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const double* __restrict__ val,
    const double* __restrict__ dinv, const double* __restrict__ r, const double* __restrict__ p_old,
    double* __restrict__ p_new, double* __restrict__ Ap, const double* __restrict__ slab_rz,
    const double* __restrict__ slab_rr, double* __restrict__ slab_pap, const CgCol* __restrict__ prev,
    CgCol* __restrict__ next, int k, double tol2, int64_t nv, int* __restrict__ all_done) {
  constexpr int G = SPDE_THREADS / NB;
  __shared__ double sh[2 * SPDE_THREADS];
  __shared__ CgCol mine[NB];
  cg_head<NB>(slab_rz, slab_rr, (int)gridDim.x, prev, k, tol2, sh, mine);
  bool all = true;
  for (int c = 0; c < NB; ++c) all = all && mine[c].done != 0;
  if (blockIdx.x == 0) {
    if (threadIdx.x < NB) next[threadIdx.x] = mine[threadIdx.x];
    if (threadIdx.x == 0) *all_done = all ? 1 : 0;
  }
  if (all) return;
  const int c = threadIdx.x % NB, g = threadIdx.x / NB;
  const bool live = mine[c].done == 0;
  const double beta = mine[c].beta;
  double part = 0.0;
  if (live) {
    for (int64_t v = (int64_t)blockIdx.x * G + g; v < nv; v += (int64_t)gridDim.x * G) {
      const int64_t j1 = rowptr[v + 1];
      double acc = 0.0, pv = 0.0;
      for (int64_t j = rowptr[v]; j < j1; ++j) {
        const int64_t u = col[j];
        const double pu = cg_direction(dinv[u], r[u * NB + c], beta, p_old[u * NB + c]);
        acc = fma(val[j], pu, acc);
        if (u == v) pv = pu;
      }
      p_new[v * NB + c] = pv;
      Ap[v * NB + c] = acc;
      part = fma(pv, acc, part);
    }
  }
  sh[threadIdx.x] = part;
  __syncthreads();
  if (threadIdx.x < NB) slab_pap[blockIdx.x * NB + threadIdx.x] = slab_total<NB>(sh);
}

// FIRST: only the dot products of the right-hand side (x = 0, r = b)
template <int NB, bool FIRST>
__global__ __launch_bounds__(SPDE_THREADS) void spde_update_kernel(
    const double* __restrict__ dinv, double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
    const double* __restrict__ Ap, const double* __restrict__ slab_pap, const CgCol* __restrict__ state,
    double* __restrict__ slab_rz, double* __restrict__ slab_rr, int64_t nv) {
  __shared__ double sh[2 * SPDE_THREADS];
  __shared__ double alpha_s[NB];
  __shared__ int done_s[NB];
  const int c = threadIdx.x % NB;
  bool live = true;
  double alpha = 0.0;
  if (!FIRST) {
    slab_partial<NB>(slab_pap, (int)gridDim.x, sh);
    __syncthreads();
    if (threadIdx.x < NB) {
      const CgCol st = state[threadIdx.x];
      done_s[threadIdx.x] = st.done;
      alpha_s[threadIdx.x] = st.done ? 0.0 : st.rho / slab_total<NB>(sh);
    }
    __syncthreads();
    bool all = true;
    for (int q = 0; q < NB; ++q) all = all && done_s[q] != 0;
    if (all) return;
    live = done_s[c] == 0;
    alpha = alpha_s[c];
    __syncthreads();   // sh is reused below
  }
  double prz = 0.0, prr = 0.0;
  if (live) {
    const int64_t n = nv * NB;
    for (int64_t i = (int64_t)blockIdx.x * SPDE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SPDE_THREADS) {
      double ri = r[i];
      if (!FIRST) {
        x[i] = fma(alpha, p[i], x[i]);
        ri = fma(-alpha, Ap[i], ri);
        r[i] = ri;
      }
      const double z = dinv[i / NB] * ri;
      prz = fma(ri, z, prz);
      prr = fma(ri, ri, prr);
    }
  }
  sh[threadIdx.x] = prz;
  sh[SPDE_THREADS + threadIdx.x] = prr;
  __syncthreads();
  if (threadIdx.x < NB) {
    slab_rz[blockIdx.x * NB + threadIdx.x] = slab_total<NB>(sh);
    slab_rr[blockIdx.x * NB + threadIdx.x] = slab_total<NB>(sh + SPDE_THREADS);
  }
}

// after the last update: the decisions the next iteration would have started with (one workgroup)
template <int NB>
__global__ __launch_bounds__(SPDE_THREADS) void spde_finish_kernel(const double* __restrict__ slab_rz,
                                                                   const double* __restrict__ slab_rr, int ngroups,
                                                                   const CgCol* __restrict__ prev,
                                                                   CgCol* __restrict__ next, int k, double tol2) {
  __shared__ double sh[2 * SPDE_THREADS];
  __shared__ CgCol mine[NB];
  cg_head<NB>(slab_rz, slab_rr, ngroups, prev, k, tol2, sh, mine);
  if (threadIdx.x < NB) next[threadIdx.x] = mine[threadIdx.x];
}

// r = b = bscale w for the nb columns of the block (zero beyond), one thread per vertex: the normals are read (or
// drawn) realisation-major, the block is written as one contiguous row per vertex
template <int NB>
__global__ __launch_bounds__(256) void spde_rhs_kernel(const double* __restrict__ noise, uint64_t seed,
                                                       int64_t first_real, int nb, const double* __restrict__ bscale,
                                                       int64_t nv, double* __restrict__ r) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const double s = bscale[v];
  for (int c = 0; c < NB; ++c) {
    double w = 0.0;
    if (c < nb) w = noise ? noise[(int64_t)c * nv + v] : philox_normal(seed, (uint32_t)(first_real + c), (uint64_t)v);
    r[v * NB + c] = c < nb ? s * w : 0.0;
  }
}

// thread i: vertex i of vout (realisation-major) and element i of eout (the mean of its three vertex values)
template <int NB>
__global__ __launch_bounds__(256) void spde_epilogue_kernel(const double* __restrict__ x, int nb, int64_t nv,
                                                            const int32_t* __restrict__ tri, int64_t nt,
                                                            double* __restrict__ vout, double* __restrict__ eout) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vout && i < nv)
    for (int c = 0; c < nb; ++c) vout[(int64_t)c * nv + i] = x[i * NB + c];
  if (eout && i < nt) {
    const int64_t a = tri[3 * i], b = tri[3 * i + 1], d = tri[3 * i + 2];
    for (int c = 0; c < nb; ++c) eout[(int64_t)c * nt + i] = ((x[a * NB + c] + x[b * NB + c]) + x[d * NB + c]) / 3.0;
  }
}

// the page-locked word the spmv kernel of workgroup 0 writes and the host reads every SPDE_POLL iterations (one per
// process: the library's lock admits one call at a time)
static int* g_spde_done = nullptr;
void spde_release() {
  if (g_spde_done) (void)hipHostFree(g_spde_done);
  g_spde_done = nullptr;
}

static int spde_block_columns() {   // columns per block: 16; GSS_SPDE_NB = 8 or 32 for measurements
  static const int nb = [] {
    const char* e = std::getenv("GSS_SPDE_NB");
    const int v = e ? std::atoi(e) : 16;
    return (v == 8 || v == 32) ? v : 16;
  }();
  return nb;
}

}  // namespace gss

using namespace gss;

struct gss_spde {
  int64_t nv = 0, nt = 0, nnz = 0;
  int dim = 0, lumped = 0;
  double kappa2 = 0.0, tau2 = 0.0;
  DevBuf tri;                      // nt x 3, 32-bit
  DevBuf rowptr, col, val;         // CSR of S
  DevBuf mass, dinv, bscale;       // diag(M), 1 / diag(S), tau m or tau sqrt(m)
  int64_t last_iters = 0, last_unconverged = 0;
  double last_relres = 0.0;
};

static const char* spde_what(int code) {
  switch (code) {
    case SPDE_BAD_INDEX: return "has a vertex index outside [0, nv)";
    case SPDE_BAD_REPEAT: return "repeats a vertex";
    case SPDE_BAD_AREA: return "has no area";
    case SPDE_BAD_COORD: return "has a coordinate that is not finite";
    default: return "belongs to no triangle (the mass matrix is singular)";
  }
}

static int32_t spde_refuse(unsigned long long word) {
  const int code = (int)(word & 7);
  set_error("gss_spde_create: %s %lld %s", code >= SPDE_BAD_COORD ? "vertex" : "triangle", (long long)(word >> 3),
            spde_what(code));
  return GSS_ERR_INVALID;
}

// the checks of the device path on host arrays, without a device
static int32_t spde_check_host(const double* x, int64_t nv, int dim, const int64_t* tri, int64_t nt) {
  for (int64_t i = 0; i < nv * dim; ++i)
    if (!(std::fabs(x[i]) <= DBL_MAX)) return spde_refuse(((unsigned long long)(i / dim) << 3) | SPDE_BAD_COORD);
  std::vector<char> used((size_t)nv, 0);
  for (int64_t t = 0; t < nt; ++t) {
    const int64_t* id = tri + 3 * t;
    int bad = 0;
    if (id[0] < 0 || id[0] >= nv || id[1] < 0 || id[1] >= nv || id[2] < 0 || id[2] >= nv) bad = SPDE_BAD_INDEX;
    else if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) bad = SPDE_BAD_REPEAT;
    else {
      double P[3][3], w[3];
      for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) P[k][a] = a < dim ? x[id[k] * dim + a] : 0.0;
      const double T = tri_geom(P, w);
      if (!(T > 0.0 && T <= DBL_MAX)) bad = SPDE_BAD_AREA;
    }
    if (bad) return spde_refuse(((unsigned long long)t << 3) | (unsigned long long)bad);
    used[(size_t)id[0]] = used[(size_t)id[1]] = used[(size_t)id[2]] = 1;
  }
  for (int64_t v = 0; v < nv; ++v)
    if (!used[(size_t)v]) return spde_refuse(((unsigned long long)v << 3) | SPDE_BAD_ORPHAN);
  return GSS_OK;
}

static int32_t spde_read_err(const DevBuf& err, hipStream_t s, unsigned long long* word) {
  GSS_HIP(hipMemcpyAsync(word, err.p, sizeof(*word), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

static int32_t spde_assemble(gss_spde* h, const double* x, const int64_t* tri, double tau, hipStream_t s) {
  ProfScope ps("spde_assemble", s);
  const int64_t nv = h->nv, nt = h->nt, n = 12 * nt;
  DevBuf err, area, bval, key[2], pos[2], head, rank, tmp;
  GSS_TRY(err.alloc(sizeof(unsigned long long)));
  GSS_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(spde_coord_check_kernel, dim3(blocks_of(nv * h->dim)), dim3(256), 0, s, x, nv * h->dim, h->dim,
                     err.as<unsigned long long>());
  GSS_HIP(hipGetLastError());
  unsigned long long word = SPDE_CLEAN;
  GSS_TRY(spde_read_err(err, s, &word));
  if (word != SPDE_CLEAN) return spde_refuse(word);

  GSS_TRY(h->tri.alloc(sizeof(int32_t) * (size_t)(3 * nt)));
  GSS_TRY(area.alloc(sizeof(double) * (size_t)nt));
  GSS_TRY(bval.alloc(sizeof(double) * (size_t)n));
  for (int i = 0; i < 2; ++i) {
    GSS_TRY(key[i].alloc(sizeof(unsigned long long) * (size_t)n));
    GSS_TRY(pos[i].alloc(sizeof(int) * (size_t)n));
  }
  hipLaunchKernelGGL(spde_emit_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, x, h->dim, nv, tri, nt,
                     h->tri.as<int32_t>(), area.as<double>(), key[0].as<unsigned long long>(), pos[0].as<int>(),
                     bval.as<double>(), err.as<unsigned long long>());
  GSS_HIP(hipGetLastError());
  GSS_TRY(spde_read_err(err, s, &word));
  if (word != SPDE_CLEAN) return spde_refuse(word);

  // equal (row, col) together, triangle order kept: a stable sort over the bits of nv * nv - 1
  int bits = 1;
  while (bits < 64 && (((unsigned long long)nv * (unsigned long long)nv - 1) >> bits) != 0) ++bits;
  hipcub::DoubleBuffer<unsigned long long> keys(key[0].as<unsigned long long>(), key[1].as<unsigned long long>());
  hipcub::DoubleBuffer<int> vals(pos[0].as<int>(), pos[1].as<int>());
  size_t sort_bytes = 0, scan_bytes = 0;
  GSS_TRY(head.alloc(sizeof(int) * (size_t)n));
  GSS_TRY(rank.alloc(sizeof(int) * (size_t)n));
  GSS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, vals, (int)n, 0, bits, s));
  GSS_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, head.as<int>(), rank.as<int>(), (int)n, s));
  GSS_TRY(tmp.alloc(sort_bytes > scan_bytes ? sort_bytes : scan_bytes));
  {
    ProfScope pss("spde_sort", s);
    size_t tb = sort_bytes;
    GSS_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, keys, vals, (int)n, 0, bits, s));
  }
  hipLaunchKernelGGL(spde_heads_kernel, dim3(blocks_of(n)), dim3(256), 0, s, keys.Current(), n, head.as<int>());
  GSS_HIP(hipGetLastError());
  {
    size_t tb = scan_bytes;
    GSS_HIP(hipcub::DeviceScan::InclusiveSum(tmp.p, tb, head.as<int>(), rank.as<int>(), (int)n, s));
  }
  int nnz = 0;
  GSS_HIP(hipMemcpyAsync(&nnz, rank.as<int>() + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  h->nnz = nnz;

  GSS_TRY(h->rowptr.alloc(sizeof(int64_t) * (size_t)(nv + 1)));
  GSS_TRY(h->col.alloc(sizeof(int32_t) * (size_t)nnz));
  GSS_TRY(h->val.alloc(sizeof(double) * (size_t)nnz));
  GSS_TRY(h->mass.alloc(sizeof(double) * (size_t)nv));
  GSS_TRY(h->dinv.alloc(sizeof(double) * (size_t)nv));
  GSS_TRY(h->bscale.alloc(sizeof(double) * (size_t)nv));
  GSS_HIP(hipMemsetAsync(h->rowptr.p, 0xFF, sizeof(int64_t) * (size_t)nv, s));   // -1: a row without entries
  const int64_t nnz64 = nnz;
  GSS_HIP(hipMemcpyAsync(h->rowptr.as<int64_t>() + nv, &nnz64, sizeof(int64_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(spde_reduce_kernel, dim3(blocks_of(n)), dim3(256), 0, s, keys.Current(), vals.Current(),
                     rank.as<int>(), bval.as<double>(), area.as<double>(), n, nv, h->kappa2, tau, h->lumped,
                     h->rowptr.as<int64_t>(), h->col.as<int32_t>(), h->val.as<double>(), h->mass.as<double>(),
                     h->dinv.as<double>(), h->bscale.as<double>());
  GSS_HIP(hipGetLastError());
  hipLaunchKernelGGL(spde_orphan_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, h->rowptr.as<int64_t>(), nv,
                     err.as<unsigned long long>());
  GSS_HIP(hipGetLastError());
  GSS_TRY(spde_read_err(err, s, &word));   // (also: nnz64 has left the stack, the scratch may go back to the pool)
  if (word != SPDE_CLEAN) return spde_refuse(word);
  return GSS_OK;
}

// what one block of columns left behind
struct SpdeBlockResult {
  CgCol colstate[SPDE_NB_MAX];
};

// Realisations first_real .. first_real + nb - 1 (nb <= NB) as one block; every array in HBM.  Returns after the
// block's column states have reached the host (the one wait besides the polls).
template <int NB>
static int32_t spde_solve_block(gss_spde* h, uint64_t seed, int64_t first_real, int nb, const double* noise,
                                double tol2, int64_t maxiter, double* vout, double* eout, double* work, CgCol* state,
                                int* done_dev, SpdeBlockResult* res, hipStream_t s) {
  const int64_t nv = h->nv, nt = h->nt;
  constexpr int G = SPDE_THREADS / NB;
  int64_t want = (nv + G - 1) / G, wantu = (nv * NB + SPDE_THREADS - 1) / SPDE_THREADS;
  if (wantu > want) want = wantu;
  const unsigned groups = (unsigned)(want < SPDE_GROUPS ? want : SPDE_GROUPS);   // a function of nv alone
  const size_t vec = (size_t)nv * NB;
  double *x = work, *r = x + vec, *P[2] = {r + vec, r + 2 * vec}, *Ap = r + 3 * vec;
  double *slab_rz = Ap + vec, *slab_rr = slab_rz + SPDE_GROUPS * NB, *slab_pap = slab_rr + SPDE_GROUPS * NB;
  GSS_HIP(hipMemsetAsync(x, 0, sizeof(double) * vec, s));
  GSS_HIP(hipMemsetAsync(P[0], 0, sizeof(double) * vec, s));   // beta = 0 multiplies it in the first iteration
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_rhs_kernel<NB>), dim3(blocks_of(nv)), dim3(256), 0, s, noise, seed,
                     first_real, nb, h->bscale.as<double>(), nv, r);
  GSS_HIP(hipGetLastError());
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_update_kernel<NB, true>), dim3(groups), dim3(SPDE_THREADS), 0, s,
                     h->dinv.as<double>(), x, r, nullptr, nullptr, nullptr, nullptr, slab_rz, slab_rr, nv);
  GSS_HIP(hipGetLastError());
  int64_t k = 0;
  {
    ProfScope ps("spde_cg", s);
    for (; k < maxiter; ++k) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_spmv_kernel<NB>), dim3(groups), dim3(SPDE_THREADS), 0, s,
                         h->rowptr.as<int64_t>(), h->col.as<int32_t>(), h->val.as<double>(), h->dinv.as<double>(), r,
                         P[k & 1], P[(k + 1) & 1], Ap, slab_rz, slab_rr, slab_pap, state + (k & 1) * NB,
                         state + ((k + 1) & 1) * NB, (int)k, tol2, nv, done_dev);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_update_kernel<NB, false>), dim3(groups), dim3(SPDE_THREADS), 0, s,
                         h->dinv.as<double>(), x, r, P[(k + 1) & 1], Ap, slab_pap, state + ((k + 1) & 1) * NB, slab_rz,
                         slab_rr, nv);
      if ((k + 1) % SPDE_POLL == 0) {
        GSS_HIP(hipGetLastError());
        GSS_HIP(hipStreamSynchronize(s));
        if (*static_cast<volatile int*>(g_spde_done)) {
          ++k;
          break;
        }
      }
    }
    GSS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_finish_kernel<NB>), dim3(1), dim3(SPDE_THREADS), 0, s, slab_rz, slab_rr,
                     (int)groups, state + (k & 1) * NB, state + ((k + 1) & 1) * NB, (int)k, tol2);
  GSS_HIP(hipGetLastError());
  GSS_HIP(hipMemcpyAsync(res->colstate, state + ((k + 1) & 1) * NB, sizeof(CgCol) * NB, hipMemcpyDeviceToHost, s));
  const int64_t m = nv > nt ? nv : nt;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_epilogue_kernel<NB>), dim3(blocks_of(m)), dim3(256), 0, s, x, nb, nv,
                     h->tri.as<int32_t>(), nt, vout, eout);
  GSS_HIP(hipGetLastError());
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

// first unconverged realisation of the call and its residual
struct SpdeFailure {
  int64_t real = -1;
  double relres = 0.0;
};

// nreals realisations, every array in HBM, block after block
template <int NB>
static int32_t spde_realize_dev(gss_spde* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                                double tol2, int64_t maxiter, double* vout, double* eout, SpdeFailure* fail,
                                hipStream_t s) {
  const int64_t nv = h->nv, nt = h->nt;
  DevBuf work, state;
  GSS_TRY(work.alloc(sizeof(double) * ((size_t)nv * NB * 5 + (size_t)3 * SPDE_GROUPS * NB)));
  GSS_TRY(state.alloc(sizeof(CgCol) * 2 * NB));
  if (!g_spde_done) GSS_HIP(hipHostMalloc(reinterpret_cast<void**>(&g_spde_done), sizeof(int), hipHostMallocDefault));
  int* done_dev = nullptr;
  GSS_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&done_dev), g_spde_done, 0));
  for (int64_t r0 = 0; r0 < nreals; r0 += NB) {
    const int nb = (int)(nreals - r0 < NB ? nreals - r0 : NB);
    SpdeBlockResult res;
    *g_spde_done = 0;
    GSS_TRY(spde_solve_block<NB>(h, seed, first_real + r0, nb, noise ? noise + r0 * nv : nullptr, tol2, maxiter,
                                 vout ? vout + r0 * nv : nullptr, eout ? eout + r0 * nt : nullptr, work.as<double>(),
                                 state.as<CgCol>(), done_dev, &res, s));
    for (int c = 0; c < nb; ++c) {
      const CgCol& q = res.colstate[c];
      const double rel = q.bn2 > 0.0 ? std::sqrt(q.rr / q.bn2) : (q.rr == 0.0 ? 0.0 : HUGE_VAL);
      if (q.iters > h->last_iters) h->last_iters = q.iters;
      if (!(rel <= h->last_relres)) h->last_relres = rel;
      if (!q.done) {
        ++h->last_unconverged;
        if (fail->real < 0) {
          fail->real = first_real + r0 + c;
          fail->relres = rel;
        }
      }
    }
  }
  return GSS_OK;
}

static int32_t spde_realize_nb(gss_spde* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                               double tol2, int64_t maxiter, double* vout, double* eout, SpdeFailure* fail,
                               hipStream_t s) {
  switch (spde_block_columns()) {
    case 8: return spde_realize_dev<8>(h, seed, first_real, nreals, noise, tol2, maxiter, vout, eout, fail, s);
    case 32: return spde_realize_dev<32>(h, seed, first_real, nreals, noise, tol2, maxiter, vout, eout, fail, s);
    default: return spde_realize_dev<16>(h, seed, first_real, nreals, noise, tol2, maxiter, vout, eout, fail, s);
  }
}

extern "C" {

int32_t gss_spde_create(gss_spde_t** out, const double* vertices, int64_t nv, int32_t dim, const int64_t* triangles,
                        int64_t nt, double sill, double range, int32_t flags, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(out != nullptr, "gss_spde_create: out is NULL");
  *out = nullptr;
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_spde_create: mem = %d", mem);
  GSS_REQUIRE(vertices != nullptr && triangles != nullptr, "gss_spde_create: NULL mesh");
  GSS_REQUIRE(nv >= 3 && nt >= 1, "gss_spde_create: a mesh needs at least 3 vertices and 1 triangle (nv = %lld, nt = %lld)",
              (long long)nv, (long long)nt);
  GSS_REQUIRE(sill > 0.0 && sill <= DBL_MAX, "gss_spde_create: sill must be positive (spde.jl:53), got %g", sill);
  GSS_REQUIRE(range > 0.0 && range <= DBL_MAX, "gss_spde_create: range must be positive (spde.jl:54), got %g", range);
  GSS_REQUIRE(flags == GSS_SPDE_NOISE_REFERENCE || flags == GSS_SPDE_NOISE_LUMPED, "gss_spde_create: flags = %d", flags);
  if (dim != 2 && dim != 3) {
    set_error("gss_spde_create: vertices of dimension %d; a surface mesh has 2 or 3", dim);
    return GSS_ERR_UNSUPPORTED;
  }
  if (nv >= INT32_MAX || nt > (INT32_MAX - 1) / 12) {
    set_error("gss_spde_create: nv = %lld, nt = %lld; the limits are nv < 2^31 - 1 and 12 nt < 2^31", (long long)nv,
              (long long)nt);
    return GSS_ERR_UNSUPPORTED;
  }
  if (mem == GSS_MEM_HOST) GSS_TRY(spde_check_host(vertices, nv, dim, triangles, nt));
  gss_spde* h = new (std::nothrow) gss_spde();
  if (!h) return GSS_ERR_ALLOC;
  struct Guard {
    gss_spde* h;
    ~Guard() { delete h; }
  } guard{h};
  const double kappa = 1.0 / range;
  h->nv = nv;
  h->nt = nt;
  h->dim = dim;
  h->lumped = flags == GSS_SPDE_NOISE_LUMPED;
  h->kappa2 = kappa * kappa;
  h->tau2 = 4.0 * 3.14159265358979323846 * (sill * sill) * h->kappa2;   // spde.jl:63 with d = 2, alpha = 2, nu = 1
  hipStream_t s = to_stream(stream);
  Staged sx, st;
  GSS_TRY(sx.in(vertices, sizeof(double) * (size_t)(nv * dim), mem, s));
  GSS_TRY(st.in(triangles, sizeof(int64_t) * (size_t)(3 * nt), mem, s));
  GSS_TRY(spde_assemble(h, sx.as<double>(), st.as<int64_t>(), std::sqrt(h->tau2), s));
  guard.h = nullptr;
  *out = h;
  return GSS_OK;
}

int32_t gss_spde_destroy(gss_spde_t* h) {
  GSS_ENTRY();
  delete h;
  return GSS_OK;
}

int32_t gss_spde_info(const gss_spde_t* h, int64_t* nv, int64_t* nt, int64_t* nnz, double* tau2) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  if (nv) *nv = h->nv;
  if (nt) *nt = h->nt;
  if (nnz) *nnz = h->nnz;
  if (tau2) *tau2 = h->tau2;
  return GSS_OK;
}

int32_t gss_spde_operator(gss_spde_t* h, int64_t* rowptr, int32_t* col, double* val, double* mass, int32_t mem,
                          void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_spde_operator: mem = %d", mem);
  hipStream_t s = to_stream(stream);
  const hipMemcpyKind kind = mem == GSS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (rowptr) GSS_HIP(hipMemcpyAsync(rowptr, h->rowptr.p, sizeof(int64_t) * (size_t)(h->nv + 1), kind, s));
  if (col) GSS_HIP(hipMemcpyAsync(col, h->col.p, sizeof(int32_t) * (size_t)h->nnz, kind, s));
  if (val) GSS_HIP(hipMemcpyAsync(val, h->val.p, sizeof(double) * (size_t)h->nnz, kind, s));
  if (mass) GSS_HIP(hipMemcpyAsync(mass, h->mass.p, sizeof(double) * (size_t)h->nv, kind, s));
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

int32_t gss_spde_realize(gss_spde_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                         double rtol, int64_t maxiter, double* vout, double* eout, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && nreals >= 0 && first_real >= 0, "gss_spde_realize: bad arguments");
  GSS_REQUIRE(vout != nullptr || eout != nullptr, "gss_spde_realize: neither vout nor eout");
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_spde_realize: mem = %d", mem);
  GSS_REQUIRE(first_real + nreals <= (int64_t)UINT32_MAX, "gss_spde_realize: realisation numbers beyond 2^32 - 1");
  GSS_REQUIRE(rtol < 1.0, "gss_spde_realize: rtol = %g; it must be below 1 (<= 0 selects 1e-10)", rtol);
  if (!(rtol > 0.0)) rtol = 1e-10;
  if (maxiter <= 0) maxiter = 20000;
  GSS_REQUIRE(maxiter <= INT32_MAX, "gss_spde_realize: maxiter = %lld", (long long)maxiter);
  h->last_iters = h->last_unconverged = 0;
  h->last_relres = 0.0;
  if (nreals == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  const int64_t nv = h->nv, nt = h->nt;
  const double tol2 = rtol * rtol;
  SpdeFailure fail;
  if (mem == GSS_MEM_DEVICE) {
    GSS_TRY(spde_realize_nb(h, seed, first_real, nreals, noise, tol2, maxiter, vout, eout, &fail, s));
  } else {
    // host arrays: chunks of whole blocks through the output ring of the other *_realize calls; chunk b's results
    // cross the bus while chunk b + 1 is solved
    const int64_t NB = spde_block_columns();
    int64_t rb = OutStream::default_chunk(sizeof(double) * (size_t)(nv + nt), nreals);
    rb = rb < NB ? NB : rb / NB * NB;
    OutStream osv, ose;
    GSS_TRY(osv.begin(vout, sizeof(double) * (size_t)nv, nreals, mem, s, rb));
    GSS_TRY(ose.begin(eout, sizeof(double) * (size_t)nt, nreals, mem, s, rb));
    DevBuf nbuf;
    if (noise) GSS_TRY(nbuf.alloc(sizeof(double) * (size_t)((nreals < rb ? nreals : rb) * nv)));
    for (int64_t r0 = 0; r0 < nreals; r0 += rb) {
      const int64_t n = nreals - r0 < rb ? nreals - r0 : rb;
      if (noise)
        GSS_HIP(hipMemcpyAsync(nbuf.p, noise + r0 * nv, sizeof(double) * (size_t)(n * nv), hipMemcpyHostToDevice, s));
      double *dv = nullptr, *de = nullptr;
      if (vout) GSS_TRY(osv.slot(r0, s, &dv));
      if (eout) GSS_TRY(ose.slot(r0, s, &de));
      GSS_TRY(spde_realize_nb(h, seed, first_real + r0, n, noise ? nbuf.as<double>() : nullptr, tol2, maxiter, dv, de,
                              &fail, s));
      GSS_TRY(osv.done(r0 + n - 1, s));
      GSS_TRY(ose.done(r0 + n - 1, s));
    }
    GSS_TRY(osv.finish(s));
    GSS_TRY(ose.finish(s));
  }
  if (fail.real >= 0) {
    set_error("gss_spde_realize: realisation %lld did not reach rtol = %g in %lld iterations (||r|| / ||b|| = %.3g; %lld "
              "of the call's %lld columns did not converge)", (long long)fail.real, rtol, (long long)maxiter,
              fail.relres, (long long)h->last_unconverged, (long long)nreals);
    return GSS_ERR_NO_CONVERGENCE;
  }
  return GSS_OK;
}

int32_t gss_spde_last_solve(const gss_spde_t* h, int64_t* iters, double* relres, int64_t* unconverged) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  if (iters) *iters = h->last_iters;
  if (relres) *relres = h->last_relres;
  if (unconverged) *unconverged = h->last_unconverged;
  return GSS_OK;
}

}  // extern "C"
