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
//
// Data (not in the reference; gss.h, "SPDEGS with data"): conditioning by kriging in the data space.  The same CG loop
// (spde_cg_block) solves W = inv(S) P' once per data set; a block of realisations is then the unconditional solve, the
// residuals at the observations, two triangular products with the factor of P Sigma P' + R, the tall-skinny product
// s^2 . (W lambda) (spde_combine_kernel) and a second solve.
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
// (ldn: doubles between two realisations of `noise`: nv, or nv + nd when the handle carries data)
template <int NB>
__global__ __launch_bounds__(256) void spde_rhs_kernel(const double* __restrict__ noise, int64_t ldn, uint64_t seed,
                                                       int64_t first_real, int nb, const double* __restrict__ bscale,
                                                       int64_t nv, double* __restrict__ r) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const double s = bscale[v];
  for (int c = 0; c < NB; ++c) {
    double w = 0.0;
    if (c < nb) w = noise ? noise[(int64_t)c * ldn + v] : philox_normal(seed, (uint32_t)(first_real + c), (uint64_t)v);
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

// ---------------------------------------------------------------------------------------------
// data: observation rows, the data-space system and the correction of a block (gss.h, "SPDEGS with data")
// ---------------------------------------------------------------------------------------------
constexpr int SPDE_LOC_CHUNK = 128;   // fewest triangles one thread of the locate kernel walks
constexpr int SPDE_CMB_ROWS = 256;    // vertices per workgroup of the combine kernel, one per thread
constexpr int SPDE_CMB_JT = 16;       // observations per LDS stage of the combine kernel (34 KiB of W, 2 KiB of lambda)

// Barycentric coordinates l[0..2] of p (of its projection onto the plane when the triangle lies in space) in the
// triangle with corners P[0..2], by signed area ratios relative to P[0]; returns whether all lie in [-tol, 1 + tol].
// *dist: distance of p from the plane, 0 when it is at most tol edge lengths (always in 2-D, where z = 0).
__host__ __device__ __forceinline__ bool tri_locate(const double (*P)[3], const double* p, double tol, double* l,
                                                    double* dist) {
#pragma clang fp contract(off)
  const double u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
  const double v[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
  const double w[3] = {p[0] - P[0][0], p[1] - P[0][1], p[2] - P[0][2]};
  const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double a[3] = {w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]};   // w x v
  const double b[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};   // u x w
  const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  l[1] = ((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]) / nn;
  l[2] = ((b[0] * n[0] + b[1] * n[1]) + b[2] * n[2]) / nn;
  l[0] = (1.0 - l[1]) - l[2];
  const double len = sqrt(sqrt(nn));                                   // sqrt(2 area)
  const double d = fabs((w[0] * n[0] + w[1] * n[1]) + w[2] * n[2]) / sqrt(nn);
  *dist = d <= tol * len ? 0.0 : d;
  const double lo = -tol, hi = 1.0 + tol;
  return l[0] >= lo && l[0] <= hi && l[1] >= lo && l[1] <= hi && l[2] >= lo && l[2] <= hi;
}

__device__ __forceinline__ void spde_corners(const double* __restrict__ x, int dim, const int32_t* __restrict__ tri,
                                             int64_t t, double (*P)[3]) {
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) P[k][a] = a < dim ? x[(int64_t)tri[3 * t + k] * dim + a] : 0.0;
}

// thread (point, chunk): the nearest accepting triangle of the chunk, the lowest index among equally near ones
__global__ __launch_bounds__(256) void spde_locate_kernel(const double* __restrict__ x, int dim,
                                                          const int32_t* __restrict__ tri, int64_t nt, int64_t chunk,
                                                          const double* __restrict__ pts, int64_t np, double tol,
                                                          int64_t* __restrict__ cand_t, double* __restrict__ cand_d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  double p[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < dim; ++a) p[a] = pts[i * dim + a];
  const int64_t t0 = (int64_t)blockIdx.y * chunk, t1 = t0 + chunk < nt ? t0 + chunk : nt;
  int64_t best = -1;
  double bd = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    double P[3][3], l[3], d;
    spde_corners(x, dim, tri, t, P);
    if (tri_locate(P, p, tol, l, &d) && (best < 0 || d < bd)) {
      best = t;
      bd = d;
    }
  }
  cand_t[(int64_t)blockIdx.y * np + i] = best;
  cand_d[(int64_t)blockIdx.y * np + i] = bd;
}

// thread point: the chunks' candidates in ascending order, then the weights in the winner
__global__ __launch_bounds__(256) void spde_locate_pick_kernel(const double* __restrict__ x, int dim,
                                                               const int32_t* __restrict__ tri,
                                                               const double* __restrict__ pts, int64_t np, double tol,
                                                               const int64_t* __restrict__ cand_t,
                                                               const double* __restrict__ cand_d, int nchunks,
                                                               int64_t* __restrict__ out_t, double* __restrict__ out_w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  int64_t best = -1;
  double bd = 0.0;
  for (int q = 0; q < nchunks; ++q) {
    const int64_t t = cand_t[(int64_t)q * np + i];
    const double d = cand_d[(int64_t)q * np + i];
    if (t >= 0 && (best < 0 || d < bd)) {
      best = t;
      bd = d;
    }
  }
  double l[3] = {0.0, 0.0, 0.0};
  if (best >= 0) {
    double p[3] = {0.0, 0.0, 0.0}, P[3][3], d;
    for (int a = 0; a < dim; ++a) p[a] = pts[i * dim + a];
    spde_corners(x, dim, tri, best, P);
    (void)tri_locate(P, p, tol, l, &d);
  }
  out_t[i] = best;
  for (int k = 0; k < 3; ++k) out_w[3 * i + k] = l[k];
}

// r (zeroed) += P' e_j for the nb observations j0 .. of a block: thread c owns column c and adds its row's three
// entries in order (a vertex named twice gets both)
template <int NB>
__global__ __launch_bounds__(64) void spde_obs_rhs_kernel(const int32_t* __restrict__ obs_v,
                                                          const double* __restrict__ obs_w, int64_t j0, int nb,
                                                          double* __restrict__ r) {
  const int c = threadIdx.x;
  if (c >= nb) return;
  for (int k = 0; k < 3; ++k) r[(int64_t)obs_v[3 * (j0 + c) + k] * NB + c] += obs_w[3 * (j0 + c) + k];
}

// the NB solved columns of a block into columns j0 .. j0 + NB - 1 of the row-major W (nv x ndp)
template <int NB>
__global__ __launch_bounds__(256) void spde_w_store_kernel(const double* __restrict__ x, int64_t nv, int64_t ndp,
                                                           int64_t j0, double* __restrict__ W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv * NB) W[(i / NB) * ndp + j0 + i % NB] = x[i];
}

__global__ __launch_bounds__(256) void spde_w_scale_kernel(const double* __restrict__ W, const double* __restrict__ s,
                                                           int64_t nv, int64_t ndp, double* __restrict__ sW) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv * ndp) sW[i] = s[i / ndp] * W[i];
}

// C += diag(r); the diagonal is kept for the pivot test
__global__ __launch_bounds__(256) void spde_gram_diag_kernel(double* __restrict__ C, int64_t nd,
                                                             const double* __restrict__ sqrt_r,
                                                             double* __restrict__ diag) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nd) return;
  double c = C[i + i * nd];
  if (sqrt_r) c = c + sqrt_r[i] * sqrt_r[i];
  C[i + i * nd] = c;
  diag[i] = c;
}

// pivot i of the factorisation is 1 / Li[i][i]^2: one that is not above 64 nd eps of its diagonal entry is rounding
__global__ __launch_bounds__(256) void spde_pivot_kernel(const double* __restrict__ Li, int64_t nd,
                                                         const double* __restrict__ diag,
                                                         unsigned long long* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nd) return;
  const double q = Li[i + i * nd], piv = 1.0 / (q * q);
  if (!(piv > 64.0 * (double)nd * DBL_EPSILON * diag[i]) || !(piv <= DBL_MAX)) atomicMin(err, (unsigned long long)i);
}

// res[i][c] = y_i - mu - (P x)_i - sqrt(r_i) n_(c,i) for the nb realisations of a block, zero beyond; x == NULL: y - mu
// alone.  The normal is read (or drawn) only where r_i > 0.
template <int NB>
__global__ __launch_bounds__(256) void spde_residual_kernel(const double* __restrict__ x,
                                                            const int32_t* __restrict__ obs_v,
                                                            const double* __restrict__ obs_w,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ sqrt_r,
                                                            const double* __restrict__ noise, int64_t ldn,
                                                            uint64_t seed, int64_t first_real, int nb, int64_t nv,
                                                            int64_t nd, double mu, double* __restrict__ res) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nd * NB) return;
  const int64_t i = idx / NB;
  const int c = (int)(idx % NB);
  double v = 0.0;
  if (c < nb) {
    v = y[i] - mu;
    if (x) {
      double px = obs_w[3 * i] * x[(int64_t)obs_v[3 * i] * NB + c];
      px = px + obs_w[3 * i + 1] * x[(int64_t)obs_v[3 * i + 1] * NB + c];
      px = px + obs_w[3 * i + 2] * x[(int64_t)obs_v[3 * i + 2] * NB + c];
      v = v - px;
      const double sr = sqrt_r ? sqrt_r[i] : 0.0;
      if (sr > 0.0) {
        const double n = noise ? noise[(int64_t)c * ldn + nv + i]
                               : philox_normal(seed, (uint32_t)(first_real + c), (uint64_t)(nv + i));
        v = v - sr * n;
      }
    }
  }
  res[idx] = v;
}

// Lt = Li' (both nd x nd, column-major), so that the product with inv(L)' reads along columns as well
__global__ __launch_bounds__(256) void spde_transpose_kernel(const double* __restrict__ Li, int64_t nd,
                                                             double* __restrict__ Lt) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < nd * nd) Lt[q] = Li[(q / nd) + (q % nd) * nd];
}

// out = A in for the NB columns of a block (in, out: nd x NB), A nd x nd column-major and triangular: lower (inv(L)) or
// UPPER (inv(L)', the transposed copy).  Thread i owns row i with its NB sums in registers: the 64 lanes of a wave read
// 64 consecutive words of column j of A, every lane the same words of `in`.  j ascends over the entries of the row's
// triangle and every column has its own sum.
template <int NB, bool UPPER>
__global__ __launch_bounds__(64) void spde_factor_apply_kernel(const double* __restrict__ A, int64_t nd,
                                                               const double* __restrict__ in,
                                                               double* __restrict__ out) {
  const int64_t i0 = (int64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
  const int64_t last = i0 + 63 < nd - 1 ? i0 + 63 : nd - 1;
  const int64_t jlo = UPPER ? i0 : 0, jhi = UPPER ? nd - 1 : last;   // the columns some row of this workgroup meets
  double acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.0;
  for (int64_t j = jlo; j <= jhi; ++j) {
    if (i < nd && (UPPER ? j >= i : j <= i)) {
      const double a = A[i + j * nd];
#pragma unroll
      for (int c = 0; c < NB; ++c) acc[c] = fma(a, in[j * NB + c], acc[c]);
    }
  }
  if (i < nd) {
#pragma unroll
    for (int c = 0; c < NB; ++c) out[i * NB + c] = acc[c];
  }
}

// t[v][c] = s[v]^2 sum_j W[v][j] lambda[j][c]: the tall-skinny product of a block.  A workgroup takes SPDE_CMB_ROWS
// vertices, one per thread, which keeps the NB sums of its vertex in registers.  W goes through LDS in stages of
// SPDE_CMB_JT observations (read once, along its rows; a thread then reads its own row, one word of padding apart) and
// so does lambda (every lane reads the same words).  j ascends and every column has its own sum: a column's bits do not
// depend on its companions.  Bytes: 8 nv ndp read, 8 nv NB written; lambda (8 nd NB) comes from the cache.
template <int NB>
__global__ __launch_bounds__(SPDE_CMB_ROWS) void spde_combine_kernel(const double* __restrict__ W, int64_t ndp,
                                                                      int64_t nd, const double* __restrict__ lam,
                                                                      const double* __restrict__ bscale, int64_t nv,
                                                                      double* __restrict__ t) {
  __shared__ double sW[SPDE_CMB_ROWS * (SPDE_CMB_JT + 1)];
  __shared__ double sL[SPDE_CMB_JT * NB];
  const int64_t v0 = (int64_t)blockIdx.x * SPDE_CMB_ROWS;
  double acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.0;
  for (int64_t j0 = 0; j0 < nd; j0 += SPDE_CMB_JT) {
    for (int q = threadIdx.x; q < SPDE_CMB_ROWS * SPDE_CMB_JT; q += SPDE_CMB_ROWS) {
      const int row = q / SPDE_CMB_JT, jj = q % SPDE_CMB_JT;
      const int64_t v = v0 + row, j = j0 + jj;
      sW[row * (SPDE_CMB_JT + 1) + jj] = (v < nv && j < nd) ? W[v * ndp + j] : 0.0;
    }
    for (int q = threadIdx.x; q < SPDE_CMB_JT * NB; q += SPDE_CMB_ROWS)
      sL[q] = j0 + q / NB < nd ? lam[j0 * NB + q] : 0.0;
    __syncthreads();
    const double* mine = sW + threadIdx.x * (SPDE_CMB_JT + 1);
    for (int jj = 0; jj < SPDE_CMB_JT; ++jj) {
      const double w = mine[jj];
#pragma unroll
      for (int c = 0; c < NB; ++c) acc[c] = fma(w, sL[jj * NB + c], acc[c]);
    }
    __syncthreads();
  }
  const int64_t v = v0 + threadIdx.x;
  if (v < nv) {
    const double s = bscale[v], s2 = s * s;
#pragma unroll
    for (int c = 0; c < NB; ++c) t[v * NB + c] = s2 * acc[c];
  }
}

// spde_epilogue_kernel for a block with data: the vertex value is (xu + xc) + mu (xu == NULL: xc + mu, the mean)
template <int NB>
__global__ __launch_bounds__(256) void spde_epilogue_cond_kernel(const double* __restrict__ xu,
                                                                 const double* __restrict__ xc, double mu, int nb,
                                                                 int64_t nv, const int32_t* __restrict__ tri,
                                                                 int64_t nt, double* __restrict__ vout,
                                                                 double* __restrict__ eout) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  auto at = [&](int64_t v, int c) {
    const double a = xu ? xu[v * NB + c] + xc[v * NB + c] : xc[v * NB + c];
    return a + mu;
  };
  if (vout && i < nv)
    for (int c = 0; c < nb; ++c) vout[(int64_t)c * nv + i] = at(i, c);
  if (eout && i < nt) {
    const int64_t a = tri[3 * i], b = tri[3 * i + 1], d = tri[3 * i + 2];
    for (int c = 0; c < nb; ++c) eout[(int64_t)c * nt + i] = ((at(a, c) + at(b, c)) + at(d, c)) / 3.0;
  }
}

// the page-locked word the spmv kernel of workgroup 0 writes and the host reads every SPDE_POLL iterations (one per
// process: the library's lock admits one call at a time)
static int* g_spde_done = nullptr;
void spde_release() {
  if (g_spde_done) (void)hipHostFree(g_spde_done);
  g_spde_done = nullptr;
}

static int32_t spde_done_word(int** dev) {   // ... and its device address
  if (!g_spde_done) GSS_HIP(hipHostMalloc(reinterpret_cast<void**>(&g_spde_done), sizeof(int), hipHostMallocDefault));
  GSS_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(dev), g_spde_done, 0));
  return GSS_OK;
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
  DevBuf xv;                       // nv x dim vertex coordinates (gss_spde_locate)
  int64_t last_iters = 0, last_unconverged = 0;
  double last_relres = 0.0;
  // data (nd == 0: none)
  int64_t nd = 0, ndp = 0;         // observations; the same rounded up to whole blocks (row length of W)
  double mu = 0.0;
  bool noisy = false;              // some error variance is positive
  DevBuf obs_v, obs_w, yobs;       // nd x 3 (32-bit), nd x 3, nd
  DevBuf sqrt_r;                   // nd
  DevBuf W;                        // nv x ndp row-major: inv(S) P'
  DevBuf Li, Lt;                   // nd x nd column-major: inv(L) of P Sigma P' + R = L L', and its transpose
  void drop_data() {
    nd = ndp = 0;
    mu = 0.0;
    noisy = false;
    obs_v.release(); obs_w.release(); yobs.release(); sqrt_r.release(); W.release(); Li.release(); Lt.release();
  }
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

// The vectors of a block, all nv x NB interleaved, and the dot-product slabs: x, r, two directions, Ap; x2 (handles
// with data only) holds the second solution of a block.
template <int NB>
struct SpdeWork {
  double *x, *r, *P[2], *Ap, *slab_rz, *slab_rr, *slab_pap, *x2;
  static size_t doubles(int64_t nv, bool second) {
    return (size_t)nv * NB * (second ? 6 : 5) + (size_t)3 * SPDE_GROUPS * NB;
  }
  SpdeWork(double* w, int64_t nv, bool second) {
    const size_t vec = (size_t)nv * NB;
    x = w; r = x + vec; P[0] = r + vec; P[1] = r + 2 * vec; Ap = r + 3 * vec;
    slab_rz = Ap + vec; slab_rr = slab_rz + SPDE_GROUPS * NB; slab_pap = slab_rr + SPDE_GROUPS * NB;
    x2 = second ? slab_pap + SPDE_GROUPS * NB : nullptr;
  }
};

// S x = b for the NB columns of a block, b already in wk.r (interleaved; a zero column is done at once): the CG loop,
// then the block's column states on their way to *res.  Everything is queued on s; the caller waits for s before it
// reads *res (the polls of the loop are the only waits in here).
template <int NB>
static int32_t spde_cg_block(gss_spde* h, const SpdeWork<NB>& wk, double* x, double tol2, int64_t maxiter, CgCol* state,
                             int* done_dev, SpdeBlockResult* res, hipStream_t s) {
  const int64_t nv = h->nv;
  constexpr int G = SPDE_THREADS / NB;
  int64_t want = (nv + G - 1) / G, wantu = (nv * NB + SPDE_THREADS - 1) / SPDE_THREADS;
  if (wantu > want) want = wantu;
  const unsigned groups = (unsigned)(want < SPDE_GROUPS ? want : SPDE_GROUPS);   // a function of nv alone
  const size_t vec = (size_t)nv * NB;
  double *r = wk.r, *const *P = wk.P, *Ap = wk.Ap;
  double *slab_rz = wk.slab_rz, *slab_rr = wk.slab_rr, *slab_pap = wk.slab_pap;
  GSS_HIP(hipMemsetAsync(x, 0, sizeof(double) * vec, s));
  GSS_HIP(hipMemsetAsync(P[0], 0, sizeof(double) * vec, s));   // beta = 0 multiplies it in the first iteration
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
  return GSS_OK;
}

// lambda = inv(L)' inv(L) res for the block in `res` (nd x NB), then wk.r = s^2 . (W lambda); tmp: nd x NB
template <int NB>
static int32_t spde_correction_rhs(gss_spde* h, const SpdeWork<NB>& wk, double* res, double* tmp, hipStream_t s) {
  const int64_t nv = h->nv, nd = h->nd;
  const unsigned fb = (unsigned)((nd + 63) / 64);
  {
    ProfScope ps("spde_lambda", s);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_factor_apply_kernel<NB, false>), dim3(fb), dim3(64), 0, s,
                       h->Li.as<double>(), nd, res, tmp);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_factor_apply_kernel<NB, true>), dim3(fb), dim3(64), 0, s,
                       h->Lt.as<double>(), nd, tmp, res);
    GSS_HIP(hipGetLastError());
  }
  ProfScope ps("spde_combine", s);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_combine_kernel<NB>), dim3((unsigned)((nv + SPDE_CMB_ROWS - 1) / SPDE_CMB_ROWS)),
                     dim3(SPDE_CMB_ROWS), 0, s, h->W.as<double>(), h->ndp, nd, res, h->bscale.as<double>(), nv, wk.r);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// Realisations first_real .. first_real + nb - 1 (nb <= NB) as one block; every array in HBM.  Returns after the
// block's column states have reached the host (the one wait besides the polls).  With data: the unconditional solve,
// the residuals at the observations, the data-space solve, the second solve and the sum (res[1]: its column states;
// dwork: 2 nd NB doubles).
template <int NB>
static int32_t spde_solve_block(gss_spde* h, uint64_t seed, int64_t first_real, int nb, const double* noise,
                                double tol2, int64_t maxiter, double* vout, double* eout, const SpdeWork<NB>& wk,
                                double* dwork, CgCol* state, int* done_dev, SpdeBlockResult* res, hipStream_t s) {
  const int64_t nv = h->nv, nt = h->nt, nd = h->nd, ldn = nv + nd;
  const int64_t m = nv > nt ? nv : nt;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_rhs_kernel<NB>), dim3(blocks_of(nv)), dim3(256), 0, s, noise, ldn, seed,
                     first_real, nb, h->bscale.as<double>(), nv, wk.r);
  GSS_HIP(hipGetLastError());
  GSS_TRY(spde_cg_block<NB>(h, wk, wk.x, tol2, maxiter, state, done_dev, &res[0], s));
  if (nd == 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_epilogue_kernel<NB>), dim3(blocks_of(m)), dim3(256), 0, s, wk.x, nb, nv,
                       h->tri.as<int32_t>(), nt, vout, eout);
    GSS_HIP(hipGetLastError());
    GSS_HIP(hipStreamSynchronize(s));
    return GSS_OK;
  }
  double *dres = dwork, *dtmp = dwork + nd * NB;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_residual_kernel<NB>), dim3(blocks_of(nd * NB)), dim3(256), 0, s, wk.x,
                     h->obs_v.as<int32_t>(), h->obs_w.as<double>(), h->yobs.as<double>(),
                     h->noisy ? h->sqrt_r.as<double>() : nullptr, noise, ldn, seed, first_real, nb, nv, nd, h->mu, dres);
  GSS_HIP(hipGetLastError());
  GSS_TRY(spde_correction_rhs<NB>(h, wk, dres, dtmp, s));
  GSS_TRY(spde_cg_block<NB>(h, wk, wk.x2, tol2, maxiter, state, done_dev, &res[1], s));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_epilogue_cond_kernel<NB>), dim3(blocks_of(m)), dim3(256), 0, s, wk.x, wk.x2,
                     h->mu, nb, nv, h->tri.as<int32_t>(), nt, vout, eout);
  GSS_HIP(hipGetLastError());
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

// a column's state into the handle's record of the call; returns its ||r|| / ||b||
static double spde_note_column(gss_spde* h, const CgCol& q) {
  const double rel = q.bn2 > 0.0 ? std::sqrt(q.rr / q.bn2) : (q.rr == 0.0 ? 0.0 : HUGE_VAL);
  if (q.iters > h->last_iters) h->last_iters = q.iters;
  if (!(rel <= h->last_relres)) h->last_relres = rel;
  return rel;
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
  const int64_t nv = h->nv, nt = h->nt, nd = h->nd, ldn = nv + nd;
  DevBuf work, dwork, state;
  GSS_TRY(work.alloc(sizeof(double) * SpdeWork<NB>::doubles(nv, nd > 0)));
  if (nd > 0) GSS_TRY(dwork.alloc(sizeof(double) * (size_t)(2 * nd * NB)));
  GSS_TRY(state.alloc(sizeof(CgCol) * 2 * NB));
  int* done_dev = nullptr;
  GSS_TRY(spde_done_word(&done_dev));
  const SpdeWork<NB> wk(work.as<double>(), nv, nd > 0);
  for (int64_t r0 = 0; r0 < nreals; r0 += NB) {
    const int nb = (int)(nreals - r0 < NB ? nreals - r0 : NB);
    SpdeBlockResult res[2];
    *g_spde_done = 0;
    GSS_TRY(spde_solve_block<NB>(h, seed, first_real + r0, nb, noise ? noise + r0 * ldn : nullptr, tol2, maxiter,
                                 vout ? vout + r0 * nv : nullptr, eout ? eout + r0 * nt : nullptr, wk,
                                 dwork.as<double>(), state.as<CgCol>(), done_dev, res, s));
    for (int c = 0; c < nb; ++c) {   // with data a realisation is two solves: the worse of the two counts
      double rel = spde_note_column(h, res[0].colstate[c]);
      bool done = res[0].colstate[c].done != 0;
      if (nd > 0) {
        const double rel2 = spde_note_column(h, res[1].colstate[c]);
        if (!(rel2 <= rel)) rel = rel2;
        done = done && res[1].colstate[c].done != 0;
      }
      if (!done) {
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

// W = inv(S) P' block after block, then C = (sW)' (sW) + diag(r) with sW = diag(s) W, its factor and the factor's
// inverse.  The observation arrays are on the handle already.  *bad_col: first column of W that did not converge.
template <int NB>
static int32_t spde_condition_dev(gss_spde* h, double tol2, int64_t maxiter, int64_t* bad_col, double* bad_rel,
                                  int64_t* pivot, hipStream_t s) {
  const int64_t nv = h->nv, nd = h->nd, ndp = h->ndp;
  *bad_col = *pivot = -1;
  {
    ProfScope ps("spde_cond_w", s);
    DevBuf work, state;
    GSS_TRY(work.alloc(sizeof(double) * SpdeWork<NB>::doubles(nv, false)));
    GSS_TRY(state.alloc(sizeof(CgCol) * 2 * NB));
    int* done_dev = nullptr;
    GSS_TRY(spde_done_word(&done_dev));
    const SpdeWork<NB> wk(work.as<double>(), nv, false);
    for (int64_t j0 = 0; j0 < ndp; j0 += NB) {
      const int nb = (int)(nd - j0 < NB ? nd - j0 : NB);
      SpdeBlockResult res;
      *g_spde_done = 0;
      GSS_HIP(hipMemsetAsync(wk.r, 0, sizeof(double) * (size_t)nv * NB, s));
      hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_obs_rhs_kernel<NB>), dim3(1), dim3(64), 0, s, h->obs_v.as<int32_t>(),
                         h->obs_w.as<double>(), j0, nb, wk.r);
      GSS_HIP(hipGetLastError());
      GSS_TRY(spde_cg_block<NB>(h, wk, wk.x, tol2, maxiter, state.as<CgCol>(), done_dev, &res, s));
      hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_w_store_kernel<NB>), dim3(blocks_of(nv * NB)), dim3(256), 0, s, wk.x, nv,
                         ndp, j0, h->W.as<double>());
      GSS_HIP(hipGetLastError());
      GSS_HIP(hipStreamSynchronize(s));
      for (int c = 0; c < nb; ++c) {
        const double rel = spde_note_column(h, res.colstate[c]);
        if (!res.colstate[c].done) {
          ++h->last_unconverged;
          if (*bad_col < 0) {
            *bad_col = j0 + c;
            *bad_rel = rel;
          }
        }
      }
    }
    if (*bad_col >= 0) return GSS_OK;
  }
  DevBuf C, diag, scr, info, err;
  GSS_TRY(C.alloc(sizeof(double) * (size_t)(nd * nd)));
  GSS_TRY(h->Li.alloc(sizeof(double) * (size_t)(nd * nd)));
  GSS_TRY(diag.alloc(sizeof(double) * (size_t)nd));
  GSS_TRY(info.alloc(sizeof(int)));
  GSS_TRY(err.alloc(sizeof(unsigned long long)));
  const int64_t ws = potrf_inverse_work_doubles(nd) > nd * nd ? potrf_inverse_work_doubles(nd) : nd * nd;
  GSS_TRY(scr.alloc(sizeof(double) * (size_t)ws));
  for (int attempt = 0;; ++attempt) {
    {
      ProfScope ps("spde_cond_gram", s);
      DevBuf sW;
      if (sW.alloc(sizeof(double) * (size_t)(nv * ndp)) != GSS_OK) {
        set_error("gss_spde_condition: no room for diag(s) W (%lld x %lld doubles) beside W", (long long)nv, (long long)ndp);
        return GSS_ERR_ALLOC;
      }
      hipLaunchKernelGGL(spde_w_scale_kernel, dim3(blocks_of(nv * ndp)), dim3(256), 0, s, h->W.as<double>(),
                         h->bscale.as<double>(), nv, ndp, sW.as<double>());
      GSS_HIP(hipGetLastError());
      GSS_TRY(gemm_f64(nd, nd, nv, 1.0, sW.as<double>(), 1, ndp, sW.as<double>(), ndp, 1, 0.0, C.as<double>(), 1, nd,
                       false, s));
      hipLaunchKernelGGL(spde_gram_diag_kernel, dim3(blocks_of(nd)), dim3(256), 0, s, C.as<double>(), nd,
                         h->noisy ? h->sqrt_r.as<double>() : nullptr, diag.as<double>());
      GSS_HIP(hipGetLastError());
      GSS_HIP(hipStreamSynchronize(s));   // (sW goes back to the pool)
    }
    ProfScope ps("spde_cond_factor", s);
    GSS_HIP(hipMemsetAsync(h->Li.p, 0, sizeof(double) * (size_t)(nd * nd), s));
    GSS_TRY(potrf_inverse_f64(C.as<double>(), nd, nd, h->Li.as<double>(), nd, scr.as<double>(), info.as<int>(), false,
                              s));
    int code = 0;
    GSS_HIP(hipMemcpyAsync(&code, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
    if (code < 0 && attempt == 0) {   // the single-launch panel gave up at a grid barrier: once more without it
      potrf_panel_disable();
      continue;
    }
    if (code < 0) {
      set_error("gss_spde_condition: the factorisation gave up waiting at a grid barrier");
      return GSS_ERR_HIP;
    }
    if (code > 0) {
      *pivot = code - 1;
      return GSS_OK;
    }
    break;
  }
  GSS_HIP(hipMemsetAsync(err.p, 0xFF, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(spde_pivot_kernel, dim3(blocks_of(nd)), dim3(256), 0, s, h->Li.as<double>(), nd, diag.as<double>(),
                     err.as<unsigned long long>());
  GSS_HIP(hipGetLastError());
  unsigned long long word = SPDE_CLEAN;
  GSS_TRY(spde_read_err(err, s, &word));
  if (word != SPDE_CLEAN) {
    *pivot = (int64_t)word;
    return GSS_OK;
  }
  GSS_TRY(h->Lt.alloc(sizeof(double) * (size_t)(nd * nd)));
  hipLaunchKernelGGL(spde_transpose_kernel, dim3(blocks_of(nd * nd)), dim3(256), 0, s, h->Li.as<double>(), nd,
                     h->Lt.as<double>());
  GSS_HIP(hipGetLastError());
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

// the kriging mean: lambda0 = inv(C) (y - mu) in column 0 of a block, one solve, mu added by the epilogue
template <int NB>
static int32_t spde_mean_dev(gss_spde* h, double tol2, int64_t maxiter, double* vout, double* eout, SpdeFailure* fail,
                             hipStream_t s) {
  const int64_t nv = h->nv, nt = h->nt, nd = h->nd;
  DevBuf work, dwork, state;
  GSS_TRY(work.alloc(sizeof(double) * SpdeWork<NB>::doubles(nv, false)));
  GSS_TRY(dwork.alloc(sizeof(double) * (size_t)(2 * nd * NB)));
  GSS_TRY(state.alloc(sizeof(CgCol) * 2 * NB));
  int* done_dev = nullptr;
  GSS_TRY(spde_done_word(&done_dev));
  const SpdeWork<NB> wk(work.as<double>(), nv, false);
  double *dres = dwork.as<double>(), *dtmp = dres + nd * NB;
  SpdeBlockResult res;
  *g_spde_done = 0;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_residual_kernel<NB>), dim3(blocks_of(nd * NB)), dim3(256), 0, s, nullptr,
                     h->obs_v.as<int32_t>(), h->obs_w.as<double>(), h->yobs.as<double>(), nullptr, nullptr, 0, 0, 0, 1,
                     nv, nd, h->mu, dres);
  GSS_HIP(hipGetLastError());
  GSS_TRY(spde_correction_rhs<NB>(h, wk, dres, dtmp, s));
  GSS_TRY(spde_cg_block<NB>(h, wk, wk.x, tol2, maxiter, state.as<CgCol>(), done_dev, &res, s));
  const int64_t m = nv > nt ? nv : nt;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spde_epilogue_cond_kernel<NB>), dim3(blocks_of(m)), dim3(256), 0, s, nullptr, wk.x,
                     h->mu, 1, nv, h->tri.as<int32_t>(), nt, vout, eout);
  GSS_HIP(hipGetLastError());
  GSS_HIP(hipStreamSynchronize(s));
  const double rel = spde_note_column(h, res.colstate[0]);
  if (!res.colstate[0].done) {
    ++h->last_unconverged;
    fail->real = 0;
    fail->relres = rel;
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

static int32_t spde_condition_nb(gss_spde* h, double tol2, int64_t maxiter, int64_t* bad_col, double* bad_rel,
                                 int64_t* pivot, hipStream_t s) {
  switch (spde_block_columns()) {
    case 8: return spde_condition_dev<8>(h, tol2, maxiter, bad_col, bad_rel, pivot, s);
    case 32: return spde_condition_dev<32>(h, tol2, maxiter, bad_col, bad_rel, pivot, s);
    default: return spde_condition_dev<16>(h, tol2, maxiter, bad_col, bad_rel, pivot, s);
  }
}

static int32_t spde_mean_nb(gss_spde* h, double tol2, int64_t maxiter, double* vout, double* eout, SpdeFailure* fail,
                            hipStream_t s) {
  switch (spde_block_columns()) {
    case 8: return spde_mean_dev<8>(h, tol2, maxiter, vout, eout, fail, s);
    case 32: return spde_mean_dev<32>(h, tol2, maxiter, vout, eout, fail, s);
    default: return spde_mean_dev<16>(h, tol2, maxiter, vout, eout, fail, s);
  }
}

// rtol and maxiter as the exports take them -> tol^2 and a positive count
static int32_t spde_solve_args(const char* who, double* rtol, int64_t* maxiter) {
  GSS_REQUIRE(*rtol < 1.0, "%s: rtol = %g; it must be below 1 (<= 0 selects 1e-10)", who, *rtol);
  if (!(*rtol > 0.0)) *rtol = 1e-10;
  if (*maxiter <= 0) *maxiter = 20000;
  GSS_REQUIRE(*maxiter <= INT32_MAX, "%s: maxiter = %lld", who, (long long)*maxiter);
  return GSS_OK;
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
  GSS_TRY(h->xv.alloc(sizeof(double) * (size_t)(nv * dim)));
  GSS_HIP(hipMemcpyAsync(h->xv.p, sx.p, sizeof(double) * (size_t)(nv * dim), hipMemcpyDeviceToDevice, s));
  GSS_HIP(hipStreamSynchronize(s));
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
  const int64_t nv = h->nv, nt = h->nt, ldn = nv + h->nd;   // with data the error normals follow the field's
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
    if (noise) GSS_TRY(nbuf.alloc(sizeof(double) * (size_t)((nreals < rb ? nreals : rb) * ldn)));
    for (int64_t r0 = 0; r0 < nreals; r0 += rb) {
      const int64_t n = nreals - r0 < rb ? nreals - r0 : rb;
      if (noise)
        GSS_HIP(hipMemcpyAsync(nbuf.p, noise + r0 * ldn, sizeof(double) * (size_t)(n * ldn), hipMemcpyHostToDevice, s));
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

int32_t gss_spde_locate(gss_spde_t* h, const double* points, int64_t np, double tol, int64_t* triangle,
                        double* weight, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_spde_locate: mem = %d", mem);
  GSS_REQUIRE(np >= 0 && np <= INT32_MAX, "gss_spde_locate: np = %lld", (long long)np);
  GSS_REQUIRE(tol < 0.5, "gss_spde_locate: tol = %g; it must be below 1/2 (<= 0 selects 1e-9)", tol);
  if (np == 0) return GSS_OK;
  GSS_REQUIRE(points != nullptr && triangle != nullptr && weight != nullptr, "gss_spde_locate: NULL array");
  if (!(tol > 0.0)) tol = 1e-9;
  hipStream_t s = to_stream(stream);
  Staged sp, st, sw;
  GSS_TRY(sp.in(points, sizeof(double) * (size_t)(np * h->dim), mem, s));
  GSS_TRY(st.out(triangle, sizeof(int64_t) * (size_t)np, mem));
  GSS_TRY(sw.out(weight, sizeof(double) * (size_t)(3 * np), mem));
  // a thread walks at least SPDE_LOC_CHUNK triangles and there are at most 1 024 chunks
  int64_t chunk = (h->nt + 1023) / 1024;
  if (chunk < SPDE_LOC_CHUNK) chunk = SPDE_LOC_CHUNK;
  const int nchunks = (int)((h->nt + chunk - 1) / chunk);
  DevBuf ct, cd;
  GSS_TRY(ct.alloc(sizeof(int64_t) * (size_t)(np * nchunks)));
  GSS_TRY(cd.alloc(sizeof(double) * (size_t)(np * nchunks)));
  hipLaunchKernelGGL(spde_locate_kernel, dim3(blocks_of(np), (unsigned)nchunks), dim3(256), 0, s, h->xv.as<double>(),
                     h->dim, h->tri.as<int32_t>(), h->nt, chunk, sp.as<double>(), np, tol, ct.as<int64_t>(),
                     cd.as<double>());
  hipLaunchKernelGGL(spde_locate_pick_kernel, dim3(blocks_of(np)), dim3(256), 0, s, h->xv.as<double>(), h->dim,
                     h->tri.as<int32_t>(), sp.as<double>(), np, tol, ct.as<int64_t>(), cd.as<double>(), nchunks,
                     st.as<int64_t>(), sw.as<double>());
  GSS_HIP(hipGetLastError());
  GSS_TRY(st.back(s));
  GSS_TRY(sw.back(s));
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

int32_t gss_spde_condition_clear(gss_spde_t* h) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_HIP(hipDeviceSynchronize());   // nothing queued reads the data any more
  h->drop_data();
  return GSS_OK;
}

int32_t gss_spde_condition(gss_spde_t* h, int64_t nd, const int64_t* obs_vertex, const double* obs_weight,
                           const double* value, const double* error_var, double mean, double rtol, int64_t maxiter,
                           int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  // The earlier data go first: whatever this call is refused for, the handle has none afterwards.
  if (h->nd > 0) {
    GSS_HIP(hipDeviceSynchronize());   // nothing queued reads them any more
    h->drop_data();
  }
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_spde_condition: mem = %d", mem);
  GSS_REQUIRE(nd >= 1, "gss_spde_condition: nd = %lld; at least one observation", (long long)nd);
  GSS_REQUIRE(obs_vertex != nullptr && obs_weight != nullptr && value != nullptr, "gss_spde_condition: NULL array");
  GSS_REQUIRE(std::fabs(mean) <= DBL_MAX, "gss_spde_condition: the mean is not finite");
  GSS_TRY(spde_solve_args("gss_spde_condition", &rtol, &maxiter));
  if (nd > INT32_MAX / 64) {
    set_error("gss_spde_condition: nd = %lld; the limit is 2^25", (long long)nd);
    return GSS_ERR_UNSUPPORTED;
  }
  hipStream_t s = to_stream(stream);
  // the observation table is small: it is checked on the host wherever it lives
  std::vector<int64_t> hv((size_t)(3 * nd));
  std::vector<double> hw((size_t)(3 * nd)), hy((size_t)nd), hr(error_var ? (size_t)nd : 0);
  if (mem == GSS_MEM_DEVICE) {
    GSS_HIP(hipMemcpyAsync(hv.data(), obs_vertex, sizeof(int64_t) * hv.size(), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipMemcpyAsync(hw.data(), obs_weight, sizeof(double) * hw.size(), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipMemcpyAsync(hy.data(), value, sizeof(double) * hy.size(), hipMemcpyDeviceToHost, s));
    if (error_var) GSS_HIP(hipMemcpyAsync(hr.data(), error_var, sizeof(double) * hr.size(), hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
  } else {
    hv.assign(obs_vertex, obs_vertex + 3 * nd);
    hw.assign(obs_weight, obs_weight + 3 * nd);
    hy.assign(value, value + nd);
    if (error_var) hr.assign(error_var, error_var + nd);
  }
  std::vector<int32_t> v32((size_t)(3 * nd));
  bool noisy = false;
  for (int64_t i = 0; i < nd; ++i) {
    for (int k = 0; k < 3; ++k) {
      const int64_t v = hv[(size_t)(3 * i + k)];
      GSS_REQUIRE(v >= 0 && v < h->nv, "gss_spde_condition: observation %lld has a vertex index outside [0, nv)",
                  (long long)i);
      GSS_REQUIRE(std::fabs(hw[(size_t)(3 * i + k)]) <= DBL_MAX,
                  "gss_spde_condition: observation %lld has a weight that is not finite", (long long)i);
      v32[(size_t)(3 * i + k)] = (int32_t)v;
    }
    GSS_REQUIRE(std::fabs(hy[(size_t)i]) <= DBL_MAX, "gss_spde_condition: observation %lld has a value that is not finite",
                (long long)i);
    if (error_var) {
      const double r = hr[(size_t)i];
      GSS_REQUIRE(std::fabs(r) <= DBL_MAX, "gss_spde_condition: observation %lld has an error variance that is not finite",
                  (long long)i);
      GSS_REQUIRE(r >= 0.0, "gss_spde_condition: observation %lld has a negative error variance (%g)", (long long)i, r);
      noisy = noisy || r > 0.0;
      hr[(size_t)i] = std::sqrt(r);
    }
  }
  struct Guard {
    gss_spde* h;
    ~Guard() { if (h) h->drop_data(); }
  } guard{h};
  const int64_t NB = spde_block_columns();
  h->nd = nd;
  h->ndp = round_up(nd, NB);
  h->mu = mean;
  h->noisy = noisy;
  h->last_iters = h->last_unconverged = 0;
  h->last_relres = 0.0;
  GSS_TRY(h->obs_v.alloc(sizeof(int32_t) * v32.size()));
  GSS_TRY(h->obs_w.alloc(sizeof(double) * hw.size()));
  GSS_TRY(h->yobs.alloc(sizeof(double) * hy.size()));
  GSS_HIP(hipMemcpyAsync(h->obs_v.p, v32.data(), sizeof(int32_t) * v32.size(), hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(h->obs_w.p, hw.data(), sizeof(double) * hw.size(), hipMemcpyHostToDevice, s));
  GSS_HIP(hipMemcpyAsync(h->yobs.p, hy.data(), sizeof(double) * hy.size(), hipMemcpyHostToDevice, s));
  if (noisy) {
    GSS_TRY(h->sqrt_r.alloc(sizeof(double) * hr.size()));
    GSS_HIP(hipMemcpyAsync(h->sqrt_r.p, hr.data(), sizeof(double) * hr.size(), hipMemcpyHostToDevice, s));
  }
  GSS_HIP(hipStreamSynchronize(s));   // the vectors above may go
  if (h->W.alloc(sizeof(double) * (size_t)h->nv * (size_t)h->ndp) != GSS_OK) {
    set_error("gss_spde_condition: W = inv(S) P' does not fit: %lld x %lld doubles (8 nv nd bytes)", (long long)h->nv,
              (long long)h->ndp);
    return GSS_ERR_ALLOC;
  }
  ProfScope ps("spde_condition", s);
  int64_t bad_col = -1, pivot = -1;
  double bad_rel = 0.0;
  GSS_TRY(spde_condition_nb(h, rtol * rtol, maxiter, &bad_col, &bad_rel, &pivot, s));
  if (bad_col >= 0) {
    set_error("gss_spde_condition: the solve for observation %lld did not reach rtol = %g in %lld iterations (||r|| / ||b|| "
              "= %.3g; %lld of the %lld columns did not converge)", (long long)bad_col, rtol, (long long)maxiter, bad_rel,
              (long long)h->last_unconverged, (long long)nd);
    return GSS_ERR_NO_CONVERGENCE;
  }
  if (pivot >= 0) {
    set_error("gss_spde_condition: the data covariance P Sigma P' + R is not positive definite (pivot %lld): two exact "
              "observations of the same quantity, or an observation with zero weights", (long long)pivot);
    return GSS_ERR_NOT_POSDEF;
  }
  guard.h = nullptr;
  return GSS_OK;
}

int32_t gss_spde_condition_info(gss_spde_t* h, int64_t* nd, double* mean, double* W, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_spde_condition_info: mem = %d", mem);
  if (nd) *nd = h->nd;
  if (mean) *mean = h->mu;
  if (W && h->nd > 0) {
    hipStream_t s = to_stream(stream);
    GSS_HIP(hipMemcpy2DAsync(W, sizeof(double) * (size_t)h->nd, h->W.p, sizeof(double) * (size_t)h->ndp,
                             sizeof(double) * (size_t)h->nd, (size_t)h->nv,
                             mem == GSS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
  }
  return GSS_OK;
}

int32_t gss_spde_mean(gss_spde_t* h, double rtol, int64_t maxiter, double* vout, double* eout, int32_t mem,
                      void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(h->nd > 0, "gss_spde_mean: the handle carries no data (gss_spde_condition)");
  GSS_REQUIRE(vout != nullptr || eout != nullptr, "gss_spde_mean: neither vout nor eout");
  GSS_REQUIRE(mem == GSS_MEM_HOST || mem == GSS_MEM_DEVICE, "gss_spde_mean: mem = %d", mem);
  GSS_TRY(spde_solve_args("gss_spde_mean", &rtol, &maxiter));
  h->last_iters = h->last_unconverged = 0;
  h->last_relres = 0.0;
  hipStream_t s = to_stream(stream);
  Staged sv, se;
  GSS_TRY(sv.out(vout, sizeof(double) * (size_t)h->nv, mem));
  GSS_TRY(se.out(eout, sizeof(double) * (size_t)h->nt, mem));
  SpdeFailure fail;
  GSS_TRY(spde_mean_nb(h, rtol * rtol, maxiter, sv.as<double>(), se.as<double>(), &fail, s));
  GSS_TRY(sv.back(s));
  GSS_TRY(se.back(s));
  if (fail.real >= 0) {
    set_error("gss_spde_mean: the solve did not reach rtol = %g in %lld iterations (||r|| / ||b|| = %.3g)", rtol,
              (long long)maxiter, fail.relres);
    return GSS_ERR_NO_CONVERGENCE;
  }
  return GSS_OK;
}

}  // extern "C"
