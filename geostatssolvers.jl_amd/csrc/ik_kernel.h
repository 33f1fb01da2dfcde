// Indicator kriging under a moving neighbourhood, the per-point system (gss.h, gss_ik_predict_knn).
//
// A sibling of K5 (krig_local.hip) built like cokrig_local_kernel.h from the shared pieces, K5 itself untouched: one wave
// per domain point, lane j = neighbour j, four points per workgroup that share the diagonal-tile duty (tile16.h,
// potrf16_inverse_x4), the k x k covariance block in registers as 16 x 16 tiles in the accumulator layout of
// v_mfma_f64_16x16x4_f64, the right-hand sides as columns of B tiles, everything finished from Gram products of the
// forward-substituted columns.  What differs:
//   columns      [c0 | i_0 .. i_{n1-1} | 1] with i_q(j) = (z_j <= c_q) (the simple variant carries i_q - F*_q and no
//                constant column).  The constant column sits at column 15, so one B tile takes n1 = 14 cutoffs under the
//                ordinary variant and 15 under the simple one; the cutoffs beyond n1 are the columns of a SECOND B tile
//                that goes through the same block steps, i.e. through the factors the first one meets: no second
//                factorisation, and no copy of the inverse diagonal factors has to outlive its step.
//   where the columns live   nowhere.  K5 hands its columns over "lane = neighbour" -> tile layout through the wave's own
//                pieces of the factorisation buffers (rhs_col: four columns per piece, three pieces, hence at most 12),
//                which is only safe because every column is read back before the first diagonal tile is written there.
//                Here an indicator entry is a comparison: lane (g, c) forms entry (row, column c) from z[row] (a
//                dedicated 64-double array of the wave) and the cutoff of ITS column, which it holds in a register.  Only
//                c0 crosses lanes, through a dedicated 64-double array.  Neither array aliases S4 or G, so there is no
//                ordering to respect between the columns and the factorisation buffers, for any number of columns.
//   full form    (FULL) one variogram per cutoff: a loop over the cutoffs on the neighbour coordinates, z and list staged
//                once; every pass evaluates its tiles with that cutoff's VgDev (a device table: K records do not fit the
//                kernel arguments), factorises, and finishes the one column [c0_q | i_q | 1].
//   finish       per cutoff q, with y_c, y_q, y_1 the forward-substituted columns:  a = y_c.y_q;  ordinary:
//                S = |y_1|^2, r = y_1.y_c - 1, F_q = a - (r / S) y_1.y_q;  simple: F_q = F*_q + a.  No variance.
//                Then lane q holds cutoff q and the order-relation correction (ik_order16) runs over 16 lanes.
#pragma once

#include "krig_local.h"
#include "tile16.h"

namespace gss {

constexpr int IK_WAVES = 4;
constexpr int IK_MAXK = 16;          // cutoffs
constexpr int IK_TAB = 2 * IK_MAXK;  // device table of a call: cutoffs at 0, F* at IK_MAXK

struct IkSpec {
  int K, ordinary, minneighbors, k;
};

// GSLIB's order-relation correction of a continuous variable over the K values of one point, lane q (of 16 consecutive
// lanes) = cutoff q: clip to [0, 1]; U_q = max(U_{q-1}, F_q) upwards; D_q = min(D_{q+1}, F_q) downwards; (U + D) / 2.
// max and min are exact, so the prefix / suffix scans give the doubles of the sequential passes.  A row with a NaN is
// all NaN.  Every lane of the wave must call it (shuffles); lanes q >= K return garbage.
__device__ __forceinline__ double ik_order16(double f, int q, int K) {
  const bool in = q < K;
  const double x = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);   // (a NaN stays)
  int nan = (in && x != x) ? 1 : 0;
  double u = in ? x : 0.0, d = in ? x : 2.0;
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
    const double tu = __shfl_up(u, off, 16);
    const double td = __shfl_down(d, off, 16);
    nan |= __shfl_xor(nan, off, 16);
    if (q >= off) u = fmax(u, tu);
    if (q + off < 16) d = fmin(d, td);
  }
  const double r = (u + d) * 0.5;
  return nan ? __longlong_as_double(0x7ff8000000000000LL) : r;
}

// one block step on both B tiles (k5_block_step with a second set of columns)
template <int KK, int NT>
__device__ __forceinline__ void ik_block_step(d4_t (&T)[10], d4_t (&B)[4], d4_t (&B2)[4], const d4_t& V, int nt,
                                              bool two) {
  const d4_t zero4 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = KK + 1; j < NT; ++j)
    if (j < nt) T[tile_id(KK, j)] = xty(V, T[tile_id(KK, j)], zero4);
  B[KK] = xty(V, B[KK], zero4);
  if (two) B2[KK] = xty(V, B2[KK], zero4);
#pragma unroll
  for (int i = KK + 1; i < NT; ++i) {
    if (i < nt) {
      const d4_t N = -T[tile_id(KK, i)];
#pragma unroll
      for (int j = i; j < NT; ++j)
        if (j < nt) T[tile_id(i, j)] = xty(N, T[tile_id(KK, j)], T[tile_id(i, j)]);
      B[i] = xty(N, B[KK], B[i]);
      if (two) B2[i] = xty(N, B2[KK], B2[i]);
    }
  }
}

#define GSS_IK_KERNEL_ATTRS(NT)        \
  __launch_bounds__(64 * IK_WAVES)     \
      __attribute__((amdgpu_waves_per_eu(NT == 1 ? 4 : (NT == 2 ? 3 : 2), NT == 1 ? 5 : (NT == 2 ? 4 : 3))))

// NT = tiles of 16 neighbours the instantiation holds (1, 2 or 4: k <= 16 NT), as in K5.  idx (m x k) / cnt (m): the
// lists of the search.  vg0: the one variogram of the median form; vgtab: K records of the full form (FULL).
// ctab: IK_TAB doubles.  ccdf (m x K, corrected), raw (m x K or NULL), status (m).
template <int DIM, int KIND, int NT, bool FULL>
__global__ GSS_IK_KERNEL_ATTRS(NT)
void ik_local_kernel(VgDev vg0, const VgDev* __restrict__ vgtab, IkSpec sp, const double* __restrict__ ctab,
                     const double* __restrict__ xg, const double* __restrict__ zg, const double* __restrict__ x0,
                     int64_t m, const int* __restrict__ idx, const int* __restrict__ cnt, double* __restrict__ ccdf,
                     double* __restrict__ raw, uint8_t* __restrict__ status_out) {
  __shared__ double nxs_[IK_WAVES][LMAX_K][3];   // neighbour coordinates
  __shared__ double zs_[IK_WAVES][LMAX_K];       // their values
  __shared__ double c0s_[IK_WAVES][LMAX_K];      // the c0 column, lane = neighbour
  __shared__ double S4[2][IK_WAVES][16 * 17];    // diagonal tiles in / inverse factors out, double buffered by step parity
  __shared__ int badflag[2][IK_WAVES];
  __shared__ double G_[IK_WAVES][16][17];

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  double (*nxs)[3] = nxs_[wave];
  double* zs = zs_[wave];
  double* c0s = c0s_[wave];
  double (*G)[17] = G_[wave];
  const int64_t pw = (int64_t)blockIdx.x * IK_WAVES + wave;
  const bool inrange = pw < m;
  const int64_t p = inrange ? pw : m - 1;
  const double NaN = __longlong_as_double(0x7ff8000000000000LL);
  const int K = sp.K;
  const bool ordinary = sp.ordinary != 0;

  int cn = cnt[p];
  cn = cn < 0 ? 0 : (cn > sp.k ? sp.k : cn);
  cn = cn > LMAX_K ? LMAX_K : cn;   // (the driver refuses k > 64)
  cn = __builtin_amdgcn_readfirstlane(cn);
  bool missing = false;
  if (cn < sp.minneighbors || cn <= 0) {
    missing = true;
    cn = 0;
  }
  const int g = lane >> 4, c = lane & 15;
  const bool act = lane < cn;
  double cen[DIM], xj[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) cen[a] = x0[p * DIM + a];
  {
    const int64_t gj = act ? (int64_t)idx[p * sp.k + lane] : 0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      xj[a] = act ? xg[gj * DIM + a] : 0.0;
      nxs[lane][a] = xj[a];
    }
    zs[lane] = act ? zg[gj] : 0.0;
  }
  // the cutoffs of this lane's columns: B tile 1 holds cutoff qb + c - 1 at columns 1 .. n1, B tile 2 cutoff n1 + c
  const int n1 = FULL ? 1 : (K < (ordinary ? 14 : 15) ? K : (ordinary ? 14 : 15));
  const bool two = !FULL && K > n1;   // wave-uniform
  const int q2 = n1 + c;
  const bool col2 = two && q2 < K;
  const double cut2 = col2 ? ctab[q2] : 0.0;
  const double fs2 = (col2 && !ordinary) ? ctab[IK_MAXK + q2] : 0.0;
  const int nt = (cn + 15) >> 4;
  const bool ragged = (cn & 15) != 0;
  const int ntk = (sp.k + 15) >> 4;
  constexpr bool UNIT = KIND >= 0;
  const d4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  bool bad = false;
  double myF = NaN;   // lane (any g, c = q): cutoff q of the point

  const int nsys = FULL ? K : 1;
  for (int qs = 0; qs < nsys; ++qs) {
    const VgDev& vg = FULL ? vgtab[qs] : vg0;
    double sca[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      sca[a] = UNIT ? (vg.aniso ? vg.ir[a] : 1.0) * kpos_scale<(KIND < 0 ? 0 : KIND)>(vg) : 1.0;
    const int q1 = qs + c - 1;
    const bool col1 = c >= 1 && c <= n1 && q1 < K;
    const double cut1 = col1 ? ctab[q1] : 0.0;
    const double fs1 = (col1 && !ordinary) ? ctab[IK_MAXK + q1] : 0.0;

    c0s[lane] = act ? cov_pair_k<DIM, KIND, UNIT>(vg, xj, cen, sca) : 0.0;
    __syncthreads();   // every wave's coordinates, values and c0 are in place (and the last pass is done with S4 and G)

    d4_t T[10];
    if constexpr (NT >= 2) {   // diagonal tiles in pairs, as in K5
#pragma unroll
      for (int Q = 0; Q < NT / 2; ++Q) {
        if (2 * Q < nt) {
          double xr[4][DIM], xc[4][DIM], v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = g + 4 * r;
            const int blk = 16 * (2 * Q + (a > c ? 1 : 0));
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
              xr[r][d] = nxs[blk + a][d];
              xc[r][d] = nxs[blk + c][d];
            }
          }
          cov_pairs4_k<DIM, KIND, UNIT>(vg, xr, xc, v, sca);
          d4_t t0, t1;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            t0[r] = v[r];
            t1[r] = (g + 4 * r == c) ? vg.sill : v[r];
          }
          if (ragged && 2 * Q + 2 >= nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int a = g + 4 * r;
              const double pad = a == c ? 1.0 : 0.0;
              if (!(32 * Q + a < cn && 32 * Q + c < cn)) t0[r] = pad;
              if (!(32 * Q + 16 + a < cn && 32 * Q + 16 + c < cn)) t1[r] = pad;
            }
          }
          T[tile_id(2 * Q, 2 * Q)] = t0;
          if (2 * Q + 1 < nt) T[tile_id(2 * Q + 1, 2 * Q + 1)] = t1;
        }
      }
    }
#pragma unroll
    for (int I = 0; I < NT; ++I) {
      if (I < nt) {
        double xr[4][DIM];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int a = 0; a < DIM; ++a) xr[r][a] = nxs[16 * I + g + 4 * r][a];
#pragma unroll
        for (int J = (NT >= 2 ? I + 1 : I); J < NT; ++J) {
          if (J < nt) {
            const int col = 16 * J + c;
            double xcol[DIM], v[4];
#pragma unroll
            for (int a = 0; a < DIM; ++a) xcol[a] = nxs[col][a];
            cov_pair4_k<DIM, KIND, UNIT>(vg, xr, xcol, v, sca);
#pragma unroll
            for (int r = 0; r < 4; ++r) T[tile_id(I, J)][r] = v[r];
            if (ragged && J == nt - 1) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + g + 4 * r;
                if (!(row < cn && col < cn)) T[tile_id(I, J)][r] = row == col ? 1.0 : 0.0;
              }
            }
          }
        }
      }
    }
    // the columns, formed in tile layout: rows beyond the neighbour count and columns not in use are zero
    d4_t B[4], B2[4];
#pragma unroll
    for (int Kt = 0; Kt < NT; ++Kt) {
      B[Kt] = zero4;
      B2[Kt] = zero4;
      if (Kt < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * Kt + g + 4 * r;
          const bool live = row < cn;
          const double zr = zs[row];
          double v = 0.0;
          if (c == 0) v = c0s[row];
          else if (col1) v = (zr <= cut1 ? 1.0 : 0.0) - fs1;
          else if (c == 15 && ordinary) v = 1.0;
          B[Kt][r] = live ? v : 0.0;
          B2[Kt][r] = (live && col2) ? (zr <= cut2 ? 1.0 : 0.0) - fs2 : 0.0;
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < NT; ++kk) {
      if (kk >= ntk) break;   // (a scalar branch; the barriers stay matched)
      double* mine = S4[kk & 1][wave];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double e = (kk < nt) ? T[tile_id(kk, kk)][r] : ((g + 4 * r) == c ? 1.0 : 0.0);
        if (NT >= 2 && (kk & 1) == 0) mine[c * 17 + (g + 4 * r)] = e;
        else mine[(g + 4 * r) * 17 + c] = e;
      }
      __syncthreads();
      if (wave == kk) potrf16_inverse_x4(&S4[kk & 1][0][0], lane, badflag[kk & 1]);
      __syncthreads();
      if (kk < nt) {
        d4_t V;
#pragma unroll
        for (int r = 0; r < 4; ++r) V[r] = mine[(g + 4 * r) * 17 + c];
        bad = bad || (badflag[kk & 1][wave] != 0);
        switch (kk) {
          case 0: ik_block_step<0, NT>(T, B, B2, V, nt, two); break;
          case 1: ik_block_step<(1 < NT ? 1 : 0), NT>(T, B, B2, V, nt, two); break;
          case 2: ik_block_step<(2 < NT ? 2 : 0), NT>(T, B, B2, V, nt, two); break;
          default: ik_block_step<(3 < NT ? 3 : 0), NT>(T, B, B2, V, nt, two); break;
        }
      }
    }
    // G = Y1'Y1: rows 0 (c0) and 15 (the constant) against every column
    d4_t Gt = zero4;
#pragma unroll
    for (int Kt = 0; Kt < NT; ++Kt)
      if (Kt < nt) Gt = xty(B[Kt], B[Kt], Gt);
#pragma unroll
    for (int r = 0; r < 4; ++r) G[g + 4 * r][c] = Gt[r];
    tile_sync<true>();   // G is read back by lanes of this wave only
    const double S = G[15][15], rr = G[15][0] - 1.0;
    const bool okS = !ordinary || S > 0.0;
    const double ratio = (ordinary && okS) ? rr / S : 0.0;
    bad = bad || !okS;
    {
      const int col = FULL ? 1 : c + 1;                     // the column of cutoff c in tile 1
      const int cc = col < 16 ? col : 0;
      const double a = G[0][cc], v = G[15][cc];
      const double f = a - ratio * v;
      const bool mineq = FULL ? c == qs : c < n1;
      if (mineq) myF = f;
    }
    if (two) {
      tile_sync<true>();
      Gt = zero4;
#pragma unroll
      for (int Kt = 0; Kt < NT; ++Kt)
        if (Kt < nt) Gt = xty(B[Kt], B2[Kt], Gt);   // (column a of tile 1) . (column b of tile 2)
#pragma unroll
      for (int r = 0; r < 4; ++r) G[g + 4 * r][c] = Gt[r];
      tile_sync<true>();
      const int cc = c >= n1 ? c - n1 : 0;
      const double a = G[0][cc], v = G[15][cc];
      if (c >= n1) myF = a - ratio * v;
    }
  }
  if (!ordinary) myF += c < K ? ctab[IK_MAXK + c] : 0.0;
  uint8_t st = GSS_PT_OK;
  if (missing) st = GSS_PT_MISSING;
  else if (bad) st = GSS_PT_SINGULAR;
  if (st != GSS_PT_OK) myF = NaN;
  const double fc = ik_order16(myF, c, K);
  if (inrange && g == 0 && c < K) {
    ccdf[p * K + c] = fc;
    if (raw) raw[p * K + c] = myF;
  }
  if (inrange && lane == 0) status_out[p] = st;
}

struct IkLaunch {
  const VgDev* vg;       // host: the one variogram (median form)
  const VgDev* vgtab;    // device: K records (full form) or NULL
  IkSpec sp;
  const double *ctab, *xg, *zg, *x0;
  int64_t m;
  const int *idx, *cnt;
  double *ccdf, *raw;
  uint8_t* status;
  hipStream_t s;
};

template <int DIM, int KIND, bool FULL>
int32_t ik_local_launch(const IkLaunch& a) {
  const dim3 grid((unsigned)((a.m + IK_WAVES - 1) / IK_WAVES)), block(64 * IK_WAVES);
#define GSS_IK_LAUNCH(NTV)                                                                                             \
  hipLaunchKernelGGL((ik_local_kernel<DIM, KIND, NTV, FULL>), grid, block, 0, a.s, *a.vg, a.vgtab, a.sp, a.ctab, a.xg,  \
                     a.zg, a.x0, a.m, a.idx, a.cnt, a.ccdf, a.raw, a.status)
  if (a.sp.k <= 16) GSS_IK_LAUNCH(1);
  else if (a.sp.k <= 32) GSS_IK_LAUNCH(2);
  else GSS_IK_LAUNCH(4);
#undef GSS_IK_LAUNCH
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

template <int DIM>
int32_t ik_local_launch_kinds(int kind, const IkLaunch& a) {
  switch (kind) {
    case GSS_VG_GAUSSIAN: return ik_local_launch<DIM, GSS_VG_GAUSSIAN, false>(a);
    case GSS_VG_EXPONENTIAL: return ik_local_launch<DIM, GSS_VG_EXPONENTIAL, false>(a);
    case GSS_VG_SPHERICAL: return ik_local_launch<DIM, GSS_VG_SPHERICAL, false>(a);
    case VG_MATERN12: return ik_local_launch<DIM, VG_MATERN12, false>(a);
    case VG_MATERN32: return ik_local_launch<DIM, VG_MATERN32, false>(a);
    default: return ik_local_launch<DIM, VG_MATERN52, false>(a);
  }
}

// the compile-time kinds of the median form in 2-D and 3-D have units of their own (ik_2d.hip, ik_3d.hip)
int32_t ik_local_launch_2d(int kind, const IkLaunch& a);
int32_t ik_local_launch_3d(int kind, const IkLaunch& a);

}  // namespace gss
