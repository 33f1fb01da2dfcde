// Moving-neighbourhood cokriging, the per-point system (gss.h, gss_cokrig_predict_knn).
//
// The shape is that of K5 (krig_local.hip): one wave per domain point, lane j = neighbour j, four points per workgroup
// that share the diagonal-tile duty (tile16.h, potrf16_inverse_x4), the K x K block in registers as 16 x 16 tiles in the
// accumulator layout of v_mfma_f64_16x16x4_f64, the right-hand sides as columns of one B tile, everything finished from
// the Gram matrix G = Y'Y of the forward-substituted columns.  What differs:
//   neighbours   the lists of the nz per-variable searches, concatenated variable by variable without gaps; lane j
//                carries its neighbour's variable id v_j next to the coordinates
//   tile (i, j)  b1[v_i][v_j] rho(x_i, x_j), or c0[v_i][v_j] = (b0 + b1)[v_i][v_j] on a zero key; both 4 x 4 tables sit
//                in LDS, one read per entry
//   columns      [c0_0 .. c0_{nz-1} | z - means[v] | 1[v = 0] .. 1[v = nz-1]]   (the indicators: ordinary variant only)
//   finish       with C_t = column t, Z = column nz, F = the indicator columns of the variables that HAVE neighbours:
//                S = Y_F'Y_F = L L' (at most 4 x 4), u_t = L^-1 (Y_F'y_{c,t} - e_t), v = L^-1 Y_F'y_z,
//                mu_t = means[t] + y_z.y_{c,t} - u_t.v,   sigma^2_t = c00_t - |y_{c,t}|^2 + |u_t|^2   (clamped at 0)
//                A variable without neighbours has a zero column: its constraint is dropped (unit pivot, zero
//                right-hand side), and as a TARGET it has no unbiased estimator: GSS_PT_MISSING.
#pragma once

#include "cokrig.h"
#include "krig_local.h"
#include "tile16.h"

namespace gss {

constexpr int COL_WAVES = 4;
constexpr int COL_TAB = 2 * COL_MAXZ * COL_MAXZ + COL_MAXZ;   // b1, c0, means as the kernel keeps them in LDS

struct CoLocalSpec {
  int nz, ordinary, minneighbors, ksum;
  int k[COL_MAXZ];      // neighbours asked of each variable (0 beyond nz)
  int koff[COL_MAXZ];   // first column of each variable in a row of the concatenated lists
  int off[COL_MAXZ];    // first grouped sample of each variable
};

// rho of four pairs and their zero-key flags.  KIND >= 0: differences scaled by sca, the shape of that one model
// (cov_pairs4_k's arithmetic); KIND < 0: the key of co_rho and the model switch taken once for the four.
template <int DIM, int KIND>
__device__ __forceinline__ void co_rho4(const VgDev& vg, const double (*a)[DIM], const double (*b)[DIM],
                                        const double* sca, double* rho, bool* zero) {
  double d2[4], q[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    d2[u] = KIND < 0 ? sqdist_nofma<DIM>(a[u], b[u], vg.ir, vg.aniso != 0) : sqdist_scaled<DIM, true>(a[u], b[u], sca);
    zero[u] = d2[u] <= 0.0;
    q[u] = fmax(d2[u], 1e-300);
  }
  if (KIND < 0) {
    vg_shape4(vg.kind, q, vg.inv_range, vg.mscale, vg.pw, rho);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      rho[u] = vg_shape_kpos<(KIND < 0 ? 0 : KIND), true>(q[u], vg.inv_range, vg.mscale, vg.pw);
  }
}

template <int DIM, int KIND>
__device__ __forceinline__ double co_rho1(const VgDev& vg, const double* a, const double* b, const double* sca,
                                          bool* zero) {
  if (KIND < 0) {
    const double d2 = sqdist_nofma<DIM>(a, b, vg.ir, vg.aniso != 0);
    *zero = d2 <= 0.0;
    return vg_shape_call(vg.kind, fmax(d2, 1e-300), vg.inv_range, vg.mscale, vg.pw);
  }
  const double d2 = sqdist_scaled<DIM, true>(a, b, sca);
  *zero = d2 <= 0.0;
  return vg_shape_kpos<(KIND < 0 ? 0 : KIND), true>(fmax(d2, 1e-300), vg.inv_range, vg.mscale, vg.pw);
}

// b1[vi][vj] rho, or c0[vi][vj] on a zero key: one LDS read (tab: b1 at 0, c0 at 16)
__device__ __forceinline__ double co_entry(const double* tab, int vi, int vj, double rho, bool zero) {
  const int e = vi * COL_MAXZ + vj;
  return tab[zero ? COL_MAXZ * COL_MAXZ + e : e] * (zero ? 1.0 : rho);
}

// The per-point system of both kernels of this header: cokrig_local_kernel (CV = false: a domain point, every variable
// a target) and cokrig_cv_kernel (CV = true: a sample of the handle as the query, its own variable the one target).
// Neighbour gather, tile assembly, block steps and the Gram matrix are the same code; CV chooses the columns
//   [c0_t | z - means[v] | 1[v = 0] .. 1[v = nz-1]]   (t = the query's variable, wave-uniform; at most nz + 2 columns)
// and the finish for that one target, stored at the caller's row of the query.
// NT = tiles of 16 neighbours the instantiation holds (1, 2 or 4: sum k <= 16 NT), as in K5.
// idx: the lists of the searches, variable a at idx + mv * koff[a], row p of it k[a] wide; cnt[a * mv + p] its length.
// x0: the m centres.  CV: they are grouped samples q0 .. q0 + m - 1 (x0 = xg + q0 DIM), qrow = row + q0 their rows in
// the caller's arrays, and mean_out / var_out / status_out are indexed by those rows (ldo is not read).
template <int DIM, int KIND, int NT, bool CV>
__device__ __forceinline__ void cokrig_point(const VgDev& vg, const CoLocalSpec& sp, const double* xg, const double* zres,
                                             const double* cotab, const double* x0, int64_t m, const int* idx,
                                             const int* cnt, double* mean_out, double* var_out, uint8_t* status_out,
                                             int64_t ldo, int64_t q0, const int* qrow) {
  __shared__ double nxs_[COL_WAVES][LMAX_K][3];   // neighbour coordinates
  __shared__ int nvs_[COL_WAVES][LMAX_K];         // and variable ids
  __shared__ double tab[COL_TAB];
  __shared__ double S4[2][COL_WAVES][16 * 17];    // diagonal tiles in / inverse factors out, double buffered by step parity
  __shared__ int badflag[2][COL_WAVES];
  __shared__ double G_[COL_WAVES][16][17];
  // right-hand-side columns pass from "lane = neighbour" into tile layout through the wave's own pieces of S4 and G_,
  // as in K5: column q at 68 doubles apart, four per piece
  static_assert(4 * (LMAX_K + 4) <= 16 * 17 && 2 * COL_MAXZ + 1 <= LMAX_RHS, "right-hand-side columns do not fit the wave's own tiles");

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  double (*nxs)[3] = nxs_[wave];
  int* nvs = nvs_[wave];
  double (*G)[17] = G_[wave];
  auto rhs_col = [&](int q) -> double* {
    double* base = q < 4 ? &S4[0][wave][0] : (q < 8 ? &S4[1][wave][0] : &G_[wave][0][0]);
    return base + (q & 3) * (LMAX_K + 4);
  };
  const int64_t pw = (int64_t)blockIdx.x * COL_WAVES + wave;
  const bool inrange = pw < m;
  const int64_t p = inrange ? pw : m - 1;
  const double NaN = __longlong_as_double(0x7ff8000000000000LL);
  const int nz = sp.nz;
  int tq = 0;   // CV: the variable of the query, from its place among the grouped samples (wave-uniform)
  if constexpr (CV) {
#pragma unroll
    for (int a = 1; a < COL_MAXZ; ++a)
      if (a < nz && q0 + p >= sp.off[a]) tq = a;
    tq = __builtin_amdgcn_readfirstlane(tq);
  }

  // the tables: 36 doubles out of the handle's table (stride CO_MAXZ), once per workgroup
  if (threadIdx.x < COL_TAB) {
    const int t = threadIdx.x;
    const int e = t & (COL_MAXZ * COL_MAXZ - 1);
    const int src = t < 2 * COL_MAXZ * COL_MAXZ
                        ? (t < COL_MAXZ * COL_MAXZ ? 0 : CO_C0) + (e / COL_MAXZ) * CO_MAXZ + (e % COL_MAXZ)
                        : CO_MEANS + (t - 2 * COL_MAXZ * COL_MAXZ);
    tab[t] = cotab[src];
  }

  // neighbour counts per variable (wave-uniform) and where each variable starts in the concatenated list
  int ca[COL_MAXZ], base[COL_MAXZ + 1];
  base[0] = 0;
#pragma unroll
  for (int a = 0; a < COL_MAXZ; ++a) {
    int c = 0;
    if (a < nz) {
      c = cnt[(int64_t)a * m + p];
      c = c < 0 ? 0 : (c > sp.k[a] ? sp.k[a] : c);
    }
    ca[a] = __builtin_amdgcn_readfirstlane(c);
    base[a + 1] = base[a] + ca[a];
  }
  int K = base[COL_MAXZ];
  K = K > LMAX_K ? LMAX_K : K;   // (the driver refuses sum k > 64)
  bool missing = false;
  if (K < sp.minneighbors || K <= 0) {
    missing = true;
    K = 0;
  }
  const int g = lane >> 4, c = lane & 15;
  constexpr bool UNIT = KIND >= 0;
  double c0[DIM], sca[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    sca[a] = UNIT ? (vg.aniso ? vg.ir[a] : 1.0) * kpos_scale<(KIND < 0 ? 0 : KIND)>(vg) : 1.0;
    c0[a] = x0[p * DIM + a];
  }
  int myv = 0;
  double myrho = 0.0, myz = 0.0;
  bool myzero = false;
  const bool act = lane < K;
  {
    // which variable lane j's neighbour belongs to, and its place in that variable's list
    int jj = lane, kk = sp.k[0], ko = sp.koff[0], go = sp.off[0];
#pragma unroll
    for (int a = 1; a < COL_MAXZ; ++a) {
      // (the fields are pinned as wave-uniform values before the choice: choosing between their addresses instead, as
      //  the optimiser otherwise does, would force a copy of sp into private memory)
      const int ka = __builtin_amdgcn_readfirstlane(sp.k[a]), koa = __builtin_amdgcn_readfirstlane(sp.koff[a]),
                goa = __builtin_amdgcn_readfirstlane(sp.off[a]);
      const bool in = lane >= base[a];
      myv = in ? a : myv;
      jj = in ? lane - base[a] : jj;
      kk = in ? ka : kk;
      ko = in ? koa : ko;
      go = in ? goa : go;
    }
    const int loc = act ? idx[m * ko + p * kk + jj] : 0;
    const int64_t gj = act ? (int64_t)go + loc : 0;
    double xj[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      xj[a] = act ? xg[gj * DIM + a] : 0.0;
      nxs[lane][a] = xj[a];
    }
    if (!act) myv = 0;
    nvs[lane] = myv;
    myz = act ? zres[gj] : 0.0;
    myrho = co_rho1<DIM, KIND>(vg, xj, c0, sca, &myzero);
  }
  __syncthreads();   // tab, and every wave's coordinates are in place
  {
    // the columns, lane = neighbour
    if constexpr (CV) {
      rhs_col(0)[lane] = act ? co_entry(tab, myv, tq, myrho, myzero) : 0.0;
      rhs_col(1)[lane] = act ? myz : 0.0;
      if (sp.ordinary) {
#pragma unroll
        for (int t = 0; t < COL_MAXZ; ++t)
          if (t < nz) rhs_col(2 + t)[lane] = (act && myv == t) ? 1.0 : 0.0;
      }
    } else {
#pragma unroll
      for (int t = 0; t < COL_MAXZ; ++t)
        if (t < nz) rhs_col(t)[lane] = act ? co_entry(tab, myv, t, myrho, myzero) : 0.0;
      rhs_col(nz)[lane] = act ? myz : 0.0;
      if (sp.ordinary) {
#pragma unroll
        for (int t = 0; t < COL_MAXZ; ++t)
          if (t < nz) rhs_col(nz + 1 + t)[lane] = (act && myv == t) ? 1.0 : 0.0;
      }
    }
  }
  tile_sync<true>();   // the columns are read back by other lanes of this wave only
  const int nt = (K + 15) >> 4;
  const bool ragged = (K & 15) != 0;
  d4_t T[10];
  // diagonal tiles in pairs, as in K5: positions (a, b) with a <= b hold tile 2Q's entry, positions a > b tile 2Q + 1's;
  // tile 2Q + 1 gets its own diagonal (c0[v][v] of its rows) put back
  if constexpr (NT >= 2) {
#pragma unroll
    for (int Q = 0; Q < NT / 2; ++Q) {
      if (2 * Q < nt) {
        double xr[4][DIM], xc[4][DIM], rho[4];
        bool zero[4];
        int vr[4], vc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int a = g + 4 * r;
          const int blk = 16 * (2 * Q + (a > c ? 1 : 0));
#pragma unroll
          for (int d = 0; d < DIM; ++d) {
            xr[r][d] = nxs[blk + a][d];
            xc[r][d] = nxs[blk + c][d];
          }
          vr[r] = nvs[blk + a];
          vc[r] = nvs[blk + c];
        }
        co_rho4<DIM, KIND>(vg, xr, xc, sca, rho, zero);
        d4_t t0, t1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = co_entry(tab, vr[r], vc[r], rho[r], zero[r]);
          t0[r] = v;
          t1[r] = v;
          if (g + 4 * r == c) {
            const int vd = nvs[32 * Q + 16 + c];
            t1[r] = tab[COL_MAXZ * COL_MAXZ + vd * (COL_MAXZ + 1)];
          }
        }
        if (ragged && 2 * Q + 2 >= nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = g + 4 * r;
            const double pad = a == c ? 1.0 : 0.0;
            if (!(32 * Q + a < K && 32 * Q + c < K)) t0[r] = pad;
            if (!(32 * Q + 16 + a < K && 32 * Q + 16 + c < K)) t1[r] = pad;
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
      int vr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) xr[r][a] = nxs[16 * I + g + 4 * r][a];
        vr[r] = nvs[16 * I + g + 4 * r];
      }
#pragma unroll
      for (int J = (NT >= 2 ? I + 1 : I); J < NT; ++J) {
        if (J < nt) {
          const int col = 16 * J + c;
          double xc[4][DIM], rho[4];
          bool zero[4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int a = 0; a < DIM; ++a) xc[r][a] = nxs[col][a];
          const int vcol = nvs[col];
          co_rho4<DIM, KIND>(vg, xr, xc, sca, rho, zero);
#pragma unroll
          for (int r = 0; r < 4; ++r) T[tile_id(I, J)][r] = co_entry(tab, vr[r], vcol, rho[r], zero[r]);
          if (ragged && J == nt - 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 16 * I + g + 4 * r;
              if (!(row < K && col < K)) T[tile_id(I, J)][r] = row == col ? 1.0 : 0.0;
            }
          }
        }
      }
    }
  }
  // right-hand sides into tile layout; columns beyond the ones in use and rows beyond the neighbour count are zero
  const int ncols = (CV ? 2 : nz + 1) + (sp.ordinary ? nz : 0);
  d4_t B[4];
  {
    const double* colc = rhs_col(c < LMAX_RHS ? c : 0);
    const bool used = c < ncols;
#pragma unroll
    for (int Kt = 0; Kt < NT; ++Kt) {
      if (Kt < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = colc[16 * Kt + g + 4 * r];
          B[Kt][r] = used ? v : 0.0;
        }
      }
    }
  }
  bool bad = false;
  const d4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  // block steps beyond ceil(sum k / 16) have nothing to do for any point of the launch (a scalar branch; the barriers
  // stay matched)
  const int ntk = (sp.ksum + 15) >> 4;
#pragma unroll
  for (int kk = 0; kk < NT; ++kk) {
    if (kk >= ntk) break;
    double* mine = S4[kk & 1][wave];
    // (the factorisation reads the lower triangle: even tiles of a pair carry their data in the upper one and are handed
    //  over transposed)
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
        case 0: k5_block_step<0, NT>(T, B, V, nt); break;
        case 1: k5_block_step<(1 < NT ? 1 : 0), NT>(T, B, V, nt); break;
        case 2: k5_block_step<(2 < NT ? 2 : 0), NT>(T, B, V, nt); break;
        default: k5_block_step<(3 < NT ? 3 : 0), NT>(T, B, V, nt); break;
      }
    }
  }
  d4_t Gt = zero4;
#pragma unroll
  for (int Kt = 0; Kt < NT; ++Kt)
    if (Kt < nt) Gt = xty(B[Kt], B[Kt], Gt);
#pragma unroll
  for (int r = 0; r < 4; ++r) G[g + 4 * r][c] = Gt[r];
  __syncthreads();

  // ---- finish: lane t = target t (the lanes beyond shadow target 0), CV: every lane the one target; S is at most
  // 4 x 4 and every lane factors it.  Columns of G: the target's covariances, the data, the first indicator.
  const int t = CV ? tq : (lane < nz ? lane : 0);
  const int ccol = CV ? 0 : t, zcol = CV ? 1 : nz, ind0 = zcol + 1;
  int ct = ca[0];
#pragma unroll
  for (int a = 1; a < COL_MAXZ; ++a)
    if (t == a) ct = ca[a];
  const double qf = G[ccol][ccol], af = G[zcol][ccol];
  double rsr = 0.0, tsr = 0.0;
  bool okS = true;
  if (sp.ordinary) {
    double L[COL_MAXZ][COL_MAXZ], u[COL_MAXZ], w[COL_MAXZ];
#pragma unroll
    for (int j = 0; j < COL_MAXZ; ++j) {
      if (j < nz) {
        const bool here = ca[j] > 0;   // wave-uniform
        const int fj = ind0 + j;
        double d = here ? G[fj][fj] : 1.0;
        double ru = here ? G[fj][ccol] - (j == t ? 1.0 : 0.0) : 0.0;
        double rw = here ? G[fj][zcol] : 0.0;
#pragma unroll
        for (int cc = 0; cc < j; ++cc) {
          d = fma(-L[j][cc], L[j][cc], d);
          ru = fma(-L[j][cc], u[cc], ru);
          rw = fma(-L[j][cc], w[cc], rw);
        }
        if (!(d > 0.0)) {
          okS = false;
          d = 1.0;
        }
        const double inv = 1.0 / sqrt(d);
        L[j][j] = d * inv;
        u[j] = ru * inv;
        w[j] = rw * inv;
        rsr = fma(u[j], u[j], rsr);
        tsr = fma(u[j], w[j], tsr);
#pragma unroll
        for (int i = j + 1; i < COL_MAXZ; ++i) {
          if (i < nz) {
            double s = (here && ca[i] > 0) ? G[ind0 + i][fj] : 0.0;
#pragma unroll
            for (int cc = 0; cc < j; ++cc) s = fma(-L[i][cc], L[j][cc], s);
            L[i][j] = s * inv;
          }
        }
      }
    }
  }
  if (inrange && (CV ? lane == 0 : lane < nz)) {
    const int64_t o = CV ? (int64_t)qrow[p] : (int64_t)lane * ldo + p;
    uint8_t st = GSS_PT_OK;
    if (missing) st = GSS_PT_MISSING;
    else if (bad || !okS) st = GSS_PT_SINGULAR;
    else if (sp.ordinary && ct == 0) st = GSS_PT_MISSING;   // no neighbour of the target's own variable
    double mu = NaN, vv = NaN;
    if (st == GSS_PT_OK) {
      mu = tab[2 * COL_MAXZ * COL_MAXZ + t] + af - tsr;
      vv = tab[COL_MAXZ * COL_MAXZ + t * (COL_MAXZ + 1)] - qf + rsr;
      vv = vv > 0.0 ? vv : 0.0;
    }
    mean_out[o] = mu;
    var_out[o] = vv;
    if (status_out) status_out[o] = st;
  }
}

#define GSS_COL_KERNEL_ATTRS(NT)        \
  __launch_bounds__(64 * COL_WAVES)     \
      __attribute__((amdgpu_waves_per_eu(NT == 1 ? 4 : 3, NT == 1 ? 5 : (NT == 2 ? 4 : 3))))

template <int DIM, int KIND, int NT>
__global__ GSS_COL_KERNEL_ATTRS(NT)
void cokrig_local_kernel(VgDev vg, CoLocalSpec sp, const double* __restrict__ xg, const double* __restrict__ zres,
                         const double* __restrict__ cotab, const double* __restrict__ x0, int64_t m,
                         const int* __restrict__ idx, const int* __restrict__ cnt, double* __restrict__ mean_out,
                         double* __restrict__ var_out, uint8_t* __restrict__ status_out, int64_t ldo) {
  cokrig_point<DIM, KIND, NT, false>(vg, sp, xg, zres, cotab, x0, m, idx, cnt, mean_out, var_out, status_out, ldo, 0,
                                     nullptr);
}

// The one-target form (gss.h, gss_cokrig_cv_knn): the m queries are grouped samples q0 .. q0 + m - 1 of the handle; pred,
// var and status are indexed by the caller's row of the query (row: the map of the grouped copy).
template <int DIM, int KIND, int NT>
__global__ GSS_COL_KERNEL_ATTRS(NT)
void cokrig_cv_kernel(VgDev vg, CoLocalSpec sp, const double* __restrict__ xg, const double* __restrict__ zres,
                      const double* __restrict__ cotab, const int* __restrict__ row, int64_t q0, int64_t m,
                      const int* __restrict__ idx, const int* __restrict__ cnt, double* __restrict__ pred,
                      double* __restrict__ var_out, uint8_t* __restrict__ status_out) {
  cokrig_point<DIM, KIND, NT, true>(vg, sp, xg, zres, cotab, xg + q0 * DIM, m, idx, cnt, pred, var_out, status_out, 0, q0,
                                    row + q0);
}

// One launch of either kernel.  CV = false: x0 are the m domain points, mean / var / status have nz columns ldo apart.
// CV = true: the queries are grouped samples q0 .. q0 + m - 1, row is the map to the caller's rows (x0, ldo not read).
struct CoLocalLaunch {
  const VgDev* vg;
  CoLocalSpec sp;
  const double *xg, *zres, *cotab, *x0;
  int64_t m;
  const int *idx, *cnt;
  double *mean, *var;
  uint8_t* status;
  int64_t ldo;
  hipStream_t s;
  const int* row = nullptr;
  int64_t q0 = 0;
};

template <int DIM, int KIND, bool CV = false>
int32_t cokrig_local_launch(const CoLocalLaunch& a) {
  const dim3 grid((unsigned)((a.m + COL_WAVES - 1) / COL_WAVES)), block(64 * COL_WAVES);
#define GSS_COL_LAUNCH(NTV)                                                                                            \
  do {                                                                                                                 \
    if constexpr (CV)                                                                                                  \
      hipLaunchKernelGGL((cokrig_cv_kernel<DIM, KIND, NTV>), grid, block, 0, a.s, *a.vg, a.sp, a.xg, a.zres, a.cotab,  \
                         a.row, a.q0, a.m, a.idx, a.cnt, a.mean, a.var, a.status);                                     \
    else                                                                                                               \
      hipLaunchKernelGGL((cokrig_local_kernel<DIM, KIND, NTV>), grid, block, 0, a.s, *a.vg, a.sp, a.xg, a.zres,        \
                         a.cotab, a.x0, a.m, a.idx, a.cnt, a.mean, a.var, a.status, a.ldo);                            \
  } while (0)
  if (a.sp.ksum <= 16) GSS_COL_LAUNCH(1);
  else if (a.sp.ksum <= 32) GSS_COL_LAUNCH(2);
  else GSS_COL_LAUNCH(4);
#undef GSS_COL_LAUNCH
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// the compile-time kinds of 2-D and 3-D have units of their own (cokrig_local_2d.hip, cokrig_local_3d.hip)
int32_t cokrig_local_launch_2d(int kind, const CoLocalLaunch& a);
int32_t cokrig_local_launch_3d(int kind, const CoLocalLaunch& a);
int32_t cokrig_cv_launch_2d(int kind, const CoLocalLaunch& a);
int32_t cokrig_cv_launch_3d(int kind, const CoLocalLaunch& a);

template <int DIM, bool CV = false>
int32_t cokrig_local_launch_kinds(int kind, const CoLocalLaunch& a) {
  switch (kind) {
    case GSS_VG_GAUSSIAN: return cokrig_local_launch<DIM, GSS_VG_GAUSSIAN, CV>(a);
    case GSS_VG_EXPONENTIAL: return cokrig_local_launch<DIM, GSS_VG_EXPONENTIAL, CV>(a);
    case GSS_VG_SPHERICAL: return cokrig_local_launch<DIM, GSS_VG_SPHERICAL, CV>(a);
    case VG_MATERN12: return cokrig_local_launch<DIM, VG_MATERN12, CV>(a);
    case VG_MATERN32: return cokrig_local_launch<DIM, VG_MATERN32, CV>(a);
    default: return cokrig_local_launch<DIM, VG_MATERN52, CV>(a);
  }
}

// the kernel of one chunk by dimension and model: the fixed kinds of 2-D and 3-D, else the general one (kind = -1 for a
// nested model); instantiated by the unit of each driver
template <bool CV>
int32_t cokrig_local_dispatch(int dim, int kind, const CoLocalLaunch& a) {
  const bool fixed = kind == GSS_VG_GAUSSIAN || kind == GSS_VG_EXPONENTIAL || kind == GSS_VG_SPHERICAL ||
                     kind == VG_MATERN12 || kind == VG_MATERN32 || kind == VG_MATERN52;
  if (dim == 3) {
    if (!fixed) return cokrig_local_launch<3, -1, CV>(a);
    return CV ? cokrig_cv_launch_3d(kind, a) : cokrig_local_launch_3d(kind, a);
  }
  if (dim == 2) {
    if (!fixed) return cokrig_local_launch<2, -1, CV>(a);
    return CV ? cokrig_cv_launch_2d(kind, a) : cokrig_local_launch_2d(kind, a);
  }
  return cokrig_local_launch<1, -1, CV>(a);
}

// the launch parameters of a call from its arguments (cokrig_local.hip); refuses nz > COL_MAXZ and sum k > LMAX_K
int32_t cokrig_spec(const CoGrouped& g, int variant, const int* k, int minneighbors, CoLocalSpec* out);

// idx_out (m x ksum, the caller's rows, -1 beyond a variable's count) and count_out (m x nz) from the lists of the
// searches (cokrig_local.hip); qrow: the output row of every point of the chunk (NULL: point p at row p)
int32_t cokrig_lists_dev(const CoLocalSpec& sp, const int* idx, const int* cnt, const int* row, const int* qrow,
                         int64_t m, int* idx_out, int* count_out, hipStream_t s);

}  // namespace gss
