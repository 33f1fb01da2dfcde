// Co-simulation of nz variables under a linear model of coregionalisation (gss.h, gss_fftgs_create_lmc; DESIGN.md
// section 4): the factors of the two coefficient matrices and the kernel that mixes unit fields and white noise into
// the variables,
//     Z_a = means[a] + sum_j L1[a][j] Y_j + sum_j L0[a][j] E_j .
// The fields Y_j come from the realisation pipelines of fftgs.hip, which also holds the driver and the two entries.
#pragma once
#include "fftgs_common.h"
#include "gss_internal.h"
#include "philox.h"

#include <cmath>

namespace gss {

// Left-looking Cholesky without pivoting of the symmetric n x n matrix B (row-major, stride LMC_MAXZ) into L (same
// layout, zero above the diagonal).  With d the largest diagonal entry, a pivot <= 1e-12 d makes its column a zero
// column, provided what would have been divided is <= 1e-12 d in magnitude as well; anything else (a pivot below
// -1e-12 d included) means that B is not positive semidefinite.  *live: bit j set for every non-zero column.  Every
// operation is rounded on its own, in this order: tests/fftgs_lmc_ref.py restates it.
inline int32_t lmc_factor(const char* who, const char* which, const double* B, int n, double* L, uint32_t* live) {
#pragma clang fp contract(off)
  double d = B[0];
  for (int j = 1; j < n; ++j) d = B[j * LMC_MAXZ + j] > d ? B[j * LMC_MAXZ + j] : d;
  const double tol = 1e-12 * d;
  for (int e = 0; e < LMC_MAXZ * LMC_MAXZ; ++e) L[e] = 0.0;
  *live = 0;
  for (int j = 0; j < n; ++j) {
    double p = B[j * LMC_MAXZ + j];
    for (int k = 0; k < j; ++k) p = p - L[j * LMC_MAXZ + k] * L[j * LMC_MAXZ + k];
    if (p < -tol) {
      set_error("%s: %s is not positive semidefinite: the pivot at [%d][%d] is %g", who, which, j, j, p);
      return GSS_ERR_INVALID;
    }
    const bool zero = p <= tol;
    const double ljj = zero ? 0.0 : std::sqrt(p);
    L[j * LMC_MAXZ + j] = ljj;
    for (int i = j + 1; i < n; ++i) {
      double t = B[i * LMC_MAXZ + j];
      for (int k = 0; k < j; ++k) t = t - L[i * LMC_MAXZ + k] * L[j * LMC_MAXZ + k];
      if (zero) {
        if (std::fabs(t) > tol) {
          set_error("%s: %s is not positive semidefinite: entry [%d][%d] leaves %g beside a zero pivot at [%d][%d]",
                    who, which, i, j, t, j, j);
          return GSS_ERR_INVALID;
        }
      } else {
        L[i * LMC_MAXZ + j] = t / ljj;
      }
    }
    if (!zero) *live |= 1u << j;
  }
  return GSS_OK;
}

// The mix, in place.  Z holds the realisations of one chunk, NZ slots of N cells each: on entry slot j of a
// realisation holds the unit field Y_j if column j of L1 is live (the other slots hold anything), on exit slot a holds
// Z_a.  A thread owns VEC adjacent cells of one realisation (grid y): it loads the live fields of its cells, draws the
// live nugget normals -- E_j of realisation r at cell e is philox_normal(nseed, r NZ + j, e), what gss_philox_normal
// returns, or element e of slot j of `E` when the caller supplied them --, and stores the NZ variables.  Nothing else
// moves: 8 N (live fields + NZ) bytes per realisation.
//   VEC = 2: 16-byte accesses; needs N even and Z (and E) 16-byte aligned, so that every slot is.  An odd N puts every
//   other slot 8 bytes off such a boundary, so those grids take VEC = 1.
//   NZ is a compile-time bound: y, w and the accumulators are registers (2 NZ VEC doubles), every loop is unrolled and
//   the tests of the live bits are scalar branches.
template <int NZ, int VEC>
__global__ __launch_bounds__(256) void fftgs_lmc_mix_kernel(LmcCoef c, double* __restrict__ Z, int64_t N, uint64_t nseed,
                                                            int64_t real0, const double* __restrict__ E) {
  const int64_t slot0 = (int64_t)blockIdx.y * NZ * N;
  double* z = Z + slot0;
  const double* en = E ? E + slot0 : nullptr;
  const uint32_t id0 = (uint32_t)((real0 + blockIdx.y) * NZ);
  const int64_t nv = N / VEC;   // (VEC = 2: N is even)
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {
    const int64_t e0 = v * VEC;
    double y[NZ][VEC], w[NZ][VEC];
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      if ((c.live1 >> j) & 1u) {
        if (VEC == 2) {
          const double2 t = *reinterpret_cast<const double2*>(z + j * N + e0);
          y[j][0] = t.x;
          y[j][VEC - 1] = t.y;
        } else {
          y[j][0] = z[j * N + e0];
        }
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) y[j][k] = 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      if ((c.live0 >> j) & 1u) {
        if (en) {
          if (VEC == 2) {
            const double2 t = *reinterpret_cast<const double2*>(en + j * N + e0);
            w[j][0] = t.x;
            w[j][VEC - 1] = t.y;
          } else {
            w[j][0] = en[j * N + e0];
          }
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) w[j][k] = philox_normal(nseed, id0 + (uint32_t)j, (uint64_t)(e0 + k));
        }
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) w[j][k] = 0.0;
      }
    }
#pragma unroll
    for (int a = 0; a < NZ; ++a) {
      double acc[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = c.means[a];
#pragma unroll
      for (int j = 0; j <= a; ++j) {   // (the factors are lower triangular)
        if ((c.live1 >> j) & 1u) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = fma(c.L1[a * LMC_MAXZ + j], y[j][k], acc[k]);
        }
      }
#pragma unroll
      for (int j = 0; j <= a; ++j) {
        if ((c.live0 >> j) & 1u) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = fma(c.L0[a * LMC_MAXZ + j], w[j][k], acc[k]);
        }
      }
      if (VEC == 2) *reinterpret_cast<double2*>(z + a * N + e0) = make_double2(acc[0], acc[VEC - 1]);
      else z[a * N + e0] = acc[0];
    }
  }
}

template <int NZ>
inline void lmc_mix_launch_nz(const LmcCoef& c, double* Z, int64_t N, int64_t nb, uint64_t nseed, int64_t real0,
                              const double* E, hipStream_t s) {
  const bool vec = N % 2 == 0 && (reinterpret_cast<uintptr_t>(Z) & 15) == 0 && (reinterpret_cast<uintptr_t>(E) & 15) == 0;
  const int64_t nv = vec ? N / 2 : N;
  int64_t gx = (nv + 255) / 256;
  if (gx > 2048) gx = 2048;   // the rest of a large grid by the stride loop
  if (vec)
    hipLaunchKernelGGL((fftgs_lmc_mix_kernel<NZ, 2>), dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, s, c, Z, N, nseed, real0, E);
  else
    hipLaunchKernelGGL((fftgs_lmc_mix_kernel<NZ, 1>), dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, s, c, Z, N, nseed, real0, E);
}

// nb realisations (<= 65 535, grid y) of nz variables in Z, the first of them realisation real0
inline int32_t lmc_mix_launch(int nz, const LmcCoef& c, double* Z, int64_t N, int64_t nb, uint64_t nseed, int64_t real0,
                              const double* E, hipStream_t s) {
  ProfScope ps("fftgs_lmc_mix", s);
  switch (nz) {
    case 1: lmc_mix_launch_nz<1>(c, Z, N, nb, nseed, real0, E, s); break;
    case 2: lmc_mix_launch_nz<2>(c, Z, N, nb, nseed, real0, E, s); break;
    case 3: lmc_mix_launch_nz<3>(c, Z, N, nb, nseed, real0, E, s); break;
    case 4: lmc_mix_launch_nz<4>(c, Z, N, nb, nseed, real0, E, s); break;
    case 5: lmc_mix_launch_nz<5>(c, Z, N, nb, nseed, real0, E, s); break;
    case 6: lmc_mix_launch_nz<6>(c, Z, N, nb, nseed, real0, E, s); break;
    case 7: lmc_mix_launch_nz<7>(c, Z, N, nb, nseed, real0, E, s); break;
    default: lmc_mix_launch_nz<8>(c, Z, N, nb, nseed, real0, E, s); break;
  }
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

}  // namespace gss
