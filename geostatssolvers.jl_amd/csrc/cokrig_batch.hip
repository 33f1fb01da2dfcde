// Batched cokriging means (gss.h, gss_cokrig_predict_global_batch; DESIGN.md section 4 "Cokriging"): many value vectors
// at the stacked samples of one fitted cokriging system, every target variable at every domain point, means only -- the
// conditioning step of co-simulation, where the data and every unconditional realisation are kriged from the same
// locations.  With WD = K^-1 [Z - means; 0] (krig.hip, krig_batch_dual)
//     mean(b, t, p) = sum_j C_{var_j t}(x_j, p) WD(j, b)  +  WD(n + t, b)  (ordinary)  |  + means[t]  (simple)
// and C_{var_j t}(x_j, p) = b1[var_j][t] rho(x_j, p), or c0[var_j][t] at a zero key.  The coefficient is folded into the
// weights once per pass (cokrig_mix_kernel), so the hot kernel evaluates rho once per (sample, point) and spends one FMA
// per column on it, whatever the column's batch and target.
#include "krig_handle.h"

namespace gss {

// Columns of one pass: column c = b * nz + t holds batch b of the pass and target t; floor(COB_COLS / nz) batches ride
// along.  Two accumulator VGPRs per column (DESIGN.md section 4 has the measured choice).
#ifndef GSS_COKRIG_BATCH_COLS
#define GSS_COKRIG_BATCH_COLS 32
#endif
constexpr int COB_COLS = GSS_COKRIG_BATCH_COLS;
static_assert(COB_COLS >= CO_MAXZ && COB_COLS % 8 == 0, "one batch of CO_MAXZ targets must fit a pass");

__global__ __launch_bounds__(256) void cokrig_batch_center_kernel(double* __restrict__ Zm, int64_t ldw,
                                                                  const int* __restrict__ var,
                                                                  const double* __restrict__ tab, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) Zm[(int64_t)blockIdx.y * ldw + i] -= tab[CO_MEANS + var[i]];
}

// The weight tables of one pass, rows of COB_COLS doubles side by side for the scalar loads, zero in the columns past
// ncol = nb * nz:  V[j][c] = b1[var_j][t] WD(j, b) and V0[j][c] = c0[var_j][t] WD(j, b) for j < n; row n of V holds what
// is added at the end, WD(n + t, b) under the ordinary variant (the e_t row of target t) and means[t] under the simple.
__global__ __launch_bounds__(256) void cokrig_mix_kernel(const double* __restrict__ WD, int64_t ldw,
                                                         const int* __restrict__ var, const double* __restrict__ tab,
                                                         int n, int nz, int nb, int ordinary, double* __restrict__ V,
                                                         double* __restrict__ V0) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > n) return;
  const double* row = j < n ? tab + var[j] * CO_MAXZ : tab;
  for (int c = 0; c < COB_COLS; ++c) {
    const int b = c / nz, t = c - b * nz;
    double v = 0.0, v0 = 0.0;
    if (b < nb) {
      if (j < n) {
        const double w = WD[j + (int64_t)b * ldw];
        v = row[t] * w;
        v0 = row[CO_C0 + t] * w;
      } else {
        v = ordinary ? WD[n + t + (int64_t)b * ldw] : tab[CO_MEANS + t];
      }
    }
    V[(int64_t)j * COB_COLS + c] = v;
    if (j < n) V0[(int64_t)j * COB_COLS + c] = v0;
  }
}

// Thread = domain point, the sample j is wave-uniform: x_j and row j of V come through the scalar cache and the weights
// enter the FMAs as scalar operands (krig_batch_mean_kernel's layout).  A lane whose key is zero takes nothing from V and
// the cross nugget row V0 instead; the second row is only read by a wave in which some lane sits on sample j, which
// on a simulation grid is one wave per sample.  The sums run over j in ascending order in every lane: the result of
// a point does not depend on the chunk or the pass it is computed in.
template <int DIM, int KIND>
__global__ __launch_bounds__(256) void cokrig_batch_mean_kernel(VgDev vg, const double* __restrict__ xd, int n,
                                                                const double* __restrict__ x0, int64_t m,
                                                                const double* __restrict__ V,
                                                                const double* __restrict__ V0, int ncol,
                                                                double* __restrict__ out, int64_t ldo) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < m;
  const int64_t pc = live ? p : m - 1;
  double c[DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k) c[k] = x0[pc * DIM + k];
  double acc[COB_COLS];
#pragma unroll
  for (int q = 0; q < COB_COLS; ++q) acc[q] = 0.0;
  for (int j = 0; j < n; ++j) {
    double x[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) x[k] = xd[(int64_t)j * DIM + k];
    bool zero;
    const double rho = co_rho<DIM, KIND>(vg, x, c, &zero);
    const double r = zero ? 0.0 : rho;
    const double* __restrict__ row = V + (int64_t)j * COB_COLS;
#pragma unroll
    for (int q = 0; q < COB_COLS; ++q) acc[q] = fma(r, row[q], acc[q]);
    if (__any(zero)) {
      const double one = zero ? 1.0 : 0.0;
      const double* __restrict__ row0 = V0 + (int64_t)j * COB_COLS;
#pragma unroll
      for (int q = 0; q < COB_COLS; ++q) acc[q] = fma(one, row0[q], acc[q]);
    }
  }
  if (!live) return;
  const double* __restrict__ tail = V + (int64_t)n * COB_COLS;
#pragma unroll
  for (int q = 0; q < COB_COLS; ++q)
    if (q < ncol) out[(int64_t)q * ldo + p] = acc[q] + tail[q];
}

template <int DIM>
static void launch_cokrig_batch_mean(hipStream_t s, const VgDev& vg, const double* xd, int n, const double* x0,
                                     int64_t m, const double* V, const double* V0, int ncol, double* out,
                                     int64_t ldo) {
  const dim3 grid((unsigned)((m + 255) / 256));
#define GSS_CB_LAUNCH(KIND)                                                                                          \
  hipLaunchKernelGGL((cokrig_batch_mean_kernel<DIM, KIND>), grid, dim3(256), 0, s, vg, xd, n, x0, m, V, V0, ncol,    \
                     out, ldo)
  switch (vg.kind) {   // (launch_cokrig_rhs's dispatch)
    case GSS_VG_GAUSSIAN: GSS_CB_LAUNCH(GSS_VG_GAUSSIAN); break;
    case GSS_VG_EXPONENTIAL: GSS_CB_LAUNCH(GSS_VG_EXPONENTIAL); break;
    case GSS_VG_SPHERICAL: GSS_CB_LAUNCH(GSS_VG_SPHERICAL); break;
    case VG_MATERN12: GSS_CB_LAUNCH(VG_MATERN12); break;
    case VG_MATERN32: GSS_CB_LAUNCH(VG_MATERN32); break;
    case VG_MATERN52: GSS_CB_LAUNCH(VG_MATERN52); break;
    default: GSS_CB_LAUNCH(-1); break;
  }
#undef GSS_CB_LAUNCH
}

}  // namespace gss

using namespace gss;

void gss::cokrig_batch_center(const gss_krig* h, double* Zm, int64_t nbatch, hipStream_t s) {
  hipLaunchKernelGGL(cokrig_batch_center_kernel, dim3((unsigned)((h->n + 255) / 256), (unsigned)nbatch), dim3(256), 0,
                     s, Zm, h->ldw, h->covar.as<int>(), h->cotab.as<double>(), (int)h->n);
}

extern "C" {

int32_t gss_cokrig_predict_global_batch(gss_krig_t* h, const double* xdom, int64_t m, const double* zbatch,
                                        int64_t nbatch, double* mean_out, int32_t mem, void* stream) {
  GSS_ENTRY();
  const char* who = "gss_cokrig_predict_global_batch";
  GSS_REQUIRE(h != nullptr, "%s: NULL handle", who);
  GSS_REQUIRE(h->nz > 0, "%s: the handle is not a cokriging system (gss_cokrig_create makes one; the batched means of "
              "one variable come from gss_krig_predict_global_batch)", who);
  GSS_REQUIRE(h->factored, "%s: the handle has no factor (gss_cokrig_create_local makes handles for the moving "
              "neighbourhood; gss_cokrig_create fits the global system)", who);
  GSS_REQUIRE(m >= 0 && nbatch >= 0, "%s: negative sizes (m = %lld, nbatch = %lld)", who, (long long)m,
              (long long)nbatch);
  if (m == 0 || nbatch == 0) return GSS_OK;
  GSS_REQUIRE(xdom && zbatch && mean_out, "%s: NULL array", who);
  GSS_REQUIRE(nbatch <= 65535, "%s: nbatch = %lld, at most 65535 value vectors per call", who, (long long)nbatch);
  hipStream_t s = to_stream(stream);
  GSS_TRY(krig_join_device(h, s));
  GSS_TRY(krig_fit_wait(h));
  const int dim = h->dim, nz = h->nz;
  const int64_t n = h->n;
  Staged sx, sz, so;
  GSS_TRY(sx.in(xdom, sizeof(double) * m * dim, mem, s));
  GSS_TRY(sz.in(zbatch, sizeof(double) * nbatch * n, mem, s));
  FrameCopy xfr;   // rotated structure: the domain in the frame of the samples
  GSS_TRY(xfr.of(h->fr, &sx, m, s));
  GSS_TRY(so.out(mean_out, sizeof(double) * (size_t)(nbatch * nz * m), mem));

  BatchDual bd;
  GSS_TRY(krig_batch_dual(h, sz.as<double>(), nbatch, &bd, s));

  // floor(COB_COLS / nz) value vectors per pass, the domain in the chunks of gss_cokrig_predict_global
  const int per = COB_COLS / nz;
  const int64_t mc = cokrig_chunk_cap(krig_chunk_points(h->N1pad * nz, m));
  DevBuf V, V0;
  GSS_TRY(V.alloc(sizeof(double) * (size_t)((n + 1) * COB_COLS)));
  GSS_TRY(V0.alloc(sizeof(double) * (size_t)(n * COB_COLS)));
  const double* xd = h->xdata.as<double>();
  for (int64_t b0 = 0; b0 < nbatch; b0 += per) {
    const int nb = (int)((nbatch - b0) < per ? (nbatch - b0) : per);
    hipLaunchKernelGGL(cokrig_mix_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s,
                       bd.WD.as<double>() + b0 * h->ldw, h->ldw, h->covar.as<int>(), h->cotab.as<double>(), (int)n, nz,
                       nb, h->variant == GSS_KRIG_ORDINARY ? 1 : 0, V.as<double>(), V0.as<double>());
    GSS_HIP(hipGetLastError());
    ProfScope ps("cokrig_batch", s);
    for (int64_t off = 0; off < m; off += mc) {
      const int64_t mv = (m - off) < mc ? (m - off) : mc;
      const double* x0 = sx.as<double>() + off * dim;
      double* out = so.as<double>() + b0 * nz * m + off;
      switch (dim) {
        case 1: launch_cokrig_batch_mean<1>(s, h->vg, xd, (int)n, x0, mv, V.as<double>(), V0.as<double>(), nb * nz, out, m); break;
        case 2: launch_cokrig_batch_mean<2>(s, h->vg, xd, (int)n, x0, mv, V.as<double>(), V0.as<double>(), nb * nz, out, m); break;
        default: launch_cokrig_batch_mean<3>(s, h->vg, xd, (int)n, x0, mv, V.as<double>(), V0.as<double>(), nb * nz, out, m); break;
      }
      GSS_HIP(hipGetLastError());
    }
  }
  GSS_TRY(so.back(s));
  GSS_HIP(hipStreamSynchronize(s));   // the weights and the tables are freed on return
  return GSS_OK;
}

}  // extern "C"
