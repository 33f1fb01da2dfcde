// Shared by the cokriging paths (cokrig.hip: the creators, the global neighbourhood and the entry of the moving one;
// cokrig_local*.hip: the moving neighbourhood; cokrig_cv.hip: its cross-validation, entry in krig_cv.hip): the layout of
// the coefficient table, the correlation with its zero-key flag, and the interfaces of the moving-neighbourhood drivers.
#pragma once

#include "gss_internal.h"

#include <cstdlib>

namespace gss {

// Coefficient table of a cokriging handle in device memory (CO_TAB doubles): b1[a * CO_MAXZ + b] (symmetrised), then
// c0 = b0 + b1 in the same layout (the value at a zero key), then means[CO_MAXZ].
constexpr int CO_MAXZ = 8;
constexpr int CO_C0 = CO_MAXZ * CO_MAXZ, CO_MEANS = 2 * CO_MAXZ * CO_MAXZ, CO_TAB = CO_MEANS + CO_MAXZ;

// rho(a, b) of the structure (sill 1, no nugget) and whether the key is zero.  The key and the shape are those of
// cov_pair / cov_d2_select: KIND >= 0 folds the model switch away, KIND < 0 reads it from vg.  The shape is evaluated on
// max(d2, 1e-300) for every lane; the caller selects the zero-key value afterwards.
template <int DIM, int KIND>
__device__ __forceinline__ double co_rho(const VgDev& vg, const double* a, const double* b, bool* zero) {
  const double d2 = KIND < 0 ? sqdist_nofma<DIM>(a, b, vg.ir, vg.aniso != 0) : sqdist_nofma<DIM>(a, b, vg.ir, true);
  *zero = d2 <= 0.0;
  return vg_shape(KIND < 0 ? vg.kind : KIND, fmax(d2, 1e-300), vg.inv_range, vg.mscale, vg.pw);
}

// ---- moving neighbourhood (gss.h, gss_cokrig_predict_knn; cokrig_local.hip) ---------------------------------------------
constexpr int COL_MAXZ = 4;   // variables of a moving-neighbourhood call: 2 nz + 1 right-hand-side columns <= LMAX_RHS

// The samples of a cokriging handle grouped by variable (variable a at off[a] .. off[a + 1] - 1, caller's row order
// inside a variable), all device memory: coordinates on the covariance frame, the same before the frame (NULL without
// one), residuals z - means[var], and the caller's row of every grouped sample.
struct CoGrouped {
  const double* x = nullptr;
  const double* x_raw = nullptr;
  const double* zres = nullptr;
  const int* row = nullptr;
  const double* tab = nullptr;   // the coefficient table (CO_TAB doubles)
  int64_t off[CO_MAXZ + 1] = {};
  int nz = 0;
};

// GSS_COKRIG_CHUNK_POINTS caps the points per chunk of every cokriging call (tests: a chunk loop that runs more than once
// at a small size)
inline int64_t cokrig_chunk_cap(int64_t chunk) {
  if (const char* e = std::getenv("GSS_COKRIG_CHUNK_POINTS")) {
    const int64_t cap = std::atoll(e) / 256 * 256;
    if (cap > 0 && cap < chunk) chunk = cap;
  }
  return chunk;
}

// what a launch of the moving-neighbourhood kernel and of its cross-validation kernel have in common: model, spec,
// grouped samples and the lists of mv queries; x0, outputs, ldo, row and q0 are left to the driver (cokrig_local.hip)
struct CoLocalSpec;
struct CoLocalLaunch;
CoLocalLaunch cokrig_launch_common(const VgDev& vg, const CoLocalSpec& sp, const CoGrouped& g, const int* idx,
                                   const int* cnt, int64_t mv, hipStream_t s);

// One search per variable (sr[a] over the samples of variable a, already given to it) and one system per domain point.
// x0: m centres on the covariance frame, x0_raw: before it (read when the searches run in another frame).  mean, var:
// nz columns of ldo doubles, status nz x ldo bytes or NULL; idx_out (m x sum k) and count_out (m x nz) may be NULL.
// Everything is device memory; `pipe` moves host arrays piece by piece.
int32_t cokrig_local_dev(const VgDev& vg, int variant, int dim, const CoGrouped& g, Searcher* sr, const int* k,
                         int minneighbors, const double* x0, const double* x0_raw, int64_t m, double* mean, double* var,
                         uint8_t* status, int64_t ldo, int* idx_out, int* count_out, hipStream_t s, HostPipe* pipe);

// Cross-validation on the same searchers and grouped samples (cokrig_cv.hip; gss.h, gss_cokrig_cv_knn): every grouped
// sample is predicted as its own variable from the k[a] nearest samples of every variable a outside its fold and, for
// ex >= 0, beyond the exclusion key ex.  fold: one id per caller's row (device) or NULL for one fold per sample.  pred,
// var, status (may be NULL), idx_out (n x sum k) and count_out (n x nz; both may be NULL) are indexed by caller's rows.
int32_t cokrig_cv_dev(const VgDev& vg, int variant, int dim, const CoGrouped& g, Searcher* sr, const int* k,
                      int minneighbors, const int* fold, double ex, double* pred, double* var, uint8_t* status,
                      int* idx_out, int* count_out, hipStream_t s);

}  // namespace gss
