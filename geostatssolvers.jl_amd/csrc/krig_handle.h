// The kriging handle (gss.h, gss_krig_t) and what the units of its entry points share: krig.hip (global kriging: the
// fit, the predictors, block support), cokrig.hip (cokriging: creators and predictors) and krig_cv.hip (cross-validation).
#pragma once

#include "gss_internal.h"
#include "cokrig.h"

namespace gss {

constexpr int MAX_NC = 64;
constexpr int NSEG = 4;  // row segments of the RHS assembly (mean partials are summed in fixed order)

struct DriftSpec {
  int variant;
  int nc;
  int dim;
  signed char e[MAX_NC][3];
  double center[3];
  double inv_scale[3];
};

}  // namespace gss

struct gss_krig {
  gss::VgDev vg;
  int variant = GSS_KRIG_ORDINARY;
  double sk_mean = 0.0;
  int degree = 0;
  int ndrift = 0;
  int dim = 0;
  int64_t n = 0;
  int nc = 0;
  int64_t N1 = 0, N1pad = 0, ldw = 0;
  gss::DriftSpec ds;
  gss::DevBuf xdata, z, drift_data;
  // rotated variogram: xdata holds the frame coordinates R^T (x - c) of the samples, xraw the coordinates as given
  // (for searches in another frame); c = the first sample.  Every predict call moves its domain into the same frame.
  gss::Frame fr;
  gss::DevBuf xraw;
  gss::DevBuf factor;  // W' (ldw x N1pad, column-major) followed by wd (N1pad)
  // fit in flight: workspace, status words, and the slot borrowed from the process (its `done` event ends the fit;
  // joined and handed back by krig_fit_wait, or by the destructor of a handle whose fit nobody joined)
  gss::DevBuf fit_ws;
  gss::FitSlot fit_slot;
  bool fit_pending = false;
  int* fit_info = nullptr;
  hipStream_t fit_stream = nullptr;  // stream of the fit in flight (a retry goes back on it)
  // GSS_KRIG_ASYNC_FIT: the fit runs on the library's fit stream beside whatever the caller queues next (K1 of the
  // first prediction); its two status words travel to the slot's pinned words on that stream, in front of `done`
  bool fit_async = false;
  ~gss_krig() {
    if (fit_pending && fit_slot.done) (void)hipEventSynchronize(fit_slot.done);
    gss::fit_slot_release(&fit_slot);
  }
  bool factored = false;
  // block support (gss_krig_set_block_support): right-hand sides regularised over a cell of size `cell` sampled at
  // the centres of nsub^dim sub-cells; c_vv = mean covariance between two samples of the cell (replaces the sill in
  // the variance).  nsub = 0: point support.
  int block_nsub = 0;
  double block_cell[3] = {0.0, 0.0, 0.0};
  double block_cvv = 0.0;
  // cokriging (gss_cokrig_create): nz > 0, the system is over the stacked samples of nz variables.  covar: the
  // variable id of every stacked sample; cotab: the coefficient table the kernels read (CO_TAB doubles); c00 / means:
  // host copies of C_tt(0) = b0[t][t] + b1[t][t] and of the known means (zero under the ordinary variant)
  int nz = 0;
  gss::DevBuf covar, cotab;
  double c00[gss::CO_MAXZ] = {}, means[gss::CO_MAXZ] = {};
  // the same samples grouped by variable for the per-variable searches of gss_cokrig_predict_knn (cokrig.h, CoGrouped):
  // coordinates on the covariance frame / as given (only with a frame), residuals z - means[var], the caller's row of
  // every grouped sample, and where each variable starts
  gss::DevBuf co_xg, co_xg_raw, co_zres, co_row;
  int64_t co_off[gss::CO_MAXZ + 1] = {};
  double* Wp() const { return factor.as<double>(); }
  double* wd() const { return factor.as<double>() + ldw * N1pad; }
};

namespace gss {
int32_t krig_local_dev(const VgDev& vg, int variant, int nc, int dim, const signed char* exps, double inv_scale,
                       double sk_mean, Searcher& sr, const double* xdata, const double* z, const double* drift_data,
                       const double* x0, const double* x0_raw, const double* drift_dom, int64_t m, int k,
                       int minneighbors, double* mean, double* var, uint8_t* status, int* idx_out, int* count_out,
                       hipStream_t s, HostPipe* pipe, int block_nsub, const double* block_cell, double block_cvv,
                       const KnnMask* mask = nullptr);

// ---- krig.hip ---------------------------------------------------------------------------------------------------------
// points per chunk of the right-hand-side workspace (N1pad rows) and the process-wide workspace itself
int64_t krig_chunk_points(int64_t N1pad, int64_t m);
int32_t krig_workspace(int64_t N1pad, int64_t mc, hipStream_t s, double** R, double** mean_part);
// x (and xraw with a frame: the coordinates as given, x then holds them on the frame) <- n host points
int32_t krig_upload_samples(const Frame& fr, const double* xhost, int64_t n, int dim, DevBuf* x, DevBuf* xraw,
                            hipStream_t s);
// the fit: queued on s (async: on the fit stream), joined on the device / on the host with its status
int32_t krig_factorize(gss_krig* h, hipStream_t s, bool async = false);
int32_t krig_join_device(gss_krig* h, hipStream_t s);
int32_t krig_fit_wait(gss_krig* h);
// K3 over one chunk of right-hand sides, and its launch attributes (once per device)
void launch_krig_quadform(const gss_krig* h, const double* Rws, int64_t ldr, double c00, double mean0, int64_t mv,
                          int64_t cols, double* mean_out, double* var_out, uint8_t* stp, double* qpart, hipStream_t s);
int32_t krig_quadform_attrs();
// entry points that know one variable only
int32_t krig_refuse_cokrig(const gss_krig* h, const char* who);
// Dual weights of nbatch data vectors (zdev: nbatch x n, device) against the factor of a kriging or cokriging handle,
// shared by gss_krig_predict_global_batch and gss_cokrig_predict_global_batch: WD is N1 x nbatch, column-major with
// leading dimension h->ldw.  Everything is queued on s; the buffers must outlive it.
struct BatchDual {
  DevBuf Zm, U, WD;
};
int32_t krig_batch_dual(const gss_krig* h, const double* zdev, int64_t nbatch, BatchDual* d, hipStream_t s);

// ---- cokrig.hip: what the fit and the cross-validation need of a cokriging handle -------------------------------------
// the n x n block of the system, the indicator columns Fd and the centring of the data vector (simple cokriging)
int32_t cokrig_fit_system(const gss_krig* h, double* M, hipStream_t s);
int32_t cokrig_fit_indicators(const gss_krig* h, double* Fd, hipStream_t s);
void cokrig_fit_center(const gss_krig* h, double* zz, hipStream_t s);
// the handle's samples grouped by variable, as the moving-neighbourhood drivers take them (cokrig.h)
void cokrig_grouped(const gss_krig* h, CoGrouped* g);
// The neighbour counts of a moving-neighbourhood call: at most COL_MAXZ variables, k[a] in 1 .. the sample count of
// variable a, at most 64 in total (*ksum).  who: the entry the messages name; clamp_note closes the range message.
int32_t cokrig_knn_counts(const gss_krig* h, const char* who, const char* clamp_note, const int32_t* k, int* ksum);
// one searcher per variable (sr[COL_MAXZ]) over that variable's grouped samples, all in the same frame
int32_t cokrig_searchers(const gss_krig* h, const CoGrouped& g, Searcher* sr, int32_t metric, double metric_param,
                         double radius, const double* inv_radii, hipStream_t s);

// ---- cokrig_batch.hip ---------------------------------------------------------------------------------------------------
// Zm(i, b) -= means[var_i] for i < n in each of nbatch columns of leading dimension h->ldw (simple cokriging)
void cokrig_batch_center(const gss_krig* h, double* Zm, int64_t nbatch, hipStream_t s);

}  // namespace gss
