// The FFTGS handle and what its pipelines export to the driver in fftgs.hip (which describes the three pipelines and how
// a grid is routed to one).  Each pipeline file is the only one that names its kernels.
#pragma once

#include "gss_internal.h"
#include "fftgs_common.h"

#include <rocfft/rocfft.h>

#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

#define GSS_FFT(call)                                                              \
  do {                                                                             \
    rocfft_status st__ = (call);                                                   \
    if (st__ != rocfft_status_success) {                                           \
      ::gss::set_error("%s:%d: %s failed: rocfft status %d", __FILE__, __LINE__, #call, (int)st__); \
      return GSS_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

namespace gss {

struct GridSpec {
  int64_t n1, n2, n3;  // n1 fastest
  int64_t nh;          // n1 / 2 + 1
  int64_t c1, c2, c3;  // 0-based centre cell (dims div 2, 1-based, fft.jl:69)
  double s1, s2, s3;   // spacing
};

// How the members of a batch of realisations (grid y) are spaced: realisation numbers `real` apart, noise arrays and
// outputs `noise` / `out` doubles apart (0: the N of the grid).  The default is the consecutive batch of
// gss_fftgs_realize; the unit fields of a co-simulation (fftgs_lmc.h) step over the columns of other fields.
struct BatchStep {
  uint32_t real = 1;
  int64_t noise = 0, out = 0;
};

constexpr int RED_BLOCKS = 1024;   // partial sums of the amplitude kernels (one per workgroup)

struct FftPlans;   // fftgs_rocfft.hip
enum class FftgsPath { ROCFFT, FUSED, GENERIC };

inline int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : dflt;
}
inline int grid_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b < 256 * 16 ? (b < 1 ? 1 : b) : 256 * 16);
}

}  // namespace gss

struct gss_fftgs {
  gss::VgDev vg;
  gss::GridSpec g;
  // rotated variogram (gss.h, rotation): the covariance grid is evaluated at rotated lags R^T lag; rot holds R as a
  // row-major 3 x 3 in HBM (identity on absent axes)
  bool rotated = false;
  gss::DevBuf rot;
  int ndim = 0;
  int64_t N = 0, NH = 0;
  double mean = 0.0;
  gss::FftgsPath path = gss::FftgsPath::ROCFFT;   // set once, by fftgs_setup_fused / fftgs_setup_generic
  // rocFFT pipeline (general grids): plans (shared with other handles of the same grid size: fft_plans), work buffer,
  // U and Xn are created on first use
  std::shared_ptr<gss::FftPlans> plans;
  rocfft_plan fwd = nullptr, inv = nullptr;   // = plans->fwd / inv
  rocfft_execution_info info = nullptr;
  gss::DevBuf state;  // Fh (NH doubles) followed by scal[2]
  gss::DevBuf U, Xn, work, Z;
  bool ready = false;  // state holds a spectrum (computed here or adopted after a broadcast)
  // fused pipeline (power-of-two 3-D grids)
  gss::FusedGrid fg;
  gss::DevBuf X, tw1, tw2, tw3, Fh_tiled, covsrc;
  // two-stream overlap (GSS_FFTGS_OVERLAP=1): P1 (instruction-issue bound) of realisation r+1 runs on a helper stream
  // beside P2..P5 (HBM bound) of realisation r; two half-spectrum buffers alternate
  gss::DevBuf X2;
  hipStream_t s2 = nullptr;
  hipEvent_t ev_p1[2] = {nullptr, nullptr}, ev_p5[2] = {nullptr, nullptr}, ev_in = nullptr;
  int overlap = 1;
  gss::DevBuf xtw;              // per-pass twiddle tables of the Stockham x passes
  int x_rows = 8;               // x lines per workgroup of the Stockham x passes (rows * M / 8 <= 256)
  int txy_log = 3, txz_log = 3; // log2 of the tile width (columns) of the y and z passes
  // generic pipeline (2-D grids, sizes 2^a 3^b 5^c 7^d: fftgs_generic.h): Stockham plans per axis and their twiddle tables;
  // the half-spectrum buffer is X, the amplitudes are read from the state in their natural layout
  gss::GenGrid gg;
  gss::GenPlan gp[3];
  gss::DevBuf gtab[3];
  int g_rows = 1, g_txlog[3] = {3, 3, 3};
  bool g_tg = false;   // x passes read their tables from global memory (long lines)
  int g_batch = 1;     // realisations per launch (small grids: X holds g_batch half-spectrum buffers, g_xbs elements apart)
  int64_t g_xbs = 0;
  // long y lines of 2-D grids (1 024 < n2 <= 4 096): n2 = L1 L2, plans and tables of the two short transforms, W_n2
  bool g_long = false;
  gss::GenLong gl;
  gss::GenPlan gpl[2];
  gss::DevBuf gltab[2], gtwl;
  // slab order of the strided passes (fftgs_slab_schedule): slab i runs on stream i mod ns (0 = the caller's, the others
  // are helper streams of the process); the events that fence them belong to the handle
  static constexpr int SLAB_MAX_STREAMS = 4;
  hipEvent_t slab_e0 = nullptr, slab_e[SLAB_MAX_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
  // co-simulation (gss_fftgs_create_lmc): the spectrum is rho's with unit sill and mean 0, the factors mix its fields
  int lmc_nz = 0;   // 0: a plain handle
  gss::LmcCoef lmc;
  double* Fh() const { return state.as<double>(); }
  double* scal() const { return state.as<double>() + NH; }
  ~gss_fftgs() {
    if (s2) {
      (void)hipStreamSynchronize(s2);
      (void)hipStreamDestroy(s2);
    }
    for (int b = 0; b < 2; ++b) {
      if (ev_p1[b]) (void)hipEventDestroy(ev_p1[b]);
      if (ev_p5[b]) (void)hipEventDestroy(ev_p5[b]);
    }
    if (ev_in) (void)hipEventDestroy(ev_in);
    for (int i = 0; i < SLAB_MAX_STREAMS; ++i)
      if (slab_e[i]) {
        (void)hipEventSynchronize(slab_e[i]);   // the helper streams may still be working on this handle's buffers
        (void)hipEventDestroy(slab_e[i]);
      }
    if (slab_e0) (void)hipEventDestroy(slab_e0);
    if (info) rocfft_execution_info_destroy(info);   // (the plans go with the last holder of `plans`)
  }
};

namespace gss {

// L / 2 complex twiddles exp(-2 pi i k / L) (the x passes of the fused and of the generic pipeline)
inline int32_t upload_twiddles(DevBuf& buf, int L, hipStream_t s) {
  std::vector<double> t((size_t)L);
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int k = 0; k < L / 2; ++k) {
    const long double a = two_pi * (long double)k / (long double)L;
    t[(size_t)(2 * k)] = (double)cosl(a);
    t[(size_t)(2 * k + 1)] = (double)(-sinl(a));
  }
  GSS_TRY(buf.alloc(sizeof(double) * (size_t)L));
  GSS_HIP(hipMemcpyAsync(buf.p, t.data(), sizeof(double) * (size_t)L, hipMemcpyHostToDevice, s));
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

// ---- what a pipeline exports -----------------------------------------------------------------------------------------
// setup (fused, generic): takes the grid if it can -- sets h->path and allocates the pipeline's buffers -- or leaves it
// spectrum: fft.jl:96-103 up to the unscaled amplitudes in the state and the RED_BLOCKS partial sums of F^2
// tile:     the state is complete (computed or adopted): the copy of the amplitudes in the order the last pass reads
// fields:   one step of nb fields (nb from fftgs_fields_step: each pipeline's batching rule), field i realisation
//           real + i * bs.real, read from noise + i * bs.noise (NULL: seeded), written to z + i * bs.out
int32_t fftgs_setup_fused(gss_fftgs* h, hipStream_t s);
int32_t fftgs_spectrum_fused(gss_fftgs* h, double* partial, hipStream_t s);
int32_t fftgs_tile_fused(gss_fftgs* h, hipStream_t s);
int32_t fftgs_fields_fused(gss_fftgs* h, uint64_t seed, int64_t real, const double* noise, double* z, hipStream_t s);
// GSS_FFTGS_OVERLAP=1, realisations of one gss_fftgs_realize call: begin once, then realisation r of the call
int32_t fftgs_fused_overlap_begin(gss_fftgs* h, hipStream_t s);
int32_t fftgs_fused_overlap_field(gss_fftgs* h, int64_t r, uint64_t seed, int64_t real, const double* noise, double* z,
                                  hipStream_t s);

int32_t fftgs_setup_generic(gss_fftgs* h, hipStream_t s);
int32_t fftgs_spectrum_generic(gss_fftgs* h, double* partial, hipStream_t s);
int32_t fftgs_tile_generic(gss_fftgs* h, hipStream_t s);
int32_t fftgs_fields_generic(gss_fftgs* h, uint64_t seed, int64_t real, int nb, const BatchStep& bs, const double* noise,
                             double* z, hipStream_t s);

int32_t fftgs_spectrum_rocfft(gss_fftgs* h, double* partial, hipStream_t s);   // (natural order: nothing to tile)
// plans and buffers for a call of `total` packed fields (0: single executions only); *batch: fields per batched execution
int32_t fftgs_begin_rocfft(gss_fftgs* h, int64_t total, int* batch);
int32_t fftgs_fields_rocfft(gss_fftgs* h, uint64_t seed, int64_t real, int nb, const double* noise, double* z,
                            hipStream_t s);

// fftgs.hip: the three strided passes slab by slab over the x tiles; launch(stream, t0, nt) issues them for one slab
int32_t fftgs_slab_schedule(gss_fftgs* h, hipStream_t s, int ntx, int per,
                            const std::function<int32_t(hipStream_t, int, int)>& launch);

}  // namespace gss
