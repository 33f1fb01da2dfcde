// FFTGS: FFT-based unconditional Gaussian simulation on Cartesian grids (Gutjahr 1997).
// Replaces preprocess (/root/reference/src/simulation/fft.jl:62-103) and solvesingle (fft.jl:145-173).
//
// preprocess, fft.jl:96-103:
//     C  = sill - gamma(centre cell, every cell)
//     F  = sqrt(|fft(fftshift(C))|), F[1] = 0
//   |fft| is invariant to the circular placement of C, so the fftshift is not materialised, and C is
//   real, so the real-to-complex transform gives the same |.| on the Hermitian half.
// solvesingle, fft.jl:163-170:
//     P  = F .* exp(im * angle(fft(rand)))
//     Z  = real(ifft(P)); Z *= sqrt(sill / var(Z, mean=0)); Z += mean
//   P is Hermitian, hence by Parseval sum(Z^2) = sum(F^2) / N for EVERY realisation: the rescale is
//   the constant s = sqrt(sill N (N-1) / sum F^2), folded with the 1/N of the unnormalised inverse
//   into the stored half-spectrum Fh = F s / N; the mean enters as the DC coefficient.
//
// Three pipelines compute these two steps, each in a file of its own that alone names its kernels; a handle is routed
// to one of them when it is created (gss_fftgs::path) and keeps it:
//   fused   (fftgs_fused.hip)    3-D grids with power-of-two sizes, 32..1024 along x and 16..1024 along y and z, whose half
//                                spectrum exceeds 12 MiB: five hand-written passes, one realisation per step
//   generic (fftgs_generic.hip)  1-D, 2-D and the remaining 3-D grids with sizes 2^a 3^b 5^c 7^d (n1 even, n1 / 2 <= 2 048,
//                                other axes <= 1 024, y of a 2-D grid <= 4 096): the same passes on run-time radix plans,
//                                up to g_batch realisations per step
//   rocFFT  (fftgs_rocfft.hip)   everything else: noise, R2C, phase, C2R; 64 or 16 realisations per step on small grids
// GSS_FFTGS_PATH = rocfft | generic | fused overrides the routing where the named pipeline can take the grid.
// This file holds what they share: the Parseval scale, the slab schedule of the strided passes, the driver that
// realises fields step by step (fftgs_fields_dev) and the C entry points, co-simulation included.
#include "fftgs_handle.h"
#include "fftgs_lmc.h"

#include <cmath>
#include <cstring>
#include <new>

namespace gss {

// scal[0] = sum F^2, scal[1] = s / N with s = sqrt(sill N (N-1) / sum F^2)
__global__ void fftgs_scale_kernel(const double* __restrict__ partial, int nparts, double sill, double N,
                                   double* __restrict__ scal) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += partial[i];
    scal[0] = s;
    scal[1] = sqrt(sill * N * (N - 1.0) / s) / N;
  }
}

__global__ __launch_bounds__(256) void fftgs_apply_scale_kernel(double* __restrict__ Fh, int64_t NH,
                                                                const double* __restrict__ scal) {
  const double f = scal[1];
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < NH; idx += (int64_t)gridDim.x * 256)
    Fh[idx] *= f;
}

// full-size F from the scaled half-spectrum (parity checks): F(k) = Fh(hermitian partner) / scal[1]
__global__ __launch_bounds__(256) void fftgs_expand_kernel(GridSpec g, const double* __restrict__ Fh,
                                                           const double* __restrict__ scal,
                                                           double* __restrict__ F) {
  const int64_t N = g.n1 * g.n2 * g.n3;
  const double inv = 1.0 / scal[1];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (int64_t)gridDim.x * 256) {
    int64_t k1 = e % g.n1, k2 = (e / g.n1) % g.n2, k3 = e / (g.n1 * g.n2);
    if (k1 >= g.nh) {
      k1 = g.n1 - k1;
      k2 = (g.n2 - k2) % g.n2;
      k3 = (g.n3 - k3) % g.n3;
    }
    F[e] = Fh[k1 + g.nh * (k2 + g.n2 * k3)] * inv;
  }
}

// (blockIdx.y: member of a batch of realisations, sources sbs and destinations n doubles apart)
__global__ __launch_bounds__(256) void gather_kernel(const double* __restrict__ src, const int64_t* __restrict__ inds,
                                                     int64_t n, double* __restrict__ dst, int64_t sbs = 0) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[(int64_t)blockIdx.y * n + i] = src[(int64_t)blockIdx.y * sbs + inds[i]];
}

// helper streams of the slab order, shared by every handle of the process (creating a stream costs milliseconds);
// what runs on them is fenced by the calling handle's events on both sides
static hipStream_t slab_stream(int i) { return helper_stream(HELPER_GEN0 + (i - 1) % 3); }   // i = 1, 2, ...

// The three strided passes run slab by slab over the ntx x tiles, `per` tiles a slab: launch(stream, t0, nt) issues P2,
// P3, P4 on the tiles of slab 0, then slab 1, ...
// A slab (fused: GSS_FFTGS_SLAB tiles; 2 tiles = 67 MB of the 1.1 GB half spectrum at 512^3) written by one pass is read
// back by the next from the 256 MB memory-side cache; consecutive slabs go to GSS_FFTGS_SLAB_STREAMS streams in
// turn (the caller's and helper streams fenced by events), so that the short launches of a slab -- two rounds of
// resident workgroups each -- overlap with those of its neighbours instead of draining the device 45 times per
// realisation.  Measured per 512^3 realisation: one launch per pass 2.23 ms; slabs of 7 tiles on one stream 2.09
// (1 tile: 2.52, the launches are too small); slabs of 2 tiles on 3 streams 1.93 (2 streams 1.93-1.97, 4 streams 1.96;
// 1 tile on 4 streams 1.95, 3 tiles on 3 streams 2.02).
int32_t fftgs_slab_schedule(gss_fftgs* h, hipStream_t s, int ntx, int per,
                            const std::function<int32_t(hipStream_t, int, int)>& launch) {
  static const int slab_streams = env_int("GSS_FFTGS_SLAB_STREAMS", 3);
  int ns = slab_streams < 1 ? 1 : (slab_streams > gss_fftgs::SLAB_MAX_STREAMS ? gss_fftgs::SLAB_MAX_STREAMS : slab_streams);
  hipStream_t side[gss_fftgs::SLAB_MAX_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 1; i < ns; ++i) {
    side[i] = slab_stream(i);
    if (!side[i]) ns = i;   // no more helper streams to be had: the slabs share what there is
  }
  if (ns > 1 && !h->slab_e0) {
    GSS_HIP(hipEventCreateWithFlags(&h->slab_e0, hipEventDisableTiming));
    for (int i = 1; i < ns; ++i) GSS_HIP(hipEventCreateWithFlags(&h->slab_e[i], hipEventDisableTiming));
  }
  if (ns > 1) {
    GSS_HIP(hipEventRecord(h->slab_e0, s));   // P1 (and whatever else the caller's stream holds) comes first
    for (int i = 1; i < ns; ++i) GSS_HIP(hipStreamWaitEvent(side[i], h->slab_e0, 0));
  }
  int islab = 0;
  for (int t0 = 0; t0 < ntx; t0 += per, ++islab) {
    const int nt = t0 + per <= ntx ? per : ntx - t0;
    GSS_TRY(launch((islab % ns) ? side[islab % ns] : s, t0, nt));
  }
  for (int i = 1; i < ns; ++i) {              // P5 waits for every slab
    GSS_HIP(hipEventRecord(h->slab_e[i], side[i]));
    GSS_HIP(hipStreamWaitEvent(s, h->slab_e[i], 0));
  }
  return GSS_OK;
}

// the state is complete (computed or adopted): derive what the realisation kernels read
static int32_t fftgs_finish_state(gss_fftgs* h, hipStream_t s) {
  double hs[2];
  GSS_HIP(hipMemcpyAsync(hs, h->scal(), sizeof(hs), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  GSS_REQUIRE(hs[0] > 0.0 && std::isfinite(hs[1]) && hs[1] > 0.0, "degenerate spectrum (sum F^2 = %g)", hs[0]);
  if (h->path == FftgsPath::FUSED) GSS_TRY(fftgs_tile_fused(h, s));
  if (h->path == FftgsPath::GENERIC) GSS_TRY(fftgs_tile_generic(h, s));
  h->ready = true;
  return GSS_OK;
}

// ---- the field driver --------------------------------------------------------------------------------------------------
// What a call needs before its first step; *batch: the most fields one step takes.  `total` packed fields (consecutive
// realisations, noise and outputs N apart) are to come, 0 when they are spaced otherwise: the generic passes take any
// spacing in one launch, the batched rocFFT plans only the packed one, sized by the call's total.
static int32_t fftgs_fields_begin(gss_fftgs* h, int64_t total, int* batch) {
  *batch = h->path == FftgsPath::GENERIC ? h->g_batch : 1;
  return h->path == FftgsPath::ROCFFT ? fftgs_begin_rocfft(h, total, batch) : GSS_OK;
}

// how many of the n fields left (in this chunk of the output) the next step takes
static int64_t fftgs_fields_step(const gss_fftgs* h, int64_t n, int batch) {
  if (h->path == FftgsPath::GENERIC) return batch < n ? batch : n;
  return batch > 1 && n >= batch ? batch : 1;   // rocFFT: a batched execution only while a full batch is left
}

// One step: nb fields of the handle's spectrum into device memory, field i realisation real + i * bs.real of `seed`,
// read from noise + i * bs.noise when the caller supplied uniforms (device memory), written to z + i * bs.out.
// gss_fftgs_realize and the co-simulation both realise through here, so a field has the bits that gss_fftgs_realize
// gives for its realisation number.
static int32_t fftgs_fields_dev(gss_fftgs* h, uint64_t seed, int64_t real, int64_t nb, const BatchStep& bs,
                                const double* noise, double* z, hipStream_t s) {
  switch (h->path) {
    case FftgsPath::FUSED: return fftgs_fields_fused(h, seed, real, noise, z, s);
    case FftgsPath::GENERIC: return fftgs_fields_generic(h, seed, real, (int)nb, bs, noise, z, s);
    default: return fftgs_fields_rocfft(h, seed, real, (int)nb, noise, z, s);
  }
}

// n fields, step by step
static int32_t fftgs_fields_all(gss_fftgs* h, uint64_t seed, int64_t id0, int64_t n, const BatchStep& bs,
                                const double* noise, double* z, hipStream_t s) {
  const int64_t N = h->N;
  const int64_t nstep = bs.noise > 0 ? bs.noise : N, zstep = bs.out > 0 ? bs.out : N;
  const bool packed = bs.real == 1 && nstep == N && zstep == N;
  int batch = 1;
  GSS_TRY(fftgs_fields_begin(h, packed ? n : 0, &batch));
  for (int64_t i = 0, nb = 0; i < n; i += nb) {
    nb = fftgs_fields_step(h, n - i, batch);
    GSS_TRY(fftgs_fields_dev(h, seed, id0 + i * (int64_t)bs.real, nb, bs, noise ? noise + i * nstep : nullptr,
                             z + i * zstep, s));
  }
  return GSS_OK;
}

// the unit fields of realisations real0 .. real0 + nb - 1 of a co-simulation into their slots of Z (nb x nz x N): every
// field of the chunk in one batch when all columns of L1 are live, else one batch per live column
static int32_t lmc_fields(gss_fftgs* h, uint64_t seed, int64_t real0, int64_t nb, const double* noise, double* Z,
                          hipStream_t s) {
  const int nz = h->lmc_nz;
  const int64_t N = h->N;
  if (h->lmc.live1 == (1u << nz) - 1u) return fftgs_fields_all(h, seed, real0 * nz, nb * nz, BatchStep(), noise, Z, s);
  BatchStep bs;
  bs.real = (uint32_t)nz;
  bs.noise = bs.out = (int64_t)nz * N;
  for (int j = 0; j < nz; ++j)
    if ((h->lmc.live1 >> j) & 1u)
      GSS_TRY(fftgs_fields_all(h, seed, real0 * nz + j, nb, bs, noise ? noise + j * N : nullptr, Z + j * N, s));
  return GSS_OK;
}

}  // namespace gss

using namespace gss;

extern "C" {

int32_t gss_fftgs_create(gss_fftgs_t** out, const gss_variogram_t* vg, int32_t ndim, const int64_t* dims,
                         const double* spacing, double mean, int32_t flags, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(out != nullptr, "gss_fftgs_create: out is NULL");
  *out = nullptr;
  GSS_REQUIRE(ndim >= 1 && ndim <= 3 && dims != nullptr, "FFTGS needs a 1-D, 2-D or 3-D Cartesian grid");
  GSS_REQUIRE(vg != nullptr, "variogram is NULL");
  gss_variogram_t v3;
  Frame fr;   // rotated variogram: the lags are rotated instead of the grid (fftgs_cov_rot_kernel, FF_SRC_COV_ROT)
  GSS_TRY(vg_frame_split(vg, &v3, &fr));
  GSS_REQUIRE(vg->dim == ndim, "variogram dimension %d does not match the grid dimension %d", vg->dim, ndim);
  v3.dim = 3;  // lags of absent axes are zero
  for (int k = ndim; k < 3; ++k) {
    v3.inv_radii[k] = 1.0;
    for (int e = 0; e < 3; ++e) v3.extra[e].inv_radii[k] = 1.0;
  }
  gss_fftgs* h = new (std::nothrow) gss_fftgs();
  if (!h) return GSS_ERR_ALLOC;
  struct Guard {
    gss_fftgs* h;
    ~Guard() { delete h; }
  } guard{h};
  GSS_REQUIRE(vg_is_stationary(&v3), "variogram model must be stationary");  // fft.jl:91, lu.jl:110
  GSS_TRY(make_vgdev(&v3, &h->vg));
  if (fr.on) {
    double R3[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};   // the leading ndim x ndim block, identity beyond
    for (int i = 0; i < ndim; ++i)
      for (int j = 0; j < ndim; ++j) R3[3 * i + j] = fr.R[3 * i + j];
    GSS_TRY(h->rot.alloc(sizeof(R3)));
    GSS_HIP(hipMemcpy(h->rot.p, R3, sizeof(R3), hipMemcpyHostToDevice));
    h->rotated = true;
  }
  int64_t d[3] = {1, 1, 1};
  double sp[3] = {1.0, 1.0, 1.0};
  for (int k = 0; k < ndim; ++k) {
    GSS_REQUIRE(dims[k] >= 2, "every grid axis needs at least two cells");
    d[k] = dims[k];
    sp[k] = spacing ? spacing[k] : 1.0;
  }
  h->ndim = ndim;
  h->mean = mean;
  h->g = GridSpec{d[0], d[1], d[2], d[0] / 2 + 1, d[0] / 2 - 1, d[1] / 2 - 1, d[2] / 2 - 1, sp[0], sp[1], sp[2]};
  // axes beyond ndim have size 1: their centre offset must be zero
  if (ndim < 2) h->g.c2 = 0;
  if (ndim < 3) h->g.c3 = 0;
  h->N = d[0] * d[1] * d[2];
  h->NH = h->g.nh * d[1] * d[2];
  GSS_REQUIRE(h->N >= 2, "FFTGS needs at least two cells");
  hipStream_t s = to_stream(stream);

  GSS_TRY(h->state.alloc(sizeof(double) * (size_t)(h->NH + 2)));
  GSS_TRY(fftgs_setup_fused(h, s));  // decides the pipeline; allocates its buffers (no rocFFT plan on that path)
  GSS_TRY(fftgs_setup_generic(h, s));
  if (flags & GSS_FFTGS_NO_SPECTRUM) {  // the state arrives by broadcast (gss_fftgs_adopt_state)
    GSS_HIP(hipStreamSynchronize(s));
    guard.h = nullptr;
    *out = h;
    return GSS_OK;
  }

  // spectrum: C -> forward transform -> sqrt|.| -> Parseval scale
  DevBuf partial;
  GSS_TRY(partial.alloc(sizeof(double) * RED_BLOCKS));
  switch (h->path) {
    case FftgsPath::FUSED: GSS_TRY(fftgs_spectrum_fused(h, partial.as<double>(), s)); break;
    case FftgsPath::GENERIC: GSS_TRY(fftgs_spectrum_generic(h, partial.as<double>(), s)); break;
    default: GSS_TRY(fftgs_spectrum_rocfft(h, partial.as<double>(), s)); break;
  }
  hipLaunchKernelGGL(fftgs_scale_kernel, dim3(1), dim3(64), 0, s, partial.as<double>(), RED_BLOCKS, h->vg.sill,
                     (double)h->N, h->scal());
  hipLaunchKernelGGL(fftgs_apply_scale_kernel, dim3(grid_blocks(h->NH)), dim3(256), 0, s, h->Fh(), h->NH,
                     h->scal());
  GSS_HIP(hipGetLastError());
  GSS_TRY(fftgs_finish_state(h, s));
  guard.h = nullptr;
  *out = h;
  return GSS_OK;
}

int32_t gss_fftgs_destroy(gss_fftgs_t* h) {
  GSS_ENTRY();
  delete h;
  return GSS_OK;
}

int32_t gss_fftgs_spectrum(gss_fftgs_t* h, double* f_out, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && f_out != nullptr, "gss_fftgs_spectrum: NULL argument");
  GSS_REQUIRE(h->ready, "handle has no spectrum");
  hipStream_t s = to_stream(stream);
  Staged so;
  GSS_TRY(so.out(f_out, sizeof(double) * (size_t)h->N, mem));
  hipLaunchKernelGGL(fftgs_expand_kernel, dim3(grid_blocks(h->N)), dim3(256), 0, s, h->g, h->Fh(), h->scal(),
                     so.as<double>());
  GSS_HIP(hipGetLastError());
  return so.back(s);
}

int32_t gss_fftgs_state_buffer(gss_fftgs_t* h, void** dev_ptr, int64_t* bytes) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && dev_ptr != nullptr && bytes != nullptr, "NULL argument");
  *dev_ptr = h->state.p;
  *bytes = (int64_t)(sizeof(double) * (size_t)(h->NH + 2));
  return GSS_OK;
}

int32_t gss_fftgs_adopt_state(gss_fftgs_t* h, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  return fftgs_finish_state(h, to_stream(stream));
}

int32_t gss_fftgs_realize(gss_fftgs_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                          const int64_t* inds, int64_t ninds, double* out, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && out != nullptr && nreals >= 0 && first_real >= 0, "gss_fftgs_realize: bad arguments");
  GSS_REQUIRE(h->lmc_nz == 0, "gss_fftgs_realize: the handle co-simulates %d variables (gss_fftgs_create_lmc): "
              "gss_fftgs_realize_lmc realises it", h->lmc_nz);
  GSS_REQUIRE(h->ready, "handle has no spectrum");
  if (nreals == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  int batch = 1;
  GSS_TRY(fftgs_fields_begin(h, nreals, &batch));
  const int64_t N = h->N;
  const int64_t npts = inds ? ninds : N;
  // Host arrays: the realisations leave chunk by chunk through a ring of at most three chunks (OutStream: the
  // reference returns every realisation as a host vector, fft.jl:173,197 -- 256 realisations of 512^3 cells are 256 GiB
  // and never sit in HBM together); supplied noise arrives one realisation at a time on the caller's stream.
  Staged sn, si;
  OutStream os;
  const bool host = mem == GSS_MEM_HOST;
  if (noise && host) {
    GSS_TRY(sn.own.alloc(sizeof(double) * (size_t)N));
    sn.p = sn.own.p;
  }
  GSS_TRY(si.in(inds, sizeof(int64_t) * (size_t)(inds ? ninds : 0), mem, s));
  GSS_TRY(os.begin(out, sizeof(double) * (size_t)npts, nreals, mem, s));
  if (inds && h->Z.bytes < sizeof(double) * (size_t)N) GSS_TRY(h->Z.alloc(sizeof(double) * (size_t)N));

  // fused pipeline with more than one realisation (GSS_FFTGS_OVERLAP=1): P1 of realisation r+1 beside P2..P5 of r
  const bool piped = h->path == FftgsPath::FUSED && h->overlap && nreals > 1 && !(noise && host);
  if (piped) GSS_TRY(fftgs_fused_overlap_begin(h, s));
  for (int64_t r = 0, nb = 0; r < nreals; r += nb) {
    double* dst = nullptr;                              // realisation r's place (caller's HBM or a slot of the ring)
    GSS_TRY(os.slot(r, s, &dst));
    // a step: consecutive realisations whose outputs are consecutive (the caller's array, or one chunk of the ring)
    int64_t n = nreals - r;
    if (os.on && n > os.chunk - r % os.chunk) n = os.chunk - r % os.chunk;
    const double* nz = noise ? noise + r * N : nullptr;
    if (noise && host) {                                // (host noise is staged one realisation at a time)
      n = 1;
      nz = sn.as<double>();
      GSS_HIP(hipMemcpyAsync(sn.p, noise + r * N, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s));
    }
    nb = fftgs_fields_step(h, n, batch);
    if (inds && nb > 1 && h->Z.bytes < sizeof(double) * (size_t)N * (size_t)nb)
      GSS_TRY(h->Z.alloc(sizeof(double) * (size_t)N * (size_t)batch));
    double* zf = inds ? h->Z.as<double>() : dst;
    if (piped) GSS_TRY(fftgs_fused_overlap_field(h, r, seed, first_real + r, nz, zf, s));
    else GSS_TRY(fftgs_fields_dev(h, seed, first_real + r, nb, BatchStep(), nz, zf, s));
    if (inds) {
      hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((ninds + 255) / 256), (unsigned)nb), dim3(256), 0, s, zf,
                         si.as<int64_t>(), ninds, dst, N);
      GSS_HIP(hipGetLastError());
    }
    GSS_TRY(os.done(r + nb - 1, s));
  }
  return os.finish(s);
}

int32_t gss_fftgs_create_lmc(gss_fftgs_t** out, const gss_variogram_t* structure, int32_t nz, const double* b0,
                             const double* b1, const double* means, int32_t ndim, const int64_t* dims,
                             const double* spacing, int32_t flags, void* stream) {
  GSS_ENTRY();
  const char* who = "gss_fftgs_create_lmc";
  GSS_REQUIRE(out != nullptr, "%s: out is NULL", who);
  *out = nullptr;
  GSS_REQUIRE(structure != nullptr, "%s: structure is NULL", who);
  GSS_REQUIRE(nz >= 1 && nz <= LMC_MAXZ, "%s: nz = %d outside 1 .. %d", who, nz, LMC_MAXZ);
  GSS_REQUIRE(b0 != nullptr && b1 != nullptr, "%s: b0 or b1 is NULL", who);
  GSS_REQUIRE(means != nullptr, "%s: means is NULL", who);
  GSS_REQUIRE(dims != nullptr, "%s: dims is NULL", who);
  if (structure->kind == GSS_VG_POWER) {
    set_error("%s: a power structure has no sill, the coregionalisation model needs one", who);
    return GSS_ERR_UNSUPPORTED;
  }
  GSS_REQUIRE(structure->nextra == 0, "%s: one structure plus nugget (nextra = %d)", who, structure->nextra);
  // the checks of gss_cokrig_create, then the factors
  LmcCoef c = {};
  double B0[LMC_MAXZ * LMC_MAXZ] = {}, B1[LMC_MAXZ * LMC_MAXZ] = {};
  double big = 0.0;
  for (int e = 0; e < nz * nz; ++e) {
    GSS_REQUIRE(std::isfinite(b0[e]) && std::isfinite(b1[e]), "%s: b0 / b1 entry [%d][%d] is not finite", who, e / nz,
                e % nz);
    big = std::fmax(big, std::fmax(std::fabs(b0[e]), std::fabs(b1[e])));
  }
  for (int a = 0; a < nz; ++a)
    for (int b = 0; b < nz; ++b) {
      GSS_REQUIRE(std::fabs(b0[a * nz + b] - b0[b * nz + a]) <= 1e-12 * big, "%s: b0 is not symmetric at [%d][%d]", who,
                  a, b);
      GSS_REQUIRE(std::fabs(b1[a * nz + b] - b1[b * nz + a]) <= 1e-12 * big, "%s: b1 is not symmetric at [%d][%d]", who,
                  a, b);
      B0[a * LMC_MAXZ + b] = 0.5 * (b0[a * nz + b] + b0[b * nz + a]);
      B1[a * LMC_MAXZ + b] = 0.5 * (b1[a * nz + b] + b1[b * nz + a]);
    }
  for (int a = 0; a < nz; ++a) {
    GSS_REQUIRE(B0[a * LMC_MAXZ + a] + B1[a * LMC_MAXZ + a] > 0.0, "%s: variable %d has no positive sill "
                "b0[%d][%d] + b1[%d][%d]", who, a, a, a, a, a);
    GSS_REQUIRE(std::isfinite(means[a]), "%s: means[%d] is not finite", who, a);
    c.means[a] = means[a];
  }
  GSS_TRY(lmc_factor(who, "b0", B0, nz, c.L0, &c.live0));
  GSS_TRY(lmc_factor(who, "b1", B1, nz, c.L1, &c.live1));
  gss_variogram_t unit = *structure;   // rho: sill 1, no nugget
  unit.sill = 1.0;
  unit.nugget = 0.0;
  GSS_TRY(gss_fftgs_create(out, &unit, ndim, dims, spacing, 0.0, flags, stream));
  (*out)->lmc_nz = nz;
  (*out)->lmc = c;
  return GSS_OK;
}

int32_t gss_fftgs_realize_lmc(gss_fftgs_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                              const double* nugget_noise, const int64_t* inds, int64_t ninds, double* out, int32_t mem,
                              void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr && out != nullptr && nreals >= 0 && first_real >= 0, "gss_fftgs_realize_lmc: bad arguments");
  GSS_REQUIRE(h->lmc_nz > 0, "gss_fftgs_realize_lmc: the handle is a plain one (gss_fftgs_create): gss_fftgs_realize "
              "realises it, gss_fftgs_create_lmc makes a handle for this call");
  GSS_REQUIRE(h->ready, "handle has no spectrum");
  GSS_REQUIRE(inds == nullptr || ninds >= 0, "gss_fftgs_realize_lmc: ninds = %lld", (long long)ninds);
  if (nreals == 0) return GSS_OK;
  hipStream_t s = to_stream(stream);
  const int nz = h->lmc_nz;
  const int64_t N = h->N, npts = inds ? ninds : N;
  const bool host = mem == GSS_MEM_HOST;
  const size_t joint = sizeof(double) * (size_t)nz * (size_t)N;   // the fields of one realisation
  // Realisations per chunk: what the ring takes at a time for a host destination, what a workspace of the ring's
  // chunk size holds when the fields cannot be realised where the results go (a grid view, staged noise); a device
  // destination without a view is mixed in place, chunked only by the launch grid.
  const bool in_place = !host && !inds;
  int64_t chunk = in_place ? nreals : OutStream::default_chunk(joint, nreals);
  if (chunk > 65535 / nz) chunk = 65535 / nz;   // (grid y of the mix and of the gather)
  if (const char* e = std::getenv("GSS_FFTGS_LMC_CHUNK_REALS")) {   // tests: a chunk loop that runs more than once
    const long long v = std::atoll(e);
    if (v > 0 && v < chunk) chunk = v;
  }
  Staged si;
  OutStream os;
  GSS_TRY(si.in(inds, sizeof(int64_t) * (size_t)(inds ? ninds : 0), mem, s));
  GSS_TRY(os.begin(out, sizeof(double) * (size_t)nz * (size_t)npts, nreals, mem, s, chunk));
  DevBuf ws, un, en;   // fields of a chunk (view), staged uniforms, staged normals
  if (inds) GSS_TRY(ws.alloc(joint * (size_t)chunk));
  if (host && noise) GSS_TRY(un.alloc(joint * (size_t)chunk));
  if (host && nugget_noise) GSS_TRY(en.alloc(joint * (size_t)chunk));
  const uint64_t nseed = seed ^ GSS_FFTGS_LMC_NUGGET_SALT;

  for (int64_t r = 0; r < nreals; r += chunk) {
    const int64_t nb = chunk < nreals - r ? chunk : nreals - r;
    double* dst = nullptr;   // the chunk's place: the caller's HBM or a chunk of the ring (chunks start at multiples)
    GSS_TRY(os.slot(r, s, &dst));
    const double* u = noise ? noise + r * nz * N : nullptr;
    const double* e = nugget_noise ? nugget_noise + r * nz * N : nullptr;
    if (host && u) {
      GSS_HIP(hipMemcpyAsync(un.p, u, joint * (size_t)nb, hipMemcpyHostToDevice, s));
      u = un.as<double>();
    }
    if (host && e) {
      GSS_HIP(hipMemcpyAsync(en.p, e, joint * (size_t)nb, hipMemcpyHostToDevice, s));
      e = en.as<double>();
    }
    double* Z = inds ? ws.as<double>() : dst;
    GSS_TRY(lmc_fields(h, seed, first_real + r, nb, u, Z, s));
    GSS_TRY(lmc_mix_launch(nz, h->lmc, Z, N, nb, nseed, first_real + r, e, s));
    if (inds && ninds > 0) {
      hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((ninds + 255) / 256), (unsigned)(nb * nz)), dim3(256), 0, s, Z,
                         si.as<int64_t>(), ninds, dst, N);
      GSS_HIP(hipGetLastError());
    }
    GSS_TRY(os.done(r + nb - 1, s));
  }
  return os.finish(s);
}

}  // extern "C"
