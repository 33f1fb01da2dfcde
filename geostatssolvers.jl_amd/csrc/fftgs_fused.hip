// FFTGS, fused five-pass pipeline for power-of-two 3-D grids (fftgs_fused.h): setup, launchers, spectrum, the tiled
// amplitudes, one realisation, and the optional two-stream overlap of consecutive realisations.
#include "fftgs_handle.h"
#include "fftgs_fused.h"

#include <cstring>
#include <type_traits>

namespace gss {

static bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
static int ilog2(int64_t v) {
  int l = 0;
  while ((1LL << l) < v) ++l;
  return l;
}

static size_t ff_xfwd2_lds(int M, int logM, int rows) { return sizeof(double2) * (size_t)(M + x_table_len(logM) + rows * M); }
static size_t ff_xinv2_lds(int M, int logM, int rows) { return sizeof(double2) * (size_t)(x_table_len(logM) + rows * M); }
static size_t ff_axis2_lds(int L, int txlog) { return sizeof(double2) * (size_t)(L / 2 + (L << txlog) + FF2_PAD); }

// per-pass twiddle tables of the Stockham x passes (forward sign; the inverse conjugates): middle passes
// T[(r-1) Ns + k] = exp(-2 pi i r k / (8 Ns)), then the last pass exp(-2 pi i r k / M)
static int32_t upload_x_tables(DevBuf& buf, int logM, hipStream_t s) {
  const int M = 1 << logM;
  const XPlan plan = x_plan(logM);
  std::vector<double> t((size_t)(2 * x_table_len(logM)));
  const long double two_pi = 6.283185307179586476925286766559005768L;
  size_t o = 0;
  int Ns = 8;
  for (int m = 0; m < plan.nmid; ++m) {
    for (int r = 1; r < 8; ++r)
      for (int k = 0; k < Ns; ++k) {
        const long double a = two_pi * (long double)(r * k) / (long double)(8 * Ns);
        t[o++] = (double)cosl(a);
        t[o++] = (double)(-sinl(a));
      }
    Ns <<= 3;
  }
  const int R = 1 << plan.ns_last;
  for (int r = 1; r < R; ++r)
    for (int k = 0; k < M / R; ++k) {
      const long double a = two_pi * (long double)(r * k) / (long double)M;
      t[o++] = (double)cosl(a);
      t[o++] = (double)(-sinl(a));
    }
  GSS_TRY(buf.alloc(sizeof(double) * t.size()));
  GSS_HIP(hipMemcpyAsync(buf.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, s));
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

// ---- the kernel variants of a handle: each pick decides both the LDS attribute (setup) and the launch ------------------
template <int V> using IC = std::integral_constant<int, V>;

// x passes <ROWS, 256, LOGM>: f(rows, logm)
template <class F>
static int32_t with_x_variant(const gss_fftgs* h, F&& f) {
  if (h->fg.l1 == 9) return f(IC<8>{}, IC<8>{});   // 512-cell lines (M = 256): the length fixed at compile time
  if (h->x_rows == 8) return f(IC<8>{}, IC<-1>{});
  return f(IC<4>{}, IC<-1>{});
}

// strided passes <MODE, TXLOG, NT, LOGL> of a line of 2^logL points in tiles of 2^txlog columns: f(txlog, nt, fast)
template <class F>
static int32_t with_axis_variant(int txlog, int logL, F&& f) {
  if (txlog == 3 && logL == 9)   // 512-point lines: the pass-by-pass kernel with every load issued up front
    return f(IC<3>{}, IC<512>{}, std::true_type{});
  if (txlog == 3) return f(IC<3>{}, IC<512>{}, std::false_type{});
  return f(IC<2>{}, IC<256>{}, std::false_type{});
}
template <int MODE, int TXL, int NT, bool FAST>
static const void* axis_kernel() {
  if constexpr (FAST) return reinterpret_cast<const void*>(ff_axis2_fast_kernel<MODE, TXL, NT, 9>);
  else return reinterpret_cast<const void*>(ff_axis2_kernel<MODE, TXL, NT, -1>);
}

static int32_t set_lds(const void* kernel, size_t bytes) {
  GSS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return GSS_OK;
}

// ---- launchers (X: the half-spectrum buffer they work on) --------------------------------------------------------------
template <int SRC>
static void launch_p1(gss_fftgs* h, double2* X, uint64_t seed, uint32_t real, const double* noise, hipStream_t s) {
  const FusedGrid& f = h->fg;
  const int M = f.n1 / 2;
  const int64_t nrows = (int64_t)f.n2 * f.n3;
  const CovSrc* cs = h->covsrc.as<CovSrc>();
  const unsigned gx = (unsigned)((nrows + h->x_rows - 1) / h->x_rows);
  const size_t lds = ff_xfwd2_lds(M, f.l1 - 1, h->x_rows);
  (void)with_x_variant(h, [&](auto rows, auto logm) -> int32_t {
    hipLaunchKernelGGL((ff_x_fwd2_kernel<SRC, decltype(rows)::value, 256, decltype(logm)::value>), dim3(gx), dim3(256), lds, s, f,
                       h->tw1.as<double2>(), h->xtw.as<double2>(), seed, real, noise, X, cs);
    return GSS_OK;
  });
}

static void launch_p5(gss_fftgs* h, const double2* X, double* z, hipStream_t s) {
  const FusedGrid& f = h->fg;
  const int M = f.n1 / 2;
  const int64_t nrows = (int64_t)f.n2 * f.n3;
  const unsigned gx = (unsigned)((nrows + h->x_rows - 1) / h->x_rows);
  const size_t lds = ff_xinv2_lds(M, f.l1 - 1, h->x_rows);
  (void)with_x_variant(h, [&](auto rows, auto logm) -> int32_t {
    hipLaunchKernelGGL((ff_x_inv2_kernel<decltype(rows)::value, 256, decltype(logm)::value>), dim3(gx), dim3(256), lds, s, f,
                       h->tw1.as<double2>(), h->xtw.as<double2>(), X, z);
    return GSS_OK;
  });
}

// strided pass `mode` (0 forward, 1 inverse, 2 forward-phase-inverse) along y (axis 1) or z (axis 2)
template <int MODE>
static int32_t launch_axis_mode(gss_fftgs* h, double2* X, int axis, hipStream_t s, int slab_t0 = 0, int slab_nt = 0) {
  FusedGrid f = h->fg;
  f.slab_t0 = slab_t0;
  f.slab_nt = slab_nt;
  const int L = axis == 1 ? f.n2 : f.n3, logL = axis == 1 ? f.l2 : f.l3, nouter = axis == 1 ? f.n3 : f.n2;
  const double2* tw = axis == 1 ? h->tw2.as<double2>() : h->tw3.as<double2>();
  const int64_t ostride = axis == 1 ? (int64_t)f.n2 * f.nhp : (int64_t)f.nhp;
  const int64_t lstride = axis == 1 ? (int64_t)f.nhp : (int64_t)f.n2 * f.nhp;
  const double* fh = MODE == 2 ? h->Fh_tiled.as<double>() : nullptr;
  const double mean = MODE == 2 ? h->mean : 0.0;
  const int txlog = axis == 1 ? h->txy_log : h->txz_log;
  const unsigned blocks = (unsigned)(nouter * (slab_nt > 0 ? slab_nt : (f.nhp >> txlog)));
  const size_t lds = ff_axis2_lds(L, txlog);
  if (slab_nt > 0 && !(txlog == 3 && logL == 9)) return GSS_ERR_UNSUPPORTED;
  GSS_TRY(with_axis_variant(txlog, logL, [&](auto txl, auto nt, auto fast) -> int32_t {
    constexpr int T = decltype(txl)::value, NT = decltype(nt)::value;
    if constexpr (decltype(fast)::value)
      hipLaunchKernelGGL((ff_axis2_fast_kernel<MODE, T, NT, 9>), dim3(blocks), dim3(NT), lds, s, f, tw, ostride, lstride, X,
                         fh, mean);
    else
      hipLaunchKernelGGL((ff_axis2_kernel<MODE, T, NT, -1>), dim3(blocks), dim3(NT), lds, s, f, logL, tw, ostride, lstride,
                         X, fh, mean);
    return GSS_OK;
  }));
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// The fused five-pass pipeline serves 3-D grids whose sizes are powers of two (32..1024 along x, 16..1024 along
// y and z); everything else, and GSS_FFTGS_PATH=rocfft, is left to the other pipelines.
int32_t fftgs_setup_fused(gss_fftgs* h, hipStream_t s) {
  const char* e = std::getenv("GSS_FFTGS_PATH");
  if (e && (std::strcmp(e, "rocfft") == 0 || std::strcmp(e, "generic") == 0)) return GSS_OK;
  const GridSpec& g = h->g;
  if (h->ndim != 3 || !pow2(g.n1) || !pow2(g.n2) || !pow2(g.n3)) return GSS_OK;
  if (g.n1 < 32 || g.n1 > 1024 || g.n2 < 16 || g.n2 > 1024 || g.n3 < 16 || g.n3 > 1024) return GSS_OK;
  // Small grids are left to the generic passes, where eight and more realisations share every launch (measured, ms per
  // realisation, fused / generic: 32^3 0.019 / 0.003, 64^3 0.024 / 0.011, 128 x 128 x 64 0.049 / 0.034, 128^3 0.064 /
  // 0.059, 256 x 128 x 128 0.095 / 0.127): up to a 12 MiB half spectrum.  GSS_FFTGS_PATH=fused keeps them here.
  const bool force = e && std::strcmp(e, "fused") == 0;
  if (!force && sizeof(double2) * (size_t)((g.nh + 7) / 8 * 8) * g.n2 * g.n3 <= ((size_t)12 << 20)) return GSS_OK;
  FusedGrid f;
  f.n1 = (int)g.n1; f.n2 = (int)g.n2; f.n3 = (int)g.n3;
  f.l1 = ilog2(g.n1); f.l2 = ilog2(g.n2); f.l3 = ilog2(g.n3);
  f.nh = (int)g.nh;
  f.nhp = (f.nh + FF_PITCH_ALIGN - 1) / FF_PITCH_ALIGN * FF_PITCH_ALIGN;
  f.ntx = f.nhp / FF_TX;
  f.slab_t0 = f.slab_nt = 0;
  h->fg = f;
  GSS_TRY(upload_twiddles(h->tw1, f.n1, s));
  GSS_TRY(upload_twiddles(h->tw2, f.n2, s));
  GSS_TRY(upload_twiddles(h->tw3, f.n3, s));
  const int64_t nt = (int64_t)f.n2 * f.ntx * f.n3 * FF_TX;
  GSS_TRY(h->Fh_tiled.alloc(sizeof(double) * (size_t)nt));
  const int M = f.n1 / 2;
  const int lmax = f.n2 > f.n3 ? f.n2 : f.n3;
  // Stockham x passes: as many lines per workgroup as give every thread one radix-8 item
  h->x_rows = M <= 256 ? 8 : 4;
  GSS_TRY(upload_x_tables(h->xtw, f.l1 - 1, s));
  GSS_TRY(with_x_variant(h, [&](auto rows, auto logm) -> int32_t {
    constexpr int R = decltype(rows)::value, LM = decltype(logm)::value;
    const size_t fwd = ff_xfwd2_lds(M, f.l1 - 1, R);
    GSS_TRY(set_lds(reinterpret_cast<const void*>(ff_x_fwd2_kernel<FF_SRC_PHILOX, R, 256, LM>), fwd));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(ff_x_fwd2_kernel<FF_SRC_ARRAY, R, 256, LM>), fwd));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(ff_x_fwd2_kernel<FF_SRC_COV, R, 256, LM>), fwd));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(ff_x_fwd2_kernel<FF_SRC_COV_ROT, R, 256, LM>), fwd));
    return set_lds(reinterpret_cast<const void*>(ff_x_inv2_kernel<R, 256, LM>), ff_xinv2_lds(M, f.l1 - 1, R));
  }));
  // the half-spectrum buffer of the fused path has the padded row pitch; padding columns stay zero
  GSS_TRY(h->X.alloc(sizeof(double2) * (size_t)f.nhp * f.n2 * f.n3));
  GSS_TRY(dev_zero_bytes(h->X.p, h->X.bytes, s));
  // measured (profiles/r02_fftgs_overlap.txt): the two-stream pipeline changes nothing at 512^3 (2.378 against
  // 2.367 ms per realisation) -- the passes fill the chip and the queues take turns; kept as an A/B switch, off
  h->overlap = env_int("GSS_FFTGS_OVERLAP", 0) != 0;
  // strided passes: 8-column tiles (4 when a 1024-point line would not leave room in LDS); the LDS bound of a kernel
  // that both axes use is that of the longer line
  h->txy_log = f.n2 > 512 ? 2 : 3;
  h->txz_log = f.n3 > 512 ? 2 : 3;
  for (int axis = 1; axis <= 2; ++axis)
    GSS_TRY(with_axis_variant(axis == 1 ? h->txy_log : h->txz_log, axis == 1 ? f.l2 : f.l3, [&](auto txl, auto nt, auto fast) -> int32_t {
      constexpr int T = decltype(txl)::value, NT = decltype(nt)::value;
      constexpr bool FAST = decltype(fast)::value;
      const size_t lds = ff_axis2_lds(FAST ? 512 : lmax, T);
      GSS_TRY(set_lds(axis_kernel<0, T, NT, FAST>(), lds));
      GSS_TRY(set_lds(axis_kernel<1, T, NT, FAST>(), lds));
      return set_lds(axis_kernel<2, T, NT, FAST>(), lds);
    }));
  h->path = FftgsPath::FUSED;
  return GSS_OK;
}

// fft.jl:96-103 on the fused passes: covariance rows are produced inside P1 (no N-sized input array), then the y and
// z forward passes; the amplitude kernel undoes the bit reversal while it writes the natural-order state.
int32_t fftgs_spectrum_fused(gss_fftgs* h, double* partial, hipStream_t s) {
  const FusedGrid& f = h->fg;
  double2* X = h->X.as<double2>();
  CovSrc cs;
  cs.vg = h->vg;
  cs.c1 = (int)h->g.c1; cs.c2 = (int)h->g.c2; cs.c3 = (int)h->g.c3;
  cs.s1 = h->g.s1; cs.s2 = h->g.s2; cs.s3 = h->g.s3;
  GSS_TRY(h->covsrc.alloc(sizeof(CovSrc)));
  GSS_HIP(hipMemcpyAsync(h->covsrc.p, &cs, sizeof(CovSrc), hipMemcpyHostToDevice, s));
  GSS_HIP(hipStreamSynchronize(s));  // `cs` is a stack object
  if (h->rotated) launch_p1<FF_SRC_COV_ROT>(h, X, 0, 0, h->rot.as<double>(), s);
  else launch_p1<FF_SRC_COV>(h, X, 0, 0, nullptr, s);
  GSS_TRY(launch_axis_mode<0>(h, X, 1, s));
  GSS_TRY(launch_axis_mode<0>(h, X, 2, s));
  hipLaunchKernelGGL(ff_amp_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, f, X, h->Fh(), partial);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// the amplitudes in the tile order of P3
int32_t fftgs_tile_fused(gss_fftgs* h, hipStream_t s) {
  const FusedGrid& f = h->fg;
  const int64_t nt = (int64_t)f.n2 * f.ntx * f.n3 * FF_TX;
  if (h->txz_log == 3)
    hipLaunchKernelGGL(ff_tile_fh2_kernel<3>, dim3(grid_blocks(nt)), dim3(256), 0, s, f, h->Fh(), h->Fh_tiled.as<double>());
  else
    hipLaunchKernelGGL(ff_tile_fh2_kernel<2>, dim3(grid_blocks(nt)), dim3(256), 0, s, f, h->Fh(), h->Fh_tiled.as<double>());
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// P1 of one realisation; `noise` (N uniforms) may be NULL
static int32_t fftgs_fused_p1(gss_fftgs* h, double2* X, uint64_t seed, int64_t real, const double* noise, hipStream_t s) {
  ProfScope ps("fftgs_p1", s);
  if (noise) launch_p1<FF_SRC_ARRAY>(h, X, seed, (uint32_t)real, noise, s);
  else launch_p1<FF_SRC_PHILOX>(h, X, seed, (uint32_t)real, nullptr, s);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// P2 .. P5; z receives N doubles
static int32_t fftgs_fused_rest(gss_fftgs* h, double2* X, double* z, hipStream_t s) {
  // slab order (fftgs_slab_schedule): GSS_FFTGS_SLAB tiles per slab, 512-point lines; GSS_FFTGS_SLAB=0: whole buffer per pass
  static const int slab = env_int("GSS_FFTGS_SLAB", 2);
  const FusedGrid& f = h->fg;
  const bool can_slab = slab > 0 && h->txy_log == 3 && h->txz_log == 3 && f.l2 == 9 && f.l3 == 9;
  if (can_slab) {
    ProfScope ps("fftgs_p234", s);
    GSS_TRY(fftgs_slab_schedule(h, s, f.nhp >> 3, slab, [&](hipStream_t st, int t0, int nt) -> int32_t {
      GSS_TRY(launch_axis_mode<0>(h, X, 1, st, t0, nt));
      GSS_TRY(launch_axis_mode<2>(h, X, 2, st, t0, nt));
      return launch_axis_mode<1>(h, X, 1, st, t0, nt);
    }));
  } else {
    {
      ProfScope ps("fftgs_p2", s);
      GSS_TRY(launch_axis_mode<0>(h, X, 1, s));
    }
    {
      ProfScope ps("fftgs_p3", s);
      GSS_TRY(launch_axis_mode<2>(h, X, 2, s));
    }
    {
      ProfScope ps("fftgs_p4", s);
      GSS_TRY(launch_axis_mode<1>(h, X, 1, s));
    }
  }
  {
    ProfScope ps("fftgs_p5", s);
    launch_p5(h, X, z, s);
  }
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

int32_t fftgs_fields_fused(gss_fftgs* h, uint64_t seed, int64_t real, const double* noise, double* z, hipStream_t s) {
  double2* X = h->X.as<double2>();
  GSS_TRY(fftgs_fused_p1(h, X, seed, real, noise, s));
  return fftgs_fused_rest(h, X, z, s);
}

// helper stream, events and the second half-spectrum buffer of the two-stream overlap (first such call); everything
// queued so far (inputs, earlier calls) precedes the helper stream's first kernel
int32_t fftgs_fused_overlap_begin(gss_fftgs* h, hipStream_t s) {
  if (!h->s2) {
    const FusedGrid& f = h->fg;
    GSS_TRY(h->X2.alloc(sizeof(double2) * (size_t)f.nhp * f.n2 * f.n3));
    GSS_TRY(dev_zero_bytes(h->X2.p, h->X2.bytes, s));   // padding columns stay zero, as in X
    GSS_HIP(hipStreamCreateWithFlags(&h->s2, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      GSS_HIP(hipEventCreateWithFlags(&h->ev_p1[b], hipEventDisableTiming));
      GSS_HIP(hipEventCreateWithFlags(&h->ev_p5[b], hipEventDisableTiming));
    }
    GSS_HIP(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
  }
  GSS_HIP(hipEventRecord(h->ev_in, s));
  GSS_HIP(hipStreamWaitEvent(h->s2, h->ev_in, 0));
  return GSS_OK;
}

// realisation r of the call: P1 on the helper stream into buffer r mod 2, beside P2..P5 of realisation r - 1 on s
int32_t fftgs_fused_overlap_field(gss_fftgs* h, int64_t r, uint64_t seed, int64_t real, const double* noise, double* z,
                                  hipStream_t s) {
  const int b = (int)(r & 1);
  double2* X = b ? h->X2.as<double2>() : h->X.as<double2>();
  if (r >= 2) GSS_HIP(hipStreamWaitEvent(h->s2, h->ev_p5[b], 0));   // buffer b is free again
  GSS_TRY(fftgs_fused_p1(h, X, seed, real, noise, h->s2));
  GSS_HIP(hipEventRecord(h->ev_p1[b], h->s2));
  GSS_HIP(hipStreamWaitEvent(s, h->ev_p1[b], 0));
  GSS_TRY(fftgs_fused_rest(h, X, z, s));
  GSS_HIP(hipEventRecord(h->ev_p5[b], s));
  return GSS_OK;
}

}  // namespace gss
