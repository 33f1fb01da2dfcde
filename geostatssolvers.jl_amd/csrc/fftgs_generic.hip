// FFTGS, generic pipeline (fftgs_generic.h): 1-D and 2-D grids and the 3-D grids that the power-of-two pipeline does not
// take, sizes 2^a 3^b 5^c 7^d.  Setup, launchers (with the split of long y lines), spectrum, the tiled amplitudes and a
// batch of realisations.
#include "fftgs_handle.h"
#include "fftgs_generic.h"

#include <cstring>
#include <type_traits>

namespace gss {

static bool gen_plan(int L, GenPlan* pl) {
  std::memset(pl, 0, sizeof(*pl));
  pl->L = L;
  int n = L, np = 0;
  while (n % 7 == 0 && np < GEN_MAX_PASSES - 4) { pl->radix[np++] = 7; n /= 7; }
  while (n % 5 == 0) { pl->radix[np++] = 5; n /= 5; if (np >= GEN_MAX_PASSES - 4) break; }
  while (n % 3 == 0 && np < GEN_MAX_PASSES - 4) { pl->radix[np++] = 3; n /= 3; }
  int e = 0;
  while (n % 2 == 0) { ++e; n /= 2; }
  if (n != 1 || L < 2) return false;
  while (e >= 3 && np < GEN_MAX_PASSES) { pl->radix[np++] = 8; e -= 3; }
  if (e == 2 && np < GEN_MAX_PASSES) { pl->radix[np++] = 4; e = 0; }
  if (e == 1 && np < GEN_MAX_PASSES) { pl->radix[np++] = 2; e = 0; }
  if (e != 0) return false;
  pl->npass = np;
  int off = 0, Ns = 1;
  for (int p = 0; p < np; ++p) {
    pl->toff[p] = off;
    off += (pl->radix[p] - 1) * Ns;
    Ns *= pl->radix[p];
  }
  pl->tlen = off;
  pl->has7 = np > 0 && pl->radix[0] == 7;
  return Ns == L;
}

static int32_t gen_upload_table(DevBuf& buf, const GenPlan& pl, hipStream_t s) {
  std::vector<double> t((size_t)2 * (pl.tlen > 0 ? pl.tlen : 1), 0.0);
  const long double two_pi = 6.283185307179586476925286766559005768L;
  int Ns = 1;
  for (int p = 0; p < pl.npass; ++p) {
    const int R = pl.radix[p];
    for (int r = 1; r < R; ++r)
      for (int k = 0; k < Ns; ++k) {
        const long double a = two_pi * (long double)r * (long double)k / ((long double)Ns * (long double)R);
        const size_t e = (size_t)(pl.toff[p] + (r - 1) * Ns + k);
        t[2 * e] = (double)cosl(a);
        t[2 * e + 1] = (double)(-sinl(a));
      }
    Ns *= R;
  }
  GSS_TRY(buf.alloc(sizeof(double) * t.size()));
  GSS_HIP(hipMemcpyAsync(buf.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, s));
  GSS_HIP(hipStreamSynchronize(s));
  return GSS_OK;
}

static size_t gen_x_lds(const GenPlan& pl, int rows, bool tg) { return sizeof(double2) * (size_t)((tg ? 0 : pl.L + pl.tlen) + rows * pl.L); }
static size_t gen_axis_lds(const GenPlan& pl, int txlog) { return sizeof(double2) * (size_t)(pl.tlen + (pl.L << txlog)); }


// ---- the kernel variants of a handle: each pick decides both the LDS attribute (setup) and the launch ------------------
// x passes <TG>: f(tg)
template <class F>
static int32_t with_x_variant(const gss_fftgs* h, F&& f) {
  return h->g_tg ? f(std::true_type{}) : f(std::false_type{});
}
// strided passes <MODE, TXLOG>: f(txlog)
template <class F>
static int32_t with_axis_variant(int txlog, F&& f) {
  return txlog == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 2>{});
}
static int32_t set_lds(const void* kernel, size_t bytes) {
  GSS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return GSS_OK;
}

// 1-D and 2-D grids and 3-D grids that the power-of-two pipeline does not take, sizes 2^a 3^b 5^c 7^d: n1 even with n1 / 2 <= 2 048,
// the other axes <= 1 024.  Everything else stays on rocFFT.
int32_t fftgs_setup_generic(gss_fftgs* h, hipStream_t s) {
  const char* e = std::getenv("GSS_FFTGS_PATH");
  if (e && std::strcmp(e, "rocfft") == 0) return GSS_OK;
  const GridSpec& g = h->g;
  if (h->path != FftgsPath::ROCFFT || (g.n1 & 1) || g.n1 / 2 > 2048 || g.n1 < 4 || g.n3 > 1024) return GSS_OK;
  const bool lng = h->ndim == 2 && g.n2 > 1024;
  if (g.n2 > (lng ? 4096 : 1024)) return GSS_OK;
  GenPlan p1, p2, p3;
  std::memset(&p2, 0, sizeof(p2));
  if (!gen_plan((int)(g.n1 / 2), &p1)) return GSS_OK;
  if (h->ndim >= 2 && !gen_plan((int)g.n2, &p2)) return GSS_OK;   // (1-D grids: the x passes and an elementwise phase step)
  if (lng) {
    // n2 = L1 L2 with both factors <= 64 (L2 the largest such divisor); tiles of at most 4 096 elements
    GenLong& gl = h->gl;
    gl.L2 = 0;
    for (int d = 64; d >= 2; --d)
      if (g.n2 % d == 0 && g.n2 / d <= 64) { gl.L2 = d; break; }
    if (gl.L2 == 0) return GSS_OK;
    gl.L1 = (int)g.n2 / gl.L2;
    if (!gen_plan(gl.L1, &h->gpl[0]) || !gen_plan(gl.L2, &h->gpl[1])) return GSS_OK;
    gl.NB = gl.NC = 1;
    for (int d = 1; d <= gl.L2; ++d)
      if (gl.L2 % d == 0 && gl.L1 * d <= (h->gpl[0].has7 ? 448 : 512)) gl.NB = d;
    for (int d = 1; d <= gl.L1; ++d)
      if (gl.L1 % d == 0 && gl.L2 * d <= (h->gpl[1].has7 ? 448 : 512)) gl.NC = d;
  }
  if (h->ndim == 3 && !gen_plan((int)g.n3, &p3)) return GSS_OK;
  if (h->ndim < 3) std::memset(&p3, 0, sizeof(p3));
  h->gp[0] = p1; h->gp[1] = p2; h->gp[2] = p3;
  GenGrid& gg = h->gg;
  gg.n1 = (int)g.n1; gg.n2 = (int)g.n2; gg.n3 = (int)g.n3;
  gg.nh = (int)g.nh;
  gg.nhp = (gg.nh + 7) / 8 * 8;
  gg.ndim = h->ndim;
  gg.c1 = (int)g.c1; gg.c2 = (int)g.c2; gg.c3 = (int)g.c3;
  gg.s1 = g.s1; gg.s2 = g.s2; gg.s3 = g.s3;
  h->g_rows = (int)((p1.has7 ? 1792 : 2048) / p1.L);
  if (h->g_rows > 16) h->g_rows = 16;
  if (h->g_rows < 1) return GSS_OK;          // (a line of 7 x 2^k > 1 792 elements: rocFFT)
  {
    // tables in the LDS unless they cost occupancy: more workgroups per CU (of 160 KB, at most 8) without them
    const int with = (int)((size_t)(160 << 10) / gen_x_lds(p1, h->g_rows, false));
    const int without = (int)((size_t)(160 << 10) / gen_x_lds(p1, h->g_rows, true));
    static const int tg_env = env_int("GSS_FFTGS_GEN_TG", -1);
    h->g_tg = tg_env >= 0 ? tg_env != 0 : (with <= 2 && without > with);   // (three and more: measured neutral, 1 000^2)
  }
  h->g_txlog[1] = p2.L <= (p2.has7 ? 448 : 512) ? 3 : 2;
  h->g_txlog[2] = (h->ndim == 3 && p3.L > (p3.has7 ? 448 : 512)) ? 2 : 3;
  if (!lng && p2.has7 && p2.L > 896) return GSS_OK;      // (980, 1 008: four columns of the line exceed 3 584 elements)
  if (h->ndim == 3 && p3.has7 && p3.L > 896) return GSS_OK;
  GSS_TRY(upload_twiddles(h->tw1, gg.n1, s));
  GSS_TRY(gen_upload_table(h->gtab[0], p1, s));
  if (lng) {
    GSS_TRY(gen_upload_table(h->gltab[0], h->gpl[0], s));
    GSS_TRY(gen_upload_table(h->gltab[1], h->gpl[1], s));
    std::vector<double> w((size_t)2 * g.n2);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int64_t k = 0; k < g.n2; ++k) {
      const long double a = two_pi * (long double)k / (long double)g.n2;
      w[2 * k] = (double)cosl(a);
      w[2 * k + 1] = (double)(-sinl(a));
    }
    GSS_TRY(h->gtwl.alloc(sizeof(double) * w.size()));
    GSS_HIP(hipMemcpyAsync(h->gtwl.p, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, s));
    GSS_HIP(hipStreamSynchronize(s));
  } else if (h->ndim >= 2) {
    GSS_TRY(gen_upload_table(h->gtab[1], p2, s));
  }
  if (h->ndim == 3) GSS_TRY(gen_upload_table(h->gtab[2], p3, s));
  // Small grids do not fill the device (100 x 100: seven workgroups in GP1) and their three or five launches cost more
  // than their work: up to g_batch realisations share every launch (blockIdx.y), each with a half-spectrum buffer of its
  // own -- as many as fit 96 MiB (the buffers of a batch stay in the memory-side cache between the passes), at most 64.
  h->g_xbs = (int64_t)gg.nhp * gg.n2 * gg.n3;
  {
    static const int batch_env = env_int("GSS_FFTGS_GEN_BATCH", 0);
    int64_t b = ((int64_t)96 << 20) / (int64_t)(sizeof(double2) * (size_t)h->g_xbs);
    if (b > 64) b = 64;
    if (batch_env > 0) b = batch_env;
    if (b < 1) b = 1;
    h->g_batch = (int)b;
  }
  GSS_TRY(h->X.alloc(sizeof(double2) * (size_t)h->g_xbs * h->g_batch));
  GSS_TRY(dev_zero_bytes(h->X.p, h->X.bytes, s));   // the padding columns stay zero
  GSS_TRY(h->Fh_tiled.alloc(sizeof(double) * (size_t)gg.nhp * gg.n2 * gg.n3));   // amplitudes in the last pass's tile order
  // (one fixed bound per kernel for every handle: the attribute belongs to the function, not to the launch)
  GSS_TRY(with_x_variant(h, [&](auto tg) -> int32_t {
    constexpr bool TG = decltype(tg)::value;
    const size_t lx = 104 * 1024;
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_x_fwd_kernel<FF_SRC_PHILOX, TG>), lx));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_x_fwd_kernel<FF_SRC_ARRAY, TG>), lx));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_x_fwd_kernel<FF_SRC_COV, TG>), lx));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_x_fwd_kernel<FF_SRC_COV_ROT, TG>), lx));
    return set_lds(reinterpret_cast<const void*>(gen_x_inv_kernel<TG>), lx);
  }));
  const size_t la = 96 * 1024;
  for (int axis = 1; axis < h->ndim && !lng; ++axis)
    GSS_TRY(with_axis_variant(h->g_txlog[axis], [&](auto txl) -> int32_t {
      constexpr int T = decltype(txl)::value;
      GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_axis_kernel<0, T>), la));
      GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_axis_kernel<1, T>), la));
      return set_lds(reinterpret_cast<const void*>(gen_axis_kernel<2, T>), la);
    }));
  if (lng) {
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_long_outer_kernel<false>), la));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_long_outer_kernel<true>), la));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_long_inner_kernel<0>), la));
    GSS_TRY(set_lds(reinterpret_cast<const void*>(gen_long_inner_kernel<2>), la));
  }
  h->g_long = lng;
  h->path = FftgsPath::GENERIC;
  return GSS_OK;
}

// ---- launchers (nb: realisations in this launch, grid y) ---------------------------------------------------------------
template <int SRC>
static void gen_launch_p1(gss_fftgs* h, uint64_t seed, uint32_t real, const double* noise, hipStream_t s, int nb = 1,
                          const BatchStep& bs = BatchStep()) {
  const GenGrid& g = h->gg;
  const int64_t nbs = bs.noise > 0 ? bs.noise : h->N;
  const int64_t nrows = (int64_t)g.n2 * g.n3;
  const unsigned gx = (unsigned)((nrows + h->g_rows - 1) / h->g_rows);
  (void)with_x_variant(h, [&](auto tg) -> int32_t {
    constexpr bool TG = decltype(tg)::value;
    hipLaunchKernelGGL((gen_x_fwd_kernel<SRC, TG>), dim3(gx, nb), dim3(GEN_XNT), gen_x_lds(h->gp[0], h->g_rows, TG), s, g, h->gp[0],
                       h->g_rows, h->tw1.as<double2>(), h->gtab[0].as<double2>(), seed, real, noise, h->X.as<double2>(), h->vg,
                       h->g_xbs, bs.real, nbs);
    return GSS_OK;
  });
}
static void gen_launch_p5(gss_fftgs* h, double* z, hipStream_t s, int nb = 1, int64_t obs = 0) {
  const GenGrid& g = h->gg;
  if (obs <= 0) obs = h->N;
  const int64_t nrows = (int64_t)g.n2 * g.n3;
  const unsigned gx = (unsigned)((nrows + h->g_rows - 1) / h->g_rows);
  (void)with_x_variant(h, [&](auto tg) -> int32_t {
    constexpr bool TG = decltype(tg)::value;
    hipLaunchKernelGGL(gen_x_inv_kernel<TG>, dim3(gx, nb), dim3(GEN_XNT), gen_x_lds(h->gp[0], h->g_rows, TG), s, g, h->gp[0], h->g_rows,
                       h->tw1.as<double2>(), h->gtab[0].as<double2>(), h->X.as<double2>(), z, h->g_xbs, obs);
    return GSS_OK;
  });
}
// strided pass `MODE` along y (axis 1) or z (axis 2)
template <int MODE>
static void gen_launch_axis(gss_fftgs* h, int axis, hipStream_t s, int slab_t0 = 0, int slab_nt = 0, int nb = 1) {
  const GenGrid& g = h->gg;
  const GenPlan& pl = h->gp[axis];
  const int txlog = h->g_txlog[axis];
  const int nouter = axis == 1 ? g.n3 : g.n2;
  const int64_t ostride = axis == 1 ? (int64_t)g.n2 * g.nhp : (int64_t)g.nhp;
  const int64_t lstride = axis == 1 ? (int64_t)g.nhp : (int64_t)g.n2 * g.nhp;
  const unsigned blocks = (unsigned)(nouter * (slab_nt > 0 ? slab_nt : (g.nhp >> txlog)));
  const size_t lds = gen_axis_lds(pl, txlog);
  (void)with_axis_variant(txlog, [&](auto txl) -> int32_t {
    hipLaunchKernelGGL((gen_axis_kernel<MODE, decltype(txl)::value>), dim3(blocks, nb), dim3(GEN_ANT), lds, s, g, pl, axis,
                       h->gtab[axis].as<double2>(), ostride, lstride, h->X.as<double2>(), h->Fh_tiled.as<double>(), h->mean,
                       slab_t0, slab_nt, h->g_xbs);
    return GSS_OK;
  });
}

// the y pass of a 2-D grid with long lines (fftgs_generic.h: outer / inner / outer); MODE 0: forward only, left in the
// order frequency c + L1 d at row L2 c + d
template <int MODE>
static void gen_launch_long(gss_fftgs* h, hipStream_t s, int nb = 1) {
  const GenGrid& g = h->gg;
  const GenLong& gl = h->gl;
  const unsigned ntx = (unsigned)(g.nhp >> 3);
  const size_t lo = sizeof(double2) * (size_t)(h->gpl[0].tlen + gl.L1 * gl.NB * 8);
  const size_t li = sizeof(double2) * (size_t)(h->gpl[1].tlen + gl.L2 * gl.NC * 8);
  hipLaunchKernelGGL(gen_long_outer_kernel<false>, dim3(ntx * (unsigned)(gl.L2 / gl.NB), nb), dim3(GEN_ANT), lo, s, g, h->gpl[0], gl,
                     h->gltab[0].as<double2>(), h->gtwl.as<double2>(), h->X.as<double2>(), h->g_xbs);
  hipLaunchKernelGGL(gen_long_inner_kernel<MODE>, dim3(ntx * (unsigned)(gl.L1 / gl.NC), nb), dim3(GEN_ANT), li, s, g, h->gpl[1], gl,
                     h->gltab[1].as<double2>(), h->X.as<double2>(), h->Fh_tiled.as<double>(), h->mean, h->g_xbs);
  if (MODE == 2)
    hipLaunchKernelGGL(gen_long_outer_kernel<true>, dim3(ntx * (unsigned)(gl.L2 / gl.NB), nb), dim3(GEN_ANT), lo, s, g, h->gpl[0], gl,
                       h->gltab[0].as<double2>(), h->gtwl.as<double2>(), h->X.as<double2>(), h->g_xbs);
}

// fft.jl:96-103 on the generic passes
int32_t fftgs_spectrum_generic(gss_fftgs* h, double* partial, hipStream_t s) {
  if (h->rotated) gen_launch_p1<FF_SRC_COV_ROT>(h, 0, 0, h->rot.as<double>(), s);
  else gen_launch_p1<FF_SRC_COV>(h, 0, 0, nullptr, s);
  if (h->g_long) gen_launch_long<0>(h, s);
  else if (h->ndim >= 2) gen_launch_axis<0>(h, 1, s);
  if (h->ndim == 3) gen_launch_axis<0>(h, 2, s);
  hipLaunchKernelGGL(gen_amp_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, h->gg, h->X.as<double2>(), h->Fh(), partial,
                     h->g_long ? h->gl.L1 : 0, h->g_long ? h->gl.L2 : 0);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// the amplitudes in the tile order of the last strided pass (1-D grids read the state as it is)
int32_t fftgs_tile_generic(gss_fftgs* h, hipStream_t s) {
  if (h->ndim < 2) return GSS_OK;
  const int axis = h->ndim == 3 ? 2 : 1;
  const int64_t nt = (int64_t)h->gg.nhp * h->gg.n2 * h->gg.n3;
  if (h->g_long)
    hipLaunchKernelGGL(gen_tile_fh_long_kernel, dim3(grid_blocks(nt)), dim3(256), 0, s, h->gg, h->gl, h->Fh(),
                       h->Fh_tiled.as<double>());
  else if (h->g_txlog[axis] == 3)
    hipLaunchKernelGGL(gen_tile_fh_kernel<3>, dim3(grid_blocks(nt)), dim3(256), 0, s, h->gg, axis, h->gp[axis].L, h->Fh(),
                       h->Fh_tiled.as<double>());
  else
    hipLaunchKernelGGL(gen_tile_fh_kernel<2>, dim3(grid_blocks(nt)), dim3(256), 0, s, h->gg, axis, h->gp[axis].L, h->Fh(),
                       h->Fh_tiled.as<double>());
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

// nb realisations in the same launches (fft.jl:163-170): five passes on 3-D grids, three on 2-D grids
int32_t fftgs_fields_generic(gss_fftgs* h, uint64_t seed, int64_t real, int nb, const BatchStep& bs, const double* noise,
                             double* z, hipStream_t s) {
  ProfScope ps("fftgs_generic", s);
  if (noise) gen_launch_p1<FF_SRC_ARRAY>(h, seed, (uint32_t)real, noise, s, nb, bs);
  else gen_launch_p1<FF_SRC_PHILOX>(h, seed, (uint32_t)real, nullptr, s, nb, bs);
  if (h->ndim == 3) {
    // The slab order of the power-of-two pipeline (fftgs_slab_schedule) is available here as an A/B switch only:
    // measured (round 4, bit-identical fields) 500^3 2.96 ms with it against 2.79 without, 400^3 1.62 / 1.64 -- these
    // passes are not bound by memory alone (GP3 is two transforms and the phase step per trip), so what the cache
    // saves the extra launches give back.  GSS_FFTGS_GEN_SLAB=<tiles of the 512^3 measure per slab> switches it on.
    static const int slab = env_int("GSS_FFTGS_GEN_SLAB", 0);
    const GenGrid& g = h->gg;
    const bool can_slab = slab > 0 && nb == 1 && h->g_txlog[1] == 3 && h->g_txlog[2] == 3 && h->X.bytes > ((size_t)200 << 20);
    if (can_slab) {
      // slabs of about the same bytes as two tiles of the 512^3 buffer (67 MB)
      int per = (int)(((size_t)64 << 20) / ((size_t)g.n2 * g.n3 * 128)) * slab / 2;
      if (per < 1) per = 1;
      GSS_TRY(fftgs_slab_schedule(h, s, g.nhp >> 3, per, [&](hipStream_t st, int t0, int nt) -> int32_t {
        gen_launch_axis<0>(h, 1, st, t0, nt);
        gen_launch_axis<2>(h, 2, st, t0, nt);
        gen_launch_axis<1>(h, 1, st, t0, nt);
        return GSS_OK;
      }));
    } else {
      gen_launch_axis<0>(h, 1, s, 0, 0, nb);
      gen_launch_axis<2>(h, 2, s, 0, 0, nb);
      gen_launch_axis<1>(h, 1, s, 0, 0, nb);
    }
  } else if (h->ndim == 1) {
    hipLaunchKernelGGL(gen_phase1d_kernel, dim3((unsigned)((h->gg.nh + 255) / 256), nb), dim3(256), 0, s, h->gg, h->X.as<double2>(),
                       h->Fh(), h->mean, h->g_xbs);
  } else if (h->g_long) {
    gen_launch_long<2>(h, s, nb);
  } else {
    gen_launch_axis<2>(h, 1, s, 0, 0, nb);
  }
  gen_launch_p5(h, z, s, nb, bs.out);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

}  // namespace gss
