// Moving-neighbourhood cokriging (gss.h, gss_cokrig_predict_knn): one search per variable over that variable's samples
// (knn.hip, the unmasked query), then one system per domain point on the lists of all variables
// (cokrig_local_kernel.h).  This unit holds the driver, the general instantiations (any model, 1-D) and what the
// cross-validation driver (cokrig_cv.hip) shares with it; the compile-time kinds of 2-D and 3-D have units of their own
// (cokrig_local_2d.hip, cokrig_local_3d.hip).
#include "cokrig_local_kernel.h"

#include <cstring>

namespace gss {

// idx_out (m x ksum, the caller's rows, -1 beyond a variable's count) and count_out (m x nz) from the lists of the
// searches; one thread per entry of idx_out, the first nz threads of a point write its counts.  qrow: the output row of
// every point (NULL: point p at row p)
__global__ __launch_bounds__(256) void cokrig_lists_kernel(CoLocalSpec sp, const int* __restrict__ idx,
                                                           const int* __restrict__ cnt, const int* __restrict__ row,
                                                           const int* __restrict__ qrow, int64_t m,
                                                           int* __restrict__ idx_out, int* __restrict__ count_out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= m * sp.ksum) return;
  const int64_t p = e / sp.ksum;
  const int col = (int)(e - p * sp.ksum);
  int a = 0, kk = sp.k[0], ko = sp.koff[0], go = sp.off[0];
#pragma unroll
  for (int b = 1; b < COL_MAXZ; ++b) {
    if (b < sp.nz && col >= sp.koff[b]) {
      a = b;
      kk = sp.k[b];
      ko = sp.koff[b];
      go = sp.off[b];
    }
  }
  const int jj = col - ko;
  int c = cnt[(int64_t)a * m + p];
  c = c < 0 ? 0 : (c > kk ? kk : c);
  const int64_t po = qrow ? qrow[p] : p;
  if (idx_out) idx_out[po * sp.ksum + col] = jj < c ? row[go + idx[m * ko + p * kk + jj]] : -1;
  if (count_out && jj == 0) count_out[po * sp.nz + a] = c;
}

int32_t cokrig_lists_dev(const CoLocalSpec& sp, const int* idx, const int* cnt, const int* row, const int* qrow,
                         int64_t m, int* idx_out, int* count_out, hipStream_t s) {
  const int64_t ne = m * sp.ksum;
  hipLaunchKernelGGL(cokrig_lists_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, sp, idx, cnt, row, qrow, m,
                     idx_out, count_out);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

int32_t cokrig_spec(const CoGrouped& g, int variant, const int* k, int minneighbors, CoLocalSpec* out) {
  const int nz = g.nz;
  GSS_REQUIRE(nz >= 1 && nz <= COL_MAXZ, "moving-neighbourhood cokriging: %d variables outside 1 .. %d", nz, COL_MAXZ);
  CoLocalSpec sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.nz = nz;
  sp.ordinary = variant == GSS_KRIG_ORDINARY ? 1 : 0;
  sp.minneighbors = minneighbors;
  for (int a = 0; a < nz; ++a) {
    sp.k[a] = k[a];
    sp.koff[a] = sp.ksum;
    sp.off[a] = (int)g.off[a];
    sp.ksum += k[a];
  }
  GSS_REQUIRE(sp.ksum >= 1 && sp.ksum <= LMAX_K, "moving-neighbourhood cokriging: %d neighbours in total outside 1 .. %d",
              sp.ksum, LMAX_K);
  *out = sp;
  return GSS_OK;
}

CoLocalLaunch cokrig_launch_common(const VgDev& vg, const CoLocalSpec& sp, const CoGrouped& g, const int* idx,
                                   const int* cnt, int64_t mv, hipStream_t s) {
  return CoLocalLaunch{&vg, sp, g.x, g.zres, g.tab, nullptr, mv, idx, cnt, nullptr, nullptr, nullptr, 0, s};
}

int32_t cokrig_local_dev(const VgDev& vg, int variant, int dim, const CoGrouped& g, Searcher* sr, const int* k,
                         int minneighbors, const double* x0, const double* x0_raw, int64_t m, double* mean, double* var,
                         uint8_t* status, int64_t ldo, int* idx_out, int* count_out, hipStream_t s, HostPipe* pipe) {
  const int nz = g.nz;
  CoLocalSpec sp;
  GSS_TRY(cokrig_spec(g, variant, k, minneighbors, &sp));

  const bool piped = pipe && pipe->on;
  const int64_t chunk = cokrig_chunk_cap(piped ? HostPipe::PIECE : (1 << 20));
  const int64_t mc = m < chunk ? m : chunk;
  DevBuf idx_s, cnt_s;
  GSS_TRY(idx_s.alloc(sizeof(int) * (size_t)(mc * sp.ksum)));
  GSS_TRY(cnt_s.alloc(sizeof(int) * (size_t)(mc * nz)));
  const int kind = vg.nextra == 0 ? vg.kind : -1;
  for (int64_t off = 0; off < m; off += chunk) {
    const int64_t mv = (m - off) < chunk ? (m - off) : chunk;
    if (piped) GSS_TRY(pipe->fetch(off, mv, s));
    int* idx = idx_s.as<int>();
    int* cnt = cnt_s.as<int>();
    {
      ProfScope ps("knn", s);
      for (int a = 0; a < nz; ++a)
        GSS_TRY(sr[a].query(x0 + off * dim, x0_raw ? x0_raw + off * dim : nullptr, mv, k[a], idx + mv * sp.koff[a],
                            cnt + (int64_t)a * mv, s));
    }
    {
      ProfScope pl("cokrig_local", s);
      CoLocalLaunch a = cokrig_launch_common(vg, sp, g, idx, cnt, mv, s);
      a.x0 = x0 + off * dim;
      a.mean = mean + off;
      a.var = var + off;
      a.status = status ? status + off : nullptr;
      a.ldo = ldo;
      GSS_TRY(cokrig_local_dispatch<false>(dim, kind, a));
    }
    if (idx_out || count_out) {
      GSS_TRY(cokrig_lists_dev(sp, idx, cnt, g.row, nullptr, mv, idx_out ? idx_out + off * sp.ksum : nullptr,
                               count_out ? count_out + off * nz : nullptr, s));
    }
    if (piped) GSS_TRY(pipe->deliver(off, mv, s));
  }
  if (piped) GSS_TRY(pipe->finish(s));
  GSS_HIP(hipStreamSynchronize(s));   // the lists are released on return
  return GSS_OK;
}

}  // namespace gss
