// Cross-validation of a cokriging handle under a moving neighbourhood (gss.h, gss_cokrig_cv_knn): the queries are the
// handle's own samples in grouped order, so a query's variable follows from its position; one fold search per variable
// over that variable's samples (knn.hip, KnnMask::Fold with separate sample and query ids), then one system per query
// for its one target (cokrig_local_kernel.h, cokrig_cv_kernel).  This unit holds the driver and the general
// instantiations (any model, 1-D); the compile-time kinds of 2-D and 3-D are in cokrig_local_2d.hip / _3d.hip.
#include "cokrig_local_kernel.h"

namespace gss {

// fold ids in grouped order: the caller's id of the sample's row, or the row itself (every sample its own fold)
__global__ __launch_bounds__(256) void cokrig_cv_fold_kernel(const int* __restrict__ fold, const int* __restrict__ row,
                                                             int64_t n, int* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int r = row[j];
  out[j] = fold ? fold[r] : r;
}

int32_t cokrig_cv_dev(const VgDev& vg, int variant, int dim, const CoGrouped& g, Searcher* sr, const int* k,
                      int minneighbors, const int* fold, double ex, double* pred, double* var, uint8_t* status,
                      int* idx_out, int* count_out, hipStream_t s) {
  const int nz = g.nz;
  CoLocalSpec sp;
  GSS_TRY(cokrig_spec(g, variant, k, minneighbors, &sp));
  const int64_t n = g.off[nz];
  if (n <= 0) return GSS_OK;

  const int64_t chunk = cokrig_chunk_cap(1 << 20);
  const int64_t mc = n < chunk ? n : chunk;
  DevBuf idx_s, cnt_s, fold_s;
  GSS_TRY(idx_s.alloc(sizeof(int) * (size_t)(mc * sp.ksum)));
  GSS_TRY(cnt_s.alloc(sizeof(int) * (size_t)(mc * nz)));
  GSS_TRY(fold_s.alloc(sizeof(int) * (size_t)n));
  int* foldg = fold_s.as<int>();
  hipLaunchKernelGGL(cokrig_cv_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fold, g.row, n, foldg);
  GSS_HIP(hipGetLastError());
  // the raw coordinates a search in a second frame reads: x_raw only exists beside a rotated structure
  const double* xq_raw = g.x_raw ? g.x_raw : g.x;
  const int kind = vg.nextra == 0 ? vg.kind : -1;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t mv = (n - off) < chunk ? (n - off) : chunk;
    int* idx = idx_s.as<int>();
    int* cnt = cnt_s.as<int>();
    {
      ProfScope ps("knn", s);
      for (int a = 0; a < nz; ++a) {
        // samples: the ids of group a; queries: the ids of this chunk (not the qoff shortcut: the queries are all the
        // grouped samples, the samples of a search one group of them)
        const KnnMask mask = KnnMask(KnnMask::Fold{foldg + g.off[a], foldg, 0, ex}).from(off);
        GSS_TRY(sr[a].query(g.x + off * dim, sr[a].two_frames ? xq_raw + off * dim : nullptr, mv, k[a],
                            idx + mv * sp.koff[a], cnt + (int64_t)a * mv, s, &mask));
      }
    }
    {
      ProfScope pl("cokrig_cv", s);
      CoLocalLaunch a = cokrig_launch_common(vg, sp, g, idx, cnt, mv, s);
      a.mean = pred;
      a.var = var;
      a.status = status;
      a.row = g.row;
      a.q0 = off;
      GSS_TRY(cokrig_local_dispatch<true>(dim, kind, a));
    }
    if (idx_out || count_out) GSS_TRY(cokrig_lists_dev(sp, idx, cnt, g.row, g.row + off, mv, idx_out, count_out, s));
  }
  GSS_HIP(hipStreamSynchronize(s));   // the lists and the gathered ids are released on return
  return GSS_OK;
}

}  // namespace gss
