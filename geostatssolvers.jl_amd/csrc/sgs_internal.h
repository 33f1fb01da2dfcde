// What the SGS translation units share: the handle, and the sizes that the team schedule (sgs_levels.hip) and the team
// kernel (sgs.hip) have to agree on.  sgs_create.hip: stage A; sgs_levels.hip: levels and team schedule; sgs.hip: stage B.
#pragma once

#include "gss_internal.h"

#include <vector>

struct gss_sgs {
  gss::VgDev vg;
  int dim = 0, k = 0;
  int64_t N = 0, nd = 0;
  double mean = 0.0;
  int filter_after = 0;   // GSS_SGS_MASK_AFTER_SEARCH
  int64_t npaths = 1, path_base = 0;  // npaths > 1: one visiting order per realisation, path p <-> realisation path_base + p
  gss::DevBuf path, rank, idx, ncond, w, sigma, dlocs, zd;   // per path: N entries (path, rank, ncond, sigma), N k (idx, w)
  gss::DevBuf field;  // working field of gss_sgs_realize, node-major [N][R] or team layout, kept between calls (grows)
  gss::DevBuf order;  // shared visiting order: nodes sorted by level of the dependency graph
  std::vector<int> lvl_off;   // lvl_off[l] .. lvl_off[l + 1] - 1: positions of level l in `order` (level 0 = conditioning cells)
  // short levels (sgs_level_team_kernel): schedule-ordered padded lists / weights / sigma, chunk boundaries in `order`
  gss::DevBuf nb_sched, w_sched, sg_sched, inv_sched, chunk_off;
  int team_chunks = 0, team_cap = 0, team_rl = 0;
  int big = 0, big_lds = 0;   // stage A ran sgs_weights_big_kernel; with the triangle in LDS (gss_sgs_schedule)
};

namespace gss {

constexpr int SGS_MAX_K = 64;   // neighbours one wave takes: sgs_weights_kernel, the lane-held lists of sgs_sweep_kernel

// sgs_level_team_kernel stages a level in chunks: per chunk at most SGS_TEAM_CAP nodes, SGS_TEAM_ENTRIES list entries
// (cap * padded row) and SGS_TEAM_NORMALS normals (cap * RL)
constexpr int SGS_TEAM_ENTRIES = 2560;
constexpr int SGS_TEAM_NORMALS = 1024;
constexpr int SGS_TEAM_CAP = 128;
// Row lengths of the staged lists (k a multiple of 4): the node slots of a wave read the same column of consecutive rows
// at once, so a row of k doubles (k = 16: 128 bytes) would put all of them into the same LDS banks.  kw = k + 2 doubles
// and kn = 4 mod 8 ints (both whole 16-byte pieces) spread eight consecutive rows over the 32 banks.
inline void sgs_team_strides(int k, int* kn, int* kw) {
  *kw = k + 2;
  *kn = k % 8 == 0 ? k + 4 : k + 8;
}

// levels of every path and, where they are short, the team schedule; h->lvl_off stays empty when switched off or given up
int32_t sgs_build_levels(gss_sgs* h, hipStream_t s);

}  // namespace gss
