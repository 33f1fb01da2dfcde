// SGS: the level schedule of the path recursion and, for orders whose levels are short, the team schedule
// (sgs_build_levels, the last step of gss_sgs_create; the sweeps that run on them are in sgs.hip).
#include "sgs_internal.h"

#include <hipcub/hipcub.hpp>

#include <cstdlib>

namespace gss {

// ---- level schedule of the path recursion (shared visiting order) ----------------------------------------------
// z[node] only needs the values of the node's own neighbours, all visited earlier: the recursion is a sparse
// triangular solve, and its dependency graph is shallow -- a node's level is 1 + the highest level among its
// neighbours (conditioning cells: level 0); a random path over 512 x 512 cells with 16 neighbours has about 250
// levels of about 1 000 nodes.  Nodes of one level are independent, so stage B runs level by level with one wave per
// (node, 64 realisations) instead of one wave per 64 realisations walking all N nodes: the same sums in the same
// order (bit-identical fields), N k gathers per realisation spread over the whole device.
__global__ __launch_bounds__(256) void sgs_level_init_kernel(const int* __restrict__ rank, int64_t N /* all paths */,
                                                             int* __restrict__ level, int* __restrict__ node) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < N) {
    level[p] = rank[p] < 0 ? 0 : -1;   // -1: not known yet
    node[p] = (int)p;
  }
}

// Levels in one launch: thread t owns the t-th node of the path and polls its neighbours' levels until all of them
// are known (-1 = not yet), then publishes its own.  A node only waits for nodes visited earlier, i.e. for threads
// of its own or of earlier workgroups, and workgroups start in index order: the earliest unfinished workgroup never
// waits for one that is not resident.  The store sits INSIDE the polling loop -- lanes of one wave wait for each
// other (consecutive nodes of a path are neighbours), and a lane parked behind the loop could not publish.
__global__ __launch_bounds__(256) void sgs_level_chain_kernel(const int64_t* __restrict__ path,
                                                              const int* __restrict__ rank, const int* __restrict__ idx,
                                                              const int* __restrict__ ncond, int k, int64_t N,
                                                              int64_t npaths, int* level, int* __restrict__ gave_up) {
  // Consecutive nodes of an order are neighbours of each other, and a level that a lane of the same wave has just
  // found is taken from its register instead of waiting for it to come back from memory: up to SC of a thread's
  // neighbours (the first ones of its list that lanes of its own wave own -- the list is sorted by distance, so these
  // are the nodes just before it in a row) are followed that way, the others are polled.
  constexpr int SC = 6;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;   // paths one after the other, N nodes each
  const bool inside = g < N * npaths;
  const int64_t gg = inside ? g : N * npaths - 1;
  const int64_t base = gg / N * N;                   // first entry of this thread's path in the per-path arrays
  const int64_t p = base + path[gg];                 // (path, node) as one index
  const bool mine = inside && rank[p] >= 0;          // not a conditioning cell (level 0, sgs_level_init_kernel)
  const int c = mine ? ncond[p] : 0;
  const int* nb = idx + p * k;                       // node numbers within the path
  level += base;
  const int lane = threadIdx.x & 63;
  int so[SC], sj[SC];                                // owner lane and list position of the followed neighbours
  unsigned long long intra = 0;                      // their positions as a mask (all within the first 64)
#pragma unroll
  for (int u = 0; u < SC; ++u) so[u] = sj[u] = -1;
  {
    const int cl = c < 64 ? c : 64;
    int nf = 0;
    for (int j = 0; j < cl && nf < SC; ++j) {
      const int rj = rank[base + nb[j]];
      const int64_t og = base + rj;                  // thread that owns the neighbour: its rank in the order
      if (rj >= 0 && (og >> 6) == (gg >> 6)) {
#pragma unroll
        for (int u = 0; u < SC; ++u)
          if (u == nf) {
            so[u] = (int)(og & 63);
            sj[u] = j;
          }
        intra |= 1ull << j;
        ++nf;
      }
    }
  }
  // neighbours are polled 64 at a time and a neighbour whose level is known is never asked again: with hundreds of
  // thousands of threads in flight, polling everything on every round makes the polls the bottleneck
  // The loop is left by the whole wave at once (__all): a lane that has published must not be parked behind the
  // loop's exit while lanes of its own wave still wait for what it published -- and a store on a path that leaves
  // the loop is, for the compiler, a store after the loop.
  bool done = !mine;
  int mylevel = mine ? -1 : 0;                       // (a conditioning cell's level is 0; lanes outside are never asked)
  int polls = 0, mx = 0, j0 = 0;
  int cc = c < 64 ? c : 64;
  unsigned long long pend = cc == 64 ? ~0ull : ((1ull << cc) - 1ull);
  auto settle = [&]() {   // pend == 0: next 64 neighbours, or publish
    j0 += 64;
    if (j0 >= c) {
      mylevel = mx + 1;
      __hip_atomic_store(&level[p - base], mx + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      done = true;
    } else {
      cc = c - j0 < 64 ? c - j0 : 64;
      pend = cc == 64 ? ~0ull : ((1ull << cc) - 1ull);
    }
  };
  bool news = false;   // a lane of this wave has found its level since the last exchange inside the wave (uniform)
  int idle = 0;        // rounds in a row without any answer (uniform)
  for (;;) {
    // inside the wave: every lane offers its level, every lane takes what its first 64 neighbours in this wave have;
    // repeated while that lets another lane finish (a row of the row-by-row order resolves lane after lane).  Only
    // when there is news: a wave that waits for other waves keeps to its polls.
    for (int sweep = 0; news && sweep < 64; ++sweep) {
      bool fresh = false;
      int lv[SC];
#pragma unroll
      for (int u = 0; u < SC; ++u) lv[u] = __shfl(mylevel, so[u] >= 0 ? so[u] : lane);   // every lane takes part
#pragma unroll
      for (int u = 0; u < SC; ++u) {
        if (!done && so[u] >= 0 && lv[u] >= 0 && ((pend >> sj[u]) & 1ull) && j0 == 0) {
          mx = lv[u] > mx ? lv[u] : mx;
          pend &= ~(1ull << sj[u]);
        }
      }
      if (!done && pend == 0) {
        settle();
        fresh = done;
      }
      if (!__any(fresh)) break;
    }
    news = false;
    const bool was_done = done;
    const unsigned long long pend_before = pend;
    const int j0_before = j0;
    if (!done) {
      // up to eight of the unknown neighbours per round, their loads in flight together: a round is one memory
      // round trip, and a round is what a hop of the chain costs between waves
      // (what a lane of this wave owns arrives through the exchange above and is not asked for in memory: with
      // hundreds of thousands of threads polling, the polls themselves are what the kernel waits for)
      unsigned long long m = j0 == 0 ? pend & ~intra : pend;
      int js[8], ls[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        js[u] = -1;
        ls[u] = -1;
        if (m) {
          js[u] = __builtin_ctzll(m);
          m &= m - 1;
          ls[u] = __hip_atomic_load(&level[nb[j0 + js[u]]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (js[u] >= 0 && ls[u] >= 0) {
          mx = ls[u] > mx ? ls[u] : mx;
          pend &= ~(1ull << js[u]);
        }
      }
      if (pend == 0) {
        settle();
      } else if (++polls > (1 << 18)) {
        // never seen; the wait is bounded all the same: publish, report, and the host drops the schedule
        mylevel = 1 << 29;
        __hip_atomic_store(&level[p - base], 1 << 29, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *gave_up = 1;
        done = true;
      }
    }
    if (__all(done)) break;
    news = __any(done && !was_done);
    // A wave that learns nothing backs off (up to ~16 us between polls): with a quarter of a million threads asking,
    // the polls of the waves far behind the front are what the waves at the front wait for.  Any answer -- one
    // neighbour's level is enough -- brings the wave back to polling at once.
    if (__any(pend != pend_before || j0 != j0_before || done != was_done)) idle = 0;
    else ++idle;
    if (!news) {
      if (idle < 4) {
        __builtin_amdgcn_s_sleep(8);
      } else {
        const int reps = idle - 3 < 4 ? idle - 3 : 4;
        for (int i = 0; i < reps; ++i) __builtin_amdgcn_s_sleep(127);
      }
    }
  }
}

// first position of every level in the level-sorted node list
__global__ __launch_bounds__(256) void sgs_level_offsets_kernel(const int* __restrict__ lvl_sorted, int64_t N,
                                                                int* __restrict__ off) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int l = lvl_sorted[i];
  if (i == 0 || lvl_sorted[i - 1] != l) off[l] = (int)i;
}

// ---- short levels: the whole schedule in one launch (sgs_level_team_kernel) -------------------------------------------
// An order whose levels are short (the row-by-row LinearPath: ~3 100 levels of ~85 nodes on 512 x 512 cells) spends its
// sweep on launches: ~5 us per level whatever the level holds.  Realisations do not depend on each other, so a
// workgroup (a team) takes RL of them through every level by itself and the step from one level to the next is a
// workgroup barrier.  The team path keeps its own layout of everything it touches:
//   field    zq[team][position in the schedule][RL]: a team's part is contiguous, a 128-byte line belongs to ONE
//            team (in the node-major [N][R] field two teams on different XCDs share a line and every gather of a
//            half-written line goes to memory: 2.7 us per level), a level's normals and results are one contiguous run;
//   lists    neighbours as schedule positions, weights, sigma -- in schedule order, entries beyond a node's ncond
//            replaced by (the node itself, weight 0): exact zeros at the end of the same sum, so the values are those of
//            sgs_level_sweep_kernel.
__global__ __launch_bounds__(256) void sgs_team_inverse_kernel(const int* __restrict__ order, int64_t N,
                                                               int* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) inv[order[i]] = (int)i;
}

__global__ __launch_bounds__(256) void sgs_team_lists_kernel(const int* __restrict__ order, const int* __restrict__ inv,
                                                             int64_t N, int k, int kn, int kw,
                                                             const int* __restrict__ ncond,
                                                             const int* __restrict__ idx, const double* __restrict__ w,
                                                             const double* __restrict__ sigma, int* __restrict__ nb_s,
                                                             double* __restrict__ w_s, double* __restrict__ sg_s) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * kn) return;   // kn >= kw: rows of kn ints and kw doubles, padded so that the rows of a wave's node slots
  const int64_t pos = e / kn;   // start in different LDS banks (sgs_team_strides)
  const int j = (int)(e - pos * kn);
  const int64_t node = order[pos];
  const bool kept = j < ncond[node];   // ncond <= k
  nb_s[e] = kept ? inv[idx[node * k + j]] : (int)pos;
  if (j < kw) w_s[pos * kw + j] = kept ? w[node * k + j] : 0.0;
  if (j == 0) sg_s[pos] = sigma[node];
}

// Levels of every (path, node) pair, path-major like the per-path arrays: h->order = the pairs sorted by level,
// h->lvl_off = where each level starts.  Both stay empty when the schedule is switched off (GSS_SGS_LEVELS=0), the
// pairs do not fit an int, or the chain kernel gave up: stage B then walks the path.
static int32_t sgs_levels_and_offsets(gss_sgs* h, hipStream_t s) {
  static const bool enabled = !(std::getenv("GSS_SGS_LEVELS") && std::getenv("GSS_SGS_LEVELS")[0] == '0');
  if (!enabled || h->N * h->npaths >= ((int64_t)1 << 30)) return GSS_OK;
  const int64_t N = h->N * h->npaths;
  DevBuf level, node, lvl_sorted, off, tmp, flag;
  GSS_TRY(level.alloc(sizeof(int) * (size_t)N));
  GSS_TRY(node.alloc(sizeof(int) * (size_t)N));
  GSS_TRY(lvl_sorted.alloc(sizeof(int) * (size_t)N));
  GSS_TRY(h->order.alloc(sizeof(int) * (size_t)N));
  const dim3 grid((unsigned)((N + 255) / 256));
  hipLaunchKernelGGL(sgs_level_init_kernel, grid, dim3(256), 0, s, h->rank.as<int>(), N, level.as<int>(), node.as<int>());
  GSS_HIP(hipGetLastError());
  GSS_TRY(flag.alloc(sizeof(int)));
  GSS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
  hipLaunchKernelGGL(sgs_level_chain_kernel, grid, dim3(256), 0, s, h->path.as<int64_t>(), h->rank.as<int>(),
                     h->idx.as<int>(), h->ncond.as<int>(), h->k, h->N, h->npaths, level.as<int>(), flag.as<int>());
  GSS_HIP(hipGetLastError());
  int gave_up = 0;
  GSS_HIP(hipMemcpyAsync(&gave_up, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  if (gave_up) {
    h->order.release();
    return GSS_OK;
  }
  size_t tb = 0;
  GSS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, level.as<int>(), lvl_sorted.as<int>(), node.as<int>(),
                                             h->order.as<int>(), (int)N, 0, 32, s));
  GSS_TRY(tmp.alloc(tb > 0 ? tb : 16));
  GSS_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, level.as<int>(), lvl_sorted.as<int>(), node.as<int>(),
                                             h->order.as<int>(), (int)N, 0, 32, s));
  int L = 0;
  GSS_HIP(hipMemcpyAsync(&L, lvl_sorted.as<int>() + (N - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  GSS_TRY(off.alloc(sizeof(int) * (size_t)(L + 2)));
  GSS_HIP(hipMemsetAsync(off.p, 0xff, sizeof(int) * (size_t)(L + 2), s));
  hipLaunchKernelGGL(sgs_level_offsets_kernel, grid, dim3(256), 0, s, lvl_sorted.as<int>(), N, off.as<int>());
  GSS_HIP(hipGetLastError());
  std::vector<int> ho((size_t)L + 2);
  GSS_HIP(hipMemcpyAsync(ho.data(), off.p, sizeof(int) * (size_t)(L + 2), hipMemcpyDeviceToHost, s));
  GSS_HIP(hipStreamSynchronize(s));
  ho[(size_t)L + 1] = (int)N;
  for (int l = L; l >= 0; --l)   // a level without nodes (only level 0 can be: no conditioning cells) starts where the next does
    if (ho[(size_t)l] < 0) ho[(size_t)l] = ho[(size_t)l + 1];
  h->lvl_off = std::move(ho);
  return GSS_OK;
}

// Orders with short levels sweep in one launch (sgs_level_team_kernel).  The average level size decides: a launch per
// level costs ~5 us whatever it holds, a team's level ~2.8 us up to 112 nodes (measured).  Where it
// applies: chunk boundaries, the inverse of the order and the padded lists; h->team_chunks stays 0 where it does not.
static int32_t sgs_team_schedule(gss_sgs* h, hipStream_t s) {
  const int64_t N = h->N * h->npaths;
  const int L = (int)h->lvl_off.size() - 2;
  static const char* team_env = std::getenv("GSS_SGS_TEAM");   // "0": never, "1": whenever it applies (measurements)
  const int64_t nsim = N - h->lvl_off[1];
  const double avg = L > 0 ? (double)nsim / (double)L : 0.0;
  const bool want = team_env ? team_env[0] != '0' : avg <= 128.0;
  // (any maxneighbors up to 64 -- the reference's default is 10 --: the staged rows are padded to a multiple of four,
  //  the padding adds exact zeros like the entries beyond a node's ncond)
  if (!(h->npaths == 1 && h->k <= 64 && L > 0 && want)) return GSS_OK;
  h->team_rl = avg <= 14.0 ? 64 : avg <= 28.0 ? 32 : avg <= 56.0 ? 16 : 8;   // one round (896 / RL nodes) per level where possible
  int kn = 0, kw = 0;
  sgs_team_strides((h->k + 3) & ~3, &kn, &kw);
  int cap = SGS_TEAM_ENTRIES / kn < SGS_TEAM_CAP ? SGS_TEAM_ENTRIES / kn : SGS_TEAM_CAP;
  if (cap > SGS_TEAM_NORMALS / h->team_rl) cap = SGS_TEAM_NORMALS / h->team_rl;
  std::vector<int> co;
  for (int l = 1; l <= L; ++l)
    for (int a = h->lvl_off[(size_t)l]; a < h->lvl_off[(size_t)l + 1]; a += cap) co.push_back(a);
  co.push_back((int)N);
  GSS_TRY(h->chunk_off.alloc(sizeof(int) * co.size()));
  GSS_HIP(hipMemcpyAsync(h->chunk_off.p, co.data(), sizeof(int) * co.size(), hipMemcpyHostToDevice, s));
  GSS_TRY(h->nb_sched.alloc(sizeof(int) * (size_t)(N * kn)));
  GSS_TRY(h->w_sched.alloc(sizeof(double) * (size_t)(N * kw)));
  GSS_TRY(h->sg_sched.alloc(sizeof(double) * (size_t)N));
  GSS_TRY(h->inv_sched.alloc(sizeof(int) * (size_t)N));
  hipLaunchKernelGGL(sgs_team_inverse_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, h->order.as<int>(), N,
                     h->inv_sched.as<int>());
  hipLaunchKernelGGL(sgs_team_lists_kernel, dim3((unsigned)((N * kn + 255) / 256)), dim3(256), 0, s,
                     h->order.as<int>(), h->inv_sched.as<int>(), N, h->k, kn, kw, h->ncond.as<int>(), h->idx.as<int>(),
                     h->w.as<double>(), h->sigma.as<double>(), h->nb_sched.as<int>(), h->w_sched.as<double>(),
                     h->sg_sched.as<double>());
  GSS_HIP(hipGetLastError());
  GSS_HIP(hipStreamSynchronize(s));   // co is a local
  h->team_chunks = (int)co.size() - 1;
  h->team_cap = cap;
  return GSS_OK;
}

int32_t sgs_build_levels(gss_sgs* h, hipStream_t s) {
  h->lvl_off.clear();
  h->team_chunks = 0;
  GSS_TRY(sgs_levels_and_offsets(h, s));
  if (!h->lvl_off.empty()) GSS_TRY(sgs_team_schedule(h, s));
  return GSS_OK;
}

}  // namespace gss
