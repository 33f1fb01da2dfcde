// SGS: sequential Gaussian simulation.
// Replaces SGS.preprocess (/root/reference/src/simulation/sgs.jl:56-85) and the SeqSim path loop
// (/root/reference/src/simulation/seq.jl:76-141) for the estimator/marginal pair SGS always builds
// (SimpleKriging(variogram, mean), Normal(mean, sqrt(sill)), sgs.jl:62-67).
//
// The reference walks the path once per realisation and, at every node, searches the already simulated
// cells (seq.jl:105), fits a simple-kriging system (seq.jl:121) and draws from Normal(mu, sigma) (seq.jl:129).
// Which cells are "already simulated" depends on the path and on the data cells only, never on the drawn
// values, and simple-kriging weights do not depend on the values either.  So the device splits the work:
//
//   stage A (gss_sgs_create, sgs_create.hip; data parallel over the N nodes, done once for every realisation):
//     neighbours, simple-kriging weights and sigma of every node; then the level schedule (sgs_levels.hip)
//   stage B (gss_sgs_realize, this file; parallel over realisations, sequential along the path):
//     z[node] = mean + sum_j lambda_j (z[nb_j] - mean) + sigma * eps(seed, realisation, node)
#include "sgs_internal.h"
#include "philox.h"

#include <climits>

namespace gss {

// The recursion step of the sweeps that read their lists from memory: acc = sum_j w_j (z[nb_j * stride + r] - mean) over
// a node's c neighbours, the terms added in list order, G gathers in flight.
template <int G>
__device__ __forceinline__ double sgs_step(const int* __restrict__ nb, const double* __restrict__ ww, int c,
                                           const double* z, int64_t stride, int64_t r, double mean) {
  double acc = 0.0;
  int j = 0;
  for (; j + G <= c; j += G) {
    double zz[G];
#pragma unroll
    for (int u = 0; u < G; ++u) zz[u] = z[(int64_t)nb[j + u] * stride + r];
#pragma unroll
    for (int u = 0; u < G; ++u) acc = fma(ww[j + u], zz[u] - mean, acc);
  }
  for (; j < c; ++j) acc = fma(ww[j], z[(int64_t)nb[j] * stride + r] - mean, acc);
  return acc;
}

// the same walk for more than 64 neighbours: the recursion without the lane-held lists
__global__ __launch_bounds__(64) void sgs_sweep_big_kernel(
    const int64_t* __restrict__ path, const int* __restrict__ rank, const int* __restrict__ idx,
    const int* __restrict__ ncond, const double* __restrict__ w, const double* __restrict__ sigma, int k, int64_t N, int R,
    double mean, double* __restrict__ zt) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  const bool live = r < R;
  const int rr = live ? r : R - 1;
  for (int64_t t = 0; t < N; ++t) {
    const int64_t node = path[t];
    if (rank[node] < 0) continue;  // conditioning cell
    const double acc = sgs_step<4>(idx + node * k, w + node * k, ncond[node], zt, R, rr, mean);
    const double v = mean + acc + sigma[node] * zt[node * R + rr];
    if (live) zt[node * R + r] = v;
  }
}

// one level of the dependency graph (sgs_levels.hip): wave = (node of the level, block of 64 realisations)
__global__ __launch_bounds__(256) void sgs_level_sweep_kernel(
    const int* __restrict__ order, int first, int count, const int* __restrict__ idx, const int* __restrict__ ncond,
    const double* __restrict__ w, const double* __restrict__ sigma, int k, int R, int rb, double mean,
    double* __restrict__ zt) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (int64_t)count * rb) return;   // whole wave
  const int64_t node = order[first + (int)(item / rb)];
  const int r = (int)(item % rb) * 64 + lane;
  const bool live = r < R;
  const int rr = live ? r : R - 1;
  const double eps = zt[node * R + rr];   // the cell's own slot holds its normal until it is simulated
  const double acc = sgs_step<8>(idx + node * k, w + node * k, ncond[node], zt, R, rr, mean);
  const double v = mean + acc + sigma[node] * eps;
  if (live) zt[node * R + r] = v;
}

// out[r][cell] from the team layout through an LDS tile: 64 cells of one team; RL * 8 bytes per cell come in, 512-byte
// runs go out
__global__ __launch_bounds__(256) void sgs_team_out_kernel(const double* __restrict__ zq, const int* __restrict__ inv,
                                                           int64_t N, int R, int RL, double* __restrict__ out) {
  __shared__ double tile[64][65];
  const int64_t c0 = (int64_t)blockIdx.x * 64;
  const int team = blockIdx.y;
  for (int e = threadIdx.x; e < 64 * RL; e += 256) {
    const int i = e / RL, rl = e % RL;
    if (c0 + i < N) tile[rl][i] = zq[((int64_t)team * N + inv[c0 + i]) * RL + rl];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * RL; e += 256) {
    const int rl = e >> 6, i = e & 63;
    const int r = team * RL + rl;
    if (c0 + i < N && r < R) out[(int64_t)r * N + c0 + i] = tile[rl][i];
  }
}

// ---- short levels: the whole schedule in one launch (schedule and layout: sgs_levels.hip) -----------------------------
// Fourteen waves compute: lane = (node slot, realisation), 896 / RL nodes per round, every gather of a node in flight
// at once.  Two waves stage: what a level needs besides its neighbours' values -- lists, weights, sigma, the level's
// normals -- does not depend on the sweep and is copied into LDS three chunks ahead with LDS-direct loads (no registers,
// so the copies stay in flight across the barriers: the staging waves wait with a COUNTED vmcnt, the barrier is the raw
// instruction; a wave's ordinary loads return in order, which is why the computing waves do not fetch any of this
// themselves).  Levels are cut into chunks of at most `cap` nodes (chunk_off); all LDS is one array.
constexpr int SGS_TEAM_THREADS = 1024;
constexpr int SGS_TEAM_STAGERS = 2;            // staging waves
constexpr int SGS_TEAM_AHEAD = 3;              // chunks in flight; LDS holds one stage more
constexpr int SGS_TEAM_STAGES = SGS_TEAM_AHEAD + 1;
struct SgsTeamStage {
  double ww[SGS_TEAM_ENTRIES];
  double eps[SGS_TEAM_NORMALS];
  double sg[SGS_TEAM_CAP];
  int nb[SGS_TEAM_ENTRIES];
};
static_assert(SGS_TEAM_STAGES * sizeof(SgsTeamStage) <= 160 * 1024, "LDS of a CU");
// LDS-direct copies issued per staging wave and chunk; the staging waves' vmcnt leaves AHEAD - 1 chunks in flight
constexpr int SGS_TEAM_GLDS = (SGS_TEAM_ENTRIES * 4 + SGS_TEAM_ENTRIES * 8 + SGS_TEAM_NORMALS * 8) / 1024 / SGS_TEAM_STAGERS +
                              SGS_TEAM_CAP * 8 / 256 / SGS_TEAM_STAGERS;
static_assert(SGS_TEAM_GLDS == 21 && SGS_TEAM_AHEAD == 3, "the waits below are written for 21 copies and 3 chunks: vmcnt(42), (21)");
static_assert(SGS_TEAM_GLDS * SGS_TEAM_AHEAD <= 63, "vmcnt counts to 63");

// `bytes` valid bytes from src to dst (LDS), the staging waves together: pieces of 64 lanes x SIZE bytes, a piece per
// instruction, lanes beyond the end repeat the last SIZE bytes (every instruction is issued: the vmcnt count is fixed)
template <int SIZE, int PIECES>
__device__ __forceinline__ void sgs_team_copy(void* dst, const void* src, int bytes, int sw, int lane) {
  static_assert(PIECES % SGS_TEAM_STAGERS == 0 && (SIZE == 16 || SIZE == 4), "pieces divide among the staging waves");
#pragma unroll
  for (int u = 0; u < PIECES / SGS_TEAM_STAGERS; ++u) {
    const int piece = u * SGS_TEAM_STAGERS + sw;
    const int off = piece * 64 * SIZE + lane * SIZE;
    const char* g = static_cast<const char*>(src) + (off < bytes ? off : bytes - SIZE);
    auto gp = (const __attribute__((address_space(1))) void*)g;
    auto lp = (__attribute__((address_space(3))) void*)(static_cast<char*>(dst) + piece * 64 * SIZE);
    if constexpr (SIZE == 16)   // the builtin wants a literal
      __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds(gp, lp, 4, 0, 0);
  }
}

template <int RL>
__global__ __launch_bounds__(SGS_TEAM_THREADS) void sgs_level_team_kernel(
    const int* __restrict__ nb_s, const double* __restrict__ w_s, const double* __restrict__ sg_s,
    const int* __restrict__ chunk_off, int nchunks, int k, int kn, int kw, int64_t N, double mean,
    double* __restrict__ zq) {
  extern __shared__ __attribute__((aligned(16))) unsigned char team_lds[];
  SgsTeamStage* stages = reinterpret_cast<SgsTeamStage*>(team_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int CW = SGS_TEAM_THREADS / 64 - SGS_TEAM_STAGERS;   // computing waves
  constexpr int NPW = 64 / RL, NPR = CW * NPW;
  const int q = lane / RL, rl = lane % RL;
  double* zb = zq + (int64_t)blockIdx.x * N * RL;   // this team's realisations, [position][RL]
  const int sw = __builtin_amdgcn_readfirstlane(wave) - CW;   // >= 0: staging wave

  auto issue = [&](int c) {
    SgsTeamStage& S = stages[c % SGS_TEAM_STAGES];
    const int first = chunk_off[c], cnt = chunk_off[c + 1] - first;
    sgs_team_copy<16, SGS_TEAM_ENTRIES * 4 / 1024>(S.nb, nb_s + (int64_t)first * kn, cnt * kn * 4, sw, lane);
    sgs_team_copy<16, SGS_TEAM_ENTRIES * 8 / 1024>(S.ww, w_s + (int64_t)first * kw, cnt * kw * 8, sw, lane);
    sgs_team_copy<16, SGS_TEAM_NORMALS * 8 / 1024>(S.eps, zb + (int64_t)first * RL, cnt * RL * 8, sw, lane);
    sgs_team_copy<4, SGS_TEAM_CAP * 8 / 256>(S.sg, sg_s + first, cnt * 8, sw, lane);
  };
  // all but the newest `left` chunks' copies have landed (left = chunks issued after the one that is needed)
  auto landed = [&](int left) {
    if (left >= 2) asm volatile("s_waitcnt vmcnt(42)" ::: "memory");
    else if (left == 1) asm volatile("s_waitcnt vmcnt(21)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  if (sw >= 0) {
    const int pre = nchunks < SGS_TEAM_AHEAD ? nchunks : SGS_TEAM_AHEAD;
    for (int c = 0; c < pre; ++c) issue(c);
    landed(pre - 1);   // chunk 0
  }
  int first = chunk_off[0], end = chunk_off[1];
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  for (int c = 0; c < nchunks; ++c) {
    const int end_next = chunk_off[c + 2 <= nchunks ? c + 2 : nchunks];   // boundaries one chunk ahead: off the chain
    if (sw >= 0) {
      // stage (c + AHEAD) % STAGES held chunk c - 1, and the barrier behind that chunk has been passed
      if (c + SGS_TEAM_AHEAD < nchunks) issue(c + SGS_TEAM_AHEAD);
      const int issued = c + SGS_TEAM_AHEAD < nchunks ? c + SGS_TEAM_AHEAD : nchunks - 1;   // newest chunk on its way
      landed(issued - (c + 1) > 0 ? issued - (c + 1) : 0);                                   // chunk c + 1 has landed
    } else {
      const SgsTeamStage& S = stages[c % SGS_TEAM_STAGES];
      const int cnt = end - first;
      for (int base = 0; base < cnt; base += NPR) {
        const int i = base + wave * NPW + q;
        const bool on = i < cnt;
        const int ii = on ? i : 0;
        const double sg = S.sg[ii];
        const double eps = S.eps[ii * RL + rl];   // the cell's own slot held its normal
        double acc = 0.0;
        const int* nbr = S.nb + ii * kn;
        const double* wwr = S.ww + ii * kw;
        auto batch = [&](int j, auto count) {     // `count` gathers in flight, then their terms in list order
          constexpr int C = decltype(count)::value;
          double zz[C];
#pragma unroll
          for (int u = 0; u < C; ++u) zz[u] = zb[(int64_t)nbr[j + u] * RL + rl];
#pragma unroll
          for (int u = 0; u < C; ++u) acc = fma(wwr[j + u], zz[u] - mean, acc);
        };
        int j = 0;
        for (; j + 16 <= k; j += 16) batch(j, std::integral_constant<int, 16>{});
        switch (k - j) {                          // k is a multiple of 4
          case 12: batch(j, std::integral_constant<int, 12>{}); break;
          case 8: batch(j, std::integral_constant<int, 8>{}); break;
          case 4: batch(j, std::integral_constant<int, 4>{}); break;
          default: break;
        }
        if (on) zb[(int64_t)(first + i) * RL + rl] = mean + acc + sg * eps;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the level's results have left before a wave of this CU gathers them
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    first = end;
    end = end_next;
  }
}

// one level of every visiting order at once: thread = (path, node) of the level
__global__ __launch_bounds__(256) void sgs_level_sweep_paths_kernel(
    const int* __restrict__ order, int first, int count, const int* __restrict__ idx, const int* __restrict__ ncond,
    const double* __restrict__ w, const double* __restrict__ sigma, int k, int64_t N, int R, int64_t path0, double mean,
    double* __restrict__ zr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int64_t g = order[first + i];
  const int64_t pi = g / N, node = g - pi * N;
  const int64_t r = pi - path0;              // realisation r of this call walks path path0 + r
  if (r < 0 || r >= R) return;
  double* z = zr + r * N;
  const double acc = sgs_step<4>(idx + g * k, w + g * k, ncond[g], z, 1, 0, mean);
  z[node] = mean + acc + sigma[g] * z[node];  // the cell's own slot holds its normal until it is simulated
}

// Field layouts.  `decode`: linear element index -> (cell, realisation) in the layout's contiguous order (padding: a
// realisation beyond R); `at`: the address of (cell, realisation).  sgs_split takes element e of n items x R realisations apart along
// the layout's fastest axis (FAST_R: the realisation); the conditioning values use it too, which only keeps their stores
// in the order they always had (any split writes the same bytes).
template <bool FAST_R>
__device__ __forceinline__ void sgs_split(int64_t e, int64_t n, int R, int64_t* i, int* r) {
  const int64_t q = FAST_R ? e / R : e / n;
  *i = FAST_R ? q : e - q * n;
  *r = (int)(FAST_R ? e - q * R : q);
}

struct SgsNodeMajor {   // zt[cell][r]: a shared visiting order, one lane per realisation, the gathers coalesce
  static constexpr bool FAST_R = true;
  int64_t N;
  int R;
  __device__ int64_t size() const { return N * R; }
  __device__ void decode(int64_t e, int64_t* cell, int* r) const { sgs_split<true>(e, N, R, cell, r); }
  __device__ int64_t at(int64_t cell, int r) const { return cell * R + r; }
};

struct SgsRealMajor {   // zr[r][cell] (= the output layout): one visiting order per realisation, nothing shared between lanes
  static constexpr bool FAST_R = false;
  int64_t N;
  int R;
  __device__ int64_t size() const { return N * R; }
  __device__ void decode(int64_t e, int64_t* cell, int* r) const { sgs_split<false>(e, N, R, cell, r); }
  __device__ int64_t at(int64_t cell, int r) const { return (int64_t)r * N + cell; }
};

// zq[team][position in the schedule][RL]: a team's part is contiguous, a 128-byte line belongs to ONE team, a level's
// normals and results are one contiguous run (sgs_levels.hip); the last team is padded to RL realisations
struct SgsTeamLayout {
  static constexpr bool FAST_R = true;
  int64_t N;
  int R, RL, nteams;
  const int* __restrict__ order;   // cell at a position of the schedule
  const int* __restrict__ inv;     // position of a cell
  __device__ int64_t size() const { return (int64_t)nteams * N * RL; }
  __device__ void decode(int64_t e, int64_t* cell, int* r) const {
    *r = (int)(e / ((int64_t)RL * N)) * RL + (int)(e % RL);
    *cell = order[(e / RL) % N];
  }
  __device__ int64_t at(int64_t cell, int r) const { return ((int64_t)(r / RL) * N + inv[cell]) * RL + r % RL; }
};

// z(dloc, r) = zdata for the conditioning cells
template <class Layout>
__global__ __launch_bounds__(256) void sgs_seed_data_kernel(Layout lay, const int64_t* __restrict__ dlocs,
                                                            const double* __restrict__ zd, int64_t nd,
                                                            double* __restrict__ z) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nd * lay.R) return;
  int64_t j;
  int r;
  sgs_split<Layout::FAST_R>(e, nd, lay.R, &j, &r);
  z[lay.at(dlocs[j], r)] = zd[j];
}

// z(cell, r) = eps(seed, realisation, cell): the standard normals the sweep consumes, drawn up front by the whole
// device (a single wave walking the path would otherwise spend half of every step inside Philox + Box-Muller); element
// e of the layout is written by thread e, padding gets zeros.  noise: supplied normals, [R][N].
template <class Layout>
__global__ __launch_bounds__(256) void sgs_noise_kernel(Layout lay, uint64_t seed, int64_t first_real,
                                                        const double* __restrict__ noise, double* __restrict__ z) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= lay.size()) return;
  int64_t cell;
  int r;
  lay.decode(e, &cell, &r);
  z[e] = r < lay.R ? (noise ? noise[(int64_t)r * lay.N + cell] : philox_normal(seed, (uint32_t)(first_real + r), (uint64_t)cell))
               : 0.0;
}

// out[r][cell] = zt[cell][r] through a 64 x 64 LDS tile (both sides coalesced)
__global__ __launch_bounds__(256) void sgs_transpose_kernel(const double* __restrict__ zt, int64_t N, int R,
                                                            double* __restrict__ out) {
  __shared__ double tile[64][65];
  const int64_t c0 = (int64_t)blockIdx.x * 64;
  const int r0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int64_t c = c0 + i;
    const int r = r0 + tx;
    if (c < N && r < R) tile[i][tx] = zt[c * R + r];
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i;
    const int64_t c = c0 + tx;
    if (c < N && r < R) out[(int64_t)r * N + c] = tile[tx][i];
  }
}

// stage B: the path recursion, one lane per realisation (all lanes visit the same node, so the neighbour list
// and the weights are wave-uniform loads and the field gathers are contiguous across lanes)
__global__ __launch_bounds__(64) void sgs_sweep_kernel(const int64_t* __restrict__ path, const int* __restrict__ rank,
                                                       const int* __restrict__ idx, const int* __restrict__ ncond,
                                                       const double* __restrict__ w, const double* __restrict__ sigma,
                                                       int k, int64_t N, int R, double mean,
                                                       double* __restrict__ zt) {
  const int lane = threadIdx.x;
  const int r = blockIdx.x * 64 + lane;
  const bool live = r < R;
  const int rr = live ? r : R - 1;  // idle lanes shadow the last realisation (no stores): the wave stays uniform
  // Everything that does not depend on simulated values is fetched one node ahead (two for the path itself):
  // lane u holds neighbour u's index and weight of the NEXT node, read back with readlane when it is consumed.
  int64_t node_n = path[0];
  int64_t node_nn = N > 1 ? path[1] : 0;
  int pc = ncond[node_n], prank = rank[node_n];
  double psg = sigma[node_n];
  int pidx = lane < k ? idx[node_n * k + lane] : 0;
  double pw = lane < k ? w[node_n * k + lane] : 0.0;
  double peps = zt[node_n * R + rr];  // the cell's own slot holds its normal until it is simulated
  for (int64_t t = 0; t < N; ++t) {
    const int64_t node = node_n;
    const int c = pc, rk = prank, myidx = pidx;
    const double sg = psg, myw = pw, eps = peps;
    if (t + 1 < N) {
      node_n = node_nn;
      node_nn = t + 2 < N ? path[t + 2] : 0;
      pc = ncond[node_n];
      prank = rank[node_n];
      psg = sigma[node_n];
      pidx = lane < k ? idx[node_n * k + lane] : 0;
      pw = lane < k ? w[node_n * k + lane] : 0.0;
      peps = zt[node_n * R + rr];
    }
    if (rk < 0) continue;  // conditioning cell
    double acc = 0.0;
    // sixteen neighbours per trip, all gathers of a trip in flight together: a node costs about one memory round trip
    for (int j0 = 0; j0 < c; j0 += 16) {
      double ww[16], zz[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int j = j0 + u < c ? j0 + u : c - 1;
        const int id = __builtin_amdgcn_readlane(myidx, j);
        const int wl = __builtin_amdgcn_readlane(__double2loint(myw), j);
        const int wh = __builtin_amdgcn_readlane(__double2hiint(myw), j);
        ww[u] = j0 + u < c ? __hiloint2double(wh, wl) : 0.0;
        zz[u] = zt[(int64_t)id * R + rr];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) acc = fma(ww[u], zz[u] - mean, acc);
    }
    const double v = mean + acc + sg * eps;
    if (live) zt[node * R + r] = v;
  }
}

// ---- one visiting order per realisation (seq.jl:99-102 calls traverse inside solvesingle: a RandomPath differs
//      from realisation to realisation).  Stage A runs once per path; the sweep gives every realisation a lane of its
//      own on the realisation-major field: every access is a per-lane gather.
__global__ __launch_bounds__(64) void sgs_sweep_paths_kernel(
    const int64_t* __restrict__ paths, const int* __restrict__ ranks, const int* __restrict__ idx,
    const int* __restrict__ ncond, const double* __restrict__ w, const double* __restrict__ sigma, int k, int64_t N, int R,
    int64_t path0, double mean, double* __restrict__ zr) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int64_t pi = path0 + r;                 // realisation r of this call walks path path0 + r
  const int64_t* path = paths + pi * N;
  const int* rank = ranks + pi * N;
  const int* nbr = idx + pi * N * k;
  const int* nc = ncond + pi * N;
  const double* wt = w + pi * N * k;
  const double* sg = sigma + pi * N;
  double* z = zr + (int64_t)r * N;
  int64_t node_n = path[0];
  for (int64_t t = 0; t < N; ++t) {
    const int64_t node = node_n;
    if (t + 1 < N) node_n = path[t + 1];        // next node's address is known a step ahead
    if (rank[node] < 0) continue;               // conditioning cell
    const double acc = sgs_step<4>(nbr + node * k, wt + node * k, nc[node], z, 1, 0, mean);
    z[node] = mean + acc + sg[node] * z[node];  // the cell's own slot holds its normal until it is simulated
  }
}

// the team kernel for RL realisations per team; its LDS attribute once per device
template <int RL>
static int32_t sgs_team_launch(const gss_sgs* h, int nteams, double* zq, hipStream_t s) {
  static uint64_t attr_set = 0;
  if (first_on_this_device(attr_set)) {
    GSS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sgs_level_team_kernel<RL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(SGS_TEAM_STAGES * sizeof(SgsTeamStage))));
  }
  int kn = 0, kw = 0;
  const int kp = (h->k + 3) & ~3;   // list length the kernel walks: the rows are padded beyond it
  sgs_team_strides(kp, &kn, &kw);
  hipLaunchKernelGGL((sgs_level_team_kernel<RL>), dim3((unsigned)nteams), dim3(SGS_TEAM_THREADS),
                     SGS_TEAM_STAGES * sizeof(SgsTeamStage), s, h->nb_sched.as<int>(), h->w_sched.as<double>(),
                     h->sg_sched.as<double>(), h->chunk_off.as<int>(), h->team_chunks, kp, kn, kw, h->N, h->mean, zq);
  return GSS_OK;
}

// the first two steps of the pipeline on any layout
template <class Layout>
static int32_t sgs_fill_field(const gss_sgs* h, const Layout& lay, size_t elements, uint64_t seed, int64_t first_real,
                              const double* noise, double* z, hipStream_t s) {
  {
    ProfScope ps("sgs_noise", s);
    hipLaunchKernelGGL((sgs_noise_kernel<Layout>), dim3((unsigned)((elements + 255) / 256)), dim3(256), 0, s, lay, seed,
                       first_real, noise, z);
    GSS_HIP(hipGetLastError());
  }
  if (h->nd > 0) {
    hipLaunchKernelGGL((sgs_seed_data_kernel<Layout>), dim3((unsigned)((h->nd * lay.R + 255) / 256)), dim3(256), 0, s, lay,
                       h->dlocs.as<int64_t>(), h->zd.as<double>(), h->nd, z);
    GSS_HIP(hipGetLastError());
  }
  return GSS_OK;
}

// Realisations first_real .. first_real + nreals - 1 (a range gss_sgs_realize has checked) with every array in HBM,
// asynchronous on s: fill normals, seed data, sweep, copy out.
static int32_t sgs_realize_block(gss_sgs_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                                 double* out, hipStream_t s) {
  const int64_t N = h->N;
  const int R = (int)nreals;
  // layout and sweep: one order per realisation works in the output itself; a shared order on the team layout where the
  // schedule has one, else node-major; level by level where there are levels, else along the path
  const bool per_order = h->npaths > 1, levels = !h->lvl_off.empty(), team = !per_order && levels && h->team_chunks > 0;
  const int RL = team ? h->team_rl : 1;
  const int nteams = (R + RL - 1) / RL;
  const size_t elements = (size_t)nteams * (size_t)N * (size_t)RL;   // (N R but for the team's padding)
  double* z = out;
  if (!per_order) {
    // the working field is GBs (8 N R bytes): allocating and freeing it on every call costs more than a short sweep
    if (h->field.bytes < sizeof(double) * elements) {
      h->field.release();
      GSS_TRY(h->field.alloc(sizeof(double) * elements));
    }
    z = h->field.as<double>();
  }
  if (per_order)
    GSS_TRY(sgs_fill_field(h, SgsRealMajor{N, R}, elements, seed, first_real, noise, z, s));
  else if (team)
    GSS_TRY(sgs_fill_field(h, SgsTeamLayout{N, R, RL, nteams, h->order.as<int>(), h->inv_sched.as<int>()}, elements, seed,
                           first_real, noise, z, s));
  else
    GSS_TRY(sgs_fill_field(h, SgsNodeMajor{N, R}, elements, seed, first_real, noise, z, s));
  {
    ProfScope ps("sgs_sweep", s);
    const int* idx = h->idx.as<int>();
    const int* nc = h->ncond.as<int>();
    const double* w = h->w.as<double>();
    const double* sg = h->sigma.as<double>();
    const dim3 walkers((unsigned)((R + 63) / 64));   // a lane per realisation walks the path
    if (team) {
      switch (RL) {
        case 64: GSS_TRY(sgs_team_launch<64>(h, nteams, z, s)); break;
        case 32: GSS_TRY(sgs_team_launch<32>(h, nteams, z, s)); break;
        case 16: GSS_TRY(sgs_team_launch<16>(h, nteams, z, s)); break;
        default: GSS_TRY(sgs_team_launch<8>(h, nteams, z, s)); break;
      }
    } else if (levels) {   // a launch per level; with one order per realisation every order's level at once
      const int L = (int)h->lvl_off.size() - 2;
      const int rb = (R + 63) / 64;
      for (int l = 1; l <= L; ++l) {
        const int first = h->lvl_off[(size_t)l], count = h->lvl_off[(size_t)l + 1] - first;
        if (count <= 0) continue;
        if (per_order)
          hipLaunchKernelGGL(sgs_level_sweep_paths_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s,
                             h->order.as<int>(), first, count, idx, nc, w, sg, h->k, N, R, first_real - h->path_base,
                             h->mean, z);
        else
          hipLaunchKernelGGL(sgs_level_sweep_kernel, dim3((unsigned)(((int64_t)count * rb + 3) / 4)), dim3(256), 0, s,
                             h->order.as<int>(), first, count, idx, nc, w, sg, h->k, R, rb, h->mean, z);
      }
    } else if (per_order) {
      hipLaunchKernelGGL(sgs_sweep_paths_kernel, walkers, dim3(64), 0, s, h->path.as<int64_t>(), h->rank.as<int>(), idx, nc,
                         w, sg, h->k, N, R, first_real - h->path_base, h->mean, z);
    } else if (h->k > SGS_MAX_K) {
      hipLaunchKernelGGL(sgs_sweep_big_kernel, walkers, dim3(64), 0, s, h->path.as<int64_t>(), h->rank.as<int>(), idx, nc, w,
                         sg, h->k, N, R, h->mean, z);
    } else {
      hipLaunchKernelGGL(sgs_sweep_kernel, walkers, dim3(64), 0, s, h->path.as<int64_t>(), h->rank.as<int>(), idx, nc, w, sg,
                         h->k, N, R, h->mean, z);
    }
    GSS_HIP(hipGetLastError());
  }
  if (team)
    hipLaunchKernelGGL(sgs_team_out_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)nteams), dim3(256), 0, s, z,
                       h->inv_sched.as<int>(), N, R, RL, out);
  else if (!per_order)
    hipLaunchKernelGGL(sgs_transpose_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((R + 63) / 64)), dim3(256), 0, s, z,
                       N, R, out);
  GSS_HIP(hipGetLastError());
  return GSS_OK;
}

}  // namespace gss

using namespace gss;

extern "C" {

int32_t gss_sgs_realize(gss_sgs_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                        double* out, int32_t mem, void* stream) {
  GSS_ENTRY();
  GSS_REQUIRE(h != nullptr, "NULL handle");
  GSS_REQUIRE(nreals >= 0 && first_real >= 0 && nreals < INT_MAX, "bad realisation range");
  if (nreals == 0) return GSS_OK;
  GSS_REQUIRE(out != nullptr, "gss_sgs_realize: out is NULL");
  hipStream_t s = to_stream(stream);
  const int64_t N = h->N;
  if (h->npaths > 1) {   // one visiting order per realisation: realisation first_real + i walks path first_real + i - path_base
    const int64_t p0 = first_real - h->path_base;
    GSS_REQUIRE(p0 >= 0 && p0 + nreals <= h->npaths, "realisations %lld..%lld have no visiting order in this handle "
                "(paths cover %lld..%lld)", (long long)first_real, (long long)(first_real + nreals - 1),
                (long long)h->path_base, (long long)(h->path_base + h->npaths - 1));
  }
  if (mem == GSS_MEM_DEVICE) {
    GSS_TRY(sgs_realize_block(h, seed, first_real, nreals, noise, out, s));
    GSS_HIP(hipStreamSynchronize(s));
    return GSS_OK;
  }
  // Host arrays (seq.jl:137-141 returns host vectors): blocks of realisations -- whole groups of 64 lanes for a shared
  // visiting order -- through the output ring; block b crosses the bus while block b + 1 is swept.
  int64_t rb = OutStream::default_chunk(sizeof(double) * (size_t)N, nreals);
  if (h->npaths <= 1 && rb < nreals) rb = rb < 64 ? 64 : rb / 64 * 64;
  if (rb > nreals) rb = nreals;
  OutStream os;
  GSS_TRY(os.begin(out, sizeof(double) * (size_t)N, nreals, mem, s, rb));
  DevBuf nbuf;
  if (noise) GSS_TRY(nbuf.alloc(sizeof(double) * (size_t)(rb * N)));
  for (int64_t r0 = 0; r0 < nreals; r0 += rb) {
    const int64_t n = nreals - r0 < rb ? nreals - r0 : rb;
    if (noise)
      GSS_HIP(hipMemcpyAsync(nbuf.p, noise + r0 * N, sizeof(double) * (size_t)(n * N), hipMemcpyHostToDevice, s));
    double* dout = nullptr;
    GSS_TRY(os.slot(r0, s, &dout));
    GSS_TRY(sgs_realize_block(h, seed, first_real + r0, n, noise ? nbuf.as<double>() : nullptr, dout, s));
    GSS_TRY(os.done(r0 + n - 1, s));
  }
  return os.finish(s);
}

}  // extern "C"
