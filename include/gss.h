/*
 * gss.h -- C-ABI of libgss_hip.so: MI355X (gfx950) kernels for the kriging-estimation and
 * Gaussian-simulation hot path of juliohm/GeoStatsSolvers.jl (KrigingSolver, FFTGS, LUGS) and, on the
 * same kernels, IDWSolver, LWRSolver and SGS.
 *
 * This is the drop-in boundary.  The reference is
 * pure Julia and has no FFI of its own; each entry point below replaces the arithmetic that the
 * cited reference lines delegate to their Julia dependencies, and is what a `ccall` from the
 * reference's `solve` / `preprocess` / `solvesingle` methods binds.
 *
 * Conventions
 *   - every function returns an int32 status (GSS_OK == 0); no C++ exception crosses the ABI;
 *     gss_last_error() returns the message of the last failure on the calling thread.
 *   - coordinates are "point-major": point i occupies d consecutive doubles.  This is the memory
 *     layout of a Julia d x n column-major matrix (PointSet coordinates), so Julia passes them
 *     without a copy.
 *   - all floating point is FP64, indices are int32/int64 as declared, 0-based on this side.
 *   - `mem` says where the LARGE arrays of the call live: GSS_MEM_HOST (library copies through
 *     PCIe; gss_krig_predict_global overlaps the copies with the computation, piece by piece) or GSS_MEM_DEVICE (pointers are HBM addresses on the current device; nothing is
 *     copied and the call is asynchronous on `stream`).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls may arrive on different streams:
 *     the library recycles its scratch memory across calls, so a call on a new stream is ordered (event wait,
 *     on the device) behind everything the library queued on the stream of the previous call.
 *     Some calls spread independent pieces of their work over helper streams of the process (gss_fftgs_realize:
 *     slabs of the strided FFT passes; gss_lugs_create / gss_lugs_realize: trailing updates beside the next panel,
 *     column blocks of L22 W; the estimation calls on host arrays: copies beside the computation; gss_krig_create
 *     with GSS_KRIG_ASYNC_FIT: the fit).  The process has five such streams, created together at the first use.
 *     Those streams are fenced by events on both sides: everything such a call does starts
 *     after what `stream` held at the call and is complete, in stream order, before whatever is put on `stream` next.
 *   - host threads: every export takes one process-wide lock for its whole duration, so calls from several host
 *     threads (Julia `Threads.@threads` over variables, finalizers on the GC thread) are SAFE and run one after
 *     another -- whichever handles and streams they use; the stream chain above then orders their device work.  What
 *     is NOT provided is concurrency: a call with host arrays holds the lock until its last byte has arrived.  A
 *     handle may be used from any thread, by one call at a time (which the lock guarantees).  `gss_last_error` is
 *     per thread.
 *   - host results of the simulation calls (gss_fftgs_realize, gss_lugs_realize, gss_sgs_realize with GSS_MEM_HOST)
 *     leave the device in chunks of ~256 MiB while the following realisations are computed; at most three chunks are
 *     staged in HBM whatever `nreals` is.  A page-locked destination (hipHostMalloc / hipHostRegister) is written by
 *     the DMA engine directly; a pageable one goes through pinned bounce buffers of the library.
 *   - handles are opaque and owned by the library; the caller owns every buffer it passes and the library never
 *     returns memory it allocated.
 */
#ifndef GSS_H
#define GSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSS_VERSION 100

/* ---- status codes ------------------------------------------------------------------------ */
enum {
  GSS_OK = 0,
  GSS_ERR_INVALID = 1,      /* bad argument (maps to ArgumentError / AssertionError in the shim) */
  GSS_ERR_HIP = 2,          /* HIP / rocFFT runtime failure                                      */
  GSS_ERR_NOT_POSDEF = 3,   /* covariance factorisation hit a non-positive pivot                  */
  GSS_ERR_UNSUPPORTED = 4,  /* feature outside the hot-path scope           */
  GSS_ERR_NO_DEVICE = 5,
  GSS_ERR_ALLOC = 6,
  GSS_ERR_NO_CONVERGENCE = 7 /* an iterative solve reached its iteration limit (gss_spde_realize)   */
};

enum { GSS_MEM_HOST = 0, GSS_MEM_DEVICE = 1 };

/* ---- variogram model: replaces Variography.jl objects at fft.jl:91,98; lu.jl:110,124,131,132;
 *      krig.jl:65 (solver parameter `variogram`) -------------------------------------------- */
enum {
  GSS_VG_GAUSSIAN = 0,
  GSS_VG_EXPONENTIAL = 1,
  GSS_VG_SPHERICAL = 2,
  GSS_VG_MATERN = 3,         /* any order nu in (0, 50]; 1 is the reference's default order                   */
  GSS_VG_CUBIC = 4,
  GSS_VG_PENTASPHERICAL = 5,
  GSS_VG_SINEHOLE = 6,       /* gamma = (sill - nugget) (1 - sin(pi h/r) / (pi h/r)) + nugget          */
  GSS_VG_POWER = 7           /* gamma = scaling h^exponent + nugget: NOT stationary.  Fields: range = scaling,
                              * nu = exponent in (0,2), sill = constant A of the pseudo-covariance A - gamma(h)
                              * (any A >= max gamma over the data; ordinary / universal / external-drift
                              * kriging results do not depend on it).  Rejected by simple kriging and by the
                              * simulation solvers (fft.jl:91, lu.jl:110).                                  */
};

typedef struct gss_variogram {
  int32_t kind;        /* GSS_VG_*                                                   */
  int32_t dim;         /* embedding dimension d, 1..3                                */
  double sill;
  double nugget;
  double range;        /* isotropic range; ignored (==1) when aniso != 0             */
  double nu;           /* Matern order                                               */
  int32_t aniso;       /* 1: Mahalanobis distance with inv_radii (MetricBall((a,b)));
                        * 2: rotated ball (MetricBall((a,b), R)): inv_radii along the columns of `rotation`  */
  int32_t reserved;
  double inv_radii[3]; /* 1 / ball radii                                             */
  /* nested models gamma = sum_i c_i gamma_i ([DEP] Variography NestedVariogram): the fields above describe the
   * first structure (its `sill` includes the TOTAL nugget), each extra structure adds `sill` = its own contribution
   * with its own kind / range / anisotropy.  Total sill = sill + sum extra[i].sill.                              */
  int32_t nextra;      /* 0..3 */
  int32_t reserved2;
  struct {
    int32_t kind;
    int32_t aniso;
    double sill;
    double range;
    double nu;
    double inv_radii[3];
  } extra[3];
  /* Rotated anisotropy (read only where a structure has aniso = 2): row-major 3 x 3 proper rotation R whose leading
   * d x d block holds the principal axes of the ball as columns; d(x, y) = || diag(1/r) R^T (x - y) ||, i.e. the
   * Mahalanobis distance with M = R diag(r^-2) R^T.  One rotation serves every rotated structure of the model.
   * The library checks max |R^T R - I| <= 1e-12 and det R > 0 (GSS_ERR_INVALID otherwise); an exact identity takes
   * the axis-aligned path.  Covariances are evaluated on the frame coordinates x' = R^T (x - c), c = the first point
   * of the array the call or handle is created with.  Appended: the offsets above are
   * unchanged and callers that never set aniso = 2 need not fill it. */
  double rotation[9];
} gss_variogram_t;

/* ---- kriging variant: replaces ui.jl:40-50 (kriging_ui) model choice ---------------------- */
enum { GSS_KRIG_SIMPLE = 0, GSS_KRIG_ORDINARY = 1, GSS_KRIG_UNIVERSAL = 2, GSS_KRIG_EXTDRIFT = 3 };

/* per-point status byte written by the predict calls (krig.jl:213-214 `missing, missing`) */
enum { GSS_PT_OK = 0, GSS_PT_MISSING = 1, GSS_PT_SINGULAR = 2 };

typedef struct gss_krig gss_krig_t;
typedef struct gss_fftgs gss_fftgs_t;
typedef struct gss_lugs gss_lugs_t;
typedef struct gss_spde gss_spde_t;
typedef struct gss_sgs gss_sgs_t;

/* ---- library ------------------------------------------------------------------------------ */
int32_t gss_version(void);
int32_t gss_device_count(int32_t* count);
int32_t gss_init(int32_t device);          /* bind the calling process to `device` (one process per GPU) */
int32_t gss_shutdown(void);
int32_t gss_last_error(char* buf, int32_t len);
int32_t gss_synchronize(void* stream);
/* Copy `bytes` from device memory (produced on `stream`) to host memory at the rate the simulation calls deliver their
 * results: a page-locked destination directly, a pageable one through the library's pinned bounce buffers (pieces of
 * 32 MiB, the host copy of one piece beside the transfer of the next).  For hosts that compose results on the device
 * (the conditional branch fft.jl:176-192) and hand the reference's host vectors back.  Returns when the data are there. */
int32_t gss_dev_to_host(void* dst, const void* src_dev, int64_t bytes, void* stream);
/* Released device blocks are cached for re-use (up to GSS_POOL_MAX_MB, default a quarter of the device memory that
 * was free at the first allocation, at most 16 GiB); gss_trim_pool gives them all back to the driver -- for a host
 * program whose own allocator (torch, RCCL, rocFFT) has just failed.  Synchronises the device. */
int32_t gss_trim_pool(void);
/* Counters for tests and diagnostics: "pool_bytes" (device bytes in the block cache), "out_ring_bytes" (HBM staged for
 * the host outputs of the last simulation call), "out_chunks" (chunks that call moved), "fit_slot_allocs" (pinned status
 * slots allocated so far for kriging fits: constant once handles are created and closed at a steady rate), "panel_giveups" (times a
 * single-launch factorisation left through its bounded wait and was repeated on the launch-per-block path),
 * "gemm_launches_128" / "gemm_launches_64" (FP64 matrix products launched so far on the 128 x 128 and on the 64 x 64
 * tile kernel: which of the two a given shape ran on),
 * "vario_tiles_total" / "vario_tiles_opened" (batch pairs of the last gss_variogram_empirical or gss_variogram_plane
 * and how many of them its box bound let through),
 * "ipc_route" (how the last gss_state_ipc_import reached the owner's device: 0 same device, 1 visible peer, 2 not among
 * the visible devices, 3 refused -- visible but not peer-accessible). */
int32_t gss_stat(const char* name, int64_t* value);

/* ---- multi-GPU: one process per GPU, the preprocess state of rank 0 replicated to the peers -----------------
 *      The reference runs `preprocess` once and maps `solvesingle` over realisations, on worker processes if asked
 *      (fft.jl:62,145; lu.jl:76,171); kriging shards domain points over a replicated factor (krig.jl:180).  Realisation
 *      r depends on (seed, r) only, so the shards need nothing else from each other.  Two routes, both behind this ABI:
 *
 *      RCCL ("ncclBroadcast of the factor over xGMI"): rank 0 calls gss_comm_unique_id, the HOST carries
 *      the GSS_COMM_ID_BYTES bytes to the peers (Julia `remotecall`, an MPI / torch.distributed broadcast, a file ...),
 *      every rank calls gss_comm_init after gss_init(device); then gss_state_bcast(kind, handle, root, stream) on every
 *      rank -- the root with the handle it computed, the peers with one created GSS_*_NO_FACTOR / _NO_SPECTRUM from the
 *      same inputs -- is one ncclBroadcast of the state buffer followed by the peers' adopt.  RCCL is loaded at run time.
 *
 *      HIP IPC (no communicator, works between processes that share one device as well): the owner writes a token with
 *      gss_state_ipc_export, the host carries its GSS_IPC_TOKEN_BYTES bytes, a peer calls gss_state_ipc_import: it maps
 *      the owner's buffer, pulls it with one device-to-device copy over its own xGMI link and adopts.  The owner keeps
 *      its handle alive until the peers have imported.  The token names the owner's device (PCI domain / bus / device):
 *      the importer enables peer access when that device is another visible one, and refuses -- GSS_ERR_UNSUPPORTED, the
 *      message names gss_state_bcast and recomputation -- when it is visible but not peer-accessible.             */
enum { GSS_STATE_KRIG = 0, GSS_STATE_FFTGS = 1, GSS_STATE_LUGS = 2 };   /* which create call `handle` came from */
#define GSS_COMM_ID_BYTES 128
#define GSS_IPC_TOKEN_BYTES 96
int32_t gss_comm_unique_id(uint8_t* id);                               /* id[GSS_COMM_ID_BYTES], root only */
int32_t gss_comm_init(const uint8_t* id, int32_t rank, int32_t nranks);
int32_t gss_comm_info(int32_t* rank, int32_t* nranks);                 /* -1, 0 without a communicator */
int32_t gss_comm_destroy(void);
int32_t gss_state_bcast(int32_t kind, void* handle, int32_t root, void* stream);
int32_t gss_state_ipc_export(int32_t kind, void* handle, uint8_t* token);          /* token[GSS_IPC_TOKEN_BYTES] */
int32_t gss_state_ipc_import(int32_t kind, void* handle, const uint8_t* token, void* stream);

/* ---- kernel timing (bench.py's roofline leg): when enabled every launch of a named hot kernel is
 *      bracketed by HIP events on the stream it is launched on; gss_profile_read synchronises
 *      those events and returns the summed duration and the launch count for `name`
 *      ("krig_rhs", "cokrig_rhs", "krig_quadform", "fftgs_noise", "fftgs_fwd", "fftgs_phase", "fftgs_inv", ...). */
int32_t gss_profile_enable(int32_t on);
int32_t gss_profile_reset(void);
int32_t gss_profile_read(const char* name, double* total_ms, int64_t* launches);

/* ---- pairwise covariance: replaces `sill(g) .- Variography.pairwise(g, A, B)` at
 *      fft.jl:98, lu.jl:124,131,132.  out is na x nb, row-major with leading dimension ldo.
 *      b == NULL computes the symmetric na x na matrix. ---------------------------------------- */
int32_t gss_cov_pairwise(const gss_variogram_t* vg, const double* a, int64_t na, const double* b,
                         int64_t nb, double* out, int64_t ldo, int32_t mem, void* stream);

/* ---- variography: replaces [DEP] Variography's EmpiricalVariogram / DirectionalVariogram and `fit`, the step that
 *      produces the solver parameter `variogram` (krig.jl:65, fft.jl:52, lu.jl:68).  That package is not in the
 *      reference tree: the conventions below are this library's own, stated so that every pair's bin can be reproduced.
 *
 * gss_variogram_empirical: one pass over the n (n - 1) / 2 unordered sample pairs (Euclidean distance only).
 *   x n x dim point-major (dim 1..3), z: nz columns of n (column c at z + c * n).  Limits: n in 2 .. 2^31 - 2,
 *   nlags in 1 .. 256, nz in 1 .. 8.  Every coordinate and value must be finite (GSS_ERR_INVALID otherwise): a missing
 *   value is the caller's to drop, and `count` is therefore one vector for all columns.
 *   Pair key   d2 = ((D0 D0) + (D1 D1)) + (D2 D2), D = x_i - x_j, one rounding per operation, no FMA (the key of
 *              gss_knn_search).  Bins are decided on d2, never on a square root: with delta = maxlag / nlags and
 *              edge2[k] = fl(fl(k delta)^2), k = 0 .. nlags, a pair belongs to bin k iff edge2[k] < d2 <= edge2[k + 1]
 *              (the bin (k delta, (k + 1) delta]).  d2 == 0 is counted in *nduplicates and otherwise skipped;
 *              d2 > edge2[nlags] is skipped.
 *   Direction  NULL: omnidirectional.  Else `dim` doubles IN HOST MEMORY whatever `mem` is (a parameter, not data), a
 *              unit vector u (| ||u|| - 1 | <= 1e-12): t = (D0 u0 + D1 u1) + D2 u2, p2 = d2 - t t (rounded operations in
 *              that order); the pair is kept iff p2 <= fl(dtol^2) (bandwidth; dtol = +inf: none) and
 *              t t >= fl(fl(cos_atol^2) d2) (cone of half-angle acos(cos_atol); 0: none).  Both senses +-u count.
 *   Outputs    count[nlags]; lagsum[nlags] = sum of h = sqrt(d2); zsum[nz x nlags] (column c at zsum + c * nlags) =
 *              sum (z_i - z_j)^2 (GSS_VARIO_MATHERON) or sum |z_i - z_j|^(1/2) (GSS_VARIO_CRESSIE).  The front-ends form
 *              the abscissa lagsum / count and gamma = zsum / (2 count)  resp.
 *              gamma = (zsum / count)^4 / (2 (0.457 + 0.494 / count)) (Cressie-Hawkins).
 *              The counts are exact and the same on every run; the floating-point sums depend on the order the device
 *              happened to add in (relative difference below 2 count 2^-53).
 *   mem        GSS_MEM_DEVICE: x, z and the four outputs are device arrays, written in stream order.  Below 32 768
 *              samples nothing waits for the stream; from there on the call waits for it once, while the samples are
 *              put in the k-d order of the neighbour search.  A non-finite input is found on the device: the call on
 *              host arrays returns GSS_ERR_INVALID; the call on device arrays cannot know it without waiting and
 *              reports it through the outputs instead -- every count and *nduplicates are -1 and the sums NaN.
 *   Samples are visited batch by batch of 64 in a space-filling order (the k-d order of the neighbour search from
 *   32 768 samples, one sort by Morton key below); a pair of batches whose bounding boxes are farther apart than maxlag
 *   is never opened.  gss_stat "vario_tiles_total" / "vario_tiles_opened" are process-wide counters for tests and
 *   tools: they describe the call whose reduction ran last (calls in flight on several streams share them), and
 *   reading the second waits for that call.  The environment variable GSS_VARIO_CULL=0 opens every tile, for tests:
 *   the results are the same.  The bin edges are formed as fl(fl(k delta)^2) where they are used. */
enum { GSS_VARIO_MATHERON = 0, GSS_VARIO_CRESSIE = 1 };
int32_t gss_variogram_empirical(const double* x, int64_t n, int32_t dim, const double* z, int32_t nz,
                                int32_t nlags, double maxlag, const double* direction, double dtol, double cos_atol,
                                int32_t estimator, int64_t* count, double* lagsum, double* zsum,
                                int64_t* nduplicates, int32_t mem, void* stream);
/* gss_variogram_fit (host code, no device): weighted least squares of gamma(h) = nugget + (sill - nugget) f(h / range)
 *   to the bins with count > 0; objective sum_k w_k (gamma_model(h_k) - gamma_k)^2 with w = count, count / h^2 or 1.
 *   For a fixed range the objective is linear least squares in (nugget, sill - nugget) >= 0 with
 *   nugget <= max_nugget_frac * sill (1: free), solved in closed form (unconstrained, else the best feasible edge);
 *   the range is searched on a log-spaced grid of 256 points over [h_min / 4, 4 h_max] and refined by golden section
 *   to a relative width of 1e-8.  Deterministic.  kinds: GSS_VG_GAUSSIAN .. GSS_VG_SINEHOLE (Matern at order nu);
 *   GSS_VG_POWER -> GSS_ERR_UNSUPPORTED.  The Gaussian kind is fitted as the bare formula: a front-end that applies
 *   the `nugget + 1e-6` rule hands the solvers nugget - 1e-6, or switches the rule off when
 *   the fitted nugget is smaller.  objective[nkinds]: per kind (NaN where no positive sill fits); *best: the kind with
 *   the smallest objective -- kind, sill, nugget, range, nu filled in, isotropic, dim = 0 left to the caller. */
enum { GSS_FIT_W_COUNT = 0, GSS_FIT_W_COUNT_OVER_H2 = 1, GSS_FIT_W_UNIFORM = 2 };
int32_t gss_variogram_fit(const double* h, const double* gamma, const int64_t* count, int32_t nlags,
                          const int32_t* kinds, int32_t nkinds, double nu, int32_t weighting,
                          double max_nugget_frac, gss_variogram_t* best, double* objective);

/* gss_variogram_plane (varioplane): the same pass over the pairs, every kept pair binned by (direction sector, lag).
 *   The sectors partition the half-circle of directions in a plane, so over the sectors the counts add up exactly to
 *   those of the omnidirectional gss_variogram_empirical on the same inputs (in 3-D: when there is no slab).
 *   Everything gss_variogram_empirical states above holds word for word: the pair key d2, the bin edges
 *   edge2[k] = fl(fl(k delta)^2), the rule edge2[k] < d2 <= edge2[k + 1], duplicates counted apart, the finite-input
 *   rule in both memory modes, the batch ordering (Morton below 32 768 samples, k-d from there), tile culling against
 *   edge2[nlags] with the vario_tiles_* counters and GSS_VARIO_CULL, both estimators, Euclidean distance only.  The lag
 *   bin always uses the full d2.
 *   dirs       2 nangles doubles IN HOST MEMORY whatever `mem` is (a parameter, like `direction`):
 *              (c_s, s_s) = (cos theta_s, sin theta_s), s = 0 .. nangles - 1, the LOWER boundaries of the sectors.  The
 *              angles are strictly increasing with theta_{nangles-1} - theta_0 < pi and each (c_s, s_s) is a unit vector
 *              to 1e-12; anything else is GSS_ERR_INVALID.  Sector s is [theta_s, theta_{s+1}), the last one
 *              [theta_{nangles-1}, theta_0 + pi), directions taken modulo pi.
 *   In-plane components (a1, a2) of the lag D = x_i - x_j:
 *              dim = 2: `basis` must be NULL and (a1, a2) = (D0, D1).
 *              dim = 3: `basis` is 9 host doubles e1, e2, nrm (three vectors, orthonormal to 1e-12):
 *                       a1 = (D0 e1_0 + D1 e1_1) + D2 e1_2, a2 likewise with e2, w = D . nrm likewise; rounded operations
 *                       in that order, no FMA.  The pair is kept iff fl(w w) <= fl(ptol^2); ptol = +inf: no slab, the
 *                       lag is projected onto the plane.  (ptol is not read when dim = 2.)
 *              dim = 1 is refused.
 *   Sector of a kept pair:
 *              1. p = fl(c_0 a2), q = fl(s_0 a1).
 *              2. If p == q the sector is 0.
 *              3. Otherwise, if p < q, negate (a1, a2) (exact).
 *              4. The sector is the number of s in 1 .. nangles - 1 with fl(c_s a2) >= fl(s_s a1).
 *              The rule is total, does not depend on which sample of a pair comes first, is closed at a sector's lower
 *              boundary and open at its upper one, and equals floor(((atan2(a2, a1) - theta_0) mod pi) / Delta) for
 *              uniform sectors up to pairs within rounding of a boundary.
 *   Limits     nangles in 2 .. 180, nlags in 1 .. 256, nz in 1 .. 4 and nangles * nlags * (2 + nz) <= 8192 (the
 *              histogram of a workgroup: 64 KiB of the 160 KiB of local memory, so that two workgroups share a compute
 *              unit); beyond any of them GSS_ERR_INVALID with a message that names the limit.
 *   Outputs    count[nangles x nlags] (sector s at count + s * nlags), lagsum likewise,
 *              zsum[nz x nangles x nlags] (column c at zsum + c * nangles * nlags), *nduplicates (all pairs with
 *              d2 == 0, whatever the slab).  Counts are exact and the same on every run. */
int32_t gss_variogram_plane(const double* x, int64_t n, int32_t dim, const double* z, int32_t nz, int32_t nlags,
                            double maxlag, int32_t nangles, const double* dirs, const double* basis, double ptol,
                            int32_t estimator, int64_t* count, double* lagsum, double* zsum, int64_t* nduplicates,
                            int32_t mem, void* stream);
/* gss_variogram_fit_aniso (host code, no device): 2-D geometric anisotropy fitted to a varioplane,
 *   gamma(h, phi) = nugget + (sill - nugget) f(h sqrt(cos^2(phi - theta) / r1^2 + sin^2(phi - theta) / r2^2)),
 *   r1 >= r2 > 0, theta in [0, pi), f as in gss_variogram_fit.  Per bin (nbins of them, any order): h (the abscissa
 *   lagsum / count), phi (the caller's angle for the bin's sector, radians: the front-ends pass the mid-sector angle),
 *   gamma and count; bins with count <= 0 are ignored.  kinds, nu, weighting, max_nugget_frac, objective as in
 *   gss_variogram_fit.  For fixed (theta, r1, r2) the inner problem is that call's closed-form solve.  Outer search,
 *   deterministic: a grid of 36 angles x 32 log-spaced r1 over [h_min / 4, 4 h_max] x 16 log-spaced ratios r2 / r1 in
 *   [1/16, 1]; the best points of the grid are each refined by cyclic golden-section searches of (r1, ratio, theta) to a
 *   relative width of 1e-8 and the best result is kept.
 *   *best is filled as a MetricBall((r1, r2), Angle2d(theta)) model: aniso = 2, range = 1, inv_radii = (1/r1, 1/r2, 1),
 *   rotation = the counter-clockwise rotation by theta (row-major 3 x 3, identity on the third axis); when the best
 *   ratio is 1 the isotropic form is returned instead: aniso = 0, range = r1, identity rotation.  dim = 0 is left to the
 *   caller.  GSS_VG_POWER -> GSS_ERR_UNSUPPORTED.  (A fit of the full 3-D ellipsoid is not offered.) */
int32_t gss_variogram_fit_aniso(const double* h, const double* phi, const double* gamma, const int64_t* count,
                                int32_t nbins, const int32_t* kinds, int32_t nkinds, double nu, int32_t weighting,
                                double max_nugget_frac, gss_variogram_t* best, double* objective);

/* gss_variogram_cross: direct AND cross variograms of nz variables in one pass over the pairs -- the pair geometry
 *   (key, bin, cull) does not depend on the column and is paid once.  Everything gss_variogram_empirical states above
 *   holds word for word: the pair key d2, the bin edges edge2[k] = fl(fl(k delta)^2), the rule
 *   edge2[k] < d2 <= edge2[k + 1], duplicates counted apart, the direction test (host unit vector, dtol, cos_atol), the
 *   finite-input rule in both memory modes, the batch ordering (Morton below 32 768 samples, k-d from there), tile
 *   culling with the vario_tiles_* counters and GSS_VARIO_CULL, Euclidean distance only, the limits of n, nlags and nz
 *   (1 .. 8; nz = 1 is the direct call).  count, lagsum and *nduplicates are the values that call returns on the same
 *   inputs.  Matheron only: the Cressie-Hawkins estimator has no cross form, so there is no `estimator`.  There is no
 *   cross form of gss_variogram_plane.
 *   csum       nz (nz + 1) / 2 rows of nlags: the pair (a, b), a <= b, at row a nz - a (a - 1) / 2 + (b - a) holds
 *              sum fl((z_a,i - z_a,j) (z_b,i - z_b,j)) over the kept pairs of the bin (one rounded product per pair, no
 *              FMA).  The product does not depend on which sample of a pair comes first.  The front-ends form
 *              gamma_ab = csum / (2 count); the rows (a, a) are the direct variograms (the zsum of
 *              gss_variogram_empirical up to the order of addition).  The counts are exact and the same on every run;
 *              a sum differs from the exact one by at most count 2^-53 sum |products|.
 *   Local memory: the histogram of a workgroup is (2 + nz (nz + 1) / 2) nlags + 2 words, 78 KiB at nz = 8 and
 *   nlags = 256 of the 160 KiB of a compute unit: two workgroups could share it there.  That is accepted and the
 *   product is not capped: the registers of the nz = 8 instantiation (one wave per SIMD, one workgroup per compute
 *   unit) bind before the local memory does. */
int32_t gss_variogram_cross(const double* x, int64_t n, int32_t dim, const double* z, int32_t nz, int32_t nlags,
                            double maxlag, const double* direction, double dtol, double cos_atol, int64_t* count,
                            double* lagsum, double* csum, int64_t* nduplicates, int32_t mem, void* stream);
/* gss_variogram_fit_lmc (host code, no device): the linear model of coregionalisation
 *   Gamma(h) = B0 + B1 f(h / range) fitted to the bins with count > 0.  Gamma is the nz x nz matrix of direct and cross
 *   variograms, given as `gamma`: nz (nz + 1) / 2 rows of nlags in the row order of csum above.  B0 (nugget matrix) and
 *   B1 (partial sills) are symmetric positive semidefinite; one structure f (a kind of gss_variogram_fit, Matern at
 *   order nu; GSS_VG_POWER -> GSS_ERR_UNSUPPORTED) and one range are shared by all pairs.  Objective
 *   sum_k w_k || Gamma_k - B0 - B1 f_k ||_F^2 over the full matrices (off-diagonals count twice), w as in
 *   gss_variogram_fit.  For a fixed range, Goulard-Voltz sweeps from the unconstrained least squares of every entry:
 *   B0 <- P+(sum w (Gamma - B1 f) / sum w), B1 <- P+(sum w f (Gamma - B0) / sum w f^2), until neither moves by more than
 *   1e-12 (||B0||_F + ||B1||_F) or 1 000 sweeps; P+ clips the negative eigenvalues of a cyclic Jacobi decomposition
 *   (fixed rotation order).  The range is searched as in gss_variogram_fit (256-point log grid over
 *   [h_min / 4, 4 h_max], golden section to 1e-8).  Deterministic.  nz = 1 returns the numbers of gss_variogram_fit
 *   with max_nugget_frac = 1.  Outputs: *kind (the best of kinds), *range, b0 and b1 (nz x nz, row-major),
 *   objective[nkinds] (NaN where some variable gets no positive sill B0_aa + B1_aa).  The Gaussian kind is the bare
 *   formula, as in gss_variogram_fit.  GSS_ERR_INVALID: nz outside 1 .. 8, fewer than two usable bins. */
int32_t gss_variogram_fit_lmc(const double* h, const double* gamma, const int64_t* count, int32_t nlags, int32_t nz,
                              const int32_t* kinds, int32_t nkinds, double nu, int32_t weighting, int32_t* kind,
                              double* range, double* b0, double* b1, double* objective);

/* ---- neighbour search: replaces `search!(neighbors, center, searcher)` krig.jl:210 and the
 *      KNearestSearch / KBallSearch construction ui.jl:27,30.  Exact; neighbours ordered by
 *      ascending (FP64 squared distance accumulated in dimension order without FMA, index).
 *      radius < 0: plain k-NN.  radius >= 0: only neighbours with d^2 <= radius^2 (isotropic) or
 *      Mahalanobis d^2 <= 1 when inv_radii != NULL.  idx is m x k (int32, -1 padded). ---------- */
enum {                        /* solver parameter `distance` (krig.jl:72, idw.jl:54, lwr.jl:57), [DEP] Distances.jl */
  GSS_METRIC_EUCLIDEAN = 0,   /* default; with inv_radii: Mahalanobis ball                                       */
  GSS_METRIC_CITYBLOCK = 1,
  GSS_METRIC_CHEBYSHEV = 2,
  GSS_METRIC_HAVERSINE = 3,   /* points are (longitude, latitude) in degrees, metric_param = sphere radius       */
  GSS_METRIC_ROTATED_BALL = 4 /* rotated ball: inv_radii points at 12 doubles -- three inverse radii, then the
                               * row-major rotation[9] of gss_variogram_t; the ball is d <= 1 (radius = 1)        */
};
/* metric != EUCLIDEAN cannot be combined with a ball (searcher_ui uses either the ball or the metric, ui.jl:25-31). */
int32_t gss_knn_search(const double* xdata, int64_t n, int32_t dim, const double* centers, int64_t m,
                       int32_t k, double radius, const double* inv_radii, int32_t metric, double metric_param,
                       int32_t* idx, int32_t* count, int32_t mem, void* stream);

/* ---- KrigingSolver ------------------------------------------------------------------------
 * gss_krig_create replaces preprocess (krig.jl:76-128) + GeoStatsModels.fit of exactsolve
 * (krig.jl:176): it uploads the non-missing samples and, unless GSS_KRIG_NO_FACTOR is set,
 * factorises the (n+nc)^2 kriging system on the device.
 *   xdata n x d point-major, z n values, drift_data n x ndrift (EXTDRIFT only, row per point).
 *   xdata, z and drift_data are HOST arrays (the preprocess of krig.jl:76-128 is host logic: the library reads the
 *   coordinates for the drift centring / scaling and the search index, then uploads them); only the predict calls
 *   take `mem`.
 */
enum {
  GSS_KRIG_NO_FACTOR = 1, /* moving-neighbourhood use only, or factor arrives by broadcast */
  /* gss_krig_create returns once the fit is queued (on a stream of the library, behind what `stream` holds): the
   * first gss_krig_predict_global assembles its right-hand sides beside it, and reports the fit's status
   * (GSS_ERR_NOT_POSDEF) itself; any other use of the factor waits for the fit first.  The reference's `solve`
   * fits and predicts in one call (krig.jl:166-186), so nothing changes for it. */
  GSS_KRIG_ASYNC_FIT = 2
};

int32_t gss_krig_create(gss_krig_t** out, const gss_variogram_t* vg, int32_t variant, double sk_mean,
                        int32_t degree, int32_t ndrift, const double* xdata, const double* z,
                        const double* drift_data, int64_t n, int32_t flags, void* stream);
int32_t gss_krig_destroy(gss_krig_t* h);

/* number of constraints nc and system size n+nc */
int32_t gss_krig_info(const gss_krig_t* h, int64_t* n, int32_t* nc);

/* device address + size of the factor state (inverse block factor W' and dual weights) so that
 * the host can broadcast it to peer GPUs over RCCL; after a broadcast into
 * a handle created with GSS_KRIG_NO_FACTOR call gss_krig_adopt_factor. */
int32_t gss_krig_factor_buffer(gss_krig_t* h, void** dev_ptr, int64_t* bytes);
int32_t gss_krig_adopt_factor(gss_krig_t* h);

/* global neighbourhood: replaces the predictprob loop krig.jl:180-183.
 * xdom m x d point-major, drift_dom m x ndrift; outputs mean[m], var[m], status[m]. */
int32_t gss_krig_predict_global(gss_krig_t* h, const double* xdom, const double* drift_dom, int64_t m,
                                double* mean, double* var, uint8_t* status, int32_t mem, void* stream);

/* Block support (optional; default: point support at the centroids).
 * krig.jl:180 hands `pdomain[ind]` -- on a grid the CELL -- to predictprob, and [RECALL] the reference's dependencies
 * then average the covariances over sample points inside the cell.  After this call gss_krig_predict_global and
 * gss_krig_predict_knn treat xdom as centroids of cells of size cell[0..d-1] and regularises by the midpoint rule with nsub points per axis
 * (nsub^d samples s): c0_i = mean_s C(x_i, c + s), variance = mean_{s,s'} C(s, s') - c0 . weights.  Simple / ordinary
 * kriging and drifts of degree <= 1 (whose cell average is the centroid value).  nsub = 0 or cell = NULL: back to
 * point support.  The dependency's own sampling scheme is version dependent and not in the tree: this one is the
 * library's documented convention. */
int32_t gss_krig_set_block_support(gss_krig_t* h, const double* cell, int32_t nsub, void* stream);

/* moving neighbourhood: replaces approxsolve krig.jl:188-234 (search + fit + predictprob per point).
 * k = maxneighbors (already clamped by searcher_ui; 1..4096: up to 64 on the MFMA-tile kernel, beyond that the
 * search runs in passes of 64 and one workgroup solves each point's system), radius / inv_radii / metric as gss_knn_search
 * (the metric only ranks neighbours; covariances keep the variogram's own distance).
 * idx_out (m x k int32) and count_out (m) may be NULL. */
int32_t gss_krig_predict_knn(gss_krig_t* h, const double* xdom, const double* drift_dom, int64_t m,
                             int32_t k, int32_t minneighbors, double radius, const double* inv_radii,
                             int32_t metric, double metric_param, double* mean, double* var, uint8_t* status,
                             int32_t* idx_out, int32_t* count_out, int32_t mem, void* stream);

/* re-use a factorised handle with new data values (same locations): the conditional-FFTGS
 * pattern fft.jl:176-188 where one kriging system serves every realisation.
 * zbatch is nbatch x n; mean_out nbatch x m (row per batch).  No variances. */
int32_t gss_krig_predict_global_batch(gss_krig_t* h, const double* xdom, int64_t m, const double* zbatch,
                                      int64_t nbatch, double* mean_out, int32_t mem, void* stream);

/* ---- cokriging under a linear model of coregionalisation: the estimation step behind gss_variogram_cross and
 *      gss_variogram_fit_lmc.  (The reference has no cokriging solver; the conventions are this library's own.)
 *
 * gss_cokrig_create: the global-neighbourhood system over the stacked samples of nz variables (1 .. 8, the limit of
 *   gss_variogram_cross), fitted like gss_krig_create fits one variable.
 *   Samples    x (n x dim, point-major), z (n), var (n ids in 0 .. nz - 1), HOST arrays in any order; the system keeps
 *              the caller's row order.  Heterotopic sampling is the normal case: any number >= 1 of samples per
 *              variable, at the same or at different locations.
 *   Model      C_ab(h) = b1[a][b] rho(h) for h != 0 and C_ab(0) = b0[a][b] + b1[a][b]; rho is the covariance of
 *              `structure` with sill 1 and nugget 0.  Of `structure` only kind, dim, range, nu, aniso, inv_radii and
 *              rotation are read; nextra must be 0; GSS_VG_POWER -> GSS_ERR_UNSUPPORTED.  A rotated ball is evaluated
 *              on frame coordinates, data and domain alike (gss_variogram_t::rotation).  b0, b1: nz x nz, row-major.
 *   h = 0      is decided as the nugget of every covariance of this library is: on the squared-distance key in frame
 *              coordinates, accumulated without FMA, being zero.  Two variables measured at one location therefore get
 *              the cross nugget b0[a][b]; so does a domain point placed on a sample.
 *   Variants   GSS_KRIG_ORDINARY: traditional ordinary cokriging, nc = nz, one unbiasedness row per variable (the
 *              weights of the target variable sum to 1, those of every other variable to 0); `means` is not read.
 *              GSS_KRIG_SIMPLE: nc = 0, means[nz] known; the residuals z_i - means[var_i] are kriged and means[t] is
 *              added back.  GSS_KRIG_UNIVERSAL / GSS_KRIG_EXTDRIFT -> GSS_ERR_UNSUPPORTED.
 *   Checks     GSS_ERR_INVALID, the message names the entry: nz outside 1 .. 8; b0 or b1 not symmetric to
 *              1e-12 max |entry| (the library then works with (B + B') / 2); a diagonal b0[a][a] + b1[a][a] <= 0; a
 *              variable id outside 0 .. nz - 1; under the ordinary variant a variable without a sample; a non-finite
 *              coefficient, mean, coordinate or value.  Semidefiniteness of b0 and b1 is NOT checked: a model that is
 *              not admissible, or collocated samples under a rank-deficient b1 without nugget, surface as
 *              GSS_ERR_NOT_POSDEF from the fit, as duplicates do for one variable.  The Gaussian kind is the bare
 *              formula: a front-end that applies the `nugget + 1e-6` rule adds it to the diagonal of b0.
 *   flags      GSS_KRIG_ASYNC_FIT as gss_krig_create.  GSS_KRIG_NO_FACTOR -> GSS_ERR_INVALID: the handle without a
 *              factor has a creator of its own, gss_cokrig_create_local.
 *   The handle is a gss_krig_t: gss_krig_destroy, gss_krig_info (n stacked samples, nc) and gss_krig_factor_buffer
 *   apply.  gss_krig_cv_global and gss_krig_cv_global_folds work on it unchanged -- the identities do not care what
 *   the blocks of the system mean: pred_i predicts sample i of variable var_i from all other stacked samples, or from
 *   those outside its fold; a caller removes a whole location by giving its collocated samples one fold id.  (Under
 *   the ordinary variant a fold that holds every sample of some variable leaves that variable's constraint without
 *   support: it is caught by the pivot test of the fold only.)  Every other entry point that takes a gss_krig_t
 *   (gss_krig_predict_global, _predict_global_batch, _predict_knn, _cv_knn, _set_block_support) refuses such a handle
 *   with GSS_ERR_INVALID; the moving neighbourhood of cokriging is gss_cokrig_predict_knn below, its cross-validation
 *   gss_cokrig_cv_knn.
 *
 * gss_cokrig_predict_global: every target variable at every domain point in one call.  xdom m x dim point-major;
 *   mean and variance: nz columns of m (column t at + t * m); status: nz x m bytes (may be NULL).
 *   variance_t = b0[t][t] + b1[t][t] - the quadratic form, clamped at 0 as gss_krig_predict_global clamps.  rho is
 *   evaluated once per (sample, point) and serves the right-hand sides of all nz targets.  `mem`: host arrays travel
 *   piece by piece beside the computation, as in gss_krig_predict_global.  The right-hand-side workspace holds nz
 *   blocks, so a chunk is 1 / nz of that call's; the environment variable GSS_COKRIG_CHUNK_POINTS caps the points per
 *   chunk (rounded down to a multiple of 256), for tests, like GSS_VARIO_CULL above: the results are the same.
 *   gss_profile_read names: "cokrig_rhs" (assembly), "krig_quadform" (the nz quadratic forms). */
int32_t gss_cokrig_create(gss_krig_t** out, const gss_variogram_t* structure, int32_t nz, const double* b0,
                          const double* b1, int32_t variant, const double* means, const double* xdata,
                          const double* z, const int32_t* var, int64_t n, int32_t flags, void* stream);
int32_t gss_cokrig_predict_global(gss_krig_t* h, const double* xdom, int64_t m, double* mean, double* variance,
                                  uint8_t* status, int32_t mem, void* stream);

/* gss_cokrig_predict_global_batch: the fitted system of gss_cokrig_create with new value vectors at the same stacked
 *   samples -- the counterpart of gss_krig_predict_global_batch, and the conditioning step of co-simulation
 *   (gss_fftgs_realize_lmc), where the data and every unconditional realisation are kriged from one set of locations.
 *   Means only: no variances, no status.
 *   zbatch     nbatch x n, one value per stacked sample in the caller's row order (the order of gss_cokrig_create's
 *              arrays); it replaces the handle's own values.  nbatch <= 65535.
 *   mean_out   nbatch x nz x m: batch r, target t at (r * nz + t) * m -- the layout of gss_fftgs_realize_lmc's `out`,
 *              so that the two arrays combine elementwise.
 *   xdom, mem, stream   as gss_cokrig_predict_global (a rotated ball: the domain is moved into the frame of the
 *              samples); host arrays are staged whole.  xdom, zbatch and mean_out live in `mem`.
 *   Variants   GSS_KRIG_SIMPLE: the residuals z - means[var] are kriged and means[t] is added back.
 *              GSS_KRIG_ORDINARY: the constraint part of the dual weights supplies the e_t row of target t.
 *   Arithmetic WD = K^-1 [Z - means; 0] by two products with the factor (the block gss_krig_predict_global_batch runs),
 *              then mean(r, t, p) = sum_j C_{var_j t}(x_j, p) WD(j, r) + WD(n + t, r) | means[t] in ascending j, with rho
 *              evaluated once per (sample, point) for all value vectors and targets of a pass.  The zero-key rule is that
 *              of gss_cokrig_create: a domain point on a sample of variable t takes c0 = b0 + b1 there, and so reproduces
 *              the value given for that sample.  The result of a point does not depend on the chunk it falls into
 *              (GSS_COKRIG_CHUNK_POINTS applies) nor on the memory space of the arrays.
 *   Refusals   GSS_ERR_INVALID, the message names the entry: a single-variable handle (gss_krig_create), a handle of
 *              gss_cokrig_create_local (no factor), negative sizes, a NULL array with non-zero sizes.  m == 0 or
 *              nbatch == 0: GSS_OK, nothing is read or written.  gss_krig_predict_global_batch keeps refusing cokriging
 *              handles.  gss_profile_read name: "cokrig_batch" (the mean kernel). */
int32_t gss_cokrig_predict_global_batch(gss_krig_t* h, const double* xdom, int64_t m, const double* zbatch,
                                        int64_t nbatch, double* mean_out, int32_t mem, void* stream);

/* ---- moving-neighbourhood cokriging: per-variable search, one small system per domain point.
 *
 * gss_cokrig_create_local: a cokriging handle without a system and without a factor, for gss_cokrig_predict_knn and
 *   gss_cokrig_cv_knn (a sparse primary variable beside a dense secondary one: sample counts beyond what the O(n^3)
 *   fit of gss_cokrig_create and its n^2 factor allow).  Arguments, checks, frame, coefficient table and row order are those
 *   of gss_cokrig_create, with one difference: nz is 1 .. 4 here; 5 .. 8 -> GSS_ERR_UNSUPPORTED (the right-hand sides
 *   of a point -- nz covariance columns, one data column, nz indicator columns -- ride along in one 16-column tile
 *   whose per-wave storage holds twelve).  gss_krig_info (n stacked samples, nc) and gss_krig_destroy apply.  Every
 *   entry point that needs a factor (gss_cokrig_predict_global, gss_krig_cv_global, gss_krig_cv_global_folds) refuses
 *   the handle with GSS_ERR_INVALID, as it refuses a GSS_KRIG_NO_FACTOR handle.  Both creators keep a copy of the
 *   samples grouped by variable on the device, with the map back to the caller's rows, so that each variable is
 *   searched on its own.
 *
 * gss_cokrig_predict_knn: every target variable at every domain point from a per-variable moving neighbourhood; on
 *   handles of either creator (nz <= 4; more -> GSS_ERR_UNSUPPORTED).
 *   Neighbourhood  for every domain point the k[a] nearest samples of variable a, each variable searched separately
 *              among its own samples (one joint search would let a dense secondary variable crowd the primary out).
 *              k: nz counts, 1 <= k[a] <= the sample count of variable a (GSS_ERR_INVALID otherwise; a front-end
 *              clamps); sum k[a] <= 64, more -> GSS_ERR_UNSUPPORTED.  radius / inv_radii / metric / metric_param:
 *              the ball, the metric and the order by ascending (key, index) of gss_knn_search, the index being the
 *              caller's row; the same ball applies to every variable.
 *   Outputs    mean and variance: nz columns of m (column t at + t * m); status: nz x m bytes (may be NULL).  idx_out:
 *              m x sum k, rows of the caller's arrays; variable a occupies columns off[a] .. off[a] + k[a] - 1 with
 *              off[a] = k[0] + .. + k[a - 1], nearest first, -1 beyond the number found.  count_out: m x nz, the
 *              number found per variable.  idx_out and count_out may be NULL.  `mem` as gss_krig_predict_knn.
 *   Per point  with c_a neighbours found of variable a and K = sum c_a:
 *              K < max(minneighbors, 1): every target GSS_PT_MISSING, mean = variance = NaN.
 *              GSS_KRIG_ORDINARY: the unbiasedness constraint of a variable with c_a = 0 is dropped (it is not
 *              reported as singular); a target t with c_t = 0 has no unbiased estimator and gets GSS_PT_MISSING and
 *              NaN, the other targets are estimated.  GSS_KRIG_SIMPLE: every target is estimated from whatever was
 *              found.  A non-positive pivot in the covariance block of the K neighbours, or in the constraint block
 *              of the present variables: GSS_PT_SINGULAR and NaN for all targets.
 *              variance_t = b0[t][t] + b1[t][t] - q_t + r_t' S^-1 r_t, clamped at 0 (q_t: the quadratic form of the
 *              covariance block, S and r_t: the Schur complement and residual of the constraints; S is absent under
 *              the simple variant).  The zero-key rule and the symmetrised coefficient table are those of
 *              gss_cokrig_create: collocated samples of two variables meet through the cross nugget inside the
 *              neighbourhood, and a domain point on a sample of variable t reproduces that datum.
 *   Not here   block support and the drift variants (refused by the creators and by gss_krig_set_block_support);
 *              gss_krig_predict_knn and gss_krig_cv_knn keep refusing cokriging handles (cross-validation under the
 *              moving neighbourhood: gss_cokrig_cv_knn, below).
 *   Chunks     the domain is walked in chunks of 2^20 points (131 072 for host arrays, which travel piece by piece);
 *              GSS_COKRIG_CHUNK_POINTS caps them as it caps gss_cokrig_predict_global's, for tests: the results are the
 *              same.  gss_profile_read names: "knn" (the nz searches), "cokrig_local" (the systems). */
int32_t gss_cokrig_create_local(gss_krig_t** out, const gss_variogram_t* structure, int32_t nz, const double* b0,
                                const double* b1, int32_t variant, const double* means, const double* xdata,
                                const double* z, const int32_t* var, int64_t n, void* stream);
int32_t gss_cokrig_predict_knn(gss_krig_t* h, const double* xdom, int64_t m, const int32_t* k, int32_t minneighbors,
                               double radius, const double* inv_radii, int32_t metric, double metric_param,
                               double* mean, double* variance, uint8_t* status, int32_t* idx_out, int32_t* count_out,
                               int32_t mem, void* stream);

/* ---- cross-validation: does the model predict the samples it was given?  ([DEP] GeoStatsBase `cverror` with
 *      LeaveOneOut / KFoldValidation / BlockValidation / LeaveBallOut; not in the reference tree.)  Every sample of the
 *      handle is predicted, at point support, from samples outside its own fold.  Handles with block support set are
 *      refused (GSS_ERR_INVALID).
 *
 * gss_krig_cv_global: leave-one-out under the global neighbourhood from the factor the handle already holds, no
 *   refit: with B = K^-1 = W'^T D W' (D = +1 on the n data rows, -1 on the nc constraint rows) and the dual weights
 *   wd = K^-1 [z - mean; 0], pred_i = z_i - wd_i / B_ii and var_i = max(0, 1 / B_ii) (Dubrule 1983), for simple,
 *   ordinary, universal and external-drift kriging alike.  B_ii is one fixed-order sum per column of W': the results are
 *   the same bits on every run.  B_ii <= 0 or not finite: GSS_PT_SINGULAR, pred = var = NaN.  Needs a factor
 *   (GSS_ERR_INVALID on a GSS_KRIG_NO_FACTOR handle that never adopted one); an asynchronous fit is waited for and its
 *   status (GSS_ERR_NOT_POSDEF) reported here.  pred, var (n doubles) and status (n bytes, may be NULL) live in `mem`.
 *
 * gss_krig_cv_global_folds: folds under the global neighbourhood, from the same factor and again without a refit.
 *   fold: n ids >= 0 in `mem`, arbitrary and not necessarily compact; equal ids form a fold (a negative id:
 *   GSS_ERR_INVALID; the ids are grouped on the host, device ids are copied there, which waits for the stream).  Every
 *   sample is predicted from all samples outside its own fold F by the block form of the identity above:
 *   z_F - pred_F = (B_FF)^-1 wd_F and var_F = diag((B_FF)^-1), where B_FF = W'[:, F]^T D W'[:, F] is a signed Gram
 *   product of the gathered columns of W' (FP64 MFMA), factorised per fold as L L^T -- in LDS, one workgroup per fold,
 *   for folds of up to 128 samples; larger folds one after the other on the factor-and-inverse routine of the fit.
 *   The constraint rows enter through D alone, so simple, ordinary, universal and external-drift kriging share one
 *   path.  fold == NULL is gss_krig_cv_global, bit for bit.  A fold whose remainder cannot determine the system,
 *   n - |F| < max(1, nc), is decided from the sizes (simple kriging is exempt: an empty remainder predicts the mean
 *   with variance C(0)); a fold whose Cholesky meets a non-positive or non-finite pivot is singular.  In both cases
 *   every sample of the fold gets GSS_PT_SINGULAR and pred = var = NaN, and the other folds are unaffected.  Limit: a
 *   remainder that passes the count but is geometrically degenerate (say, collinear samples under a planar drift) is
 *   caught by the pivot test only, and rounding may let a pivot that is zero in exact arithmetic pass as a tiny
 *   positive one.  No floating-point atomics, every sum in a fixed order: the same bits on every run.  Refusals and
 *   the asynchronous fit as gss_krig_cv_global.  pred, var, status (may be NULL) live in `mem`; the call returns when
 *   they are complete.
 *
 * gss_krig_cv_knn: moving neighbourhood.  Sample p is predicted from its k nearest samples j that satisfy
 *   fold[j] != fold[p] and, when exclude_radius >= 0, search distance(p, j) > exclude_radius (leave-ball-out: a sample
 *   exactly on the radius is left out), besides what gss_krig_predict_knn requires (the ball radius / inv_radii, the
 *   order by (key, index)).  fold: n ids >= 0 in `mem` (a negative id: GSS_ERR_INVALID; ids in device memory are copied
 *   to the host for that check, which waits for the stream); NULL: leave-one-out.  Coordinates duplicated across folds
 *   are ordinary zero-distance neighbours.  k in 1 .. n - 1; minneighbors, radius, inv_radii, metric, metric_param as
 *   gss_krig_predict_knn; GSS_METRIC_HAVERSINE has no indexed search: GSS_ERR_UNSUPPORTED.  Fewer than minneighbors
 *   eligible samples: GSS_PT_MISSING, pred = var = NaN.  External drifts at the queries are the handle's own rows.
 *   Works on GSS_KRIG_NO_FACTOR handles.  pred, var, status, idx_out (n x k) / count_out (may be NULL) live in `mem`.
 *   A cokriging handle is refused (GSS_ERR_INVALID); its moving-neighbourhood cross-validation is gss_cokrig_cv_knn.
 *
 * gss_cokrig_cv_knn: moving-neighbourhood cross-validation of a cokriging handle of either creator (gss_cokrig_create,
 *   gss_cokrig_create_local; nz <= 4, more -> GSS_ERR_UNSUPPORTED; a handle that is no cokriging system:
 *   GSS_ERR_INVALID) -- the conventions of gss_krig_cv_knn and gss_cokrig_predict_knn put together, without the O(n^3)
 *   fit and the n^2 factor the global identities need.
 *   Per sample  stacked sample p (variable v_p, caller's row p) is predicted as target v_p at its own location from,
 *              for every variable a, the k[a] nearest samples j of variable a with fold[j] != fold[p] and, when
 *              exclude_radius >= 0, search distance(p, j) > exclude_radius (a sample exactly on the radius is left
 *              out).  Each variable is searched separately among its own samples, in ascending (key, caller's row).
 *   fold       n ids >= 0 in `mem` (a negative id: GSS_ERR_INVALID; ids in device memory are copied to the host for
 *              that check, which waits for the stream).  NULL: every stacked sample is its own fold, leave one DATUM
 *              out -- collocated samples of other variables stay in play and a sample never sees itself.  A caller
 *              removes a whole location by giving its collocated samples one id, the convention of gss_cokrig_create
 *              for gss_krig_cv_global_folds.  exclude_radius NaN: GSS_ERR_INVALID.
 *   k          nz counts, 1 <= k[a] <= the sample count of variable a (GSS_ERR_INVALID otherwise), sum k[a] <= 64
 *              (more -> GSS_ERR_UNSUPPORTED); fewer eligible samples than k[a] give a shorter list.  minneighbors,
 *              radius, inv_radii, metric, metric_param as gss_cokrig_predict_knn; GSS_METRIC_HAVERSINE has no indexed
 *              search, which the fold search needs: GSS_ERR_UNSUPPORTED.
 *   Outcome    with c_a neighbours found of variable a and K = sum c_a: K < max(minneighbors, 1): GSS_PT_MISSING.
 *              GSS_KRIG_ORDINARY: c_{v_p} = 0 leaves no unbiased estimator, GSS_PT_MISSING; the constraint of any other
 *              variable with c_a = 0 is dropped.  A non-positive pivot: GSS_PT_SINGULAR.  In all of those
 *              pred = var = NaN.  The variance formula, its clamp at 0, the zero-key rule and the symmetrised
 *              coefficient table are those of gss_cokrig_predict_knn: a collocated sample of another variable that is
 *              still eligible enters the right-hand side through the cross nugget c0[v_j][v_p], and a duplicate
 *              coordinate of the same variable in another fold reproduces that datum.
 *   Outputs    pred, var: n doubles; status: n bytes, may be NULL; idx_out: n x sum k laid out as in
 *              gss_cokrig_predict_knn (caller's rows, -1 beyond the number found); count_out: n x nz; both may be NULL.
 *              Everything is indexed by the caller's row and lives in `mem`, as for gss_krig_cv_knn.
 *   The system of a sample carries one target, so its right-hand sides are [c0_{v_p} | z - means | indicators], at most
 *   nz + 2 columns where gss_cokrig_predict_knn carries 2 nz + 1.  No atomics, every sum in a fixed order: the same
 *   bits on every run.  GSS_COKRIG_CHUNK_POINTS caps the samples per chunk as it caps the points of
 *   gss_cokrig_predict_knn, for tests: the results are the same.  gss_profile_read names: "knn" (the nz fold searches
 *   of every chunk), "cokrig_cv" (the systems).
 *
 * gss_cv_summary: one deterministic reduction (per-workgroup partial sums in a fixed order, then one workgroup; no
 *   floating-point atomics: the same bits on every run) over e_i = z_i - pred_i.
 *   Over the points with GSS_PT_OK: n_ok, me = mean e, mae = mean |e|, mse = mean e^2.  Over those with var > 0
 *   (mse_std_n of them): mean_std = mean e / sigma, msq_std = mean e^2 / sigma^2.  n_missing, n_singular: counts.
 *   cverror: the mean over the non-empty folds of the fold's mean squared error (the default squared loss of the
 *   GeoStats family); fold == NULL (leave-one-out): the mse.  fold: n ids in 0 .. nfolds - 1; fold_mse (nfolds doubles
 *   in `mem`, or NULL) receives the per-fold mean squared errors, NaN for a fold without an OK point.  Means over an
 *   empty set are NaN.  One wave per fold reads all n ids: meant for tens to thousands of folds.
 *   z, pred, var, status (NULL: all OK), fold, fold_mse live in `mem`; `out` is host memory and the call returns when it
 *   is filled. */
int32_t gss_krig_cv_global(gss_krig_t* h, double* pred, double* var, uint8_t* status, int32_t mem, void* stream);
int32_t gss_krig_cv_global_folds(gss_krig_t* h, const int32_t* fold, double* pred, double* var, uint8_t* status,
                                 int32_t mem, void* stream);
int32_t gss_krig_cv_knn(gss_krig_t* h, const int32_t* fold, double exclude_radius, int32_t k, int32_t minneighbors,
                        double radius, const double* inv_radii, int32_t metric, double metric_param,
                        double* pred, double* var, uint8_t* status, int32_t* idx_out, int32_t* count_out,
                        int32_t mem, void* stream);
int32_t gss_cokrig_cv_knn(gss_krig_t* h, const int32_t* fold, double exclude_radius, const int32_t* k,
                          int32_t minneighbors, double radius, const double* inv_radii, int32_t metric,
                          double metric_param, double* pred, double* var, uint8_t* status, int32_t* idx_out,
                          int32_t* count_out, int32_t mem, void* stream);
typedef struct gss_cv_summary {
  double n_ok, n_missing, n_singular, me, mae, mse, mse_std_n, mean_std, msq_std, cverror;
} gss_cv_summary_t;
int32_t gss_cv_summary(const double* z, const double* pred, const double* var, const uint8_t* status,
                       const int32_t* fold, int64_t n, int32_t nfolds, gss_cv_summary_t* out, double* fold_mse,
                       int32_t mem, void* stream);

/* ---- IDWSolver / LWRSolver on the neighbour-search kernel -------------
 * gss_idw_predict replaces the estimation loop idw.jl:111-142: neighbours by gss_knn_search's rule,
 *   w_i = 1 / d_i^exponent, mean = sum w_i z_i / sum w_i, dist = min d_i; a zero distance copies that
 *   sample and reports dist = 0 (idw.jl:131-134).  Output column `dist` is `<var>_distance` (idw.jl:149).
 * gss_lwr_predict replaces lwr.jl:114-147: delta_i = d_i / max d, W = diag(weight(delta_i)),
 *   theta = (X'WX)^-1 X'Wz with X = [1 x], mean = theta . [1; x0], var = |W X (X'WX)^-1 [1; x0]|
 *   (stored under `<var>_variance` exactly as lwr.jl:145,154 does).
 *   weight(h) = exp(-weight_a * h^weight_p) for GSS_WEIGHT_EXP (reference default a = 3, p = 2,
 *   lwr.jl:58) or (1 - h^3)^3 for GSS_WEIGHT_TRICUBE.
 * k = number of neighbours the searcher returns (ui.jl:16-23): 1..n; k == n is `maxneighbors = nothing` (every
 * sample, no search); beyond 64 the search runs in passes of 64 (haversine: on the exhaustive kernel).  radius / inv_radii /
 * metric as gss_knn_search;
 * the weights use the distances of that metric (searchdists!, idw.jl:120).
 * status: GSS_PT_MISSING when fewer than minneighbors were found (idw.jl:123, lwr.jl:126),
 * GSS_PT_SINGULAR when the LWR normal equations are not positive definite (the reference throws).
 * xdata n x d and xdom m x d point-major; status may be NULL. */
enum { GSS_WEIGHT_EXP = 0, GSS_WEIGHT_TRICUBE = 1 };

int32_t gss_idw_predict(const double* xdata, const double* z, int64_t n, int32_t dim, const double* xdom,
                        int64_t m, int32_t k, int32_t minneighbors, double radius, const double* inv_radii,
                        int32_t metric, double metric_param, double exponent, double* mean, double* dist,
                        uint8_t* status, int32_t mem, void* stream);
int32_t gss_lwr_predict(const double* xdata, const double* z, int64_t n, int32_t dim, const double* xdom,
                        int64_t m, int32_t k, int32_t minneighbors, double radius, const double* inv_radii,
                        int32_t metric, double metric_param, int32_t weight_kind, double weight_a,
                        double weight_p, double* mean, double* var, uint8_t* status, int32_t mem, void* stream);
/* Several value columns on ONE search and ONE weight vector per point.  The reference's estimation loop is generic over
 * the value type (idw.jl:128-141: `mu = sum(ws[i] * vs[i])`, exercised with CoDa compositions in
 * test/estimation/idw.jl:47-65, whose arithmetic is linear in the log-parts) and several variables measured on the same
 * samples share everything but the values.  z: nz columns of n (column c at z + c * n); mean: nz columns of m (column c
 * at mean + c * m); dist / var / status: one per point, as in the single-column calls (which are these with nz = 1). */
int32_t gss_idw_predict_cols(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz,
                             const double* xdom, int64_t m, int32_t k, int32_t minneighbors, double radius,
                             const double* inv_radii, int32_t metric, double metric_param, double exponent,
                             double* mean, double* dist, uint8_t* status, int32_t mem, void* stream);
int32_t gss_lwr_predict_cols(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz,
                             const double* xdom, int64_t m, int32_t k, int32_t minneighbors, double radius,
                             const double* inv_radii, int32_t metric, double metric_param, int32_t weight_kind,
                             double weight_a, double weight_p, double* mean, double* var, uint8_t* status,
                             int32_t mem, void* stream);
/* LWR with the neighbours' weights supplied by the caller, for weight functions that cannot cross the ABI -- an arbitrary
 * `weightfun` closure (lwr.jl:58,136): the host searches (gss_knn_search), evaluates delta = d / max d and w = f(delta)
 * itself and hands over idx (m x k, 0-based, as the search wrote it), count (m) and weights (m x k); the rest of
 * lwr.jl:137-145 (normal equations about the estimation point, norm(r)) runs here.  The lists are the caller's: a count
 * above k is clamped and a point whose list holds an index outside 0 .. n-1 is reported GSS_PT_SINGULAR, never gathered. */
int32_t gss_lwr_predict_weights(const double* xdata, const double* z, int64_t n, int32_t dim, const double* xdom, int64_t m,
                                int32_t k, int32_t minneighbors, const int32_t* idx, const int32_t* count,
                                const double* weights, double* mean, double* var, uint8_t* status, int32_t mem,
                                void* stream);

/* ---- cross-validation of IDWSolver / LWRSolver: every sample predicted at its own location from samples outside its
 *      own fold, by the estimators above.  No model is fitted, so there is no handle: the samples are the call's.
 *   Eligibility  sample p is predicted from the samples j with fold[j] != fold[p] and, when exclude_radius >= 0, search
 *              distance(p, j) > exclude_radius (leave-ball-out: a sample exactly on the radius is left out; the radius
 *              is compared in the search key, as in gss_krig_cv_knn).  fold: n ids >= 0 in `mem`, arbitrary and not
 *              necessarily compact (a negative id: GSS_ERR_INVALID; ids in device memory are copied to the host for
 *              that check, which waits for the stream); NULL: leave-one-out, a sample's fold is its own index.
 *              exclude_radius NaN: GSS_ERR_INVALID.  n >= 2.
 *   Columns    z: nz columns of n values (column c at z + c * n), pred: nz columns of n (column c at pred + c * n); one
 *              search and one weight vector per sample, dist / var / status one per sample, as in the _cols calls.
 *   Zero distances  a coordinate duplicated in another fold is an ordinary zero-distance neighbour: IDW copies the first
 *              such sample and reports dist = 0 (idw.jl:131-134).  A duplicate inside the sample's own fold is invisible
 *              and does not trigger that rule.
 *   Outcome    fewer eligible neighbours than max(minneighbors, 1): GSS_PT_MISSING, pred = dist / var = NaN -- a fold that
 *              holds every sample makes all of them missing.  LWR normal equations that are not positive definite:
 *              GSS_PT_SINGULAR, as in gss_lwr_predict.
 *   1 <= k <= n - 1  the search path: the k nearest eligible samples by the fold-aware search of gss_krig_cv_knn (order
 *              by (key, index); beyond 64 in passes of 64), then the list estimators of gss_idw_predict /
 *              gss_lwr_predict with the samples as estimation points -- the same kernels, lists and order of summation
 *              as a prediction from the eligible samples alone.  GSS_METRIC_HAVERSINE has no indexed search, which the
 *              fold search needs: GSS_ERR_UNSUPPORTED.  idx_out (n x k, -1 beyond the count) and count_out (n) may be
 *              NULL.
 *   k == n     every eligible sample (inside the neighbourhood ball, if one is given): no search, a self-join of the
 *              samples.  Thread = sample p; the samples pass by in pieces of 1 024 staged through LDS with their fold
 *              ids beside them, and a sample contributes only if it is eligible by fold, exclusion key and ball.  IDW
 *              completes in one sweep (sums, nearest eligible distance, first eligible zero distance); LWR takes two
 *              (farthest eligible sample, then the moments X'WX, X'W^2X, X'Wz), the mask applied identically in both.
 *              All four metrics, haversine included, with or without a ball.  The reference's default IDW (Euclidean, no
 *              ball, no exclusion radius, exponent 1 or 2, one column) runs on a dedicated kernel: the sample index is
 *              wave-uniform, so coordinates, value and fold id arrive through the scalar cache as scalar operands; the
 *              weight of an ineligible sample is selected to zero (never multiplied: the sample itself has d^2 = 0) and
 *              its d^2 is kept out of the running minimum; a coincident eligible sample is found by a rescan under the
 *              same test.  With an exclusion radius the general kernel runs, whose key is the search's own (no FMA).
 *              idx_out / count_out must be NULL (GSS_ERR_INVALID otherwise).  k outside 1 .. n: GSS_ERR_INVALID.
 *   minneighbors, radius, inv_radii, metric, metric_param, exponent, weight_* as gss_idw_predict / gss_lwr_predict.
 *   No floating-point atomics and every sum in a fixed order: the same bits on every run.  The samples are served in
 *   chunks (2^20 per chunk on the search path up to 64 neighbours, as in the prediction calls); the environment
 *   variable GSS_EST_CV_CHUNK caps the samples per chunk on every path, for tests, like GSS_COKRIG_CHUNK_POINTS: the
 *   results are the same.  pred, dist / var, status (may be NULL), idx_out, count_out live in `mem`; the call returns
 *   when they are complete.  gss_profile_read names: "knn" (the fold searches), "idw_cv" / "lwr_cv" (the estimator,
 *   on either path).  The errors are summarised by gss_cv_summary with a zero variance column: neither estimator has a
 *   prediction variance (dist is a distance, var the norm of lwr.jl:145). */
int32_t gss_idw_cv(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz, const int32_t* fold,
                   double exclude_radius, int32_t k, int32_t minneighbors, double radius, const double* inv_radii,
                   int32_t metric, double metric_param, double exponent, double* pred, double* dist, uint8_t* status,
                   int32_t* idx_out, int32_t* count_out, int32_t mem, void* stream);
int32_t gss_lwr_cv(const double* xdata, const double* z, int64_t n, int32_t dim, int32_t nz, const int32_t* fold,
                   double exclude_radius, int32_t k, int32_t minneighbors, double radius, const double* inv_radii,
                   int32_t metric, double metric_param, int32_t weight_kind, double weight_a, double weight_p,
                   double* pred, double* var, uint8_t* status, int32_t* idx_out, int32_t* count_out, int32_t mem,
                   void* stream);

/* ---- FFTGS ------------------------------------------------------------------------------
 * gss_fftgs_create replaces preprocess fft.jl:62-103 (unconditional part): covariance to the
 * centre cell, F = sqrt(|fft(fftshift(C))|), F[1] = 0.  dims[0] is the fastest axis (Julia
 * column-major), ndim in 1..3.
 */
enum { GSS_FFTGS_NO_SPECTRUM = 1 /* the spectrum arrives by broadcast: allocate the state, compute nothing */ };
int32_t gss_fftgs_create(gss_fftgs_t** out, const gss_variogram_t* vg, int32_t ndim, const int64_t* dims,
                         const double* spacing, double mean, int32_t flags, void* stream);
int32_t gss_fftgs_destroy(gss_fftgs_t* h);
/* full-size spectral amplitude F (prod(dims) doubles, element order) for parity checks */
int32_t gss_fftgs_spectrum(gss_fftgs_t* h, double* f_out, int32_t mem, void* stream);
/* device address + size of the state (rescaled half-spectrum amplitude, then sum F^2 and the rescale factor) so that
 * rank 0's preprocess (fft.jl:62-103, run once) can be broadcast to the peer GPUs over RCCL, which then realise their
 * share (fft.jl:145); after a broadcast into a handle created with GSS_FFTGS_NO_SPECTRUM call gss_fftgs_adopt_state. */
int32_t gss_fftgs_state_buffer(gss_fftgs_t* h, void** dev_ptr, int64_t* bytes);
int32_t gss_fftgs_adopt_state(gss_fftgs_t* h, void* stream);
/* replaces solvesingle fft.jl:145-173 for realisations first_real .. first_real+nreals-1.
 * noise == NULL: Philox4x32-10 uniform noise keyed by (seed, realisation) generated on device;
 * else noise is nreals x N uniform values supplied by the caller (parity-test mode).
 * inds (ninds int64, 0-based parent indices, may be NULL) gathers a grid view (fft.jl:152,173).
 * out is nreals x (ninds or N). */
int32_t gss_fftgs_realize(gss_fftgs_t* h, uint64_t seed, int64_t first_real, int64_t nreals,
                          const double* noise, const int64_t* inds, int64_t ninds, double* out,
                          int32_t mem, void* stream);

/* ---- FFTGS co-simulation under a linear model of coregionalisation ------------------------
 * nz variables (1 .. 8) with the conventions of gss_cokrig_create: C_ab(h) = b1[a][b] rho(h) for h != 0 and
 * C_ab(0) = b0[a][b] + b1[a][b], rho = `structure` with sill 1 and nugget 0 (only kind, dim, range, nu, aniso,
 * inv_radii and rotation are read; nextra must be 0, GSS_VG_POWER gives GSS_ERR_UNSUPPORTED, Gaussian is the bare
 * formula: a front end adds its 1e-6 to the diagonal of b0).  b0, b1: nz x nz row-major, symmetric to 1e-12 of the
 * largest absolute entry, finite, b0[a][a] + b1[a][a] > 0; means: nz doubles.  A realisation is
 *     Z_a = means[a] + sum_j L1[a][j] Y_j + sum_j L0[a][j] E_j ,   a = 0 .. nz-1,
 * with Y_j independent unconditional FFTGS fields of rho (what a gss_fftgs_create handle with sill 1, nugget 0 and
 * mean 0 realises), E_j independent standard-normal white noise, and L0 / L1 the lower factors of (b0 + b0^T) / 2 and
 * (b1 + b1^T) / 2.  The nugget is explicit Gaussian white noise here, not a floor in the spectrum: the marginal of
 * the nugget part is exactly normal and independent from cell to cell, where a plain handle with a nugget shapes one
 * uniform-phase field by spectrum + nugget.
 *   Factors: left-looking Cholesky without pivoting, on the host, the same on every rank.  With d the largest
 * diagonal entry, a pivot <= 1e-12 d makes its column a zero column (what remains of the column must then be
 * <= 1e-12 d in magnitude too); otherwise, and for a pivot below -1e-12 d, the matrix is not positive semidefinite:
 * GSS_ERR_INVALID, the message names the matrix and the entry.  A zero column costs nothing afterwards -- no
 * transform, no noise stream --, so a rank-1 b1 (intrinsic correlation) costs one field per realisation whatever nz.
 *   The handle is a gss_fftgs_t whose spectrum is that of rho with unit sill: gss_fftgs_destroy, _spectrum,
 * _state_buffer and _adopt_state apply unchanged, GSS_FFTGS_NO_SPECTRUM is accepted (the factors are recomputed from
 * the arguments on every rank).  gss_fftgs_realize refuses such a handle, gss_fftgs_realize_lmc a plain one.
 *   Stream numbering: Y_j of realisation r is what gss_fftgs_realize(plain unit handle, seed, first_real = r nz + j,
 * nreals = 1) returns; E_j of realisation r is gss_philox_normal(seed ^ GSS_FFTGS_LMC_NUGGET_SALT, r nz + j, N).
 * Numbers depend on (seed, r, j) only: sharding the realisations over ranks or splitting a call changes nothing.
 *   out: nreals x nz x (ninds or N); variable a of realisation r (counted from first_real) at ((r nz) + a) npts.
 * inds gathers a grid view as in gss_fftgs_realize.  noise (may be NULL): nreals x nz x N uniforms, slot j feeds Y_j
 * (parity mode of gss_fftgs_realize); nugget_noise (may be NULL, independently): nreals x nz x N normals, slot j is
 * E_j.  Slots of zero columns are not read.  `mem` says where noise, nugget_noise, inds and out live.  A device `out`
 * without inds receives the fields in the slots of their realisation and is mixed in place (8 N (live fields + nz)
 * bytes of traffic per realisation, no workspace); a grid view goes through a workspace and a host `out` through the
 * ring of gss_fftgs_realize, chunk by chunk -- the environment variable GSS_FFTGS_LMC_CHUNK_REALS caps the
 * realisations per chunk, for tests, like GSS_COKRIG_CHUNK_POINTS: the results are the same bits. */
#define GSS_FFTGS_LMC_NUGGET_SALT 0x6e75676765744c4dULL /* "nuggetLM" */
int32_t gss_fftgs_create_lmc(gss_fftgs_t** out, const gss_variogram_t* structure, int32_t nz, const double* b0,
                             const double* b1, const double* means, int32_t ndim, const int64_t* dims,
                             const double* spacing, int32_t flags, void* stream);
int32_t gss_fftgs_realize_lmc(gss_fftgs_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                              const double* nugget_noise, const int64_t* inds, int64_t ninds, double* out, int32_t mem,
                              void* stream);

/* ---- LUGS -------------------------------------------------------------------------------
 * gss_lugs_create replaces preprocess lu.jl:105-147 for one variable: covariance blocks,
 * L11, B12 = L11 \ C12, d2, L22 = chol(C22 - B12'B12).  centroids N x d point-major;
 * dlocs nd sorted 0-based data locations with values z1 (after initbuff, lu.jl:86,113-114).
 */
enum {
  GSS_LUGS_NO_FACTOR = 1, /* L22 / d2 arrive by broadcast (lu.jl:76 runs on one rank): allocate, do not factorise */
  GSS_LUGS_FACT_LU = 2    /* solver parameter `factorization = lu` (lu.jl:70,107): L11 and L22 are the unit lower
                           * factors `lu(Symmetric(.)).L` of a partial-pivot LU, exactly as the reference takes them
                           * (they are not square roots of the covariance); default is `cholesky` */
};
int32_t gss_lugs_create(gss_lugs_t** out, const gss_variogram_t* vg, const double* centroids, int64_t N,
                        const int64_t* dlocs, const double* z1, int64_t nd, double mean, int32_t flags,
                        void* stream);
int32_t gss_lugs_destroy(gss_lugs_t* h);
int32_t gss_lugs_info(const gss_lugs_t* h, int64_t* ns, int64_t* nd);
/* copy out L22 (ns x ns, column-major, lower) and d2 (ns) for parity checks; either may be NULL */
int32_t gss_lugs_factor(gss_lugs_t* h, double* l22, double* d2, int32_t mem, void* stream);
/* device address + size of the state (L22 then d2) for the RCCL broadcast of SURVEY.md section 8e: rank 0 runs the
 * preprocess, the peers create their handle with GSS_LUGS_NO_FACTOR, receive the state and call gss_lugs_adopt_state. */
int32_t gss_lugs_state_buffer(gss_lugs_t* h, void** dev_ptr, int64_t* bytes);
int32_t gss_lugs_adopt_state(gss_lugs_t* h);
/* replaces solvesingle / lusim lu.jl:171-224: y2 = d2 + L22 * w  (w = rho*w1 + sqrt(1-rho^2)*w2
 * when w1 != NULL), scatter to dlocs/slocs, add mean when unconditional.
 * noise == NULL: w2 = Philox normals keyed by (seed, realisation); else nreals x ns supplied.
 * out nreals x N; w_out (nreals x ns, may be NULL) returns the w2 used (for co-simulation). */
int32_t gss_lugs_realize(gss_lugs_t* h, uint64_t seed, int64_t first_real, int64_t nreals,
                         const double* noise, double rho, const double* w1, double* out, double* w_out,
                         int32_t mem, void* stream);

/* ---- SPDEGS (spde.jl:29-115; Lindgren et al. 2011) -------------------------------------------
 * Gaussian simulation on a triangle mesh.  The reference forms the dense precision Q = A'A / tau^2 with
 * A = kappa^2 I - inv(M) B, factorises it and draws z = L w with L L' = inv(Q) (spde.jl:60-68, 98-99).  The same
 * distribution is z = tau inv(A) w, i.e. one sparse symmetric positive definite solve per realisation,
 *     (kappa^2 M - B) z = tau M w,
 * which is what this handle does: S = kappa^2 M - B is assembled once in CSR and every block of realisations is one
 * Jacobi-preconditioned conjugate-gradient run over interleaved columns ("SPDEGS").
 *
 * Operators ([DEP] Meshes.jl `laplacematrix` / `measurematrix`, written out).  For a triangle (a, b, c) with area
 * T > 0 (in 3-D half the norm of the cross product) the angle at c is opposite the edge (a, b) and
 * cot_c = ((a - c) . (b - c)) / (2 T).  The triangle adds +cot_c / 2 to B[a][b] and B[b][a], -cot_c / 2 to B[a][a] and
 * B[b][b], and T / 3 to the lumped mass M[a][a]; cyclically for the other two corners.  kappa = 1 / range; with the
 * parameter dimension d = 2 of a surface and alpha = 2, nu = alpha - d / 2 = 1 and
 * tau^2 = sill^2 kappa^(2 nu) (4 pi)^(d/2) Gamma(alpha) / Gamma(nu) = 4 pi sill^2 kappa^2.  The reference squares
 * `sill` (spde.jl:50, 63) and so does the library: the parameter acts as a standard deviation.
 *
 * Noise.  GSS_SPDE_NOISE_REFERENCE is the reference's w ~ N(0, I) (right-hand side tau M w), whose vertex variance
 * scales with the vertex area; GSS_SPDE_NOISE_LUMPED is Lindgren's lumped discretisation Q = A' M A / tau^2, i.e.
 * w ~ N(0, inv(M)) (right-hand side tau M^(1/2) w with w ~ N(0, I)), whose variance does not.
 *
 * Refusals, before any other device work (host arrays are checked on the host, device arrays on the device).
 * GSS_ERR_INVALID: a coordinate that is not finite, sill <= 0 or range <= 0 (spde.jl:53-54), an index outside
 * [0, nv), a triangle with a repeated vertex or without area, a vertex that belongs to no triangle (M singular: the
 * reference's inv(M) fails there too), nv < 3 or nt < 1.  GSS_ERR_UNSUPPORTED: dim outside {2, 3}, nv >= 2^31 - 1,
 * 12 nt >= 2^31 (the assembly sorts 12 contributions per triangle with 32-bit positions).
 * The assembly uses no floating-point atomics: the twelve contributions of every triangle are sorted by (row, column)
 * with a stable radix sort and summed in triangle order, so equal inputs give equal bits.
 */
enum { GSS_SPDE_NOISE_REFERENCE = 0,   /* b = tau M w       (spde.jl:98-99, w ~ N(0, I))        */
       GSS_SPDE_NOISE_LUMPED    = 1 }; /* b = tau M^(1/2) w (Lindgren 2011: Q = A' M A / tau^2) */
int32_t gss_spde_create(gss_spde_t** out, const double* vertices, int64_t nv, int32_t dim /* 2 or 3 */,
                        const int64_t* triangles, int64_t nt /* nt x 3, 0-based */,
                        double sill, double range, int32_t flags, int32_t mem, void* stream);
int32_t gss_spde_destroy(gss_spde_t* h);
int32_t gss_spde_info(const gss_spde_t* h, int64_t* nv, int64_t* nt, int64_t* nnz, double* tau2);
/* parity: CSR of S = kappa^2 M - B (rowptr nv+1, col nnz, val nnz; columns ascending within a row) and diag(M);
 * any of the four may be NULL */
int32_t gss_spde_operator(gss_spde_t* h, int64_t* rowptr, int32_t* col, double* val, double* mass,
                          int32_t mem, void* stream);
/* realisations first_real .. first_real+nreals-1.  noise == NULL: w = gss_philox_normal(seed, r, nv); else
 * nreals x nv normals supplied (parity mode).  vout (nreals x nv, may be NULL): vertex values z.  eout (nreals x nt,
 * may be NULL): element values, the mean of the three vertex values (spde.jl:108-109, `integrate` of the piecewise
 * linear field divided by the element's area).  At least one of the two outputs.
 * rtol <= 0: 1e-10; maxiter <= 0: 20 000.  A column stops (and its solution is no longer touched) once its recursive
 * residual satisfies ||r|| <= rtol ||b||; a column that reaches maxiter makes the call return GSS_ERR_NO_CONVERGENCE
 * after every output has been written, the message names the first such realisation and its residual.
 * Realisation r depends on (seed, r) and the mesh only: splitting a call, another first_real or other companions in
 * the block give the same bits.  Profile scopes: "spde_assemble", "spde_cg". */
int32_t gss_spde_realize(gss_spde_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                         double rtol, int64_t maxiter, double* vout, double* eout, int32_t mem, void* stream);
/* after a realize: largest iteration count of any column, largest final ||r||/||b||, columns that did not converge */
int32_t gss_spde_last_solve(const gss_spde_t* h, int64_t* iters, double* relres, int64_t* unconverged);

/* ---- SPDEGS with data: conditioning by kriging in the data space ("SPDEGS") ----
 * Not in the reference (spde.jl:30 refuses data).  With s = the right-hand-side scale of the handle (tau m or
 * tau sqrt(m)) the vertex field has the covariance Sigma = inv(S) diag(s^2) inv(S).  An observation i is a sparse row
 * of P (three vertices, three weights), a value y_i, an error variance r_i >= 0 and the known field mean mu.
 *   set-up      W = inv(S) P' (nd columns through the block CG), C = W' diag(s^2) W + diag(r) = P Sigma P' + R,
 *               C = L L' and inv(L)
 *   mean        mu + inv(S) (s^2 . (W inv(C) (y - mu)))                                      one solve
 *   realisation x_u = inv(S) (s . w_r), today's unconditional realisation of (seed, r), same bits;
 *               e_i = sqrt(r_i) n_(r,i);  lambda = inv(C) (y - mu - P x_u - e);
 *               x_c = (x_u + inv(S) (s^2 . (W lambda))) + mu                                 two solves
 * Only solves with S occur; r = 0 (exact data) is allowed and then P x_c = y up to the CG tolerance.
 *
 * gss_spde_locate: for np points (np x dim of the mesh) the triangle that contains each and its barycentric weights
 *   (np x 3, in the order of the triangle's vertices).  Brute force: every point against every triangle.  A triangle
 *   accepts a point whose barycentric coordinates (of its projection onto the triangle's plane when dim = 3) all lie in
 *   [-tol, 1 + tol]; among the accepting triangles the one nearest to the point wins (distance to the plane; a distance
 *   of at most tol edge lengths counts as zero, in 2-D every distance is zero), and among equally near ones the lowest
 *   index: a point on an edge or a vertex goes to the lowest triangle that shares it.  No triangle: index -1, weights 0.
 *   tol <= 0 selects 1e-9.
 * gss_spde_condition: attaches nd observations to the handle (replacing earlier ones).  obs_vertex nd x 3 (0-based),
 *   obs_weight nd x 3, value nd, error_var NULL (all zero) or nd values.  rtol / maxiter as gss_spde_realize, for the
 *   nd solves of W.  Refusals.  GSS_ERR_INVALID: nd < 1, an index outside [0, nv), a value, weight or variance that is
 *   not finite, a negative variance, a mean that is not finite.  GSS_ERR_NOT_POSDEF: C is singular to working precision
 *   (e.g. two exact observations with the same row); the message names the pivot.  GSS_ERR_NO_CONVERGENCE: a column of
 *   W did not reach rtol.  GSS_ERR_ALLOC: W does not fit; it takes 8 nv ceil16(nd) bytes for the life of the data, and
 *   the set-up the same again for diag(s) W.  After a refusal the handle has no data: earlier data are dropped before
 *   anything else is looked at (only a NULL handle leaves them).
 * gss_spde_condition_clear: back to unconditional realisations (the same bits as before the data).
 * gss_spde_condition_info: nd (0 without data), the mean, and (parity) W as nv x nd row-major; any may be NULL.
 * gss_spde_mean: the kriging mean at the vertices (vout, nv) and elements (eout, nt; the mean of the three vertex
 *   values); at least one of the two.  GSS_ERR_INVALID without data.
 * gss_spde_realize with data attached returns conditional realisations: `noise` is then nreals x (nv + nd), the field
 *   normals followed by the error normals (read only where r_i > 0), and the seeded error normal of observation i in
 *   realisation r is gss_philox_normal(seed, r, nv + i).  Realisation r depends on (seed, r), the mesh and the data
 *   only.  gss_spde_last_solve reports the worse of the two solves.  Profile scopes: "spde_condition" and inside it
 *   "spde_cond_w", "spde_cond_gram", "spde_cond_factor"; per block "spde_lambda" (the two triangular products) and
 *   "spde_combine" (the combine kernel).
 */
int32_t gss_spde_locate(gss_spde_t* h, const double* points, int64_t np, double tol, int64_t* triangle,
                        double* weight, int32_t mem, void* stream);
int32_t gss_spde_condition(gss_spde_t* h, int64_t nd, const int64_t* obs_vertex, const double* obs_weight,
                           const double* value, const double* error_var, double mean, double rtol, int64_t maxiter,
                           int32_t mem, void* stream);
int32_t gss_spde_condition_clear(gss_spde_t* h);
int32_t gss_spde_condition_info(gss_spde_t* h, int64_t* nd, double* mean, double* W, int32_t mem, void* stream);
int32_t gss_spde_mean(gss_spde_t* h, double rtol, int64_t maxiter, double* vout, double* eout, int32_t mem,
                      void* stream);

/* ---- SGS -----------------------------------------------------------
 * gss_sgs_create replaces SGS.preprocess (sgs.jl:56-85: SimpleKriging(variogram, mean) and the marginal
 *   Normal(mean, sqrt(sill))) and the realisation-independent part of the SeqSim path loop: for every
 *   node of `path` the masked search among already simulated cells (seq.jl:105), the fit (seq.jl:121)
 *   and the simple-kriging weights / standard deviation behind predictprob (seq.jl:126).  Nodes with
 *   fewer than minneighbors simulated neighbours, or a failed fit, draw from the marginal (seq.jl:107-109,
 *   124-128).  centroids N x d (host), path = visiting order (N 0-based cell indices, NULL = LinearPath),
 *   dlocs / zdata = conditioning cells and their values (initbuff with NearestInit, seq.jl:85);
 *   maxneighbors <= 1024 (beyond 64: the search in passes of 64, one workgroup per node for the weights);
 *   radius / inv_radii as gss_knn_search.  All realisations of a handle share the path.  The handle also keeps the
 *   levels of the recursion's dependency graph (a node's level = 1 + the highest level among its neighbours): the
 *   realisations are then simulated level by level, every node of a level at once, with the same sums in the same
 *   order as the walk along the path (bit-identical fields).
 * gss_sgs_realize replaces solvesingle (seq.jl:76-141) for realisations first_real..first_real+nreals-1:
 *   z[node] = mean + sum_j lambda_j (z[nb_j] - mean) + sigma eps, eps = Philox normal (seed, realisation,
 *   cell) or noise[r * N + cell] when given.  out is nreals x N.  The handle keeps its node-major working field
 *   (8 N nreals bytes for the largest nreals seen) until gss_sgs_destroy.
 * gss_sgs_weights (test support): per node the neighbour list (N x k), the number of conditioning
 *   neighbours actually used (0 = marginal or data cell), the weights (N x k) and sigma (N). */
/* flags: how `search!(neighbors, p, searcher, mask=simulated)` (seq.jl:105) treats the mask.  0: the k nearest AMONG the
 * already simulated cells.  GSS_SGS_MASK_AFTER_SEARCH: the k nearest cells of the whole domain (the node itself
 * included), of which the already simulated ones are kept -- what [DEP] Meshes' KNearestSearch / KBallSearch are recalled
 * to do (the mask is applied to the result of the tree query); the front-ends pass it by default. */
enum { GSS_SGS_MASK_AFTER_SEARCH = 1 };
/* bits 4..6 of flags: GSS_METRIC_* of the neighbour search (the solver parameter `distance`, seq.jl:91-98):
 * Euclidean (0, the only one that combines with a ball), Cityblock or Chebyshev; Haversine (its key has no box bounds:
 * exhaustive search) with GSS_SGS_MASK_AFTER_SEARCH only -- the masked search has no exhaustive variant;
 * GSS_METRIC_ROTATED_BALL (4) with inv_radii -> 12 doubles (see gss_knn_search). */
#define GSS_SGS_METRIC_SHIFT 4
int32_t gss_sgs_create(gss_sgs_t** out, const gss_variogram_t* vg, double mean, const double* centroids, int64_t N,
                       int32_t dim, const int64_t* path, const int64_t* dlocs, const double* zdata, int64_t nd,
                       int32_t maxneighbors, int32_t minneighbors, double radius, const double* inv_radii,
                       int32_t flags, void* stream);
/* One visiting order per realisation -- what the reference does for a RandomPath, whose `traverse` is called inside
 * solvesingle (seq.jl:99-102): paths = npaths x N cell indices, path p belongs to realisation path_base + p; stage A
 * (search, fit, weights) runs once per path and gss_sgs_realize(first_real, nreals) needs
 * path_base <= first_real and first_real + nreals <= path_base + npaths.  npaths == 1 is gss_sgs_create (every
 * realisation shares the order and one stage A serves them all). */
int32_t gss_sgs_create_paths(gss_sgs_t** out, const gss_variogram_t* vg, double mean, const double* centroids,
                             int64_t N, int32_t dim, const int64_t* paths, int64_t npaths, int64_t path_base,
                             const int64_t* dlocs, const double* zdata, int64_t nd, int32_t maxneighbors,
                             int32_t minneighbors, double radius, const double* inv_radii, int32_t flags,
                             void* stream);
int32_t gss_sgs_destroy(gss_sgs_t* h);
int32_t gss_sgs_weights(gss_sgs_t* h, int32_t* idx, int32_t* ncond, double* w, double* sigma, int32_t mem,
                        void* stream);
int32_t gss_sgs_realize(gss_sgs_t* h, uint64_t seed, int64_t first_real, int64_t nreals, const double* noise,
                        double* out, int32_t mem, void* stream);
/* gss_sgs_schedule (test support; launches nothing): which kernels the handle was built with and will sweep with.
 * out[0..6] (n >= GSS_SGS_SCHEDULE_WORDS): the number of visiting orders; the number of levels of the schedule (0: stage B
 * walks the path); the chunks, the realisations per team and the nodes per chunk of the team schedule (all 0 where the
 * sweep is not the team kernel's); 1 if the weights came from the workgroup-per-node kernel (more than 64 neighbours);
 * 1 if that kernel kept its covariance triangle in LDS, 0 in HBM. */
#define GSS_SGS_SCHEDULE_WORDS 7
int32_t gss_sgs_schedule(gss_sgs_t* h, int32_t* out, int32_t n);

/* ---- SIS: sequential indicator simulation (GSLIB sisim, median form) on an SGS handle -----------------------------
 * (The reference has no indicator simulator; the conventions are this library's own, those of the indicator-kriging
 * section below.)  Median indicator kriging has one variogram for all cutoffs, hence one simple-kriging weight vector
 * per node: a handle of gss_sgs_create / gss_sgs_create_paths built with the INDICATOR variogram holds the whole
 * realisation-independent part.  Its mean and sigma are not used; its zdata are the values at the conditioning cells
 * (categorical kind: codes 0 .. K-1 stored as doubles).
 *
 * Per node, for each realisation, with the node's list idx[0 .. ncond-1] and weights w taken in list order:
 *   GSS_SIS_CONTINUOUS   1 <= K <= 16 strictly increasing finite cutoffs, fstar in [0, 1] and non-decreasing,
 *       zmin < c_0, zmax > c_{K-1}, w_lo, w_hi > 0.  F_q = F*_q + sum_j w_j ((z_j <= c_q) - F*_q), the sum by fma in list
 *       order (no neighbours: the marginal F*); the order-relation correction of the indicator-kriging section (the same
 *       doubles); the value is the smallest z with F(z) >= u under the ccdf model of gss_ik_post (linear inside classes,
 *       power tails to zmin / zmax, a flat segment returns its left end).
 *   GSS_SIS_CATEGORICAL  2 <= K <= 16 categories, cutoffs NULL, fstar the K global proportions (each in [0, 1], summing
 *       to 1 within 1e-9).  p_s = p*_s + sum_j w_j ((z_j == s) - p*_s), each clipped to [0, 1]; divided by the clipped sum
 *       where that is positive, else p*; cumulated in category order; the draw is the first category s with u < cum_s, or,
 *       if rounding at the top leaves none, the last one with a positive probability.  The output is the code as a double.
 *       The codes in the handle's zdata are checked in the call, on a host copy: integral and in 0 .. K-1.
 *   Data cells keep their zdata.
 * cutoffs, fstar: HOST memory.  uniforms: NULL, or nreals x N in `mem`; NULL: the uniform of (realisation r, cell c) is
 * element c of gss_philox_uniform(seed, first_real + r, N).  out: nreals x N in `mem`; host output goes through the
 * output ring in blocks, as gss_sgs_realize, whose realisation-range rule for handles with one visiting order per
 * realisation holds here too.  GSS_ERR_INVALID before any launch: K out of range, bad cutoffs, proportions or tails, a
 * NULL out with nreals > 0, an unknown kind, a zdata that is no code.
 * Sweeps: level by level where the handle has levels (a team schedule is not used: node-major field, a launch per
 * level), along the path where it has none or where its levels hold fewer than 2 simulated nodes on average (DESIGN.md
 * section 4; the environment variable GSS_SIS_WALK_BELOW, read at every call, replaces the 2).  Every sweep gives the
 * same bits.  Not offered: full indicator simulation (one variogram per cutoff needs K sets of weights), ordinary
 * indicator kriging inside the recursion (stage A is simple kriging).  Profile scopes: "sis_fill", "sis_sweep". */
enum { GSS_SIS_CONTINUOUS = 0, GSS_SIS_CATEGORICAL = 1 };
int32_t gss_sis_realize(gss_sgs_t* h, int32_t kind, const double* cutoffs, int32_t K, const double* fstar,
                        double zmin, double zmax, double w_lo, double w_hi, uint64_t seed, int64_t first_real,
                        int64_t nreals, const double* uniforms, double* out, int32_t mem, void* stream);

/* ---- normal-score transform: skewed data into Gaussian space and realisations back (GSLIB nscore / backtr, the
 * reversible Quantile() step of a GeoStats pipeline).  Not in the reference's solvers; DESIGN.md section 4.
 *   Fit (host, preprocess): n >= 1 finite values z with optional weights w (finite, > 0; NULL = 1) are sorted stably,
 * equal values merged into distinct v_1 < ... < v_K with class weights W_k; cumulative weights are summed in long
 * double from both ends.  With B_k the weight strictly below v_k, A_k strictly above and T the total,
 *     y_k = Phi^-1((B_k + W_k / 2) / T)  if B_k <= A_k,   y_k = -Phi^-1((A_k + W_k / 2) / T)  otherwise
 * (the survival form keeps the upper tail as accurate as the lower one).  Phi^-1: a rational start and one correction
 * step on erfc.  Scores that rounding leaves non-increasing give GSS_ERR_INVALID (the message names the knot).
 *   FORWARD z -> y: z <= v_1 gives y_1, z >= v_K gives y_K, otherwise linear between the bracketing knots; a datum
 * gets exactly its class score.  INVERSE y -> z: inside [y_1, y_K] linear with the roles swapped;
 *     y < y_1:  z = zmin + (v_1 - zmin) t^power_lo,  t = Q(-y) / Q(-y_1),   Q(x) = erfc(x / sqrt 2) / 2
 *     y > y_K:  z = zmax - (zmax - v_K) t^power_hi,  t = Q(y) / Q(y_K)
 * (GSLIB's linear / power tails, written so that no probability near 1 is subtracted).  zmin / zmax = NaN mean v_1 /
 * v_K (clamp).  -inf gives zmin, +inf zmax, NaN gives NaN in both directions.  K = 1: forward is 0 everywhere and the
 * inverse is the two tails around y_1 = 0.
 *   gss_nscore_create takes HOST arrays and validates before it touches the device: n < 1, a non-finite value, a
 * weight that is not finite and positive, zmin > v_1, zmax < v_K, a power <= 0 and K > 2^24 are GSS_ERR_INVALID.
 * gss_nscore_table copies the knots (K doubles each) out of the device tables.
 *   gss_nscore_apply transforms nblocks runs of len doubles that start in_stride / out_stride elements apart (variable
 * a of every realisation of a gss_fftgs_realize_lmc output: nblocks = nreals, stride = nz N, one launch).  out == in
 * with equal strides is allowed; any other overlap, or a stride < len with nblocks > 1, is GSS_ERR_INVALID.
 * GSS_MEM_DEVICE: one launch in stream order, no allocation.  GSS_MEM_HOST: chunk by chunk through staged images;
 * the environment variable GSS_NSCORE_CHUNK_ELEMS caps the elements per chunk, for tests, like
 * GSS_COKRIG_CHUNK_POINTS: the results are the same bits.  Tables of up to 1 280 knots are searched in LDS, larger ones
 * in global memory; GSS_NSCORE_LDS_KNOTS (tests; at most 2 048, 0 = never) moves that threshold.  Both find exactly
 * the interval of a binary search and give the same bits.  Profile scope: "nscore_apply". */
typedef struct gss_nscore gss_nscore_t;
int32_t gss_nscore_create(gss_nscore_t** out, const double* z, const double* w, int64_t n, double zmin, double zmax,
                          double power_lo, double power_hi, void* stream);
int32_t gss_nscore_destroy(gss_nscore_t* h);
int32_t gss_nscore_info(const gss_nscore_t* h, int64_t* nknots);
int32_t gss_nscore_table(gss_nscore_t* h, double* v, double* y, int32_t mem, void* stream);
enum { GSS_NSCORE_FORWARD = 0, GSS_NSCORE_INVERSE = 1 };
int32_t gss_nscore_apply(gss_nscore_t* h, int32_t direction, const double* in, double* out, int64_t nblocks,
                         int64_t len, int64_t in_stride, int64_t out_stride, int32_t mem, void* stream);

/* ---- declustering: weights for preferentially sampled data, the first link of the chain (GSLIB declus, the
 * ecosystem's weight(data, BlockWeighting(sides)); what gss_nscore_create takes as w).  Not in the reference's solvers;
 * DESIGN.md section 4.  x is n x dim point-major, dim 1 .. 3, 1 <= n < 2^31 - 1, every coordinate finite.
 *   A cell.  For an origin o and sides s (one per axis, finite, > 0) the index of sample x along axis a is
 *     floor((x_a - o_a) / s_a)
 * in FP64: one subtraction and one IEEE division, no reciprocal, nothing fused.  A sample exactly on an edge therefore
 * belongs to the upper cell.  Every sample's index along every axis must lie in [0, 2^21) (a cell id then fits 63
 * bits); otherwise the call returns GSS_ERR_INVALID and the message names the axis.
 *   gss_decluster_cell_counts, one grid: count[i] = samples in the cell of sample i (itself included), *noccupied (a host
 * word) = distinct occupied cells.  The integer core of block weighting: w_i = n / (noccupied count[i]).
 *   gss_decluster_cells, the GSLIB sweep: sides is ncs x dim (1 <= ncs <= 256), each size is laid noff times
 * (1 <= noff <= 64).  With lo_a the smallest coordinate along axis a, offset k = 0 .. noff - 1 of size c has the origin
 *     o_a = lo_a - (s_a k) / noff          (the product and the quotient each rounded once).
 * The weights of one grid are n / (noccupied count_i): the integer product formed exactly (64 bits), converted to FP64
 * (exact below 2^53) and one division.  The weights of a size are the mean over its grids: summed in ascending k from
 * 0, then one division by noff.  wmean[c] = (sum_i w_i z_i) / n, reduced in a fixed order without floating-point
 * atomics: two calls on the same input give the same bits.  *best = the first c that attains the minimum
 * (GSS_DECLUS_MIN) or the maximum (GSS_DECLUS_MAX) of wmean, and w receives the weights of that size.  z must be
 * finite; z == NULL is allowed with ncs == 1 only: wmean is then untouched and *best = 0.  wmean and best are host
 * memory whatever `mem` says.
 *   The grids are counted in batches (a radix sort of (cell, sample) pairs and a scan per batch) of at most 2^24 pairs,
 * with scratch from the block pool.  The environment variable GSS_DECLUS_CHUNK_GRIDS caps the grids per batch, for
 * tests, like GSS_COKRIG_CHUNK_POINTS: the results are the same bits whatever the batching.
 *   gss_decluster_nearest, polygonal (Voronoi) declustering by discretisation: the M = prod dims points
 *     lo_a + (j_a + 1/2) step_a,   0 <= j_a < dims_a   (product and sum each rounded once; step finite, > 0; M <= 2^53)
 * are formed in HBM in pieces of 2^22 (GSS_DECLUS_CHUNK_QUERIES lowers that, for tests: same results), each is given
 * to its nearest sample by the searcher of gss_knn_search (k = 1, Euclidean, ties to the lower index), the hits are
 * counted with 64-bit integer atomics, and w_i = (n hits_i) / M.  *nzero (a host word) = samples nobody chose, whose
 * weight is 0: a finer lattice is needed before such weights go into gss_nscore_create.
 *   All three validate before they touch the device what can be checked without it: sizes, sides, steps, and for
 * GSS_MEM_HOST arrays also the coordinates, the values and the index range (device arrays are checked on the device).
 * Profile scopes: "declus_cell_counts", "declus_cells", "declus_nearest"; "declus_sort" is the radix sorts inside the
 * first two. */
enum { GSS_DECLUS_MIN = 0, GSS_DECLUS_MAX = 1 };
int32_t gss_decluster_cell_counts(const double* x, int64_t n, int32_t dim, const double* origin, const double* sides,
                                  int32_t* count, int64_t* noccupied, int32_t mem, void* stream);
int32_t gss_decluster_cells(const double* x, const double* z, int64_t n, int32_t dim, const double* sides, int32_t ncs,
                            int32_t noff, int32_t criterion, double* w, double* wmean, int32_t* best, int32_t mem,
                            void* stream);
int32_t gss_decluster_nearest(const double* x, int64_t n, int32_t dim, const double* lo, const double* step,
                              const int64_t* dims, double* w, int64_t* nzero, int32_t mem, void* stream);

/* ---- indicator kriging: the local distribution of a continuous variable without a Gaussian model (GSLIB ik3d +
 *      postik).  (The reference has no indicator solver; the conventions are this library's own.)
 *
 * Cutoffs      c_0 < c_1 < .. < c_{K-1}, 1 <= K <= 16, finite and strictly increasing (GSS_ERR_INVALID otherwise).
 * Indicator    i_jq = (z_j <= c_q) ? 1 : 0, formed in the kernel from z: a sample exactly on a cutoff counts as below it.
 * Variant      GSS_KRIG_ORDINARY: weights sum to one.  GSS_KRIG_SIMPLE about the global proportions fstar (K doubles in
 *              [0, 1], HOST memory like cutoffs): F_q = F*_q + sum_j lambda_j (i_jq - F*_q).  No drift variants.
 * Variograms   vgs / nvg, HOST memory.  nvg = 1: median indicator kriging, one system per point serves the K cutoffs.
 *              nvg = K: full indicator kriging, one system per cutoff and point on the same neighbour list.  Every
 *              stationary model of gss_krig_predict_knn, nested ones included; GSS_VG_POWER -> GSS_ERR_UNSUPPORTED.
 *              Rotated structures go through the frame contract of gss_variogram_t::rotation; the rotated models of one
 *              call must share one rotation and the others must not depend on a frame (isotropic structures, or equal
 *              radii): GSS_ERR_UNSUPPORTED otherwise.
 * Order relations (GSLIB, continuous variable)  clip each value to [0, 1]; upward pass U_q = max(U_{q-1}, F_q); downward
 *              pass from the top D_q = min(D_{q+1}, F_q); result (U_q + D_q) / 2.  Pure FP64 in a fixed order.  A row
 *              that holds a NaN stays all NaN.
 *
 * gss_ik_predict_knn: samples xdata (n x dim, point-major) and z (n), domain xdom (m x dim), all in `mem`.  k (1 .. 64,
 *   <= n; more than 64 -> GSS_ERR_UNSUPPORTED, the limit of the cokriging moving neighbourhood), minneighbors, radius,
 *   inv_radii, metric, metric_param: as gss_krig_predict_knn, one search per call.  Outputs: ccdf (m x K, point-major,
 *   corrected), raw (m x K, before the correction; may be NULL), status (m; may be NULL), idx_out (m x k) and
 *   count_out (m) as gss_krig_predict_knn (may be NULL).  Fewer than max(minneighbors, 1) neighbours: GSS_PT_MISSING
 *   and NaN in the K outputs; a non-positive pivot in any of the point's factorisations (or in the constraint's Schur
 *   complement): GSS_PT_SINGULAR and NaN.  No kriging variance is formed.  The domain is walked in chunks of 2^20
 *   points; the environment variable GSS_IK_CHUNK_POINTS caps the points per chunk (any positive count), for tests,
 *   like GSS_COKRIG_CHUNK_POINTS: the results are the same bits.  Profile scopes: "knn", "ik_local".
 *
 * gss_ik_order_relations: the correction alone, in place on m x K rows (for ccdfs assembled elsewhere, e.g. from the
 *   global neighbourhood).  *ncorrected (host word, may be NULL): the (point, cutoff) values it changed; *maxcorr
 *   (host word, may be NULL): the largest absolute change; a row that holds a NaN becomes all NaN and counts in neither
 *   figure.  gss_ik_predict_knn applies the same device function.
 *
 * gss_ik_post: from corrected rows, under the ccdf model
 *     inside a class (c_{q-1}, c_q]   F linear
 *     below c_0                       F(z) = F_0 ((z - zmin) / (c_0 - zmin))^w_lo
 *     above c_{K-1}                   F(z) = 1 - (1 - F_{K-1}) ((zmax - z) / (zmax - c_{K-1}))^w_hi
 *   (w = 1: linear tails; no hyperbolic tail, whose mean need not exist), any of: etype[m] (mean) and cvar[m]
 *   (variance, clamped at 0) from the closed-form class moments of DESIGN.md section 4; pabove[m x nthr] = 1 - F(t_i);
 *   quant[m x nq] = the smallest z with F(z) >= p_i (a flat segment returns its left end).  A row with a NaN gives
 *   NaNs.  zmin < c_0, zmax > c_{K-1}, w > 0, 0 < p < 1, thresholds inside [zmin, zmax], nthr and nq at most 16
 *   (GSS_ERR_INVALID otherwise); cutoffs, thresholds and probs are HOST arrays.  Profile scope: "ik_post". */
int32_t gss_ik_predict_knn(const double* xdata, const double* z, int64_t n, int32_t dim, const double* cutoffs,
                           int32_t K, const gss_variogram_t* vgs, int32_t nvg, int32_t variant, const double* fstar,
                           int32_t k, int32_t minneighbors, double radius, const double* inv_radii, int32_t metric,
                           double metric_param, const double* xdom, int64_t m, double* ccdf, double* raw,
                           uint8_t* status, int32_t* idx_out, int32_t* count_out, int32_t mem, void* stream);
int32_t gss_ik_order_relations(double* ccdf, int64_t m, int32_t K, int64_t* ncorrected, double* maxcorr, int32_t mem,
                               void* stream);
int32_t gss_ik_post(const double* ccdf, int64_t m, int32_t K, const double* cutoffs, double zmin, double zmax,
                    double w_lo, double w_hi, const double* thresholds, int32_t nthr, const double* probs, int32_t nq,
                    double* etype, double* cvar, double* pabove, double* quant, int32_t mem, void* stream);

/* ---- noise (test support): the Philox streams used above, n values for one realisation ----- */
int32_t gss_philox_uniform(uint64_t seed, int64_t real, int64_t n, double* out, int32_t mem, void* stream);
int32_t gss_philox_normal(uint64_t seed, int64_t real, int64_t n, double* out, int32_t mem, void* stream);

/* ---- dense FP64 building blocks on the MFMA path (exported for unit tests) ------------------
 * column-major, lower triangle; potrf overwrites the lower triangle of a with L; trtri writes
 * inv(L) (lower) to w.  Device pointers only. */
int32_t gss_dev_potrf(double* a, int64_t n, int64_t lda, void* stream);
/* a (n x n, full) <- unit lower-triangular L of the partial-pivot LU P a = L U (LAPACK getrf pivoting rule) */
int32_t gss_dev_getrf_l(double* a, int64_t n, int64_t lda, void* stream);
int32_t gss_dev_trtri(const double* l, int64_t n, int64_t ldl, double* w, int64_t ldw, void* stream);
/* factor and inverse in one go (the fit of gss_krig_fit and of gss_lugs_create): lower triangle of a <- L,
 * w <- inv(L) with zeros above the diagonal */
int32_t gss_dev_potrf_inverse(double* a, int64_t n, int64_t lda, double* w, int64_t ldw, void* stream);
/* D = alpha * A * B + beta * D with arbitrary element strides (A is M x K, B is K x N) */
int32_t gss_dev_gemm(int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t sa_i,
                     int64_t sa_k, const double* B, int64_t sb_k, int64_t sb_j, double beta, double* D,
                     int64_t sd_i, int64_t sd_j, int32_t lower_only, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSS_H */
