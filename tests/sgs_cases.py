"""One run per compiled instantiation of the SGS kernels (csrc/sgs_create.hip, csrc/sgs.hip, csrc/sgs_levels.hip).

tests/test_sgs_census.py holds this table against the kernels the compiler emitted into libgss_hip.so
(tools/kernel_census.py): every compiled kernel of FAMILIES has exactly one entry in CASES and every entry names a compiled
kernel.  A run launches several kernels, so the table has two parts: RUNS, the named runs, and CASES, which maps every key
to the name of a run that launches it or to UNREACHABLE("reason citing the dispatch line that rules it out").
tests/test_gpu_sgs_matrix.py does every run on the device and checks it stage by stage against tests/sgs_matrix.py: the
lists against a brute-force search, the weights and sigmas against an 80-bit Cholesky on the device's lists, the field
against the 80-bit recursion on the device's weights, and `SGSHandle.schedule()` against the kernels the run claims.
profiles/kernel_census_sgs.txt is the listing of the compiled kernels.

Keys are (kernel family, template arguments as the demangler prints them): the dimension of sgs_weights_kernel<DIM> and
sgs_weights_big_kernel<DIM> (with_dim in gss_sgs_create_paths), the realisations per team of sgs_level_team_kernel<RL>
(sgs_team_schedule, csrc/sgs_levels.hip) and the field layout of sgs_noise_kernel<Layout> / sgs_seed_data_kernel<Layout>
(sgs_realize_block, csrc/sgs.hip).

What routes a run (a Run's `expect` says where it must arrive; the test asserts it through schedule()):
 * k <= 64: sgs_weights_kernel, a wave per node; beyond: sgs_weights_big_kernel, a workgroup per node over a grid of
   min(N, 1024) workgroups (sgs_path, csrc/sgs_create.hip) -- N > 1024 gives the first N - 1024 workgroups a second node;
   its triangle in LDS while k (k + 1) / 2 + k <= 16640 (k <= 180), in a slab of HBM beyond;
 * stage B: one path, k <= 64 and an average level of at most 128 nodes: the team kernel, RL = 64 / 32 / 16 / 8 for an
   average of at most 14 / 28 / 56 / 128; other single paths level by level (sgs_level_sweep_kernel); several paths
   sgs_level_sweep_paths_kernel; with GSS_SGS_LEVELS=0 (read once per process: such runs go to a child process) the walks
   sgs_sweep_kernel, sgs_sweep_big_kernel (k > 64) and sgs_sweep_paths_kernel.

The geometry (sgs_matrix.geometry): cell centres of a grid moved by up to 0.3 of a cell, so no two search keys tie.
A `fail` run makes seq.jl:124-128 certain: sill exactly 1, cells a < b on the same point next to cell T, a path that ends
a, b, T.  T's list starts a, b, so the second pivot of its system is 1 - 1 * 1 = 0 on the device and in LAPACK alike: T
draws from the marginal (ncond 0, sigma 1, z = mean + eps).  b's own system is exact too: a leads its list at distance 0,
so lambda = e_0 and sigma = 0.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

FAMILIES = (
    # stage A (csrc/sgs_create.hip)
    "sgs_batch_minrank_kernel", "sgs_weights_kernel", "sgs_weights_big_kernel",
    # levels and team schedule (csrc/sgs_levels.hip)
    "sgs_level_init_kernel", "sgs_level_chain_kernel", "sgs_level_offsets_kernel", "sgs_team_inverse_kernel",
    "sgs_team_lists_kernel",
    # stage B (csrc/sgs.hip)
    "sgs_noise_kernel", "sgs_seed_data_kernel", "sgs_sweep_kernel", "sgs_sweep_big_kernel", "sgs_sweep_paths_kernel",
    "sgs_level_sweep_kernel", "sgs_level_sweep_paths_kernel", "sgs_level_team_kernel", "sgs_team_out_kernel",
    "sgs_transpose_kernel",
)

MAX_N, MAX_R = 2200, 130


def _rot2(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s], [s, c]])


def _rot3(a, b, g):
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Z = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]])
    Y = np.array([[cb, 0, sb], [0, 1.0, 0], [-sb, 0, cb]])
    X = np.array([[1.0, 0, 0], [0, cg, -sg], [0, sg, cg]])
    return Z @ Y @ X


ROT = {2: _rot2(0.5235987755982988), 3: _rot3(0.4, -0.7, 1.2)}


@dataclass(frozen=True)
class Run:
    dims: Tuple[int, ...]
    k: int                                         # maxneighbors
    R: int                                         # realisations
    expect: Tuple[Tuple[str, object], ...]         # what schedule() must say: sweep, team_rl, big, big_lds
    kind: str = "spherical"
    range: float = 9.0
    sill: float = 1.3
    nugget: float = 0.13
    mean: float = 0.4
    vg_radii: Optional[Tuple[float, ...]] = None   # the variogram's ball instead of `range` ...
    rotated: bool = False                          # ... on the frame ROT[d]
    nmin: int = 1                                  # minneighbors
    mask_after: bool = False                       # GSS_SGS_MASK_AFTER_SEARCH
    nd: int = 0                                    # data cells ...
    data: Optional[Tuple[int, ...]] = None         # ... these, else drawn
    radius: Optional[float] = None                 # search ball
    ball_radii: Optional[Tuple[float, ...]] = None
    path: str = "random"                           # "random" | "linear" (path = NULL)
    first: Optional[int] = None                    # the cell a random path starts with
    npaths: int = 1
    path_base: int = 0
    first_real: int = 0
    fail: Optional[Tuple[int, int, int]] = None    # (T, a, b): the failed factorisation of the module docstring
    seeded: bool = False                           # also draws its own normals (against oracle.philox.normal)
    env: Tuple[Tuple[str, str], ...] = ()          # switches read once per process: the run goes to a child process

    @property
    def expected(self):
        return dict(self.expect)


@dataclass(frozen=True)
class UNREACHABLE:
    reason: str


def _e(sweep, **kw):
    return tuple(dict(sweep=sweep, **kw).items())


_WALK = (("GSS_SGS_LEVELS", "0"),)
# the three exits of the grid-stride loop of sgs_weights_big_kernel at cells below N - 1024 = 76, each followed by an
# ordinary node (cell + 1024) in the same workgroup: data cells 10 and 40 (700: one that is nobody's predecessor), the
# path starts with cell 20, which has the 3 data cells < minneighbors = 4 for neighbours, and the failing node T = 5
_TRIP2 = dict(dims=(44, 25), R=3, kind="exponential", range=4.0, sill=1.0, nugget=0.0, nd=3, data=(10, 40, 700), nmin=4,
              first=20, fail=(5, 900, 901))

RUNS = {
    # ---- (a) sgs_weights_kernel<1 | 2 | 3>: k = 1, 7, 64, both readings of the mask, with and without data cells
    # 1-D, the row-by-row order: every level one node (sgs_level_team_kernel<64>); 301 cells, 67 realisations: two teams,
    # the second with 3 of its 64 realisations
    "line_k7_team64": Run((301,), 7, 67, _e("team", team_rl=64, band=True), kind="exponential", range=6.0, nugget=0.0, nd=4,
                          path="linear", seeded=True),
    # one neighbour inside an anisotropic search ball, no data: 10 levels of some 200 nodes, above the 128 of the team
    # kernel: sgs_level_sweep_kernel on the node-major field, sgs_transpose_kernel with N = 33 * 64 + 3, R = 64 + 6
    "plane_k1_ball": Run((47, 45), 1, 70, _e("levels", band=True), ball_radii=(3.0, 1.5), seeded=True),
    # a full wave of neighbours, minneighbors = 3 (the first nodes of the path draw from the marginal), a ball
    "plane_k64_min3": Run((41, 33), 64, 3, _e("team", team_rl=64), nmin=3, radius=7.0),
    "plane_k64_after": Run((31, 23), 64, 3, _e("team", team_rl=64), nmin=3, mask_after=True, nd=6),
    # a rotated variogram ball: covariances on the frame
    "cube_k7_rot": Run((13, 11, 9), 7, 5, _e("team", team_rl=8), vg_radii=(9.0, 6.0, 4.0), rotated=True, mask_after=True,
                       nd=5),
    "plane_k7_rot": Run((29, 21), 7, 5, _e("team", team_rl=64), vg_radii=(9.0, 5.0), rotated=True, nd=5),
    # (c) through the wave kernel
    "plane_k7_fail": Run((27, 21), 7, 5, _e("team", team_rl=64), kind="exponential", range=6.0, sill=1.0, nugget=0.0, nd=4,
                         fail=(300, 100, 101)),
    # ---- (b) sgs_weights_big_kernel<1 | 2 | 3>: k = 65, 180 (LDS, above 48 KiB: hipFuncSetAttribute), 181 (HBM).  More
    # than 64 neighbours never sweep with the team kernel (`h->k <= 64`, sgs_team_schedule): sgs_level_sweep_kernel
    "line_k181_hbm": Run((500,), 181, 3, _e("levels", big=True, big_lds=False), kind="exponential", range=6.0, nd=4,
                         mask_after=True),
    "cube_k65_lds": Run((12, 10, 8), 65, 3, _e("levels", big=True, big_lds=True), nd=5, nmin=2),
    "plane_k180_lds_trip2": Run(k=180, expect=_e("levels", big=True, big_lds=True), **_TRIP2),
    "plane_k181_hbm_trip2": Run(k=181, expect=_e("levels", big=True, big_lds=False), mask_after=True, **_TRIP2),
    # ---- (d) sgs_level_team_kernel<32 | 16 | 8> (<64>: line_k7_team64), the average level (21.3, 39.0, 70.2 nodes) at
    # least 15 % inside its band; the longest level (58, 120, 185 nodes) longer than the cap (32, 64, 128): several chunks
    "plane_team32": Run((30, 30), 5, 37, _e("team", team_rl=32, band=True), nd=7),
    "plane_team16": Run((47, 45), 6, 21, _e("team", team_rl=16, band=True), nd=7),
    "plane_team8": Run((47, 45), 3, 13, _e("team", team_rl=8, band=True), nd=9),
    # ---- (e) the other sweeps: one visiting order per realisation (paths 2..6 of which realisations 3, 4, 5 are drawn:
    # `path0` = 1 in the kernels), level by level and, without levels, along the paths; the two walks of a shared order
    "paths_levels": Run((23, 19), 7, 3, _e("level_paths"), nd=5, npaths=5, path_base=2, first_real=3, seeded=True),
    "walk_k9": Run((33, 21), 9, 67, _e("walk"), nd=5, env=_WALK),
    "walk_k65": Run((30, 17), 65, 67, _e("walk", big=True, big_lds=True), nd=5, env=_WALK),
    "walk_paths": Run((23, 19), 7, 3, _e("walk"), nd=5, npaths=5, path_base=2, first_real=3, env=_WALK),
}

# Error bars, in units of 2^-53 of the quantity's scale: max(1, max |lambda|) for a node's weights, sqrt(sill) for sigma,
# max |z - mean| for a field.  "oracle": the largest error over RUNS of the FP64 restatement (numpy.linalg on the
# covariances as oracle/sgs.py, a plain numpy recursion) against the 80-bit one of tests/sgs_matrix.py, measured on the CPU
# with tools/sgs_matrix_oracle.py, never on the device; "bar" = 16 x that and at least 8 units -- the device factorises in
# another order with fused multiply-adds and has its own exp and sqrt; "scale": the largest scale met, with which
# tests/test_sgs_census.py shows that no bar is looser than TOL, what tests/test_gpu_sgs.py already holds.
TOL = {"w": 1e-11, "sigma": 1e-11, "z": 1e-9}
BARS = {
    "w": {"oracle": 19.05, "bar": 304.76, "scale": 1.000},
    "sigma": {"oracle": 5.99, "bar": 95.88, "scale": 1.140},
    "z": {"oracle": 6.99, "bar": 111.77, "scale": 5.688},
}

CASES = {
    ("sgs_batch_minrank_kernel", ()): "plane_k64_min3",
    **{("sgs_weights_kernel", (d,)): r for d, r in ((1, "line_k7_team64"), (2, "plane_k64_min3"), (3, "cube_k7_rot"))},
    **{("sgs_weights_big_kernel", (d,)): r
       for d, r in ((1, "line_k181_hbm"), (2, "plane_k180_lds_trip2"), (3, "cube_k65_lds"))},
    ("sgs_level_init_kernel", ()): "plane_k1_ball",
    ("sgs_level_chain_kernel", ()): "plane_k1_ball",
    ("sgs_level_offsets_kernel", ()): "plane_k1_ball",
    ("sgs_team_inverse_kernel", ()): "plane_team16",
    ("sgs_team_lists_kernel", ()): "plane_team16",
    ("sgs_noise_kernel", ("gss::SgsNodeMajor",)): "plane_k1_ball",
    ("sgs_noise_kernel", ("gss::SgsRealMajor",)): "paths_levels",
    ("sgs_noise_kernel", ("gss::SgsTeamLayout",)): "line_k7_team64",
    ("sgs_seed_data_kernel", ("gss::SgsNodeMajor",)): "plane_k181_hbm_trip2",
    ("sgs_seed_data_kernel", ("gss::SgsRealMajor",)): "paths_levels",
    ("sgs_seed_data_kernel", ("gss::SgsTeamLayout",)): "line_k7_team64",
    ("sgs_sweep_kernel", ()): "walk_k9",
    ("sgs_sweep_big_kernel", ()): "walk_k65",
    ("sgs_sweep_paths_kernel", ()): "walk_paths",
    ("sgs_level_sweep_kernel", ()): "plane_k1_ball",
    ("sgs_level_sweep_paths_kernel", ()): "paths_levels",
    ("sgs_level_team_kernel", (64,)): "line_k7_team64",
    ("sgs_level_team_kernel", (32,)): "plane_team32",
    ("sgs_level_team_kernel", (16,)): "plane_team16",
    ("sgs_level_team_kernel", (8,)): "plane_team8",
    ("sgs_team_out_kernel", ()): "line_k7_team64",
    ("sgs_transpose_kernel", ()): "plane_k1_ball",
}
