"""One run per compiled instantiation of the sequential-indicator-simulation kernels (csrc/sis.hip).

tests/test_sis_census.py holds this table against the kernels the compiler emitted into libgss_hip.so
(tools/kernel_census.py): every compiled kernel whose name starts with `sis_` has exactly one entry in CASES and every entry
names a compiled kernel and a run of RUNS that launches it.  tests/test_sis_host.py shows on the CPU that no draw of any
run is a close call (tests/sis_ref.py), so tests/test_gpu_sis.py compares every run on the device with the sequential
restatement without exclusions.

Keys are (kernel family, template arguments as the demangler prints them): (KT, CAT) of the four sweeps -- KT = K rounded
up to 4 / 8 / 16 (sis_realize_kinds), CAT = the categorical kind -- and the field layout of sis_fill_kernel<NODE_MAJOR> /
sis_seed_data_kernel<NODE_MAJOR> (node-major for a shared order, realisation-major for one order per realisation).

What routes a run (sis_realize_block):
 * a shared order with levels: sis_level_sweep_kernel; one order per realisation with levels: sis_level_sweep_paths_kernel.
   Levels shorter than 2 nodes on average would be walked instead, so these runs are done with GSS_SIS_WALK_BELOW=0 (read
   at every call) and assert that the handle has levels;
 * without levels -- GSS_SGS_LEVELS=0, read once per process: such runs go to a child process -- sis_sweep_kernel and
   sis_sweep_paths_kernel.
The geometry is that of tests/sgs_matrix.py (jittered cell centres: no two search keys tie).
"""
from dataclasses import dataclass
from typing import Tuple

FAMILIES = ("sis_fill_kernel", "sis_seed_data_kernel", "sis_level_sweep_kernel", "sis_level_sweep_paths_kernel",
            "sis_sweep_kernel", "sis_sweep_paths_kernel", "sis_transpose_kernel")

MAX_N, MAX_R = 256, 130
SWEEP_FAMILY = {"levels": "sis_level_sweep_kernel", "level_paths": "sis_level_sweep_paths_kernel",
                "walk": "sis_sweep_kernel", "walk_paths": "sis_sweep_paths_kernel"}
_WALK = (("GSS_SGS_LEVELS", "0"),)


@dataclass(frozen=True)
class Run:
    dims: Tuple[int, ...]
    k: int                                  # maxneighbors
    R: int                                  # realisations
    K: int                                  # cutoffs | categories
    categorical: bool
    sweep: str                              # levels | level_paths | walk | walk_paths
    nd: int = 0                             # conditioning cells
    nmin: int = 1                           # minneighbors
    nugget_only: bool = False               # sill = nugget: every weight is zero, the draws are independent
    tail: Tuple[float, float] = (1.0, 1.0)  # w_lo, w_hi (continuous)
    npaths: int = 1
    path_base: int = 0
    first_real: int = 0
    seed: int = 2024
    env: Tuple[Tuple[str, str], ...] = ()   # switches read once per process: the run goes to a child process

    @property
    def KT(self):
        return 4 if self.K <= 4 else (8 if self.K <= 8 else 16)


def _paths(**kw):
    return dict(npaths=5, path_base=2, first_real=3, R=3, **kw)


RUNS = {
    # ---- level by level, shared order: 130 realisations = one full wave, one partial wave, a second block of the host ring
    "lv_cont_K1": Run((16, 16), 4, 130, 1, False, "levels", nd=6, tail=(2.0, 0.5)),
    "lv_cont_K3_free": Run((16, 16), 16, 67, 3, False, "levels"),                        # no conditioning cells
    "lv_cont_K4_k80": Run((16, 16), 80, 67, 4, False, "levels", nd=6),                   # lists longer than 64
    "lv_cont_K5": Run((8, 8, 4), 16, 130, 5, False, "levels", nd=6, tail=(1.0, 2.5)),
    "lv_cont_K8_min": Run((16, 16), 16, 67, 8, False, "levels", nd=6, nmin=9),           # the first 3 nodes are marginal
    "lv_cont_K9": Run((13, 11), 4, 67, 9, False, "levels", nd=6),                       # 143 cells: a partial tile
    "lv_cont_K16": Run((16, 16), 16, 130, 16, False, "levels", nd=9, tail=(1.5, 1.5)),
    "lv_cat_K2": Run((16, 16), 4, 130, 2, True, "levels", nd=6),
    "lv_cat_K3_nugget": Run((16, 16), 16, 130, 3, True, "levels", nd=6, nugget_only=True),
    "lv_cat_K8_k80": Run((8, 8, 4), 80, 67, 8, True, "levels", nd=9),
    "lv_cat_K16": Run((16, 16), 16, 67, 16, True, "levels", nd=20),
    # ---- level by level, one order per realisation: paths 2 .. 6, of which realisations 3, 4, 5 are drawn
    "lp_cont_K3": Run((16, 16), 16, K=3, categorical=False, sweep="level_paths", **_paths(nd=6)),
    "lp_cont_K8": Run((13, 11), 4, K=8, categorical=False, sweep="level_paths", **_paths(nd=5, tail=(2.0, 2.0))),
    "lp_cont_K16": Run((13, 11), 16, K=16, categorical=False, sweep="level_paths", **_paths()),
    "lp_cat_K3": Run((13, 11), 16, K=3, categorical=True, sweep="level_paths", **_paths(nd=5)),
    "lp_cat_K8": Run((8, 8, 4), 4, K=8, categorical=True, sweep="level_paths", **_paths(nd=9)),
    "lp_cat_K16": Run((13, 11), 80, K=16, categorical=True, sweep="level_paths", **_paths(nd=17)),
    # ---- along the path (GSS_SGS_LEVELS=0), shared order
    "wk_cont_K4": Run((16, 16), 16, 67, 4, False, "walk", nd=6, env=_WALK),
    "wk_cont_K5_k80": Run((13, 11), 80, 67, 5, False, "walk", nd=5, tail=(0.5, 3.0), env=_WALK),
    "wk_cont_K9_min": Run((16, 16), 4, 130, 9, False, "walk", nd=2, nmin=4, env=_WALK),  # the first 2 nodes are marginal
    "wk_cat_K2": Run((13, 11), 16, 67, 2, True, "walk", env=_WALK),
    "wk_cat_K8": Run((16, 16), 4, 130, 8, True, "walk", nd=9, env=_WALK),
    "wk_cat_K16": Run((13, 11), 16, 67, 16, True, "walk", nd=17, env=_WALK),
    # ---- along the paths, one order per realisation
    "wp_cont_K1": Run((13, 11), 16, K=1, categorical=False, sweep="walk_paths", env=_WALK, **_paths(nd=5)),
    "wp_cont_K8": Run((13, 11), 80, K=8, categorical=False, sweep="walk_paths", env=_WALK, **_paths(nd=5)),
    "wp_cont_K16": Run((8, 8, 4), 4, K=16, categorical=False, sweep="walk_paths", env=_WALK, **_paths(nd=9)),
    "wp_cat_K3": Run((13, 11), 4, K=3, categorical=True, sweep="walk_paths", env=_WALK, **_paths(nd=5)),
    "wp_cat_K8": Run((13, 11), 16, K=8, categorical=True, sweep="walk_paths", env=_WALK, **_paths(nd=9)),
    "wp_cat_K16": Run((16, 16), 16, K=16, categorical=True, sweep="walk_paths", env=_WALK, **_paths()),
}


def _cat(b):
    return "true" if b else "false"


CASES = {
    **{(SWEEP_FAMILY[sweep], (kt, _cat(cat))): name
       for sweep, kt, cat, name in (
           ("levels", 4, False, "lv_cont_K4_k80"), ("levels", 8, False, "lv_cont_K5"), ("levels", 16, False, "lv_cont_K16"),
           ("levels", 4, True, "lv_cat_K2"), ("levels", 8, True, "lv_cat_K8_k80"), ("levels", 16, True, "lv_cat_K16"),
           ("level_paths", 4, False, "lp_cont_K3"), ("level_paths", 8, False, "lp_cont_K8"),
           ("level_paths", 16, False, "lp_cont_K16"), ("level_paths", 4, True, "lp_cat_K3"),
           ("level_paths", 8, True, "lp_cat_K8"), ("level_paths", 16, True, "lp_cat_K16"),
           ("walk", 4, False, "wk_cont_K4"), ("walk", 8, False, "wk_cont_K5_k80"), ("walk", 16, False, "wk_cont_K9_min"),
           ("walk", 4, True, "wk_cat_K2"), ("walk", 8, True, "wk_cat_K8"), ("walk", 16, True, "wk_cat_K16"),
           ("walk_paths", 4, False, "wp_cont_K1"), ("walk_paths", 8, False, "wp_cont_K8"),
           ("walk_paths", 16, False, "wp_cont_K16"), ("walk_paths", 4, True, "wp_cat_K3"),
           ("walk_paths", 8, True, "wp_cat_K8"), ("walk_paths", 16, True, "wp_cat_K16"))},
    ("sis_fill_kernel", ("true",)): "lv_cont_K1",
    ("sis_fill_kernel", ("false",)): "lp_cont_K3",
    ("sis_seed_data_kernel", ("true",)): "lv_cont_K1",
    ("sis_seed_data_kernel", ("false",)): "lp_cont_K3",
    ("sis_transpose_kernel", ()): "lv_cont_K9",
}
