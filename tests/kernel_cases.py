"""One case per compiled instantiation of the kriging kernels.

tests/test_kernel_census.py holds this table against the kernels the compiler actually emitted into libgss_hip.so
(tools/kernel_census.py): every compiled kernel of FAMILIES has exactly one entry here and every entry names a compiled
kernel, so an instantiation added to a dispatch switch without a case fails on the CPU.  An entry is a Case, or
UNREACHABLE("reason citing the dispatch line that rules the instantiation out").  tests/test_gpu_kernel_matrix.py runs
every Case on the device against the 50-digit answer of tests/kernel_matrix.py.

Keys are (kernel family, template arguments as the demangler prints them).  KIND arguments: 0 Gaussian, 1 exponential,
2 spherical, 30 / 31 / 32 Matern 1/2, 3/2, 5/2, -1 the general kernel (any other model: cubic and pentaspherical here,
which vanish beyond the range as the decoupled clusters need; SineHole never does).  The dispatch picks
 * krig_rhs2_kernel<DIM, KIND>, krig_batch_mean_kernel<DIM, KIND>: by the model (csrc/krig.hip, launch_krig_rhs and
   launch_krig_batch_mean; the batched means have no Matern-1/2 copy: it takes the general one);
 * krig_rhs_block_kernel<DIM>, block_cvv_kernel<DIM>: block support, by the dimension only;
 * krig_local_mfma_kernel<DIM, KIND, NT>: NT = 1 / 2 / 4 for k <= 16 / 32 / 64 neighbours (csrc/krig_local.hip);
 * krig_local_tiles_kernel<DIM, KIND, NTMAX>: NTMAX = 6 / 8 / 16 for k <= 96 / 128 / 256 (csrc/krig_tiles.hip);
 * krig_local_slab_kernel<DIM, KIND>: 257 .. 768 neighbours (csrc/krig_slab.hip);
 * krig_local_big_kernel<DIM>: 769 neighbours and more (csrc/krig_local.hip).
Neighbour counts sit at the ends of each size class.  Moving-neighbourhood cases have exactly k samples, so every
estimation point sees all of them and the block structure of tests/kernel_matrix.py holds for each system.
"""
from dataclasses import dataclass
from typing import Optional


@dataclass(frozen=True)
class Case:
    model: str                  # key of kernel_matrix.MODELS
    dim: int
    k: Optional[int] = None     # neighbours of the moving neighbourhood (and sample count); None: the global path
    n: Optional[int] = None     # samples of a global case
    ball: bool = False          # MetricBall with unequal radii (kernel_matrix.RADII) instead of an isotropic range
    variant: str = "OK"         # "OK", or "UK" with degree 1
    batch: int = 0              # > 0: that many data vectors through predict_global_batch
    block: bool = False         # block support (set_block_support) on the global path


@dataclass(frozen=True)
class UNREACHABLE:
    reason: str


FAMILIES = ("krig_rhs2_kernel", "krig_batch_mean_kernel", "krig_rhs_block_kernel", "block_cvv_kernel",
            "krig_local_mfma_kernel", "krig_local_tiles_kernel", "krig_local_slab_kernel", "krig_local_big_kernel")

# Error bars, in units of 2^-53 sill (kernel_matrix.UNIT).  "oracle": the largest error of oracle.kriging (FP64, LAPACK)
# against the 50-digit answer over the family's cases, measured with tools/kernel_matrix_oracle.py; "bar" = 16 x that
# with a floor of 8 (the device eliminates in another order -- tile Cholesky, Schur complement, MFMA accumulation --
# and has its own exp / sqrt of 2.2e-16 relative error), and never looser than the 1e-9 of DESIGN.md section 3.
# "cov" is the pairwise covariance C(x0, x) of the same points (HipEngine.cov_pairwise against oracle.variogram).
BARS = {
    "krig_rhs2_kernel": {
        "mean": {"oracle": 22.33, "bar": 357.3},
        "var": {"oracle": 5.33, "bar": 85.3},
        "cov": {"oracle": 8.51, "bar": 136.2},
    },
    "krig_batch_mean_kernel": {
        "mean": {"oracle": 29.33, "bar": 469.3},
        "var": {"oracle": 2.00, "bar": 32.0},
        "cov": {"oracle": 8.51, "bar": 136.2},
    },
    "krig_rhs_block_kernel": {
        "mean": {"oracle": 6.00, "bar": 96.0},
        "var": {"oracle": 1.33, "bar": 21.3},
        "cov": {"oracle": 8.51, "bar": 136.2},
    },
    "block_cvv_kernel": {
        "mean": {"oracle": 4.00, "bar": 64.0},
        "var": {"oracle": 2.50, "bar": 40.0},
        "cov": {"oracle": 1.00, "bar": 16.0},
    },
    "krig_local_mfma_kernel": {
        "mean": {"oracle": 9.33, "bar": 149.3},
        "var": {"oracle": 3.67, "bar": 58.7},
        "cov": {"oracle": 8.51, "bar": 136.2},
    },
    "krig_local_tiles_kernel": {
        "mean": {"oracle": 12.67, "bar": 202.7},
        "var": {"oracle": 2.33, "bar": 37.3},
        "cov": {"oracle": 8.51, "bar": 136.2},
    },
    "krig_local_slab_kernel": {
        "mean": {"oracle": 17.92, "bar": 286.7},
        "var": {"oracle": 2.00, "bar": 32.0},
        "cov": {"oracle": 8.51, "bar": 136.2},
    },
    "krig_local_big_kernel": {
        "mean": {"oracle": 14.25, "bar": 228.0},
        "var": {"oracle": 2.33, "bar": 37.3},
        "cov": {"oracle": 8.51, "bar": 136.2},
    },
}

CASES = {
    # ---- krig_rhs2_kernel
    ("krig_rhs2_kernel", (1, -1)): Case("cubic", 1, n=20, variant="UK"),
    ("krig_rhs2_kernel", (1, 0)): Case("gaussian", 1, n=33),
    ("krig_rhs2_kernel", (1, 1)): Case("exponential", 1, n=16),
    ("krig_rhs2_kernel", (1, 2)): Case("spherical", 1, n=25),
    ("krig_rhs2_kernel", (1, 30)): Case("matern12", 1, n=20),
    ("krig_rhs2_kernel", (1, 31)): Case("matern32", 1, n=33),
    ("krig_rhs2_kernel", (1, 32)): Case("matern52", 1, n=16),
    ("krig_rhs2_kernel", (2, -1)): Case("pentaspherical", 2, n=25, variant="UK"),
    ("krig_rhs2_kernel", (2, 0)): Case("gaussian", 2, n=20, ball=True),
    ("krig_rhs2_kernel", (2, 1)): Case("exponential", 2, n=33),
    ("krig_rhs2_kernel", (2, 2)): Case("spherical", 2, n=16, ball=True),
    ("krig_rhs2_kernel", (2, 30)): Case("matern12", 2, n=25),
    ("krig_rhs2_kernel", (2, 31)): Case("matern32", 2, n=20, ball=True),
    ("krig_rhs2_kernel", (2, 32)): Case("matern52", 2, n=33),
    ("krig_rhs2_kernel", (3, -1)): Case("cubic", 3, n=16, variant="UK", ball=True),
    ("krig_rhs2_kernel", (3, 0)): Case("gaussian", 3, n=25),
    ("krig_rhs2_kernel", (3, 1)): Case("exponential", 3, n=20, ball=True),
    ("krig_rhs2_kernel", (3, 2)): Case("spherical", 3, n=33),
    ("krig_rhs2_kernel", (3, 30)): Case("matern12", 3, n=16, ball=True),
    ("krig_rhs2_kernel", (3, 31)): Case("matern32", 3, n=25),
    ("krig_rhs2_kernel", (3, 32)): Case("matern52", 3, n=20, ball=True),
    # ---- krig_batch_mean_kernel
    ("krig_batch_mean_kernel", (1, -1)): Case("cubic", 1, n=18, batch=5),
    ("krig_batch_mean_kernel", (1, 0)): Case("gaussian", 1, n=31, batch=16),
    ("krig_batch_mean_kernel", (1, 1)): Case("exponential", 1, n=23, batch=3),
    ("krig_batch_mean_kernel", (1, 2)): Case("spherical", 1, n=18, batch=5),
    ("krig_batch_mean_kernel", (1, 31)): Case("matern32", 1, n=31, batch=16),
    ("krig_batch_mean_kernel", (1, 32)): Case("matern52", 1, n=23, batch=3),
    ("krig_batch_mean_kernel", (2, -1)): Case("pentaspherical", 2, n=18, batch=5, ball=True),
    ("krig_batch_mean_kernel", (2, 0)): Case("gaussian", 2, n=31, batch=16),
    ("krig_batch_mean_kernel", (2, 1)): Case("exponential", 2, n=23, batch=3, ball=True),
    ("krig_batch_mean_kernel", (2, 2)): Case("spherical", 2, n=18, batch=5),
    ("krig_batch_mean_kernel", (2, 31)): Case("matern32", 2, n=31, batch=16, ball=True),
    ("krig_batch_mean_kernel", (2, 32)): Case("matern52", 2, n=23, batch=3),
    ("krig_batch_mean_kernel", (3, -1)): Case("cubic", 3, n=18, batch=5, ball=True),
    ("krig_batch_mean_kernel", (3, 0)): Case("gaussian", 3, n=31, batch=16),
    ("krig_batch_mean_kernel", (3, 1)): Case("exponential", 3, n=23, batch=3, ball=True),
    ("krig_batch_mean_kernel", (3, 2)): Case("spherical", 3, n=18, batch=5),
    ("krig_batch_mean_kernel", (3, 31)): Case("matern32", 3, n=31, batch=16, ball=True),
    ("krig_batch_mean_kernel", (3, 32)): Case("matern52", 3, n=23, batch=3),
    # ---- krig_rhs_block_kernel
    ("krig_rhs_block_kernel", (1,)): Case("exponential", 1, n=14, block=True),
    ("krig_rhs_block_kernel", (2,)): Case("matern52", 2, n=21, block=True),
    ("krig_rhs_block_kernel", (3,)): Case("cubic", 3, n=19, block=True, ball=True),
    # ---- block_cvv_kernel
    ("block_cvv_kernel", (1,)): Case("spherical", 1, n=14, block=True),
    ("block_cvv_kernel", (2,)): Case("gaussian", 2, n=21, block=True),
    ("block_cvv_kernel", (3,)): Case("matern32", 3, n=19, block=True, ball=True),
    # ---- krig_local_mfma_kernel
    ("krig_local_mfma_kernel", (1, -1, 1)): Case("pentaspherical", 1, k=16),
    ("krig_local_mfma_kernel", (1, -1, 2)): Case("cubic", 1, k=32),
    ("krig_local_mfma_kernel", (1, -1, 4)): Case("pentaspherical", 1, k=64),
    ("krig_local_mfma_kernel", (2, -1, 1)): Case("cubic", 2, k=16),
    ("krig_local_mfma_kernel", (2, -1, 2)): Case("pentaspherical", 2, k=32, ball=True),
    ("krig_local_mfma_kernel", (2, -1, 4)): Case("cubic", 2, k=64),
    ("krig_local_mfma_kernel", (2, 0, 1)): Case("gaussian", 2, k=16, ball=True),
    ("krig_local_mfma_kernel", (2, 0, 2)): Case("gaussian", 2, k=17),
    ("krig_local_mfma_kernel", (2, 0, 4)): Case("gaussian", 2, k=33, ball=True),
    ("krig_local_mfma_kernel", (2, 1, 1)): Case("exponential", 2, k=16),
    ("krig_local_mfma_kernel", (2, 1, 2)): Case("exponential", 2, k=32, ball=True),
    ("krig_local_mfma_kernel", (2, 1, 4)): Case("exponential", 2, k=64),
    ("krig_local_mfma_kernel", (2, 2, 1)): Case("spherical", 2, k=16, ball=True),
    ("krig_local_mfma_kernel", (2, 2, 2)): Case("spherical", 2, k=17),
    ("krig_local_mfma_kernel", (2, 2, 4)): Case("spherical", 2, k=33, ball=True),
    ("krig_local_mfma_kernel", (2, 31, 1)): Case("matern32", 2, k=16),
    ("krig_local_mfma_kernel", (2, 31, 2)): Case("matern32", 2, k=32, ball=True),
    ("krig_local_mfma_kernel", (2, 31, 4)): Case("matern32", 2, k=64),
    ("krig_local_mfma_kernel", (2, 32, 1)): Case("matern52", 2, k=16, ball=True),
    ("krig_local_mfma_kernel", (2, 32, 2)): Case("matern52", 2, k=17),
    ("krig_local_mfma_kernel", (2, 32, 4)): Case("matern52", 2, k=33, ball=True),
    ("krig_local_mfma_kernel", (3, -1, 1)): Case("pentaspherical", 3, k=16),
    ("krig_local_mfma_kernel", (3, -1, 2)): Case("cubic", 3, k=17, ball=True),
    ("krig_local_mfma_kernel", (3, -1, 4)): Case("pentaspherical", 3, k=33),
    ("krig_local_mfma_kernel", (3, 0, 1)): Case("gaussian", 3, k=16, ball=True),
    ("krig_local_mfma_kernel", (3, 0, 2)): Case("gaussian", 3, k=32),
    ("krig_local_mfma_kernel", (3, 0, 4)): Case("gaussian", 3, k=64, ball=True),
    ("krig_local_mfma_kernel", (3, 1, 1)): Case("exponential", 3, k=16),
    ("krig_local_mfma_kernel", (3, 1, 2)): Case("exponential", 3, k=17, ball=True),
    ("krig_local_mfma_kernel", (3, 1, 4)): Case("exponential", 3, k=33),
    ("krig_local_mfma_kernel", (3, 2, 1)): Case("spherical", 3, k=16, ball=True),
    ("krig_local_mfma_kernel", (3, 2, 2)): Case("spherical", 3, k=32),
    ("krig_local_mfma_kernel", (3, 2, 4)): Case("spherical", 3, k=64, ball=True),
    ("krig_local_mfma_kernel", (3, 31, 1)): Case("matern32", 3, k=16),
    ("krig_local_mfma_kernel", (3, 31, 2)): Case("matern32", 3, k=17, ball=True),
    ("krig_local_mfma_kernel", (3, 31, 4)): Case("matern32", 3, k=33),
    ("krig_local_mfma_kernel", (3, 32, 1)): Case("matern52", 3, k=16, ball=True),
    ("krig_local_mfma_kernel", (3, 32, 2)): Case("matern52", 3, k=32),
    ("krig_local_mfma_kernel", (3, 32, 4)): Case("matern52", 3, k=64, ball=True),
    # ---- krig_local_tiles_kernel
    ("krig_local_tiles_kernel", (1, -1, 16)): Case("pentaspherical", 1, k=256),
    ("krig_local_tiles_kernel", (1, -1, 6)): Case("cubic", 1, k=96),
    ("krig_local_tiles_kernel", (1, -1, 8)): Case("pentaspherical", 1, k=128),
    ("krig_local_tiles_kernel", (2, -1, 16)): Case("cubic", 2, k=256),
    ("krig_local_tiles_kernel", (2, -1, 6)): Case("pentaspherical", 2, k=96, ball=True),
    ("krig_local_tiles_kernel", (2, -1, 8)): Case("cubic", 2, k=128),
    ("krig_local_tiles_kernel", (2, 1, 16)): Case("exponential", 2, k=129, ball=True),
    ("krig_local_tiles_kernel", (2, 1, 6)): Case("exponential", 2, k=65),
    ("krig_local_tiles_kernel", (2, 1, 8)): Case("exponential", 2, k=97, ball=True),
    ("krig_local_tiles_kernel", (2, 2, 16)): Case("spherical", 2, k=256),
    ("krig_local_tiles_kernel", (2, 2, 6)): Case("spherical", 2, k=96, ball=True),
    ("krig_local_tiles_kernel", (2, 2, 8)): Case("spherical", 2, k=128),
    ("krig_local_tiles_kernel", (2, 31, 16)): Case("matern32", 2, k=129, ball=True),
    ("krig_local_tiles_kernel", (2, 31, 6)): Case("matern32", 2, k=65),
    ("krig_local_tiles_kernel", (2, 31, 8)): Case("matern32", 2, k=97, ball=True),
    ("krig_local_tiles_kernel", (3, -1, 16)): Case("pentaspherical", 3, k=129),
    ("krig_local_tiles_kernel", (3, -1, 6)): Case("cubic", 3, k=65, ball=True),
    ("krig_local_tiles_kernel", (3, -1, 8)): Case("pentaspherical", 3, k=97),
    ("krig_local_tiles_kernel", (3, 1, 16)): Case("exponential", 3, k=256, ball=True),
    ("krig_local_tiles_kernel", (3, 1, 6)): Case("exponential", 3, k=96),
    ("krig_local_tiles_kernel", (3, 1, 8)): Case("exponential", 3, k=128, ball=True),
    ("krig_local_tiles_kernel", (3, 2, 16)): Case("spherical", 3, k=129),
    ("krig_local_tiles_kernel", (3, 2, 6)): Case("spherical", 3, k=65, ball=True),
    ("krig_local_tiles_kernel", (3, 2, 8)): Case("spherical", 3, k=97),
    ("krig_local_tiles_kernel", (3, 31, 16)): Case("matern32", 3, k=256, ball=True),
    ("krig_local_tiles_kernel", (3, 31, 6)): Case("matern32", 3, k=96),
    ("krig_local_tiles_kernel", (3, 31, 8)): Case("matern32", 3, k=128, ball=True),
    # ---- krig_local_slab_kernel
    ("krig_local_slab_kernel", (1, -1)): Case("cubic", 1, k=257),
    ("krig_local_slab_kernel", (2, -1)): Case("pentaspherical", 2, k=768),
    ("krig_local_slab_kernel", (2, 1)): Case("exponential", 2, k=257, ball=True),
    ("krig_local_slab_kernel", (2, 2)): Case("spherical", 2, k=768),
    ("krig_local_slab_kernel", (2, 31)): Case("matern32", 2, k=257, ball=True),
    ("krig_local_slab_kernel", (3, -1)): Case("cubic", 3, k=768),
    ("krig_local_slab_kernel", (3, 1)): Case("exponential", 3, k=257, ball=True),
    ("krig_local_slab_kernel", (3, 2)): Case("spherical", 3, k=768),
    ("krig_local_slab_kernel", (3, 31)): Case("matern32", 3, k=257, ball=True),
    # ---- krig_local_big_kernel
    ("krig_local_big_kernel", (1,)): Case("spherical", 1, k=769),
    ("krig_local_big_kernel", (2,)): Case("exponential", 2, k=769),
    ("krig_local_big_kernel", (3,)): Case("cubic", 3, k=769, ball=True),
}
