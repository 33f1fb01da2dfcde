"""One case per compiled instantiation of the neighbour-search kernels (csrc/knn.hip, csrc/knn_build.hip) and of the
IDW / LWR kernels built on them (csrc/idw_lwr.hip).

tests/test_search_census.py holds this table against the kernels the compiler emitted into libgss_hip.so
(tools/kernel_census.py): every compiled kernel of FAMILIES has exactly one entry and every entry names a compiled
kernel.  An entry is a Case, or UNREACHABLE("reason citing the .hip dispatch line").  tests/test_gpu_search_matrix.py
runs every Case on the device: neighbour indices and counts for equality against the integer ranking of
tests/search_matrix.py, estimates against its 50-digit answers within BARS.

Keys are (kernel family, template arguments as the demangler prints them).  Which rule picks an instantiation:
 * Searcher::query (knn.hip) takes the exhaustive knn_kernel<DIM, METRIC> for the haversine key (METRIC 3: no box
   bounds; Searcher::init admits it in 2-D only), with GSS_KNN_BRUTE=1 (route "brute"), and for a one-shot search of
   m <= 4096 centres in n >= 32768 samples (route "few"); never for k > 64 or a masked query, except haversine, whose
   passes of 64 run on the exhaustive kernel.  METRIC: 0 Euclidean, 1 cityblock, 2 Chebyshev.
 * Searcher::pass launches knn_pruned_kernel<DIM, MASKED, METRIC> otherwise: MASKED with the ranks of a sequential
   simulation (only an SGS handle passes them; lists read back with SGSHandle.weights(), mask_after_search=False).
 * k > 64: Searcher::query runs passes of 64 between knn_any_init_kernel and knn_any_append_kernel<DIM>.
 * Searcher::index orders n >= 16384 samples on the device (the kd_* kernels of knn_build.hip; GSS_KNN_BUILD=device /
   host forces one path; `build` below).  kd_bbox / kd_keys need more than one batch (n > 64).
 * est_local_dev (idw_lwr.hip): k <= 16 est_knn_kernel<DIM, 16>, 17..64 <DIM, 64>; 65 <= k < n est_list_kernel<DIM, ZC>;
   k = n > 64: idw_all_fast_kernel<DIM, E1> (one column, Euclidean, no ball, exponent 1 -> E1 true, 2 -> false),
   lwr_all_fast_kernel<DIM> (one column, Euclidean, no ball, exp weight with p = 2), else est_all_kernel<DIM, ZC>;
   ZC = 4 for several value columns, 1 for one.
"""
from dataclasses import dataclass
from typing import Tuple


@dataclass(frozen=True)
class Case:
    op: str                     # "search", "masked" (SGS handle), "idw", "lwr"
    dim: int
    n: int                      # samples (masked: cells, every one a query)
    k: int
    m: int = 0                  # queries
    metric: str = "euclidean"   # "cityblock", "chebyshev", "haversine"
    ball: str = ""              # "radius", "radii", "rotated" (radii turned by a signed permutation)
    ballx: int = 2              # ball size in lattice spacings (a power of two for radii)
    route: str = "index"        # "brute": GSS_KNN_BRUTE=1, "few": the few-queries rule
    build: str = ""             # "host" / "device": GSS_KNN_BUILD, "both": once each
    path: str = "random"        # masked: "random" permutation or lexicographic "sweep" (whole batches stay unsimulated)
    nd: int = 0                 # masked: conditioning cells (rank -1)
    nz: int = 1                 # value columns
    exponent: float = 1.0       # IDW
    weight: Tuple = (0, 3.0, 2.0)   # LWR (kind, a, p): exp(-a h^p), or (1, 0, 0) tricube
    minn: int = 1
    expect: Tuple = ()          # edges the reference answer must show (search_matrix.assert_expectations)


@dataclass(frozen=True)
class UNREACHABLE:
    reason: str


SEARCH_FAMILIES = ("knn_kernel", "knn_pruned_kernel", "knn_any_append_kernel", "knn_any_init_kernel",
                   "kd_init_kernel", "kd_bbox_kernel", "kd_keys_kernel", "kd_gather_kernel", "kd_boxes_kernel")
EST_FAMILIES = ("est_knn_kernel", "est_list_kernel", "est_all_kernel", "idw_all_fast_kernel", "lwr_all_fast_kernel")
FAMILIES = SEARCH_FAMILIES + EST_FAMILIES

# Tolerances tests/test_gpu_idw_lwr.py already holds the same quantities to (relative to 1 + |value|): no bar is looser.
EXISTING_TOL = {"idw_mean": 1e-10, "idw_aux": 1e-10, "lwr_mean": 1e-9, "lwr_aux": 1e-9}

# Error bars in units of 2^-53 x the data scale (search_matrix.scales: the largest |value| for the means, the largest
# auxiliary output, at least 1, for the distance / norm column).  "oracle": the largest error of oracle.idw_lwr (FP64)
# against the 50-digit answer over the family's cases, measured with tools/search_matrix_oracle.py; "bar" = 16 x that
# with a floor of 8 (the device sums in another order and has its own pow, exp and sqrt), never looser than
# EXISTING_TOL.  The measurement is of the oracle, never of the device.
BARS = {
    "est_knn_kernel": {
        "idw_aux": {"oracle": 1.62, "bar": 25.9},
        "idw_mean": {"oracle": 2.89, "bar": 46.3},
        "lwr_aux": {"oracle": 848.30, "bar": 13572.8},
        "lwr_mean": {"oracle": 168.16, "bar": 2690.6},
    },
    "est_list_kernel": {
        "idw_aux": {"oracle": 0.00, "bar": 8.0},
        "idw_mean": {"oracle": 3.93, "bar": 62.8},
        "lwr_aux": {"oracle": 5.50, "bar": 88.0},
        "lwr_mean": {"oracle": 11.68, "bar": 186.8},
    },
    "est_all_kernel": {
        "idw_aux": {"oracle": 0.00, "bar": 8.0},
        "idw_mean": {"oracle": 2.97, "bar": 47.6},
        "lwr_aux": {"oracle": 13.50, "bar": 216.0},
        "lwr_mean": {"oracle": 9.32, "bar": 149.1},
    },
    "idw_all_fast_kernel": {
        "idw_aux": {"oracle": 0.00, "bar": 8.0},
        "idw_mean": {"oracle": 2.97, "bar": 47.6},
    },
    "lwr_all_fast_kernel": {
        "lwr_aux": {"oracle": 3.25, "bar": 52.0},
        "lwr_mean": {"oracle": 8.92, "bar": 142.7},
    },
}

HAV = "Searcher::init (knn.hip: GSS_REQUIRE(dim_ == 2, \"the haversine distance needs (longitude, latitude) points\")) " \
      "rejects the haversine key outside 2-D before any launch of Searcher::pass"
B, S, E, F = "boundary", "short", "empty", "full"

CASES = {
    # ---- knn_kernel<DIM, METRIC>: the exhaustive search
    ("knn_kernel", (1, 0)): Case("search", 1, 63, 1, m=1, route="brute"),
    ("knn_kernel", (1, 1)): Case("search", 1, 64, 7, m=5, metric="cityblock", route="brute"),
    ("knn_kernel", (1, 2)): Case("search", 1, 65, 8, m=13, metric="chebyshev", route="brute"),
    ("knn_kernel", (1, 3)): UNREACHABLE(HAV),
    ("knn_kernel", (2, 0)): Case("search", 2, 4095, 12, m=37, ball="radius", route="brute", expect=(B, S, E)),
    ("knn_kernel", (2, 1)): Case("search", 2, 4097, 63, m=50, metric="cityblock", route="brute", expect=("ties",)),
    ("knn_kernel", (2, 2)): Case("search", 2, 4096, 64, m=33, metric="chebyshev", route="brute", expect=("ties",)),
    ("knn_kernel", (2, 3)): Case("search", 2, 500, 70, m=40, metric="haversine"),
    ("knn_kernel", (3, 0)): Case("search", 3, 32768, 12, m=100, ball="radii", ballx=1, route="few", expect=(B, S, E)),
    ("knn_kernel", (3, 1)): Case("search", 3, 4097, 1, m=1, metric="cityblock", route="brute"),
    ("knn_kernel", (3, 2)): Case("search", 3, 65, 64, m=7, metric="chebyshev", route="brute"),
    ("knn_kernel", (3, 3)): UNREACHABLE(HAV),
    # ---- knn_pruned_kernel<DIM, false, METRIC>: the indexed search
    ("knn_pruned_kernel", (1, "false", 0)): Case("search", 1, 4096, 65, m=21, expect=("tie64",)),
    ("knn_pruned_kernel", (1, "false", 1)): Case("search", 1, 63, 63, m=9, metric="cityblock"),
    ("knn_pruned_kernel", (1, "false", 2)): Case("search", 1, 4097, 128, m=17, metric="chebyshev"),
    ("knn_pruned_kernel", (2, "false", 0)): Case("search", 2, 20000, 12, m=1000, ball="rotated", build="both",
                                                 expect=(B, S, E, F)),
    ("knn_pruned_kernel", (2, "false", 1)): Case("search", 2, 4095, 129, m=10, metric="cityblock"),
    ("knn_pruned_kernel", (2, "false", 2)): Case("search", 2, 64, 7, m=3, metric="chebyshev"),
    # more than 64 groups of 64 batches: the outer box-group loop of the kernel takes a second round
    ("knn_pruned_kernel", (3, "false", 0)): Case("search", 3, 300000, 8, m=5000,
                                                 expect=("ties", "on_sample", "last_group")),
    ("knn_pruned_kernel", (3, "false", 1)): Case("search", 3, 4096, 200, m=19, metric="cityblock"),
    ("knn_pruned_kernel", (3, "false", 2)): Case("search", 3, 16384, 64, m=999, metric="chebyshev"),
    # ---- knn_pruned_kernel<DIM, true, METRIC>: masked by the visiting ranks of a sequential simulation
    ("knn_pruned_kernel", (1, "true", 0)): Case("masked", 1, 4097, 7, path="sweep", expect=("rank0",)),
    ("knn_pruned_kernel", (1, "true", 1)): Case("masked", 1, 65, 64, metric="cityblock", nd=3),
    ("knn_pruned_kernel", (1, "true", 2)): Case("masked", 1, 4096, 65, metric="chebyshev", expect=("rank0",)),
    ("knn_pruned_kernel", (2, "true", 0)): Case("masked", 2, 4095, 12, ball="radii", path="sweep", nd=5, expect=(S, E)),
    ("knn_pruned_kernel", (2, "true", 1)): Case("masked", 2, 64, 8, metric="cityblock", expect=("rank0",)),
    ("knn_pruned_kernel", (2, "true", 2)): Case("masked", 2, 4097, 128, metric="chebyshev", path="sweep", nd=4),
    ("knn_pruned_kernel", (3, "true", 0)): Case("masked", 3, 20000, 63, path="sweep", nd=10),
    ("knn_pruned_kernel", (3, "true", 1)): Case("masked", 3, 4096, 1, metric="cityblock", expect=("rank0",)),
    ("knn_pruned_kernel", (3, "true", 2)): Case("masked", 3, 65, 7, metric="chebyshev", nd=2),
    # ---- passes of 64
    ("knn_any_append_kernel", (1,)): Case("search", 1, 4097, 200, m=23, ball="radius", ballx=64, expect=(B, S, E)),
    ("knn_any_append_kernel", (2,)): Case("search", 2, 4096, 129, m=11, ball="radii", ballx=8, expect=(S, E)),
    ("knn_any_append_kernel", (3,)): Case("search", 3, 4095, 65, m=6, metric="cityblock"),
    ("knn_any_init_kernel", ()): Case("search", 2, 65, 65, m=1),
    # ---- the device-side k-d ordering (knn_build.hip)
    ("kd_init_kernel", ()): Case("search", 2, 63, 7, m=5, build="device"),
    ("kd_bbox_kernel", (1,)): Case("search", 1, 20000, 8, m=333),
    ("kd_bbox_kernel", (2,)): Case("search", 2, 4097, 12, m=21, metric="cityblock", build="device"),
    ("kd_bbox_kernel", (3,)): Case("search", 3, 4095, 8, m=10, ball="rotated", ballx=1, build="device",
                                   expect=(B, S, E)),
    ("kd_keys_kernel", (1,)): Case("search", 1, 65, 7, m=5, build="device"),
    ("kd_keys_kernel", (2,)): Case("search", 2, 4095, 63, m=14, metric="chebyshev", build="device"),
    ("kd_keys_kernel", (3,)): Case("search", 3, 4097, 129, m=9, build="device"),
    ("kd_gather_kernel", (1,)): Case("search", 1, 64, 8, m=6, build="device"),
    ("kd_gather_kernel", (2,)): Case("search", 2, 4096, 63, m=30, metric="chebyshev", build="device"),
    ("kd_gather_kernel", (3,)): Case("search", 3, 16385, 12, m=200, ball="radius", ballx=1, expect=(B, S, E)),
    ("kd_boxes_kernel", (1,)): Case("search", 1, 4095, 64, m=12, metric="cityblock", build="device"),
    ("kd_boxes_kernel", (2,)): Case("search", 2, 16384, 1, m=50, ball="radius", ballx=1, expect=(E, F)),
    ("kd_boxes_kernel", (3,)): Case("search", 3, 65, 65, m=4, build="device"),
    # ---- est_knn_kernel<DIM, GW>: GW 16 for k <= 16, 64 for 17..64
    ("est_knn_kernel", (1, 16)): Case("idw", 1, 200, 16, m=30, exponent=1.0, expect=("on_sample",)),
    ("est_knn_kernel", (1, 64)): Case("lwr", 1, 300, 64, m=27, weight=(1, 0.0, 0.0)),
    ("est_knn_kernel", (2, 16)): Case("lwr", 2, 400, 16, m=29, ball="radius", ballx=4, minn=12, expect=("missing",)),
    ("est_knn_kernel", (2, 64)): Case("idw", 2, 300, 17, m=26, metric="haversine", exponent=2.0),
    ("est_knn_kernel", (3, 16)): Case("idw", 3, 500, 16, m=31, nz=5, exponent=3.0, ball="radii", ballx=2, minn=3,
                                      expect=("missing",)),
    ("est_knn_kernel", (3, 64)): Case("lwr", 3, 600, 17, m=25, nz=4, weight=(0, 2.0, 1.0)),
    # ---- est_list_kernel<DIM, ZC>: 65 <= k < n
    ("est_list_kernel", (1, 1)): Case("lwr", 1, 120, 65, m=22),
    ("est_list_kernel", (1, 4)): Case("idw", 1, 80, 79, m=21, nz=5, exponent=2.0, expect=("on_sample",)),
    ("est_list_kernel", (2, 1)): Case("idw", 2, 150, 65, m=23, metric="cityblock", exponent=1.0),
    ("est_list_kernel", (2, 4)): Case("lwr", 2, 90, 89, m=19, nz=4, weight=(1, 0.0, 0.0)),
    ("est_list_kernel", (3, 1)): Case("lwr", 3, 70, 69, m=18, weight=(0, 2.0, 1.0)),
    ("est_list_kernel", (3, 4)): Case("idw", 3, 100, 65, m=26, nz=5, exponent=3.0, ball="radii", ballx=2, minn=3,
                                      expect=("missing",)),
    # ---- est_all_kernel<DIM, ZC>: k = n > 64, whatever the two dedicated kernels do not take
    ("est_all_kernel", (1, 1)): Case("idw", 1, 65, 65, m=21, exponent=3.0, expect=("on_sample",)),
    ("est_all_kernel", (1, 4)): Case("lwr", 1, 70, 70, m=17, nz=4),
    ("est_all_kernel", (2, 1)): Case("lwr", 2, 80, 80, m=19, weight=(1, 0.0, 0.0)),
    ("est_all_kernel", (2, 4)): Case("idw", 2, 90, 90, m=27, nz=5, exponent=1.0, ball="radius", ballx=2, minn=3,
                                     expect=("missing",)),
    ("est_all_kernel", (3, 1)): Case("idw", 3, 66, 66, m=22, metric="cityblock", exponent=2.0),
    ("est_all_kernel", (3, 4)): Case("lwr", 3, 100, 100, m=23, nz=5, ball="radii", ballx=4, minn=20,
                                     expect=("missing",)),
    # ---- idw_all_fast_kernel<DIM, E1>: k = n > 64, Euclidean, no ball, one column, exponent 1 (true) or 2 (false)
    ("idw_all_fast_kernel", (1, "false")): Case("idw", 1, 65, 65, m=21, exponent=2.0, expect=("on_sample",)),
    ("idw_all_fast_kernel", (1, "true")): Case("idw", 1, 97, 97, m=18, exponent=1.0),
    ("idw_all_fast_kernel", (2, "false")): Case("idw", 2, 80, 80, m=25, exponent=2.0),
    ("idw_all_fast_kernel", (2, "true")): Case("idw", 2, 65, 65, m=22, exponent=1.0, expect=("on_sample",)),
    ("idw_all_fast_kernel", (3, "false")): Case("idw", 3, 129, 129, m=19, exponent=2.0),
    ("idw_all_fast_kernel", (3, "true")): Case("idw", 3, 70, 70, m=26, exponent=1.0, expect=("on_sample",)),
    # ---- lwr_all_fast_kernel<DIM>: k = n > 64, Euclidean, no ball, one column, exp(-a h^2)
    ("lwr_all_fast_kernel", (1,)): Case("lwr", 1, 65, 65, m=21),
    ("lwr_all_fast_kernel", (2,)): Case("lwr", 2, 90, 90, m=18),
    ("lwr_all_fast_kernel", (3,)): Case("lwr", 3, 128, 128, m=23),
}


def quantities(case):
    return ("%s_mean" % case.op, "%s_aux" % case.op)
