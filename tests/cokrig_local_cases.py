"""Case table of the moving-neighbourhood cokriging tests (tests/test_gpu_cokriging_local.py on the device,
tests/test_cokriging_local_host.py for the conditioning cap and the census).  A case is a dict: structure (the keywords
of cokrig_local_ref.Model), B0, B1, x, z, var, xdom, k, variant, means and the search (minneighbors, radius, radii,
rotation).  Units, tolerance and cap are those of tests/cokrig_cases.py: the largest diagonal of B0 + B1 is 1, the bar
is TOL = 1e-9 (1 + |value|), and cond_2 of every per-point system stays <= COND_CAP (the Gaussian cases too: a nugget
of 0.1 and a lattice spacing of 0.7 ranges keep them near 20).  Samples are jittered lattices,
so no two keys tie inside a variable.

KERNELS names, for every compiled instantiation cokrig_local_kernel<DIM, KIND, NT>, the case that launches it
(tests/test_cokriging_local_host.py holds the table against the built library): NT = 1 / 2 / 4 for sum k <= 16 / 32 / 64;
KIND 0 Gaussian, 1 exponential, 2 spherical, 30 / 31 / 32 Matern 1/2, 3/2, 5/2, -1 any other model; 1-D has the general
kernel only.
"""
import numpy as np

import cokrig_cases as CC

B1_2 = np.array([[0.9, 0.5], [0.5, 0.7]])
B0_2 = np.array([[0.1, 0.03], [0.03, 0.08]])


def _case(structure, B0, B1, x, var, xdom, k, seed, variant="ordinary", means=None, **search):
    c = CC._case(structure, B0, B1, x, var, xdom, seed, variant, means)
    if means is not None:
        c["z"] = c["z"] + np.asarray(means)[c["var"]]
    c["k"] = tuple(int(v) for v in k)
    c["search"] = dict(minneighbors=1, radius=None, radii=None, rotation=None)
    c["search"].update(search)
    return c


def two_vars(dim, n0, n1, seed, spacing=10.0):
    """Heterotopic samples of two variables on one jittered lattice, shuffled row order."""
    dims = {1: (n0 + n1,), 2: (15, 14), 3: (6, 6, 6)}[dim]
    loc = CC.lattice(dims, spacing, seed)
    rng = np.random.default_rng(seed + 1)
    loc = loc[rng.permutation(loc.shape[0])[:n0 + n1]]
    var = rng.permutation(np.repeat([0, 1], [n0, n1]))
    return loc, var, rng


def tiles(k):
    """nz = 2, 2-D, about 200 samples, m = 5 (the last workgroup of four waves is partly idle)."""
    loc, var, rng = two_vars(2, 90, 110, 100)
    xdom = rng.uniform(20.0, 120.0, (5, 2))
    return _case(dict(kind="exponential", range=25.0), B0_2, B1_2, loc, var, xdom, k, 102)


STRUCT = {0: dict(kind="gaussian", range=14.0), 1: dict(kind="exponential", range=25.0),
          2: dict(kind="spherical", range=30.0), 30: dict(kind="matern", range=25.0, nu=0.5),
          31: dict(kind="matern", range=26.0, nu=1.5), 32: dict(kind="matern", range=22.0, nu=2.5)}
GENERAL = {1: dict(kind="pentaspherical", range=30.0), 2: dict(kind="cubic", range=24.0),
           3: dict(kind="pentaspherical", range=30.0)}
K_OF_NT = {1: (8, 8), 2: (9, 8), 4: (17, 16)}


def kernel_case(dim, kind, nt):
    """The case of cokrig_local_kernel<dim, kind, nt>: two variables, k at the low end of the size class (ragged last
    tile) or full tiles, m = 6."""
    seed = 1000 + 100 * dim + 3 * (kind if kind >= 0 else 7) + nt
    n = {1: (40, 50), 2: (90, 110), 3: (100, 116)}[dim]
    loc, var, rng = two_vars(dim, n[0], n[1], seed)
    lo, hi = loc.min(axis=0) + 15.0, loc.max(axis=0) - 15.0
    xdom = rng.uniform(lo, hi, (6, dim))
    structure = dict(STRUCT[kind]) if kind >= 0 else dict(GENERAL[dim])
    k = K_OF_NT[nt] if (dim + nt) % 2 else {1: (8, 8), 2: (16, 16), 4: (32, 32)}[nt]
    B0 = B0_2 if kind != 0 else np.diag([0.1, 0.08])
    return _case(structure, B0, B1_2, loc, var, xdom, k, seed + 2)


KERNELS = {(dim, kind, nt): (lambda d=dim, q=kind, t=nt: kernel_case(d, q, t))
           for dim in (2, 3) for kind in (-1, 0, 1, 2, 30, 31, 32) for nt in (1, 2, 4)}
KERNELS.update({(1, -1, nt): (lambda t=nt: kernel_case(1, -1, t)) for nt in (1, 2, 4)})


def four_vars():
    """nz = 4, heterotopic counts (12, 30, 50, 70) in shuffled row order, 3-D; k = (5, 9, 12, 16) -> sum 42."""
    loc = CC.lattice((6, 6, 6), 10.0, 200)
    rng = np.random.default_rng(201)
    loc = loc[rng.permutation(216)[:162]]
    var = rng.permutation(np.repeat([0, 1, 2, 3], [12, 30, 50, 70]))
    xdom = rng.uniform(10.0, 40.0, (9, 3))
    B0 = np.diag([0.1, 0.05, 0.02, 0.08])
    return _case(dict(kind="spherical", range=30.0), B0, CC.b1_of(4), loc, var, xdom, (5, 9, 12, 16), 202)


def simple_means():
    loc, var, rng = two_vars(2, 70, 90, 210)
    xdom = rng.uniform(20.0, 120.0, (7, 2))
    B0 = np.array([[0.15, 0.05], [0.05, 0.1]])
    return _case(dict(kind="exponential", range=24.0), B0, B1_2, loc, var, xdom, (10, 12), 212, "simple",
                 means=[2.5, -1.0])


def rotated():
    """A rotated MetricBall structure; plain k-NN (the searches run on the covariance frame)."""
    a = 0.6
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    loc, var, rng = two_vars(2, 80, 100, 220)
    xdom = rng.uniform(20.0, 120.0, (7, 2))
    B1 = np.array([[0.9, -0.4], [-0.4, 0.8]])
    return _case(dict(kind="exponential", radii=(40.0, 16.0), rotation=R), np.diag([0.1, 0.1]), B1, loc, var, xdom,
                 (12, 12), 222)


def short_lists(variant="ordinary"):
    """A ball of radius 14 around points of which some lie in a region where only variable 1 was sampled, some far from
    every sample, some in the middle of both: with k = (3, 3) and minneighbors = 2 all four outcomes occur."""
    loc = CC.lattice((14, 10), 10.0, 230)
    rng = np.random.default_rng(231)
    left = loc[:, 0] < 60.0
    var = np.where(left, rng.integers(0, 2, loc.shape[0]), 1)          # variable 0 only on the left half
    xdom = np.concatenate([rng.uniform((15.0, 15.0), (45.0, 75.0), (6, 2)),       # both variables around
                           rng.uniform((95.0, 15.0), (120.0, 75.0), (6, 2)),      # variable 1 only
                           np.array([[160.0, 40.0], [139.5, 101.0], [-20.0, -20.0]])])   # nothing / fewer than 2
    means = [0.4, -0.2] if variant == "simple" else None
    return _case(dict(kind="spherical", range=30.0), B0_2, B1_2, loc, var, xdom, (3, 3), 232, variant, means,
                 minneighbors=2, radius=14.0)


def collocated():
    """Variable 0 at all 80 locations, variable 1 at the first 60 of them: collocated pairs meet through the cross nugget
    on a zero key inside the tile.  The domain is five of the locations that hold variable 0 only."""
    loc = CC.lattice((10, 8), 10.0, 240)
    x = np.concatenate([loc, loc[:60]])
    var = np.repeat([0, 1], [80, 60])
    B0 = np.array([[0.1, 0.04], [0.04, 0.12]])
    B1 = np.array([[0.9, 0.45], [0.45, 0.75]])
    return _case(dict(kind="matern", range=26.0, nu=1.5), B0, B1, x, var, loc[62:67].copy(), (10, 10), 242)


def single(variant="ordinary"):
    loc = CC.lattice((12, 10), 10.0, 250)
    xdom = np.random.default_rng(251).uniform(10.0, 100.0, (9, 2))
    return _case(dict(kind="exponential", range=25.0), [[0.15]], [[0.85]], loc, np.zeros(120, dtype=np.int32), xdom,
                 (20,), 252, variant, means=[0.7] if variant == "simple" else None)


def intrinsic():
    """B0 = 0.2 B1, isotopic, equal k: each variable is its own moving-neighbourhood kriging."""
    loc = CC.lattice((11, 9), 10.0, 260)
    x = np.concatenate([loc, loc])
    var = np.repeat([0, 1], 99)
    xdom = np.random.default_rng(261).uniform(10.0, 90.0, (9, 2))
    B1 = np.array([[1.0, 0.55], [0.55, 0.8]])
    return _case(dict(kind="spherical", range=28.0), 0.2 * B1, B1, x, var, xdom, (12, 12), 262)


def global_limit(variant="ordinary"):
    """k[a] = every variable's count, no ball, n = 60 <= 64: the moving neighbourhood IS the global one."""
    loc = CC.lattice((8, 8), 10.0, 270)
    rng = np.random.default_rng(271)
    loc = loc[rng.permutation(64)[:60]]
    var = rng.permutation(np.repeat([0, 1], [22, 38]))
    xdom = rng.uniform(0.0, 70.0, (11, 2))
    return _case(dict(kind="exponential", range=25.0), B0_2, B1_2, loc, var, xdom, (22, 38), 272, variant,
                 means=[0.3, 1.1] if variant == "simple" else None)


def chunks():
    """m = 600 points: three chunks under a cap of 256."""
    loc, var, rng = two_vars(3, 100, 116, 280)
    xdom = rng.uniform(5.0, 45.0, (600, 3))
    return _case(dict(kind="spherical", range=30.0), B0_2, B1_2, loc, var, xdom, (8, 11), 282)


CASES = {"tiles_8_8": lambda: tiles((8, 8)), "tiles_9_8": lambda: tiles((9, 8)), "tiles_16_16": lambda: tiles((16, 16)),
         "tiles_17_16": lambda: tiles((17, 16)), "tiles_32_32": lambda: tiles((32, 32)), "four_vars": four_vars,
         "simple_means": simple_means, "rotated": rotated, "short_ok": short_lists,
         "short_sk": lambda: short_lists("simple"), "collocated": collocated, "single_ok": single,
         "single_sk": lambda: single("simple"), "intrinsic": intrinsic, "global_ok": global_limit,
         "global_sk": lambda: global_limit("simple"), "chunks": chunks}
CASES.update({"kernel_%d_%d_%d" % key: fn for key, fn in KERNELS.items()})
