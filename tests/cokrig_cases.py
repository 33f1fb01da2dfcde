"""Case table of the cokriging tests (tests/test_gpu_cokriging.py on the device, tests/test_cokriging_host.py for the
conditioning cap).  Every case is a dict: structure (the keywords of cokrig_ref.Model), B0, B1, x, z, var, xdom,
variant, means.  Units: the largest diagonal of B0 + B1 is 1, which is what the 1e-9 (1 + |value|) bar refers to.

The bar only means something while the numpy reference is itself good to well under it, so every case keeps
cond_2 of its full constrained matrix <= COND_CAP (LAPACK's own error is then ~1e-11): jittered lattices with a minimum
separation of about a quarter of the range, exponential / spherical / Matern-3/2 structures, B1 with its smallest
eigenvalue >= 0.05 of its largest.  A case that breaks the cap gets another geometry, never another cap.  The Gaussian
case is apart (GAUSSIAN): nugget on the diagonal of B0, held at the 1e-6 DESIGN.md gives Gaussian systems, cap not
asserted.
"""
import numpy as np

COND_CAP = 1e5
TOL = 1e-9
TOL_GAUSSIAN = 1e-6


def lattice(dims, spacing, seed, jitter=0.2):
    """Jittered lattice: points at least (1 - 2 jitter) spacing apart."""
    rng = np.random.default_rng(seed)
    axes = [np.arange(d) * spacing for d in dims]
    g = np.stack([a.ravel() for a in np.meshgrid(*axes, indexing="ij")], axis=1)
    return g + rng.uniform(-jitter * spacing, jitter * spacing, g.shape)


def unit_scale(B0, B1):
    s = np.max(np.diag(B0) + np.diag(B1))
    return np.asarray(B0) / s, np.asarray(B1) / s


def b1_of(nz, common=0.4):
    """(1 - common) I + common 11': eigenvalues 1 - common (nz - 1 times) and 1 - common + nz common."""
    return (1.0 - common) * np.eye(nz) + common * np.ones((nz, nz))


def values(x, var, seed):
    """Smooth per-variable surfaces plus noise: O(1) values with a different level per variable."""
    rng = np.random.default_rng(seed)
    s = np.sin(0.07 * x.sum(axis=1) + var) + 0.5 * np.cos(0.05 * x[:, 0] - 0.3 * var)
    return s + 0.3 * var + 0.2 * rng.normal(size=x.shape[0])


def _case(structure, B0, B1, x, var, xdom, seed, variant="ordinary", means=None):
    B0, B1 = unit_scale(np.asarray(B0, dtype=np.float64), np.asarray(B1, dtype=np.float64))
    x = np.ascontiguousarray(x, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.int32)
    return dict(structure=structure, B0=B0, B1=B1, x=x, z=values(x, var, seed), var=var,
                xdom=np.ascontiguousarray(xdom, dtype=np.float64), variant=variant, means=means)


def iso2d():
    """2-D, nz = 2, isotopic: 63 locations -> n = 126, N1 = 128 (the dual-weight row opens a second 128-row block);
    m = 257 is one past a 256 block."""
    loc = lattice((9, 7), 10.0, 1)
    x = np.concatenate([loc, loc])
    var = np.repeat([0, 1], 63)
    xdom = np.random.default_rng(2).uniform(-5.0, 85.0, (257, 2))
    B1 = np.array([[0.9, 0.5], [0.5, 0.7]])
    B0 = np.array([[0.1, 0.03], [0.03, 0.08]])
    return _case(dict(kind="exponential", range=25.0), B0, B1, x, var, xdom, 3)


def hetero3d():
    """3-D, nz = 3, heterotopic counts (5, 40, 90) in shuffled row order: N1 = 138, n = 135 is no multiple of the 4 row
    segments; m = 700 is past one 512-point unit."""
    loc = lattice((5, 5, 6), 10.0, 4)
    rng = np.random.default_rng(5)
    loc = loc[rng.permutation(150)[:135]]
    var = rng.permutation(np.repeat([0, 1, 2], [5, 40, 90]))
    xdom = rng.uniform(-5.0, 55.0, (700, 3))
    B1 = np.array([[0.8, 0.3, -0.2], [0.3, 0.7, 0.1], [-0.2, 0.1, 0.9]])
    B0 = np.diag([0.1, 0.05, 0.02])
    return _case(dict(kind="spherical", range=30.0), B0, B1, loc, var, xdom, 6)


def many1d():
    """1-D, nz = 8, counts 1 .. 8 (n = 36): the largest nz, a variable with a single sample; m = 1 is the clamped
    padding point."""
    loc = lattice((36,), 10.0, 7)
    rng = np.random.default_rng(8)
    var = rng.permutation(np.repeat(np.arange(8), np.arange(1, 9)))
    xdom = np.array([[123.4]])
    return _case(dict(kind="matern", range=28.0, nu=1.5), 0.05 * np.eye(8), b1_of(8), loc, var, xdom, 9)


def single(variant="ordinary"):
    """nz = 1, n = 50: a kriging system with sill = b0 + b1, nugget = b0."""
    loc = lattice((10, 5), 10.0, 10)
    xdom = np.random.default_rng(11).uniform(0.0, 90.0, (300, 2))
    return _case(dict(kind="exponential", range=25.0), [[0.15]], [[0.85]], loc, np.zeros(50, dtype=np.int32), xdom, 12,
                 variant, means=[0.7] if variant == "simple" else None)


def intrinsic():
    """B0 = 0.2 B1, isotopic, nz = 2: autokrigeable."""
    loc = lattice((8, 6), 10.0, 13)
    x = np.concatenate([loc, loc])
    var = np.repeat([0, 1], 48)
    xdom = np.random.default_rng(14).uniform(0.0, 70.0, (200, 2))
    B1 = np.array([[1.0, 0.55], [0.55, 0.8]])
    return _case(dict(kind="spherical", range=28.0), 0.2 * B1, B1, x, var, xdom, 15)


def simple_means():
    """Simple variant with unequal means; the last four domain points are far from all data."""
    loc = lattice((7, 7), 10.0, 16)
    rng = np.random.default_rng(17)
    var = rng.permutation(np.repeat([0, 1], [20, 29]))
    xdom = np.concatenate([rng.uniform(0.0, 60.0, (150, 2)), 1e4 + rng.uniform(0.0, 60.0, (4, 2))])
    B1 = np.array([[0.85, 0.4], [0.4, 0.6]])
    B0 = np.array([[0.15, 0.05], [0.05, 0.1]])
    c = _case(dict(kind="exponential", range=24.0), B0, B1, loc, var, xdom, 18, "simple", means=[2.5, -1.0])
    c["z"] = c["z"] + np.asarray(c["means"])[c["var"]]
    return c


def on_samples():
    """Variable 0 at 40 locations, variable 1 at the first 25 of them and at 20 others; the domain is the 15 locations
    where variable 0 was measured and variable 1 was not."""
    loc = lattice((10, 6), 10.0, 19)
    x = np.concatenate([loc[:40], loc[:25], loc[40:60]])
    var = np.repeat([0, 1], [40, 45])
    B1 = np.array([[0.9, 0.45], [0.45, 0.75]])
    B0 = np.array([[0.1, 0.04], [0.04, 0.12]])
    return _case(dict(kind="matern", range=26.0, nu=1.5), B0, B1, x, var, loc[25:40].copy(), 20)


def rotated():
    """Rotated MetricBall structure, 2-D, nz = 2, heterotopic."""
    a = 0.6
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    loc = lattice((8, 8), 10.0, 21)
    rng = np.random.default_rng(22)
    var = rng.permutation(np.repeat([0, 1], [24, 40]))
    xdom = rng.uniform(0.0, 70.0, (300, 2))
    B1 = np.array([[0.9, -0.4], [-0.4, 0.8]])
    B0 = np.array([[0.1, 0.0], [0.0, 0.1]])
    return _case(dict(kind="exponential", radii=(40.0, 16.0), rotation=R), B0, B1, loc, var, xdom, 23)


def gaussian():
    """The Gaussian case: a nugget on the diagonal of B0, a wider lattice relative to the range."""
    loc = lattice((7, 6), 10.0, 24)
    rng = np.random.default_rng(25)
    var = rng.permutation(np.repeat([0, 1], [17, 25]))
    xdom = rng.uniform(0.0, 60.0, (200, 2))
    B1 = np.array([[0.9, 0.4], [0.4, 0.7]])
    B0 = np.diag([0.1, 0.08])
    return _case(dict(kind="gaussian", range=18.0), B0, B1, loc, var, xdom, 26)


CASES = {"iso2d": iso2d, "hetero3d": hetero3d, "many1d": many1d, "single_ok": single,
         "single_sk": lambda: single("simple"), "intrinsic": intrinsic, "simple_means": simple_means,
         "on_samples": on_samples, "rotated": rotated}
GAUSSIAN = {"gaussian": gaussian}


def location_folds(x, nfolds, seed):
    """Fold ids that keep the samples of one location together: locations are dealt to `nfolds` folds at random."""
    _, inv = np.unique(np.asarray(x), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    deal = np.random.default_rng(seed).integers(0, nfolds, inv.max() + 1)
    return np.ascontiguousarray(deal[inv], dtype=np.int32)
