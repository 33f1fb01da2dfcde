"""Case table of the cokriging cross-validation tests (tests/test_gpu_cokriging_cv.py on the device,
tests/test_cokriging_cv_host.py for the conditioning cap).  A case is a dict of tests/cokrig_local_cases.py -- structure,
B0, B1, x, z, var, k, variant, means, search -- plus `fold` (one id per stacked sample, or None: every sample its own
fold) and `exclude_radius` (None: no ball); its `xdom` is not read, the queries are the samples.  The samples come from
the generators of cokrig_local_cases.py and cokrig_cases.py, so units, tolerance and conditioning cap are theirs: the
largest diagonal of B0 + B1 is 1, the bar is cokrig_cases.TOL (1 + |value|), and every per-sample system keeps
cond_2 <= COND_CAP (a per-sample system is a per-point system of the moving neighbourhood on a subset of the same
jittered lattice).

KERNELS names, for every compiled cokrig_cv_kernel<DIM, KIND, NT>, the case that launches it: the keys of
cokrig_local_cases.KERNELS, k = K_OF_NT[NT] (ragged last tile, the size-class edges), 5 folds of locations.
"""
import numpy as np

import cokrig_cases as CC
import cokrig_local_cases as LC


def _cv(c, fold=None, exclude_radius=None, k=None, **search):
    c = dict(c)
    c["search"] = dict(c["search"], **search)
    if k is not None:
        c["k"] = tuple(int(v) for v in k)
    c["fold"] = None if fold is None else np.ascontiguousarray(fold, dtype=np.int32)
    c["exclude_radius"] = exclude_radius
    return c


def kernel(dim, kind, nt):
    """The samples of cokrig_local_cases.kernel_case (nz = 2, heterotopic, about 200 samples; 90 in 1-D)."""
    c = LC.kernel_case(dim, kind, nt)
    return _cv(c, CC.location_folds(c["x"], 5, 3000 + 100 * dim + nt), k=LC.K_OF_NT[nt])


KERNELS = {key: (lambda q=key: kernel(*q)) for key in LC.KERNELS}


def datum_loo_collocated():
    """fold = None on collocated samples: the partner of the other variable at the query's own location stays eligible
    and meets the right-hand side on a zero key, through the cross nugget."""
    return _cv(LC.collocated())


def location_folds():
    """The same samples, one fold per location: collocated partners leave together."""
    c = LC.collocated()
    _, inv = np.unique(c["x"], axis=0, return_inverse=True)
    return _cv(c, np.asarray(inv).reshape(-1))


def ball_on_radius():
    """An unjittered integer lattice of spacing 10 and exclude_radius = 10: the four axis neighbours of a sample lie
    exactly on the radius (their squared keys are the integer 100 in both implementations) and are left out."""
    g = np.stack([a.ravel() for a in np.meshgrid(np.arange(12) * 10.0, np.arange(10) * 10.0, indexing="ij")], axis=1)
    rng = np.random.default_rng(300)
    var = rng.permutation(np.repeat([0, 1], [50, 70]))
    c = LC._case(dict(kind="exponential", range=25.0), LC.B0_2, LC.B1_2, g, var, g[:1], (6, 6), 301)
    return _cv(c, None, 10.0)


def short_lists(variant="ordinary"):
    """A ball of radius 14, k = (3, 3), minneighbors = 2, and folds under which all four outcomes occur: every sample of
    variable 1 sits in fold 0, so a variable-1 query never finds its own variable (ordinary: MISSING; simple: estimated
    from variable 0) and a variable-0 query of fold 0 finds no variable 1 (its constraint is dropped); variable-0 queries
    of the other folds find both; three isolated samples find nothing (MISSING by minneighbors)."""
    loc = CC.lattice((14, 10), 10.0, 310)
    rng = np.random.default_rng(311)
    x = np.concatenate([loc, np.array([[300.0, 300.0], [-200.0, 50.0], [400.0, -100.0]])])
    var = np.concatenate([rng.integers(0, 2, loc.shape[0]), [0, 0, 0]])
    fold = np.where(var == 1, 0, rng.integers(0, 5, x.shape[0]))
    means = [0.4, -0.2] if variant == "simple" else None
    c = LC._case(dict(kind="spherical", range=30.0), LC.B0_2, LC.B1_2, x, var, x[:1], (3, 3), 312, variant, means,
                 minneighbors=2, radius=14.0)
    return _cv(c, fold)


def four_vars():
    c = LC.four_vars()
    return _cv(c, CC.location_folds(c["x"], 5, 320))


def simple_means():
    c = LC.simple_means()
    return _cv(c, CC.location_folds(c["x"], 5, 330))


def rotated():
    """A rotated structure AND a rotated search ball with an exclusion radius (in the ball's scaled units): the searches
    run on a second frame and read the raw query coordinates."""
    c = LC.rotated()
    a = 0.5
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return _cv(c, CC.location_folds(c["x"], 5, 340), 0.25, radii=(45.0, 18.0), rotation=R)


def global_limit(variant="ordinary"):
    """n = 60, k[a] = every variable's count, no ball, 6 folds by location: the moving neighbourhood is the global one."""
    c = LC.global_limit(variant)
    return _cv(c, CC.location_folds(c["x"], 6, 350))


def chunks():
    """n = 600 stacked samples in 3-D: three chunks under a cap of 256; 10 folds by location."""
    loc = CC.lattice((9, 9, 8), 10.0, 360)
    rng = np.random.default_rng(361)
    loc = loc[rng.permutation(648)[:600]]
    var = rng.permutation(np.repeat([0, 1], [250, 350]))
    c = LC._case(dict(kind="spherical", range=30.0), LC.B0_2, LC.B1_2, loc, var, loc[:1], (8, 11), 362)
    return _cv(c, CC.location_folds(c["x"], 10, 363))


CASES = {"datum_loo_collocated": datum_loo_collocated, "location_folds": location_folds,
         "ball_on_radius": ball_on_radius, "short_ok": short_lists, "short_sk": lambda: short_lists("simple"),
         "four_vars": four_vars, "simple_means": simple_means, "rotated": rotated, "global_ok": global_limit,
         "global_sk": lambda: global_limit("simple"), "chunks": chunks}
CASES.update({"kernel_%d_%d_%d" % key: fn for key, fn in KERNELS.items()})


def tolerance(c):
    return CC.TOL_GAUSSIAN if c["structure"]["kind"] == "gaussian" else CC.TOL
