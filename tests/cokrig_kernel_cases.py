"""One case per compiled (DIM, KIND) of the global-cokriging kernels cokrig_rhs_kernel and cokrig_batch_mean_kernel
(csrc/cokrig.hip, launch_cokrig_rhs; csrc/cokrig_batch.hip, launch_cokrig_batch_mean: one switch on the device kind of
the structure), built with cokrig_cases._case and lattice.  tests/test_cokrig_census.py holds the table against the
built library and the conditioning cap; tests/test_gpu_cokriging.py and tests/test_gpu_cokriging_batch.py run every entry.

    KERNELS = {(DIM, KIND): a function that builds the case}

KIND 0 Gaussian, 1 exponential, 2 spherical, 30 / 31 / 32 Matern 1/2, 3/2, 5/2, -1 any other model (cubic and
pentaspherical here, through cokrig_local_ref.Model).  Every case: 84 samples of two or three heterotopic variables
(three for the spherical and the general entries, so in every dimension) on a jittered lattice in shuffled row order,
a positive B0 with a cross nugget, m = 517 domain points (odd and past one 512-point unit of cokrig_rhs_kernel, whose
last pair of points is clamped at m - 1), of which the first three sit exactly on samples (the zero-key select), and the
ordinary and the simple variant with unequal means by turns.  Units, tolerance and cap are those of
tests/cokrig_cases.py: cond_2 <= COND_CAP for every entry, the Gaussian ones included (a lattice spacing of 0.7 ranges).
"""
import numpy as np

import cokrig_cases as CC
import cokrig_local_ref as LR
import cokrig_ref as CR

KINDS = (-1, 0, 1, 2, 30, 31, 32)
STRUCT = {0: dict(kind="gaussian", range=14.0), 1: dict(kind="exponential", range=25.0),
          2: dict(kind="spherical", range=30.0), 30: dict(kind="matern", range=25.0, nu=0.5),
          31: dict(kind="matern", range=26.0, nu=1.5), 32: dict(kind="matern", range=22.0, nu=2.5)}
GENERAL = {1: dict(kind="pentaspherical", range=30.0), 2: dict(kind="cubic", range=24.0),
           3: dict(kind="pentaspherical", range=28.0)}
# the kind a case must be told apart from (same range)
NEIGHBOUR = {0: dict(kind="exponential"), 1: dict(kind="gaussian"), 2: dict(kind="exponential"),
             30: dict(kind="matern", nu=1.5), 31: dict(kind="matern", nu=2.5), 32: dict(kind="matern", nu=1.5),
             -1: dict(kind="spherical")}
N, M, ON = 84, 517, 3
B1 = {2: np.array([[0.9, 0.5], [0.5, 0.7]]), 3: np.array([[0.8, 0.3, -0.2], [0.3, 0.7, 0.1], [-0.2, 0.1, 0.9]])}
B0 = {2: np.array([[0.1, 0.03], [0.03, 0.08]]),
      3: np.array([[0.1, 0.02, 0.01], [0.02, 0.05, 0.01], [0.01, 0.01, 0.08]])}
MEANS = {2: [2.5, -1.0], 3: [2.5, -1.0, 0.5]}


def seed_of(dim, kind):
    return 3000 + 100 * dim + 3 * (kind if kind >= 0 else 7)


def kernel_case(dim, kind, structure=None):
    """The case of cokrig_rhs_kernel<dim, kind> and cokrig_batch_mean_kernel<dim, kind> (`structure`: keywords that
    replace the kind, for the discrimination check)."""
    seed = seed_of(dim, kind)
    nz = 3 if kind in (2, -1) else 2
    dims = {1: (96,), 2: (10, 9), 3: (5, 4, 5)}[dim]
    loc = CC.lattice(dims, 10.0, seed)
    rng = np.random.default_rng(seed + 1)
    loc = loc[rng.permutation(loc.shape[0])[:N]]
    counts = [20, 64] if nz == 2 else [12, 30, 42]
    var = rng.permutation(np.repeat(np.arange(nz), counts))
    lo, hi = loc.min(axis=0) - 5.0, loc.max(axis=0) + 5.0
    xdom = rng.uniform(lo, hi, (M, dim))
    on = np.array([np.flatnonzero(var == a)[0] for a in range(nz)] + [np.flatnonzero(var == 0)[1]])[:ON]
    xdom[:ON] = loc[on]                                        # exactly on samples of one variable each
    s = dict(STRUCT[kind]) if kind >= 0 else dict(GENERAL[dim])
    if structure is not None:
        s = dict(range=s["range"], **structure)
    simple = (len(KINDS) * (dim - 1) + KINDS.index(kind)) % 2 == 1
    c = CC._case(s, B0[nz], B1[nz], loc, var, xdom, seed + 2, "simple" if simple else "ordinary",
                 MEANS[nz] if simple else None)
    if simple:
        c["z"] = c["z"] + np.asarray(c["means"])[c["var"]]
    c["seed"] = seed + 2
    c["on"] = on                                               # sample rows the first domain points sit on
    return c


def model_of(c):
    cls = LR.Model if c["structure"]["kind"] in ("cubic", "pentaspherical") else CR.Model
    return cls(c["structure"], c["B0"], c["B1"])


def batch_of(c, nbatch):
    """Value vectors of a batch: vector 0 is the case's own data, vector r the surfaces of seed + r."""
    shift = np.asarray(c["means"], dtype=np.float64)[c["var"]] if c["means"] is not None else 0.0
    return np.stack([CC.values(c["x"], c["var"], c["seed"] + r) + shift for r in range(nbatch)])


KERNELS = {(dim, kind): (lambda d=dim, q=kind: kernel_case(d, q)) for dim in (1, 2, 3) for kind in KINDS}
