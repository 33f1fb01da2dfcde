"""Case table of the pair kernels of csrc/variography.hip: one case per compiled instantiation of
vario_window_kernel<DIM, NZ, CRESSIE>, vario_plane_kernel<DIM, NZ, CRESSIE> and vario_cross_kernel<DIM, NZ>, keyed as
tools/kernel_census.py prints it
(tests/test_variography_instances_host.py holds the table against the built library and the cases against what they
claim; tests/test_gpu_variography_instances.py runs them on the device against variography_ref / varioplane_ref /
variography_cross_ref).

A case is a dict: form ("window", "plane", "cross"), x (129, dim), z (nz, 129), estimator, calls = [(nlags, maxlag), ..]
and, for the plane, dirs, basis and ptol.  129 samples are three batches of 64, the last with one point: diagonal and
off-diagonal tiles, a partial batch J and a partial batch I.  Coordinates are distinct cells of an integer lattice plus
one exact duplicate; values are integers with |z| <= 2^10, so every squared difference and every product of differences
is an integer below 2^22 and every sum of them an integer below 2^53: Matheron and cross sums carry no rounding in any
order of addition.

Calls.  7 lags of integer width that end inside the lattice's diameter (pairs beyond the last edge, pairs on edges).
The window cases add 256 lags that cover the diameter with bins narrower than the lattice spacing (1-D: as wide): see
window_overflows()."""
import numpy as np

FAMILIES = ("vario_window_kernel", "vario_plane_kernel", "vario_cross_kernel")
N = 129
LATTICE = {1: (256,), 2: (16, 16), 3: (8, 8, 4)}           # 256 cells each; diameters 255, 21.2, 10.3
MAXLAG_7 = {1: 140.0, 2: 14.0, 3: 7.0}                      # delta = 20, 2, 1
MAXLAG_256 = {1: 256.0, 2: 32.0, 3: 16.0}                   # delta = 1, 1/8, 1/16
NANGLES = 5                                                 # not a power of two: the bisection's last step repeats
# an oblique orthonormal basis: rows e1, e2, normal (3-4-5 and 5-12-13 rotations composed; orthonormal to 1e-16)
OBLIQUE = np.ascontiguousarray(np.array([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
                               @ np.array([[1.0, 0.0, 0.0], [0.0, 5.0 / 13.0, -12.0 / 13.0],
                                           [0.0, 12.0 / 13.0, 5.0 / 13.0]]))
PTOL = 2.0


def window_vw(nz):
    """VW, the bins of the register window of vario_window_kernel<., nz, .>"""
    return 6 if nz <= 2 else 4


def samples(dim, nz, seed):
    rng = np.random.default_rng(seed)
    shape = LATTICE[dim]
    cells = rng.choice(int(np.prod(shape)), N - 1, replace=False)
    x = np.stack(np.unravel_index(cells, shape), axis=1).astype(np.float64)
    x = np.concatenate([x, x[:1]])                          # sample 128 (alone in the last batch) repeats sample 0
    z = rng.integers(-1024, 1025, (nz, N)).astype(np.float64)
    return np.ascontiguousarray(x), np.ascontiguousarray(z)


def _bool(b):
    return "true" if b else "false"


def window_case(dim, nz, cressie):
    x, z = samples(dim, nz, 1000 + 100 * dim + 10 * nz + cressie)
    return dict(form="window", x=x, z=z, estimator="cressie" if cressie else "matheron",
                calls=[(7, MAXLAG_7[dim]), (256, MAXLAG_256[dim])])


def plane_case(dim, nz, cressie):
    x, z = samples(dim, nz, 2000 + 100 * dim + 10 * nz + cressie)
    ang = 0.3 + np.arange(NANGLES) * (np.pi / NANGLES)
    return dict(form="plane", x=x, z=z, estimator="cressie" if cressie else "matheron", calls=[(7, MAXLAG_7[dim])],
                dirs=np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1)),
                basis=OBLIQUE if dim == 3 else None, ptol=PTOL if dim == 3 else np.inf)


def cross_case(dim, nz):
    x, z = samples(dim, nz, 3000 + 100 * dim + 10 * nz)
    return dict(form="cross", x=x, z=z, estimator="matheron", calls=[(7, MAXLAG_7[dim])])


def kernel_of(case):
    """The dispatch of csrc/variography.hip (vario_kernel) restated: the call's form, dim, nz and estimator -> key."""
    dim, nz, cressie = case["x"].shape[1], case["z"].shape[0], case["estimator"] == "cressie"
    if case["form"] == "cross":
        return ("vario_cross_kernel", (dim, nz))
    return ("vario_%s_kernel" % case["form"], (dim, nz, _bool(cressie)))


def _key(form, dim, nz, cressie=False):
    return kernel_of(dict(form=form, x=np.empty((0, dim)), z=np.empty((nz, 0)),
                          estimator="cressie" if cressie else "matheron"))


CASES = {}
for _dim in (1, 2, 3):
    for _nz in range(1, 9):
        for _cr in (False, True):
            CASES[_key("window", _dim, _nz, _cr)] = (lambda d=_dim, q=_nz, c=_cr: window_case(d, q, c))
            if _dim >= 2 and _nz <= 4:
                CASES[_key("plane", _dim, _nz, _cr)] = (lambda d=_dim, q=_nz, c=_cr: plane_case(d, q, c))
        CASES[_key("cross", _dim, _nz)] = (lambda d=_dim, q=_nz: cross_case(d, q))


def case_id(key):
    return "%s-%s" % (key[0].split("_")[1], "-".join(str(a) for a in key[1]))


def window_overflows(case, nlags, maxlag):
    """True when, whatever order the samples are put in, a tile of this call has kept pairs beyond its register window.
    A full batch meets itself in a diagonal tile of 64 * 63 / 2 pairs whose lower bound is 0, so its window is the bins
    0 .. VW - 1.  If fewer pairs than that, over the whole set, are duplicates, lie beyond the last edge or fall into
    those bins, some pair of that tile is kept in a bin >= VW: the tile spans more than VW bins."""
    import variography_ref as vref
    x = case["x"]
    count, _, _, ndup = vref.empirical(x, case["z"], nlags, maxlag)
    n = x.shape[0]
    beyond = n * (n - 1) // 2 - ndup - int(count.sum())
    near = int(count[:window_vw(case["z"].shape[0])].sum())
    return ndup + beyond + near < 64 * 63 // 2
