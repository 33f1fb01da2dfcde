"""One case per compiled instantiation ik_local_kernel<DIM, KIND, NT, FULL> (csrc/ik_kernel.h), with the conventions of
tests/cokrig_local_cases.KERNELS and on the helpers of tests/ik_cases.py.  tests/test_ik_census.py holds the table
against the kernels the compiler emitted, restates the dispatch on every case and asserts the conditions below on the
reference alone; tests/test_gpu_ik.py runs every entry on the device; tools/ik_oracle.py measures its error bar.

    KERNELS = {(DIM, KIND, NT, FULL): a function that builds the case, or UNREACHABLE("reason citing the dispatch line")}

The dispatch (csrc/ik.hip, ik_dispatch; csrc/ik_kernel.h, ik_local_launch and ik_local_launch_kinds): FULL for one
variogram per cutoff (nvg = K > 1), which has the general kernel only; KIND 0 Gaussian, 1 exponential, 2 spherical,
30 / 31 / 32 Matern 1/2, 3/2, 5/2 for a single structure of that kind in 2-D and 3-D, -1 for any other model (cubic,
pentaspherical, nested) and for 1-D; NT = 1 / 2 / 4 for maxneighbors <= 16 / 32 / 64.

Every case has 200 samples and 67 domain points (not a multiple of the four waves of a workgroup: the last workgroup
holds an out-of-range wave that still meets the barriers).  maxneighbors is 13 / 29 / 50 (a ragged last tile in each
size class) inside a ball, so the counts differ from point to point: point 0 sits where the ball holds few samples
(a whole tile stays empty for NT >= 2), point 1 in the middle (the full count).  Cutoffs are sample values.  NT = 1 and
2 take K = 5, NT = 4 takes K = 16 under the ordinary variant (the second B tile at the highest register pressure); NT = 1
is always the simple variant with F*, NT = 2 alternates.  Nugget 0.15, sill 1.3.  The NT = 2 entries of 2-D and 3-D have
axis-aligned anisotropic radii.  The general median entries alternate between cubic / pentaspherical and nested
models.  The full form has K = 3 variograms of three kinds, one nested; its NT = 2 entries in 2-D and 3-D have a rotated
member.
"""
from dataclasses import dataclass

import numpy as np

import gss
import ik_cases as IC

KINDS = (0, 1, 2, 30, 31, 32)
K_OF_NT = {1: 13, 2: 29, 4: 50}
N, M = 200, 67
SILL, NUGGET = 1.3, 0.15
RANGE = {0: 16.0, 1: 35.0, 2: 45.0, 30: 35.0, 31: 35.0, 32: 30.0, -1: 40.0}
RADII = {2: (48.0, 26.0), 3: (48.0, 26.0, 36.0)}
# search radius by (dim, NT): about 1.6 k samples inside the ball in the middle of the data
RADIUS = {(1, 1): 5.2, (1, 2): 11.6, (1, 4): 20.0, (2, 1): 18.0, (2, 2): 24.0, (2, 4): 36.0,
          (3, 1): 31.0, (3, 2): 38.0, (3, 4): 46.0}
# the kind a case must be told apart from (tests/test_ik_census.py): same range, sill and nugget
NEIGHBOUR = {0: 1, 1: 0, 2: 1, 30: 31, 31: 32, 32: 31}


@dataclass(frozen=True)
class UNREACHABLE:
    reason: str


def name_of(key):
    dim, kind, nt, full = key
    return "ik_%d_%s_%d_%s" % (dim, "g" if kind < 0 else kind, nt, "full" if full else "median")


def single(kind, ball_or_range, sill=SILL, nugget=NUGGET):
    """The one-structure model of a compile-time kind: an isotropic range or a MetricBall."""
    ctor = {0: gss.GaussianVariogram, 1: gss.ExponentialVariogram, 2: gss.SphericalVariogram,
            30: gss.MaternVariogram, 31: gss.MaternVariogram, 32: gss.MaternVariogram}[kind]
    kw = dict(sill=sill, nugget=nugget)
    if kind >= 30:
        kw["order"] = {30: 0.5, 31: 1.5, 32: 2.5}[kind]
    if isinstance(ball_or_range, gss.MetricBall):
        return ctor(ball_or_range, **kw)
    return ctor(range=ball_or_range, **kw)


def _rotation3():
    a, b = 0.6, 0.35
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    return Rz @ Rx


def _nested(dim, aniso):
    if aniso:
        a = gss.ExponentialVariogram(gss.MetricBall(RADII[dim]), sill=SILL, nugget=NUGGET)
        b = gss.SphericalVariogram(gss.MetricBall(tuple(1.5 * r for r in RADII[dim])), sill=SILL)
    else:
        a = gss.ExponentialVariogram(range=20.0, sill=SILL, nugget=NUGGET)
        b = gss.SphericalVariogram(range=60.0, sill=SILL)
    return gss.NestedVariogram([(0.6, a), (0.4, b)])


def models_of(key, kind=None):
    """The variograms of an entry (`kind`: another compile-time kind in its place, for the discrimination check)."""
    dim, kd, nt, full = key
    aniso = nt == 2 and dim >= 2
    if full:
        third = gss.MaternVariogram(range=30.0, order=1.5, sill=1.1, nugget=0.05)
        if aniso:
            rot = 0.6 if dim == 2 else _rotation3()
            radii = (50.0, 15.0) if dim == 2 else (50.0, 30.0, 15.0)
            third = gss.ExponentialVariogram(gss.MetricBall(radii, rot), sill=0.9, nugget=0.05)
        return [gss.SphericalVariogram(range=25.0, sill=1.2, nugget=0.1), _nested(dim, False), third]
    if kd >= 0:
        return [single(kd if kind is None else kind, gss.MetricBall(RADII[dim]) if aniso else RANGE[kd])]
    i = 3 * (dim - 1) + {1: 0, 2: 1, 4: 2}[nt]      # the nine general median entries in order: nested and not, by turns
    if i % 2 == 0:
        return [_nested(dim, aniso)]
    ctor = gss.CubicVariogram if i % 4 == 1 else gss.PentasphericalVariogram
    if aniso:
        return [ctor(gss.MetricBall(RADII[dim]), sill=SILL, nugget=NUGGET)]
    return [ctor(range=RANGE[-1], sill=SILL, nugget=NUGGET)]


def kernel_case(key, kind=None):
    dim, kd, nt, full = key
    seed = 5000 + 1000 * dim + 20 * (kd if kd >= 0 else 7) + 2 * nt + int(full)
    x, z, x0 = IC._data(seed, N, dim, m=M)
    r = RADIUS[(dim, nt)]
    if dim == 1:   # a jittered lattice in shuffled order: no near-coincident samples on the line
        rng = np.random.default_rng(seed + 1)
        x = ((np.arange(N) + 0.5 + rng.uniform(-0.3, 0.3, N)) * (100.0 / N))[rng.permutation(N), None]
        x0[0] = -0.5 * r            # half a ball's reach outside the data: a quarter of the interior count
    else:
        x0[0] = 2.0 if dim == 2 else 10.0   # near a corner: about 1 / 4 (2-D) or 1 / 8 (3-D) of the ball holds samples
    x0[1] = 50.0
    if full:
        K, simple = 3, nt == 1
    elif nt == 4:
        K, simple = 16, False
    else:
        K, simple = 5, nt == 1 or (kd if kd >= 0 else 1) % 2 == 1
    cut = IC._cutoffs(z, K)
    return dict(x=x, z=z, x0=x0, cutoffs=cut, models=models_of(key, kind), k=K_OF_NT[nt], radius=r,
                fstar=IC._fstar(z, cut) if simple else None)


KERNELS = {(dim, kind, nt, False): (lambda key=(dim, kind, nt, False): kernel_case(key))
           for dim in (2, 3) for kind in KINDS for nt in (1, 2, 4)}
KERNELS.update({(dim, -1, nt, full): (lambda key=(dim, -1, nt, full): kernel_case(key))
                for dim in (1, 2, 3) for nt in (1, 2, 4) for full in (False, True)})
