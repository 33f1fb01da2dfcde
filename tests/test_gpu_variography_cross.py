"""gss_variogram_cross on the device against the numpy restatement (tests/variography_cross_ref.py), against
gss_variogram_empirical, its front-ends and examples/covariography.py.

Bars.  Counts and nduplicates are compared exactly.  With integer values |z| <= 2^10 every product is an integer below
2^22 and every bin sum an integer below 2^53: whatever the order of addition no rounding happens, and csum is compared
bit for bit.  lagsum keeps the bar of test_gpu_variography.py (2 count 2^-53 S).  A sum of `count` real products added in
any order differs from the exact sum by at most (count - 1) 2^-53 sum |products| to first order; the device sum is
compared with the correctly rounded one (math.fsum) at 2 count 2^-53 sum |products|.  Derived, not measured."""
import os
import subprocess
import sys

import numpy as np
import pytest

import variography_cross_ref as cref
import variography_ref as vref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
MAXLAG = {1: 1.0, 7: 1.75, 256: 2.0}      # delta = 1, 1/4, 1/128: lattice distances (multiples of 1/8) fall on edges


def _engine():
    from gss.engine import HipEngine
    return HipEngine


def lattice(n, d, seed):
    """coordinates on multiples of 1/8 in [0, 2): every key is exact, many pairs sit exactly on a bin edge, and (in 1-D
    and 2-D by themselves, in 3-D by the copies) samples coincide"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 16, (n, d)).astype(np.float64) / 8.0
    x[n // 2] = x[0]
    x[n - 1] = x[1]
    return np.ascontiguousarray(x)


def int_values(n, nz, seed):
    return np.ascontiguousarray(np.random.default_rng(seed + 500).integers(-1024, 1025, (nz, n)).astype(np.float64))


def check_exact(dev, ref):
    count, lagsum, csum, ndup = dev
    rcount, rlagsum, rcsum, rndup, _ = ref
    assert np.array_equal(count, rcount)
    assert ndup == rndup
    assert np.array_equal(csum, rcsum)                                     # integers below 2^53: bit for bit
    assert (np.abs(lagsum - rlagsum) <= 2.0 * rcount * U * rlagsum).all()


@pytest.mark.parametrize("nlags", [1, 7, 256])
@pytest.mark.parametrize("nz", [1, 2, 3, 8])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_exact_sums_on_a_lattice(n, d, nz, nlags):
    x, z = lattice(n, d, 7 * n + d), int_values(n, nz, nlags)
    ref = cref.cross(x, z, nlags, MAXLAG[nlags])
    if (n, d, nz, nlags) == (129, 2, 2, 7):                                # the cases are what they claim to be
        i, j, k, dk, ndup = cref.kept_pairs(x, nlags, MAXLAG[nlags])
        assert ndup >= 2 and np.isin(dk, vref.edges2(nlags, MAXLAG[nlags])[1:]).sum() > 100
    assert ref[0].sum() > 0
    check_exact(_engine().variogram_cross(x, z, nlags, MAXLAG[nlags]), ref)


@pytest.mark.parametrize("d,u", [(2, (0.6, 0.8)), (3, (0.36, 0.48, 0.8))])
def test_exact_sums_directional(d, u):
    n = 129
    x, z = lattice(n, d, 3 + d), int_values(n, 3, d)
    dtol, cos_atol = 0.5, float(np.cos(np.pi / 5))
    ref = cref.cross(x, z, 7, 1.75, direction=u, dtol=dtol, cos_atol=cos_atol)
    assert 0 < ref[0].sum() < cref.cross(x, z, 7, 1.75)[0].sum()           # the filter does filter
    check_exact(_engine().variogram_cross(x, z, 7, 1.75, direction=u, dtol=dtol, cos_atol=cos_atol), ref)


_CULL_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from gss import _lib
from gss.engine import HipEngine
from test_gpu_variography_cross import clustered_grid, int_values
x, z = clustered_grid(3000, 3), int_values(3000, 3, 5)
count, lagsum, csum, ndup = HipEngine.variogram_cross(x, z, 20, 3.0)
np.savez(%r, count=count, lagsum=lagsum, csum=csum, ndup=ndup, total=_lib.stat("vario_tiles_total"),
         opened=_lib.stat("vario_tiles_opened"))
"""


def clustered_grid(n, d):
    """clusters, coordinates rounded to the 2^-10 grid"""
    rng = np.random.default_rng(17)
    centres = rng.uniform(0.0, 100.0, (12, d))
    x = centres[rng.integers(0, 12, n)] + rng.normal(scale=3.0, size=(n, d))
    return np.ascontiguousarray(np.round(x * 1024.0) / 1024.0)


def test_culling_changes_nothing(tmp_path):
    """A child process with GSS_VARIO_CULL=0 (every tile opened) against the default: fewer tiles opened, the same
    counts and -- integer values -- the same sums bit for bit."""
    res = []
    for cull in ("1", "0"):
        out = str(tmp_path / ("cull%s.npz" % cull))
        code = _CULL_CHILD % (ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests"), out)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSS_VARIO_CULL=cull), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(np.load(out))
    on, off = res
    assert int(off["opened"]) == int(off["total"]) == int(on["total"]) and 0 < int(on["opened"]) < int(on["total"])
    assert np.array_equal(on["count"], off["count"]) and int(on["ndup"]) == int(off["ndup"]) and on["count"].sum() > 0
    assert np.array_equal(on["csum"], off["csum"])
    assert (np.abs(on["lagsum"] - off["lagsum"]) <= 2.0 * on["count"] * U * on["lagsum"]).all()


def test_real_values_of_unequal_scale():
    """Columns of scale 1 and 10^6: every bin sum within 2 count 2^-53 sum |products| of the correctly rounded sum.
    Beside it, printed only, the error of the polarisation route through gss_variogram_empirical on (z_a, z_b,
    z_a + z_b): the small cross sum is the difference of large ones there."""
    n, nlags, maxlag = 1500, 20, 40.0
    x = clustered_grid(n, 3)
    rng = np.random.default_rng(3)
    z = np.ascontiguousarray(np.stack([rng.normal(size=n), 1e6 * rng.normal(size=n)]))
    count, lagsum, csum, ndup = _engine().variogram_cross(x, z, nlags, maxlag)
    rcount, rlagsum, rcsum, rndup, asum = cref.cross(x, z, nlags, maxlag, exact=True)
    assert np.array_equal(count, rcount) and ndup == rndup
    bar = 2.0 * rcount * U * asum
    err = np.abs(csum - rcsum)
    pc, pl, pz, pn = _engine().variogram_empirical(x, np.stack([z[0], z[1], z[0] + z[1]]), nlags, maxlag)
    polar = 0.5 * (pz[2] - pz[0] - pz[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        print("cross sum (a, b): largest error / bar = %.3f; polarisation route: largest error / the same bar = %.3g"
              % (np.nanmax(err[1] / bar[1]), np.nanmax(np.abs(polar - rcsum[1]) / bar[1])))
        print("all rows: largest error / bar = %.3f" % np.nanmax(err / bar))
    assert (err <= bar).all(), (err, bar)


def test_direct_rows_equal_the_direct_call():
    n, nlags, maxlag = 3000, 25, 30.0
    x = clustered_grid(n, 2)
    z = np.ascontiguousarray(np.random.default_rng(8).normal(size=(3, n)))
    count, lagsum, csum, ndup = _engine().variogram_cross(x, z, nlags, maxlag)
    c1, l1, z1, n1 = _engine().variogram_empirical(x, z, nlags, maxlag)
    assert np.array_equal(count, c1) and ndup == n1
    assert (np.abs(lagsum - l1) <= 2.0 * count * U * np.maximum(lagsum, l1)).all()
    for a in range(3):
        row = csum[cref.pair_row(3, a, a)]
        assert (np.abs(row - z1[a]) <= 2.0 * count * U * np.maximum(row, z1[a])).all()
    u = np.array([0.6, 0.8])
    cd = _engine().variogram_cross(x, z, nlags, maxlag, direction=u, dtol=5.0, cos_atol=0.9)
    ed = _engine().variogram_empirical(x, z, nlags, maxlag, direction=u, dtol=5.0, cos_atol=0.9)
    assert np.array_equal(cd[0], ed[0]) and cd[3] == ed[3] and 0 < cd[0].sum() < count.sum()


def test_exact_sums_on_the_kd_order_40000():
    """A size that runs on the k-d order with 16-tile units (2-D, lags to 2 % of the extent): the reference enumerates
    its candidate pairs by cells."""
    n, nlags, maxlag = 40000, 20, 20.0
    rng = np.random.default_rng(40)
    x = np.ascontiguousarray(np.round(rng.uniform(0.0, 1000.0, (n, 2)) * 1024.0) / 1024.0)
    x[7], x[n - 3] = x[100], x[101]
    z = int_values(n, 3, 41)
    ref = cref.cross(x, z, nlags, maxlag, candidates=cref.cell_candidates(x, maxlag))
    assert ref[3] == 2 and ref[0].sum() > 500000
    check_exact(_engine().variogram_cross(x, z, nlags, maxlag), ref)


def test_device_arrays_repeats_and_non_finite_input():
    import torch
    from gss import _lib
    n = 5000
    x, z = clustered_grid(n, 3), int_values(n, 2, 9)
    host = _engine().variogram_cross(x, z, 20, 25.0)
    xd, zd = torch.as_tensor(x, device="cuda"), torch.as_tensor(z, device="cuda")
    d1 = _engine().variogram_cross(xd, zd, 20, 25.0)
    d2 = _engine().variogram_cross(xd, zd, 20, 25.0)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in d1)
    assert torch.equal(d1[0], d2[0]) and torch.equal(d1[3], d2[3])        # two calls: identical counts
    assert np.array_equal(d1[0].cpu().numpy(), host[0]) and int(d1[3].cpu()[0]) == host[3]
    assert np.array_equal(d1[2].cpu().numpy(), host[2])                   # integer values: exact in any order
    z[1, 17] = np.nan
    with pytest.raises(_lib.GSSError) as e:
        _engine().variogram_cross(x, z, 20, 25.0)
    assert e.value.code == _lib.ERR_INVALID and "NaN" in str(e.value)
    count, lagsum, csum, ndup = _engine().variogram_cross(xd, torch.as_tensor(z, device="cuda"), 20, 25.0)
    assert int(ndup.cpu()[0]) == -1 and (count.cpu().numpy() == -1).all()
    assert np.isnan(lagsum.cpu().numpy()).all() and np.isnan(csum.cpu().numpy()).all()


def test_front_end_to_lmc_to_kriging():
    """Two variables built from two smooth factors on 1 500 scattered samples: shapes, a positive semidefinite model,
    and the direct model of a variable goes into KrigingSolver."""
    import gss
    rng = np.random.default_rng(12)
    n = 1500
    x = rng.uniform(0.0, 100.0, (n, 2))

    def factor(seed):
        r = np.random.default_rng(seed)
        k, ph = r.normal(scale=0.08, size=(40, 2)), r.uniform(0, 2 * np.pi, 40)
        return np.sqrt(2.0 / 40) * np.cos(x @ k.T + ph).sum(axis=1)

    f1, f2 = factor(1), factor(2)
    u = f1 + 0.3 * rng.normal(size=n)
    v = 0.8 * f1 + 0.6 * f2
    v[::50] = np.nan                                                       # dropped for both variables
    data = gss.georef({"u": u, "v": v}, x)
    g = gss.EmpiricalCrossVariogram(data, ["u", "v"], nlags=15, maxlag=40.0)
    keep = np.isfinite(v)
    ref = cref.cross(x[keep], np.stack([u[keep], v[keep]]), 15, 40.0)
    assert g.ordinate.shape == (3, 15) and g.abscissa.shape == (15,) and np.array_equal(g.count, ref[0])
    assert np.allclose(g.gamma("u", "v"), ref[2][1] / (2 * ref[0]), rtol=1e-9, atol=1e-12)
    assert np.array_equal(g.gamma("v", "u"), g.gamma(0, 1)) and np.array_equal(g.direct("v").ordinate, g.gamma(1, 1))
    m = gss.fit_lmc(["spherical", "exponential", "gaussian"], g)
    print("LMC %s range %.3f  B0 %s  B1 %s  correlation %.4f" % (m.kind, m.range, m.B0.tolist(), m.B1.tolist(),
                                                                m.correlation("u", "v")))
    assert m.B0.shape == m.B1.shape == (2, 2)
    for b in (m.B0, m.B1):
        assert np.array_equal(b, b.T) and np.linalg.eigvalsh(b).min() >= -1e-12 * np.trace(b)
    assert -1.0 <= m.correlation("u", "v") <= 1.0 and g.abscissa.min() / 4 <= m.range <= 4 * g.abscissa.max()
    sub = gss.georef({"u": u[:400]}, x[:400])
    sol = gss.solve(gss.EstimationProblem(sub, gss.CartesianGrid(32, 32), "u"),
                    gss.KrigingSolver(("u", dict(variogram=m.variogram("u"), maxneighbors=16))))
    assert np.isfinite(sol["u"]).all() and (sol["u_variance"] > -1e-9).all()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "covariography.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    assert "fitted correlation" in r.stdout and "true" in r.stdout
