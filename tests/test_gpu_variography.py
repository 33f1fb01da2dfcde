"""gss_variogram_empirical on the device against the numpy restatement (tests/variography_ref.py), its invariants, the
front-ends of gss.variography and examples/variography.py.

Bars.  Counts and nduplicates are compared exactly.  A sum S of count non-negative terms, added in any order in FP64,
differs from the exact sum by at most (count - 1) 2^-53 S to first order; two such sums (device, numpy) of the same
terms therefore differ by at most 2 count 2^-53 S.  Derived, not measured.  Largest observed ratio |S_dev - S_ref| to
that bar over every case of this file on an MI355X: see SUMS_WORST below."""
import os
import runpy
import subprocess
import sys

import numpy as np
import pytest

import variography_ref as vref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SUMS_WORST = "0.24 (MI355X, the 92 cases of this file)"   # largest |S_dev - S_ref| / (2 count 2^-53 S_ref) observed
_worst = [0.0]


def _engine():
    from gss.engine import HipEngine
    return HipEngine


def clustered(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.0, 100.0, (12, d))
    x = centres[rng.integers(0, 12, n)] + rng.normal(scale=3.0, size=(n, d))
    return np.ascontiguousarray(x)


def values(n, nz, seed):
    return np.ascontiguousarray(np.random.default_rng(seed + 1000).normal(size=(nz, n)))


def check_against(dev, ref):
    count, lagsum, zsum, ndup = dev
    rcount, rlagsum, rzsum, rndup = ref
    assert np.array_equal(count, rcount)
    assert ndup == rndup
    for s_dev, s_ref, c in [(lagsum, rlagsum, rcount)] + [(zsum[i], rzsum[i], rcount) for i in range(zsum.shape[0])]:
        bar = 2.0 * c * U * s_ref
        err = np.abs(s_dev - s_ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
        _worst[0] = max(_worst[0], float(ratio.max()))
        print("sum-to-bar ratio %.4f (worst so far %.4f)" % (ratio.max(), _worst[0]))
        assert (err <= bar).all(), (err, bar)


def check_sums_close(a, b, count):
    """two device results of the same pairs: each within count 2^-53 S of the exact sum"""
    assert (np.abs(a - b) <= 2.0 * count * U * np.maximum(np.abs(a), np.abs(b))).all()


@pytest.mark.parametrize("estimator", ["matheron", "cressie"])
@pytest.mark.parametrize("nlags", [1, 20, 256])
@pytest.mark.parametrize("nz", [1, 3, 8])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_parity_clustered_2000(d, nz, nlags, estimator):
    x, z = clustered(2000, d, 10 * d + nz), values(2000, nz, nlags)
    maxlag = 40.0
    dev = _engine().variogram_empirical(x, z, nlags, maxlag, estimator=0 if estimator == "matheron" else 1)
    check_against(dev, vref.empirical(x, z, nlags, maxlag, estimator=estimator))


@pytest.mark.parametrize("d,nz,nlags,estimator", [(3, 1, 20, "matheron"), (2, 3, 256, "cressie"), (1, 8, 20, "matheron")])
def test_parity_uniform_20000(d, nz, nlags, estimator):
    rng = np.random.default_rng(77 + d)
    x = np.ascontiguousarray(rng.uniform(0.0, 1000.0, (20000, d)))
    z = values(20000, nz, d)
    maxlag = 0.3 * 1000.0 * np.sqrt(d)
    dev = _engine().variogram_empirical(x, z, nlags, maxlag, estimator=0 if estimator == "matheron" else 1)
    check_against(dev, vref.empirical(x, z, nlags, maxlag, estimator=estimator))


def test_lattice_pairs_on_bin_edges():
    """50 x 50 lattice of spacing 0.5 with delta = 2: every lattice distance that is a multiple of 2 (along the axes,
    3-4-5 triangles, ...) lies exactly on an edge and belongs to the bin below it -- the case that pins the edge2 rule."""
    g = np.arange(50) * 0.5
    x = np.ascontiguousarray(np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2))
    z = values(2500, 3, 5)
    nlags, maxlag = 10, 20.0
    e2 = vref.edges2(nlags, maxlag)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    assert np.isin(d2[np.triu_indices(2500, 1)], e2[1:]).sum() > 10000        # many pairs sit exactly on an edge
    for est in ("matheron", "cressie"):
        dev = _engine().variogram_empirical(x, z, nlags, maxlag, estimator=0 if est == "matheron" else 1)
        check_against(dev, vref.empirical(x, z, nlags, maxlag, estimator=est))


def test_duplicated_samples_are_counted_apart():
    x = clustered(1500, 3, 3)
    x[1000:1400] = x[:400]          # 400 coincident pairs
    x[1400:1450] = x[0]             # and a point repeated 52 times in all
    z = values(1500, 2, 9)
    dev = _engine().variogram_empirical(x, z, 20, 30.0)
    ref = vref.empirical(x, z, 20, 30.0)
    assert ref[3] >= 400 + 51 * 52 // 2 - 1
    check_against(dev, ref)


DIRECTIONS = {2: [(1.0, 0.0), (np.sqrt(0.5), np.sqrt(0.5)), (0.28, 0.96)],
              3: [(0.0, 0.0, 1.0), (1 / np.sqrt(3.0),) * 3, (0.36, 0.48, 0.8)]}


@pytest.mark.parametrize("mode", ["band", "cone", "both"])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("d", [2, 3])
def test_directional_parity_and_symmetry(d, which, mode):
    u = np.asarray(DIRECTIONS[d][which])
    u = u / np.sqrt((u * u).sum())
    assert abs(np.sqrt((u * u).sum()) - 1.0) <= 1e-12
    x, z = clustered(2000, d, 40 + d), values(2000, 2, 4)
    dtol = 6.0 if mode in ("band", "both") else np.inf
    cos_atol = np.cos(np.pi / 7) if mode in ("cone", "both") else 0.0
    dev = _engine().variogram_empirical(x, z, 20, 40.0, direction=u, dtol=dtol, cos_atol=cos_atol)
    ref = vref.empirical(x, z, 20, 40.0, direction=u, dtol=dtol, cos_atol=cos_atol)
    assert 0 < ref[0].sum() < vref.empirical(x, z, 20, 40.0)[0].sum()           # the filter does filter
    check_against(dev, ref)
    neg = _engine().variogram_empirical(x, z, 20, 40.0, direction=-u, dtol=dtol, cos_atol=cos_atol)
    assert np.array_equal(neg[0], dev[0]) and neg[3] == dev[3]
    check_sums_close(neg[1], dev[1], dev[0])
    check_sums_close(neg[2], dev[2], dev[0][None, :])


def test_counts_sum_to_all_pairs_and_survive_a_permutation():
    n = 3000
    x, z = clustered(n, 3, 8), values(n, 1, 2)
    x[10] = x[20]
    diam = float(np.sqrt(((x.max(0) - x.min(0)) ** 2).sum()))
    count, lagsum, zsum, ndup = _engine().variogram_empirical(x, z, 20, 1.01 * diam)
    assert ndup >= 1 and int(count.sum()) == n * (n - 1) // 2 - ndup
    p = np.random.default_rng(3).permutation(n)
    c2, l2, z2, nd2 = _engine().variogram_empirical(np.ascontiguousarray(x[p]), np.ascontiguousarray(z[:, p]), 20, 1.01 * diam)
    assert np.array_equal(c2, count) and nd2 == ndup
    check_sums_close(l2, lagsum, count)
    check_sums_close(z2, zsum, count[None, :])


@pytest.mark.parametrize("n", [40000, 32768, 32767])
def test_all_pairs_and_permutation_on_both_orderings(n):
    """Either side of the size where the ordering changes from one Morton sort to the k-d order and the work units from
    4 to 16 tiles: with maxlag beyond the diameter the counts sum to n (n - 1) / 2 - nduplicates and do not change
    when the samples are permuted."""
    rng = np.random.default_rng(n)
    x = np.ascontiguousarray(rng.uniform(0.0, 50.0, (n, 3)))
    x[5], x[n - 1] = x[77], x[78]
    z = values(n, 2, 12)
    count, lagsum, zsum, ndup = _engine().variogram_empirical(x, z, 20, 90.0)
    assert ndup == 2 and int(count.sum()) == n * (n - 1) // 2 - ndup
    p = rng.permutation(n)
    c2, l2, z2, nd2 = _engine().variogram_empirical(np.ascontiguousarray(x[p]), np.ascontiguousarray(z[:, p]), 20, 90.0)
    assert np.array_equal(c2, count) and nd2 == ndup
    check_sums_close(l2, lagsum, count)
    check_sums_close(z2, zsum, count[None, :])


def test_parity_on_the_kd_order_40000():
    """The restatement at a size that runs on the k-d order with 16-tile units (2-D, lags to a tenth of the extent)."""
    rng = np.random.default_rng(40)
    x = np.ascontiguousarray(rng.uniform(0.0, 1000.0, (40000, 2)))
    z = values(40000, 1, 41)
    dev = _engine().variogram_empirical(x, z, 20, 100.0)
    check_against(dev, vref.empirical(x, z, 20, 100.0))


def test_columns_in_one_call_equal_single_column_calls():
    x, z = clustered(2500, 2, 21), values(2500, 5, 6)
    count, lagsum, zsum, ndup = _engine().variogram_empirical(x, z, 30, 35.0, estimator=1)
    for c in range(5):
        c1, l1, z1, n1 = _engine().variogram_empirical(x, z[c:c + 1], 30, 35.0, estimator=1)
        assert np.array_equal(c1, count) and n1 == ndup
        check_sums_close(z1[0], zsum[c], count)


_CULL_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from gss import _lib
from gss.engine import HipEngine
from test_gpu_variography import clustered, values
n, frac = %d, %r
x, z = clustered(n, 3, 5), values(n, 2, 5)
ext = float((x.max(0) - x.min(0)).max())
count, lagsum, zsum, ndup = HipEngine.variogram_empirical(x, z, 20, frac * ext)
np.savez(%r, count=count, lagsum=lagsum, zsum=zsum, ndup=ndup, total=_lib.stat("vario_tiles_total"),
         opened=_lib.stat("vario_tiles_opened"))
"""


@pytest.mark.parametrize("n,frac", [(20000, 0.02), (200000, 0.01)])
def test_culling_skips_tiles_and_changes_nothing(tmp_path, n, frac):
    """maxlag = 2 % of the extent on a clustered set: most batch pairs are never opened, and a child process with
    GSS_VARIO_CULL=0 (every tile opened) returns the same counts and sums within the bar.  The second size runs on the
    k-d order with 16-tile units drawn several at a time (the first: one Morton sort, 4-tile units drawn singly)."""
    res = []
    for cull in ("1", "0"):
        out = str(tmp_path / ("cull%s.npz" % cull))
        code = _CULL_CHILD % (ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests"), n, frac,
                              out)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSS_VARIO_CULL=cull), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(np.load(out))
    on, off = res
    nb = (n + 63) // 64
    assert int(on["total"]) == int(off["total"]) == nb * (nb + 1) // 2
    assert int(off["opened"]) == int(off["total"])
    assert 0 < int(on["opened"]) < int(on["total"]) // 4
    print("tiles opened %d of %d" % (int(on["opened"]), int(on["total"])))
    assert np.array_equal(on["count"], off["count"]) and int(on["ndup"]) == int(off["ndup"])
    assert on["count"].sum() > 0
    check_sums_close(on["lagsum"], off["lagsum"], on["count"])
    check_sums_close(on["zsum"], off["zsum"], on["count"][None, :])


def test_host_and_device_memory_agree_and_the_stream_chain_holds():
    """Device arrays on a non-default stream give the counts of the host call, and such a call between two kriging
    calls on the default stream leaves their results unchanged (gss.h: the stream chain)."""
    import torch
    import gss
    from gss.engine import KrigHandle, OK
    x, z = clustered(6000, 3, 31), values(6000, 2, 7)
    host = _engine().variogram_empirical(x, z, 25, 30.0)
    rng = np.random.default_rng(0)
    xs, zs, x0 = rng.uniform(0, 100, (200, 3)), rng.normal(size=200), rng.uniform(0, 100, (5000, 3))
    kh = KrigHandle(gss.ExponentialVariogram(range=30.0), OK, xs, zs)
    x0d = torch.as_tensor(x0, device="cuda")
    mu1, var1, _ = kh.predict_global(x0d)
    side = torch.cuda.Stream()
    xd, zd = torch.as_tensor(x, device="cuda"), torch.as_tensor(z, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev = _engine().variogram_empirical(xd, zd, 25, 30.0)
    mu2, var2, _ = kh.predict_global(x0d)
    torch.cuda.synchronize()
    assert torch.equal(mu1, mu2) and torch.equal(var1, var2)
    assert np.array_equal(dev[0].cpu().numpy(), host[0]) and int(dev[3].cpu()[0]) == host[3]
    check_sums_close(dev[1].cpu().numpy(), host[1], host[0])
    check_sums_close(dev[2].cpu().numpy(), host[2], host[0][None, :])
    kh.close()


def test_non_finite_values_are_refused():
    from gss import _lib
    x, z = clustered(500, 2, 1), values(500, 2, 1)
    z[1, 17] = np.nan
    with pytest.raises(_lib.GSSError) as e:
        _engine().variogram_empirical(x, z, 10, 20.0)
    assert e.value.code == _lib.ERR_INVALID and "NaN" in str(e.value)


@pytest.mark.parametrize("n", [500, 40000])
def test_non_finite_coordinates_are_refused(n):
    """found before anything is ordered by them, on both orderings; on device arrays the outputs carry the refusal"""
    import torch
    from gss import _lib
    x, z = clustered(n, 2, 1), values(n, 1, 1)
    x[n // 3, 1] = np.inf
    with pytest.raises(_lib.GSSError) as e:
        _engine().variogram_empirical(x, z, 10, 20.0)
    assert e.value.code == _lib.ERR_INVALID and "NaN" in str(e.value)
    count, lagsum, zsum, ndup = _engine().variogram_empirical(torch.as_tensor(x, device="cuda"),
                                                              torch.as_tensor(z, device="cuda"), 10, 20.0)
    assert int(ndup.cpu()[0]) == -1 and (count.cpu().numpy() == -1).all()
    assert np.isnan(lagsum.cpu().numpy()).all() and np.isnan(zsum.cpu().numpy()).all()


def test_front_end_drops_missing_values_per_variable():
    """A pair takes part in a variable only if both values exist: a variable with NaNs equals the variogram of its
    own finite samples, and the complete variable beside it is untouched."""
    import gss
    x, z = clustered(1200, 2, 2), values(1200, 2, 3)
    z[1, ::7] = np.nan
    both = gss.EmpiricalVariogram(gss.georef({"a": z[0], "b": z[1]}, x), ["a", "b"], nlags=15, maxlag=25.0)
    keep = np.isfinite(z[1])
    ra = vref.empirical(x, z[:1], 15, 25.0)
    rb = vref.empirical(x[keep], z[1:, keep], 15, 25.0)
    assert np.array_equal(both["a"].counts, ra[0]) and np.array_equal(both["b"].counts, rb[0])
    assert np.allclose(both["a"].ordinate, ra[2][0] / (2 * ra[0]), rtol=1e-12)
    assert np.allclose(both["b"].ordinate, rb[2][0] / (2 * rb[0]), rtol=1e-12)
    assert np.allclose(both["b"].abscissa, rb[1] / rb[0], rtol=1e-12)


def test_end_to_end_fftgs_field_to_kriging():
    """One unconditional FFTGS realisation (exponential, range 30, 512 x 512), 20 000 random cells as samples,
    empirical variogram, fit, kriging with the fitted model.  Only structure is asserted; how close the fitted range
    comes to 30 is a statistical quantity: printed (DESIGN.md section 4 records the value of the first run)."""
    import gss
    grid = gss.CartesianGrid(512, 512)
    ens = gss.solve(gss.SimulationProblem(grid, ("z", float), 1),
                    gss.FFTGS(("z", dict(variogram=gss.ExponentialVariogram(range=30.0))), rng=2024))
    field = np.asarray(ens["z"][0])
    cells = np.sort(np.random.default_rng(5).choice(512 * 512, 20000, replace=False))
    data = gss.georef({"z": field[cells]}, grid.centroids()[cells])
    g = gss.EmpiricalVariogram(data, "z", nlags=30, maxlag=90.0)
    assert (g.counts > 0).all() and g.nduplicates == 0 and np.isfinite(g.ordinate).all()
    model, obj = gss.fit(["exponential"], g, return_objectives=True)
    print("fitted %s: sill %.4f nugget %.4f range %.3f (generating range 30, sill 1); objective %.3e"
          % (model.kind, model.sill, model.nugget, model.range, obj["exponential"]))
    assert model.kind == "exponential"
    assert 0.0 <= model.nugget <= model.sill
    h = g.abscissa
    assert h.min() / 4 <= model.range <= 4 * h.max()
    sub = gss.georef({"z": field[cells[:1500]]}, grid.centroids()[cells[:1500]])
    sol = gss.solve(gss.EstimationProblem(sub, gss.CartesianGrid(64, 64), "z"),
                    gss.KrigingSolver(("z", dict(variogram=model, maxneighbors=16))))
    assert np.isfinite(sol["z"]).all() and (sol["z_variance"] > -1e-9).all()


def test_example_runs_and_its_results_are_sane():
    ns = runpy.run_path(os.path.join(ROOT, "examples", "variography.py"))
    out = ns["out"]
    g = out["empirical"]
    # 11 samples 10 apart: 10, 9, 8, 7, 6 pairs at lags 10 .. 50, each exactly on a bin edge
    assert np.array_equal(g.counts, [10, 9, 8, 7, 6]) and g.nduplicates == 0
    assert np.allclose(g.abscissa, [10, 20, 30, 40, 50]) and (np.diff(g.ordinate) > 0).all()
    m = out["model"]
    assert m.kind in ("gaussian", "spherical", "exponential") and 0 <= m.nugget <= m.sill and 2.5 <= m.range <= 200
    assert out["objectives"][m.kind] == min(out["objectives"].values())
    mu, var = out["kriging"]
    assert mu.shape == (100,) and np.isfinite(mu).all() and (var > -1e-9).all()
    assert np.array_equal(out["both"]["z"].counts, g.counts) and np.allclose(out["both"]["z"].ordinate, g.ordinate)
    assert np.array_equal(out["directional"].counts, g.counts)      # on a line every pair lies along the axis
