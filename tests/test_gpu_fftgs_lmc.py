"""Co-simulation under a linear model of coregionalisation on the device (gss.h, gss_fftgs_create_lmc /
gss_fftgs_realize_lmc), against tests/fftgs_lmc_ref.py.

Every term of the mixture is fetched from the device through the exports the header names -- Y_j from
gss_fftgs_realize on a plain unit handle, E_j from gss_philox_normal, with the documented stream numbers --, the mixture is
formed in numpy and compared elementwise with the derived rounding bound (fftgs_lmc_ref.bound).  Grids: 24 x 20 x 16 (the
library's own Stockham passes), 15 x 14 (210 cells) and 101 (prime, rocFFT)."""
import ctypes as C

import numpy as np
import pytest

import fftgs_lmc_ref as R

pytestmark = pytest.mark.gpu

GRIDS = [(24, 20, 16), (15, 14), (101,)]


def _psd(n, rank, seed, ridge=0.0):
    A = np.random.default_rng(seed).normal(size=(n, rank))
    return A @ A.T / rank + ridge * np.eye(n)


def _structure(dims, **kw):
    import gss
    if "radii" in kw:
        return gss.ExponentialVariogram(gss.MetricBall(kw["radii"], kw.get("rotation")))
    return gss.ExponentialVariogram(range=kw.get("range", 0.3 * dims[0]))


def _handles(dims, b0, b1, means, **kw):
    """(LMC handle, plain unit handle of the same structure)."""
    from gss.engine import FFTGSHandle
    st = _structure(dims, **kw)
    return FFTGSHandle.lmc(st, b0, b1, means, dims), FFTGSHandle(st, dims)


def _normal(seed, real, n):
    from gss import _lib
    out = np.empty(n)
    _lib.check(_lib.lib().gss_philox_normal(seed ^ R.NUGGET_SALT, real, n, _lib.ptr(out), 0, None))
    return out


def _expected(plain, b0, b1, means, seed, r, N, noise=None, nugget=None):
    """Realisation r term by term: (Z[nz, N], bound[nz, N], live0, live1)."""
    L0, live0 = R.factor(b0, "b0")
    L1, live1 = R.factor(b1, "b1")
    nz = len(means)
    if noise is None:
        Y = {j: plain.realize(seed, r * nz + j, 1)[0] for j in live1}
    else:
        Y = {j: plain.realize(0, 0, 1, noise=np.ascontiguousarray(noise[j][None]))[0] for j in live1}
    E = {j: (_normal(seed, r * nz + j, N) if nugget is None else nugget[j]) for j in live0}
    if not Y and not E:
        Y = {}
        Z = np.repeat(np.asarray(means, dtype=np.float64)[:, None], N, axis=1)
        return Z, R.bound(live0, live1, np.abs(Z)), live0, live1
    Z, S = R.mix(L0, live0, L1, live1, means, Y, E)
    return Z, R.bound(live0, live1, S), live0, live1


def _cases():
    v3 = np.array([1.0, -0.6, 0.8])
    mid = np.outer([1.0, 2.0, 0.5], [1.0, 2.0, 0.5]) + np.outer([0.0, 0.0, 1.5], [0.0, 0.0, 1.5])
    rot = ((np.cos(0.6), -np.sin(0.6)), (np.sin(0.6), np.cos(0.6)))
    return {
        "nz=1": ((24, 20, 16), np.array([[0.2]]), np.array([[1.3]]), [0.5], {}),
        "nz=2 full rank": ((15, 14), _psd(2, 2, 1, 0.1), _psd(2, 2, 2, 0.1), [1.0, -2.0], {}),
        "nz=3 full rank": ((24, 20, 16), _psd(3, 3, 3, 0.1), _psd(3, 3, 4, 0.1), [0.0, 3.0, -1.0], {}),
        "nz=8 full rank": ((15, 14), _psd(8, 8, 5, 0.05), _psd(8, 8, 6, 0.05), np.arange(8.0) - 3.0, {}),
        "nz=8 1-D": ((101,), _psd(8, 8, 7, 0.05), _psd(8, 8, 8, 0.05), np.zeros(8), {}),
        "rank-1 b1, nz=3": ((24, 20, 16), np.diag([0.1, 0.2, 0.3]), np.outer(v3, v3), [1.0, 2.0, 3.0], {}),
        "rank-1 b1, 1-D": ((101,), np.diag([0.1, 0.2, 0.3]), np.outer(v3, v3), [1.0, 2.0, 3.0], {}),
        "b0 = 0": ((15, 14), np.zeros((3, 3)), _psd(3, 3, 9, 0.1), [0.0, 0.0, 7.0], {}),
        "zero middle column": ((15, 14), np.diag([0.0, 0.3, 0.0]), mid, [0.0, 1.0, 0.0], {}),
        "rotated anisotropy 2-D": ((15, 14), _psd(2, 2, 10, 0.1), _psd(2, 2, 11, 0.1), [0.5, 0.25],
                                   dict(radii=(6.0, 2.0), rotation=rot)),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_mixture_parity_term_by_term(name):
    dims, b0, b1, means, kw = CASES[name]
    N, nz, seed = int(np.prod(dims)), len(means), 20240
    h, plain = _handles(dims, b0, b1, means, **kw)
    z = h.realize_lmc(seed, 2, 2)
    assert z.shape == (2, nz, N) and np.all(np.isfinite(z))
    for i, r in enumerate((2, 3)):
        ref, bnd, live0, live1 = _expected(plain, b0, b1, means, seed, r, N)
        err = np.abs(z[i] - ref)
        print(name, "r", r, "live0", live0, "live1", live1, "max err", err.max(), "max err / bound",
              np.max(err / np.maximum(bnd, 1e-300)))
        assert np.all(err <= bnd)
    h.close()
    plain.close()


@pytest.mark.parametrize("name", ["nz=3 full rank", "rank-1 b1, 1-D", "zero middle column"])
def test_caller_noise(name):
    import torch
    dims, b0, b1, means, kw = CASES[name]
    N, nz = int(np.prod(dims)), len(means)
    rng = np.random.default_rng(5)
    noise, nugget = rng.uniform(size=(2, nz, N)), rng.normal(size=(2, nz, N))
    h, plain = _handles(dims, b0, b1, means, **kw)
    live0, live1 = R.factor(b0)[1], R.factor(b1)[1]
    for j in range(nz):                      # slots of dead columns are not read
        if j not in live1:
            noise[:, j] = np.nan
        if j not in live0:
            nugget[:, j] = np.nan
    z = h.realize_lmc(0, 0, 2, noise=noise, nugget_noise=nugget)
    zd = h.realize_lmc(0, 0, 2, noise=torch.as_tensor(noise, device="cuda"),
                       nugget_noise=torch.as_tensor(nugget, device="cuda"))
    assert np.all(np.isfinite(z)) and np.array_equal(zd.cpu().numpy(), z)
    for r in range(2):
        ref, bnd, _, _ = _expected(plain, b0, b1, means, 0, r, N, noise=noise[r], nugget=nugget[r])
        assert np.all(np.abs(z[r] - ref) <= bnd)
    # each of the two alone: the other comes from Philox with the documented numbers
    zu = h.realize_lmc(11, 1, 1, noise=noise[:1])
    ref, bnd, _, _ = _expected(plain, b0, b1, means, 11, 1, N, noise=noise[0])
    assert np.all(np.abs(zu[0] - ref) <= bnd)
    zn = h.realize_lmc(11, 1, 1, nugget_noise=nugget[:1])
    ref, bnd, _, _ = _expected(plain, b0, b1, means, 11, 1, N, nugget=nugget[0])
    assert np.all(np.abs(zn[0] - ref) <= bnd)
    h.close()
    plain.close()


@pytest.mark.parametrize("dims", GRIDS)
@pytest.mark.parametrize("rank1", [False, True])
def test_call_shape_does_not_matter(dims, rank1, monkeypatch):
    N, nz, seed = int(np.prod(dims)), 3, 77
    v3 = np.array([1.0, -0.6, 0.8])
    b0, b1, means = _psd(3, 3, 12, 0.1), (np.outer(v3, v3) if rank1 else _psd(3, 3, 13, 0.1)), [1.0, 0.0, -1.0]
    h, plain = _handles(dims, b0, b1, means)
    one = h.realize_lmc(seed, 3, 4)
    assert np.array_equal(np.concatenate([h.realize_lmc(seed, 3 + r, 1) for r in range(4)]), one)
    dev = h.realize_lmc(seed, 3, 4, device=True)                         # the in-place route
    assert np.array_equal(dev.cpu().numpy(), one)
    views = [np.arange(1, N, 3), np.random.default_rng(1).permutation(N)]
    for inds in views:
        assert np.array_equal(h.realize_lmc(seed, 3, 4, inds=inds), one[:, :, inds])
        assert np.array_equal(h.realize_lmc(seed, 3, 4, inds=inds, device=True).cpu().numpy(), one[:, :, inds])
    monkeypatch.setenv("GSS_FFTGS_LMC_CHUNK_REALS", "1")
    assert np.array_equal(h.realize_lmc(seed, 3, 4), one)
    assert np.array_equal(h.realize_lmc(seed, 3, 4, device=True).cpu().numpy(), one)
    assert np.array_equal(h.realize_lmc(seed, 3, 4, inds=views[0]), one[:, :, views[0]])
    h.close()
    plain.close()


def test_one_variable_without_nugget_is_a_plain_handle():
    import gss
    from gss.engine import FFTGSHandle
    from oracle import fftgs as O
    from oracle.variogram import Variogram
    dims, s, mean, seed = (24, 20, 16), 2.5, -0.75, 31
    N = int(np.prod(dims))
    h, plain = _handles(dims, [[0.0]], [[s]], [mean], range=6.0)
    z = h.realize_lmc(seed, 4, 1)[0, 0]
    y = plain.realize(seed, 4, 1)[0]
    ref = mean + np.sqrt(s) * y
    assert np.all(np.abs(z - ref) <= R.bound([], [0], abs(mean) + np.sqrt(s) * np.abs(y)))
    # ... and a plain handle of sill s, to the tolerance of tests/test_gpu_fftgs.py for a device realisation of an
    # algebraic spectrum against oracle/fftgs (1e-9)
    ps = FFTGSHandle(gss.ExponentialVariogram(range=6.0, sill=s), dims, None, mean)
    assert np.max(np.abs(z - ps.realize(seed, 4, 1)[0])) < 1e-9
    pre = O.preprocess(Variogram("exponential", range=6.0, sill=s), dims, mean=mean)
    assert np.max(np.abs(z - O.realize(pre, seed, 4, 1)[0])) < 1e-9
    for x in (h, plain, ps):
        x.close()


def test_handle_contract():
    import torch
    from gss import _lib
    from gss.engine import FFTGSHandle
    dims = (15, 14)
    b0, b1, means = _psd(2, 2, 1, 0.1), _psd(2, 2, 2, 0.1), [1.0, 2.0]
    h, plain = _handles(dims, b0, b1, means)
    assert np.array_equal(h.spectrum(), plain.spectrum())
    with pytest.raises(_lib.GSSError, match="gss_fftgs_realize_lmc") as e:
        h.realize(1, 0, 1)
    assert e.value.code == _lib.ERR_INVALID
    out = np.empty((1, 2, 210))
    code = _lib.lib().gss_fftgs_realize_lmc(plain._h, 1, 0, 1, None, None, None, 0, _lib.ptr(out), 0, None)
    assert code == _lib.ERR_INVALID and "gss_fftgs_realize" in _lib.last_error() and "plain" in _lib.last_error()
    one = h.realize_lmc(9, 0, 2)
    peer = FFTGSHandle.lmc(_structure(dims), b0, b1, means, dims, spectrum=False)
    with pytest.raises(_lib.GSSError, match="no spectrum"):
        peer.realize_lmc(9, 0, 2)
    peer.state_tensor().copy_(h.state_tensor())
    torch.cuda.synchronize()
    peer.adopt_state()
    assert np.array_equal(peer.realize_lmc(9, 0, 2), one)
    for x in (h, plain, peer):
        x.close()


def test_statistics_follow_the_model():
    """cov(Z_a(x), Z_b(x + h)) about the known means, averaged over the cells of a 64 x 64 grid and 64 realisations, at
    h = 0 and h = 4 cells along x, against b0 [h = 0] + b1 rho(h) (exponential, range 8; fftgs_lmc_ref.stat_model).

    The band was set with the numpy restatement (fftgs_lmc_ref.realize: oracle fields and oracle normals), never with the
    device: over 64 seeds (1000 .. 1063) the largest absolute deviations from the model were
        lag 0: [[0.002929, 0.009317], [0.009317, 0.015041]]     lag 4: [[0.010148, 0.012354], [0.012354, 0.018680]]
    about the model values [[1, 0.8], [0.8, 1]] and [[0.200817, 0.167348], [0.167348, 0.200817]]; the band of each entry
    is twice its deviation (the 64 seeds are not the worst case): lag 0 [[0.005858, 0.018634], [., 0.030083]], lag 4
    [[0.020296, 0.024709], [., 0.037361]].  One fixed seed here."""
    h, _plain = _handles(R.STAT_DIMS, R.STAT_B0, R.STAT_B1, R.STAT_MEANS, range=R.STAT_RANGE)
    _plain.close()
    z = h.realize_lmc(4242, 0, R.STAT_NREALS)
    h.close()
    got = R.lag_covariances(z, R.STAT_MEANS, R.STAT_DIMS, R.STAT_LAG)
    model = R.stat_model()
    print("covariances", got.tolist(), "model", model.tolist(), "deviation", np.abs(got - model).tolist())
    assert np.all(np.abs(got - model) <= 2.0 * STAT_MAXDEV)


# largest deviations of the numpy restatement over 64 seeds (the docstring of the test above)
STAT_MAXDEV = np.array([[[0.002928724876766875, 0.009316730456171318], [0.009316730456171318, 0.015041409443602882]],
                        [[0.01014752471165098, 0.012354238858017175], [0.012354238858017175, 0.018680219699901107]]])


def test_twin_end_to_end():
    import gss
    from types import SimpleNamespace
    from gss.engine import FFTGSHandle
    grid = gss.CartesianGrid(24, 20)
    lmc = SimpleNamespace(names=("zn", "pb", "cu"), kind="exponential", range=5.0, order=1.0,
                          B0=np.diag([0.2, 0.1, 0.3]), B1=_psd(3, 3, 21, 0.1))
    idx = [2, 0]                                             # ("cu", "zn") of the model's ("zn", "pb", "cu")
    b0, b1 = lmc.B0[np.ix_(idx, idx)], lmc.B1[np.ix_(idx, idx)]
    solver = lambda: gss.FFTGS(("cu", dict(mean=1.5)), (("cu", "zn"), dict(model=lmc)), rng=7)
    sol = gss.solve(gss.SimulationProblem(grid, {"cu": float, "zn": float}, 5), solver())
    h = FFTGSHandle.lmc(gss.ExponentialVariogram(range=5.0), b0, b1, [1.5, 0.0], grid.dims, grid.spacing)
    ref = h.realize_lmc(7, 0, 5)
    assert np.array_equal(np.stack(sol["cu"]), ref[:, 0]) and np.array_equal(np.stack(sol["zn"]), ref[:, 1])
    # a grid view
    inds = np.arange(3, 24 * 20, 7)
    vsol = gss.solve(gss.SimulationProblem(gss.view(grid, inds), {"cu": float, "zn": float}, 5), solver())
    assert np.array_equal(np.stack(vsol["zn"]), ref[:, 1][:, inds])
    # the generic loop (one realisation per call) gives the same ensemble
    loop = gss.solvers.simulate_with_generic_loop(gss.SimulationProblem(grid, {"cu": float, "zn": float}, 3), solver())
    assert np.array_equal(np.stack(loop["cu"]), ref[:3, 0])
    # a third, single-variable group is simulated as without the joint group
    vg = gss.SphericalVariogram(range=6.0, sill=2.0)
    both = gss.solve(gss.SimulationProblem(grid, {"cu": float, "zn": float, "w": float}, 4),
                     gss.FFTGS(("cu", dict(mean=1.5)), ("w", dict(variogram=vg)), (("cu", "zn"), dict(model=lmc)), rng=7))
    alone = gss.solve(gss.SimulationProblem(grid, {"cu": float, "zn": float, "w": float}, 4),
                      gss.FFTGS(("w", dict(variogram=vg)), rng=7))
    assert np.array_equal(np.stack(both["w"]), np.stack(alone["w"]))
    assert np.array_equal(np.stack(both["cu"]), ref[:4, 0])
    h.close()


def test_cosimulation_example_runs():
    """examples/cosimulation.py stays runnable: cross variogram -> fit_lmc -> FFTGS with the model as the joint parameter;
    the two simulated fields are correlated as the fitted model says (16 realisations of 128 x 128 cells of a model with
    a range of a tenth of the grid: the correlation of the ensemble is within 0.1 of the model's)."""
    import os
    import runpy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = runpy.run_path(os.path.join(root, "examples", "cosimulation.py"))["out"]
    assert len(out["ensemble"]["cu"]) == 16 and np.all(np.isfinite(np.stack(out["ensemble"]["zn"])))
    assert abs(out["correlation"] - out["lmc"].correlation("cu", "zn")) < 0.1
