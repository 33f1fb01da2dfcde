"""SPDEGS on the device against tests/spde_ref.py: the assembled operator, the solve, the reference's covariance, the
element values, the independence of the columns of a block, non-convergence and the front end."""
import numpy as np
import pytest

import gss
from gss import _lib
from gss.engine import SPDEHandle
from oracle import philox

import spde_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-10


def _handle(name, noise="reference", dim=None):
    V, T, sill, rng = R.mesh(name)
    if dim == 3 and V.shape[1] == 2:
        V = np.concatenate([V, np.zeros((len(V), 1))], axis=1)
    return SPDEHandle(V, T, sill=sill, range=rng, noise=noise)


def _cond(S):
    return float(np.linalg.cond(S))


# ---- 1. operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dim", [("jitter", 2), ("jitter", 3), ("sphere", 3), ("fan", 2), ("fan", 3), ("strip", 2),
                                      ("strip", 3)])
def test_operator_matches_the_dense_restatement(name, dim):
    V, T, sill, rng = R.mesh(name)
    _, m, S, tau2 = R.dense(name)
    h = _handle(name, dim=dim)
    rowptr, col, val, mass = h.operator()
    nv = len(m)
    assert (h.nv, h.nt, h.nnz) == (nv, len(T), np.count_nonzero(S)) and abs(h.tau2 - tau2) <= 4 * R.EPS * tau2
    assert rowptr[0] == 0 and rowptr[-1] == h.nnz and (np.diff(rowptr) > 0).all()
    D = np.zeros((nv, nv))
    for v in range(nv):
        c = col[rowptr[v]:rowptr[v + 1]]
        assert (np.diff(c) > 0).all() and c[0] >= 0 and c[-1] < nv           # strictly ascending, in range
        D[v, c] = val[rowptr[v]:rowptr[v + 1]]
    err, merr = np.max(np.abs(D - S)), np.max(np.abs(mass - m) / m)
    print(name, dim, "max|S| %.4g" % np.max(np.abs(S)), "operator error %.3g" % err, "mass error %.3g" % merr)
    assert err <= 8 * R.EPS * np.max(np.abs(S))
    assert merr <= 4 * R.EPS
    h2 = _handle(name, dim=dim)
    for a, b in zip((rowptr, col, val, mass), h2.operator()):
        assert a.tobytes() == b.tobytes()
    h.close()
    h2.close()


def test_device_arrays_give_the_same_operator_and_are_checked_on_the_device():
    import torch
    V, T, sill, rng = R.mesh("jitter")
    ref = _handle("jitter").operator()
    h = SPDEHandle(torch.as_tensor(V, device="cuda"), torch.as_tensor(T, device="cuda"), sill=sill, range=rng)
    for a, b in zip(ref, h.operator()):
        assert a.tobytes() == b.tobytes()
    h.close()
    bad = {"outside": T.copy(), "repeats": T.copy(), "no triangle": T[2:].copy()}
    bad["outside"][5, 1] = len(V)
    bad["repeats"][7, 2] = bad["repeats"][7, 0]
    for word, tri in bad.items():
        with pytest.raises(_lib.GSSError, match=word) as e:
            SPDEHandle(torch.as_tensor(V, device="cuda"), torch.as_tensor(tri, device="cuda"), sill=sill, range=rng)
        assert e.value.code == _lib.ERR_INVALID
    Vn = V.copy()
    Vn[9, 1] = np.nan
    with pytest.raises(_lib.GSSError, match="vertex 9 has a coordinate that is not finite"):
        SPDEHandle(torch.as_tensor(Vn, device="cuda"), torch.as_tensor(T, device="cuda"), sill=sill, range=rng)
    Vz = V.copy()
    Vz[T[3, 1]] = Vz[T[3, 0]]
    with pytest.raises(_lib.GSSError, match="no area"):
        SPDEHandle(torch.as_tensor(Vz, device="cuda"), torch.as_tensor(T, device="cuda"), sill=sill, range=rng)


# ---- 2. solve ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["reference", "lumped"])
@pytest.mark.parametrize("name", ["jitter", "sphere"])
def test_solve_reaches_the_residual_and_the_direct_solution(name, noise):
    _, m, S, tau2 = R.dense(name)
    nv = len(m)
    w = np.random.default_rng(3).normal(size=(5, nv))
    b = R.rhs_scale(m, tau2, noise == "lumped")[:, None] * w.T
    _, host_iters = R.cg(S, b, RTOL)
    h = _handle(name, noise)
    z, _ = h.realize(0, 0, 5, noise=w, rtol=RTOL, vertices=True)
    iters, relres, unconverged = h.last_solve()
    zs = np.linalg.solve(S, b)
    res = np.linalg.norm(b - S @ z.T, axis=0) / np.linalg.norm(b, axis=0)
    err = np.linalg.norm(z.T - zs, axis=0) / np.linalg.norm(zs, axis=0)
    print(name, noise, "iterations", iters, "host", host_iters, "recursive %.3g" % relres, "true", res, "error", err,
          "cond %.4g" % _cond(S))
    assert unconverged == 0 and relres <= RTOL
    assert (res <= 2 * RTOL).all()
    assert (err <= 2 * RTOL * _cond(S)).all()
    for c in range(5):                                   # a column alone: its own iteration count, the same bits
        zc, _ = h.realize(0, 0, 1, noise=w[c:c + 1], rtol=RTOL, vertices=True)
        assert 1 <= h.last_solve()[0] <= 2 * host_iters[c]
        assert zc[0].tobytes() == z[c].tobytes()
    assert iters <= 2 * host_iters.max()
    h.close()


# ---- 3. the reference's covariance -------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["reference", "lumped"])
@pytest.mark.parametrize("name", ["jitter", "fan"])
def test_realisations_of_the_unit_vectors_give_the_covariance_of_spde_jl(name, noise):
    """w = e_r for every vertex r in one call (full blocks and a short one): Z'Z is the covariance of the field, which
    spde.jl:60-68 states as inv(A'A / tau^2) -- and tau^2 inv(S) M inv(S) for the lumped noise."""
    V, T, sill, rng = R.mesh(name)
    _, m, S, tau2 = R.dense(name)
    nv = len(m)
    Si = np.linalg.inv(S)
    Cref = tau2 * Si @ np.diag(m) @ Si if noise == "lumped" else R.reference_cov(V, T, sill, rng)
    bound = 8 * RTOL * _cond(S) * np.max(np.abs(Cref))
    L, _ = R.cg(S, np.diag(R.rhs_scale(m, tau2, noise == "lumped")), RTOL)
    assert np.max(np.abs(L @ L.T - Cref)) <= bound                     # the host CG meets the bound
    h = _handle(name, noise)
    Z, _ = h.realize(0, 0, nv, noise=np.eye(nv), rtol=RTOL, vertices=True)
    err = np.max(np.abs(Z.T @ Z - Cref))
    print(name, noise, "max|C| %.4g" % np.max(np.abs(Cref)), "error %.3g" % err, "bound %.3g" % bound)
    assert h.last_solve()[2] == 0
    assert err <= bound
    h.close()


# ---- 4. element values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["strip", "sphere"])
def test_element_values_are_the_vertex_means(name):
    V, T, _, _ = R.mesh(name)
    h = _handle(name)
    v, e = h.realize(11, 2, 3, vertices=True)
    assert v.shape == (3, len(V)) and e.shape == (3, len(T))
    tri = v[:, T]                                                      # (3, nt, 3)
    ref = tri.mean(axis=2)
    err = np.max(np.abs(e - ref) / np.abs(tri).max(axis=2))
    print(name, "element error %.3g" % err)
    assert err <= 2 * R.EPS
    assert h.realize(11, 2, 3).tobytes() == e.tobytes()                # elements alone: the same bits
    import torch
    vd, ed = h.realize(11, 2, 3, vertices=True, device=True)           # device outputs: the same bits
    assert isinstance(ed, torch.Tensor) and ed.is_cuda
    assert vd.cpu().numpy().tobytes() == v.tobytes() and ed.cpu().numpy().tobytes() == e.tobytes()
    h.close()


# ---- 5. independence of columns --------------------------------------------------------------------------------------------
def test_splitting_a_call_changes_no_bit():
    h = _handle("sphere")
    v, e = h.realize(7, 0, 19, vertices=True)
    assert np.isfinite(v).all() and h.last_solve()[2] == 0
    parts = [h.realize(7, lo, n, vertices=True) for lo, n in ((0, 1), (1, 15), (16, 3))]
    assert np.concatenate([p[0] for p in parts]).tobytes() == v.tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == e.tobytes()
    v2, e2 = h.realize(7, 0, 19, vertices=True)
    assert v2.tobytes() == v.tobytes() and e2.tobytes() == e.tobytes()
    assert len({v[r].tobytes() for r in range(19)}) == 19              # and the realisations differ
    h.close()


def test_a_column_does_not_see_its_companions():
    """Companions that stop at other iterations (a zero column, an early one), and one scaled by 1e8: the bits of a
    column are those of the column alone."""
    h = _handle("sphere")
    w = R.mixed_columns("sphere")
    z, _ = h.realize(0, 0, 5, noise=w, vertices=True)
    iters_block = h.last_solve()[0]
    alone, iters = [], []
    for c in range(5):
        alone.append(h.realize(0, 0, 1, noise=w[c:c + 1], vertices=True)[0][0])
        iters.append(h.last_solve()[0])
    print("iterations alone", iters, "block", iters_block)
    assert iters[1] == 0 and 0 < iters[3] < iters[0] and iters_block == max(iters)
    for c in range(5):
        assert alone[c].tobytes() == z[c].tobytes(), c
    assert not z[1].any()                                              # the zero column: x = 0, never touched
    w8 = w.copy()
    w8[2] *= 1e8
    z8, _ = h.realize(0, 0, 5, noise=w8, vertices=True)
    for c in (0, 1, 3, 4):
        assert z8[c].tobytes() == z[c].tobytes(), c
    assert np.allclose(z8[2], 1e8 * z[2], rtol=1e-6)
    h.close()


def test_the_seeded_normals_are_the_philox_stream():
    _, m, S, tau2 = R.dense("sphere")
    nv = len(m)
    h = _handle("sphere")
    z, _ = h.realize(21, 4, 3, vertices=True)
    lib_w = np.empty((3, nv))
    for r in range(3):
        _lib.check(_lib.lib().gss_philox_normal(21, 4 + r, nv, _lib.ptr(lib_w[r]), 0, None))
    zl, _ = h.realize(0, 0, 3, noise=lib_w, vertices=True)
    assert zl.tobytes() == z.tobytes()                                 # the library's normals: the same bits
    w = np.stack([philox.normal(21, 4 + r, nv) for r in range(3)])
    assert np.max(np.abs(w - lib_w)) < 1e-13                           # (tests/test_gpu_fftgs.py holds the device to this)
    zo, _ = h.realize(0, 0, 3, noise=w, vertices=True)
    # z is linear in w: the difference of the normals through tau inv(S) M, and each solve within 2 rtol cond of exact
    G = np.sqrt(tau2) * np.linalg.inv(S) * m[None, :]
    bound = np.linalg.norm(G, 2) * 1e-13 * np.sqrt(nv) + 4 * RTOL * _cond(S) * np.linalg.norm(z, axis=1).max()
    assert np.linalg.norm(zo - z, axis=1).max() <= bound
    h.close()


# ---- 6. non-convergence ----------------------------------------------------------------------------------------------------
def test_a_solve_that_runs_out_of_iterations_says_so():
    h = _handle("jitter")
    with pytest.raises(_lib.GSSError, match="realisation 2 did not reach") as e:
        h.realize(5, 2, 4, maxiter=3)
    assert e.value.code == _lib.ERR_NO_CONVERGENCE == 7
    iters, relres, unconverged = h.last_solve()
    assert iters == 3 and unconverged == 4 and relres > RTOL
    out = h.realize(5, 2, 4)
    assert np.isfinite(out).all() and h.last_solve()[2] == 0 and h.last_solve()[0] > 3
    h.close()


# ---- 7. front end ------------------------------------------------------------------------------------------------------------
def test_front_end_returns_the_handle_level_realisations(monkeypatch):
    V, T, _, _ = R.mesh("jitter")
    mesh = gss.SimpleMesh(V, T)
    sol = gss.solve(gss.SimulationProblem(mesh, ("z", float), 5), gss.SPDEGS(("z", dict(sill=1.5, range=4.0)), rng=3))
    assert isinstance(sol, gss.Ensemble) and len(sol) == 5 and sol.domain is mesh
    h = SPDEHandle(V, T, sill=1.5, range=4.0)
    ref = h.realize(3, 0, 5)
    h.close()
    for r in range(5):
        assert sol["z"][r].shape == (len(T),) and np.isfinite(sol["z"][r]).all()
        assert np.array_equal(sol["z"][r], ref[r]) and np.array_equal(sol[r].z, ref[r])
    # the generic loop of the reference (one realisation per solvesingle call) gives the same ensemble
    loop = gss.simulate_with_generic_loop(gss.SimulationProblem(mesh, ("z", float), 3),
                                          gss.SPDEGS(("z", dict(sill=1.5, range=4.0)), rng=3))
    for r in range(3):
        assert np.array_equal(loop["z"][r], ref[r])
    # equal parameters share a handle, and two variables get different fields
    made = []

    class Engine(gss.engine.HipEngine):
        @staticmethod
        def SPDE(*a, **kw):
            made.append(kw)
            return SPDEHandle(*a, **kw)
    p = dict(sill=1.5, range=4.0)
    two = gss.solve(gss.SimulationProblem(mesh, (("a", float), ("b", float)), 2),
                    gss.SPDEGS(("a", p), ("b", p), rng=3, engine=Engine))
    assert len(made) == 1
    assert np.array_equal(two["a"][0], ref[0]) and not np.array_equal(two["a"][0], two["b"][0])
    three = gss.solve(gss.SimulationProblem(mesh, (("a", float), ("b", float)), 1),
                      gss.SPDEGS(("a", p), ("b", dict(sill=1.5, range=2.0)), rng=3, engine=Engine, noise="lumped"))
    assert len(made) == 3 and made[-1]["noise"] == "lumped" and np.isfinite(three["b"][0]).all()
    with pytest.raises(RuntimeError, match="did not reach"):
        gss.solve(gss.SimulationProblem(mesh, ("z", float), 2), gss.SPDEGS(("z", p), rng=3, maxiter=2))
