"""SPDEGS without a device: the identity the sparse solve rests on, the host restatement of the CG the GPU tests compare
with, the front end's refusals and the argument checks of gss_spde_create."""
import ctypes as C

import numpy as np
import pytest

import gss
from gss import _lib

import spde_ref as R


@pytest.mark.parametrize("name", ["jitter", "sphere"])
def test_sparse_solve_has_the_covariance_of_the_dense_method(name):
    """inv(A'A / tau^2) of spde.jl:60-64 equals tau^2 inv(S) diag(m^2) inv(S) with S = kappa^2 M - B = M A."""
    V, T, sill, rng = R.mesh(name)
    _, m, S, tau2 = R.dense(name)
    Cref = R.reference_cov(V, T, sill, rng)
    Si = np.linalg.inv(S)
    C2 = tau2 * Si @ np.diag(m * m) @ Si
    err = np.max(np.abs(Cref - C2))
    print(name, "max|C| %.4g" % np.max(np.abs(Cref)), "max abs difference %.3g" % err)
    assert err <= 1e-9 * np.max(np.abs(Cref))
    assert np.allclose(S, S.T, rtol=0, atol=8 * R.EPS * np.max(np.abs(S))) and np.linalg.eigvalsh(S).min() > 0


@pytest.mark.parametrize("lumped", [False, True])
@pytest.mark.parametrize("name", R.MESHES)
def test_host_cg_reaches_the_true_residual(name, lumped):
    _, m, S, tau2 = R.dense(name)
    w = np.random.default_rng(2).normal(size=(len(m), 5))
    b = R.rhs_scale(m, tau2, lumped)[:, None] * w
    x, iters = R.cg(S, b, 1e-10)
    res = np.linalg.norm(b - S @ x, axis=0) / np.linalg.norm(b, axis=0)
    print(name, "iterations", iters, "true residuals", res)
    assert (res <= 2e-10).all() and (iters >= 1).all()
    x1, it1 = R.cg(S, b[:, 3], 1e-10)                       # a column alone (another BLAS product: not the same bits)
    assert np.linalg.norm(x1 - x[:, 3]) <= 4e-10 * np.linalg.cond(S) * np.linalg.norm(x1) and abs(it1 - iters[3]) <= 1


def test_host_cg_columns_of_the_mixed_block_stop_at_different_iterations():
    """The block tests/test_gpu_spde.py uses for the frozen-column path really has columns that finish apart."""
    _, m, S, tau2 = R.dense("sphere")
    b = R.rhs_scale(m, tau2, False)[:, None] * R.mixed_columns("sphere").T
    _, iters = R.cg(S, b, 1e-10)
    print("iterations", iters)
    assert iters[1] == 0 and 0 < iters[3] < iters[0] // 2      # done at once, done early, running on


@pytest.mark.parametrize("name,lumped", [("jitter", False), ("jitter", True), ("fan", False), ("fan", True)])
def test_host_cg_meets_the_covariance_bound(name, lumped):
    """What tests/test_gpu_spde.py asks of the device, asked of the host CG first: the realisations of the unit vectors
    reproduce the reference's covariance to 8 rtol cond(S) max|C|."""
    V, T, sill, rng = R.mesh(name)
    _, m, S, tau2 = R.dense(name)
    Si = np.linalg.inv(S)
    Cref = tau2 * Si @ np.diag(m) @ Si if lumped else R.reference_cov(V, T, sill, rng)
    L, _ = R.cg(S, np.diag(R.rhs_scale(m, tau2, lumped)), 1e-10)
    err = np.max(np.abs(L @ L.T - Cref))
    bound = 8 * 1e-10 * np.linalg.cond(S) * np.max(np.abs(Cref))
    print(name, lumped, "error %.3g" % err, "bound %.3g" % bound)
    assert err <= bound


def test_front_end_defaults_and_refusals():
    s = gss.SPDEGS()
    assert s.params("z") == dict(sill=1.0, range=1.0)
    assert s.globals["noise"] == "reference" and s.globals["rtol"] == 1e-10 and s.globals["maxiter"] is None
    assert s.globals["rng"] is None
    with pytest.raises(ValueError, match="invalid parameters"):
        gss.SPDEGS(("z", dict(variogram=None)))
    mesh = gss.triangulate(gss.CartesianGrid(4, 3))
    data = gss.georef({"z": [1.0]}, [(0.5, 0.5)])
    with pytest.raises(NotImplementedError, match="conditional simulation is not implemented"):
        gss.solve(gss.SimulationProblem(data, mesh, ("z", float), 2), gss.SPDEGS())
    with pytest.raises(ValueError, match="triangulate"):
        gss.solve(gss.SimulationProblem(gss.CartesianGrid(4, 3), ("z", float), 2), gss.SPDEGS())


def test_triangulate_and_simple_mesh():
    grid = gss.CartesianGrid((5, 3), (1.0, -2.0), (0.5, 2.0))
    mesh = gss.triangulate(grid)
    assert mesh.nvertices == 6 * 4 and mesh.nelements() == 2 * 5 * 3 == len(mesh) and mesh.embeddim() == 2
    assert mesh.vertices.min(axis=0).tolist() == [1.0, -2.0] and mesh.vertices.max(axis=0).tolist() == [3.5, 4.0]
    assert np.array_equal(np.unique(mesh.triangles), np.arange(24))
    u = mesh.vertices[mesh.triangles[:, 1]] - mesh.vertices[mesh.triangles[:, 0]]
    v = mesh.vertices[mesh.triangles[:, 2]] - mesh.vertices[mesh.triangles[:, 0]]
    assert np.allclose(0.5 * (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]), 0.5)      # counter-clockwise halves of a cell
    # the same diagonal in every cell: the two triangles of a cell share its first and its last node
    tri = mesh.triangles.reshape(-1, 2, 3)
    assert (tri[:, 0, 0] == tri[:, 1, 0]).all() and (tri[:, 0, 2] == tri[:, 1, 1]).all()
    assert np.allclose(mesh.centroids(), mesh.vertices[mesh.triangles].mean(axis=1))
    assert np.allclose(mesh.centroids()[0], [1.0 + 0.5 * 2 / 3, -2.0 + 2.0 / 3])
    with pytest.raises(ValueError):
        gss.triangulate(gss.CartesianGrid(3, 3, 3))
    with pytest.raises(ValueError):
        gss.SimpleMesh(np.zeros((4, 2)), np.zeros((2, 4), dtype=int))
    V, T, _, _ = R.mesh("strip")
    assert gss.SimpleMesh(V, T) == gss.SimpleMesh(V.copy(), T.copy())
    assert gss.SPDEGS is not None and "SimpleMesh" in gss.__all__ and "triangulate" in gss.__all__


def _create(V, T, sill=1.0, rng=1.0, dim=None, nv=None, nt=None, flags=0):
    V = np.ascontiguousarray(V, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.int64)
    h = C.c_void_p()
    code = _lib.load().gss_spde_create(C.byref(h), _lib.ptr(V), V.shape[0] if nv is None else nv,
                                       V.shape[1] if dim is None else dim, _lib.ptr(T),
                                       T.shape[0] if nt is None else nt, sill, rng, flags, _lib.MEM_HOST, None)
    assert h.value is None
    return code, _lib.last_error()


SQUARE = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
TWO = np.array([[0, 1, 2], [0, 2, 3]])

INVALID = {
    "nan coordinate": (dict(V=np.array([[0.0, 0.0], [1.0, np.nan], [1.0, 1.0], [0.0, 1.0]]), T=TWO), "not finite"),
    "inf coordinate": (dict(V=np.array([[0.0, 0.0], [1.0, 0.0], [np.inf, 1.0], [0.0, 1.0]]), T=TWO), "not finite"),
    "zero sill": (dict(V=SQUARE, T=TWO, sill=0.0), "sill"),
    "negative sill": (dict(V=SQUARE, T=TWO, sill=-1.0), "sill"),
    "nan sill": (dict(V=SQUARE, T=TWO, sill=float("nan")), "sill"),
    "zero range": (dict(V=SQUARE, T=TWO, rng=0.0), "range"),
    "negative range": (dict(V=SQUARE, T=TWO, rng=-2.0), "range"),
    "index == nv": (dict(V=SQUARE, T=np.array([[0, 1, 2], [0, 2, 4]])), "outside"),
    "negative index": (dict(V=SQUARE, T=np.array([[0, 1, 2], [0, -1, 3]])), "outside"),
    "repeated vertex": (dict(V=SQUARE, T=np.array([[0, 1, 2], [0, 2, 2]])), "repeats"),
    "collinear triangle": (dict(V=np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [0.0, 1.0]]),
                                T=np.array([[0, 1, 3], [0, 1, 2]])), "no area"),
    "coincident vertices": (dict(V=np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 2.0]]),
                                 T=np.array([[0, 1, 3], [0, 1, 2]])), "no area"),
    "vertex in no triangle": (dict(V=SQUARE, T=np.array([[0, 1, 2]])), "no triangle"),
    "two vertices": (dict(V=SQUARE[:2], T=np.array([[0, 1, 1]])), "at least 3"),
    "no triangle": (dict(V=SQUARE, T=TWO, nt=0), "at least 3"),
    "unknown flag": (dict(V=SQUARE, T=TWO, flags=2), "flags"),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_meshes_are_refused_without_a_device(case):
    kw, word = INVALID[case]
    code, msg = _create(**kw)
    assert code == _lib.ERR_INVALID and word in msg, (code, msg)


def test_unsupported_sizes_are_refused_without_a_device():
    for dim in (1, 4):
        code, msg = _create(SQUARE, TWO, dim=dim)
        assert code == _lib.ERR_UNSUPPORTED and "dimension" in msg
    code, msg = _create(SQUARE, TWO, nv=2 ** 31 - 1)
    assert code == _lib.ERR_UNSUPPORTED and "2^31" in msg
    code, msg = _create(SQUARE, TWO, nt=2 ** 31 // 12 + 1)
    assert code == _lib.ERR_UNSUPPORTED and "2^31" in msg
    assert _lib.ERR_NO_CONVERGENCE == 7
    assert _lib.load().gss_spde_realize(None, 0, 0, 1, None, 0.0, 0, None, None, 0, None) == _lib.ERR_INVALID
    assert _lib.load().gss_spde_last_solve(None, None, None, None) == _lib.ERR_INVALID
