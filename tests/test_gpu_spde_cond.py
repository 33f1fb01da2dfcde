"""SPDEGS with data on the device against tests/spde_cond_ref.py: point location, W = inv(S) P', the kriging mean, the
posterior covariance, honouring of exact data, the independence of the columns of a block, the seeded error normals,
the refusals and the front end.  Bound of the numeric comparisons (the solves run at rtol = 1e-13):
8 rtol cond(S) (1 + cond(P Sigma P' + R)) max|Sigma|, printed beside every measured error."""
import numpy as np
import pytest

import gss
from gss import _lib
from gss.engine import SPDEHandle

import spde_cond_ref as CR
import spde_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-13


def _handle(name, noise="reference"):
    V, T, sill, rng = R.mesh(name)
    return SPDEHandle(V, T, sill=sill, range=rng, noise=noise)


def _attach(h, name, mode, noisy, rtol=RTOL, device=False):
    _, idx, w, y, _ = CR.case(name, mode)
    arrs = [idx, w, y] + ([CR.error_variance(name, True)] if noisy else [])
    if device:
        import torch
        arrs = [torch.as_tensor(np.array(a), device="cuda") for a in arrs]
    h.condition(arrs[0], arrs[1], arrs[2], arrs[3] if noisy else None, mean=CR.MEAN, rtol=rtol)


def _dense(name, mode, lumped, noisy):
    """(P, Sigma, dense mean, dense posterior, bound) of a shared case."""
    _, m, S, _ = R.dense(name)
    _, idx, w, y, _ = CR.case(name, mode)
    P, Sigma = CR.dense_P(len(m), idx, w), CR.prior_cov(name, lumped)
    _, mean, post, C = CR.dense_kriging(Sigma, P, CR.error_variance(name, noisy), y, CR.MEAN)
    return P, Sigma, mean, post, CR.bound(RTOL, S, C, Sigma)


# ---- 1. locate -----------------------------------------------------------------------------------------------------
def _lowest_with(T, *verts):
    return int(np.flatnonzero(np.all([(T == v).any(axis=1) for v in verts], axis=0))[0])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["jitter", "sphere"])
def test_locate_returns_the_triangle_and_the_weights(name, device):
    V, T, _, _ = R.mesh(name)
    nt = len(T)
    edges = sorted({(min(a, b), max(a, b)) for t in T for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))})
    tri_d, _, w_d, _, pts_d = CR.case(name, "point")
    pts = [V[T].mean(axis=1), V, np.array([0.5 * V[a] + 0.5 * V[b] for a, b in edges]), pts_d]
    want = [np.arange(nt), np.array([_lowest_with(T, v) for v in range(len(V))]),
            np.array([_lowest_with(T, a, b) for a, b in edges]), tri_d]
    h = _handle(name)
    arg = np.concatenate(pts)
    if device:
        import torch
        arg = torch.as_tensor(arg, device="cuda")
    tri, w = h.locate(arg)
    if device:
        assert tri.is_cuda and w.is_cuda
        tri, w = tri.cpu().numpy(), w.cpu().numpy()
    assert tri.dtype == np.int64 and w.shape == (len(arg), 3)
    assert np.array_equal(tri, np.concatenate(want))
    # the weights rebuild the point, and are the known ones: 1/3, a 1 at the vertex, 1/2 at the two ends, the drawn ones
    o = np.cumsum([0] + [len(p) for p in pts])
    known = np.zeros((len(arg), 3))
    known[o[0]:o[1]] = 1.0 / 3.0
    for v in range(len(V)):
        known[o[1] + v, list(T[tri[o[1] + v]]).index(v)] = 1.0
    for i, (a, b) in enumerate(edges):
        known[o[2] + i, list(T[tri[o[2] + i]]).index(a)] = known[o[2] + i, list(T[tri[o[2] + i]]).index(b)] = 0.5
    known[o[3]:] = w_d
    err = np.max(np.abs(w - known))
    print(name, "device" if device else "host", len(arg), "points, weight error %.3g = %.1f eps" % (err, err / R.EPS))
    assert err <= 64 * R.EPS
    if name == "sphere":                                   # lifted off the surface along the triangle's normal
        n = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
        up = pts[0] + 1e-3 * n / np.linalg.norm(n, axis=1)[:, None]
        t3, w3 = h.locate(up)
        print("lifted: weight error %.3g" % np.max(np.abs(w3 - 1.0 / 3.0)))
        assert np.array_equal(t3, np.arange(nt))
        t4, _ = h.locate(pts_d * 1.001)
        assert np.array_equal(t4, tri_d)
    else:
        t3, w3 = h.locate(np.array([[-5.0, 2.0], [6.0, 5.0], [100.0, 100.0]]))
        assert t3[0] == -1 and t3[1] >= 0 and t3[2] == -1
        tm, wm = gss.SimpleMesh(V, T).locate(np.array([[6.0, 5.0]]))
        assert tm[0] == t3[1] and wm.tobytes() == w3[1:2].tobytes()
        assert not w3[0].any() and not w3[2].any()
    h.close()


# ---- 2. W ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", CR.MODES)
@pytest.mark.parametrize("name", R.MESHES)
def test_w_is_the_solution_of_s_w_equals_p_transposed(name, mode):
    _, m, S, _ = R.dense(name)
    P, _, _, _, bound = _dense(name, mode, False, False)
    h = _handle(name)
    _attach(h, name, mode, False)
    iters, relres, unconverged = h.last_solve()
    W = h.weights()
    err = np.max(np.abs(W - np.linalg.solve(S, P.T)))
    print(name, mode, "iterations", iters, "W error %.3g" % err, "bound %.3g" % bound)
    assert h.nd == CR.NOBS[name] and W.shape == (len(m), h.nd) and unconverged == 0 and relres <= RTOL
    assert err <= bound
    _attach(h, name, mode, False, device=True)             # device arrays, attached over the earlier data: the same bits
    assert h.weights().tobytes() == W.tobytes()
    h.close()


# ---- 3, 4, 5. the mean, the posterior covariance, honouring ------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("noise", ["reference", "lumped"])
@pytest.mark.parametrize("mode", CR.MODES)
@pytest.mark.parametrize("name", R.MESHES)
def test_mean_and_posterior_covariance_are_those_of_simple_kriging(name, mode, noise, noisy):
    """The realisations of the nv + nd unit vectors, the mean subtracted, are a square root of the posterior covariance
    Sigma - K P Sigma with Sigma from the reference's own Q (noise="reference"); and with R = 0 seeded realisations
    honour the data."""
    V, T, _, _ = R.mesh(name)
    P, Sigma, mean, post, bound = _dense(name, mode, noise == "lumped", noisy)
    nv, nd = P.shape[1], P.shape[0]
    y = CR.case(name, mode)[3]
    h = _handle(name, noise)
    _attach(h, name, mode, noisy)
    mv, me = h.mean(rtol=RTOL, vertices=True)
    errm = np.max(np.abs(mv - mean))
    assert h.last_solve()[2] == 0 and np.max(np.abs(me - mv[T].mean(axis=1))) <= 4 * R.EPS * np.max(np.abs(mv))
    Z, _ = h.realize(0, 0, nv + nd, noise=np.eye(nv + nd), rtol=RTOL, vertices=True)
    errp = np.max(np.abs((Z - mv).T @ (Z - mv) - post))
    print(name, mode, noise, noisy, "mean error %.3g" % errm, "posterior error %.3g" % errp, "bound %.3g" % bound,
          "max|post| %.3g" % np.max(np.abs(post)))
    assert h.last_solve()[2] == 0
    assert errm <= bound and errp <= bound
    v, e = h.realize(13, 3, 4, rtol=RTOL, vertices=True)
    if not noisy:
        errh = np.max(np.abs(v @ P.T - y))
        print("honouring %.3g" % errh)
        assert errh <= bound
    else:
        assert np.max(np.abs(v @ P.T - y)) > 1e-3          # noisy data are not interpolated
    assert len({v[r].tobytes() for r in range(4)}) == 4
    h.close()


# ---- 6. bits ---------------------------------------------------------------------------------------------------------
def test_splitting_a_call_or_moving_its_start_changes_no_bit():
    h = _handle("sphere")
    _attach(h, "sphere", "point", True)
    v, e = h.realize(7, 0, 19, vertices=True)
    assert np.isfinite(v).all() and h.last_solve()[2] == 0
    parts = [h.realize(7, lo, n, vertices=True) for lo, n in ((0, 1), (1, 15), (16, 3))]
    assert np.concatenate([p[0] for p in parts]).tobytes() == v.tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == e.tobytes()
    assert h.realize(7, 0, 19).tobytes() == e.tobytes()
    import torch
    vd, ed = h.realize(7, 0, 19, vertices=True, device=True)
    assert vd.cpu().numpy().tobytes() == v.tobytes() and ed.cpu().numpy().tobytes() == e.tobytes()
    h.close()


def test_a_column_does_not_see_its_companions():
    h = _handle("sphere")
    _attach(h, "sphere", "point", True)
    nd = h.nd
    w = np.concatenate([R.mixed_columns("sphere"), np.random.default_rng(6).normal(size=(5, nd))], axis=1)
    z, _ = h.realize(0, 0, 5, noise=w, vertices=True)
    for c in range(5):
        assert h.realize(0, 0, 1, noise=w[c:c + 1], vertices=True)[0][0].tobytes() == z[c].tobytes(), c
    w8 = w.copy()
    w8[2] *= 1e8
    z8, _ = h.realize(0, 0, 5, noise=w8, vertices=True)
    for c in (0, 1, 3, 4):
        assert z8[c].tobytes() == z[c].tobytes(), c
    import torch
    zd, _ = h.realize(0, 0, 5, noise=torch.as_tensor(w, device="cuda"), vertices=True)
    assert zd.cpu().numpy().tobytes() == z.tobytes()
    with pytest.raises(ValueError, match="nv \\+ nd"):
        h.realize(0, 0, 5, noise=w[:, :h.nv])
    h.close()


def test_the_unconditional_part_and_clearing_keep_their_bits():
    """Exact data that realisation r already honours leave it alone: its residual, lambda and correction are exactly
    zero, so x_c is the unconditional realisation of (seed, r) bit for bit, while its companions in the block move."""
    V, T, _, _ = R.mesh("sphere")
    h = _handle("sphere")
    xu, eu = h.realize(5, 0, 6, rtol=RTOL, vertices=True)
    verts = np.array([3, 40, 77, 101, 160])
    idx = np.stack([verts, (verts + 1) % len(V), (verts + 2) % len(V)], axis=1)
    wts = np.tile([1.0, 0.0, 0.0], (5, 1))
    h.condition(idx, wts, xu[4, verts], mean=0.0, rtol=RTOL)
    xc, ec = h.realize(5, 0, 6, rtol=RTOL, vertices=True)
    assert xc[4].tobytes() == xu[4].tobytes() and ec[4].tobytes() == eu[4].tobytes()
    for r in (0, 1, 2, 3, 5):
        assert np.max(np.abs(xc[r] - xu[r])) > 1e-3
        assert np.max(np.abs(xc[r, verts] - xu[4, verts])) <= 1e-9
    # x_c - x_u is the correction inv(S) (s^2 . (W lambda)) of the restatement
    _, m, S, tau2 = R.dense("sphere")
    ref = CR.Conditioned(S, R.rhs_scale(m, tau2, False), idx, wts, xu[4, verts], np.zeros(5), 0.0, RTOL)
    for r in (0, 1, 2, 3, 5):
        corr = ref._correct(ref.y - ref.P @ xu[r])
        err = np.max(np.abs((xc[r] - xu[r]) - corr))
        bound = 8 * RTOL * np.linalg.cond(S) * (1 + np.linalg.cond(ref.C)) * np.max(np.abs(xu))
        print("realisation", r, "correction error %.3g" % err, "bound %.3g" % bound)
        assert err <= bound
    h.condition_clear()
    assert h.nd == 0
    x2, e2 = h.realize(5, 0, 6, rtol=RTOL, vertices=True)
    assert x2.tobytes() == xu.tobytes() and e2.tobytes() == eu.tobytes()
    h.close()


# ---- 7. seeded error normals -------------------------------------------------------------------------------------------
def test_the_seeded_error_normals_continue_the_philox_stream():
    h = _handle("sphere")
    _attach(h, "sphere", "element", True)
    n = h.nv + h.nd
    z, _ = h.realize(21, 4, 3, vertices=True)
    w = np.empty((3, n))
    for r in range(3):
        _lib.check(_lib.lib().gss_philox_normal(21, 4 + r, n, _lib.ptr(w[r]), 0, None))
    zl, _ = h.realize(0, 0, 3, noise=w, vertices=True)
    assert zl.tobytes() == z.tobytes()
    w2 = w.copy()
    w2[:, h.nv:] += 1.0                                     # and the error normals do enter
    assert np.max(np.abs(h.realize(0, 0, 3, noise=w2, vertices=True)[0] - z)) > 1e-3
    h.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_without_data():
    V, T, _, _ = R.mesh("jitter")
    _, idx, w, y, _ = CR.case("jitter", "point")
    nd = len(y)
    h = _handle("jitter")
    ref = h.realize(5, 0, 3)

    def changed(a, at, value):
        a = np.array(a)
        a[at] = value
        return a
    bad = {"vertex index outside": (changed(idx, (4, 1), len(V)), w, y, None),
           "vertex index outside ": (changed(idx, (0, 0), -1), w, y, None),
           "weight that is not finite": (idx, changed(w, (2, 2), np.inf), y, None),
           "value that is not finite": (idx, w, changed(y, 7, np.nan), None),
           "negative error variance": (idx, w, y, changed(np.zeros(nd), 3, -1e-3)),
           "error variance that is not finite": (idx, w, y, changed(np.zeros(nd), 3, np.nan)),
           "at least one observation": (idx[:0], w[:0], y[:0], None)}
    noise = np.random.default_rng(8).normal(size=(3, h.nv))
    ref_noise = h.realize(0, 0, 3, noise=noise)

    def bare():
        """The library holds no data for the handle, and both forms of realize give the unconditional bits."""
        return (h.nd == 0 and h.attached()[0] == 0 and h.realize(5, 0, 3).tobytes() == ref.tobytes()
                and h.realize(0, 0, 3, noise=noise).tobytes() == ref_noise.tobytes())
    for word, args in bad.items():                         # every refusal meets a handle that carries valid data
        h.condition(idx, w, y, mean=1.0)
        assert h.attached() == (nd, 1.0) and h.realize(5, 0, 3).tobytes() != ref.tobytes()
        with pytest.raises(_lib.GSSError, match=word.strip()) as e:
            h.condition(*args)
        assert e.value.code == _lib.ERR_INVALID and bare(), word
    h.condition(idx, w, y)
    with pytest.raises(_lib.GSSError, match="mean is not finite"):
        h.condition(idx, w, y, mean=float("inf"))
    assert bare()
    h.condition(idx, w, y)
    with pytest.raises(_lib.GSSError, match="rtol"):
        h.condition(idx, w, y, rtol=2.0)
    assert bare()
    h.condition(idx, w, y)
    with pytest.raises(_lib.GSSError, match=r"not positive definite \(pivot 5\)") as e:    # rows 2 and 5 are the same
        h.condition(changed(idx, 5, idx[2]), changed(w, 5, w[2]), y)
    assert e.value.code == _lib.ERR_NOT_POSDEF and bare()
    h.condition(changed(idx, 5, idx[2]), changed(w, 5, w[2]), y, np.full(nd, 1e-2))           # fine once they are noisy
    assert h.nd == nd == h.attached()[0]
    with pytest.raises(_lib.GSSError, match="observation 0 did not reach") as e:             # an error return, no fault
        h.condition(idx, w, y, maxiter=3)
    assert e.value.code == _lib.ERR_NO_CONVERGENCE and h.nd == 0 and h.attached()[0] == 0
    iters, relres, unconverged = h.last_solve()
    assert iters == 3 and unconverged == nd and relres > 1e-10
    with pytest.raises(_lib.GSSError, match="carries no data") as e:
        h.mean()
    assert e.value.code == _lib.ERR_INVALID
    assert h.realize(5, 0, 3).tobytes() == ref.tobytes()       # unconditional, as before
    h.condition(idx, w, y)
    with pytest.raises(_lib.GSSError, match="realisation 2 did not reach") as e:
        h.realize(5, 2, 4, maxiter=3)
    assert e.value.code == _lib.ERR_NO_CONVERGENCE and h.last_solve()[2] == 4
    with pytest.raises(_lib.GSSError, match="did not reach"):
        h.mean(maxiter=2)
    assert np.isfinite(h.realize(5, 2, 4)).all() and h.last_solve()[2] == 0
    h.close()


# ---- 9. front end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", CR.MODES)
def test_front_end_returns_the_handle_level_realisations_and_the_mean(mode):
    V, T, sill, rng = R.mesh("jitter")
    tri, idx, w, y, pts = CR.case("jitter", mode)
    mesh = gss.SimpleMesh(V, T)
    yy = np.append(y, np.nan)                              # a missing value is skipped
    data = gss.georef({"z": yy}, np.concatenate([pts, [[3.0, 3.0]]]))
    p = dict(sill=sill, range=rng)
    sol = gss.solve(gss.SimulationProblem(data, mesh, ("z", float), 5),
                    gss.SPDEGS(("z", p), rng=3, condition=mode, mean=CR.MEAN, rtol=RTOL))
    h = SPDEHandle(V, T, sill=sill, range=rng)
    t2, w2 = h.locate(pts)
    assert np.array_equal(t2, tri)
    h.condition(T[t2], w if mode == "element" else w2, y, mean=CR.MEAN, rtol=RTOL)
    ref = h.realize(3, 0, 5, rtol=RTOL)
    mean = h.mean(rtol=RTOL)
    h.close()
    for r in range(5):
        assert np.array_equal(sol["z"][r], ref[r])
    if mode == "element":                                  # the ensemble's value of a data triangle is the datum
        _, _, _, _, bound = _dense("jitter", mode, False, False)
        err = max(np.max(np.abs(sol["z"][r][tri] - y)) for r in range(5))
        print("element honouring %.3g" % err, "bound %.3g" % bound)
        assert err <= bound
    loop = gss.simulate_with_generic_loop(gss.SimulationProblem(data, mesh, ("z", float), 2),
                                          gss.SPDEGS(("z", p), rng=3, condition=mode, mean=CR.MEAN, rtol=RTOL))
    assert np.array_equal(loop["z"][1], ref[1])
    est = gss.solve(gss.EstimationProblem(data, mesh, "z"),
                    gss.SPDEKriging(("z", p), condition=mode, mean=CR.MEAN, rtol=RTOL))
    assert np.array_equal(np.asarray(est["z"]), mean) and est.domain is mesh
    noisy = gss.solve(gss.EstimationProblem(data, mesh, "z"),
                      gss.SPDEKriging(("z", p), condition=mode, mean=CR.MEAN, error_variance={"z": 0.5}))
    assert np.max(np.abs(np.asarray(noisy["z"]) - mean)) > 1e-3
    with pytest.raises(ValueError, match="lies outside the mesh"):
        gss.solve(gss.EstimationProblem(gss.georef({"z": [1.0]}, [(-4.0, 0.0)]), mesh, "z"), gss.SPDEKriging(("z", p)))
    with pytest.raises(RuntimeError, match="did not reach"):
        gss.solve(gss.SimulationProblem(data, mesh, ("z", float), 2),
                  gss.SPDEGS(("z", p), rng=3, condition=mode, maxiter=2))
