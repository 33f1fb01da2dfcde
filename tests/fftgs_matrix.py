"""The reference of tests/test_gpu_fftgs_matrix.py: fft.jl:96-103 (the spectral amplitude) and fft.jl:163-170 (one
realisation) restated in numpy.longdouble with scipy.fft, whose pocketfft keeps long double -- 80-bit where this suite
runs (eps 1.08e-19), some 2000 times finer than the FP64 of the device and of oracle/fftgs.py.

    lag   = (cell - centre cell) * spacing                      (the centroids' difference; rotated: R^T lag, as
                                                                 tests/rotated_frame.py, then / radii)
    C     = sill - gamma(|lag|)
    F     = sqrt|fftn(fftshift C)|, F[0] = 0
    z     = real(ifftn(F X / |X|)),  X = fftn(uniforms);  z *= sqrt(sill / (sum z^2 / (N - 1)));  z += mean

The uniforms are the very doubles the device receives: oracle.philox.uniform (which the device's generator equals bit
for bit, tests/test_gpu_fftgs.py) for a seeded realisation, the caller's array for supplied noise.  A co-simulation is
built term by term from the unit fields of the same restatement (sill 1, no nugget), the factors of
tests/fftgs_lmc_ref.py (the library's own rule, one IEEE operation at a time) and the normals the device uses: the
caller's, or those of gss_philox_normal with the documented stream numbers.

device_run and oracle_run do one run of tests/fftgs_cases.py on the device and on oracle/fftgs.py; errors() measures
either against reference().  Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fftgs_lmc_ref as LR

LD = np.longdouble
SEED, REAL = 20261, 3                 # the seeded realisation of every run (a co-simulation: realisation REAL of SEED)
SCOPES = {"fused": "fftgs_p1", "generic": "fftgs_generic", "rocfft": "fftgs_fwd"}   # a ProfScope only that pipeline opens


def long_double_ok():
    """The guard of the matrix: long double must be finer than 1e-18 (x87 80-bit: 1.08e-19)."""
    return np.finfo(LD).eps < 1e-18


def noise_of(run):
    """The supplied uniforms (and, for a co-simulation, normals) of a run: (uniforms, normals or None), one realisation."""
    N = int(np.prod(run.dims))
    rng = np.random.default_rng(N + 7 * run.nz)
    if run.nz == 0:
        return rng.uniform(size=(1, N)), None
    return rng.uniform(size=(1, run.nz, N)), rng.normal(size=(1, run.nz, N))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def covariance(run, sill, nugget):
    """C to the centre cell, shape dims[::-1], long double."""
    dims = run.dims
    d = len(dims)
    sp = run.spacing if run.spacing is not None else (1.0,) * d
    # fft.jl:69: the centre cell is CartesianIndex(dims .÷ 2), 1-based; centroid differences are (i - c) * spacing
    axes = [(np.arange(n, dtype=LD) - LD(n // 2 - 1)) * LD(s) for n, s in zip(dims, sp)]
    u = np.meshgrid(*axes[::-1], indexing="ij")[::-1]        # u[k]: lag along axis k, arrays of shape dims[::-1]
    if run.rotated:
        R = np.asarray(run.rotation, dtype=np.float64).astype(LD)
        u = [sum(R[i, k] * u[i] for i in range(d)) for k in range(d)]          # x' = R^T lag
        r = [LD(v) for v in run.model["radii"]]
    else:
        r = [LD(run.model["range"])] * d
    x = np.sqrt(sum((u[k] / r[k]) ** 2 for k in range(d)))
    if run.kind == "exponential":
        rho = np.exp(-3 * x)
    elif run.kind == "spherical":
        rho = np.where(x < 1, 1 - (LD(3) / 2) * x + x ** 3 / 2, LD(0))
    else:
        raise ValueError(run.kind)
    return (LD(sill) - LD(nugget)) * rho + LD(nugget) * (x == 0)


def amplitude(C):
    from scipy import fft as sfft
    F = np.sqrt(np.abs(sfft.fftn(sfft.fftshift(C))))
    assert F.dtype == LD, F.dtype                   # scipy's pocketfft kept the precision
    F.flat[0] = 0
    return F


def field(F, uniforms, sill, mean):
    """fft.jl:163-170 from one array of uniforms (flat, element order): N long doubles."""
    from scipy import fft as sfft
    N = F.size
    X = sfft.fftn(np.asarray(uniforms, dtype=np.float64).astype(LD).reshape(F.shape))
    mag = np.abs(X)
    phase = np.where(mag > 0, X / np.where(mag > 0, mag, 1), 1)              # angle(0) = 0
    z = np.real(sfft.ifftn(F * phase))
    s2 = np.sum(z * z) / (N - 1)
    return (np.sqrt(LD(sill) / s2) * z + LD(mean)).ravel()


def _mix(run, Y, E):
    """Z_a = means[a] + sum_j L1[a][j] Y_j + sum_j L0[a][j] E_j in long double; Y, E: (nz, N)."""
    import fftgs_cases as FC
    L0, live0 = LR.factor(FC.lmc_b0(run.nz), "b0")
    L1, live1 = LR.factor(FC.lmc_b1(run.nz), "b1")
    assert len(live0) == len(live1) == run.nz          # the runs' matrices have full rank
    means = FC.lmc_means(run.nz)
    out = np.empty((run.nz, Y.shape[1]), dtype=LD)
    for a in range(run.nz):
        z = np.full(Y.shape[1], LD(means[a]))
        for j in range(run.nz):
            z = z + LD(L1[a, j]) * Y[j].astype(LD) + LD(L0[a, j]) * E[j].astype(LD)
        out[a] = z
    return out


def _fields(run, F, sill, mean, make_field, normals):
    """{"z_seeded": ..., "z_noise": ...} of a run, from F and a function (F, uniforms, sill, mean) -> field; `normals`
    (seeded, supplied) for a co-simulation."""
    from oracle import philox
    N = int(np.prod(run.dims))
    u, _ = noise_of(run)
    if run.nz == 0:
        return {"z_seeded": make_field(F, philox.uniform(SEED, REAL, N), sill, mean)[None],
                "z_noise": make_field(F, u[0], sill, mean)[None]}
    nz = run.nz
    Ys = np.stack([make_field(F, philox.uniform(SEED, REAL * nz + j, N), 1.0, 0.0) for j in range(nz)])
    Yn = np.stack([make_field(F, u[0, j], 1.0, 0.0) for j in range(nz)])
    return {"z_seeded": _mix(run, Ys, normals[0])[None], "z_noise": _mix(run, Yn, normals[1])[None]}


def _model_scalars(run):
    """(sill, nugget, mean) of the handle's spectrum: a co-simulation realises the unit structure."""
    import fftgs_cases as FC
    return (1.0, 0.0, 0.0) if run.nz else (FC.SILL, FC.NUGGET, FC.MEAN)


def oracle_normals(run):
    """(seeded, supplied) normals of a co-simulation as the oracle numbers them: E_j of realisation r is stream r nz + j of
    seed ^ salt."""
    from oracle import philox
    if run.nz == 0:
        return None
    N = int(np.prod(run.dims))
    seeded = np.stack([philox.normal(SEED ^ LR.NUGGET_SALT, REAL * run.nz + j, N) for j in range(run.nz)])
    return seeded, noise_of(run)[1][0]


def reference(run, normals=None):
    """{"F": N long doubles, "z_seeded": (1, [nz,] N), "z_noise": (1, [nz,] N)}."""
    sill, nugget, mean = _model_scalars(run)
    F = amplitude(covariance(run, sill, nugget))
    out = {"F": F.ravel()}
    out.update(_fields(run, F, sill, mean, field, normals))
    return out


# ---- the FP64 oracle ---------------------------------------------------------------------------------------------------
def oracle_run(run, normals=None):
    """The same quantities from oracle/fftgs.py (rotated: its covariance on the frame of tests/rotated_frame.py)."""
    from oracle import fftgs as O
    from oracle.variogram import Variogram, cov_pairwise
    from rotated_frame import frame
    sill, nugget, mean = _model_scalars(run)
    kw = dict(run.model, sill=sill, nugget=nugget)
    vg = Variogram(run.kind, **kw)
    if run.rotated:
        cent = O.grid_centroids(run.dims, spacing=run.spacing)
        ci = np.ravel_multi_index(tuple(n // 2 - 1 for n in run.dims)[::-1], run.dims[::-1])
        fc = frame(cent, run.rotation)
        C = cov_pairwise(vg, fc[ci:ci + 1], fc)[0].reshape(run.dims[::-1])
        F = np.sqrt(np.abs(np.fft.fftn(np.fft.fftshift(C))))
        F.flat[0] = 0.0
        pre = O.FFTGSPreproc(vg, float(mean), tuple(run.dims), F)
    else:
        pre = O.preprocess(vg, run.dims, spacing=run.spacing, mean=mean)

    def make_field(F, uniforms, s, m):
        return O.solvesingle(O.FFTGSPreproc(Variogram(run.kind, **dict(kw, sill=s)), float(m), tuple(run.dims), F), uniforms)

    out = {"F": pre.F.ravel()}
    if run.nz == 0:
        out.update(_fields(run, pre.F, sill, mean, make_field, None))
        return out
    # a co-simulation: the FP64 mixture of tests/fftgs_lmc_ref.py over the oracle's unit fields
    import fftgs_cases as FC
    from oracle import philox
    N, nz = int(np.prod(run.dims)), run.nz
    L0, live0 = LR.factor(FC.lmc_b0(nz), "b0")
    L1, live1 = LR.factor(FC.lmc_b1(nz), "b1")
    u, _ = noise_of(run)
    for name, unis, E in (("z_seeded", [philox.uniform(SEED, REAL * nz + j, N) for j in range(nz)], normals[0]),
                          ("z_noise", list(u[0]), normals[1])):
        Y = {j: make_field(pre.F, unis[j], 1.0, 0.0) for j in live1}
        out[name] = LR.mix(L0, live0, L1, live1, FC.lmc_means(nz), Y, {j: E[j] for j in live0})[0][None]
    return out


# ---- the device --------------------------------------------------------------------------------------------------------
def _variogram(run):
    import gss
    ctor = dict(exponential=gss.ExponentialVariogram, spherical=gss.SphericalVariogram)[run.kind]
    kw = dict(run.model)
    radii = kw.pop("radii", None)
    if radii is not None:
        return ctor(gss.MetricBall(tuple(radii), run.rotation), **kw)
    return ctor(**kw)


def device_normals(run):
    """(seeded, supplied) normals of a co-simulation: the seeded ones through the export the header names for them."""
    from gss import _lib
    if run.nz == 0:
        return None
    N = int(np.prod(run.dims))
    seeded = np.empty((run.nz, N))
    for j in range(run.nz):
        _lib.check(_lib.lib().gss_philox_normal(SEED ^ LR.NUGGET_SALT, REAL * run.nz + j, N, _lib.ptr(seeded[j]), 0, None))
    return seeded, noise_of(run)[1][0]


def device_run(run):
    """One run on the device (GSS_FFTGS_PATH is the caller's to set): the quantities of reference() and "scopes", how
    often each pipeline's profile scope was opened by the two realisation calls."""
    import fftgs_cases as FC
    from gss import _lib
    from gss.engine import FFTGSHandle
    u, e = noise_of(run)
    if run.nz:
        h = FFTGSHandle.lmc(_variogram(run), FC.lmc_b0(run.nz), FC.lmc_b1(run.nz), FC.lmc_means(run.nz), run.dims,
                            run.spacing)
    else:
        h = FFTGSHandle(_variogram(run), run.dims, run.spacing, FC.MEAN)
    out = {"F": h.spectrum()}
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        if run.nz:
            out["z_seeded"] = h.realize_lmc(SEED, REAL, 1)
            out["z_noise"] = h.realize_lmc(0, 0, 1, noise=u, nugget_noise=e)
        else:
            out["z_seeded"] = h.realize(SEED, REAL, 1)
            out["z_noise"] = h.realize(0, 0, 1, noise=u)
    finally:
        _lib.profile_enable(False)
    out["scopes"] = {p: _lib.profile_read(s)[1] for p, s in SCOPES.items()}
    h.close()
    return out


# ---- errors ------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """{"F": (error relative to max F, flat index of the worst frequency), "z": (absolute error, (which, flat index))}."""
    dF = np.abs(got["F"].astype(LD) - ref["F"])
    eF = (float(dF.max() / ref["F"].max()), int(dF.argmax()))
    ez = (0.0, None)
    for name in ("z_seeded", "z_noise"):
        assert got[name].shape == ref[name].shape, (name, got[name].shape, ref[name].shape)
        dz = np.abs(got[name].astype(LD) - ref[name])
        if float(dz.max()) >= ez[0]:
            ez = (float(dz.max()), (name, int(dz.argmax())))
    return {"F": eF, "z": ez}
