"""How far the FP64 oracle is from the 50-digit covariances of tests/cov_probe.py, per model class and route: the figures
the error bars of tests/test_gpu_cov_probe.py are derived from (cov_probe.bar: 16 x the figure, floored at 8 units).
CPU only.

Routes: A oracle.variogram.cov_pairwise(origin, points); B oracle.kriging.exactsolve and C oracle.kriging.approxsolve
with one neighbour (F: the same for cov_probe.F_MODELS without the regularised Gaussian nugget), both simple kriging of one sample z = 1 at the origin under known mean 0 ("cov": the mean, which is
C / C(0); "var": C(0) - C^2 / C(0)).  Every model of the class, dimensions 1 .. 3, the isotropic range and (BALL_MODELS)
the ball of unequal radii, with and without a nugget; no lag is left out (the general orders' lags below the ladder
are kept as a class of their own, cov_probe.TINY).  Units of 2^-53 sill.

For the Bessel and general-order classes also the float64 transcription of the device's own algorithm: Temme's series
and Steed's continued fraction (tools/gen_matern_general.py) and the Chebyshev expansions of K0 / x K1 (below), with the
tables read from csrc/gss_internal.h, evaluated at the argument the device forms (cov_probe.shape_arg).

    python tools/cov_probe_oracle.py        # prints ORACLE = {...} for tests/cov_probe.py
"""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cov_probe as cp  # noqa: E402
import gen_matern_general as gmg  # noqa: E402

HEADER = os.path.join(ROOT, "geostatssolvers.jl_amd", "csrc", "gss_internal.h")


def header_table(name):
    """The doubles of `static __device__ const double NAME[n] = {...};` in gss_internal.h."""
    with open(HEADER) as f:
        text = f.read()
    body = re.search(r"const double %s\[\d+\] = \{(.*?)\};" % re.escape(name), text, re.S).group(1)
    return [float(v) for v in body.replace("\n", " ").split(",") if v.strip()]


def clenshaw(c, u):
    b1 = b2 = 0.0
    for j in range(len(c) - 1, 0, -1):
        b1, b2 = 2.0 * u * b1 + (c[j] - b2), b1
    return u * b1 + (c[0] - b2)


_TAB = {}


def _tab(name):
    if name not in _TAB:
        _TAB[name] = header_table(name)
    return _TAB[name]


def bessel_k0_xk1(x):
    """float64 transcription of gss_bessel_k0_xk1: (K0(x), x K1(x))."""
    if x <= 2.0:
        y = 0.25 * x * x
        s0 = t0 = s1 = t1 = 1.0
        for k in range(1, 16):
            t0 = t0 * y * (1.0 / (k * k))
            s0 += t0
            t1 = t1 * y * (1.0 / (k * (k + 1)))
            s1 += t1
        lg = math.log(0.5 * x)
        u = 0.5 * x * x - 1.0
        return clenshaw(_tab("GSS_BK_P0"), u) - lg * s0, (x * lg) * (0.5 * x * s1) + clenshaw(_tab("GSS_BK_P1"), u)
    u = 4.0 / x - 1.0
    e = math.exp(-x) / math.sqrt(x)
    return e * clenshaw(_tab("GSS_BK_Q0"), u), x * (e * clenshaw(_tab("GSS_BK_Q1"), u))


def transcription(m, d):
    """The correlation as vg_shape computes it for a Bessel or general-order Matern model at argument d > 0."""
    if d > 700.0:
        return 0.0
    if m.cls == "bessel":
        k0, dk1 = bessel_k0_xk1(d)
        if m.nu == 1.0:
            return dk1
        d2k2 = d * d * k0 + 2.0 * dk1
        if m.nu == 2.0:
            return 0.5 * d2k2
        return 0.125 * (d * d * dk1 + 4.0 * d2k2)
    if m.nu * math.log(2.0 / d) + ((m.nu - 0.5) * math.log(m.nu) - m.nu + 1.01) > 690.0:
        return 1.0 - d * d / (4.0 * (m.nu - 1.0))
    return gmg.matern_general(d, m.nu, _tab("GSS_TEMME_G1"), _tab("GSS_TEMME_G2"))


def configurations(m):
    """(dim, ball, nugget) of every run of a model."""
    for dim in (1, 2, 3):
        for ball in ((False, True) if (dim > 1 and m.name in cp.BALL_MODELS) else (False,)):
            for nugget in cp.NUGGETS:
                yield dim, ball, nugget


def units(got, ref, sill=cp.SILL):
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float("inf") if not np.all(np.isfinite(d)) else float(d.max() / (2.0 ** -53 * sill))


def oracle_run(m, dim, ball, nugget, route):
    """(cov or mean, var or None) of the FP64 oracle over cp.points(m, dim, ball).  Route F is route C with the model as
    the cokriging handle evaluates it: the shape alone, no regularised Gaussian nugget."""
    from oracle import kriging as K
    from oracle.variogram import cov_pairwise, gamma_h
    vg = cp.oracle_model(m, dim, ball, nugget, raw=route == "F")
    pts, o = cp.points(m, dim, ball), cp.origin(dim)
    if m.kind == "power":           # no sill: the pseudo-covariance A - gamma(h) of gss.h, A at a zero lag
        h = np.sqrt(np.sum(pts * pts, axis=1))
        return cp.power_sill(m, dim) - gamma_h(vg, h), None
    if route == "A":
        return cov_pairwise(vg, o, pts)[0], None
    if route == "B":
        return K.exactsolve(K.SK, vg, o, np.ones(1), pts, mean=0.0)
    mu, var, st = K.approxsolve(K.SK, vg, o, np.ones(1), pts, 1, mean=0.0)
    assert not np.any(st)
    return mu, var


def routes_of(m):
    if m.kind == "power":
        return ("A",)               # simple kriging needs a sill
    return cp.ROUTES + (("F",) if m.name in cp.F_MODELS else ())


def measure(classes=cp.CLASSES):
    """bar class (cov_probe.bar_classes) -> {"A": {"cov": e}, "B": {"cov": e, "var": e}, "C": ..., ["F": ...,]
    ["transcription": e,] "cases": lags compared per route}"""
    out = {}
    for cls in classes:
        for m in cp.by_class(cls):
            for dim, ball, nugget in configurations(m):
                sill = cp.sill_of(m, dim)
                tiny = cp.tiny(m, dim, ball)
                for bc, mask in zip(cp.bar_classes(cls), (~tiny, tiny)):
                    if not mask.any():
                        continue
                    res = out.setdefault(bc, {"cases": 0})
                    res["cases"] += int(mask.sum())
                    for r in routes_of(m):
                        cov, mean, var = cp.reference_set(m, dim, ball, nugget, raw=r == "F")
                        got, gvar = oracle_run(m, dim, ball, nugget, r)
                        e = res.setdefault(r, {"cov": 0.0} if gvar is None else {"cov": 0.0, "var": 0.0})
                        e["cov"] = max(e["cov"], units(got[mask], (cov if r == "A" else mean)[mask], sill))
                        if gvar is not None:
                            e["var"] = max(e["var"], units(gvar[mask], var[mask], sill))
                    if cls in ("bessel", "general", "high") and nugget == 0.0:
                        cov = cp.reference_set(m, dim, ball, nugget)[0]
                        d = cp.shape_arg(m, dim, ball, cp.points(m, dim, ball))
                        got = np.array([cp.SILL if v == 0.0 else cp.SILL * transcription(m, float(v)) for v in d])
                        res["transcription"] = max(res.get("transcription", 0.0), units(got[mask], cov[mask]))
    return out


def rounded(res):
    def r(v):
        return {k: r(x) for k, x in v.items()} if isinstance(v, dict) else (v if isinstance(v, int) else round(v, 2))
    return r(res)


def main():
    print("ORACLE = {")
    for cls, v in rounded(measure()).items():
        print(f"    {cls!r}: {v},")
    print("}")


if __name__ == "__main__":
    main()
