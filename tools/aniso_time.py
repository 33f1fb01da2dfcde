"""Rotated against axis-aligned anisotropy, same radii, timed alternately in one process (the
frame transform is one pass over n d doubles per call; the hot kernels are the axis-aligned ones).

  python tools/aniso_time.py [--reps 5] [--out profiles/aniso_time.json]

Cases: configs[1] (OK, 1000 3-D data -> 10^6 points, global, device arrays) and configs[4] (UK degree 1, 5000 3-D
data, k = 64, 10^7 points, device arrays) and FFTGS 512^3 (preprocess, whose covariance grid is evaluated at rotated
lags, and 64 realisations, which do not depend on the rotation)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "geostatssolvers.jl_amd"))

import torch  # noqa: E402

import gss  # noqa: E402
from gss.engine import OK, UK, FFTGSHandle, KrigHandle  # noqa: E402

_a, _b = np.radians(30.0), np.radians(20.0)       # 30 degrees from north, dipping 20 degrees
R3 = np.array([[np.cos(_a), -np.sin(_a), 0.0], [np.sin(_a), np.cos(_a), 0.0], [0.0, 0.0, 1.0]]) @ \
    np.array([[1.0, 0.0, 0.0], [0.0, np.cos(_b), -np.sin(_b)], [0.0, np.sin(_b), np.cos(_b)]])
RADII = (40.0, 20.0, 10.0)


def sync():
    torch.cuda.synchronize()


def timed(fn, reps):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts


def alternate(fa, fr, reps):
    """Median milliseconds of fa (axis-aligned) and fr (rotated), interleaved rep by rep."""
    ta, tr = [], []
    fa(); fr(); sync()
    for _ in range(reps):
        ta += timed(fa, 1)
        tr += timed(fr, 1)
    return round(float(np.median(ta)) * 1e3, 3), round(float(np.median(tr)) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aniso_time.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "rotation": R3.tolist(), "radii": RADII, "cases": []}

    n, m = 1000, (100_000 if a.quick else 1_000_000)
    x = np.random.default_rng(2).uniform(0.0, 100.0, (n, 3))
    z = np.random.default_rng(1002).normal(size=n)
    x0 = torch.as_tensor(np.random.default_rng(3).uniform(0.0, 100.0, (m, 3)), device="cuda")
    ha = KrigHandle(gss.MaternVariogram(gss.MetricBall(RADII), order=1.5), OK, x, z)
    hr = KrigHandle(gss.MaternVariogram(gss.MetricBall(RADII, R3), order=1.5), OK, x, z)
    ta, tr = alternate(lambda: ha.predict_global(x0), lambda: hr.predict_global(x0), a.reps)
    out["cases"].append({"case": "configs[1] OK global, 1000 3-D data -> %d points, device arrays" % m,
                         "axis_aligned_ms": ta, "rotated_ms": tr, "ratio": round(tr / ta, 4)})
    ha.close(); hr.close()

    n, m = 5000, (1_000_000 if a.quick else 10_000_000)
    x = np.random.default_rng(6).uniform(0, 100, (n, 3))
    z = 1.0 + 0.03 * x[:, 0] + np.random.default_rng(60).normal(size=n)
    x0 = torch.rand((m, 3), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(7)) * 100
    ha = KrigHandle(gss.MaternVariogram(gss.MetricBall(RADII), order=1.5), UK, x, z, degree=1, factor=False)
    hr = KrigHandle(gss.MaternVariogram(gss.MetricBall(RADII, R3), order=1.5), UK, x, z, degree=1, factor=False)
    ta, tr = alternate(lambda: ha.predict_knn(x0, 64), lambda: hr.predict_knn(x0, 64), max(2, a.reps // 2))
    out["cases"].append({"case": "configs[4] UK degree 1, 5000 3-D data, k=64 (covariance-frame search), %d points, "
                                 "device arrays" % m, "axis_aligned_ms": ta, "rotated_ms": tr, "ratio": round(tr / ta, 4)})
    ha.close(); hr.close()
    del x0

    e = 256 if a.quick else 512
    nr = 64
    vga = gss.ExponentialVariogram(gss.MetricBall(tuple(r * e / 512 for r in RADII)))
    vgr = gss.ExponentialVariogram(gss.MetricBall(tuple(r * e / 512 for r in RADII), R3))
    pre = {"a": [], "r": []}
    real = {"a": [], "r": []}
    zbuf = torch.empty((1, e ** 3), dtype=torch.float64, device="cuda")
    FFTGSHandle(vga, (e, e, e)).close(); FFTGSHandle(vgr, (e, e, e)).close(); sync()   # first calls of the process
    for _ in range(max(2, a.reps // 2)):
        for key, vg in (("a", vga), ("r", vgr)):
            t0 = time.perf_counter()
            f = FFTGSHandle(vg, (e, e, e))
            sync()
            pre[key].append(time.perf_counter() - t0)
            f.realize(4, 0, 1, out=zbuf); sync()
            t0 = time.perf_counter()
            for r in range(nr):
                f.realize(4, r, 1, out=zbuf)
            sync()
            real[key].append(time.perf_counter() - t0)
            f.close()
    med = lambda v: round(float(np.median(v)) * 1e3, 3)   # noqa: E731
    out_case = {"case": "FFTGS %d^3 exponential: preprocess, and %d realisations (device output)" % (e, nr),
                "axis_aligned_preprocess_ms": med(pre["a"]), "rotated_preprocess_ms": med(pre["r"]),
                "preprocess_ratio": round(med(pre["r"]) / med(pre["a"]), 4),
                "axis_aligned_realisations_ms": med(real["a"]), "rotated_realisations_ms": med(real["r"]),
                "realisations_ratio": round(med(real["r"]) / med(real["a"]), 4)}
    out["cases"].append(out_case)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
