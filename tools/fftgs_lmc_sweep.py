#!/usr/bin/env python3
"""Timing of gss_fftgs_realize_lmc into device memory (the in-place route) beside what it is made of.

  Grid n^3 (default 512), exponential structure.  Rows:
    joint_nz2        nz = 2, full-rank b1, b0 != 0: ms per joint realisation, and of that the mix ("fftgs_lmc_mix")
    joint_rank1_nz3  nz = 3, rank-1 b1 (one live field), b0 != 0: the same
    plain_x2         two realisations of gss_fftgs_realize on a plain handle of the same structure
    copy_4N          a device-to-device copy of 8 N 4 bytes: 8 N 2 read and 8 N 2 written, the traffic of the nz = 2 mix
                     (two live fields in, two variables out), as the achievable rate
  Expectation: joint_nz2 ~ plain_x2 + mix, and the mix within a small factor of the copy.  The mix draws its nz normals
  per cell from Philox in the kernel (one Philox block, a logarithm, a square root and a cosine each), which the copy does
  not do.

Method: the rows alternate; per row `--warmup` untimed calls, then `--reps` timed ones bracketed by events on the
stream, median and spread (min .. max) reported; the mix alone is the mean of "fftgs_lmc_mix" over `--reps` profiled
calls (gss_profile_read brackets the launch with events of its own).  One JSON line on stdout, written to
profiles/fftgs_lmc_sweep.json as well.  python tools/fftgs_lmc_sweep.py [--n 512] [--reals 2] [--reps 5]

--conditional: the conditioning of a joint group instead (gss_cokrig_predict_global_batch).  Grid n^3 (default 128), nz = 2,
cu at 500 cells and zn at 2 000 others, `--reals` (default 16) realisations.  Rows, in ms:
    create_data      gss_cokrig_create on the 2 500 stacked samples (simple variant; the fit included)
    create_cells     the same at the centroids of the data cells (the handle every block of realisations makes)
    predict_batch    CoKrigHandle.predict_batch: reals value vectors x nz targets at all n^3 centroids, in HBM; of that
                     the mean kernel alone ("cokrig_batch")
    yardstick        gss_krig_predict_global_batch of ONE variable over the same 2 500 locations with nz x reals value
                     columns: the same arithmetic per column, rho evaluated again for every 16 columns
    solve_cond       gss.solve of the conditioned problem, host arrays out (wall clock of the whole call)
    solve_uncond     the same problem without data
`--tag` labels the line (the column count a variant of the library was built with); the line is also written to
profiles/fftgs_lmc_cond_sweep[_TAG].json."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gss  # noqa: E402
from gss import _lib  # noqa: E402
from gss.engine import FFTGSHandle  # noqa: E402


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def conditional(a):
    import time
    from gss.engine import HipEngine, KrigHandle, SK
    n, R = a.n or 128, a.reals or 16
    grid = gss.CartesianGrid(n, n, n)
    N = n ** 3
    st = gss.ExponentialVariogram(range=n / 16.0)
    b0 = np.array([[0.1, 0.05], [0.05, 0.1]])
    b1 = np.array([[0.9, 0.75], [0.75, 0.9]])
    means = np.array([1.0, -2.0])
    rng = np.random.default_rng(5)
    cells = rng.choice(N, 2500, replace=False)
    cent = grid.centroids()
    x = cent[cells] + rng.uniform(-0.3, 0.3, (2500, 3))           # samples off the centroids, as drill-hole data are
    var = np.repeat([0, 1], [500, 2000]).astype(np.int32)
    z = means[var] + rng.normal(size=2500)
    cdev = torch.as_tensor(cent, device="cuda")
    zdat = torch.as_tensor(rng.normal(size=(R, 2500)) + means[var], device="cuda")
    zcols = torch.as_tensor(rng.normal(size=(2 * R, 2500)), device="cuda")
    mk = lambda pts: HipEngine.cokrig(st, b0, b1, SK, pts, z, var, means=means)      # noqa: E731
    h = mk(cent[cells])
    hk = KrigHandle(st, SK, cent[cells], z, mean=0.0)
    rows = {
        "create_data": lambda: mk(x).close(),
        "create_cells": lambda: mk(cent[cells]).close(),
        "predict_batch": lambda: h.predict_batch(cdev, zdat),
        "yardstick": lambda: hk.predict_global_batch(cdev, zcols),
    }
    times = {k: [] for k in rows}
    for k, fn in rows.items():
        timed(fn, 0, a.warmup)
    for _ in range(a.reps):
        for k, fn in rows.items():
            times[k] += timed(fn, 1, 0)
    res = {"mode": "conditional", "tag": a.tag, "grid": [n] * 3, "nz": 2, "samples": [500, 2000], "reals": R,
           "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for k, ms in times.items():
        res[k] = {"ms_median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(a.reps):
        rows["predict_batch"]()
    torch.cuda.synchronize()
    ms, cnt = _lib.profile_read("cokrig_batch")
    _lib.profile_enable(False)
    res["predict_batch"]["kernel_ms"] = ms / a.reps
    res["predict_batch"]["passes"] = cnt // a.reps
    h.close()
    hk.close()
    if not a.no_solve:
        cu, zn = np.full(2500, np.nan), np.full(2500, np.nan)
        cu[:500], zn[500:] = z[:500], z[500:]
        data = gss.georef(dict(cu=cu, zn=zn), x)
        lmc = SimpleNamespace(names=("cu", "zn"), kind="exponential", range=n / 16.0, order=1.0, B0=b0, B1=b1)
        variables = {"cu": float, "zn": float}
        mksolver = lambda: gss.FFTGS(("cu", dict(mean=means[0])), ("zn", dict(mean=means[1])),      # noqa: E731
                                     (("cu", "zn"), dict(model=lmc)), rng=7)
        for key, prob in (("solve_cond", gss.SimulationProblem(data, grid, variables, R)),
                          ("solve_uncond", gss.SimulationProblem(grid, variables, R))):
            wall = []
            for i in range(1 + max(a.reps // 2, 1)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gss.solve(prob, mksolver())
                torch.cuda.synchronize()
                if i:                                                   # the first call warms the pools
                    wall.append(1e3 * (time.perf_counter() - t0))
            res[key] = {"ms_median": statistics.median(wall), "min": min(wall), "max": max(wall)}
    res["ratios"] = {"yardstick_over_predict_batch": res["yardstick"]["ms_median"] / res["predict_batch"]["ms_median"]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "fftgs_lmc_cond_sweep%s.json" % ("_" + a.tag if a.tag else "")
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reals", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--conditional", action="store_true")
    ap.add_argument("--no-solve", action="store_true", help="--conditional: skip the two whole-solve rows")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.conditional:
        return conditional(a)
    a.n, a.reals = a.n or 512, a.reals or 2
    dims, N, R = (a.n,) * 3, a.n ** 3, a.reals
    st = gss.ExponentialVariogram(range=a.n / 16.0)
    b0 = np.array([[0.1, 0.05], [0.05, 0.1]])
    b1 = np.array([[0.9, 0.75], [0.75, 0.9]])
    v = np.array([1.0, -0.6, 0.8])
    hj = FFTGSHandle.lmc(st, b0, b1, [0.0, 0.0], dims)
    h1 = FFTGSHandle.lmc(st, np.diag([0.1, 0.2, 0.3]), np.outer(v, v), [0.0, 0.0, 0.0], dims)
    hp = FFTGSHandle(st, dims)
    out2 = torch.empty((R, 2, N), dtype=torch.float64, device="cuda")
    out3 = torch.empty((R, 3, N), dtype=torch.float64, device="cuda")
    outp = torch.empty((2 * R, N), dtype=torch.float64, device="cuda")
    src, dst = torch.empty(2 * N, dtype=torch.float64, device="cuda"), torch.empty(2 * N, dtype=torch.float64, device="cuda")
    rows = {
        "joint_nz2": lambda: hj.realize_lmc(1, 0, R, out=out2),
        "joint_rank1_nz3": lambda: h1.realize_lmc(1, 0, R, out=out3),
        "plain_x2": lambda: hp.realize(1, 0, 2 * R, out=outp),
        "copy_4N": lambda: [dst.copy_(src) for _ in range(R)],
    }
    times = {k: [] for k in rows}
    for k, fn in rows.items():                 # warm every row first, then alternate the timed calls
        timed(fn, 0, a.warmup)
    for _ in range(a.reps):
        for k, fn in rows.items():
            times[k] += timed(fn, 1, 0)
    res = {"grid": list(dims), "reals_per_call": R, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    for k, ms in times.items():
        per = [m / R for m in ms]
        res[k] = {"ms_per_realisation_median": statistics.median(per), "min": min(per), "max": max(per)}
    _lib.profile_enable(True)
    for k in ("joint_nz2", "joint_rank1_nz3"):
        _lib.profile_reset()
        for _ in range(a.reps):
            rows[k]()
        torch.cuda.synchronize()
        ms, n = _lib.profile_read("fftgs_lmc_mix")
        res[k]["mix_ms_per_realisation"] = ms / max(n, 1) / R
        res[k]["mix_launches"] = n
    _lib.profile_enable(False)
    j, p, c = (res[k]["ms_per_realisation_median"] for k in ("joint_nz2", "plain_x2", "copy_4N"))
    mix = res["joint_nz2"]["mix_ms_per_realisation"]
    res["ratios"] = {"joint_over_plain_x2_plus_mix": j / (p + mix), "mix_over_copy": mix / c,
                     "copy_GBps": 8.0 * N * 4 / (c * 1e-3) / 1e9, "mix_traffic_GBps": 8.0 * N * 4 / (mix * 1e-3) / 1e9}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fftgs_lmc_sweep.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
