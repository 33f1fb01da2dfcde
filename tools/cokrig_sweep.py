#!/usr/bin/env python3
"""Timing of gss_cokrig_predict_global on device arrays beside what the library offered before it.

  1 000 primary + 4 000 secondary 3-D samples (heterotopic, uniform in a cube), nz = 2, spherical structure, ordinary
  cokriging -> 10^6 domain points.  Per call: the total, and the split into right-hand-side assembly ("cokrig_rhs") and
  the nz quadratic forms ("krig_quadform") from gss_profile_read.

  Baseline, on the same stacked coordinates: nz single-variable gss_krig_predict_global calls on one ordinary-kriging
  handle over all 5 000 locations.  Each call evaluates the structure at every (sample, point) pair again
  ("krig_rhs") and runs one quadratic form of the same order, so it is what "one rho evaluation for all targets" is
  compared against; it does not compute a cokriging estimate.  The two alternate.

Method: warm-up, then `--reps` timed runs bracketed by events on the stream; the median is reported.  One JSON line on
stdout.  python tools/cokrig_sweep.py [--reps 3] [--points 1000000]

--local: the moving neighbourhood on the same inputs, gss_cokrig_predict_knn with 16 neighbours per variable, split into
  the per-variable searches ("knn") and the system kernel ("cokrig_local"); beside it, in the same session, the global
  call, and single-variable ordinary gss_krig_predict_knn with k = 32 over the same 5 000 locations and points, split
  into its one search ("knn") and K5 ("krig_local").  The three alternate.  Written to
  profiles/cokrig_local_sweep.json as well.

--cv: cross-validation under the moving neighbourhood on the same samples (no domain), gss_cokrig_cv_knn with 16
  neighbours per variable on device arrays: leave-one-out (every location is its own fold) and 10 folds of locations,
  split into the fold searches ("knn") and the one-target kernel ("cokrig_cv").  Beside them, in the same session on the
  same samples and k, gss_cokrig_predict_knn at the 5 000 sample locations, split into its plain searches ("knn") and
  "cokrig_local".  The three alternate; the splits are means over `--split-reps` profiled calls.  Per-query kernel times
  in microseconds.  Written to profiles/cokrig_cv_sweep.json as well."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gss import _lib  # noqa: E402
from gss.engine import OK, HipEngine, KrigHandle  # noqa: E402
import gss  # noqa: E402


def timed(fn, reps, warm=1):
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
    return statistics.median(ms)


def split(fn, names, reps=1):
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {k: (round(_lib.profile_read(k)[0] / reps, 4 if reps > 1 else 3), _lib.profile_read(k)[1] // reps)
           for k in names}
    _lib.profile_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--primary", type=int, default=1000)
    ap.add_argument("--secondary", type=int, default=4000)
    ap.add_argument("--local", action="store_true", help="the moving neighbourhood beside the global call and K5")
    ap.add_argument("--cv", action="store_true", help="cross-validation beside the moving neighbourhood at the samples")
    ap.add_argument("--split-reps", type=int, default=20, help="--cv: profiled calls behind every split")
    ap.add_argument("--neighbors", type=int, default=16, help="--local, --cv: neighbours per variable")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    _lib.lib()
    rng = np.random.default_rng(1)
    n = args.primary + args.secondary
    x = rng.uniform(0.0, 1000.0, (n, 3))
    var = np.repeat([0, 1], [args.primary, args.secondary]).astype(np.int32)
    z = rng.normal(size=n)
    B1 = np.array([[0.9, 0.5], [0.5, 0.8]])
    B0 = np.array([[0.1, 0.02], [0.02, 0.2]])
    g = gss.SphericalVariogram(range=120.0)
    if args.cv:
        return cv(args, g, B0, B1, x, z, var)
    xdom = torch.as_tensor(rng.uniform(0.0, 1000.0, (args.points, 3)), device="cuda")

    if args.local:
        return local(args, g, B0, B1, x, z, var, xdom)
    co = HipEngine.cokrig(g, B0, B1, OK, x, z, var)
    single = KrigHandle(gss.SphericalVariogram(range=120.0, sill=1.0, nugget=0.1), OK, x, z)

    def cokrig():
        co.predict_global(xdom)

    def separate():
        for _ in range(2):
            single.predict_global(xdom)
    tc, ts = [], []
    for _ in range(2):                                      # alternating blocks
        tc.append(timed(cokrig, args.reps))
        ts.append(timed(separate, args.reps))
    c, s = statistics.median(tc), statistics.median(ts)
    cs = split(cokrig, ("cokrig_rhs", "krig_quadform"))
    ss = split(separate, ("krig_rhs", "krig_quadform"))
    co.close()
    single.close()
    print(json.dumps({"what": "cokrig_predict_global", "primary": args.primary, "secondary": args.secondary, "nz": 2,
                      "points": args.points, "cokrig_ms": round(c, 2), "cokrig_rhs_ms": cs["cokrig_rhs"][0],
                      "cokrig_chunks": cs["cokrig_rhs"][1], "cokrig_quadform_ms": cs["krig_quadform"][0],
                      "separate_calls_ms": round(s, 2), "separate_rhs_ms": ss["krig_rhs"][0],
                      "separate_quadform_ms": ss["krig_quadform"][0],
                      "rhs_separate_over_cokrig": round(ss["krig_rhs"][0] / cs["cokrig_rhs"][0], 3),
                      "total_separate_over_cokrig": round(s / c, 3),
                      "points_per_s": round(args.points / (c * 1e-3), 1)}), flush=True)


def local(args, g, B0, B1, x, z, var, xdom):
    k = args.neighbors
    co = HipEngine.cokrig(g, B0, B1, OK, x, z, var)                      # with the factor: serves both calls
    single = KrigHandle(gss.SphericalVariogram(range=120.0, sill=1.0, nugget=0.1), OK, x, z, factor=False)

    def co_local():
        co.predict_knn(xdom, k)

    def co_global():
        co.predict_global(xdom)

    def k5():
        single.predict_knn(xdom, 2 * k)
    tl, tg, tk = [], [], []
    for _ in range(2):                                      # alternating blocks
        tl.append(timed(co_local, args.reps))
        tg.append(timed(co_global, args.reps))
        tk.append(timed(k5, args.reps))
    l, gl, kk = statistics.median(tl), statistics.median(tg), statistics.median(tk)
    ls = split(co_local, ("knn", "cokrig_local"))
    ks = split(k5, ("knn", "krig_local"))
    co.close()
    single.close()
    res = {"what": "cokrig_predict_knn", "primary": args.primary, "secondary": args.secondary, "nz": 2,
           "points": args.points, "neighbors_per_variable": k, "local_ms": round(l, 3),
           "local_search_ms": ls["knn"][0], "local_kernel_ms": ls["cokrig_local"][0], "global_ms": round(gl, 2),
           "global_over_local": round(gl / l, 1), "krig_knn_k": 2 * k, "krig_knn_ms": round(kk, 3),
           "krig_knn_search_ms": ks["knn"][0], "krig_knn_kernel_ms": ks["krig_local"][0],
           "kernel_cokrig_over_krig": round(ls["cokrig_local"][0] / ks["krig_local"][0], 3),
           "search_cokrig_over_krig": round(ls["knn"][0] / ks["knn"][0], 3),
           "points_per_s": round(args.points / (l * 1e-3), 1)}
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "cokrig_local_sweep.json"), "w") as f:
        f.write(line + "\n")


def cv(args, g, B0, B1, x, z, var):
    k, n = (args.neighbors, args.neighbors), x.shape[0]
    h = HipEngine.cokrig(g, B0, B1, OK, x, z, var, factor=False)
    xs = torch.as_tensor(x, device="cuda")
    # the samples are scattered: every location holds one of them, so folds of locations are folds of samples
    assert np.unique(x, axis=0).shape[0] == n
    fold10 = torch.as_tensor(np.random.default_rng(2).integers(0, 10, n).astype(np.int32), device="cuda")

    def loo():
        h.cv_knn(k, device=True)

    def folds():
        h.cv_knn(k, fold=fold10)

    def at_samples():
        h.predict_knn(xs, k)
    tl, tf, tp = [], [], []
    for _ in range(3):                                      # alternating blocks
        tl.append(timed(loo, args.reps, warm=2))
        tf.append(timed(folds, args.reps, warm=2))
        tp.append(timed(at_samples, args.reps, warm=2))
    ls = split(loo, ("knn", "cokrig_cv"), args.split_reps)
    fs = split(folds, ("knn", "cokrig_cv"), args.split_reps)
    ps = split(at_samples, ("knn", "cokrig_local"), args.split_reps)
    h.close()
    us = lambda ms: round(1e3 * ms / n, 4)                      # noqa: E731
    res = {"what": "cokrig_cv_knn", "primary": args.primary, "secondary": args.secondary, "nz": 2, "queries": n,
           "neighbors_per_variable": args.neighbors, "reps": args.reps, "split_reps": args.split_reps,
           "loo_ms": round(statistics.median(tl), 3), "folds10_ms": round(statistics.median(tf), 3),
           "predict_at_samples_ms": round(statistics.median(tp), 3),
           "loo_search_ms": ls["knn"][0], "loo_kernel_ms": ls["cokrig_cv"][0],
           "folds10_search_ms": fs["knn"][0], "folds10_kernel_ms": fs["cokrig_cv"][0],
           "plain_search_ms": ps["knn"][0], "local_kernel_ms": ps["cokrig_local"][0],
           "cv_kernel_us_per_query": us(ls["cokrig_cv"][0]), "cv_kernel_folds10_us_per_query": us(fs["cokrig_cv"][0]),
           "local_kernel_us_per_point": us(ps["cokrig_local"][0]),
           "kernel_cv_over_local": round(ls["cokrig_cv"][0] / ps["cokrig_local"][0], 3),
           "search_loo_over_plain": round(ls["knn"][0] / ps["knn"][0], 3),
           "search_folds10_over_plain": round(fs["knn"][0] / ps["knn"][0], 3)}
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "cokrig_cv_sweep.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
