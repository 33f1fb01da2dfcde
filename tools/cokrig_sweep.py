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
stdout.  python tools/cokrig_sweep.py [--reps 3] [--points 1000000]"""
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


def split(fn, names):
    _lib.profile_enable(True)
    _lib.profile_reset()
    fn()
    torch.cuda.synchronize()
    out = {k: (round(_lib.profile_read(k)[0], 3), _lib.profile_read(k)[1]) for k in names}
    _lib.profile_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--primary", type=int, default=1000)
    ap.add_argument("--secondary", type=int, default=4000)
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
    xdom = torch.as_tensor(rng.uniform(0.0, 1000.0, (args.points, 3)), device="cuda")
    g = gss.SphericalVariogram(range=120.0)

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


if __name__ == "__main__":
    main()
