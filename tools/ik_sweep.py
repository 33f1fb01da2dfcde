#!/usr/bin/env python3
"""Timing of gss_ik_predict_knn on device arrays beside the only way to the same answer before it.

  5 000 3-D samples (uniform in a cube, lognormal values), spherical model, ordinary variant -> 1.25 x 10^6 domain
  points; k = 16 and 64 neighbours; K = 4, 8, 12, 16 cutoffs; the median form (one variogram) and the full form (K
  variograms of different ranges).  Per call: the total, and the split into the search ("knn") and the system kernel
  ("ik_local") from gss_profile_read.

  Yardstick, in the same session on the same samples and points: K calls of gss_krig_predict_knn, one per pre-formed
  indicator column (K handles without a factor, created outside the timed region), each with its own search.  The
  calls alternate in blocks.

  gss_ik_post (mean, variance, one threshold, one quantile) on the m x K rows beside a device-to-device copy of the same
  bytes, as the normal-score row does.

Method: warm-up, then `--reps` timed runs bracketed by events on the stream; the median over two alternating blocks is
reported.  One JSON line per (k, K) on stdout and appended to --out (default profiles/ik_sweep.jsonl).
python tools/ik_sweep.py [--reps 3] [--points 1250000]"""
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
    out = {k: round(_lib.profile_read(k)[0], 3) for k in names}
    _lib.profile_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_250_000)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--neighbors", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--cutoffs", type=int, nargs="*", default=[4, 8, 12, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_sweep.jsonl"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    _lib.lib()
    rng = np.random.default_rng(1)
    n, m = args.samples, args.points
    x = rng.uniform(0.0, 1000.0, (n, 3))
    z = np.exp(rng.normal(size=n))
    xd = torch.as_tensor(x, device="cuda")
    zd = torch.as_tensor(z, device="cuda")
    xdom = torch.as_tensor(rng.uniform(0.0, 1000.0, (m, 3)), device="cuda")
    g = gss.SphericalVariogram(range=120.0, sill=1.0, nugget=0.1)
    for k in args.neighbors:
        for K in args.cutoffs:
            cut = np.quantile(z, np.linspace(0.1, 0.9, K))
            models = [gss.SphericalVariogram(range=80.0 + 10.0 * q, sill=1.0, nugget=0.1) for q in range(K)]
            handles = [KrigHandle(g, OK, x, (z <= c).astype(np.float64), factor=False) for c in cut]

            def median_form():
                return HipEngine.ik_predict_knn(xd, zd, xdom, cut, g, k)

            def full_form():
                return HipEngine.ik_predict_knn(xd, zd, xdom, cut, models, k)

            def separate():
                for h in handles:
                    h.predict_knn(xdom, k)
            tm, tf, ts = [], [], []
            for _ in range(2):                                      # alternating blocks
                tm.append(timed(median_form, args.reps))
                tf.append(timed(full_form, args.reps))
                ts.append(timed(separate, args.reps))
            med, full, sep = statistics.median(tm), statistics.median(tf), statistics.median(ts)
            ms_ = split(median_form, ("knn", "ik_local"))
            fs_ = split(full_form, ("knn", "ik_local"))
            ss_ = split(separate, ("knn", "krig_local"))
            for h in handles:
                h.close()
            ccdf = median_form()[0]
            spare = torch.empty_like(ccdf)

            def post():
                HipEngine.ik_post(ccdf, cut, 0.0, float(z.max()) * 1.2, (1.0, 1.5), (float(cut[K // 2]),), (0.5,))

            def copy():
                spare.copy_(ccdf)
            tp, tc = [], []
            for _ in range(2):
                tp.append(timed(post, args.reps))
                tc.append(timed(copy, args.reps))
            p, c = statistics.median(tp), statistics.median(tc)
            res = {"what": "ik_predict_knn", "samples": n, "points": m, "k": k, "K": K, "reps": args.reps,
                   "median_ms": round(med, 3), "median_search_ms": ms_["knn"], "median_kernel_ms": ms_["ik_local"],
                   "full_ms": round(full, 3), "full_search_ms": fs_["knn"], "full_kernel_ms": fs_["ik_local"],
                   "separate_calls_ms": round(sep, 3), "separate_search_ms": ss_["knn"],
                   "separate_kernel_ms": ss_["krig_local"], "one_call_ms": round(sep / K, 3),
                   "separate_over_median": round(sep / med, 2), "separate_over_full": round(sep / full, 2),
                   "median_over_one_call": round(med / (sep / K), 2),
                   "post_ms": round(p, 4), "copy_ms": round(c, 4), "post_over_copy": round(p / c, 2)}
            line = json.dumps(res)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del ccdf, spare


if __name__ == "__main__":
    main()
