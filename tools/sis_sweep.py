#!/usr/bin/env python3
"""Timing of the sweep of gss_sis_realize beside the SGS sweep of the same handle, and of its two ways through a handle
with many short levels.

  Handle: the SGS row of the README -- 512 x 512 cells, spherical range 35, k = 16 inside a ball of 30, 200 conditioning
  cells, 1 024 realisations, device output -- once with a shared random visiting order and once row by row (LinearPath).
  On each handle, in the same session: the "sgs_sweep" scope of gss_sgs_realize, then the "sis_sweep" scope of
  gss_sis_realize for K = 4 / 8 / 16 cutoffs and K = 3 / 8 categories.  SIS reads the same lists and gathers the same
  bytes, so the ratio is what the K accumulators and the draw cost.

  The launch rule: on the row-by-row handle, and on a 1-D line of 32 768 cells whose every level is one node, the sweep
  level by level (GSS_SIS_WALK_BELOW=0) beside the walk along the path (GSS_SIS_WALK_BELOW=1e30): time per level of the
  one, per node of the other, and their ratio -- the average level size below which the walk wins.

Method: one warm-up call, then `--reps` calls with the profile scopes on; the median is reported.  One JSON line per
(handle, kind, K) on stdout and appended to --out (default profiles/sis_sweep.jsonl).
python tools/sis_sweep.py [--reps 3] [--edge 512] [--reals 1024]"""
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
from gss.engine import SGSHandle  # noqa: E402
import gss  # noqa: E402


def scope_ms(fn, scope, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    _lib.profile_enable(True)
    for _ in range(reps):
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        ms.append(_lib.profile_read(scope)[0])
    _lib.profile_enable(False)
    return statistics.median(ms)


def rule(kind, K):
    if kind == "categorical":
        return ("categorical", None, np.full(K, 1.0 / K), 0.0, 0.0, (1.0, 1.0))
    return ("continuous", np.linspace(-0.5, 2.5, K), np.linspace(0.05, 0.95, K), -1.0, 3.0, (1.0, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--reals", type=int, default=1024)
    ap.add_argument("--line", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sis_sweep.jsonl"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    _lib.lib()
    from oracle.fftgs import grid_centroids
    R = args.reals
    vg = gss.SphericalVariogram(range=35.0)
    kinds = [("continuous", 4), ("continuous", 8), ("continuous", 16), ("categorical", 3), ("categorical", 8)]

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    def handle(dims, order):
        cent = grid_centroids(dims)
        N = cent.shape[0]
        rng = np.random.default_rng(5)
        dl = np.sort(rng.choice(N, 200, replace=False))
        zd = rng.integers(0, 3, 200).astype(np.float64)      # codes of three categories; values like any for the others
        path = None if order == "linear" else np.random.default_rng(6).permutation(N)
        return SGSHandle(vg, cent, path, dl, zd, 0.0, 16, 1, 30.0), N

    for dims, order in (((args.edge, args.edge), "random"), ((args.edge, args.edge), "linear"), ((args.line,), "linear")):
        h, N = handle(dims, order)
        sch = h.schedule()
        out = torch.empty((R, N), dtype=torch.float64, device="cuda")
        base = dict(what="sis_sweep", dims=list(dims), order=order, k=16, reals=R, reps=args.reps, levels=sch["levels"],
                    team_rl=sch["team_rl"], nodes_per_level=round((N - 200) / max(sch["levels"], 1), 2))
        sgs = scope_ms(lambda: h.realize(1, 0, R, out=out), "sgs_sweep", args.reps)
        for kind, K in kinds:
            if len(dims) == 1 and (kind, K) not in (("continuous", 4), ("categorical", 3)):
                continue
            res = dict(base, kind=kind, K=K, sgs_sweep_ms=round(sgs, 3))
            for name, below in (("levels", "0"), ("walk", "1e30")):
                if name == "walk" and order == "random" and (kind, K) != ("continuous", 4):
                    continue                                 # the walk of a random order: once, for the record
                os.environ["GSS_SIS_WALK_BELOW"] = below
                ms = scope_ms(lambda: h.realize_indicator(*rule(kind, K), 1, 0, R, out=out), "sis_sweep", args.reps)
                res["sis_%s_ms" % name] = round(ms, 3)
            os.environ.pop("GSS_SIS_WALK_BELOW", None)
            res["sis_over_sgs"] = round(res["sis_levels_ms"] / sgs, 2)
            if "sis_walk_ms" in res:
                res["us_per_level"] = round(res["sis_levels_ms"] * 1e3 / max(sch["levels"], 1), 3)
                res["us_per_walked_node"] = round(res["sis_walk_ms"] * 1e3 / (N - 200), 3)
                res["walk_wins_below_nodes_per_level"] = round(res["us_per_level"] / res["us_per_walked_node"], 2)
            emit(res)
        h.close()
        del out


if __name__ == "__main__":
    main()
