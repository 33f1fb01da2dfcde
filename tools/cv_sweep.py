#!/usr/bin/env python3
"""Timing of the cross-validation calls on device arrays, each beside the call of the library it shares its work with.

  * gss_krig_cv_knn (ordinary kriging, Matern-3/2, uniform 3-D samples; leave-one-out and 10 block folds) at n = 10^5
    and 10^6 samples with k = 16 and 64, beside gss_krig_predict_knn on the same handle at n query points -- the samples
    shifted by a fraction of their spacing -- and the same k: the same kriging work per point, an unmasked search.  The
    two are measured alternating; the search / solve split of each is read from gss_profile_read ("knn", "krig_local").
  * gss_krig_cv_global at n = 1 000 and 4 000 beside gss_krig_create, the fit whose factor it reads.
  * gss_krig_cv_global_folds at n = 1 000 and 4 000 with 10 shuffled folds, and at n = 4 000 with a few hundred block
    folds, beside what a user does without it: per fold gss_krig_create on the other samples and
    gss_krig_predict_global at the fold's samples.  The two alternate; the Gram kernel's share and its fraction of the
    FP64 matrix peak (--fp64-peak-tflops, 78.6 for the MI355X) come from gss_profile_read ("cv_fold_gram").

  * --estimators: gss_idw_cv / gss_lwr_cv at 5 000 and 100 000 uniform 3-D samples -- k = 16 with leave-one-out and ten
    folds, and k = n (every eligible sample) for IDW with exponent 2 under leave-one-out -- each beside the plain
    gss_idw_predict / gss_lwr_predict with xdom = xdata and the same k in the same session, alternating; the "knn" /
    estimator split of each comes from gss_profile_read ("idw_cv" / "lwr_cv" beside "idw" / "lwr"), and the k = n rows
    report the pair rate of the masked self-join beside the unmasked all-sample kernel, the latter also at a domain of
    other points (at xdom = xdata each of its points hits its own sample and rescans).  At 100 000 samples two more
    rows with exponent 3, k = n: the general est_all_kernel (predict at the other points) and est_cv_all_kernel
    (leave-one-out), which the fast kernels of exponent 1 and 2 leave the call to.

Method: warm-up, then `--reps` timed runs bracketed by events on the stream; the median is reported.  One JSON line per
row on stdout.  python tools/cv_sweep.py [--reps 5] [--max-n 1000000]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gss import _lib  # noqa: E402
from gss.engine import OK, KrigHandle  # noqa: E402
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


def split(fn):
    """(search ms, solve ms) of one call from the library's own event timers."""
    _lib.profile_enable(True)
    _lib.profile_reset()
    fn()
    torch.cuda.synchronize()
    knn, solve = _lib.profile_read("knn")[0], _lib.profile_read("krig_local")[0]
    _lib.profile_enable(False)
    return round(knn, 3), round(solve, 3)


def knn_rows(lib, reps, max_n):
    rng = np.random.default_rng(1)
    for n in (100_000, 1_000_000):
        if n > max_n:
            continue
        x = rng.uniform(0.0, 1000.0, (n, 3))
        h = KrigHandle(gss.MaternVariogram(range=60.0, order=1.5), OK, x, rng.normal(size=n), factor=False)
        spacing = 1000.0 / n ** (1.0 / 3.0)
        xq = torch.as_tensor(x + rng.uniform(-0.25, 0.25, x.shape) * spacing, device="cuda")
        block, nblocks = gss.BlockValidation((500.0, 200.0, 1001.0)).folds(x)              # 2 x 5 x 1 blocks
        assert nblocks == 10
        folds = {"loo": None, "10 block folds": torch.as_tensor(block, device="cuda")}
        out = [torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"),
               torch.empty(n, dtype=torch.uint8, device="cuda")]
        po = [C.c_void_p(o.data_ptr()) for o in out]
        for k in (16, 64):
            def predict():
                _lib.check(lib.gss_krig_predict_knn(h._h, C.c_void_p(xq.data_ptr()), None, n, k, 1, -1.0, None, 0, 0.0,
                                                    *po, None, None, _lib.MEM_DEVICE, _lib.current_stream()))
            for name, fold in folds.items():
                fp = None if fold is None else C.c_void_p(fold.data_ptr())

                def cv():
                    _lib.check(lib.gss_krig_cv_knn(h._h, fp, -1.0, k, 1, -1.0, None, 0, 0.0, *po, None, None,
                                                   _lib.MEM_DEVICE, _lib.current_stream()))
                tc, tp = [], []
                for _ in range(3):                      # alternating blocks
                    tc.append(timed(cv, reps))
                    tp.append(timed(predict, reps))
                c, p = statistics.median(tc), statistics.median(tp)
                cs, ps = split(cv), split(predict)
                print(json.dumps({"what": "cv_knn", "n": n, "k": k, "folds": name, "cv_ms": round(c, 3),
                                  "predict_knn_ms": round(p, 3), "cv_over_predict": round(c / p, 3),
                                  "cv_search_ms": cs[0], "cv_solve_ms": cs[1], "predict_search_ms": ps[0],
                                  "predict_solve_ms": ps[1], "points_per_s": round(n / (c * 1e-3), 1)}), flush=True)
        h.close()


def global_rows(lib, reps):
    rng = np.random.default_rng(2)
    for n in (1000, 4000):
        x = rng.uniform(0.0, 1000.0, (n, 3))
        z = rng.normal(size=n)
        g = gss.MaternVariogram(range=60.0, order=1.5)
        fits = []
        for _ in range(reps + 1):                       # the fit it reuses: create returns when the factor is there
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = KrigHandle(g, OK, x, z)
            fits.append((time.perf_counter() - t0) * 1e3)
            if _ < reps:
                h.close()
        out = [torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"),
               torch.empty(n, dtype=torch.uint8, device="cuda")]
        po = [C.c_void_p(o.data_ptr()) for o in out]

        def cv():
            _lib.check(lib.gss_krig_cv_global(h._h, *po, _lib.MEM_DEVICE, _lib.current_stream()))
        t = timed(cv, reps)
        h.close()
        fit = statistics.median(fits[1:])
        print(json.dumps({"what": "cv_global", "n": n, "cv_global_ms": round(t, 4), "fit_ms": round(fit, 3),
                          "cv_over_fit": round(t / fit, 5)}), flush=True)


def fold_rows(lib, reps, peak_tflops):
    rng = np.random.default_rng(3)
    g = gss.MaternVariogram(range=60.0, order=1.5)
    for n, kind in ((1000, "10 shuffled folds"), (4000, "10 shuffled folds"), (4000, "block folds")):
        x = rng.uniform(0.0, 1000.0, (n, 3))
        z = rng.normal(size=n)
        if kind == "block folds":
            fold, nfolds = gss.BlockValidation(125.0).folds(x)                             # up to 8^3 occupied blocks
        else:
            fold, nfolds = gss.KFoldValidation(10, rng=1).folds(x)
        sizes = np.bincount(fold)
        groups = [np.flatnonzero(fold == f) for f in range(nfolds)]
        rest = [np.flatnonzero(fold != f) for f in range(nfolds)]
        xin = [torch.as_tensor(x[gi], device="cuda") for gi in groups]
        h = KrigHandle(g, OK, x, z)
        dfold = torch.as_tensor(fold, device="cuda")
        out = [torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"),
               torch.empty(n, dtype=torch.uint8, device="cuda")]
        po = [C.c_void_p(o.data_ptr()) for o in out]

        def cv():
            _lib.check(lib.gss_krig_cv_global_folds(h._h, C.c_void_p(dfold.data_ptr()), *po, _lib.MEM_DEVICE,
                                                    _lib.current_stream()))

        def refits():
            for f in range(nfolds):
                hf = KrigHandle(g, OK, x[rest[f]], z[rest[f]])
                hf.predict_global(xin[f])
                hf.close()
        tc, tr = [], []
        for _ in range(3):                              # alternating blocks
            tc.append(timed(cv, reps))
            tr.append(timed(refits, 1 if kind == "block folds" else reps))
        c, r = statistics.median(tc), statistics.median(tr)
        _lib.profile_enable(True)
        _lib.profile_reset()
        cv()
        torch.cuda.synchronize()
        parts = {k: round(_lib.profile_read("cv_fold_" + k)[0], 4) for k in ("gram", "solve", "large")}
        _lib.profile_enable(False)
        pred = out[0].cpu().numpy().copy()
        refits_pred = np.empty(n)
        for f in range(min(nfolds, 3)):                 # the two routes agree (first folds only: this is a timing tool)
            hf = KrigHandle(g, OK, x[rest[f]], z[rest[f]])
            refits_pred[groups[f]] = hf.predict_global(xin[f])[0].cpu().numpy()
            hf.close()
            assert np.max(np.abs(refits_pred[groups[f]] - pred[groups[f]])) < 1e-8
        h.close()
        # useful work: the lower triangle of every B_FF, N1 s^2 / 2 multiply-adds per fold, two flops each (the kernel
        # issues whole 16 x 16 tiles and skips the k below the first column of a row block)
        flops = (n + 1) * float(np.sum(sizes.astype(np.float64) ** 2))
        gram_tflops = flops / (parts["gram"] * 1e-3) / 1e12 if parts["gram"] > 0 else float("nan")
        print(json.dumps({"what": "cv_global_folds", "n": n, "folds": kind, "nfolds": int(nfolds),
                          "largest_fold": int(sizes.max()), "cv_folds_ms": round(c, 3), "refits_ms": round(r, 3),
                          "refits_over_cv": round(r / c, 2), "gram_ms": parts["gram"], "solve_ms": parts["solve"],
                          "large_ms": parts["large"], "gram_nominal_tflops": round(gram_tflops, 3),
                          "gram_fraction_of_fp64_matrix_peak": round(gram_tflops / peak_tflops, 4)}), flush=True)


def estimator_rows(reps, max_n):
    from gss.engine import HipEngine
    rng = np.random.default_rng(4)

    def parts(fn, names):
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        out = [round(_lib.profile_read(nm)[0], 4) for nm in names]
        _lib.profile_enable(False)
        return out

    for n in (5_000, 100_000):
        if n > max_n:
            continue
        x = torch.as_tensor(rng.uniform(0.0, 1000.0, (n, 3)), device="cuda")
        z = torch.as_tensor(rng.normal(size=n), device="cuda")
        xo = x + 0.25 * 1000.0 / n ** (1.0 / 3.0)          # the same cloud a quarter of a spacing away: no sample is hit
        folds = {"loo": None, "10 folds": torch.as_tensor(gss.KFoldValidation(10, rng=1).folds(np.empty((n, 3)))[0],
                                                          device="cuda")}
        rows = [("idw", 16, name, dict(exponent=2.0)) for name in folds] + \
               [("lwr", 16, name, dict(weight=(0, 3.0, 2.0))) for name in folds] + [("idw", n, "loo", dict(exponent=2.0))]
        for est, k, name, kw in rows:
            cvf = HipEngine.idw_cv if est == "idw" else HipEngine.lwr_cv
            prf = HipEngine.idw if est == "idw" else HipEngine.lwr

            def cv():
                cvf(x, z, k, fold=folds[name], device=True, **kw)

            def predict():
                prf(x, z, x, k, **kw)
            tc, tp = [], []
            for _ in range(3):                          # alternating blocks
                tc.append(timed(cv, reps))
                tp.append(timed(predict, reps))
            c, p = statistics.median(tc), statistics.median(tp)
            cs, ps = parts(cv, ("knn", est + "_cv")), parts(predict, ("knn", est))
            row = {"what": est + "_cv", "n": n, "k": "n" if k == n else k, "folds": name, "cv_ms": round(c, 4),
                   "predict_ms": round(p, 4), "cv_over_predict": round(c / p, 3), "cv_search_ms": cs[0],
                   "cv_estimator_ms": cs[1], "predict_search_ms": ps[0], "predict_estimator_ms": ps[1]}
            if cs[0] > 0 and ps[0] > 0:
                row["search_ratio"] = round(cs[0] / ps[0], 3)
            if k == n:
                # with xdom = xdata every point of the unmasked kernel meets its own sample, its sum turns NaN and it
                # rescans the samples up to its own index one by one: the fair baseline predicts at other points
                prf(x, z, xo, k, **kw)
                po = parts(lambda: prf(x, z, xo, k, **kw), ("knn", est))
                row["predict_other_points_estimator_ms"] = po[1]
                row["predict_other_points_pairs_per_s"] = float("%.4g" % (n * float(n) / (po[1] * 1e-3)))
                row["kernel_ratio_other_points"] = round(cs[1] / po[1], 3)
                row["cv_pairs_per_s"] = float("%.4g" % (n * float(n) / (cs[1] * 1e-3)))
                row["predict_pairs_per_s"] = float("%.4g" % (n * float(n) / (ps[1] * 1e-3)))
                row["kernel_ratio"] = round(cs[1] / ps[1], 3)
            print(json.dumps(row), flush=True)
        if n == 100_000:
            # exponent 3 is not one of the fast kernels': est_all_kernel (predict at the other points) and
            # est_cv_all_kernel (leave-one-out) take these two calls
            def general():
                HipEngine.idw(x, z, xo, n, exponent=3.0)

            def general_cv():
                HipEngine.idw_cv(x, z, n, device=True, exponent=3.0)
            tg, tc = [], []
            for _ in range(3):                          # alternating blocks
                tg.append(timed(general, reps))
                tc.append(timed(general_cv, reps))
            for what, fn, t, scope in (("idw_general_predict_other_points", general, tg, "idw"),
                                       ("idw_general_cv", general_cv, tc, "idw_cv")):
                ms, est_ms = statistics.median(t), parts(fn, (scope,))[0]
                print(json.dumps({"what": what, "n": n, "k": "n", "exponent": 3.0, "folds": "loo", "ms": round(ms, 4),
                                  "estimator_ms": est_ms,
                                  "pairs_per_s": float("%.4g" % (n * float(n) / (est_ms * 1e-3)))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fp64-peak-tflops", type=float, default=78.6)
    ap.add_argument("--only-folds", action="store_true", help="the gss_krig_cv_global_folds rows only")
    ap.add_argument("--max-n", type=int, default=1_000_000)
    ap.add_argument("--estimators", action="store_true", help="the gss_idw_cv / gss_lwr_cv rows only")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.lib()
    if args.estimators:
        return estimator_rows(args.reps, args.max_n)
    fold_rows(lib, args.reps, args.fp64_peak_tflops)
    if args.only_folds:
        return
    global_rows(lib, args.reps)
    knn_rows(lib, args.reps, args.max_n)


if __name__ == "__main__":
    main()
