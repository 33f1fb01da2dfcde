#!/usr/bin/env python3
"""Timing of gss_variogram_empirical on device arrays: uniform 3-D samples, nz = 1, nlags = 20.

  * n = 2*10^4 and 10^5 with maxlag = the full diameter and with 5 % of the extent; n = 10^6 with 5 % only;
  * the yardstick: gss_cov_pairwise with b == NULL (exponential model, device memory) on the same 2*10^4 samples runs
    the same pair loop over BOTH triangles plus an exp and an 8-byte store per pair -- the full-diameter variogram call
    at that size must not take longer.  The two are measured alternating in one session.

Method: warm-up, then `--reps` timed runs, each bracketed by events on the stream (the call includes the ordering of the
samples and the reduction: what a user pays; both calls are bare ctypes calls on preallocated outputs); the median is
reported.  One JSON line
per row on stdout.  python tools/vario_sweep.py [--reps 7] [--max-n 1000000]

--plane: instead, the varioplane rows (gss_variogram_plane, 18 sectors x 20 lags, one value column, 2-D and 3-D with
ptol = inf) at 2*10^4 and 10^5 samples with the full diameter and at 10^5 with lags to 5 % of the extent.  Beside each:
the only way to the same table without that call -- 18 calls of gss_variogram_empirical with direction = the
mid-sector unit vector and cos_atol = cos(pi / 36), timed as one block -- and the omnidirectional call.  The three are
measured alternating.  (To time the 18 calls on another build of the library, run this with GSS_LIB_PATH set to it and
--yardstick-only: that build need not have the plane call.)

--cross: 10^5 samples in 3-D, all pairs, 20 lags, nz = 2 and 8: gss_variogram_cross against the polarisation route on the
same library -- gss_variogram_empirical on the nz (nz + 1) / 2 columns z_a and z_a + z_b, in as many calls as its limit
of 8 columns needs.  The two alternate, every run in a fresh process (one warm-up call, one timed call between events),
five runs each; the medians are compared."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gss import _lib  # noqa: E402
from gss.engine import _vg_struct  # noqa: E402
import gss  # noqa: E402


def timed(fn, reps, warm=2):
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
    return statistics.median(ms), min(ms)


def bare_variogram(lib, x, z, nlags, maxlag):
    """The call as a bare ctypes call on preallocated outputs -- what the yardstick's call is timed as."""
    n, d = x.shape
    count = torch.empty(nlags, dtype=torch.int64, device="cuda")
    lagsum = torch.empty(nlags, dtype=torch.float64, device="cuda")
    zsum = torch.empty((z.shape[0], nlags), dtype=torch.float64, device="cuda")
    ndup = torch.empty(1, dtype=torch.int64, device="cuda")
    args = (C.c_void_p(x.data_ptr()), n, d, C.c_void_p(z.data_ptr()), z.shape[0], nlags, float(maxlag), None,
            float("inf"), 0.0, 0, C.c_void_p(count.data_ptr()), C.c_void_p(lagsum.data_ptr()),
            C.c_void_p(zsum.data_ptr()), C.c_void_p(ndup.data_ptr()), _lib.MEM_DEVICE)

    def run():
        _lib.check(lib.gss_variogram_empirical(*args, _lib.current_stream()))
    return run, (count, lagsum, zsum, ndup)


def bare_directional(lib, x, z, nlags, maxlag, nangles):
    """`nangles` directional calls (mid-sector direction, cone of half a sector) as one block of bare calls."""
    n, d = x.shape
    outs = (torch.empty(nlags, dtype=torch.int64, device="cuda"), torch.empty(nlags, dtype=torch.float64, device="cuda"),
            torch.empty((z.shape[0], nlags), dtype=torch.float64, device="cuda"),
            torch.empty(1, dtype=torch.int64, device="cuda"))
    us = []
    for s in range(nangles):
        a = (s + 0.5) * np.pi / nangles
        us.append(np.ascontiguousarray([np.cos(a), np.sin(a), 0.0][:d] if d == 3 else [np.cos(a), np.sin(a)]))
    cos_atol = float(np.cos(np.pi / (2 * nangles)))

    def run():
        for u in us:
            _lib.check(lib.gss_variogram_empirical(
                C.c_void_p(x.data_ptr()), n, d, C.c_void_p(z.data_ptr()), z.shape[0], nlags, float(maxlag), _lib.ptr(u),
                float("inf"), cos_atol, 0, *(C.c_void_p(o.data_ptr()) for o in outs), _lib.MEM_DEVICE,
                _lib.current_stream()))
    return run


def bare_plane(lib, x, z, nlags, maxlag, nangles):
    n, d = x.shape
    ang = np.arange(nangles) * np.pi / nangles
    dirs = np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1))
    basis = np.ascontiguousarray(np.eye(3)) if d == 3 else None
    count = torch.empty((nangles, nlags), dtype=torch.int64, device="cuda")
    outs = (count, torch.empty((nangles, nlags), dtype=torch.float64, device="cuda"),
            torch.empty((z.shape[0], nangles, nlags), dtype=torch.float64, device="cuda"),
            torch.empty(1, dtype=torch.int64, device="cuda"))

    def run():
        _lib.check(lib.gss_variogram_plane(
            C.c_void_p(x.data_ptr()), n, d, C.c_void_p(z.data_ptr()), z.shape[0], nlags, float(maxlag), nangles,
            _lib.ptr(dirs), _lib.ptr(basis), float("inf"), 0, *(C.c_void_p(o.data_ptr()) for o in outs), _lib.MEM_DEVICE,
            _lib.current_stream()))
    return run, outs


def plane_rows(lib, reps, yardstick_only):
    rng = np.random.default_rng(1)
    nangles, nlags = 18, 20
    for d in (2, 3):
        for n, label in ((20_000, "full"), (100_000, "full"), (100_000, "5pct")):
            x = torch.as_tensor(rng.uniform(0.0, 1000.0, (n, d)), device="cuda")
            z = torch.as_tensor(rng.normal(size=(1, n)), device="cuda")
            maxlag = 1000.0 * d ** 0.5 if label == "full" else 50.0
            run_dir = bare_directional(lib, x, z, nlags, maxlag, nangles)
            run_omni, _ = bare_variogram(lib, x, z, nlags, maxlag)
            row = {"what": "varioplane", "n": n, "dim": d, "maxlag": label, "nangles": nangles, "nlags": nlags, "nz": 1}
            if yardstick_only:
                row["directional_x18_ms"] = round(timed(run_dir, reps, warm=1)[0], 4)
                row["omnidirectional_ms"] = round(timed(run_omni, reps, warm=1)[0], 4)
            else:
                run_plane, outs = bare_plane(lib, x, z, nlags, maxlag, nangles)
                tp, td, to = [], [], []
                for _ in range(3):                      # alternating blocks
                    tp.append(timed(run_plane, reps, warm=1)[0])
                    td.append(timed(run_dir, reps, warm=1)[0])
                    to.append(timed(run_omni, reps, warm=1)[0])
                _lib.profile_enable(True)
                _lib.profile_reset()
                run_plane()
                kms, launches = _lib.profile_read("vario_plane")
                _lib.profile_enable(False)
                p, dd, o = statistics.median(tp), statistics.median(td), statistics.median(to)
                row.update({"plane_ms": round(p, 4), "directional_x18_ms": round(dd, 4), "omnidirectional_ms": round(o, 4),
                            "plane_kernel_ms": round(kms / max(launches, 1), 4),
                            "plane_over_directional": round(p / dd, 4), "plane_over_omnidirectional": round(p / o, 3),
                            "pairs_binned": int(outs[0].sum().item()),
                            "tiles_opened": _lib.stat("vario_tiles_opened"), "tiles_total": _lib.stat("vario_tiles_total")})
            print(json.dumps(row), flush=True)


def cross_child(route, nz):
    """one timed call of one route in this process -> milliseconds on stdout"""
    lib = _lib.lib()
    rng = np.random.default_rng(1)
    n, nlags, maxlag = 100_000, 20, 1000.0 * 3 ** 0.5
    x = torch.as_tensor(rng.uniform(0.0, 1000.0, (n, 3)), device="cuda")
    zh = rng.normal(size=(nz, n))
    if route == "cross":
        z = torch.as_tensor(zh, device="cuda")
        outs = (torch.empty(nlags, dtype=torch.int64, device="cuda"), torch.empty(nlags, dtype=torch.float64, device="cuda"),
                torch.empty((nz * (nz + 1) // 2, nlags), dtype=torch.float64, device="cuda"),
                torch.empty(1, dtype=torch.int64, device="cuda"))

        def run():
            _lib.check(lib.gss_variogram_cross(
                C.c_void_p(x.data_ptr()), n, 3, C.c_void_p(z.data_ptr()), nz, nlags, maxlag, None, float("inf"), 0.0,
                *(C.c_void_p(o.data_ptr()) for o in outs), _lib.MEM_DEVICE, _lib.current_stream()))
    else:
        cols = [zh[a] for a in range(nz)] + [zh[a] + zh[b] for a in range(nz) for b in range(a + 1, nz)]
        runs = [bare_variogram(lib, x, torch.as_tensor(np.stack(cols[lo:lo + 8]), device="cuda"), nlags, maxlag)[0]
                for lo in range(0, len(cols), 8)]

        def run():
            for r in runs:
                r()
    med, _ = timed(run, 1, warm=1)
    print(json.dumps({"route": route, "nz": nz, "ms": med}), flush=True)


def cross_rows(runs=5):
    import subprocess
    for nz in (2, 8):
        times = {"cross": [], "polarisation": []}
        for _ in range(runs):
            for route in ("cross", "polarisation"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cross-child", route, str(nz)],
                                   capture_output=True, text=True, timeout=600, check=True)
                times[route].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        c, p = statistics.median(times["cross"]), statistics.median(times["polarisation"])
        print(json.dumps({"what": "cross-variogram", "n": 100_000, "dim": 3, "maxlag": "full", "nlags": 20, "nz": nz,
                          "columns_polarisation": nz * (nz + 1) // 2, "calls_polarisation": (nz * (nz + 1) // 2 + 7) // 8,
                          "cross_ms": [round(t, 4) for t in times["cross"]],
                          "polarisation_ms": [round(t, 4) for t in times["polarisation"]],
                          "cross_median_ms": round(c, 4), "polarisation_median_ms": round(p, 4),
                          "cross_over_polarisation": round(c / p, 4), "cross_not_slower": c <= p}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cross", action="store_true", help="the cross-variogram rows instead")
    ap.add_argument("--cross-child", nargs=2, metavar=("ROUTE", "NZ"), help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-n", type=int, default=1_000_000)
    ap.add_argument("--plane", action="store_true", help="the varioplane rows instead")
    ap.add_argument("--yardstick-only", action="store_true", help="with --plane: only the 18 directional calls and the "
                    "omnidirectional one (for a build of the library without the plane call)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.cross_child:
        cross_child(args.cross_child[0], int(args.cross_child[1]))
        return
    if args.cross:
        cross_rows()
        return
    lib = _lib.lib()
    if args.plane:
        plane_rows(lib, args.reps, args.yardstick_only)
        return
    rng = np.random.default_rng(1)
    for n in (20_000, 100_000, 1_000_000):
        if n > args.max_n:
            continue
        x = torch.as_tensor(rng.uniform(0.0, 1000.0, (n, 3)), device="cuda")
        z = torch.as_tensor(rng.normal(size=(1, n)), device="cuda")
        diam = 1000.0 * 3 ** 0.5
        for label, maxlag in (("full", diam), ("5pct", 50.0)):
            if label == "full" and n > 100_000:
                continue
            run, outs = bare_variogram(lib, x, z, 20, maxlag)
            reps = args.reps if n <= 100_000 else 3
            _lib.profile_enable(True)
            _lib.profile_reset()
            med, best = timed(run, reps)
            kms, launches = _lib.profile_read("vario_pairs")
            _lib.profile_enable(False)
            pairs = int(outs[0].sum().item())
            row = {"what": "variogram", "n": n, "maxlag": label, "nlags": 20, "nz": 1, "median_ms": round(med, 4),
                   "min_ms": round(best, 4), "pairs_kernel_ms": round(kms / max(launches, 1), 4),
                   "pairs_binned": pairs, "pairs_visited": n * (n - 1) // 2 if label == "full" else None,
                   "binned_pairs_per_s": round(pairs / (med * 1e-3), 1),
                   "tiles_opened": _lib.stat("vario_tiles_opened"), "tiles_total": _lib.stat("vario_tiles_total")}
            print(json.dumps(row), flush=True)
        if n == 20_000:
            # the yardstick, alternating with the full-diameter call
            vg = _vg_struct(gss.ExponentialVariogram(range=300.0), 3)
            cov = torch.empty((n, n), dtype=torch.float64, device="cuda")

            def run_cov():
                _lib.check(lib.gss_cov_pairwise(C.byref(vg), C.c_void_p(x.data_ptr()), n, None, n,
                                                C.c_void_p(cov.data_ptr()), n, _lib.MEM_DEVICE, _lib.current_stream()))

            run_var, _ = bare_variogram(lib, x, z, 20, diam)
            tv, tc = [], []
            for _ in range(3):
                tv.append(timed(run_var, args.reps, warm=1)[0])
                tc.append(timed(run_cov, args.reps, warm=1)[0])
            print(json.dumps({"what": "yardstick", "n": n, "variogram_full_ms": [round(t, 4) for t in tv],
                              "cov_pairwise_ms": [round(t, 4) for t in tc],
                              "variogram_median_ms": round(statistics.median(tv), 4),
                              "cov_pairwise_median_ms": round(statistics.median(tc), 4),
                              "variogram_not_slower": statistics.median(tv) <= statistics.median(tc)}), flush=True)
            del cov


if __name__ == "__main__":
    main()
