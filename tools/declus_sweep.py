#!/usr/bin/env python3
"""Timing of the declustering calls on device arrays, beside the numpy restatement of the tests on the host.

  Rows:
    cells_1e5, cells_1e6   gss_decluster_cells, 3-D clustered samples, 24 sizes x 8 offsets (192 grids); with the share
                           of the radix sorts (profile scopes "declus_sort" / "declus_cells")
    counts_1e6             gss_decluster_cell_counts, one grid
    nearest_1e6            gss_decluster_nearest, 10^6 samples, 256^3 lattice, beside gss_knn_search (k = 1) of the same
                           16.8 M centres formed by torch beforehand (the search alone)
    host_*                 tests/decluster_ref.py on the same inputs: `--host-grids` grids of the sweep are timed (all 192
                           take minutes at 10^6) and the figure for 192 is that time scaled, marked "extrapolated"

Method: every device row is warmed `--warmup` times, then the rows alternate for `--reps` rounds; a call is bracketed by
events on the stream (the calls end with a wait for their host words, so this is the call as a user sees it) and the
median and the spread (min .. max) are reported.  One JSON line on stdout and in profiles/declus_sweep.jsonl, then the
README row.
python tools/declus_sweep.py [--reps 7] [--warmup 2] [--host-grids 8] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import decluster_ref as R  # noqa: E402
from gss import _lib  # noqa: E402
from gss.engine import HipEngine as E  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def clustered(n, seed):
    """70 % of the samples in a blob of high values, the rest uniform over [0, 1000]^3"""
    rng = np.random.default_rng(seed)
    nb = (7 * n) // 10
    x = np.concatenate([500.0 + 40.0 * rng.standard_normal((nb, 3)), rng.uniform(0.0, 1000.0, (n - nb, 3))])
    z = np.concatenate([10.0 + rng.standard_normal(nb), 1.0 + 0.1 * rng.standard_normal(n - nb)])
    p = rng.permutation(n)
    return np.ascontiguousarray(x[p]), np.ascontiguousarray(z[p])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-grids", type=int, default=8)
    ap.add_argument("--small", action="store_true", help="a tenth of every size (a quick check of the tool itself)")
    a = ap.parse_args()
    scale = 10 if a.small else 1
    n5, n6, lat = 100_000 // scale, 1_000_000 // scale, (256 if not a.small else 64)
    ncs, noff = 24, 8
    sides = np.repeat(np.linspace(5.0, 120.0, ncs)[:, None], 3, axis=1)
    data = {n: clustered(n, n % 1000) for n in (n5, n6)}
    dev = {n: (torch.as_tensor(x, device="cuda"), torch.as_tensor(z, device="cuda")) for n, (x, z) in data.items()}
    x6, _ = dev[n6]
    lo6 = data[n6][0].min(axis=0)
    step = (data[n6][0].max(axis=0) - lo6) / lat
    ax = [torch.as_tensor(lo6[k] + (np.arange(lat) + 0.5) * step[k], device="cuda") for k in range(3)]
    centres = torch.stack(torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")[::-1], dim=-1).reshape(-1, 3).contiguous()

    rows = {
        "cells_1e5": lambda: E.decluster_cells(*dev[n5], sides, noff),
        "cells_1e6": lambda: E.decluster_cells(*dev[n6], sides, noff),
        "counts_1e6": lambda: E.decluster_cell_counts(x6, lo6, sides[5]),
        "nearest_1e6": lambda: E.decluster_nearest(x6, lo6, step, [lat] * 3),
        "knn_search_same_centres": lambda: E.knn_search(x6, centres, 1),
    }
    for fn in rows.values():
        for _ in range(a.warmup):
            event_ms(fn)
    times = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            times[k].append(event_ms(fn))
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "n": [n5, n6], "ncs": ncs,
           "noff": noff, "lattice": [lat] * 3}
    for k, ms in times.items():
        res[k] = {"ms_median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    _lib.profile_enable(True)
    for key in ("cells_1e5", "cells_1e6"):
        _lib.profile_reset()
        for _ in range(3):
            rows[key]()
        torch.cuda.synchronize()
        total, _ = _lib.profile_read("declus_cells")
        sort, nsort = _lib.profile_read("declus_sort")
        res[key]["sort_share"] = sort / total if total > 0 else None
        res[key]["sorts_per_call"] = nsort // 3
    _lib.profile_enable(False)

    # the device against the restatement (exact quantities) and the restatement's time on the host
    hg = max(1, min(a.host_grids, noff))
    for key, n in (("host_cells_1e5", n5), ("host_cells_1e6", n6)):
        x, z = data[n]
        lo = x.min(axis=0)
        t0 = time.perf_counter()
        cnts = [R.cell_counts(x, R.origin_of(lo, sides[0], k, noff), sides[0]) for k in range(hg)]
        dt = time.perf_counter() - t0
        res[key] = {"grids_timed": hg, "s_timed": dt, "s_192_grids_extrapolated": dt * ncs * noff / hg}
        cnt, occ = E.decluster_cell_counts(dev[n][0], R.origin_of(lo, sides[0], hg - 1, noff), sides[0])
        assert np.array_equal(cnt.cpu().numpy(), cnts[-1][0]) and occ == cnts[-1][1]
    print(json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "declus_sweep.jsonl"), "w") as f:
        f.write(json.dumps(res) + "\n")
    c5, c6 = res["cells_1e5"], res["cells_1e6"]
    print("| declustering weights on the device (`tools/declus_sweep.py`), 3-D clustered samples, device arrays: the GSLIB "
          "cell sweep of 24 sizes x 8 offsets at 10^5 / 10^6 samples; one grid at 10^6; polygonal weights of 10^6 samples "
          "on a %d^3 lattice | %.1f / %.1f ms (radix sorts %.0f %% / %.0f %% of it; the numpy restatement on the host: "
          "%.0f / %.0f s, extrapolated from %d grids); %.2f ms; %.1f ms, against %.1f ms for `gss_knn_search` of the same "
          "centres alone (DESIGN.md section 4 \"Declustering\") |"
          % (lat, c5["ms_median"], c6["ms_median"], 100 * (c5["sort_share"] or 0), 100 * (c6["sort_share"] or 0),
             res["host_cells_1e5"]["s_192_grids_extrapolated"], res["host_cells_1e6"]["s_192_grids_extrapolated"], hg,
             res["counts_1e6"]["ms_median"], res["nearest_1e6"]["ms_median"],
             res["knn_search_same_centres"]["ms_median"]))


if __name__ == "__main__":
    main()
