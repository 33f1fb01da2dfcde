#!/usr/bin/env python3
"""Timing of the normal-score back-transform (gss_nscore_apply, inverse, in place, device memory) beside a copy of the
same bytes and beside what a user writes in torch today.

  Workloads: one n^3 field (default 512), and 16 fields of (n/4)^3 laid out as variable 0 of a 16 x 2 x N co-simulation
  output (16 runs, 2 N apart, one launch).  Scores are standard normal.  Rows, per workload:
    nscore_lds     table of 1 000 knots (searched in LDS)
    nscore_global  table of 10^6 knots (searched in global memory / L2)
    copy           torch `dst.copy_(src)` of the same 8 N bytes in and 8 N bytes out
    torch_1000     the composition on the 1 000-knot table: special.ndtr, searchsorted on the knots' probabilities, two
    torch_1e6      gathers of the values and a lerp -- six passes and an int64 index as large as the field; the same on
                   the 10^6-knot table
  The kernel must beat the torch rows (asserted); its ratio to the copy is reported.

Method: every row is warmed `--warmup` times, then the rows alternate for `--reps` rounds; a call is bracketed by events
on the stream (the in-place rows restore their input before the first event) and the medians and the spread (min .. max)
are reported.  The kernel alone is also read from the library's profile scope "nscore_apply" over `--reps` further
calls.  One JSON line per workload on stdout and in profiles/nscore_sweep.jsonl.
python tools/nscore_sweep.py [--n 512] [--reps 20] [--warmup 3]"""
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
from gss.engine import NScoreHandle  # noqa: E402


def event_ms(fn, before=None):
    if before:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_inverse(y, pk, vk):
    """Quantile back-transform of an equal-weight table in torch: p = Phi(y), bracket among the knots' probabilities
    (k + 1/2) / K, gather the two values, lerp; clamped at the extreme values as the default tails do."""
    K = vk.numel()
    p = torch.special.ndtr(y)
    i = torch.searchsorted(pk, p, right=True).clamp_(1, K - 1)
    lo, hi = vk[i - 1], vk[i]
    w = (p * K - (i.to(torch.float64) - 0.5)).clamp_(0.0, 1.0)
    return torch.lerp(lo, hi, w)


def workload(name, view, base, a, tables):
    """`view`: the tensor the rows transform (a view of `base`, which is restored from a pristine copy)."""
    pristine = base.clone()
    restore = lambda: base.copy_(pristine)                                        # noqa: E731
    src = view.clone()                                                            # contiguous, never transformed
    dst = torch.empty_like(src)
    rows = {}
    for key, (h, pk, vk) in tables.items():
        rows["nscore_" + key] = (lambda h=h: h.inverse(view, out=view), restore)
    rows["copy"] = (lambda: dst.copy_(src), None)
    rows["torch_1000"] = (lambda: torch_inverse(src, *tables["lds"][1:]), None)
    rows["torch_1e6"] = (lambda: torch_inverse(src, *tables["global"][1:]), None)
    for fn, before in rows.values():
        for _ in range(a.warmup):
            event_ms(fn, before)
    times = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, (fn, before) in rows.items():
            times[k].append(event_ms(fn, before))
    n = view.numel()
    res = {"workload": name, "elements": n, "bytes_moved": 16 * n, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    for k, ms in times.items():
        med = statistics.median(ms)
        res[k] = {"ms_median": med, "min": min(ms), "max": max(ms), "GBps": 16.0 * n / (med * 1e-3) / 1e9}
    _lib.profile_enable(True)
    for key in tables:
        fn, before = rows["nscore_" + key]
        _lib.profile_reset()
        for _ in range(a.reps):
            before()
            fn()
        torch.cuda.synchronize()
        ms, cnt = _lib.profile_read("nscore_apply")
        res["nscore_" + key]["scope_ms_mean"] = ms / max(cnt, 1)
        res["nscore_" + key]["launches_per_call"] = cnt // a.reps
    _lib.profile_enable(False)
    # the torch composition is the same table read linearly in p between the knots, where the kernel is linear in y:
    # close, not equal
    restore()
    got = tables["lds"][0].inverse(src)
    ref = torch_inverse(src, *tables["lds"][1:])
    res["max_abs_diff_torch_vs_kernel"] = float((got - ref).abs().max())
    c = res["copy"]["ms_median"]
    res["ratios"] = {"lds_over_copy": res["nscore_lds"]["ms_median"] / c,
                     "global_over_copy": res["nscore_global"]["ms_median"] / c,
                     "torch_1000_over_lds": res["torch_1000"]["ms_median"] / res["nscore_lds"]["ms_median"],
                     "torch_1e6_over_global": res["torch_1e6"]["ms_median"] / res["nscore_global"]["ms_median"]}
    assert res["ratios"]["torch_1000_over_lds"] > 1.0 and res["ratios"]["torch_1e6_over_global"] > 1.0, res["ratios"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--knots-global", type=int, default=1000000)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    tables = {}
    for key, K in (("lds", 1000), ("global", a.knots_global)):
        z = np.exp(rng.normal(0.3, 0.9, K))
        h = NScoreHandle(z)
        v, _ = h.table()
        assert v.size == K
        pk = torch.as_tensor((np.arange(K) + 0.5) / K, device="cuda")
        tables[key] = (h, pk, torch.as_tensor(v, device="cuda"))
    gen = torch.Generator(device="cuda").manual_seed(3)
    N = a.n ** 3
    lines = []
    field = torch.randn(N, dtype=torch.float64, device="cuda", generator=gen)
    lines.append(workload("1 x %d^3" % a.n, field, field, a, tables))
    del field
    m = (a.n // 4) ** 3
    joint = torch.randn((16, 2, m), dtype=torch.float64, device="cuda", generator=gen)
    lines.append(workload("16 x %d^3, variable 0 of nz = 2" % (a.n // 4), joint[:, 0], joint, a, tables))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "nscore_sweep.jsonl"), "w") as f:
        for r in lines:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
