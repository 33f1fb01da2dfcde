"""How far the FP64 restatement of indicator kriging (tests/ik_ref.py) is from the same systems solved in long double,
on the inputs of tests/ik_cases.py and of the kernel table tests/ik_kernel_cases.py: the figures the error bars of tests/test_gpu_ik.py are derived from (bar = 16 x the
figure, floored at 8 and capped at 1e-9, as tests/test_kernel_census.py holds the kriging bars).  CPU only.

Raw ccdf: units of 2^-53 max(1, sum |lambda|) per (point, cutoff).  Post-processing: units of 2^-53 x the scale of the
output (zmax for the mean and the quantiles, zmax^2 for the variance, 1 for the probabilities).

    python tools/ik_oracle.py        # prints ORACLE = {...} for tests/test_gpu_ik.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ik_cases  # noqa: E402
import ik_kernel_cases  # noqa: E402
import ik_ref  # noqa: E402

UNIT = 2.0 ** -53


def raw_error(c):
    """-> (the figure, the FP64 result) of one case"""
    kw = dict(minneighbors=c.get("minneighbors", 1), fstar=c["fstar"], radius=c.get("radius"))
    a = ik_ref.predict(c["x"], c["z"], c["x0"], c["cutoffs"], c["models"], c["k"], **kw)
    b = ik_ref.predict(c["x"], c["z"], c["x0"], c["cutoffs"], c["models"], c["k"], longdouble=True, **kw)
    ok = a["status"] == 0
    if not ok.any():
        return 0.0, a
    err = np.abs(a["raw"][ok].astype(np.longdouble) - b["raw_ld"][ok]) / (UNIT * a["wsum"][ok])
    return float(err.max()), a


def global_error(c, a):
    """The dual form of the global route (ik_ref.predict_global) in FP64 against long double, in the units of the
    moving route with every sample a neighbour (a: its FP64 result, for sum |lambda|)."""
    d = ik_ref.predict_global(c["x"], c["z"], c["x0"], c["cutoffs"], c["models"], fstar=c["fstar"])
    e = ik_ref.predict_global(c["x"], c["z"], c["x0"], c["cutoffs"], c["models"], fstar=c["fstar"], longdouble=True)
    return float((np.abs(d["raw"].astype(np.longdouble) - e["raw_ld"]) / (UNIT * a["wsum"])).max())


def post_scales(zmax):
    return dict(etype=zmax, cvar=zmax * zmax, pabove=1.0, quant=zmax)


def post_error(rows, cutoffs, wlo, whi, **kw):
    a = ik_ref.post(rows, cutoffs, wlo=wlo, whi=whi, **kw)
    b = ik_ref.post(rows, cutoffs, wlo=wlo, whi=whi, longdouble=True, **kw)
    worst = 0.0
    for name, scale in post_scales(kw["zmax"]).items():
        d = np.abs(a[name] - b[name])
        if np.isfinite(d).any():
            worst = max(worst, float(np.nanmax(d)) / (UNIT * scale))
    return worst


def main():
    out = {}
    post_cases = 0.0
    for name, c in ik_cases.cases().items():
        err, a = raw_error(c)
        out[name] = round(err, 2)
        if name.startswith("route_"):
            out[name + "_global"] = round(global_error(c, a), 2)
        # post-processing of the case's corrected ccdf, with the arguments the test uses
        for w, w2 in ik_cases.POST_TAILS:
            post_cases = max(post_cases, post_error(a["ccdf"], c["cutoffs"], w, w2, **ik_cases.post_args_for(c)))
    # the table of compiled kernels (raw ccdf only: the post-processing test runs on the cases above)
    for key, entry in ik_kernel_cases.KERNELS.items():
        if not isinstance(entry, ik_kernel_cases.UNREACHABLE):
            out[ik_kernel_cases.name_of(key)] = round(raw_error(entry())[0], 2)
    rows = ik_cases.post_rows()
    out["post"] = round(max(post_error(rows, ik_cases.POST_CUTOFFS, w, w2, **ik_cases.POST_ARGS)
                            for w, w2 in ik_cases.POST_TAILS), 2)
    out["post_cases"] = round(post_cases, 2)
    print("ORACLE = {")
    for k, v in out.items():
        print(f"    {k!r}: {v},")
    print("}")


if __name__ == "__main__":
    main()
