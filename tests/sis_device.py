"""The runs of tests/sis_cases.py on the device, for tests/test_gpu_sis.py: the handle's lists and weights of every path the
run draws from, its number of levels, and the field from the run's Philox seed and from the same uniforms passed
explicitly.  `python sis_device.py OUT.npz RUN ...` does runs in a process of its own (GSS_SGS_LEVELS is read once per
process).  Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sis_cases as SC
import sis_ref as SR


def variogram(run):
    import gss
    kind, rng, sill, nugget = SR.variogram_args(run)
    assert kind == "spherical"
    return gss.SphericalVariogram(range=rng, sill=sill, nugget=nugget)


def handle(run, geo, paths=None, zdata=None, path_base=None):
    from gss.engine import SGSHandle
    if paths is None:
        paths = geo["paths"] if run.npaths > 1 else geo["paths"][0]
    return SGSHandle(variogram(run), geo["cent"], paths, geo["dl"], geo["zd"] if zdata is None else zdata, mean=0.0,
                     maxneighbors=run.k, minneighbors=run.nmin, path_base=run.path_base if path_base is None else path_base)


def rule(run, geo):
    """The leading arguments of SGSHandle.realize_indicator."""
    return ("categorical" if run.categorical else "continuous", geo["cut"], geo["fs"], geo["zmin"], geo["zmax"], run.tail)


def device_run(run):
    geo = SR.geometry(run)
    h = handle(run, geo)
    out = {"levels": np.int64(h.schedule()["levels"])}
    old = os.environ.get("GSS_SIS_WALK_BELOW")
    os.environ["GSS_SIS_WALK_BELOW"] = "0"          # level by level however short the levels (read at every call)
    try:
        out["z"] = h.realize_indicator(*rule(run, geo), run.seed, run.first_real, run.R)
        out["z_u"] = h.realize_indicator(*rule(run, geo), 0, run.first_real, run.R, uniforms=geo["U"])
    finally:
        os.environ.pop("GSS_SIS_WALK_BELOW")
        if old is not None:
            os.environ["GSS_SIS_WALK_BELOW"] = old
    if run.npaths == 1:
        out["idx0"], out["nc0"], out["w0"], _ = h.weights()
    h.close()
    if run.npaths > 1:
        for p, _ in SR.blocks(run):
            hp = handle(run, geo, paths=geo["paths"][p], path_base=0)
            out["idx%d" % p], out["nc%d" % p], out["w%d" % p], _ = hp.weights()
            hp.close()
    return out


def main(argv):
    res = {}
    for name in argv[2:]:
        for q, v in device_run(SC.RUNS[name]).items():
            res[name + "/" + q] = v
    np.savez(argv[1], **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
