#!/usr/bin/env python3
"""Fingerprint of what the FFTGS entry points return: a SHA-256 of the spectrum and of the realisations of a few grids per
pipeline and kernel variant (grids from the lists of tests/test_gpu_fftgs.py), and of two co-simulation cases of
tests/test_gpu_fftgs_lmc.py.  Per grid: seeded noise into device and into host memory (the host destination with
GSS_OUT_CHUNK_MB=1, so that it spans several chunks of the output ring), supplied noise in device and in host memory, an
index view, and a count that crosses a batch boundary (67 = 64 + 3 on the grids whose realisations share launches).

One JSON line per case on stdout: {"case", "sha256", "arrays"}.  Two builds of the library compute the same bytes iff
their listings are equal line for line; GSS_LIB_PATH selects the build, and the GSS_FFTGS_* switches of INTEGRATION.md
select the code path (a GSS_FFTGS_PATH of the environment overrides the one a case would set):
    python tools/fftgs_bytes.py > new.jsonl;  GSS_LIB_PATH=<other libgss_hip.so> python tools/fftgs_bytes.py > other.jsonl
`--skip-large` leaves out the two grids that only the slab branches need."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

# (name, dims, GSS_FFTGS_PATH at create or None, large)
GRIDS = [
    ("generic 1-D 64", (64,), None, False),
    ("generic 2-D 100x100", (100, 100), None, False),
    ("generic 2-D long lines 64x2048", (64, 2048), None, False),
    ("generic 3-D 48x36x30", (48, 36, 30), None, False),
    ("generic 3-D slab 240x360x360", (240, 360, 360), None, True),
    ("fused l1=9 512x16x16", (512, 16, 16), "fused", False),
    ("fused x_rows=8 64x128x64", (64, 128, 64), "fused", False),
    ("fused x_rows=4 1024x32x16", (1024, 32, 16), "fused", False),
    ("fused 512-point lines 32x512x512", (32, 512, 512), "fused", True),
    ("rocfft odd 15x9", (15, 9), None, False),
    ("rocfft odd 51x47x23", (51, 47, 23), None, False),
]
ENV_PATH = os.environ.get("GSS_FFTGS_PATH")


def line(name, arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    print(json.dumps({"case": name, "sha256": h.hexdigest(), "arrays": len(arrays)}), flush=True)


def grid_cases(name, dims, path, large):
    import torch
    import gss
    from gss.engine import FFTGSHandle
    if ENV_PATH is None and path is not None:
        os.environ["GSS_FFTGS_PATH"] = path
    h = FFTGSHandle(gss.ExponentialVariogram(range=0.2 * dims[0] + 2.0, sill=1.4, nugget=0.05), dims, mean=0.3)
    if ENV_PATH is None:
        os.environ.pop("GSS_FFTGS_PATH", None)
    N = int(np.prod(dims))
    line(name + ": spectrum", [h.spectrum()])
    if large:
        line(name + ": seeded, device, 2", [h.realize(11, 3, 2, device=True)])
        h.close()
        return
    R = 67 if N <= 200000 else 3
    line(name + ": seeded, device, %d" % R, [h.realize(11, 2, R, device=True)])
    os.environ["GSS_OUT_CHUNK_MB"] = "1"
    line(name + ": seeded, host ring, %d" % R, [h.realize(11, 2, R)])
    del os.environ["GSS_OUT_CHUNK_MB"]
    noise = np.random.default_rng(N).uniform(size=(R, N))
    line(name + ": noise, device, %d" % R, [h.realize(0, 0, R, noise=torch.as_tensor(noise, device="cuda"))])
    line(name + ": noise, host, 3", [h.realize(0, 0, 3, noise=noise[:3])])
    inds = np.arange(3, N, 5)
    line(name + ": view, device, %d" % R, [h.realize(11, 2, R, inds=inds, device=True)])
    line(name + ": view, host, %d" % R, [h.realize(11, 2, R, inds=inds)])
    h.close()


def lmc_cases():
    import test_gpu_fftgs_lmc as T
    from gss.engine import FFTGSHandle
    for key in ("nz=3 full rank", "rank-1 b1, nz=3"):
        dims, b0, b1, means, kw = T.CASES[key]
        h = FFTGSHandle.lmc(T._structure(dims, **kw), b0, b1, means, dims)
        N = int(np.prod(dims))
        line("lmc %s: seeded, device, 5" % key, [h.realize_lmc(7, 1, 5, device=True)])
        line("lmc %s: seeded, host, 5" % key, [h.realize_lmc(7, 1, 5)])
        u = np.random.default_rng(1).uniform(size=(2, len(means), N))
        line("lmc %s: noise, host, 2" % key, [h.realize_lmc(7, 0, 2, noise=u)])
        line("lmc %s: view, device, 5" % key, [h.realize_lmc(7, 1, 5, inds=np.arange(1, N, 3), device=True)])
        h.close()


def main():
    skip_large = "--skip-large" in sys.argv
    for name, dims, path, large in GRIDS:
        if not (large and skip_large):
            grid_cases(name, dims, path, large)
    lmc_cases()


if __name__ == "__main__":
    main()
