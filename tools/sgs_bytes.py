#!/usr/bin/env python3
"""Fingerprint of what SGS returns: a SHA-256 over the realisations and the four weights() arrays (lists, counts,
weights, sigmas) of a set of small cases -- the CASES of tests/test_gpu_sgs.py and the cases of
test_more_than_64_neighbours with both mask readings, a 1-D grid with 70 neighbours, one visiting order per realisation
(7 and 80 neighbours), and a 33 x 21 grid (693 cells: no multiple of 64) over neighbour counts 1 ... 17 and realisation
counts 1 ... 130 with and without conditioning cells, drawn and supplied normals, into host and into device memory.

Every case runs under the three sweeps, GSS_SGS_LEVELS=0 / GSS_SGS_TEAM=0 / GSS_SGS_TEAM=1, one child process each (the
switches are read once per process).  One JSON line per case on stdout: {"case", "sha256": {hash: the settings that gave
it, joined by "="}}.  Two builds of the library compute the same bytes iff their listings are equal line for line;
GSS_LIB_PATH selects the build:
    python tools/sgs_bytes.py > new.jsonl;  GSS_LIB_PATH=<other libgss_hip.so> python tools/sgs_bytes.py > other.jsonl"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (("walk", {"GSS_SGS_LEVELS": "0"}), ("launches", {"GSS_SGS_TEAM": "0"}), ("team", {"GSS_SGS_TEAM": "1"}))


def sha(arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def cases():
    """(name, dims, variogram, mean, k, minneighbors, ball, ndata, order, mask_after, R, first_real, noise, device)
    order: None (row by row), "random", or (number of orders, path_base)."""
    import gss
    import test_gpu_sgs as T
    sph = gss.SphericalVariogram
    for after in (False, True):
        for i, (dims, vgspec, mean, k, nmin, ball, nd, rpath) in enumerate(T.CASES):
            yield ("case%d-after%d" % (i, after), dims, T._vg(vgspec[0], **vgspec[1])[0], mean, k, nmin, ball, nd,
                   "random" if rpath else None, after, 3, 3, False, False)
        for dims, k, rpath, nd in (((30, 20), 80, False, 5), ((14, 12, 6), 100, True, 0), ((40, 25), 200, True, 7),
                                   ((400,), 70, False, 5)):
            yield ("bigk-%s-k%d-after%d" % ("x".join(map(str, dims)), k, after), dims,
                   sph(range=0.4 * max(dims), sill=1.2, nugget=0.1), 0.3, k, 1, {}, nd, "random" if rpath else None, after,
                   3, 0, False, False)
    vg = sph(range=7.0, sill=1.3, nugget=0.05)
    yield ("orders-18x13-k7", (18, 13), vg, 0.4, 7, 1, {}, 9, (5, 4), False, 3, 5, False, False)
    yield ("orders-30x20-k80", (30, 20), vg, 0.4, 80, 1, {}, 5, (2, 0), True, 2, 0, False, False)
    vg = sph(range=12.0, nugget=0.05)
    shapes = [(5, R) for R in (1, 63, 64, 65, 130)] + [(k, 65) for k in (1, 3, 4, 8, 9, 17)]
    for k, R in shapes:
        for nd in (25, 0):
            for noise in (False, True):
                for device in (False, True):
                    yield ("33x21-k%d-R%d-nd%d-%s-%s" % (k, R, nd, "supplied" if noise else "drawn",
                                                         "device" if device else "host"),
                           (33, 21), vg, 0.3, k, 1, {}, nd, None, False, R, 2, noise, device)


def child(setting):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests")]
    import numpy as np
    from gss.engine import SGSHandle
    from oracle import fftgs as offt
    for name, dims, vg, mean, k, nmin, ball, nd, order, after, R, first, noise, device in cases():
        cent = offt.grid_centroids(dims)
        N = cent.shape[0]
        rng = np.random.default_rng(N + k)
        dl = np.sort(rng.choice(N, nd, replace=False)) if nd else None
        zd = rng.normal(size=nd) if nd else None
        if order == "random":
            path, base = rng.permutation(N), 0
        elif order is None:
            path, base = None, 0
        else:
            path, base = np.stack([rng.permutation(N) for _ in range(order[0])]), order[1]
        h = SGSHandle(vg, cent, path, dl, zd, mean, k, nmin, ball.get("radius"), ball.get("radii"), path_base=base,
                      mask_after_search=after)
        eps = rng.normal(size=(R, N)) if noise else None
        if noise and device:   # one memory space per call: the normals live where the realisations go
            import torch
            eps = torch.as_tensor(eps, device="cuda")
        z = h.realize(42, first, R, noise=eps, device=device)
        z = z.cpu().numpy() if device else z
        idx, nc, w, sg = h.weights()
        h.close()
        print(json.dumps({"case": name, setting: sha([z, idx, nc, w, sg])}), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    lines = {}   # case -> its line, in the order of cases()
    for setting, extra in SETTINGS:
        env = {k: v for k, v in os.environ.items() if k not in ("GSS_SGS_LEVELS", "GSS_SGS_TEAM")}
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting], check=True,
                             env=dict(env, **extra), timeout=900, stdout=subprocess.PIPE, text=True).stdout
        for d in map(json.loads, out.splitlines()):
            lines.setdefault(d["case"], {}).update(d)
    for case, d in lines.items():   # the settings that gave each hash: the three sweeps agree iff there is one entry
        by = {}
        for setting, _ in SETTINGS:
            by.setdefault(d[setting], []).append(setting)
        print(json.dumps({"case": case, "sha256": {h: "=".join(ss) for h, ss in by.items()}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
