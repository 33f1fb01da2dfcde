"""Stage A (the masked neighbour search, profile scope "sgs_search") of one gss_sgs_create: the SGS bench row
(512 x 512, k = 16, ball 30, 200 data, row order) and the 3-D row of tools/sgs_sizes.py (96^3, k = 16, random path).
One JSON line per case.  GSS_LIB_PATH selects another build of the library: python tools/sgs_search_time.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np, torch
import gss
from gss import _lib
from gss.engine import SGSHandle
from oracle import fftgs as offt
torch.cuda.set_device(0)
for name, dims, vg, k, rad, nd, order in (("sgs512x512", (512, 512), gss.SphericalVariogram(range=35.0), 16, 30.0, 200, "linear"),
                                          ("sgs96^3", (96, 96, 96), gss.SphericalVariogram(range=20.0), 16, 25.0, 50, "random")):
    cent = offt.grid_centroids(dims)
    N = cent.shape[0]
    rng = np.random.default_rng(5)
    dl = np.sort(rng.choice(N, nd, replace=False)); zd = rng.normal(size=nd)
    path = None if order == "linear" else rng.permutation(N)
    nw = 20000
    SGSHandle(vg, cent[:nw], None, dl[dl < nw], zd[dl < nw], 0.0, k, 1, rad).close()   # code objects loaded
    torch.cuda.synchronize()
    _lib.profile_reset(); _lib.profile_enable(True)
    h = SGSHandle(vg, cent, path, dl, zd, 0.0, k, 1, rad)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    print(json.dumps({"case": name, "sgs_search_ms": round(_lib.profile_read("sgs_search")[0], 3)}), flush=True)
    h.close()
