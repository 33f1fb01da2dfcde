"""The cases of tests/test_gpu_ik.py, shared with tools/ik_oracle.py (which measures the FP64 restatement against the
long-double one on exactly these inputs).  Every case is small: at most 400 samples and 203 domain points."""
import numpy as np

import gss


def _data(seed, n, dim, m=203):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 100.0, (n, dim))
    z = np.exp(rng.normal(size=n))                      # skewed
    x0 = rng.uniform(0.0, 100.0, (m, dim))              # 203: not a multiple of four
    return x, z, x0


def _cutoffs(z, K):
    """K increasing cutoffs that ARE sample values (a sample exactly on a cutoff counts as below it)."""
    s = np.unique(z)
    pos = np.linspace(0.08, 0.92, K) if K > 1 else np.array([0.5])
    return s[(pos * (s.size - 1)).astype(int)]


def _fstar(z, cut):
    return np.array([np.mean(z <= c) for c in cut])


def cases():
    out = {}
    kinds = [gss.ExponentialVariogram(range=30.0, sill=1.3, nugget=0.1), gss.SphericalVariogram(range=45.0),
             gss.MaternVariogram(range=35.0, order=1.5, nugget=0.05), gss.GaussianVariogram(range=12.0, nugget=0.02),
             gss.MaternVariogram(range=30.0, order=0.5), gss.MaternVariogram(range=30.0, order=2.5, nugget=0.1),
             gss.CubicVariogram(range=40.0, nugget=0.05)]
    # neighbour counts around the tile sizes, ragged counts from a ball, both dimensions, every compiled kind
    for i, k in enumerate((1, 15, 16, 17, 33, 64)):
        dim = 2 + (i % 2)
        x, z, x0 = _data(10 + i, 300, dim)
        cut = _cutoffs(z, 5)
        simple = i % 2 == 1
        out[f"k{k}"] = dict(x=x, z=z, x0=x0, cutoffs=cut, models=[kinds[i]], k=k, radius=22.0 if dim == 2 else 38.0,
                            fstar=_fstar(z, cut) if simple else None)
    # the last single-pass and the first two-pass count under each variant
    for K in (1, 2, 14, 15, 16):
        for simple in (False, True):
            x, z, x0 = _data(40 + K, 200, 2, m=101)
            cut = _cutoffs(z, K)
            out[f"K{K}_{'sk' if simple else 'ok'}"] = dict(x=x, z=z, x0=x0, cutoffs=cut, models=[kinds[K % 3]], k=17,
                                                          fstar=_fstar(z, cut) if simple else None)
    # every kind not yet met, 3-D, full neighbourhoods
    x, z, x0 = _data(70, 150, 3, m=61)
    for j, g in enumerate(kinds):
        cut = _cutoffs(z, 4)
        out[f"kind{j}"] = dict(x=x, z=z, x0=x0, cutoffs=cut, models=[g], k=20, fstar=None)
    # full form: three variograms of different kinds and ranges, one nested, one rotated
    x, z, x0 = _data(80, 250, 2, m=83)
    cut = _cutoffs(z, 3)
    nested = gss.NestedVariogram([(0.6, gss.ExponentialVariogram(range=20.0, nugget=0.1)),
                                  (0.4, gss.SphericalVariogram(range=60.0))])
    rotated = gss.ExponentialVariogram(gss.MetricBall((50.0, 15.0), 0.6), sill=0.9)
    for simple in (False, True):
        out[f"full_{'sk' if simple else 'ok'}"] = dict(x=x, z=z, x0=x0, cutoffs=cut, k=20,
                                                      models=[gss.SphericalVariogram(range=25.0), nested, rotated],
                                                      fstar=_fstar(z, cut) if simple else None)
    # all below the lowest cutoff (ones under the ordinary variant) and all above the highest (zeros)
    x, z, x0 = _data(90, 120, 2, m=41)
    out["all_below"] = dict(x=x, z=z, x0=x0, cutoffs=np.array([z.max() + 1.0, z.max() + 2.0]), models=[kinds[0]], k=12,
                            fstar=None)
    out["all_above"] = dict(x=x, z=z, x0=x0, cutoffs=np.array([z.min() - 2.0, z.min() - 1.0]), models=[kinds[0]], k=12,
                            fstar=None)
    # too few neighbours at some points
    out["missing"] = dict(x=x, z=z, x0=x0, cutoffs=_cutoffs(z, 3), models=[kinds[1]], k=8, radius=9.0, minneighbors=3,
                          fstar=None)
    # a duplicated location, unit sill and no nugget: the two copies are the two nearest neighbours of the points
    # beside them (the second pivot is 1 - 1 * 1, exactly zero) and are outside every other point's four nearest
    rng = np.random.default_rng(95)
    xs = rng.uniform(0.0, 50.0, (60, 2))
    xs[1] = xs[0] = np.array([90.0, 90.0])
    zs = np.exp(rng.normal(size=60))
    near = np.array([90.0, 90.0]) + rng.uniform(-0.5, 0.5, (6, 2))
    far = rng.uniform(5.0, 45.0, (31, 2))
    out["duplicate"] = dict(x=xs, z=zs, x0=np.vstack([near, far]), cutoffs=_cutoffs(zs, 3), k=4,
                            models=[gss.ExponentialVariogram(range=20.0)], fstar=None)
    # built to violate the order relations: clusters under a Gaussian model with a small nugget, so that screening
    # produces negative weights
    rng = np.random.default_rng(7)
    cen = rng.uniform(10.0, 90.0, (25, 2))
    xc = (cen[:, None, :] + rng.normal(scale=1.5, size=(25, 8, 2))).reshape(-1, 2)
    zc = np.exp(rng.normal(size=xc.shape[0]))
    out["order"] = dict(x=xc, z=zc, x0=rng.uniform(5.0, 95.0, (203, 2)), cutoffs=_cutoffs(zc, 6), k=16,
                        models=[gss.GaussianVariogram(range=25.0, nugget=0.001)], fstar=None)
    # the second B tile and the loop of the full form on one tile and on four (k = 12, 40), and the 1-D dispatch
    x, z, x0 = _data(85, 200, 2, m=67)
    cut16, cut3 = _cutoffs(z, 16), _cutoffs(z, 3)
    full3 = [gss.SphericalVariogram(range=25.0), nested, gss.MaternVariogram(range=30.0, order=1.5, nugget=0.05)]
    for k in (12, 40):
        for simple in (False, True):
            tag = "sk" if simple else "ok"
            out[f"K16_{tag}_k{k}"] = dict(x=x, z=z, x0=x0, cutoffs=cut16, models=[kinds[0]], k=k,
                                          fstar=_fstar(z, cut16) if simple else None)
            out[f"full_{tag}_k{k}"] = dict(x=x, z=z, x0=x0, cutoffs=cut3, models=full3, k=k,
                                           fstar=_fstar(z, cut3) if simple else None)
    x, z, x0 = _data(86, 120, 1, m=45)
    x = np.round(x, 1) + np.arange(120)[:, None] * 1e-3          # (no near-coincident samples on the line)
    out["dim1"] = dict(x=x, z=z, x0=x0, cutoffs=_cutoffs(z, 15), models=[kinds[0]], k=20, fstar=None)
    out["dim1_full"] = dict(x=x, z=z, x0=x0, cutoffs=_cutoffs(z, 2), k=10, fstar=None,
                            models=[gss.ExponentialVariogram(range=20.0, nugget=0.1), gss.SphericalVariogram(range=30.0)])
    # every sample a neighbour (k = n <= 64): the system the global-neighbourhood route solves
    rng = np.random.default_rng(11)
    xr = rng.uniform(0.0, 30.0, (48, 2))
    zr = np.exp(rng.normal(size=48))
    cut = np.quantile(zr, [0.25, 0.5, 0.75])
    for simple in (False, True):
        out[f"route_{'sk' if simple else 'ok'}"] = dict(x=xr, z=zr, x0=rng.uniform(0.0, 30.0, (57, 2)), cutoffs=cut, k=48,
                                                       models=[gss.ExponentialVariogram(range=10.0, nugget=0.1)],
                                                       fstar=_fstar(zr, cut) if simple else None)
    out["route_full"] = dict(out["route_sk"], models=[gss.ExponentialVariogram(range=10.0, nugget=0.1),
                                                      gss.SphericalVariogram(range=14.0, nugget=0.05),
                                                      gss.MaternVariogram(range=12.0, order=1.5, nugget=0.1)])
    return out


POST_TAILS = ((1.0, 1.0), (2.5, 2.5), (1.0, 2.5))


def post_args_for(c):
    """How the corrected ccdf of a case is post-processed: zmin / zmax around its cutoffs, a threshold on the lowest
    cutoff, one inside the classes and one in the upper tail, three probabilities."""
    cut = c["cutoffs"]
    zmin = float(cut[0]) - 1.0
    zmax = max(float(c["z"].max()), float(cut[-1])) * 1.5 + 1.0
    return dict(zmin=zmin, zmax=zmax, thresholds=(float(cut[0]), 0.5 * float(cut[0] + cut[-1]), zmax * 0.9),
                probs=(0.1, 0.5, 0.9))


def post_rows():
    """Hand-made corrected rows for gss_ik_post: zero-probability classes, F_0 = 0, F_{K-1} = 1, a NaN row."""
    return np.array([[0.1, 0.3, 0.3, 0.8], [0.0, 0.0, 0.5, 1.0], [0.0, 0.2, 0.2, 0.2], [1.0, 1.0, 1.0, 1.0],
                     [0.0, 0.0, 0.0, 0.0], [0.25, 0.5, 0.75, 1.0], [np.nan, np.nan, np.nan, np.nan],
                     [0.05, 0.05, 0.95, 0.95]])


POST_CUTOFFS = np.array([0.5, 1.0, 2.5, 6.0])
POST_ARGS = dict(zmin=0.0, zmax=30.0, thresholds=(0.0, 0.25, 0.5, 1.7, 2.5, 6.0, 11.0, 30.0),
                 probs=(0.01, 0.05, 0.25, 0.3, 0.5, 0.8, 0.95, 0.999))
