"""Recorder and cases that pin the Python binding call for call (tests/test_engine_calls.py).

`record(fn)` runs `fn` against a stand-in for libgss_hip.so: every `gss_*` call is written down -- scalars by value,
arrays by dtype, shape, memory space and (for the `const` pointers of include/gss.h) contents, variogram structures
field by field -- and answers 0.  No kernel runs.  Only names that gss._lib has always had are touched (`lib`, `load`,
`ptr`, `current_stream`), so the file replays on any commit of the binding.

`python tests/engine_calls.py` rewrites tests/golden/engine_calls.json from the host forms of the cases.
"""
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_calls.json")
for _p in (ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FAKE_HANDLE = 0x1000


# ---- include/gss.h: parameter names, and which pointers are inputs (const) ------------------------------------
def _header_params():
    src = open(os.path.join(ROOT, "include", "gss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint32_t\s+(gss_[a-z0-9_]+)\s*\(([^)]*)\)", src):
        ps = []
        for p in params.split(","):
            p = " ".join(p.split())
            if p in ("", "void"):
                continue
            ps.append((re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1], "*" in p and p.startswith("const")))
        out[name] = ps
    return out


PARAMS = _header_params()


# ---- values -> JSON ---------------------------------------------------------------------------------------------
def _num(v):
    """JSON has no NaN / inf that compare equal: they travel as strings."""
    if isinstance(v, float) and not math.isfinite(v):
        return repr(v)
    return v


def _nums(v):
    return [_nums(e) for e in v] if isinstance(v, list) else _num(v)


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _array(a, contents):
    if _is_tensor(a):
        d = {"kind": "torch", "mem": "device" if a.is_cuda else "host", "dtype": str(a.dtype).replace("torch.", ""),
             "shape": list(a.shape)}
        if contents:
            d["data"] = _nums(a.detach().cpu().tolist())
        return d
    d = {"kind": "numpy", "mem": "host", "dtype": str(a.dtype), "shape": list(a.shape)}
    if contents:
        d["data"] = _nums(a.tolist())
    return d


def _ctypes(o):
    if isinstance(o, C.Structure):
        return {f: _ctypes(getattr(o, f)) for f, _ in o._fields_}
    if isinstance(o, C.Array):
        return [_ctypes(e) for e in o]
    return _num(o)


class _Ptr:
    """What the wrapped `ptr` hands to the stand-in library: the array itself."""

    def __init__(self, a):
        self.a = a


def _arg(v, const):
    if v is None:
        return None
    if isinstance(v, _Ptr):
        return _array(v.a, const)
    if isinstance(v, bool):
        return ["bool", v]
    if isinstance(v, (int, np.integer)):
        return ["int", int(v)]
    if isinstance(v, (float, np.floating)):
        return ["float", _num(float(v))]
    if isinstance(v, (C.Structure, C.Array)):
        return ["ctypes", type(v).__name__, _ctypes(v)]
    if isinstance(v, C.c_void_p):
        return ["void*", "null" if not v.value else "set"]
    if hasattr(v, "_obj"):                                   # C.byref(...)
        o = v._obj
        return ["byref", type(o).__name__, _ctypes(o) if isinstance(o, C.Structure) else None]
    if isinstance(v, bytes):
        return ["bytes", len(v)]
    raise TypeError(f"recorder: unexpected argument {v!r}")


def describe(r):
    """The shape of what a method returned: (type, dtype, shape) of arrays, the types of everything else."""
    if isinstance(r, (tuple, list)):
        return [type(r).__name__] + [describe(e) for e in r]
    if isinstance(r, dict):
        return ["dict"] + [[k, describe(v)] for k, v in r.items()]
    if _is_tensor(r):
        return ["tensor", str(r.dtype).replace("torch.", ""), list(r.shape), "device" if r.is_cuda else "host"]
    if isinstance(r, np.ndarray):
        return ["ndarray", str(r.dtype), list(r.shape), "host"]
    return [type(r).__name__]


# ---- the stand-in library -----------------------------------------------------------------------------------------
class FakeLib:
    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        if not name.startswith("gss_"):
            raise AttributeError(name)
        params = PARAMS.get(name, [])

        def call(*args):
            rec = []
            for i, v in enumerate(args):
                pname, const = params[i] if i < len(params) else (f"arg{i}", False)
                rec.append([pname, "stream" if pname == "stream" else _arg(v, const)])
                if isinstance(v, _Ptr) and not const and isinstance(v.a, np.ndarray) and v.a.flags.writeable:
                    # host outputs get a fixed filling, so that host code that reads them (lwr_callable reads the
                    # neighbour lists of its own search) runs the same way every time
                    v.a[...] = (np.arange(v.a.size) % 3).reshape(v.a.shape) if v.a.dtype == np.int32 else 0
                if "_create" in name and hasattr(v, "_obj") and isinstance(v._obj, C.c_void_p):
                    v._obj.value = FAKE_HANDLE
            self._calls.append([name, rec])
            return 0
        return call


def record(fn):
    """Run `fn()` against the stand-in library -> {"calls": [...], "returned": ... | "raised": [type, message]}."""
    from gss import _lib
    calls = []
    fake = FakeLib(calls)
    real_ptr = _lib.ptr
    users = [m for n, m in list(sys.modules.items()) if n.split(".")[0] == "gss" and getattr(m, "ptr", None) is real_ptr]
    saved = (_lib.lib, _lib.load)

    def ptr(x):
        return None if x is None else _Ptr(x)
    _lib.lib = _lib.load = lambda: fake
    for m in users:
        m.ptr = ptr
    try:
        try:
            out = {"returned": describe(fn())}
        except Exception as e:       # noqa: BLE001 -- the refusals are part of what is pinned
            out = {"raised": [type(e).__name__, str(e)]}
    finally:
        _lib.lib, _lib.load = saved
        for m in users:
            m.ptr = real_ptr
    out["calls"] = calls
    return out


# ---- inputs: exact binary fractions, n = 7 samples, m = 5 centres, k = 3, nz = 2, K = 3 cutoffs --------------------
N, M, K, NZ, NCUT = 7, 5, 3, 2, 3


def X(d, n=N):
    return ((np.arange(n * d) * 37 % 101) / 8.0).reshape(n, d)


def C0(d, m=M):
    return ((np.arange(m * d) * 53 % 89) / 4.0 + 0.5).reshape(m, d)


Z = (np.arange(N) * 29 % 17) / 4.0 - 1.0
Z2 = np.stack([Z, Z[::-1] * 0.5])
FOLD = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.int64)
VAR = np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.int64)
RADII = (2.0, 4.0, 8.0)
ROT = {2: ((0.6, -0.8), (0.8, 0.6)), 3: ((0.6, -0.8, 0.0), (0.8, 0.6, 0.0), (0.0, 0.0, 1.0))}
DISTANCES = ["euclidean", "cityblock", "chebyshev", ("haversine", 6371.0)]


def searches(d, distance=True):
    """(name, keyword arguments) of every search form in d dimensions."""
    out = [("none", {}), ("radius", dict(radius=2.5)), ("radii", dict(radii=RADII[:d]))]
    if d > 1:
        out.append(("rotated", dict(radii=RADII[:d], rotation=ROT[d])))
    if distance:
        for dist in DISTANCES:
            if not isinstance(dist, str) and d != 2:
                continue                                     # (longitude, latitude)
            out.append((dist if isinstance(dist, str) else dist[0], dict(distance=dist)))
    return out


def bad_searches(d=2, distance=True):
    out = [("rotation_without_radii", dict(rotation=ROT[d]))]
    if distance:
        out += [("ball_cityblock", dict(radii=RADII[:d], rotation=ROT[d], distance="cityblock")),
                ("haversine_zero", dict(distance=("haversine", 0))),
                ("unknown_distance", dict(distance="minkowski")),
                ("bad_distance_before_bad_rotation", dict(rotation=ROT[d], distance="minkowski"))]
    return out


class Ctx:
    """What a case sees: `T(a)` puts an array where the form under test wants it (numpy, or a CUDA tensor), `dev` is
    the `device=` argument."""

    def __init__(self, dev):
        self.dev = dev

    def T(self, a):
        if a is None or not self.dev:
            return a
        import torch
        return torch.as_tensor(np.asarray(a), device="cuda")


def _vg(d=None, aniso=False):
    import gss
    if aniso:
        return gss.SphericalVariogram(gss.MetricBall(RADII[:d], ROT.get(d)), sill=2.0, nugget=0.25)
    return gss.ExponentialVariogram(range=3.0, sill=1.5, nugget=0.125)


def _krig(d, **kw):
    from gss.engine import KrigHandle, OK
    return KrigHandle(_vg(), OK, X(d), Z, **kw)


def _cokrig(d, factor=True):
    from gss.engine import CoKrigHandle, OK
    return CoKrigHandle(_vg(), [[0.25, 0.0], [0.0, 0.5]], [[1.0, 0.5], [0.5, 2.0]], OK, X(d), Z, VAR, factor=factor)


def cases():
    """[(id, host_only, fn(ctx))]: every method of the handles and of HipEngine that calls the library."""
    from gss import engine as E
    H = E.HipEngine
    out = []

    def add(name, fn, host_only=False):
        out.append((name, host_only, fn))

    def closing(make, use):
        def fn(c):
            h = make()
            try:
                return use(h, c)
            finally:
                h.close()
        return fn

    flat = X(1).ravel()
    # -- the moving-neighbourhood entry points x every search form ----------------------------------------------
    for d in (1, 2, 3):
        for ok, forms in ((True, searches(d)), (False, bad_searches(d) if d > 1 else [])):
            for sname, s in forms:
                tag = f"d{d}-{sname}"
                add(f"krig.predict_knn[{tag}]", closing(lambda d=d: _krig(d, factor=False),
                    lambda h, c, d=d, s=s: h.predict_knn(c.T(C0(d)), K, **s)))
                add(f"krig.cv_knn[{tag}]", closing(lambda d=d: _krig(d, factor=False),
                    lambda h, c, s=s: h.cv_knn(K, device=c.dev, **s)))
                add(f"sgs.create[{tag}]", closing(
                    lambda d=d, s=s: E.SGSHandle(_vg(), X(d), None, [1, 4], [0.5, -0.5], maxneighbors=K, **s),
                    lambda h, c: None), host_only=True)
                add(f"ik_predict_knn[{tag}]", lambda c, d=d, s=s: H.ik_predict_knn(
                    X(d), Z, c.T(C0(d)), [-0.5, 0.5, 1.5], _vg(), K, **s))
                add(f"knn_search[{tag}]", lambda c, d=d, s=s: H.knn_search(c.T(X(d)), c.T(C0(d)), K, **s))
                add(f"idw[{tag}]", lambda c, d=d, s=s: H.idw(X(d), Z, c.T(C0(d)), K, **s))
                add(f"lwr[{tag}]", lambda c, d=d, s=s: H.lwr(c.T(X(d)), c.T(Z), c.T(C0(d)), K, **s))
                add(f"idw_cv[{tag}]", lambda c, d=d, s=s: H.idw_cv(c.T(X(d)), c.T(Z), K, device=c.dev, **s))
                add(f"lwr_cv[{tag}]", lambda c, d=d, s=s: H.lwr_cv(c.T(X(d)), c.T(Z), K, device=c.dev, **s))
                add(f"lwr_callable[{tag}]", lambda c, d=d, s=s: H.lwr_callable(
                    X(d), Z, C0(d), K, 1, lambda t: (1.0 - t) ** 2, **s), host_only=True)
        for ok, forms in ((True, searches(d, False)), (False, bad_searches(d, False) if d > 1 else [])):
            for sname, s in forms:                           # cokriging takes no distance
                tag = f"d{d}-{sname}"
                add(f"cokrig.predict_knn[{tag}]", closing(lambda d=d: _cokrig(d, factor=False),
                    lambda h, c, d=d, s=s: h.predict_knn(c.T(C0(d)), [2, 1], **s)))
                add(f"cokrig.cv_knn[{tag}]", closing(lambda d=d: _cokrig(d, factor=False),
                    lambda h, c, s=s: h.cv_knn([2, 1], device=c.dev, **s)))
    # -- options: folds, lists, value columns, flat 1-D input -----------------------------------------------------
    d = 2
    for fold in (None, FOLD):
        for ri in (False, True):
            tag = f"fold{int(fold is not None)}-idx{int(ri)}"
            add(f"krig.cv_knn[{tag}]", closing(lambda: _krig(d, factor=False), lambda h, c, f=fold, ri=ri: h.cv_knn(
                K, fold=c.T(f), exclude_radius=1.5, minneighbors=2, return_idx=ri, device=c.dev)))
            add(f"cokrig.cv_knn[{tag}]", closing(lambda: _cokrig(d, factor=False), lambda h, c, f=fold, ri=ri: h.cv_knn(
                [2, 1], fold=c.T(f), exclude_radius=1.5, minneighbors=2, return_idx=ri, device=c.dev)))
            add(f"cokrig.cv_knn_scalar_k[{tag}]", closing(lambda: _cokrig(d, factor=False),
                lambda h, c, f=fold, ri=ri: h.cv_knn(K, fold=c.T(f), return_idx=ri, radii=RADII[:2], rotation=ROT[2],
                                                     device=c.dev)))
            for zname, z in (("z1", Z), ("z2", Z2)):
                add(f"idw_cv[{tag}-{zname}]", lambda c, f=fold, ri=ri, z=z: H.idw_cv(
                    c.T(X(d)), c.T(z), K, fold=c.T(f), exclude_radius=1.5, minneighbors=2, exponent=2.0, return_idx=ri,
                    device=c.dev))
                add(f"lwr_cv[{tag}-{zname}]", lambda c, f=fold, ri=ri, z=z: H.lwr_cv(
                    c.T(X(d)), c.T(z), K, fold=c.T(f), weight=(1, 2.0, 3.0), return_idx=ri, device=c.dev))
        add(f"krig.cv_global_folds[fold{int(fold is not None)}]", closing(lambda: _krig(d),
            lambda h, c, f=fold: h.cv_global_folds(c.T(f), device=c.dev)))
    for ri in (False, True):
        add(f"krig.predict_knn[idx{int(ri)}]", closing(lambda: _krig(d, factor=False),
            lambda h, c, ri=ri: h.predict_knn(c.T(C0(d)), K, minneighbors=2, return_idx=ri)))
        add(f"cokrig.predict_knn[idx{int(ri)}]", closing(lambda: _cokrig(d, factor=False),
            lambda h, c, ri=ri: h.predict_knn(c.T(C0(d)), 2, minneighbors=2, return_idx=ri)))
        for raw in (False, True):
            add(f"ik_predict_knn[idx{int(ri)}-raw{int(raw)}]", lambda c, ri=ri, raw=raw: H.ik_predict_knn(
                c.T(X(d)), c.T(Z), c.T(C0(d)), [-0.5, 0.5, 1.5], [_vg(), _vg(2, True), _vg()], K, minneighbors=2,
                fstar=[0.25, 0.5, 0.75], return_raw=raw, return_idx=ri))
    for zname, z in (("z1", Z), ("z2", Z2)):
        add(f"idw[{zname}]", lambda c, z=z: H.idw(c.T(X(d)), c.T(z), c.T(C0(d)), K, minneighbors=2, exponent=2.0))
        add(f"lwr[{zname}]", lambda c, z=z: H.lwr(X(d), z, c.T(C0(d)), K, weight=(1, 2.0, 3.0)))
    add("krig.create[flat]", closing(lambda: E.KrigHandle(_vg(), E.SK, flat, Z, mean=0.5), lambda h, c: None), True)
    add("krig.predict_knn[flat]", closing(lambda: E.KrigHandle(_vg(), E.OK, flat, Z, factor=False),
        lambda h, c: h.predict_knn(c.T(C0(1)), K)))
    add("cokrig.create[flat]", closing(lambda: E.CoKrigHandle(_vg(), 0.25, 1.0, E.SK, flat, Z, np.zeros(N), means=0.5),
                                       lambda h, c: None), True)
    add("sgs.create[flat]", closing(lambda: E.SGSHandle(_vg(), flat, None, None, None), lambda h, c: None), True)
    add("lugs.create[flat]", closing(lambda: E.LUGSHandle(_vg(), flat, [1, 4], [0.5, -0.5]), lambda h, c: None), True)
    add("ik_predict_knn[flat]", lambda c: H.ik_predict_knn(flat, Z, c.T(C0(1).ravel()), [0.5], _vg(), K))
    add("knn_search[flat]", lambda c: H.knn_search(c.T(flat), c.T(C0(1).ravel()), K))
    add("idw[flat]", lambda c: H.idw(flat, Z, c.T(C0(1).ravel()), K))
    add("idw_cv[flat]", lambda c: H.idw_cv(c.T(flat), c.T(Z), K, device=c.dev))
    add("lwr_callable[flat]", lambda c: H.lwr_callable(flat, Z, C0(1).ravel(), K, 1, lambda t: 1.0 - t), True)
    add("cov_pairwise[flat]", lambda c: H.cov_pairwise(_vg(), flat, C0(1).ravel()), True)
    add("variogram_empirical[flat]", lambda c: H.variogram_empirical(c.T(flat), c.T(Z), 4, 6.0))
    add("decluster_cell_counts[flat]", lambda c: H.decluster_cell_counts(c.T(flat), [0.0], [2.0]))
    # -- the remaining refusals --------------------------------------------------------------------------------------
    for name, f in (("host_fold_device", FOLD), ("short_fold", FOLD[:5])):
        devkw = dict(device=True) if name == "host_fold_device" else {}
        add(f"krig.cv_knn[{name}]", closing(lambda: _krig(d, factor=False),
            lambda h, c, f=f, kw=devkw: h.cv_knn(K, fold=f if kw else c.T(f), **kw)), bool(devkw))
        add(f"krig.cv_global_folds[{name}]", closing(lambda: _krig(d),
            lambda h, c, f=f, kw=devkw: h.cv_global_folds(f if kw else c.T(f), **kw)), bool(devkw))
        add(f"cokrig.cv_knn[{name}]", closing(lambda: _cokrig(d, factor=False),
            lambda h, c, f=f, kw=devkw: h.cv_knn([2, 1], fold=f if kw else c.T(f), **kw)), bool(devkw))
        add(f"idw_cv[{name}]", lambda c, f=f, kw=devkw: H.idw_cv(c.T(X(d)), c.T(Z), K, fold=f if kw else c.T(f), **kw),
            bool(devkw))
    add("cokrig.cv_knn[k_wrong_length]", closing(lambda: _cokrig(d, factor=False),
                                                 lambda h, c: h.cv_knn([2, 1, 1], device=c.dev)))
    add("idw_cv[idx_with_k_n]", lambda c: H.idw_cv(c.T(X(d)), c.T(Z), N, return_idx=True, device=c.dev))
    add("lwr_cv[z_wrong_shape]", lambda c: H.lwr_cv(c.T(X(d)), c.T(Z[:5]), K, device=c.dev))
    add("idw[z_wrong_shape]", lambda c: H.idw(X(d), Z[:5], c.T(C0(d)), K))
    add("ik_predict_knn[fstar_wrong_length]", lambda c: H.ik_predict_knn(
        X(d), Z, c.T(C0(d)), [-0.5, 0.5, 1.5], _vg(), K, fstar=[0.25, 0.75]))
    add("ik_predict_knn[z_wrong_shape]", lambda c: H.ik_predict_knn(X(d), Z2, c.T(C0(d)), [0.5], _vg(), K))
    add("variogram_empirical[direction_wrong_size]", lambda c: H.variogram_empirical(
        c.T(X(d)), c.T(Z), 4, 6.0, direction=[1.0, 0.0, 0.0]))
    add("variogram_cross[direction_wrong_size]", lambda c: H.variogram_cross(
        c.T(X(d)), c.T(Z2), 4, 6.0, direction=[1.0]))
    add("variogram_empirical[cityblock]", lambda c: H.variogram_empirical(c.T(X(d)), c.T(Z), 4, 6.0, distance="cityblock"))
    add("variogram_empirical[mixed_spaces]", lambda c: H.variogram_empirical(c.T(X(d)), Z, 4, 6.0))
    add("knn_search[mixed_spaces]", lambda c: H.knn_search(c.T(X(d)), C0(d), K))
    # -- kriging handles: every other method -------------------------------------------------------------------------
    for dd in (1, 2, 3):
        add(f"krig.predict_global[d{dd}]", closing(lambda dd=dd: _krig(dd), lambda h, c, dd=dd: h.predict_global(c.T(C0(dd)))))
    add("krig.create[uk]", closing(lambda: E.KrigHandle(_vg(2, True), E.UK, X(2), Z, degree=1, async_fit=True),
                                   lambda h, c: None), True)
    add("krig.create[power]", closing(lambda: E.KrigHandle(__import__("gss").PowerVariogram(scaling=2.0, exponent=1.5),
                                                           E.OK, X(3), Z), lambda h, c: None), True)
    add("krig.create[nested]", closing(lambda: E.KrigHandle(
        0.5 * _vg() + 2.0 * __import__("gss").GaussianVariogram(range=5.0, nugget=0.125), E.OK, X(3), Z),
        lambda h, c: None), True)
    add("krig.predict_global[edk]", closing(lambda: E.KrigHandle(_vg(), E.EDK, X(2), Z, drift_data=X(2)[:, 0] * 2.0),
        lambda h, c: h.predict_global(c.T(C0(2)), drift_dom=c.T(C0(2)[:, :1] * 2.0))))
    add("krig.predict_knn[edk]", closing(
        lambda: E.KrigHandle(_vg(), E.EDK, X(2), Z, drift_data=X(2)[:, 0] * 2.0, factor=False),
        lambda h, c: h.predict_knn(c.T(C0(2)), K, drift_dom=c.T(C0(2)[:, :1] * 2.0))))
    add("krig.predict_global_batch", closing(lambda: _krig(2), lambda h, c: h.predict_global_batch(c.T(C0(2)), c.T(Z2))))
    add("krig.predict_global_batch[mixed_spaces]", closing(lambda: _krig(2),
        lambda h, c: h.predict_global_batch(c.T(C0(2)), __import__("torch").as_tensor(Z2))))
    add("krig.cv_global", closing(lambda: _krig(2), lambda h, c: h.cv_global(device=c.dev)))
    add("krig.set_block_support", closing(lambda: _krig(2), lambda h, c: (h.set_block_support(0.5, 3),
                                                                            h.set_block_support(None, 0))), True)
    add("krig.adopt_factor", closing(lambda: _krig(2, factor=False), lambda h, c: h.adopt_factor()), True)
    add("krig.state_routes", closing(lambda: _krig(2), lambda h, c: (h.bcast_state(1), len(h.export_state()),
                                                                     h.import_state(bytes(96)))), True)
    add("cokrig.create[factor]", closing(lambda: _cokrig(2), lambda h, c: None), True)
    add("cokrig.via_engine", closing(lambda: H.cokrig(_vg(), [[0.25, 0.0], [0.0, 0.5]], [[1.0, 0.5], [0.5, 2.0]], E.SK,
                                                      X(2), Z, VAR, means=[0.5, 1.5], async_fit=True),
                                     lambda h, c: None), True)
    add("cokrig.predict_global", closing(lambda: _cokrig(2), lambda h, c: h.predict_global(c.T(C0(2)))))
    add("cokrig.predict_batch", closing(lambda: _cokrig(2), lambda h, c: h.predict_batch(c.T(C0(2)), c.T(Z2))))
    add("cokrig.predict_batch[one_vector]", closing(lambda: _cokrig(2), lambda h, c: h.predict_batch(c.T(C0(2)), c.T(Z))))
    add("cokrig.cv_global_folds", closing(lambda: _cokrig(2), lambda h, c: h.cv_global_folds(c.T(FOLD), device=c.dev)))
    # -- simulation handles ----------------------------------------------------------------------------------------
    fft = lambda: E.FFTGSHandle(_vg(2, True), (4, 3), spacing=(1.0, 2.0), mean=0.5)            # noqa: E731
    add("fftgs.spectrum", closing(fft, lambda h, c: h.spectrum()), True)
    add("fftgs.create[no_spectrum]", closing(lambda: E.FFTGSHandle(_vg(), (4, 3, 2), spectrum=False),
                                             lambda h, c: h.adopt_state()), True)
    add("fftgs.realize", closing(fft, lambda h, c: h.realize(3, 1, 2, device=c.dev)))
    add("fftgs.realize[noise_inds]", closing(fft, lambda h, c: h.realize(
        3, 1, 2, noise=c.T(np.arange(24.0).reshape(2, 12) / 32.0), inds=[0, 5, 7])))
    add("fftgs.realize[out]", closing(fft, lambda h, c: h.realize(3, 1, 2, out=c.T(np.zeros((2, 12))))))
    add("fftgs.realize[noise_elsewhere]", closing(fft, lambda h, c: h.realize(
        3, 1, 2, noise=__import__("torch").zeros(2, 12, dtype=__import__("torch").float64), out=c.T(np.zeros((2, 12))))))
    lmc = lambda: E.FFTGSHandle.lmc(_vg(), [[0.25, 0.0], [0.0, 0.5]], [[1.0, 0.5], [0.5, 2.0]], [0.5, 1.5], (4, 3))  # noqa: E731
    add("fftgs_lmc.realize", closing(lmc, lambda h, c: h.realize_lmc(3, 1, 2, device=c.dev)))
    add("fftgs_lmc.realize[noise_inds]", closing(lmc, lambda h, c: h.realize_lmc(
        3, 1, 2, noise=c.T(np.arange(48.0).reshape(2, 2, 12) / 64.0), nugget_noise=c.T(np.ones((2, 2, 12))),
        inds=[0, 5, 7])))
    add("fftgs_lmc.realize[noise_wrong_shape]", closing(lmc, lambda h, c: h.realize_lmc(
        3, 1, 2, noise=c.T(np.zeros((2, 12))))))
    add("fftgs_lmc.via_engine", closing(lambda: H.FFTGS_LMC(_vg(), 0.25, 1.0, None, (4,), spectrum=False),
                                        lambda h, c: None), True)
    lugs = lambda **kw: E.LUGSHandle(_vg(), X(2), [1, 4], [0.5, -0.5], mean=0.5, **kw)           # noqa: E731
    add("lugs.factor", closing(lugs, lambda h, c: h.factor()), True)
    add("lugs.create[lu_no_factor]", closing(lambda: lugs(factor=False, factorization="lu"),
                                             lambda h, c: h.adopt_state()), True)
    add("lugs.create[bad_factorization]", lambda c: lugs(factorization="qr"), True)
    add("lugs.realize", closing(lugs, lambda h, c: h.realize(3, 1, 2, device=c.dev)))
    add("lugs.realize[noise_w1]", closing(lugs, lambda h, c: h.realize(
        3, 1, 2, noise=c.T(np.arange(10.0).reshape(2, 5) / 16.0), rho=0.5, w1=c.T(np.ones((2, 5))))))
    sgs = lambda **kw: E.SGSHandle(_vg(), X(2), kw.pop("path", None), [1, 4], [0.5, -0.5], mean=0.5, maxneighbors=K,  # noqa: E731
                                   **kw)
    add("sgs.weights_schedule", closing(sgs, lambda h, c: (h.weights(), h.schedule())), True)
    add("sgs.create[paths]", closing(lambda: sgs(path=np.stack([np.arange(N), np.arange(N)[::-1]]), path_base=2,
                                                 minneighbors=2, mask_after_search=True, distance="chebyshev"),
                                     lambda h, c: None), True)
    add("sgs.create[paths_wrong_length]", lambda c: sgs(path=np.zeros((2, 5))), True)
    add("sgs.realize", closing(sgs, lambda h, c: h.realize(3, 1, 2, device=c.dev)))
    add("sgs.realize[noise_out]", closing(sgs, lambda h, c: h.realize(
        3, 1, 2, noise=c.T(np.arange(14.0).reshape(2, 7) / 16.0), out=c.T(np.zeros((2, 7))))))
    add("sgs.realize[out_wrong_shape]", closing(sgs, lambda h, c: h.realize(3, 1, 2, out=c.T(np.zeros((2, 5))))))
    # -- normal scores -------------------------------------------------------------------------------------------------
    ns = lambda: H.nscore(Z, weights=np.arange(1.0, 8.0), tails=(-2.0, None), tail_power=(1.5, 2.0))   # noqa: E731
    add("nscore.table", closing(ns, lambda h, c: h.table()), True)
    add("nscore.create[plain]", closing(lambda: E.NScoreHandle(Z2), lambda h, c: None), True)
    add("nscore.create[weights_wrong_length]", lambda c: E.NScoreHandle(Z, weights=[1.0, 2.0]), True)
    add("nscore.forward", closing(ns, lambda h, c: h.forward(c.T(Z2))))
    add("nscore.inverse[strided]", closing(ns, lambda h, c: h.inverse(c.T(np.arange(24.0).reshape(2, 3, 4))[:, 1])))
    add("nscore.forward[in_place]", closing(ns, lambda h, c: (lambda x: h.forward(x, out=x))(c.T(Z2.copy()))))
    add("nscore.forward[out_other_runs]", closing(ns, lambda h, c: h.forward(
        c.T(Z2), out=c.T(np.zeros((2, 2 * N)))[:, ::2])))
    add("nscore.forward[float32]", closing(ns, lambda h, c: h.forward(c.T(Z2.astype(np.float32)))))
    add("nscore.forward[out_wrong_shape]", closing(ns, lambda h, c: h.forward(c.T(Z2), out=c.T(np.zeros(3)))))
    # -- indicator post-processing, covariances, variography, declustering, summaries ----------------------------------
    ccdf = np.array([[0.25, 0.5, 0.75], [0.5, 0.25, 1.0]])
    add("ik_order_relations", lambda c: H.ik_order_relations(c.T(ccdf.copy())))
    add("ik_order_relations[vector]", lambda c: H.ik_order_relations(c.T(ccdf[0].copy())))
    add("ik_post", lambda c: H.ik_post(c.T(ccdf), [-0.5, 0.5, 1.5], -2.0, 3.0, tail_power=(1.5, 2.0), thresholds=[0.0, 1.0],
                                       probs=[0.25, 0.5, 0.75]))
    add("ik_post[moments_only]", lambda c: H.ik_post(c.T(ccdf), [-0.5, 0.5, 1.5], -2.0, 3.0))
    add("ik_post[no_moments]", lambda c: H.ik_post(c.T(ccdf), [-0.5, 0.5, 1.5], -2.0, 3.0, probs=[0.5], moments=False))
    add("ik_post[cutoffs_wrong_length]", lambda c: H.ik_post(c.T(ccdf), [-0.5, 0.5], -2.0, 3.0))
    for dd in (2, 3):
        add(f"cov_pairwise[d{dd}]", lambda c, dd=dd: H.cov_pairwise(_vg(dd, True), X(dd), C0(dd)), True)
        add(f"cov_pairwise[d{dd}-self]", lambda c, dd=dd: H.cov_pairwise(_vg(), X(dd)), True)
        for zname, z in (("z1", Z), ("z2", Z2)):
            add(f"variogram_empirical[d{dd}-{zname}]", lambda c, dd=dd, z=z: H.variogram_empirical(
                c.T(X(dd)), c.T(z), 4, 6.0, direction=[1.0, 0.0, 0.0][:dd], dtol=0.5, cos_atol=0.25, estimator=1))
            add(f"variogram_cross[d{dd}-{zname}]", lambda c, dd=dd, z=z: H.variogram_cross(
                c.T(X(dd)), c.T(z), 4, 6.0, direction=[1.0, 0.0, 0.0][:dd], dtol=0.5))
        add(f"variogram_empirical[d{dd}-omni]", lambda c, dd=dd: H.variogram_empirical(c.T(X(dd)), c.T(Z), 4, 6.0))
        add(f"variogram_cross[d{dd}-omni]", lambda c, dd=dd: H.variogram_cross(c.T(X(dd)), c.T(Z2), 4, 6.0))
        add(f"decluster_cell_counts[d{dd}]", lambda c, dd=dd: H.decluster_cell_counts(c.T(X(dd)), [0.0] * dd, [2.0] * dd))
        add(f"decluster_cells[d{dd}]", lambda c, dd=dd: H.decluster_cells(
            c.T(X(dd)), c.T(Z), np.array([[1.0] * dd, [2.0] * dd]), 4, criterion="max"))
        add(f"decluster_cells[d{dd}-one_size_no_z]", lambda c, dd=dd: H.decluster_cells(c.T(X(dd)), None, [2.0] * dd, 1))
        add(f"decluster_nearest[d{dd}]", lambda c, dd=dd: H.decluster_nearest(
            c.T(X(dd)), [0.0] * dd, [0.5] * dd, [4] * dd))
    dirs = np.array([[1.0, 0.0], [0.0, 1.0]])
    add("variogram_plane[d2]", lambda c: H.variogram_plane(c.T(X(2)), c.T(Z2), 4, 6.0, dirs, ptol=0.5, estimator=1))
    add("variogram_plane[d3]", lambda c: H.variogram_plane(c.T(X(3)), c.T(Z), 4, 6.0, dirs, basis=np.eye(3)))
    add("variogram_plane[dirs_wrong_shape]", lambda c: H.variogram_plane(c.T(X(2)), c.T(Z), 4, 6.0, [1.0, 0.0]))
    add("variogram_plane[basis_wrong_shape]", lambda c: H.variogram_plane(c.T(X(3)), c.T(Z), 4, 6.0, dirs, basis=np.eye(2)))
    add("decluster_cells[bad_criterion]", lambda c: H.decluster_cells(c.T(X(2)), c.T(Z), [2.0, 2.0], 1, criterion="mean"))
    add("decluster_cells[mixed_spaces]", lambda c: H.decluster_cells(c.T(X(2)), __import__("torch").as_tensor(Z),
                                                                    [2.0, 2.0], 1))
    add("decluster_cell_counts[x_3d]", lambda c: H.decluster_cell_counts(c.T(np.zeros((2, 2, 2))), [0.0], [1.0]))
    hh, gg, cc = np.arange(1.0, 5.0), np.arange(1.0, 5.0) / 4.0, np.arange(4, 8)
    add("variogram_fit", lambda c: H.variogram_fit(hh, gg, cc, ["gaussian", "spherical"], nu=1.5, weighting=1,
                                                   max_nugget_frac=0.5), True)
    add("variogram_fit[lengths_differ]", lambda c: H.variogram_fit(hh, gg[:3], cc, ["gaussian"]), True)
    add("variogram_fit_aniso", lambda c: H.variogram_fit_aniso(hh, gg * 2.0, gg, cc, ["exponential"]), True)
    add("variogram_fit_lmc", lambda c: H.variogram_fit_lmc(hh, np.stack([gg, gg * 0.5, gg * 2.0]), cc,
                                                           ["exponential", "matern"], nu=1.5, weighting=1), True)
    add("variogram_fit_lmc[rows_not_triangular]", lambda c: H.variogram_fit_lmc(hh, np.stack([gg, gg]), cc,
                                                                              ["exponential"]), True)
    st = np.array([0, 0, 1, 0, 2, 0, 0])
    add("cv_summary", lambda c: H.cv_summary(c.T(Z), c.T(Z * 0.5), c.T(Z * Z + 1.0)))
    add("cv_summary[folds]", lambda c: H.cv_summary(c.T(Z), c.T(Z * 0.5), c.T(Z * Z + 1.0), status=c.T(st),
                                                    fold=c.T(FOLD), nfolds=3))
    add("cv_summary[lengths_differ]", lambda c: H.cv_summary(c.T(Z), c.T(Z[:5]), c.T(Z)))
    add("to_host", lambda c: E.to_host(c.T(__import__("torch").as_tensor(Z2)) if c.dev
                                       else __import__("torch").as_tensor(Z2)))
    return out


def run_all(dev=False):
    """{id: record} of the host forms, or of the device forms of the cases that have one."""
    ctx = Ctx(dev)
    return {name: record(lambda fn=fn: fn(ctx)) for name, host_only, fn in cases() if not (dev and host_only)}


# ---- the golden file: every distinct argument, call and outcome is written once --------------------------------------
def pack(records):
    """{id: record} -> {"args": [...], "calls": [[function, [arg number, ...]], ...], "outcomes": [...],
    "cases": {id: [[call number, ...], outcome number]}}: the cases share most of what they record."""
    pools = {"args": {}, "calls": {}, "outcomes": {}}

    def intern(pool, v):
        return pools[pool].setdefault(json.dumps(v, sort_keys=True), len(pools[pool]))
    cases_ = {}
    for name, rec in records.items():
        calls = [intern("calls", [fn, [intern("args", a) for a in args]]) for fn, args in rec["calls"]]
        cases_[name] = [calls, intern("outcomes", {k: v for k, v in rec.items() if k != "calls"})]
    out = {pool: [json.loads(k) for k in keys] for pool, keys in pools.items()}
    out["cases"] = cases_
    return out


def unpack(packed):
    out = {}
    for name, (calls, outcome) in packed["cases"].items():
        out[name] = dict(packed["outcomes"][outcome])
        out[name]["calls"] = [[fn, [packed["args"][a] for a in args]]
                              for fn, args in (packed["calls"][c] for c in calls)]
    return out


def load_golden():
    with open(GOLDEN) as f:
        return unpack(json.load(f))


def save_golden(records):
    packed = pack(json.loads(json.dumps(records)))
    with open(GOLDEN, "w") as f:                 # one entry per line: a change to one shows as one line
        f.write("{\n")
        for pool in ("args", "calls", "outcomes"):
            f.write(f'"{pool}": [\n' + ",\n".join(json.dumps(v, separators=(",", ":"), sort_keys=True)
                                                  for v in packed[pool]) + "\n],\n")
        f.write('"cases": {\n' + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}"
                                             for k, v in sorted(packed["cases"].items())) + "\n}\n}\n")


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    got = run_all()
    save_golden(got)
    print(len(got), "cases,", os.path.getsize(GOLDEN), "bytes")
