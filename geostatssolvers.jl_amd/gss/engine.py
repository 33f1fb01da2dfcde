"""Array-level engine over the C-ABI: the one place where Python touches libgss_hip.so.

Every method takes numpy arrays (host: the library stages them through PCIe) or CUDA torch tensors
(device: zero-copy, asynchronous on torch's current stream) and returns the same kind.
`HipEngine` is the only engine the product ships; the solver front-ends take an `engine=` argument
so that the CPU-only multi-process tests can exercise the sharding/host logic with a stand-in.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from . import _staging as st
from ._lib import MEM_HOST, check, current_stream, is_torch, make_variogram, ptr

SK, OK, UK, EDK = 0, 1, 2, 3


def _vg_struct(vg, dim, extent=None):
    if getattr(vg, "kind", None) == "power":
        # pseudo-covariance A - gamma(h): A = 2 gamma(diameter of the data box) keeps the data block positive
        # definite; constrained kriging results do not depend on A (gss.h, GSS_VG_POWER)
        if extent is None:
            raise ValueError("a power variogram is not stationary: only kriging with data can use it")
        a = 2.0 * (vg.range * max(float(extent), 1e-300) ** vg.nu) + vg.nugget + 1e-300
        return make_variogram("power", dim, a, vg.nugget, vg.range, vg.nu, None)
    if getattr(vg, "kind", None) == "nested":
        # first structure carries the total nugget; every structure contributes c_i (sill_i - nugget_i); a Gaussian
        # structure's nugget is the regularised one (variograms.py: nugget + 1e-6 unless regularize=False)
        for w, m in vg.terms:
            if m.effective_nugget > m.sill:
                # (a Gaussian structure with nugget = sill: the 1e-6 of the regularisation would make its structured part
                #  negative -- the single model is refused by the library for the same reason)
                raise ValueError(f"nested variogram: the (regularised) nugget {m.effective_nugget} of a {m.kind} structure "
                                 f"exceeds its sill {m.sill}")
        terms = [(w, m) for w, m in vg.terms if w * (m.sill - m.effective_nugget) > 0.0]
        if not terms:
            raise ValueError("nested variogram without a structured (non-nugget) component")
        w0, m0 = terms[0]
        nug = vg.effective_nugget
        extras = [(m.kind, w * (m.sill - m.effective_nugget), m.range, m.nu, m.radii, getattr(m, "rotation", None))
                  for w, m in terms[1:]]
        return make_variogram(m0.kind, dim, w0 * (m0.sill - m0.effective_nugget) + nug, nug, m0.range, m0.nu, m0.radii,
                              extras, rotation=getattr(m0, "rotation", None))
    return make_variogram(vg.kind, dim, vg.sill, getattr(vg, "effective_nugget", vg.nugget), vg.range, vg.nu, vg.radii,
                          rotation=getattr(vg, "rotation", None))


def _extent(x):
    """Diameter of the bounding box of point-major coordinates (numpy or CUDA tensor)."""
    if is_torch(x):
        return float(((x.max(dim=0).values - x.min(dim=0).values) ** 2).sum().sqrt())
    x = np.asarray(x)
    return float(np.sqrt(((x.max(axis=0) - x.min(axis=0)) ** 2).sum()))


def to_host(t):
    """numpy copy of a contiguous CUDA tensor through the library's transfer path (gss_dev_to_host: pinned bounce
    buffers, ~45 GB/s into pageable memory where `tensor.cpu()` manages ~10)."""
    t = t.contiguous()
    out = np.empty(tuple(t.shape), dtype={v: k for k, v in st.torch_dtypes().items()}[t.dtype])
    check(_lib.lib().gss_dev_to_host(ptr(out), C.c_void_p(t.data_ptr()), out.nbytes, current_stream()))
    return out


def _alias_tensor(owner, dev_ptr, nbytes):
    """CUDA float64 tensor aliasing `nbytes` of library-owned HBM at `dev_ptr` (for torch.distributed.broadcast over
    RCCL); it keeps `owner` (the handle) alive."""
    import torch

    class _Alias:
        __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (dev_ptr, False),
                                    "version": 3, "strides": None}
    t = torch.as_tensor(_Alias(), device=f"cuda:{torch.cuda.current_device()}")
    t._gss_keepalive = owner
    return t


class _NativeState:
    """The library's own replication routes (gss.h "multi-GPU"): RCCL broadcast inside the library and HIP IPC."""
    _STATE_KIND = None

    def bcast_state(self, root=0):
        """ncclBroadcast of the state on the communicator of `parallel.native_comm()`; the peers adopt."""
        _lib.state_bcast(self._STATE_KIND, self._h, root)

    def export_state(self) -> bytes:
        """Token of `_lib.IPC_TOKEN_BYTES` (96) bytes that another process passes to `import_state` (keep this handle
        alive until it has)."""
        return _lib.state_ipc_export(self._STATE_KIND, self._h)

    def import_state(self, token: bytes):
        """Pull the owner's state into this handle (created without factor / spectrum) and adopt it."""
        _lib.state_ipc_import(self._STATE_KIND, self._h, token)


class KrigHandle(_NativeState):
    _STATE_KIND = _lib.STATE_KRIG

    """gss_krig_t*: fitted kriging system living in HBM."""

    def __init__(self, vg, variant, xdata, z, mean=0.0, degree=0, drift_data=None, factor=True, async_fit=False):
        """`async_fit`: GSS_KRIG_ASYNC_FIT -- the constructor returns once the fit is queued; the first global
        prediction assembles its right-hand sides beside it and reports the fit's status itself (the order of
        `solve`: fit, then predict, krig.jl:166-186)."""
        self._l = _lib.lib()
        x = st.samples(xdata)
        self.n, self.dim = x.shape
        zz = np.ascontiguousarray(z, dtype=np.float64)
        dd = None if drift_data is None else np.ascontiguousarray(drift_data, dtype=np.float64).reshape(self.n, -1)
        self.ndrift = 0 if dd is None else dd.shape[1]
        self.variant = variant
        h = C.c_void_p()
        v = _vg_struct(vg, self.dim, extent=_extent(x))
        check(self._l.gss_krig_create(C.byref(h), C.byref(v), variant, float(mean or 0.0), int(degree or 0),
                                      self.ndrift, ptr(x), ptr(zz), ptr(dd), self.n,
                                      (0 if factor else _lib.KRIG_NO_FACTOR) |
                                      (_lib.KRIG_ASYNC_FIT if (async_fit and factor) else 0), current_stream()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._l.gss_krig_destroy(self._h)
            self._h = None

    __del__ = close

    def factor_tensor(self):
        """CUDA tensor aliasing the factor state (for torch.distributed.broadcast over RCCL)."""
        p, nb = C.c_void_p(), C.c_int64()
        check(self._l.gss_krig_factor_buffer(self._h, C.byref(p), C.byref(nb)))
        return _alias_tensor(self, p.value, nb.value)

    def adopt_factor(self):
        check(self._l.gss_krig_adopt_factor(self._h))

    state_tensor, adopt_state = factor_tensor, adopt_factor      # the names parallel.replicate_state uses

    def set_block_support(self, cell, nsub=3):
        """Regularise the right-hand sides of `predict_global` over cells of size `cell` (gss.h,
        gss_krig_set_block_support); `nsub=0` returns to point support."""
        c = None if not nsub else np.ascontiguousarray(np.broadcast_to(np.asarray(cell, dtype=np.float64), (self.dim,)))
        check(self._l.gss_krig_set_block_support(self._h, ptr(c), int(nsub or 0), current_stream()))

    def predict_global(self, xdom, drift_dom=None):
        xdom = st.prep(xdom)
        m = xdom.shape[0]
        mean, var, status = st.estimate_out(xdom, (m,), (m,))[:3]
        dd = st.prep(drift_dom)
        check(self._l.gss_krig_predict_global(self._h, ptr(xdom), ptr(dd), m, ptr(mean), ptr(var), ptr(status),
                                              st.mem_flag(xdom), current_stream()))
        return mean, var, status

    def predict_knn(self, xdom, k, minneighbors=1, radius=None, radii=None, drift_dom=None, return_idx=False,
                    distance=None, rotation=None):
        """`rotation`: of the search ball `radii` (MetricBall.rotation; GSS_METRIC_ROTATED_BALL)."""
        xdom = st.prep(xdom)
        m = xdom.shape[0]
        out = st.estimate_out(xdom, (m,), (m,), ((m, k), (m,)) if return_idx else None)
        mean, var, status, idx, cnt = out
        dd = st.prep(drift_dom)
        r, ir, met, mpar = st.search_args(radius, radii, distance, rotation)
        check(self._l.gss_krig_predict_knn(self._h, ptr(xdom), ptr(dd), m, int(k), int(minneighbors), r, ptr(ir),
                                           met, mpar, ptr(mean), ptr(var), ptr(status), ptr(idx), ptr(cnt),
                                           st.mem_flag(xdom), current_stream()))
        return st.estimate_result(out, return_idx)

    def cv_global(self, device=False):
        """Leave-one-out predictions of every sample under the global neighbourhood, from the factor of the handle
        (gss.h, gss_krig_cv_global) -> (pred, variance, status)."""
        pred, var, status = st.estimate_out(bool(device), (self.n,), (self.n,))[:3]
        check(self._l.gss_krig_cv_global(self._h, ptr(pred), ptr(var), ptr(status), st.mem_flag(bool(device)),
                                         current_stream()))
        return pred, var, status

    def cv_global_folds(self, fold, device=False):
        """Every sample predicted from all samples outside its own fold under the global neighbourhood, from the factor
        of the handle (gss.h, gss_krig_cv_global_folds).  `fold`: n ids >= 0, arbitrary (numpy: host arrays out; CUDA
        int32 tensor: everything stays in HBM) or None for leave-one-out (`cv_global`).  -> (pred, variance, status)."""
        fold, device = st.fold_arg(fold, self.n, device)
        pred, var, status = st.estimate_out(device, (self.n,), (self.n,))[:3]
        check(self._l.gss_krig_cv_global_folds(self._h, ptr(fold), ptr(pred), ptr(var), ptr(status),
                                               st.mem_flag(device), current_stream()))
        return pred, var, status

    def cv_knn(self, k, fold=None, exclude_radius=None, minneighbors=1, radius=None, radii=None, return_idx=False,
               distance=None, rotation=None, device=False):
        """Every sample predicted from its k nearest samples outside its own fold (gss.h, gss_krig_cv_knn).  `fold`: n
        ids >= 0 (numpy: host arrays out; CUDA int32 tensor, or `device=True` without folds: everything stays in HBM)
        or None for leave-one-out; `exclude_radius`: leave-ball-out.  -> (pred, variance, status[, idx, count])."""
        fold, device = st.fold_arg(fold, self.n, device)
        out = st.estimate_out(device, (self.n,), (self.n,), ((self.n, int(k)), (self.n,)) if return_idx else None)
        pred, var, status, idx, cnt = out
        r, ir, met, mpar = st.search_args(radius, radii, distance, rotation)
        check(self._l.gss_krig_cv_knn(self._h, ptr(fold), -1.0 if exclude_radius is None else float(exclude_radius),
                                      int(k), int(minneighbors), r, ptr(ir), met, mpar, ptr(pred), ptr(var), ptr(status),
                                      ptr(idx), ptr(cnt), st.mem_flag(device), current_stream()))
        return st.estimate_result(out, return_idx)

    def predict_global_batch(self, xdom, zbatch):
        xdom = st.prep(xdom)
        zb = st.prep(zbatch)
        st.same_space("xdom and zbatch", xdom, zb)
        nb = zb.shape[0]
        m = xdom.shape[0]
        out = st.empty(xdom, (nb, m))
        check(self._l.gss_krig_predict_global_batch(self._h, ptr(xdom), m, ptr(zb), nb, ptr(out), st.mem_flag(xdom),
                                                    current_stream()))
        return out


class CoKrigHandle(KrigHandle):
    """gss_krig_t* of a cokriging system (gss.h, gss_cokrig_create): the stacked samples of nz variables under
    C_ab(h) = B1[a, b] rho(h) (+ B0[a, b] at a zero lag).  `structure` is a single variogram model of which only the
    shape is read (kind, range or ball, order).  `cv_global` and `cv_global_folds` are those of the kriging handle,
    `predict_knn` and `cv_knn` are the moving neighbourhood of cokriging; every other method of the kriging handle is refused by the
    library."""

    def __init__(self, structure, B0, B1, variant, xdata, z, var, means=None, async_fit=False, factor=True):
        """`factor=False`: gss_cokrig_create_local -- no system, no factor; the handle serves `predict_knn` and `cv_knn` only
        (at most four variables)."""
        self._l = _lib.lib()
        x = st.samples(xdata)
        self.n, self.dim = x.shape
        zz = np.ascontiguousarray(z, dtype=np.float64)
        vv = np.ascontiguousarray(var, dtype=np.int32)
        if zz.shape != (self.n,) or vv.shape != (self.n,):
            raise ValueError(f"z and var must hold one entry per stacked sample ({self.n})")
        b0 = np.ascontiguousarray(np.atleast_2d(np.asarray(B0, dtype=np.float64)))
        b1 = np.ascontiguousarray(np.atleast_2d(np.asarray(B1, dtype=np.float64)))
        self.nz = b1.shape[0]
        if b0.shape != (self.nz, self.nz) or b1.shape != (self.nz, self.nz):
            raise ValueError(f"B0 and B1 must be square matrices of one size (got {b0.shape}, {b1.shape})")
        mm = None
        if variant == SK:
            mm = np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if means is None else means, dtype=np.float64),
                                                      (self.nz,)))
        self.variant, self.ndrift = variant, 0
        if getattr(structure, "kind", None) in ("power", "nested"):
            raise ValueError("cokriging takes one stationary structure (the LMC has one structure plus nugget)")
        v = make_variogram(structure.kind, self.dim, 1.0, 0.0, structure.range, structure.nu, structure.radii,
                           rotation=getattr(structure, "rotation", None))
        h = C.c_void_p()
        if factor:
            check(self._l.gss_cokrig_create(C.byref(h), C.byref(v), self.nz, ptr(b0), ptr(b1), variant, ptr(mm), ptr(x),
                                            ptr(zz), ptr(vv), self.n, _lib.KRIG_ASYNC_FIT if async_fit else 0,
                                            current_stream()))
        else:
            check(self._l.gss_cokrig_create_local(C.byref(h), C.byref(v), self.nz, ptr(b0), ptr(b1), variant, ptr(mm),
                                                  ptr(x), ptr(zz), ptr(vv), self.n, current_stream()))
        self._h = h

    def predict_global(self, xdom):
        """-> (mean[nz, m], variance[nz, m], status[nz, m]); numpy in, numpy out; CUDA tensors stay in HBM."""
        xdom = st.prep(xdom)
        m = xdom.shape[0]
        mean, var, status = st.estimate_out(xdom, (self.nz, m), (self.nz, m))[:3]
        check(self._l.gss_cokrig_predict_global(self._h, ptr(xdom), m, ptr(mean), ptr(var), ptr(status), st.mem_flag(xdom),
                                                current_stream()))
        return mean, var, status

    def predict_batch(self, xdom, zbatch):
        """Means of every target for many value vectors at the handle's stacked samples (gss.h,
        gss_cokrig_predict_global_batch).  `zbatch`: (nbatch, n) in the row order the handle was created with (one
        vector: (n,)); numpy in, numpy out; CUDA tensors stay in HBM.  -> mean[nbatch, nz, m].  (The inherited
        `predict_global_batch` is the single-variable call, which the library refuses for a cokriging system.)"""
        xdom = st.prep(xdom)
        zb = st.prep(zbatch)
        if zb.ndim == 1:
            zb = zb[None, :]
        st.same_space("xdom and zbatch", xdom, zb)
        if zb.ndim != 2 or zb.shape[1] != self.n:
            raise ValueError(f"zbatch must hold one value per stacked sample ({self.n}) in every row, got shape "
                             f"{tuple(zb.shape)}")
        nb, m = zb.shape[0], xdom.shape[0]
        out = st.empty(xdom, (nb, self.nz, m))
        check(self._l.gss_cokrig_predict_global_batch(self._h, ptr(xdom), m, ptr(zb), nb, ptr(out), st.mem_flag(xdom),
                                                      current_stream()))
        return out

    def predict_knn(self, xdom, k, minneighbors=1, radius=None, radii=None, return_idx=False, rotation=None):
        """Moving neighbourhood (gss.h, gss_cokrig_predict_knn): the `k[a]` nearest samples of every variable a, each
        variable searched on its own.  `k`: one count per variable, or an int for all of them.
        -> (mean[nz, m], variance[nz, m], status[nz, m][, idx[m, sum k], count[m, nz]])."""
        xdom = st.prep(xdom)
        m = xdom.shape[0]
        kk = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.int32), (self.nz,)))
        ksum = int(kk.sum())
        out = st.estimate_out(xdom, (self.nz, m), (self.nz, m),
                              ((m, max(ksum, 0)), (m, self.nz)) if return_idx else None)
        mean, var, status, idx, cnt = out
        r, ir, met, mpar = st.search_args(radius, radii, rotation=rotation)     # cokriging searches Euclidean only
        check(self._l.gss_cokrig_predict_knn(self._h, ptr(xdom), m, ptr(kk), int(minneighbors), r, ptr(ir), met, mpar,
                                             ptr(mean), ptr(var), ptr(status), ptr(idx), ptr(cnt), st.mem_flag(xdom),
                                             current_stream()))
        return st.estimate_result(out, return_idx)

    def cv_knn(self, k, fold=None, exclude_radius=None, minneighbors=1, radius=None, radii=None, return_idx=False,
               rotation=None, device=False):
        """Cross-validation under the moving neighbourhood (gss.h, gss_cokrig_cv_knn): every stacked sample predicted as
        its own variable from the `k[a]` nearest samples of every variable a outside its fold.  `k`: one count per
        variable, as a sequence (a bare int stays the one-variable call of the kriging handle, gss_krig_cv_knn, which
        the library refuses for a cokriging system and answers with the name of this one).  `fold`: n ids >= 0 (numpy: host arrays out; CUDA int32 tensor, or
        `device=True` without folds: everything stays in HBM) or None, every sample its own fold (collocated samples of
        other variables stay in play; one id per location removes whole locations); `exclude_radius`: leave-ball-out.
        -> (pred[n], variance[n], status[n][, idx[n, sum k], count[n, nz]])."""
        if np.ndim(k) == 0:
            return KrigHandle.cv_knn(self, k, fold, exclude_radius, minneighbors, radius, radii, return_idx,
                                     rotation=rotation, device=device)
        fold, device = st.fold_arg(fold, self.n, device)
        kk = np.ascontiguousarray(k, dtype=np.int32)
        if kk.shape != (self.nz,):
            raise ValueError(f"k must hold one count per variable ({self.nz}), got shape {kk.shape}")
        ksum = int(kk.sum())
        out = st.estimate_out(device, (self.n,), (self.n,),
                              ((self.n, max(ksum, 0)), (self.n, self.nz)) if return_idx else None)
        pred, var, status, idx, cnt = out
        r, ir, met, mpar = st.search_args(radius, radii, rotation=rotation)     # cokriging searches Euclidean only
        check(self._l.gss_cokrig_cv_knn(self._h, ptr(fold), -1.0 if exclude_radius is None else float(exclude_radius),
                                        ptr(kk), int(minneighbors), r, ptr(ir), met, mpar, ptr(pred), ptr(var),
                                        ptr(status), ptr(idx), ptr(cnt), st.mem_flag(device), current_stream()))
        return st.estimate_result(out, return_idx)


class FFTGSHandle(_NativeState):
    _STATE_KIND = _lib.STATE_FFTGS

    """gss_fftgs_t*: spectral amplitude + rocFFT plans for one variable."""

    def __init__(self, vg, dims, spacing=None, mean=0.0, spectrum=True):
        """`spectrum=False`: allocate the state only; it arrives by `state_tensor()` broadcast + `adopt_state()`."""
        self._l = _lib.lib()
        self.dims = tuple(int(d) for d in dims)
        nd = len(self.dims)
        d = (C.c_int64 * 3)(*(list(self.dims) + [1] * (3 - nd)))
        sp = (C.c_double * 3)(*([float(s) for s in (spacing if spacing is not None else [1.0] * nd)] + [1.0] * (3 - nd)))
        v = _vg_struct(vg, nd)
        h = C.c_void_p()
        check(self._l.gss_fftgs_create(C.byref(h), C.byref(v), nd, d, sp, float(mean),
                                       0 if spectrum else _lib.FFTGS_NO_SPECTRUM, current_stream()))
        self._h = h
        self.N = int(np.prod(self.dims))

    @classmethod
    def lmc(cls, structure, B0, B1, means, dims, spacing=None, spectrum=True):
        """The handle of a co-simulation under a linear model of coregionalisation (gss.h, gss_fftgs_create_lmc):
        C_ab(h) = B1[a, b] rho(h) (+ B0[a, b] at a zero lag), rho the shape of `structure` (kind, range or ball, order)
        with unit sill.  Its spectrum is rho's, so `spectrum`, `state_tensor` and `adopt_state` are those of a plain
        handle; `realize_lmc` realises it."""
        self = cls.__new__(cls)
        self._l = _lib.lib()
        self.dims = tuple(int(d) for d in dims)
        nd = len(self.dims)
        b0 = np.ascontiguousarray(np.atleast_2d(np.asarray(B0, dtype=np.float64)))
        b1 = np.ascontiguousarray(np.atleast_2d(np.asarray(B1, dtype=np.float64)))
        self.nz = b1.shape[0]
        if b0.shape != (self.nz, self.nz) or b1.shape != (self.nz, self.nz):
            raise ValueError(f"B0 and B1 must be square matrices of one size (got {b0.shape}, {b1.shape})")
        mm = np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if means is None else means, dtype=np.float64),
                                                  (self.nz,)))
        if getattr(structure, "kind", None) in ("power", "nested"):
            raise ValueError("a co-simulation takes one stationary structure (the LMC has one structure plus nugget)")
        d = (C.c_int64 * 3)(*(list(self.dims) + [1] * (3 - nd)))
        sp = (C.c_double * 3)(*([float(s) for s in (spacing if spacing is not None else [1.0] * nd)] + [1.0] * (3 - nd)))
        v = make_variogram(structure.kind, nd, 1.0, 0.0, structure.range, structure.nu, structure.radii,
                           rotation=getattr(structure, "rotation", None))
        h = C.c_void_p()
        check(self._l.gss_fftgs_create_lmc(C.byref(h), C.byref(v), self.nz, ptr(b0), ptr(b1), ptr(mm), nd, d, sp,
                                           0 if spectrum else _lib.FFTGS_NO_SPECTRUM, current_stream()))
        self._h = h
        self.N = int(np.prod(self.dims))
        return self

    def state_tensor(self):
        """CUDA tensor aliasing the spectral state (fft.jl:62-103 runs on one rank, the peers receive this)."""
        p, nb = C.c_void_p(), C.c_int64()
        check(self._l.gss_fftgs_state_buffer(self._h, C.byref(p), C.byref(nb)))
        return _alias_tensor(self, p.value, nb.value)

    def adopt_state(self):
        check(self._l.gss_fftgs_adopt_state(self._h, current_stream()))

    def close(self):
        if getattr(self, "_h", None):
            self._l.gss_fftgs_destroy(self._h)
            self._h = None

    __del__ = close

    def spectrum(self):
        out = np.empty(self.N)
        check(self._l.gss_fftgs_spectrum(self._h, ptr(out), MEM_HOST, current_stream()))
        return out

    @staticmethod
    def _inds(inds, out):
        """Cell indices of a partial realisation, in the memory space of `out`."""
        if inds is None:
            return None
        if st.on_device(out):
            import torch
            return torch.as_tensor(np.asarray(inds, dtype=np.int64), device=out.device)
        return np.ascontiguousarray(inds, dtype=np.int64)

    def realize(self, seed, first_real, nreals, noise=None, inds=None, out=None, device=False, pinned=False):
        """nreals x npts realisations; `device=True` (or a CUDA `out`/`noise`) keeps them in HBM.  Host results leave
        the device chunk by chunk while the next realisations are computed (at most three chunks of ~256 MiB staged in
        HBM, csrc OutStream); `pinned=True` returns a numpy view of page-locked memory, which the DMA engine writes
        directly (a pageable array goes through the library's pinned bounce buffers); `out` may be a numpy array or a
        CPU / pinned / CUDA tensor of shape (nreals, npts)."""
        noise = st.prep(noise)
        npts = self.N if inds is None else len(inds)
        if out is None:
            dev = bool(device) or st.on_device(noise)
            if pinned and not dev:
                import torch
                out = torch.empty((nreals, npts), dtype=torch.float64, pin_memory=True)
            else:
                out = st.empty(dev, (nreals, npts))
        if noise is not None:
            st.same_space("noise and out", out, noise)
        ii = self._inds(inds, out)
        check(self._l.gss_fftgs_realize(self._h, int(seed), int(first_real), int(nreals), ptr(noise), ptr(ii),
                                        0 if inds is None else npts, ptr(out), st.mem_flag(out), current_stream()))
        return out.numpy() if pinned and is_torch(out) and not out.is_cuda else out

    def realize_lmc(self, seed, first_real, nreals, noise=None, nugget_noise=None, inds=None, out=None, device=False):
        """nreals x nz x npts joint realisations of a handle made by `lmc` (gss.h, gss_fftgs_realize_lmc).  `noise`:
        (nreals, nz, N) uniforms for the unit fields, `nugget_noise`: (nreals, nz, N) normals for the nugget, each
        optional (parity checks); `device=True` (or a CUDA `out` / noise array) keeps everything in HBM, where the
        fields are mixed in place in `out`."""
        noise, nugget_noise = st.prep(noise), st.prep(nugget_noise)
        npts = self.N if inds is None else len(inds)
        given = [a for a in (noise, nugget_noise) if a is not None]
        if out is None:
            out = st.empty(bool(device) or any(st.on_device(a) for a in given), (nreals, self.nz, npts))
        st.same_space("noise, nugget_noise and out", out, *given)
        if any(tuple(a.shape) != (nreals, self.nz, self.N) for a in given):
            raise ValueError(f"noise and nugget_noise have the shape (nreals, nz, N) = {(nreals, self.nz, self.N)}")
        ii = self._inds(inds, out)
        check(self._l.gss_fftgs_realize_lmc(self._h, int(seed), int(first_real), int(nreals), ptr(noise),
                                            ptr(nugget_noise), ptr(ii), 0 if inds is None else npts, ptr(out),
                                            st.mem_flag(out), current_stream()))
        return out


class LUGSHandle(_NativeState):
    _STATE_KIND = _lib.STATE_LUGS

    """gss_lugs_t*: d2 and L22 in HBM for one variable."""

    def __init__(self, vg, centroids, dlocs, z1, mean=0.0, factor=True, factorization="cholesky"):
        """`factor=False`: allocate the state only; it arrives by `state_tensor()` broadcast + `adopt_state()`.
        `factorization`: "cholesky" (default) or "lu" (lu.jl:70: the unit lower factor of a pivoted LU)."""
        if factorization not in ("cholesky", "lu"):
            raise ValueError(f"factorization={factorization!r}: 'cholesky' or 'lu'")
        self._l = _lib.lib()
        c = st.samples(centroids)
        self.N, dim = c.shape
        dl = np.ascontiguousarray(dlocs, dtype=np.int64)
        zz = np.ascontiguousarray(z1, dtype=np.float64)
        v = _vg_struct(vg, dim)
        h = C.c_void_p()
        check(self._l.gss_lugs_create(C.byref(h), C.byref(v), ptr(c), self.N, ptr(dl), ptr(zz), dl.size,
                                      float(mean), (0 if factor else _lib.LUGS_NO_FACTOR)
                                      | (_lib.LUGS_FACT_LU if factorization == "lu" else 0), current_stream()))
        self._h = h
        self.nd = int(dl.size)
        self.ns = self.N - self.nd

    def state_tensor(self):
        """CUDA tensor aliasing L22 and d2 (lu.jl:76-169 runs on one rank, the peers receive this)."""
        p, nb = C.c_void_p(), C.c_int64()
        check(self._l.gss_lugs_state_buffer(self._h, C.byref(p), C.byref(nb)))
        return _alias_tensor(self, p.value, nb.value)

    def adopt_state(self):
        check(self._l.gss_lugs_adopt_state(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._l.gss_lugs_destroy(self._h)
            self._h = None

    __del__ = close

    def factor(self):
        l22 = np.empty((self.ns, self.ns))
        d2 = np.empty(self.ns)
        check(self._l.gss_lugs_factor(self._h, ptr(l22), ptr(d2), MEM_HOST, current_stream()))
        return l22.T.copy(), d2          # column-major on the wire -> numpy (row, col)

    def realize(self, seed, first_real, nreals, noise=None, rho=None, w1=None, device=False):
        noise = st.prep(noise)
        w1 = st.prep(w1)
        dev = bool(device) or is_torch(noise) or is_torch(w1)
        out, wout = st.empty(dev, (nreals, self.N)), st.empty(dev, (nreals, self.ns))
        check(self._l.gss_lugs_realize(self._h, int(seed), int(first_real), int(nreals), ptr(noise),
                                       0.0 if rho is None else float(rho), ptr(w1), ptr(out), ptr(wout), st.mem_flag(out),
                                       current_stream()))
        return out, wout


class SPDEHandle:
    """gss_spde_t*: the CSR of S = kappa^2 M - B of a triangle mesh in HBM; every realisation is one sparse solve."""

    NOISE = {"reference": _lib.SPDE_NOISE_REFERENCE, "lumped": _lib.SPDE_NOISE_LUMPED}

    def __init__(self, vertices, triangles, sill=1.0, range=1.0, noise="reference"):
        """`vertices` (nv, 2 or 3) and `triangles` (nt, 3; 0-based) as numpy arrays or CUDA tensors (both in one
        space).  `noise`: "reference" (spde.jl:98, w ~ N(0, I)) or "lumped" (Lindgren's w ~ N(0, inv(M)))."""
        if noise not in self.NOISE:
            raise ValueError(f"noise={noise!r}: 'reference' or 'lumped'")
        self._l = _lib.lib()
        dev = st.same_space("vertices and triangles", vertices, triangles)
        v = st.samples(vertices, dev)
        t = st.prep(triangles, np.int64)
        if v.ndim != 2 or t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("vertices (nv, d) and triangles (nt, 3)")
        h = C.c_void_p()
        check(self._l.gss_spde_create(C.byref(h), ptr(v), v.shape[0], v.shape[1], ptr(t), t.shape[0], float(sill),
                                      float(range), self.NOISE[noise], st.mem_flag(v), current_stream()))
        self._h = h
        nv, nt, nnz, tau2 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        check(self._l.gss_spde_info(h, C.byref(nv), C.byref(nt), C.byref(nnz), C.byref(tau2)))
        self.nv, self.nt, self.nnz, self.tau2 = nv.value, nt.value, nnz.value, tau2.value
        self.nd = 0                                                    # observations attached by condition()

    def close(self):
        if getattr(self, "_h", None):
            self._l.gss_spde_destroy(self._h)
            self._h = None

    __del__ = close

    def operator(self):
        """(rowptr, col, val, mass): the CSR of S (columns ascending within a row) and diag(M), on the host."""
        rowptr, col = np.empty(self.nv + 1, dtype=np.int64), np.empty(self.nnz, dtype=np.int32)
        val, mass = np.empty(self.nnz), np.empty(self.nv)
        check(self._l.gss_spde_operator(self._h, ptr(rowptr), ptr(col), ptr(val), ptr(mass), MEM_HOST,
                                        current_stream()))
        return rowptr, col, val, mass

    def locate(self, points, tol=None):
        """(triangle (np,) int64, weights (np, 3)) of `points` (np, dim): the triangle that contains each point (the
        nearest one whose plane projection contains it in 3-D; the lowest index on an edge or a vertex; -1 for none) and
        the barycentric weights in the order of its vertices.  Numpy in, numpy out; CUDA tensor in, CUDA tensors out."""
        p = st.prep(points)
        if p.ndim != 2:
            raise ValueError("points (np, dim)")
        tri, w = st.empty(p, (p.shape[0],), np.int64), st.empty(p, (p.shape[0], 3))
        check(self._l.gss_spde_locate(self._h, ptr(p), p.shape[0], 0.0 if tol is None else float(tol), ptr(tri), ptr(w),
                                      st.mem_flag(p), current_stream()))
        return tri, w

    def condition(self, obs_vertex, obs_weight, value, error_variance=None, mean=0.0, rtol=None, maxiter=None):
        """Attach observations: row i of `obs_vertex` (nd, 3) and `obs_weight` (nd, 3) is a sparse row of P, `value`
        (nd) what it observed, `error_variance` None (exact data) or (nd) values >= 0, `mean` the known field mean.
        Replaces earlier data; `realize` then returns conditional realisations and `mean()` the kriging mean."""
        v = st.prep(obs_vertex, np.int64)
        dev = st.same_space("the observation arrays", v, obs_weight, value,
                            *([] if error_variance is None else [error_variance]))
        w, y, r = st.prep(obs_weight), st.prep(value), st.prep(error_variance)
        nd = y.shape[0]
        if tuple(v.shape) != (nd, 3) or tuple(w.shape) != (nd, 3) or (r is not None and tuple(r.shape) != (nd,)):
            raise ValueError("obs_vertex (nd, 3), obs_weight (nd, 3), value (nd,) and error_variance (nd,)")
        self.nd = 0
        check(self._l.gss_spde_condition(self._h, nd, ptr(v), ptr(w), ptr(y), ptr(r), float(mean),
                                         0.0 if rtol is None else float(rtol), 0 if maxiter is None else int(maxiter),
                                         st.mem_flag(dev), current_stream()))
        self.nd = nd

    def condition_clear(self):
        check(self._l.gss_spde_condition_clear(self._h))
        self.nd = 0

    def attached(self):
        """(nd, mean) of the data the library holds for this handle; nd = 0: none."""
        nd, mean = C.c_int64(), C.c_double()
        check(self._l.gss_spde_condition_info(self._h, C.byref(nd), C.byref(mean), None, MEM_HOST, current_stream()))
        return nd.value, mean.value

    def weights(self):
        """W = inv(S) P' (nv, nd) of the attached data, on the host (parity)."""
        W = np.empty((self.nv, self.nd))
        check(self._l.gss_spde_condition_info(self._h, None, None, ptr(W), MEM_HOST, current_stream()))
        return W

    def mean(self, rtol=None, maxiter=None, vertices=False, device=False):
        """The kriging mean of the attached data per element (nt,); `vertices=True`: the pair (vertices (nv,), elements)."""
        eout = st.empty(bool(device), (self.nt,))
        vout = st.empty(bool(device), (self.nv,)) if vertices else None
        check(self._l.gss_spde_mean(self._h, 0.0 if rtol is None else float(rtol), 0 if maxiter is None else int(maxiter),
                                    ptr(vout), ptr(eout), st.mem_flag(eout), current_stream()))
        return (vout, eout) if vertices else eout

    def realize(self, seed, first_real, nreals, noise=None, rtol=None, maxiter=None, vertices=False, device=False):
        """Element values (nreals, nt) of realisations first_real .. first_real + nreals - 1; `vertices=True`: the pair
        (vertex values (nreals, nv), element values).  `noise`: (nreals, nv) normals instead of the Philox stream of
        `seed`; with data attached (nreals, nv + nd), the field normals followed by the error normals.  A column that
        does not converge raises GSSError (ERR_NO_CONVERGENCE); `last_solve()` has the counts."""
        noise = st.prep(noise)
        dev = bool(device) or st.on_device(noise)
        if noise is not None:
            if dev and not st.on_device(noise):
                raise ValueError("device=True needs the noise as a CUDA tensor")
            if self.nd:
                if tuple(noise.shape) != (nreals, self.nv + self.nd):
                    raise ValueError(f"noise must be (nreals, nv + nd) = ({nreals}, {self.nv + self.nd}), got "
                                     f"{tuple(noise.shape)}")
            elif tuple(noise.shape) != (nreals, self.nv):
                raise ValueError(f"noise must be (nreals, nv) = ({nreals}, {self.nv}), got {tuple(noise.shape)}")
        where = noise if st.on_device(noise) else dev
        eout = st.empty(where, (nreals, self.nt))
        vout = st.empty(where, (nreals, self.nv)) if vertices else None
        check(self._l.gss_spde_realize(self._h, int(seed), int(first_real), int(nreals), ptr(noise),
                                       0.0 if rtol is None else float(rtol), 0 if maxiter is None else int(maxiter),
                                       ptr(vout), ptr(eout), st.mem_flag(eout), current_stream()))
        return (vout, eout) if vertices else eout

    def last_solve(self):
        """(largest iteration count of a column, largest final ||r|| / ||b||, unconverged columns) of the last realize."""
        it, rel, un = C.c_int64(), C.c_double(), C.c_int64()
        check(self._l.gss_spde_last_solve(self._h, C.byref(it), C.byref(rel), C.byref(un)))
        return it.value, rel.value, un.value


class SGSHandle:
    """gss_sgs_t*: neighbour lists, simple-kriging weights and sigmas of every path node in HBM.

    `path`: None (LinearPath), a visiting order of N cells shared by every realisation, or an (npaths, N) array with
    one visiting order per realisation -- row p belongs to realisation `path_base + p` (seq.jl:99-102)."""

    def __init__(self, vg, centroids, path, dlocs, zdata, mean=0.0, maxneighbors=10, minneighbors=1, radius=None,
                 radii=None, path_base=0, mask_after_search=False, distance=None, rotation=None):
        """`mask_after_search`: GSS_SGS_MASK_AFTER_SEARCH (the k nearest cells of the whole domain, then the simulated
        ones) instead of the k nearest among the simulated cells.  `distance`: the search metric (euclidean,
        cityblock, chebyshev)."""
        self._l = _lib.lib()
        c = st.samples(centroids)
        self.N, dim = c.shape
        self.k = int(maxneighbors)
        pa = None if path is None else np.ascontiguousarray(path, dtype=np.int64)
        npaths = 1
        if pa is not None and pa.ndim == 2:
            npaths = pa.shape[0]
            if pa.shape[1] != self.N:
                raise ValueError(f"paths must have {self.N} cells each")
        dl = np.ascontiguousarray(dlocs if dlocs is not None else [], dtype=np.int64)
        zd = np.ascontiguousarray(zdata if zdata is not None else [], dtype=np.float64)
        r, ir, met, _ = st.search_args(radius, radii, distance, rotation)   # the flags word carries the metric id only
        v = _vg_struct(vg, dim)
        h = C.c_void_p()
        check(self._l.gss_sgs_create_paths(C.byref(h), C.byref(v), float(mean), ptr(c), self.N, dim, ptr(pa), npaths,
                                           int(path_base), ptr(dl), ptr(zd), dl.size, self.k, int(minneighbors), r,
                                           ptr(ir), (_lib.SGS_MASK_AFTER_SEARCH if mask_after_search else 0) |
                                           (met << _lib.SGS_METRIC_SHIFT),
                                           current_stream()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._l.gss_sgs_destroy(self._h)
            self._h = None

    __del__ = close

    def weights(self):
        idx = np.empty((self.N, self.k), dtype=np.int32)
        nc = np.empty(self.N, dtype=np.int32)
        w = np.empty((self.N, self.k))
        sg = np.empty(self.N)
        check(self._l.gss_sgs_weights(self._h, ptr(idx), ptr(nc), ptr(w), ptr(sg), MEM_HOST, current_stream()))
        return idx, nc, w, sg

    def schedule(self):
        """gss_sgs_schedule: which kernels the handle was built with and sweeps with (launches nothing)."""
        o = np.zeros(7, dtype=np.int32)
        check(self._l.gss_sgs_schedule(self._h, ptr(o), o.size))
        return dict(npaths=int(o[0]), levels=int(o[1]), team_chunks=int(o[2]), team_rl=int(o[3]), team_cap=int(o[4]),
                    big=bool(o[5]), big_lds=bool(o[6]))

    def realize(self, seed, first_real, nreals, noise=None, device=False, out=None):
        noise = st.prep(noise)
        if out is not None:
            if tuple(out.shape) != (nreals, self.N):
                raise ValueError(f"out must have shape ({nreals}, {self.N})")
        else:
            out = st.empty(bool(device) or is_torch(noise), (nreals, self.N))
        check(self._l.gss_sgs_realize(self._h, int(seed), int(first_real), int(nreals), ptr(noise), ptr(out),
                                      st.mem_flag(out), current_stream()))
        return out

    def realize_indicator(self, kind, cutoffs, fstar, zmin=0.0, zmax=0.0, tail_power=(1.0, 1.0), seed=0, first_real=0,
                          nreals=1, uniforms=None, device=False, out=None):
        """gss_sis_realize: sequential indicator simulation on this handle, which must have been built with the
        indicator variogram.  `kind`: "continuous" (`cutoffs`, the global ccdf `fstar`, `zmin` / `zmax` / `tail_power` of
        the ccdf model) or "categorical" (`cutoffs=None`, `fstar` the global proportions; the handle's zdata and the
        result are codes 0 .. K-1).  `uniforms`: (nreals, N) instead of the Philox ones."""
        kinds = {"continuous": _lib.SIS_CONTINUOUS, "categorical": _lib.SIS_CATEGORICAL}
        if kind not in kinds:
            raise ValueError(f"kind={kind!r}: 'continuous' or 'categorical'")
        cut = None if cutoffs is None else np.ascontiguousarray(cutoffs, dtype=np.float64).reshape(-1)
        fs = np.ascontiguousarray(fstar, dtype=np.float64).reshape(-1)
        if cut is not None and cut.size != fs.size:
            raise ValueError(f"fstar has {fs.size} values for {cut.size} cutoffs")
        uniforms = st.prep(uniforms)
        if uniforms is not None and tuple(uniforms.shape) != (nreals, self.N):
            raise ValueError(f"uniforms must have shape ({nreals}, {self.N})")
        if out is not None:
            if tuple(out.shape) != (nreals, self.N):
                raise ValueError(f"out must have shape ({nreals}, {self.N})")
        else:
            out = st.empty(bool(device) or is_torch(uniforms), (nreals, self.N))
        check(self._l.gss_sis_realize(self._h, kinds[kind], ptr(cut), int(fs.size), ptr(fs), float(zmin), float(zmax),
                                      float(tail_power[0]), float(tail_power[1]), int(seed), int(first_real),
                                      int(nreals), ptr(uniforms), ptr(out), st.mem_flag(out), current_stream()))
        return out


def _runs(shape, strides):
    """(nblocks, len, stride) of an array with element `strides` if it is `nblocks` contiguous runs of `len` elements
    that start `stride` elements apart -- a contiguous array, or a view strided along its first axes --, else None."""
    size = 1
    for n in shape:
        size *= n
    if size == 0:
        return None
    nd = len(shape)
    j, run = nd, 1
    while j > 0 and (shape[j - 1] == 1 or strides[j - 1] == run):     # trailing axes that are contiguous
        run *= shape[j - 1]
        j -= 1
    lead = [(n, s) for n, s in zip(shape[:j], strides[:j]) if n != 1]
    if not lead:
        return 1, run, run
    for (n0, s0), (n1, s1) in zip(lead, lead[1:]):                    # leading axes that collapse into one stride
        if s0 != n1 * s1:
            return None
    nb = 1
    for n, _ in lead:
        nb *= n
    st = lead[-1][1]
    return (nb, run, st) if st >= run else None


def _elem_strides(a):
    if is_torch(a):
        return tuple(a.stride())
    return tuple(s // a.itemsize if s % a.itemsize == 0 else -1 for s in a.strides)


class NScoreHandle:
    """gss_nscore_t*: the knots of a normal-score transform and their guide tables in HBM (gss.h).

    `values` / `weights`: host arrays (the fit is preprocess); `tails`: (zmin, zmax), None or NaN entries meaning the
    smallest / largest value; `tail_power`: (lower, upper).  `forward` and `inverse` take numpy arrays (host: staged in
    chunks) or CUDA tensors (device: one launch on torch's current stream) of any shape and return the same kind; a
    float64 view that is strided along its first axes only -- variable a of an (nreals, nz, N) ensemble -- is
    transformed where it lies, anything else is made contiguous first.  `out=x` transforms in place; an `out` that is
    not such runs, or not the runs of the input, is filled from a contiguous temporary."""

    def __init__(self, values, weights=None, tails=None, tail_power=(1.0, 1.0)):
        z = np.ascontiguousarray(values, dtype=np.float64).ravel()
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).ravel()
        if w is not None and w.size != z.size:
            raise ValueError(f"{w.size} weights for {z.size} values")
        lo, hi = (None, None) if tails is None else tails
        self._l = _lib.lib()
        h = C.c_void_p()
        check(self._l.gss_nscore_create(C.byref(h), ptr(z), ptr(w), z.size, float("nan") if lo is None else float(lo),
                                        float("nan") if hi is None else float(hi), float(tail_power[0]),
                                        float(tail_power[1]), current_stream()))
        self._h = h
        k = C.c_int64()
        check(self._l.gss_nscore_info(h, C.byref(k)))
        self.nknots = k.value

    def close(self):
        if getattr(self, "_h", None):
            self._l.gss_nscore_destroy(self._h)
            self._h = None

    __del__ = close

    def table(self):
        """(v, y): the distinct values and their scores, read back from the device tables."""
        v, y = np.empty(self.nknots), np.empty(self.nknots)
        check(self._l.gss_nscore_table(self._h, ptr(v), ptr(y), MEM_HOST, current_stream()))
        return v, y

    @staticmethod
    def _as_runs(a):
        """`a` as it is when the library can walk it, else a contiguous float64 copy; and its (nblocks, len, stride)."""
        if is_torch(a):
            import torch
            if not a.is_cuda:
                a = a.numpy()
            else:
                r = _runs(tuple(a.shape), _elem_strides(a)) if a.dtype == torch.float64 else None
                if r is None:
                    a = a.to(torch.float64).contiguous()
                    r = (1, a.numel(), a.numel())
                return a, r
        a = np.asarray(a)
        r = _runs(a.shape, _elem_strides(a)) if a.dtype == np.float64 and a.ctypes.data % 8 == 0 else None
        if r is None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            r = (1, a.size, a.size)
        return a, r

    def _apply(self, direction, x, out):
        x, (nb, ln, si) = self._as_runs(x)
        if out is None:
            out = st.empty(x, tuple(x.shape))
            so = ln
        else:
            if is_torch(out) and not out.is_cuda:
                out = out.numpy()
            if tuple(out.shape) != tuple(x.shape) or st.mem_flag(out) != st.mem_flag(x):
                raise ValueError("out must have the shape of the input and live where it lives")
            if nb * ln == 0:
                return out
            f64 = str(out.dtype).endswith("float64")
            r = _runs(tuple(out.shape), _elem_strides(out)) if f64 else None
            if r is not None and r[0] == 1 and nb > 1:   # a contiguous side is the runs of the other side, back to back
                r = (nb, ln, ln)
            elif r is not None and nb == 1 and r[0] > 1:
                nb, ln, si = r[0], r[1], r[1]
            if r is None or (r[0], r[1]) != (nb, ln):
                # `out` is no such runs, or other runs than the input: through a contiguous temporary
                tmp = self._apply(direction, x, None)
                if is_torch(out):
                    out.copy_(tmp)
                else:
                    out[...] = tmp
                return out
            so = r[2]
        if nb * ln:
            check(self._l.gss_nscore_apply(self._h, direction, ptr(x), ptr(out), nb, ln, si, so, st.mem_flag(x),
                                           current_stream()))
        return out

    def forward(self, x, out=None):
        """Values to scores: linear between the knots, y_1 below the smallest value and y_K above the largest."""
        return self._apply(_lib.NSCORE_FORWARD, x, out)

    def inverse(self, y, out=None):
        """Scores to values: linear between the knots, the tail model outside [y_1, y_K]."""
        return self._apply(_lib.NSCORE_INVERSE, y, out)


class HipEngine:
    """The product engine: every call lands in a gfx950 kernel."""
    name = "hip"
    device_resident = True     # handles accept / return CUDA tensors, so solvers may keep intermediates in HBM
    Krig = KrigHandle
    CoKrig = CoKrigHandle
    FFTGS = FFTGSHandle
    FFTGS_LMC = FFTGSHandle.lmc
    LUGS = LUGSHandle
    SGS = SGSHandle
    SPDE = SPDEHandle

    @staticmethod
    def nscore(values, weights=None, tails=None, tail_power=(1.0, 1.0)):
        """A normal-score transform fitted to `values` (NScoreHandle): `.forward(x)`, `.inverse(y)`, `.table()`."""
        return NScoreHandle(values, weights=weights, tails=tails, tail_power=tail_power)

    @staticmethod
    def cokrig(structure, B0, B1, variant, xdata, z, var, means=None, async_fit=False, factor=True):
        """A cokriging handle (CoKrigHandle).  `factor=True`: the fitted global system -- `predict_global(xdom)`,
        `predict_batch(xdom, zbatch)`, `cv_global()`, `cv_global_folds(fold)`, `predict_knn(xdom, k)`; `factor=False`: the samples only, for
        `predict_knn` (moving neighbourhood)."""
        return CoKrigHandle(structure, B0, B1, variant, xdata, z, var, means=means, async_fit=async_fit, factor=factor)

    @staticmethod
    def ik_predict_knn(xdata, z, xdom, cutoffs, variograms, k, minneighbors=1, fstar=None, radius=None, radii=None,
                       distance=None, rotation=None, return_raw=False, return_idx=False):
        """Indicator kriging under a moving neighbourhood (gss.h, gss_ik_predict_knn).  `variograms`: one model (median
        form) or a sequence of one per cutoff (full form).  `fstar=None`: the ordinary variant; K global proportions:
        simple kriging about them.  Host arrays in -> host arrays out; with a CUDA `xdom` everything stays in HBM.
        -> ccdf[m, K] (corrected), status[m][, raw[m, K]][, idx[m, k], count[m]]."""
        l = _lib.lib()
        dev = st.on_device(xdom)
        x, zz = st.samples(xdata, dev), st.values(z, dev)
        c = st.centres(xdom, x.shape[1], dev)
        n, d = int(x.shape[0]), int(x.shape[1])
        m = int(c.shape[0])
        if zz.ndim != 1 or zz.shape[0] != n:
            raise ValueError("z must have shape (n,)")
        cut = np.ascontiguousarray(cutoffs, dtype=np.float64).reshape(-1)
        K = int(cut.size)
        models = list(variograms) if isinstance(variograms, (list, tuple)) else [variograms]
        vgs = (_lib.Variogram * len(models))(*[_vg_struct(v, d) for v in models])
        fs = None if fstar is None else np.ascontiguousarray(fstar, dtype=np.float64).reshape(-1)
        if fs is not None and fs.size != K:
            raise ValueError(f"fstar has {fs.size} values for {K} cutoffs")
        ccdf = st.empty(c, (m, K))
        raw = st.empty(c, (m, K)) if return_raw else None
        status = st.empty(c, (m,), np.uint8)
        idx = st.empty(c, (m, int(k)), np.int32) if return_idx else None
        cnt = st.empty(c, (m,), np.int32) if return_idx else None
        r, ir, met, mpar = st.search_args(radius, radii, distance, rotation)
        check(l.gss_ik_predict_knn(ptr(x), ptr(zz), n, d, ptr(cut), K, vgs, len(models), SK if fs is not None else OK,
                                   ptr(fs), int(k), int(minneighbors), r, ptr(ir), met, mpar, ptr(c), m, ptr(ccdf),
                                   ptr(raw), ptr(status), ptr(idx), ptr(cnt), st.mem_flag(dev), current_stream()))
        out = (ccdf, status)
        if return_raw:
            out += (raw,)
        if return_idx:
            out += (idx, cnt)
        return out

    @staticmethod
    def ik_order_relations(ccdf):
        """GSLIB's order-relation correction of m x K rows, IN PLACE (gss.h, gss_ik_order_relations; numpy array or CUDA
        tensor, contiguous float64) -> (ccdf, ncorrected, maxcorr)."""
        l = _lib.lib()
        ok = ccdf.is_contiguous() if is_torch(ccdf) else (ccdf.flags.c_contiguous and ccdf.dtype == np.float64)
        if len(ccdf.shape) != 2 or not ok:
            raise ValueError("ccdf must be a contiguous float64 array of shape (m, K)")
        nc, mx = C.c_int64(0), C.c_double(0.0)
        check(l.gss_ik_order_relations(ptr(ccdf), int(ccdf.shape[0]), int(ccdf.shape[1]), C.byref(nc), C.byref(mx),
                                       st.mem_flag(ccdf), current_stream()))
        return ccdf, int(nc.value), float(mx.value)

    @staticmethod
    def ik_post(ccdf, cutoffs, zmin, zmax, tail_power=(1.0, 1.0), thresholds=(), probs=(), moments=True):
        """Post-processing of corrected ccdf rows (gss.h, gss_ik_post) -> dict with `etype`[m] and `cvar`[m] (when
        `moments`), `pabove`[m, nthr] (when thresholds are given) and `quant`[m, nq] (when probs are given), in the
        memory space of `ccdf`."""
        l = _lib.lib()
        f = st.values(ccdf, st.on_device(ccdf))
        if len(f.shape) != 2:
            raise ValueError("ccdf must have shape (m, K)")
        m, K = int(f.shape[0]), int(f.shape[1])
        cut = np.ascontiguousarray(cutoffs, dtype=np.float64).reshape(-1)
        if cut.size != K:
            raise ValueError(f"{cut.size} cutoffs for rows of {K}")
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = {}
        if moments:
            out["etype"] = st.empty(f, (m,))
            out["cvar"] = st.empty(f, (m,))
        if thr.size:
            out["pabove"] = st.empty(f, (m, thr.size))
        if pr.size:
            out["quant"] = st.empty(f, (m, pr.size))
        check(l.gss_ik_post(ptr(f), m, K, ptr(cut), float(zmin), float(zmax), float(tail_power[0]), float(tail_power[1]),
                            ptr(thr) if thr.size else None, int(thr.size), ptr(pr) if pr.size else None, int(pr.size),
                            ptr(out.get("etype")), ptr(out.get("cvar")), ptr(out.get("pabove")), ptr(out.get("quant")),
                            st.mem_flag(f), current_stream()))
        return out

    @staticmethod
    def cov_pairwise(vg, a, b=None):
        l = _lib.lib()
        a = st.samples(a)
        bb = a if b is None else st.centres(b, a.shape[1])
        out = np.empty((a.shape[0], bb.shape[0]))
        v = _vg_struct(vg, a.shape[1])
        check(l.gss_cov_pairwise(C.byref(v), ptr(a), a.shape[0], None if b is None else ptr(bb), bb.shape[0],
                                 ptr(out), bb.shape[0], MEM_HOST, current_stream()))
        return out

    @staticmethod
    def knn_search(xdata, centers, k, radius=None, radii=None, distance=None, rotation=None):
        """Host arrays in -> host arrays out; CUDA tensors for both point sets keep the search in HBM."""
        l = _lib.lib()
        # (the search is parsed, and a bad one refused, before the arrays are looked at)
        r, ir, met, mpar = st.search_args(radius, radii, distance, rotation)
        dev = st.same_space("xdata and centers", xdata, centers)
        x = st.samples(xdata, dev)
        c = st.centres(centers, x.shape[1], dev)
        m = c.shape[0]
        idx, cnt = st.empty(x, (m, k), np.int32), st.empty(x, m, np.int32)
        check(l.gss_knn_search(ptr(x), x.shape[0], x.shape[1], ptr(c), m, int(k), r, ptr(ir), met, mpar, ptr(idx),
                               ptr(cnt), st.mem_flag(dev), current_stream()))
        return idx, cnt

    @staticmethod
    def _estimate(fn_name, extra, xdata, z, xdom, k, minneighbors, radius, radii, distance=None, rotation=None):
        """Host arrays in -> host arrays out; if `xdom` is a CUDA tensor everything stays in HBM.  `z` of shape (n,) is
        one value column; (nz, n) is nz columns that share the search and the weights (gss_*_predict_cols: the mean
        comes back as (nz, m), distance / variance / status per point)."""
        l = _lib.lib()
        dev = st.on_device(xdom)
        x, zz = st.samples(xdata, dev), st.values(z, dev)
        c = st.centres(xdom, x.shape[1], dev)
        m = c.shape[0]
        mean, aux, status = st.estimate_out(dev, (m,) if zz.ndim == 1 else (zz.shape[0], m), m)[:3]
        if zz.ndim not in (1, 2) or zz.shape[-1] != x.shape[0]:
            raise ValueError("z must have shape (n,) or (nz, n)")
        r, ir, met, mpar = st.search_args(radius, radii, distance, rotation)
        if zz.ndim == 1:
            check(getattr(l, fn_name)(ptr(x), ptr(zz), x.shape[0], x.shape[1], ptr(c), m, int(k), int(minneighbors), r,
                                      ptr(ir), met, mpar, *extra, ptr(mean), ptr(aux), ptr(status),
                                      st.mem_flag(dev), current_stream()))
        else:
            check(getattr(l, fn_name + "_cols")(ptr(x), ptr(zz), x.shape[0], x.shape[1], int(zz.shape[0]), ptr(c), m, int(k),
                                                int(minneighbors), r, ptr(ir), met, mpar, *extra, ptr(mean), ptr(aux),
                                                ptr(status), st.mem_flag(dev), current_stream()))
        return mean, aux, status

    @staticmethod
    def idw(xdata, z, xdom, k, minneighbors=1, exponent=1.0, radius=None, radii=None, distance=None, rotation=None):
        """gss_idw_predict (idw.jl:111-142) -> mean, distance to the nearest sample, status."""
        return HipEngine._estimate("gss_idw_predict", (float(exponent),), xdata, z, xdom, k, minneighbors, radius,
                                   radii, distance, rotation)

    @staticmethod
    def lwr(xdata, z, xdom, k, minneighbors=1, weight=(0, 3.0, 2.0), radius=None, radii=None, distance=None,
            rotation=None):
        """gss_lwr_predict (lwr.jl:114-147); weight = (kind, a, p) -> mean, norm(r), status."""
        kind, a, p = weight
        return HipEngine._estimate("gss_lwr_predict", (int(kind), float(a), float(p)), xdata, z, xdom, k,
                                   minneighbors, radius, radii, distance, rotation)

    @staticmethod
    def _estimate_cv(fn_name, extra, xdata, z, k, fold, exclude_radius, minneighbors, radius, radii, return_idx,
                     distance, rotation, device):
        """gss_idw_cv / gss_lwr_cv (gss.h): every sample predicted from samples outside its own fold.  Host arrays in ->
        host arrays out; CUDA tensors for `xdata` / `z` / `fold` (all of them) with `device=True`, or a CUDA `fold`,
        keep everything in HBM.  `z` of shape (n,) is one value column, (nz, n) nz columns on one search and one weight
        vector per sample (`pred` comes back in the shape of `z`).  `k == n`: every eligible sample, no search (no
        lists: `return_idx` is refused).  -> (pred, aux, status[, idx, count])."""
        l = _lib.lib()
        n = len(xdata)
        fold, device = st.fold_arg(fold, n, device)
        x, zz = st.samples(xdata, device), st.values(z, device)
        if zz.ndim not in (1, 2) or zz.shape[-1] != n:
            raise ValueError("z must have shape (n,) or (nz, n)")
        if return_idx and int(k) >= n:
            raise ValueError("maxneighbors = n takes every eligible sample and runs no search: there are no lists")
        out = st.estimate_out(x if device else False, tuple(zz.shape), (n,), ((n, int(k)), (n,)) if return_idx else None)
        pred, aux, status, idx, cnt = out
        r, ir, met, mpar = st.search_args(radius, radii, distance, rotation)
        check(getattr(l, fn_name)(ptr(x), ptr(zz), n, x.shape[1], 1 if zz.ndim == 1 else int(zz.shape[0]), ptr(fold),
                                  -1.0 if exclude_radius is None else float(exclude_radius), int(k), int(minneighbors),
                                  r, ptr(ir), met, mpar, *extra, ptr(pred), ptr(aux), ptr(status), ptr(idx), ptr(cnt),
                                  st.mem_flag(device), current_stream()))
        return st.estimate_result(out, return_idx)

    @staticmethod
    def idw_cv(xdata, z, k, fold=None, exclude_radius=None, minneighbors=1, exponent=1.0, radius=None, radii=None,
               return_idx=False, distance=None, rotation=None, device=False):
        """Cross-validation of inverse distance weighting (gss.h, gss_idw_cv) -> (pred, distance to the nearest eligible
        sample, status[, idx, count]); the arguments of `_estimate_cv`."""
        return HipEngine._estimate_cv("gss_idw_cv", (float(exponent),), xdata, z, k, fold, exclude_radius, minneighbors,
                                      radius, radii, return_idx, distance, rotation, device)

    @staticmethod
    def lwr_cv(xdata, z, k, fold=None, exclude_radius=None, minneighbors=1, weight=(0, 3.0, 2.0), radius=None,
               radii=None, return_idx=False, distance=None, rotation=None, device=False):
        """Cross-validation of locally weighted regression (gss.h, gss_lwr_cv); weight = (kind, a, p) -> (pred, norm(r),
        status[, idx, count]); the arguments of `_estimate_cv`."""
        kind, a, p = weight
        return HipEngine._estimate_cv("gss_lwr_cv", (int(kind), float(a), float(p)), xdata, z, k, fold, exclude_radius,
                                      minneighbors, radius, radii, return_idx, distance, rotation, device)

    @staticmethod
    def lwr_callable(xdata, z, xdom, k, minneighbors, weightfun, radius=None, radii=None, distance=None, rotation=None):
        """LWR with an arbitrary `weightfun` callable (lwr.jl:58,136): the search runs on the device, delta = d / max d
        and w = weightfun(delta) are evaluated here on the host (the callable cannot cross the C-ABI), the normal
        equations and norm(r) on the device again (gss_lwr_predict_weights).  Host arrays."""
        x, zz = st.samples(xdata), st.values(z)
        c = st.centres(xdom, x.shape[1])
        m = c.shape[0]
        idx, cnt = HipEngine.knn_search(x, c, k, radius, radii, distance, rotation)
        valid = np.arange(k)[None, :] < cnt[:, None]
        nb = np.where(valid, idx, 0)
        diff = x[nb] - c[:, None, :]                              # m x k x d
        met, mpar = st.search_args(radius, radii, distance, rotation)[2:]    # as the search above parsed them
        if rotation is not None:                                 # frame of the ball: R^T (x - c) per neighbour
            diff = diff @ np.asarray(rotation, dtype=np.float64)
        if radii is not None:
            diff = diff / np.asarray(radii, dtype=np.float64)
        if met in (_lib.METRICS["euclidean"], _lib.METRIC_ROTATED_BALL):
            d = np.sqrt(np.sum(diff * diff, axis=-1))
        elif met == _lib.METRICS["cityblock"]:
            d = np.sum(np.abs(diff), axis=-1)
        elif met == _lib.METRICS["chebyshev"]:
            d = np.max(np.abs(diff), axis=-1)
        else:                                                    # ("haversine", r): (longitude, latitude) in degrees
            D = np.pi / 180.0
            s1 = np.sin((c[:, None, 1] - x[nb][..., 1]) * 0.5 * D)
            s2 = np.sin((c[:, None, 0] - x[nb][..., 0]) * 0.5 * D)
            key = s1 * s1 + np.cos(x[nb][..., 1] * D) * np.cos(c[:, None, 1] * D) * (s2 * s2)
            d = 2.0 * mpar * np.arcsin(np.minimum(np.sqrt(key), 1.0))
        d = np.where(valid, d, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            delta = d / d.max(axis=1, keepdims=True)             # lwr.jl:132
        # lwr.jl:136 `weightfun.(deltas)`: elementwise, on the neighbours that exist only; a scalar-only callable
        # (`lambda h: 1 - h if h < 1 else 0`) is mapped over them; a NaN weight (every distance zero: 0 / 0) stays NaN,
        # so that the point is reported singular as the reference's NaN estimate would show
        dv = delta[valid]
        try:
            wv = np.asarray(weightfun(dv), dtype=np.float64)
            if wv.shape != dv.shape:
                raise ValueError("weightfun did not map elementwise")
        except (TypeError, ValueError):
            wv = np.fromiter((float(weightfun(float(t))) for t in dv), dtype=np.float64, count=dv.size)
        w = np.zeros_like(delta)
        w[valid] = wv
        w = np.ascontiguousarray(w)
        mean, var, status = st.estimate_out(False, m, m)[:3]
        check(_lib.lib().gss_lwr_predict_weights(ptr(x), ptr(zz), x.shape[0], x.shape[1], ptr(c), m, int(k),
                                                 int(minneighbors), ptr(np.ascontiguousarray(idx)),
                                                 ptr(np.ascontiguousarray(cnt)), ptr(w), ptr(mean), ptr(var), ptr(status),
                                                 MEM_HOST, current_stream()))
        return mean, var, status


    # ---- variography (gss.h "variography") --------------------------------------------------------------------
    @staticmethod
    def _vario_xz(x, z):
        """x (n, d) and z (nz, n) in their one memory space, and whether that is the device."""
        dev = st.same_space("x and z", x, z)
        x = st.samples(x, dev)
        return x, st.values(z, dev).reshape(-1, x.shape[0]), dev

    @staticmethod
    def _vario_out(x, dev, shape, zshape):
        """count, lagsum of `shape`, the sums of `zshape` and the duplicate counter beside `x`."""
        ndup = st.empty(x, 1, np.int64) if dev else np.zeros(1, dtype=np.int64)
        return st.empty(x, shape, np.int64), st.empty(x, shape), st.empty(x, zshape), ndup

    @staticmethod
    def variogram_empirical(x, z, nlags, maxlag, direction=None, dtol=float("inf"), cos_atol=0.0, estimator=0,
                            distance=None):
        """Bin sums of the empirical variogram: x (n, d), z (nz, n) -> count (nlags,) int64, lagsum (nlags,),
        zsum (nz, nlags), nduplicates.  numpy arrays in -> numpy out; CUDA tensors for x and z keep everything in HBM
        (the outputs are tensors, nduplicates a 1-element tensor).  `direction`: a unit vector (host) or None."""
        if st.search_args(None, None, distance)[2] != 0:
            raise _lib.GSSError(_lib.ERR_UNSUPPORTED, "empirical variograms use the Euclidean distance only")
        l = _lib.lib()
        x, z, dev = HipEngine._vario_xz(x, z)
        (n, d), nz, nlags = x.shape, z.shape[0], int(nlags)
        count, lagsum, zsum, ndup = HipEngine._vario_out(x, dev, max(nlags, 0), (nz, max(nlags, 0)))
        u = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64).reshape(-1)
        if u is not None and u.size != d:
            raise ValueError(f"direction has {u.size} components for {d}-D samples")
        check(l.gss_variogram_empirical(ptr(x), n, d, ptr(z), nz, nlags, float(maxlag), ptr(u), float(dtol),
                                        float(cos_atol), int(estimator), ptr(count), ptr(lagsum), ptr(zsum), ptr(ndup),
                                        st.mem_flag(dev), current_stream()))
        return count, lagsum, zsum, (ndup if dev else int(ndup[0]))

    # ---- declustering (gss.h "declustering") ------------------------------------------------------------------
    @staticmethod
    def _declus_x(x):
        x = st.prep(x)
        if x.ndim not in (1, 2):
            raise ValueError("x must be (n, d) point-major coordinates")
        return st.samples(x, st.on_device(x)), st.on_device(x)

    @staticmethod
    def decluster_cell_counts(x, origin, sides):
        """One grid: x (n, d), origin and sides (d,) on the host -> count (n,) int32 (samples in each sample's cell) in
        the memory space of x, and the number of occupied cells (int)."""
        l = _lib.lib()
        x, dev = HipEngine._declus_x(x)
        n, d = x.shape
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        s = np.ascontiguousarray(sides, dtype=np.float64).reshape(-1)
        if o.size != d or s.size != d:
            raise ValueError(f"origin and sides need {d} components each, not {o.size} and {s.size}")
        count = st.empty(x, (n,), np.int32)
        nocc = C.c_int64()
        check(l.gss_decluster_cell_counts(ptr(x), n, d, ptr(o), ptr(s), ptr(count), C.byref(nocc),
                                          st.mem_flag(dev), current_stream()))
        return count, nocc.value

    @staticmethod
    def decluster_cells(x, z, sides, noffsets, criterion="min"):
        """The GSLIB sweep: x (n, d), z (n,) or None (one size only), sides (ncs, d) on the host -> weights (n,) of the
        best size in the memory space of x, wmean (ncs,) numpy (None without z), best (int)."""
        l = _lib.lib()
        x, dev = HipEngine._declus_x(x)
        n, d = x.shape
        if z is not None:
            st.same_space("x and z", x, z)
            z = st.prep(z).reshape(-1)
            if z.shape[0] != n:
                raise ValueError(f"{z.shape[0]} values for {n} samples")
        s = np.ascontiguousarray(sides, dtype=np.float64)
        if s.ndim == 1:
            s = s[None, :]
        if s.ndim != 2 or s.shape[1] != d:
            raise ValueError(f"sides must be (ncs, {d}), not {s.shape}")
        if criterion not in ("min", "max"):
            raise ValueError(f"criterion {criterion!r}: 'min' or 'max'")
        w = st.empty(x, (n,))
        wmean = None if z is None else np.empty(s.shape[0])
        best = C.c_int32()
        check(l.gss_decluster_cells(ptr(x), ptr(z), n, d, ptr(s), s.shape[0], int(noffsets),
                                    _lib.DECLUS_MIN if criterion == "min" else _lib.DECLUS_MAX, ptr(w), ptr(wmean),
                                    C.byref(best), st.mem_flag(dev), current_stream()))
        return w, wmean, best.value

    @staticmethod
    def decluster_nearest(x, lo, step, dims):
        """Polygonal declustering by discretisation: every point lo + (j + 1/2) step of the `dims` lattice goes to its
        nearest sample -> weights (n,) in the memory space of x, nzero (samples without a point)."""
        l = _lib.lib()
        x, dev = HipEngine._declus_x(x)
        n, d = x.shape
        lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1)
        step = np.ascontiguousarray(step, dtype=np.float64).reshape(-1)
        dims = np.ascontiguousarray(dims, dtype=np.int64).reshape(-1)
        if not (lo.size == step.size == dims.size == d):
            raise ValueError(f"lo, step and dims need {d} components each")
        w = st.empty(x, (n,))
        nzero = C.c_int64()
        check(l.gss_decluster_nearest(ptr(x), n, d, ptr(lo), ptr(step), ptr(dims), ptr(w), C.byref(nzero),
                                      st.mem_flag(dev), current_stream()))
        return w, nzero.value

    @staticmethod
    def variogram_fit(h, gamma, count, kinds, nu=1.0, weighting=0, max_nugget_frac=1.0):
        """gss_variogram_fit (host code of the library, no device): -> (kind name, sill, nugget, range, nu,
        objective per kind)."""
        l = _lib.load()
        h = np.ascontiguousarray(h, dtype=np.float64)
        g = np.ascontiguousarray(gamma, dtype=np.float64)
        c = np.ascontiguousarray(count, dtype=np.int64)
        if not (h.shape == g.shape == c.shape and h.ndim == 1):
            raise ValueError("h, gamma and count must be vectors of one length")
        names = {v: k for k, v in _lib._KINDS.items()}
        kk = np.ascontiguousarray([_lib._KINDS[k] for k in kinds], dtype=np.int32)
        obj = np.empty(len(kk))
        best = _lib.Variogram()
        check(l.gss_variogram_fit(ptr(h), ptr(g), ptr(c), h.size, ptr(kk), len(kk), float(nu), int(weighting),
                                  float(max_nugget_frac), C.byref(best), ptr(obj)))
        return names[best.kind], best.sill, best.nugget, best.range, best.nu, obj

    @staticmethod
    def variogram_plane(x, z, nlags, maxlag, dirs, basis=None, ptol=float("inf"), estimator=0):
        """gss_variogram_plane: x (n, d), d = 2 or 3, z (nz, n), dirs (nangles, 2) = (cos, sin) of the sectors' lower
        boundaries (host), basis (3, 3) = e1, e2, normal for d = 3 (host) -> count (nangles, nlags) int64,
        lagsum (nangles, nlags), zsum (nz, nangles, nlags), nduplicates.  Memory as in variogram_empirical."""
        l = _lib.lib()
        x, z, dev = HipEngine._vario_xz(x, z)
        (n, d), nz, nlags = x.shape, z.shape[0], int(nlags)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64)
        if dirs.ndim != 2 or dirs.shape[1] != 2:
            raise ValueError("dirs is an (nangles, 2) array of (cos, sin)")
        nang = dirs.shape[0]
        b = None
        if basis is not None:
            b = np.ascontiguousarray(basis, dtype=np.float64)
            if b.shape != (3, 3):
                raise ValueError("basis is a (3, 3) array: e1, e2 and the normal as rows")
        shape = (nang, max(nlags, 0))
        count, lagsum, zsum, ndup = HipEngine._vario_out(x, dev, shape, (nz,) + shape)
        check(l.gss_variogram_plane(ptr(x), n, d, ptr(z), nz, nlags, float(maxlag), nang, ptr(dirs), ptr(b), float(ptol),
                                    int(estimator), ptr(count), ptr(lagsum), ptr(zsum), ptr(ndup),
                                    st.mem_flag(dev), current_stream()))
        return count, lagsum, zsum, (ndup if dev else int(ndup[0]))

    @staticmethod
    def variogram_fit_aniso(h, phi, gamma, count, kinds, nu=1.0, weighting=0, max_nugget_frac=1.0):
        """gss_variogram_fit_aniso (host code of the library, no device): per-bin vectors -> (kind name, sill, nugget,
        (r1, r2) or None when the fit is isotropic, theta, isotropic range, nu, objective per kind)."""
        l = _lib.load()
        h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
        p = np.ascontiguousarray(phi, dtype=np.float64).reshape(-1)
        g = np.ascontiguousarray(gamma, dtype=np.float64).reshape(-1)
        c = np.ascontiguousarray(count, dtype=np.int64).reshape(-1)
        if not h.shape == p.shape == g.shape == c.shape:
            raise ValueError("h, phi, gamma and count must have one length")
        names = {v: k for k, v in _lib._KINDS.items()}
        kk = np.ascontiguousarray([_lib._KINDS[k] for k in kinds], dtype=np.int32)
        obj = np.empty(len(kk))
        best = _lib.Variogram()
        check(l.gss_variogram_fit_aniso(ptr(h), ptr(p), ptr(g), ptr(c), h.size, ptr(kk), len(kk), float(nu),
                                        int(weighting), float(max_nugget_frac), C.byref(best), ptr(obj)))
        if best.aniso == 0:
            return names[best.kind], best.sill, best.nugget, None, 0.0, best.range, best.nu, obj
        radii = (1.0 / best.inv_radii[0], 1.0 / best.inv_radii[1])
        theta = float(np.arctan2(best.rotation[3], best.rotation[0]))
        return names[best.kind], best.sill, best.nugget, radii, theta, best.range, best.nu, obj

    @staticmethod
    def variogram_cross(x, z, nlags, maxlag, direction=None, dtol=float("inf"), cos_atol=0.0):
        """gss_variogram_cross: x (n, d), z (nz, n) -> count (nlags,) int64, lagsum (nlags,), csum (nz (nz + 1) / 2,
        nlags) -- row a nz - a (a - 1) / 2 + (b - a) holds the pair (a, b), a <= b -- and nduplicates.  Memory as in
        variogram_empirical."""
        l = _lib.lib()
        x, z, dev = HipEngine._vario_xz(x, z)
        (n, d), nz, nlags = x.shape, z.shape[0], int(nlags)
        shape = (nz * (nz + 1) // 2, max(nlags, 0))
        count, lagsum, csum, ndup = HipEngine._vario_out(x, dev, shape[1], shape)
        u = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64).reshape(-1)
        if u is not None and u.size != d:
            raise ValueError(f"direction has {u.size} components for {d}-D samples")
        check(l.gss_variogram_cross(ptr(x), n, d, ptr(z), nz, nlags, float(maxlag), ptr(u), float(dtol), float(cos_atol),
                                    ptr(count), ptr(lagsum), ptr(csum), ptr(ndup), st.mem_flag(dev), current_stream()))
        return count, lagsum, csum, (ndup if dev else int(ndup[0]))

    @staticmethod
    def variogram_fit_lmc(h, gamma, count, kinds, nu=1.0, weighting=0):
        """gss_variogram_fit_lmc (host code of the library, no device): h, count (nlags,), gamma (nz (nz + 1) / 2,
        nlags) in the row order of variogram_cross -> (kind name, range, B0 (nz, nz), B1 (nz, nz), objective per
        kind)."""
        l = _lib.load()
        h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
        g = np.ascontiguousarray(gamma, dtype=np.float64).reshape(-1, h.size)
        c = np.ascontiguousarray(count, dtype=np.int64).reshape(-1)
        if c.shape != h.shape:
            raise ValueError("h and count must be vectors of one length")
        nz = int(round((np.sqrt(8.0 * g.shape[0] + 1.0) - 1.0) / 2.0))
        if nz * (nz + 1) // 2 != g.shape[0]:
            raise ValueError("gamma has nz (nz + 1) / 2 rows: one per pair of variables (a, b), a <= b")
        names = {v: k for k, v in _lib._KINDS.items()}
        kk = np.ascontiguousarray([_lib._KINDS[k] for k in kinds], dtype=np.int32)
        obj = np.empty(len(kk))
        kind, rng = C.c_int32(0), C.c_double(0.0)
        b0, b1 = np.zeros((max(nz, 1), max(nz, 1))), np.zeros((max(nz, 1), max(nz, 1)))
        check(l.gss_variogram_fit_lmc(ptr(h), ptr(g), ptr(c), h.size, nz, ptr(kk), len(kk), float(nu), int(weighting),
                                      C.byref(kind), C.byref(rng), ptr(b0), ptr(b1), ptr(obj)))
        return names[kind.value], rng.value, b0, b1, obj

    @staticmethod
    def cv_summary(z, pred, var, status=None, fold=None, nfolds=0):
        """gss_cv_summary: the error summary of a cross-validation, reduced on the device in a fixed order -> (dict of
        the fields of gss_cv_summary_t, per-fold mean squared errors or None).  numpy arrays or CUDA tensors, all in
        one memory space."""
        l = _lib.lib()
        dev = st.on_device(z)
        stage = st.prep if dev else np.ascontiguousarray     # every array lies where z does
        z, pred, var = (stage(a, dtype=np.float64) for a in (z, pred, var))
        status = None if status is None else stage(status, dtype=np.uint8)
        fold = None if fold is None else stage(fold, dtype=np.int32)
        n = z.shape[0]
        if any(a is not None and tuple(a.shape) != (n,) for a in (pred, var, status, fold)):
            raise ValueError("z, pred, var, status and fold must have one length")
        nf = int(nfolds) if fold is not None else 0
        fmse = st.empty(z, (nf,)) if nf > 0 else None
        out = _lib.CVSummary()
        check(l.gss_cv_summary(ptr(z), ptr(pred), ptr(var), ptr(status), ptr(fold), n, nf, C.byref(out), ptr(fmse),
                               st.mem_flag(dev), current_stream()))
        return {f: getattr(out, f) for f, _ in _lib.CVSummary._fields_}, fmse


def default_engine():
    return HipEngine
