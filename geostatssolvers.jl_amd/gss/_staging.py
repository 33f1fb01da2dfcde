"""Argument staging of the binding: what every entry point does to its arguments before the library call.

Search ball and metric, fold ids, point sets and value columns, output arrays and the memory flag each have one
function here; gss/engine.py calls them and keeps only what is an entry point's own.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import MEM_DEVICE, MEM_HOST, is_torch


# ---- search ball and metric ---------------------------------------------------------------------------------------
def search_args(radius, radii, distance=None, rotation=None):
    """Solver parameters -> (radius, inv_radii, metric, metric_param) of gss_knn_search (gss.h): no ball is radius -1,
    an anisotropic ball the unit ball of its inverse radii, a rotated one GSS_METRIC_ROTATED_BALL with the 12-double
    inv_radii."""
    ir = None if radii is None else np.ascontiguousarray(1.0 / np.asarray(radii, dtype=np.float64))
    r = -1.0 if radius is None and radii is None else (1.0 if radii is not None else float(radius))
    met, mpar = _lib.metric_spec(distance)
    if rotation is not None:
        if radii is None:
            raise ValueError("a rotation needs an anisotropic ball (radii)")
        if met != 0:
            raise ValueError("a search ball cannot be combined with a non-Euclidean distance")
        met, ir = _lib.METRIC_ROTATED_BALL, _lib.rotated_ball_spec(radii, rotation)
    return r, ir, met, mpar


# ---- memory space ---------------------------------------------------------------------------------------------------
def on_device(x):
    """True for CUDA tensors; numpy arrays and CPU tensors (pinned ones included) are host memory."""
    return is_torch(x) and x.is_cuda


def mem_flag(x):
    """MEM_DEVICE / MEM_HOST of an array, or of a `device` flag."""
    return MEM_DEVICE if (x is True or on_device(x)) else MEM_HOST


def same_space(names, first, *others):
    """Refuse arrays that lie in two memory spaces -> True when their one space is the device."""
    dev = on_device(first)
    if any(on_device(a) != dev for a in others):
        raise ValueError(f"{names} must live in the same memory space")
    return dev


# ---- arrays in ------------------------------------------------------------------------------------------------------
def torch_dtypes():
    """numpy scalar type -> torch dtype of everything that crosses the C-ABI."""
    import torch
    return {np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}


def prep(x, dtype=np.float64):
    """Contiguous array of the right dtype in the space it already lives in."""
    if x is None:
        return None
    if is_torch(x):
        if not x.is_cuda:
            return np.ascontiguousarray(x.numpy(), dtype=dtype)
        return x.to(torch_dtypes()[dtype]).contiguous()
    return np.ascontiguousarray(x, dtype=dtype)


def values(z, device=False):
    """Contiguous float64 values on the host, or (`device`) in HBM: a host array beside CUDA centres is uploaded."""
    if not device:
        return np.ascontiguousarray(z, dtype=np.float64)
    if not is_torch(z):
        import torch
        z = torch.as_tensor(np.asarray(z, dtype=np.float64), device="cuda")
    return prep(z)


def samples(x, device=False):
    """Point-major (n, d) coordinates staged like `values`; a flat vector is n points on a line."""
    x = values(x, device)
    if device:
        return x.reshape(x.shape[0], -1)
    return x[:, None] if x.ndim == 1 else x


def centres(c, d, device=False):
    """(m, d) targets staged like `values`."""
    return values(c, device).reshape(-1, d)


def fold_arg(fold, n, device):
    """Fold ids of a cross-validation -> (int32 ids or None, device): a CUDA `fold` keeps the call in HBM as
    `device=True` does."""
    device = bool(device) or on_device(fold)
    if fold is None:
        return None, device
    if device:
        if not on_device(fold):
            raise ValueError("device=True needs the fold ids as a CUDA tensor")
        fold = prep(fold, np.int32)
    else:
        fold = np.ascontiguousarray(fold, dtype=np.int32)
    if tuple(fold.shape) != (n,):
        raise ValueError(f"fold must hold one id per sample ({n}), got shape {tuple(fold.shape)}")
    return fold, device


# ---- arrays out -----------------------------------------------------------------------------------------------------
def empty(where, shape, dtype=np.float64):
    """Uninitialised output: a CUDA tensor beside the tensor `where` (or on the current device for `where=True`), a
    numpy array for anything else."""
    if where is True or is_torch(where):
        import torch
        return torch.empty(shape, dtype=torch_dtypes()[dtype], device=where.device if is_torch(where) else "cuda")
    return np.empty(shape, dtype=dtype)


def estimate_out(where, shape, aux_shape, lists=None):
    """[estimate of `shape`, its variance / distance and status of `aux_shape`, idx, count]; `lists`: the shapes of
    the neighbour lists, or None for none (both entries None)."""
    out = [empty(where, shape), empty(where, aux_shape), empty(where, aux_shape, np.uint8)]
    return out + ([empty(where, s, np.int32) for s in lists] if lists else [None, None])


def estimate_result(out, return_idx):
    """(estimate, aux, status[, idx, count])"""
    return tuple(out) if return_idx else tuple(out[:3])
