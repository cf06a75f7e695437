"""Hierarchy simplification over the C ABI: pcp::algorithm::hierarchy_simplification
(include/pcp/algorithm/hierarchy_simplification.hpp) on the GPU.

Host arrays in, host arrays out (`hierarchy_simplification`); torch tensors on the GPU in, torch tensors out
(`hierarchy_simplification_dev`).  The kept points come out in the reference's queue order; the contract, and where it
departs from the reference, is in include/pcpx.h and DESIGN.md section 14.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import HierarchyParams, check


def _params(cluster_size, var_max):
    if int(cluster_size) < 0:
        raise ValueError("cluster_size must be >= 0")
    return HierarchyParams(C.sizeof(HierarchyParams), int(cluster_size), float(var_max))


def hierarchy_simplification(points, cluster_size, var_max=1.0 / 3.0, device=0, return_indices=False):
    """Kept points ((K, 3) float32) of `points` ((n, 3) float32-convertible); with return_indices=True also their input
    indices ((K,) uint32)."""
    lib = _capi.load()
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    prm = _params(cluster_size, var_max)
    n = p.shape[0]
    count = C.c_uint64(0)
    out = np.empty((n, 3), np.float32)  # (at most n points are kept: one call, no sizing pass)
    idx = np.empty(n, np.uint32)
    check(lib.pcpx_hierarchy_simplification(p.ctypes.data_as(C.c_void_p), n, C.byref(prm), device, out.ctypes.data_as(C.c_void_p),
                                            idx.ctypes.data_as(C.c_void_p), n, C.byref(count)))
    out, idx = out[:count.value].copy(), idx[:count.value].copy()
    return (out, idx) if return_indices else out


def hierarchy_simplification_raw(points, cluster_size, var_max, capacity, device=0, want_indices=True):
    """pcpx_hierarchy_simplification with an explicit capacity (the capacity protocol as the C ABI has it):
    (status, count, points, indices), the arrays sized by the capacity (indices None unless want_indices)."""
    lib = _capi.load()
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    prm = _params(cluster_size, var_max)
    out = np.full((capacity, 3), -7.0, np.float32)
    idx = np.full(capacity, 0xFFFFFFFF, np.uint32) if want_indices else None
    count = C.c_uint64(12345)
    st = lib.pcpx_hierarchy_simplification(p.ctypes.data_as(C.c_void_p), p.shape[0], C.byref(prm), device,
                                           out.ctypes.data_as(C.c_void_p) if capacity > 0 else None,
                                           idx.ctypes.data_as(C.c_void_p) if want_indices and capacity > 0 else None, capacity, C.byref(count))
    return st, int(count.value), out, idx


def hierarchy_simplification_dev(points, cluster_size, var_max=1.0 / 3.0, return_indices=False):
    """The same on a contiguous (n, 3) float32 CUDA tensor, on its device and current stream: a (K, 3) tensor (and the
    (K,) int32 tensor of input indices, as uint32 bits, with return_indices=True)."""
    import torch
    if points.dtype != torch.float32 or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a contiguous (n, 3) float32 tensor")
    lib = _capi.load()
    prm = _params(cluster_size, var_max)
    dev = points.device.index or 0
    stream = torch.cuda.current_stream(points.device).cuda_stream
    n = points.shape[0]
    count = C.c_uint64(0)
    out = torch.empty((n, 3), dtype=torch.float32, device=points.device)  # (at most n points are kept: one call)
    idx = torch.empty(n, dtype=torch.int32, device=points.device)
    check(lib.pcpx_hierarchy_simplification_dev(C.c_void_p(points.data_ptr()), n, C.byref(prm), dev, C.c_void_p(stream),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr()), n, C.byref(count)))
    out, idx = out[:count.value].clone(), idx[:count.value].clone()
    return (out, idx) if return_indices else out
