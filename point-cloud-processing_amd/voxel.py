"""Voxel-grid downsampling over the C ABI (include/pcpx_voxel.h): the points of every occupied cell of a regular
grid replaced by their centroid, attributes averaged with them, in ascending order of the cell key and to the bit: PCL's VoxelGrid,
Open3D's voxel_down_sample.

Host arrays in, host arrays out (`voxel_grid`); device arrays in and out, enqueued without a synchronisation (`voxel_grid_dev`):
torch tensors or plain device addresses.  `voxel_plan` is the device scratch such a call takes.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check
from .match import _device_of, _dptr, _stream_of, _vp

NONE = _capi.PCPX_VOXEL_NONE


def voxel_params(leaf, origin=None, attr_columns=0):
    """pcpx_voxel_params: leaf one edge or three; origin None: the per-axis minimum of the finite points."""
    p = _capi.VoxelParams()
    edges = np.broadcast_to(np.asarray(leaf, np.float32).reshape(-1), (3,))
    p.leaf[:] = [float(v) for v in edges]
    if origin is not None:
        p.origin[:] = [float(v) for v in np.asarray(origin, np.float32).reshape(3)]
        p.flags = _capi.PCPX_VOXEL_ORIGIN
    p.attr_columns = int(attr_columns)
    return p


def voxel_plan(n, capacity=None):
    """pcpx_voxel_plan: {"sort_bytes", "scratch_bytes"} of a call over n rows with room for `capacity` voxels (None: n)."""
    sort, scratch = C.c_uint64(0), C.c_uint64(0)
    check(_capi.load().pcpx_voxel_plan(int(n), int(n if capacity is None else capacity), C.byref(sort), C.byref(scratch)))
    return {"sort_bytes": sort.value, "scratch_bytes": scratch.value}


def voxel_grid(points, leaf, attrs=None, origin=None, capacity=None, device=0):
    """One point per occupied cell of the grid of edge(s) `leaf` over `points` ((n, 3) float32-convertible): the centroid of the
    cell's points, and the mean of their rows of `attrs` ((n, A), A <= 16).  Cells come in ascending key order (z, then y, then x).
    Rows with a non-finite coordinate, or outside the 2^21 cells an axis has from the origin on, are dropped.  Returns a dict:
    "points" ((V, 3) float32), "attrs" ((V, A), with attrs), "counts" ((V,) uint32), "keys" ((V,) uint64), "rows" ((V,) uint32: the
    cell's point nearest its centroid), "owner" ((n,) uint32: the cell of every row, NONE for a dropped one), "dropped", "origin"
    ((3,) float32).  capacity: room for that many cells instead of n; PcpxError with status PCPX_ERR_CAPACITY (and "count" in its
    `voxels`) when there are more."""
    P = np.ascontiguousarray(points, dtype=np.float32)
    if P.ndim != 2 or P.shape[1] != 3:
        raise ValueError("points must be (points, 3)")
    n = len(P)
    Q = None
    if attrs is not None:
        Q = np.ascontiguousarray(attrs, dtype=np.float32)
        if Q.ndim != 2 or len(Q) != n:
            raise ValueError("attrs must be (points, columns)")
    A = 0 if Q is None else Q.shape[1]
    prm = voxel_params(leaf, origin, A)
    cap = n if capacity is None else int(capacity)
    count, dropped = C.c_uint64(0), C.c_uint64(0)
    xyz, mean = np.zeros((cap, 3), np.float32), np.zeros((cap, A), np.float32)
    counts, keys, rows = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
    owner, org = np.full(n, NONE, np.uint32), np.zeros(3, np.float32)
    st = _capi.load().pcpx_voxel_grid(_vp(P), n, _vp(Q) if A else None, C.byref(prm), cap, device, C.byref(count), _vp(xyz), _vp(mean) if A else None,
                                      _vp(counts), _vp(keys), _vp(rows), _vp(owner), C.byref(dropped), _vp(org))
    try:
        check(st)
    except _capi.PcpxError as e:
        e.voxels = count.value
        raise
    V = count.value
    out = {"points": xyz[:V].copy(), "counts": counts[:V].copy(), "keys": keys[:V].copy(), "rows": rows[:V].copy(), "owner": owner,
           "dropped": dropped.value, "origin": org}
    if A:
        out["attrs"] = mean[:V].copy()
    return out


def voxel_grid_dev(d_points, n, params, capacity, d_count, d_attrs=None, d_xyz=None, d_mean=None, d_counts=None, d_keys=None, d_rows=None,
                   d_owner=None, d_dropped=None, d_origin=None, device=None, stream=None):
    """Device form: points (n, 3) float32, attrs (n, params.attr_columns) float32, params from voxel_params, count and dropped one
    uint64 each, xyz (capacity, 3) and mean (capacity, A) float32, counts and rows (capacity,) uint32, keys (capacity,) uint64, owner
    (n,) uint32, origin 3 float32, as torch tensors or device addresses.  The first min(count, capacity) cells are written.  Enqueued
    on `stream` (default: torch's current stream of the tensors' device, else the null stream) of `device` (default: the tensors',
    else 0) with no synchronisation and no read-back: the centroids can go on to Index(...) with no wait in between."""
    check(_capi.load().pcpx_voxel_grid_dev(_dptr(d_points), int(n), _dptr(d_attrs), C.byref(params), int(capacity), _device_of(device, d_points, d_count),
                                           _stream_of(stream, d_points, d_count),
                                           *(_dptr(d) for d in (d_count, d_xyz, d_mean, d_counts, d_keys, d_rows, d_owner, d_dropped, d_origin))))
