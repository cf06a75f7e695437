"""Plane detection over the C ABI (include/pcpx_planes.h): the plane most points of a cloud lie on -- a fixed
number of three-point hypotheses, each scored against all points, every step defined to the bit --, the least-squares plane of a set
of points, and the extraction of plane after plane as one enqueued loop.

Host arrays in, host values out (`ransac_plane`, `plane_fit`, `extract_planes`); device arrays in and out, enqueued without a
synchronisation (`ransac_plane_dev`, `plane_fit_dev`, `extract_planes_dev`): torch tensors or plain device addresses.  A plane is
four float64 (n0, n1, n2, d) with n . x + d = 0.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check
from .match import _device_of, _dptr, _stream_of, _vp

NONE = _capi.PCPX_PLANE_NONE


def _cloud(a, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s must be (points, 3)" % name)
    return a


def unit_axis(axis):
    """the axis of the axis gate as the C ABI takes it: normalised in float64, rounded to float32 once"""
    a = np.asarray(axis, np.float64).reshape(3)
    norm = float(np.sqrt((a * a).sum()))
    if not np.isfinite(a).all() or not norm > 0:
        raise ValueError("axis must be finite and not zero")
    return (a / norm).astype(np.float32)


def plane_params(hypotheses, max_distance, seed=0, refit=False, min_normal_cos=None, axis=None, min_axis_cos=0.0, origin_row=None, min_inliers=0,
                 max_planes=0):
    """pcpx_plane_params: min_normal_cos not None turns the normal gate on, axis not None the axis gate (the axis is normalised here)."""
    p = _capi.PlaneParams()
    p.hypotheses, p.seed, p.max_distance = int(hypotheses), int(seed) & 0xFFFFFFFF, float(max_distance)
    p.flags = (_capi.PCPX_PLANE_REFIT if refit else 0) | (_capi.PCPX_PLANE_NORMALS if min_normal_cos is not None else 0) | \
        (_capi.PCPX_PLANE_AXIS if axis is not None else 0)
    p.min_normal_cos = float(min_normal_cos) if min_normal_cos is not None else 0.0
    if axis is not None:
        p.axis[:] = [float(v) for v in unit_axis(axis)]
        p.min_axis_cos = float(min_axis_cos)
    p.origin_row = _capi.PCPX_PLANE_ORIGIN_FIRST if origin_row is None else int(origin_row)
    p.min_inliers, p.max_planes = int(min_inliers), int(max_planes)
    return p


def plane_plan(hypotheses, rows_capacity, normals=False, max_planes=0):
    """pcpx_plane_plan: {"segments", "segment_rows", "scratch_bytes"} of a call with that many hypotheses and room for that many rows
    (max_planes = 0: ransac_plane; else extract_planes)."""
    s, r, b = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    check(_capi.load().pcpx_plane_plan(int(hypotheses), int(rows_capacity), _capi.PCPX_PLANE_NORMALS if normals else 0, int(max_planes),
                                       C.byref(s), C.byref(r), C.byref(b)))
    return {"segments": s.value, "segment_rows": r.value, "scratch_bytes": b.value}


def _list(rows, stand_in):
    """(array or None, pointer, count): the C ABI tells "all rows" from a list by the pointer, so an empty list gets a stand-in's address"""
    if rows is None:
        return None, None, 0
    r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    return r, (_vp(r) if r.size else _vp(stand_in)), len(r)


def ransac_plane(points, hypotheses, max_distance, seed=0, rows=None, normals=None, min_normal_cos=None, axis=None, min_axis_cos=0.0, refit=True,
                 origin_row=None, device=0):
    """The plane most of `points` ((n, 3) float32-convertible; or of points[rows]) lie within max_distance of, among `hypotheses`
    planes through three sampled points.  normals with min_normal_cos: a point counts only where |n . normal| >= min_normal_cos.
    axis with min_axis_cos: only planes with |n . axis| >= min_axis_cos are considered (the ground: axis = up).  Ties in the inlier
    count go to the lowest hypothesis.  Returns a dict: "found" (bool), "hypothesis", "inliers" (rows of points in record order,
    uint32), "plane" ((4,) float64: the winning hypothesis itself) and, with refit (the default, as in pcp::gpu::ransac_plane),
    "refit" (the least-squares plane over the inliers)."""
    P = _cloud(points, "points")
    N = None if min_normal_cos is None else _cloud(normals, "normals")
    stand_in = np.zeros(1, np.uint32)
    r, r_ptr, count = _list(rows, stand_in)
    prm = plane_params(hypotheses, max_distance, seed, refit, min_normal_cos, axis, min_axis_cos, origin_row)
    found, h, score = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    inl = np.empty(len(P) if r is None else count, np.uint32)
    plane, re = np.zeros(4, np.float64), np.zeros(4, np.float64)
    check(_capi.load().pcpx_plane_ransac(_vp(P), len(P), _vp(N), r_ptr, count, C.byref(prm), device, C.byref(found), C.byref(h), C.byref(score),
                                         _vp(inl), _vp(plane), _vp(re) if refit else None))
    out = {"found": bool(found.value), "hypothesis": h.value, "inliers": inl[:score.value].copy(), "plane": plane}
    if refit:
        out["refit"] = re
    return out


def ransac_plane_dev(d_points, n, params, d_found, d_normals=None, d_rows=None, rows_capacity=0, d_rows_count=None, d_hypothesis=None, d_score=None,
                     d_inliers=None, d_inlier_count=None, d_plane=None, d_refit=None, device=None, stream=None):
    """Device form: points (n, 3) float32, normals likewise, rows uint32 with room for rows_capacity and rows_count one uint64 (None:
    all n rows), params from plane_params (PCPX_PLANE_REFIT there asks for d_refit), found / hypothesis / score one uint32 each,
    inliers uint32 with room for rows_capacity (n without rows), inlier_count one uint64, plane and refit 4 float64 each, as torch
    tensors or device addresses.  Enqueued on `stream` (default: torch's current stream of the tensors' device, else the null stream)
    of `device` (default: the tensors', else 0) with no synchronisation and no read-back."""
    check(_capi.load().pcpx_plane_ransac_dev(_dptr(d_points), int(n), _dptr(d_normals), _dptr(d_rows), int(rows_capacity), _dptr(d_rows_count),
                                             C.byref(params), _device_of(device, d_points, d_found), _stream_of(stream, d_points, d_found),
                                             *(_dptr(d) for d in (d_found, d_hypothesis, d_score, d_inliers, d_inlier_count, d_plane, d_refit))))


def plane_fit(points, rows=None, device=0):
    """The least-squares plane of `points` (or of points[rows]) in float64.  Returns ((4,) float64, the root mean square distance);
    zeros and NaN with fewer than three usable rows."""
    P = _cloud(points, "points")
    stand_in = np.zeros(1, np.uint32)
    _r, r_ptr, count = _list(rows, stand_in)
    plane = np.zeros(4, np.float64)
    rms = C.c_double(0)
    check(_capi.load().pcpx_plane_fit(_vp(P), len(P), r_ptr, count, device, _vp(plane), C.byref(rms)))
    return plane, rms.value


def plane_fit_dev(d_points, n, d_plane, d_rows=None, rows_capacity=0, d_rows_count=None, d_rms=None, device=None, stream=None):
    """Device form of plane_fit: rows uint32 with room for rows_capacity and rows_count one uint64 (what ransac_plane_dev leaves as
    inliers and inlier_count), plane 4 float64, rms one float64.  Enqueued as ransac_plane_dev."""
    check(_capi.load().pcpx_plane_fit_dev(_dptr(d_points), int(n), _dptr(d_rows), int(rows_capacity), _dptr(d_rows_count),
                                          _device_of(device, d_points, d_plane), _stream_of(stream, d_points, d_plane), _dptr(d_plane), _dptr(d_rms)))


def extract_planes(points, hypotheses, max_distance, min_inliers, max_planes, seed=0, normals=None, min_normal_cos=None, axis=None,
                   min_axis_cos=0.0, refit=True, device=0):
    """Plane after plane: every round is ransac_plane over the points no earlier plane took, and the loop stops at the first round
    whose best plane has fewer than min_inliers points, or after max_planes.  Returns a dict: "labels" ((n,) uint32, NONE where no
    plane took the point), "planes" ((count, 4) float64), "scores" ((count,) uint32) and, with refit, "refits" ((count, 4))."""
    P = _cloud(points, "points")
    N = None if min_normal_cos is None else _cloud(normals, "normals")
    prm = plane_params(hypotheses, max_distance, seed, refit, min_normal_cos, axis, min_axis_cos, None, min_inliers, max_planes)
    m = max(int(max_planes), 1)
    labels = np.empty(len(P), np.uint32)
    count = C.c_uint32(0)
    planes, refits, scores = np.zeros((m, 4)), np.zeros((m, 4)), np.zeros(m, np.uint32)
    check(_capi.load().pcpx_extract_planes(_vp(P), len(P), _vp(N), C.byref(prm), device, _vp(labels), C.byref(count), _vp(planes),
                                           _vp(refits) if refit else None, _vp(scores)))
    out = {"labels": labels, "planes": planes[:count.value].copy(), "scores": scores[:count.value].copy()}
    if refit:
        out["refits"] = refits[:count.value].copy()
    return out


def extract_planes_dev(d_points, n, params, d_labels, d_count, d_normals=None, d_planes=None, d_refits=None, d_scores=None, device=None, stream=None):
    """Device form: labels (n,) uint32, count one uint32, planes and refits (max_planes, 4) float64, scores (max_planes,) uint32.
    Enqueued whole, as ransac_plane_dev: the unlabelled rows can go on to Index.cluster_dev with no wait in between."""
    check(_capi.load().pcpx_extract_planes_dev(_dptr(d_points), int(n), _dptr(d_normals), C.byref(params), _device_of(device, d_points, d_labels),
                                               _stream_of(stream, d_points, d_labels), _dptr(d_labels), _dptr(d_count), _dptr(d_planes),
                                               _dptr(d_refits), _dptr(d_scores)))
