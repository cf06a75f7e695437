"""Sphere and cylinder detection over the C ABI (include/pcpx_shapes.h): the sphere or the cylinder most points
of a cloud lie on -- a fixed number of hypotheses from two oriented points each, every one scored against all points, every step
defined to the bit and none depending on the normals' signs --, and the closed-form least-squares sphere or cylinder of a set.

Host arrays in, host values out (`ransac_sphere`, `ransac_cylinder`, `sphere_fit`, `cylinder_fit`); device arrays in and out, enqueued
without a synchronisation (`ransac_shape_dev`, `shape_fit_dev`): torch tensors or plain device addresses.  A model is eight float64:
a sphere (cx, cy, cz, R, 0, 0, 0, 0), a cylinder (px, py, pz, ux, uy, uz, R, 0).
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check
from .match import _device_of, _dptr, _stream_of, _vp
from .planes import _cloud, _list, unit_axis

SPHERE, CYLINDER = _capi.PCPX_SHAPE_SPHERE, _capi.PCPX_SHAPE_CYLINDER
_KINDS = {"sphere": SPHERE, "cylinder": CYLINDER, SPHERE: SPHERE, CYLINDER: CYLINDER}


def shape_params(kind, hypotheses, max_distance, seed=0, radius=(0.0, np.inf), min_normal_sin=0.1, min_normal_cos=None, axis=None,
                 min_axis_cos=0.0, refit=False, origin_row=None, on_device=False):
    """pcpx_shape_params: kind "sphere" or "cylinder"; radius = (lo, hi); min_normal_cos not None turns the normal gate on, axis not
    None the axis gate (cylinders; the axis is normalised here); on_device: the arrays of the call are device arrays."""
    p = _capi.ShapeParams()
    p.kind = _KINDS[kind]
    p.hypotheses, p.seed, p.max_distance = int(hypotheses), int(seed) & 0xFFFFFFFF, float(max_distance)
    p.min_radius, p.max_radius, p.min_normal_sin = float(radius[0]), float(radius[1]), float(min_normal_sin)
    p.flags = (_capi.PCPX_SHAPE_REFIT if refit else 0) | (_capi.PCPX_SHAPE_NORMALS if min_normal_cos is not None else 0) | \
        (_capi.PCPX_SHAPE_AXIS if axis is not None else 0) | (_capi.PCPX_SHAPE_ON_DEVICE if on_device else 0)
    p.min_normal_cos = float(min_normal_cos) if min_normal_cos is not None else 0.0
    if axis is not None:
        p.axis[:] = [float(v) for v in unit_axis(axis)]
        p.min_axis_cos = float(min_axis_cos)
    p.origin_row = _capi.PCPX_SHAPE_ORIGIN_FIRST if origin_row is None else int(origin_row)
    return p


def shape_plan(hypotheses, rows_capacity):
    """pcpx_shape_plan: {"segments", "segment_rows", "scratch_bytes"} of a call with that many hypotheses and room for that many rows."""
    s, r, b = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    check(_capi.load().pcpx_shape_plan(int(hypotheses), int(rows_capacity), C.byref(s), C.byref(r), C.byref(b)))
    return {"segments": s.value, "segment_rows": r.value, "scratch_bytes": b.value}


def _ransac(kind, points, normals, hypotheses, max_distance, seed, rows, radius, min_normal_sin, min_normal_cos, axis, min_axis_cos, refit, origin_row,
            device):
    P, N = _cloud(points, "points"), _cloud(normals, "normals")
    if len(N) != len(P):
        raise ValueError("normals must have a row per point")
    stand_in = np.zeros(1, np.uint32)
    r, r_ptr, count = _list(rows, stand_in)
    prm = shape_params(kind, hypotheses, max_distance, seed, radius, min_normal_sin, min_normal_cos, axis, min_axis_cos, refit, origin_row)
    found, h, score, ninl = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    inl = np.empty(len(P) if r is None else count, np.uint32)
    model, re = np.zeros(8, np.float64), np.zeros(8, np.float64)
    check(_capi.load().pcpx_shape_ransac(_vp(P), len(P), _vp(N), r_ptr, count, None, C.byref(prm), device, None, C.byref(found), C.byref(h),
                                         C.byref(score), _vp(inl), C.byref(ninl), _vp(model), _vp(re) if refit else None))
    out = {"found": bool(found.value), "hypothesis": h.value, "inliers": inl[:ninl.value].copy(), "model": model}
    if refit:
        out["refit"] = re
    best = re if refit else model
    if kind == "sphere":
        out.update(center=best[:3].copy(), radius=float(best[3]))
    else:
        out.update(point=best[:3].copy(), axis=best[3:6].copy(), radius=float(best[6]))
    return out


def ransac_sphere(points, normals, hypotheses, max_distance, seed=0, rows=None, radius=(0.0, np.inf), min_normal_sin=0.1, min_normal_cos=None,
                  refit=True, origin_row=None, device=0):
    """The sphere most of `points` ((n, 3) float32-convertible; or of points[rows]) lie within max_distance of, among `hypotheses`
    spheres from two sampled points and their `normals` (unit vectors of either sign).  radius = (lo, hi): only spheres of such a
    radius; min_normal_sin: the two sampled normals span at least that sine; min_normal_cos: a point counts only where its normal is
    within that cosine of the sphere's.  Ties in the inlier count go to the lowest hypothesis.  Returns a dict: "found", "hypothesis",
    "inliers" (rows of points in record order, uint32), "model" ((8,) float64: the winning hypothesis itself), with refit (the
    default) "refit" (the least-squares sphere over the inliers), and "center" and "radius" of the refit if asked for, else of the
    hypothesis."""
    return _ransac("sphere", points, normals, hypotheses, max_distance, seed, rows, radius, min_normal_sin, min_normal_cos, None, 0.0, refit, origin_row,
                   device)


def ransac_cylinder(points, normals, hypotheses, max_distance, seed=0, rows=None, radius=(0.0, np.inf), min_normal_sin=0.1, min_normal_cos=None,
                    axis=None, min_axis_cos=0.0, refit=True, origin_row=None, device=0):
    """The cylinder, as ransac_sphere; axis with min_axis_cos: only cylinders whose axis u has |u . axis| >= min_axis_cos (poles: axis
    = up).  Returns "point", "axis" and "radius" in place of "center" and "radius"."""
    return _ransac("cylinder", points, normals, hypotheses, max_distance, seed, rows, radius, min_normal_sin, min_normal_cos, axis, min_axis_cos, refit,
                   origin_row, device)


def ransac_shape_dev(d_points, n, d_normals, params, d_found, d_rows=None, rows_capacity=0, d_rows_count=None, d_hypothesis=None, d_score=None,
                     d_inliers=None, d_inlier_count=None, d_model=None, d_refit=None, device=None, stream=None):
    """Device form: points and normals (n, 3) float32, rows uint32 with room for rows_capacity and rows_count one uint64 (None: all n
    rows), params from shape_params(..., on_device=True) (refit there asks for d_refit), found / hypothesis / score one uint32 each,
    inliers uint32 with room for rows_capacity (n without rows), inlier_count one uint64, model and refit 8 float64 each, as torch
    tensors or device addresses.  Enqueued on `stream` (default: torch's current stream of the tensors' device, else the null stream)
    of `device` (default: the tensors', else 0) with no synchronisation and no read-back."""
    if not params.flags & _capi.PCPX_SHAPE_ON_DEVICE:
        raise ValueError("params without on_device=True")
    check(_capi.load().pcpx_shape_ransac(_dptr(d_points), int(n), _dptr(d_normals), _dptr(d_rows), int(rows_capacity), _dptr(d_rows_count),
                                         C.byref(params), _device_of(device, d_points, d_found), _stream_of(stream, d_points, d_found),
                                         *(_dptr(d) for d in (d_found, d_hypothesis, d_score, d_inliers, d_inlier_count, d_model, d_refit))))


def _fit(kind, points, normals, rows, device):
    P = _cloud(points, "points")
    N = _cloud(normals, "normals") if kind == CYLINDER else None
    stand_in = np.zeros(1, np.uint32)
    _r, r_ptr, count = _list(rows, stand_in)
    model = np.zeros(8, np.float64)
    rms, status = C.c_double(0), C.c_uint32(0)
    check(_capi.load().pcpx_shape_fit(_vp(P), len(P), _vp(N), r_ptr, count, None, kind, 0, device, None, _vp(model), C.byref(rms), C.byref(status)))
    return model, rms.value, status.value == _capi.PCPX_SHAPE_FIT_OK


def sphere_fit(points, rows=None, device=0):
    """The algebraic least-squares sphere of `points` (or of points[rows]) in float64.  Returns (model (8,) float64, the root mean
    square of the radial distances, ok); zeros, NaN and False for a degenerate set (fewer than four usable rows, coincident points)."""
    return _fit(SPHERE, points, None, rows, device)


def cylinder_fit(points, normals, rows=None, device=0):
    """The least-squares cylinder: the axis the `normals` span least, and the least-squares circle across it.  Returns as sphere_fit."""
    return _fit(CYLINDER, points, normals, rows, device)


def shape_fit_dev(kind, d_points, n, d_model, d_normals=None, d_rows=None, rows_capacity=0, d_rows_count=None, d_rms=None, d_status=None, device=None,
                  stream=None):
    """Device form of sphere_fit / cylinder_fit (kind "sphere" or "cylinder"): rows uint32 with room for rows_capacity and rows_count
    one uint64 (what ransac_shape_dev leaves as inliers and inlier_count), model 8 float64, rms one float64, status one uint32.
    Enqueued as ransac_shape_dev."""
    check(_capi.load().pcpx_shape_fit(_dptr(d_points), int(n), _dptr(d_normals), _dptr(d_rows), int(rows_capacity), _dptr(d_rows_count), _KINDS[kind],
                                      _capi.PCPX_SHAPE_ON_DEVICE, _device_of(device, d_points, d_model), _stream_of(stream, d_points, d_model),
                                      _dptr(d_model), _dptr(d_rms), _dptr(d_status)))
