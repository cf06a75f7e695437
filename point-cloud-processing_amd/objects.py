"""Objects from labels over the C ABI (include/pcpx_objects.h): what follows every call that ends in a label per
row -- Index.cluster, Index.segment, extract_planes, the owners of voxel_grid and Index.subsample.  The rows of every label, its size,
centroid, covariance, axis-aligned and oriented box, and the minimum / maximum size filter of PCL's EuclideanClusterExtraction, in
ascending label order and to the bit (the oriented box: given its axes).

Host arrays in, host arrays out (`label_objects`); device arrays in and out, enqueued without a synchronisation
(`label_objects_dev`): torch tensors or plain device addresses.  `objects_plan` is the device scratch such a call takes.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check
from .match import _device_of, _dptr, _stream_of, _vp

NONE = _capi.PCPX_OBJECTS_NONE


def objects_params(none_label=None, min_size=1, max_size=0, on_device=False):
    """pcpx_objects_params: none_label None: every label value is a label; max_size 0: no upper bound."""
    p = _capi.ObjectsParams()
    p.flags = (_capi.PCPX_OBJECTS_ON_DEVICE if on_device else 0) | (_capi.PCPX_OBJECTS_SKIP if none_label is not None else 0)
    p.none_label = 0 if none_label is None else int(none_label)
    p.min_size, p.max_size = int(min_size), int(max_size)
    return p


def objects_plan(n, capacity=None):
    """pcpx_objects_plan: {"sort_bytes", "scratch_bytes"} of a call over n rows with room for `capacity` objects (None: n)."""
    sort, scratch = C.c_uint64(0), C.c_uint64(0)
    check(_capi.load().pcpx_objects_plan(int(n), int(n if capacity is None else capacity), C.byref(sort), C.byref(scratch)))
    return {"sort_bytes": sort.value, "scratch_bytes": scratch.value}


def label_objects(points, labels, none_label=None, min_size=1, max_size=0, capacity=None, device=0):
    """The objects of `labels` ((n,) uint32) over `points` ((n, 3) float32-convertible).  A row is a member iff its coordinates are
    finite and its label is not `none_label`; the distinct labels of the members, ascending, with min_size <= members <= max_size
    (0: unbounded), are the objects.  Returns a dict: "labels", "counts", "first_row" ((S,) uint32), "offsets" ((S + 1,) uint32) and
    "rows" ((offsets[S],) uint32: object o's member rows, ascending, at [offsets[o], offsets[o + 1])), "centroid" ((S, 3) float64),
    "cov" ((S, 6) float64: xx, xy, xz, yy, yz, zz), "aabb" ((S, 6) float32: lo, hi), "obb" ((S, 15) float64: centre, the axes e0, e1,
    e2, the half sizes), "object_of_row" ((n,) uint32, NONE for a row in no object), "skipped".  capacity: room for that many objects
    instead of n; PcpxError with status PCPX_ERR_CAPACITY (and the count in its `objects`) when there are more."""
    P = np.ascontiguousarray(points, dtype=np.float32)
    if P.ndim != 2 or P.shape[1] != 3:
        raise ValueError("points must be (points, 3)")
    n = len(P)
    L = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    if len(L) != n:
        raise ValueError("labels must be (points,)")
    prm = objects_params(none_label, min_size, max_size)
    cap = n if capacity is None else int(capacity)
    count, skipped = C.c_uint64(0), C.c_uint64(0)
    room = max(cap, 1)
    lab, counts, first = np.zeros(room, np.uint32), np.zeros(room, np.uint32), np.zeros(room, np.uint32)
    offsets, rows = np.zeros(room + 1, np.uint32), np.zeros(max(n, 1), np.uint32)
    centroid, cov = np.zeros((room, 3), np.float64), np.zeros((room, 6), np.float64)
    aabb, obb = np.zeros((room, 6), np.float32), np.zeros((room, 15), np.float64)
    owner = np.full(max(n, 1), NONE, np.uint32)
    st = _capi.load().pcpx_label_objects(_vp(P), _vp(L), n, C.byref(prm), cap, device, None, C.byref(count), _vp(lab), _vp(counts), _vp(first),
                                         _vp(offsets), _vp(rows), _vp(centroid), _vp(cov), _vp(aabb), _vp(obb), _vp(owner), C.byref(skipped))
    try:
        check(st)
    except _capi.PcpxError as e:
        e.objects = count.value
        raise
    S = count.value
    return {"labels": lab[:S].copy(), "counts": counts[:S].copy(), "first_row": first[:S].copy(), "offsets": offsets[:S + 1].copy(),
            "rows": rows[:int(offsets[S])].copy(), "centroid": centroid[:S].copy(), "cov": cov[:S].copy(), "aabb": aabb[:S].copy(),
            "obb": obb[:S].copy(), "object_of_row": owner[:n].copy(), "skipped": skipped.value}


def label_objects_dev(d_points, d_labels, n, params, capacity, d_count, d_labels_out=None, d_counts=None, d_first_row=None, d_offsets=None,
                      d_rows=None, d_centroid=None, d_cov=None, d_aabb=None, d_obb=None, d_object_of_row=None, d_skipped=None, device=None,
                      stream=None):
    """Device form: points (n, 3) float32 and labels (n,) uint32, params from objects_params(..., on_device=True), count and skipped
    one uint64 each; labels_out, counts and first_row (capacity,) uint32, offsets (capacity + 1,) uint32, rows and object_of_row (n,)
    uint32, centroid (capacity, 3), cov (capacity, 6) and obb (capacity, 15) float64, aabb (capacity, 6) float32, as torch tensors or
    device addresses.  The first min(count, capacity) objects are written.  Enqueued on `stream` (default: torch's current stream of
    the tensors' device, else the null stream) of `device` (default: the tensors', else 0) with no synchronisation and no
    read-back: the labels of Index.cluster_dev go in and the boxes come out with no wait in between."""
    if not params.flags & _capi.PCPX_OBJECTS_ON_DEVICE:
        raise ValueError("label_objects_dev needs params with PCPX_OBJECTS_ON_DEVICE (objects_params(..., on_device=True))")
    check(_capi.load().pcpx_label_objects(_dptr(d_points), _dptr(d_labels), int(n), C.byref(params), int(capacity), _device_of(device, d_points, d_count),
                                          _stream_of(stream, d_points, d_count),
                                          *(_dptr(d) for d in (d_count, d_labels_out, d_counts, d_first_row, d_offsets, d_rows, d_centroid, d_cov,
                                                               d_aabb, d_obb, d_object_of_row, d_skipped))))
