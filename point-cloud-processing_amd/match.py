"""Descriptor matching over the C ABI (include/pcpx_match.h): the exact nearest and second nearest row of
`tgt` for every row of `src`, by brute force over all pairs, and the correspondences that pass the ratio and the mutual test.

Host arrays in, host arrays out (`match_nearest`, `match_correspondences`); device arrays in and out, enqueued without a
synchronisation (`match_nearest_dev`, `match_correspondences_dev`): torch tensors or plain device addresses, so what
`Index.fpfh_dev` left on the device goes straight in.  Distances are squared, float32, summed in column order without FMA; ties go to
the lower index.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check

NONE = 0xFFFFFFFF


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _rows(a, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or not 1 <= a.shape[1] <= _capi.PCPX_MATCH_MAX_DIMS:
        raise ValueError("%s must be (rows, dims) with 1 <= dims <= %d" % (name, _capi.PCPX_MATCH_MAX_DIMS))
    return a


def _pair(src, tgt):
    s, t = _rows(src, "src"), _rows(tgt, "tgt")
    if s.shape[1] != t.shape[1]:
        raise ValueError("src and tgt have %d and %d columns" % (s.shape[1], t.shape[1]))
    return s, t


def _flags(skip_zero_rows, mutual=False):
    return (_capi.PCPX_MATCH_SKIP_ZERO_ROWS if skip_zero_rows else 0) | (_capi.PCPX_MATCH_MUTUAL if mutual else 0)


def _ratio_sq(max_ratio):
    r = np.float32(max_ratio)
    return float(r * r)  # (one float32 product)


def match_plan(m, n, dims):
    """pcpx_match_plan: {"width", "segments", "segment_rows", "scratch_bytes"} of a call on m sources and n targets."""
    w, s, r, b = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    check(_capi.load().pcpx_match_plan(int(m), int(n), int(dims), C.byref(w), C.byref(s), C.byref(r), C.byref(b)))
    return {"width": w.value, "segments": s.value, "segment_rows": r.value, "scratch_bytes": b.value}


def match_nearest(src, tgt, skip_zero_rows=False, device=0):
    """For every row of src ((m, dims) float32-convertible) its nearest and second nearest row of tgt ((n, dims)):
    (idx uint32 (m,), d2 float32 (m,), second_idx uint32 (m,), second_d2 float32 (m,)); NONE and +inf where there is none.  A pair
    whose d2 is NaN is skipped; with skip_zero_rows, all-zero rows (descriptors that could not be computed) take no part on either side."""
    s, t = _pair(src, tgt)
    m = len(s)
    idx, idx2 = np.empty(m, np.uint32), np.empty(m, np.uint32)
    d2, d22 = np.empty(m, np.float32), np.empty(m, np.float32)
    check(_capi.load().pcpx_match_nearest(_vp(s), m, _vp(t), len(t), s.shape[1], _flags(skip_zero_rows), device, _vp(idx), _vp(d2), _vp(idx2),
                                          _vp(d22)))
    return idx, d2, idx2, d22


def match_correspondences(src, tgt, max_ratio=1.0, mutual=True, skip_zero_rows=False, device=0):
    """The pairs (i, j) with j the nearest row of tgt to row i of src that pass Lowe's ratio test d_best <= max_ratio * d_second --
    evaluated on squared distances: max_ratio is squared in float32 here and the test is d2_best <= max_ratio^2 * d2_second; 1.0 is no
    test -- and, with mutual, for which i is also the nearest row of src to row j of tgt.
    Returns (pairs uint32 (K, 2), ascending i; d2 float32 (K,))."""
    s, t = _pair(src, tgt)
    m = len(s)
    pairs, d2 = np.empty((m, 2), np.uint32), np.empty(m, np.float32)
    count = C.c_uint64(0)
    check(_capi.load().pcpx_match_correspondences(_vp(s), m, _vp(t), len(t), s.shape[1], _ratio_sq(max_ratio), _flags(skip_zero_rows, mutual),
                                                  device, _vp(pairs), _vp(d2), C.byref(count)))
    k = int(count.value)
    return pairs[:k].copy(), d2[:k].copy()


def _dptr(d):
    """a device array as the C ABI takes it: None, an address, or anything with data_ptr() (a torch tensor)"""
    if d is None:
        return None
    addr = d.data_ptr() if hasattr(d, "data_ptr") else int(d)
    return C.c_void_p(addr) if addr else None


def _stream_of(stream, *arrays):
    """the stream as an address: given, or the current torch stream of the first torch tensor among the arrays, or the null stream"""
    if stream is not None:
        return C.c_void_p(int(getattr(stream, "cuda_stream", stream)) or None)
    for a in arrays:
        if hasattr(a, "is_cuda") and a.is_cuda:
            import torch
            return C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream or None)
    return None


def _device_of(device, *arrays):
    """the device number: given, or that of the first torch tensor among the arrays, or 0"""
    if device is not None:
        return int(device)
    for a in arrays:
        if hasattr(a, "is_cuda") and a.is_cuda:
            return a.device.index or 0
    return 0


def match_nearest_dev(d_src, m, d_tgt, n, dims, d_idx, d_d2=None, d_second_idx=None, d_second_d2=None, skip_zero_rows=False, device=None,
                      stream=None):
    """Device form: src (m, dims) and tgt (n, dims) float32, idx and second_idx uint32 (m,), d2 and second_d2 float32 (m,), as torch
    tensors or device addresses.  Enqueued on `stream` (default: torch's current stream of the tensors' device, else the null
    stream) of `device` (default: the tensors', else 0) with no synchronisation."""
    check(_capi.load().pcpx_match_nearest_dev(_dptr(d_src), int(m), _dptr(d_tgt), int(n), int(dims), _flags(skip_zero_rows), _device_of(device, d_src, d_tgt),
                                              _stream_of(stream, d_src, d_tgt), *(_dptr(d) for d in (d_idx, d_d2, d_second_idx, d_second_d2))))


def match_correspondences_dev(d_src, m, d_tgt, n, dims, d_pairs, d_d2=None, d_count=None, max_ratio=1.0, mutual=True, skip_zero_rows=False,
                              device=None, stream=None):
    """Device form: pairs uint32 with room for (m, 2), d2 float32 with room for m, count one uint64 (entries [0, count) are written;
    max_ratio is squared in float32 as in match_correspondences).  Enqueued as match_nearest_dev: the count stays on the device."""
    check(_capi.load().pcpx_match_correspondences_dev(_dptr(d_src), int(m), _dptr(d_tgt), int(n), int(dims), _ratio_sq(max_ratio),
                                                      _flags(skip_zero_rows, mutual), _device_of(device, d_src, d_tgt), _stream_of(stream, d_src, d_tgt),
                                                      *(_dptr(d) for d in (d_pairs, d_d2, d_count))))
