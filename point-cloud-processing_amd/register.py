"""Rigid registration from correspondences over the C ABI (include/pcpx_register.h): the rigid pose that most
of a list of (source, target) pairs agree on -- a fixed number of three-pair hypotheses, each scored against all pairs, every step
defined to the bit -- and the least-squares rigid fit over a list of pairs.

Host arrays in, host values out (`ransac_rigid`, `rigid_fit`); device arrays in and out, enqueued without a synchronisation
(`ransac_rigid_dev`, `rigid_fit_dev`): torch tensors or plain device addresses, so the pairs and the count word that
`match_correspondences_dev` left on the device go straight in.  Transforms are 4 x 4 float64, row-major, and take points of `p` to
points of `q`.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check
from .match import _device_of, _dptr, _stream_of, _vp


def _cloud(a, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s must be (points, 3)" % name)
    return a


def _pair_rows(pairs):
    a = np.ascontiguousarray(pairs, dtype=np.uint32)
    if a.size == 0:
        return a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("pairs must be (count, 2)")
    return a


def _sq(x):
    v = np.float32(x)
    return float(v * v)  # (one float32 product)


def ransac_plan(hypotheses, pairs_capacity):
    """pcpx_ransac_plan: {"segments", "segment_rows", "scratch_bytes"} of a call with that many hypotheses and room for that many pairs."""
    s, r, b = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    check(_capi.load().pcpx_ransac_plan(int(hypotheses), int(pairs_capacity), C.byref(s), C.byref(r), C.byref(b)))
    return {"segments": s.value, "segment_rows": r.value, "scratch_bytes": b.value}


def ransac_rigid(p, q, pairs, hypotheses, max_distance, seed=0, edge_similarity=0.0, refit=True, device=0):
    """The rigid pose most of `pairs` ((C, 2) uint32 rows of p and q, both (n, 3) float32-convertible) agree on, among `hypotheses`
    triad alignments of three sampled pairs: a pair is an inlier when its target lies within max_distance of its moved source
    (max_distance and edge_similarity are squared in float32 here; edge_similarity s in [0, 1] rejects a triple one of whose edges
    is shorter than s times its partner, 0 = no gate).  Ties in the inlier count go to the lowest hypothesis.
    Returns a dict: "found" (bool), "hypothesis", "inliers" (positions into pairs, ascending, uint32), "transform" ((4, 4) float64:
    the winning hypothesis itself) and, with refit (the default, as in pcp::gpu::ransac_rigid), "refit" (the least-squares
    transform over the inliers)."""
    P, Q, pr = _cloud(p, "p"), _cloud(q, "q"), _pair_rows(pairs)
    n = len(pr)
    found, h, score = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    inl = np.empty(n, np.uint32)
    xf, re = np.empty(16, np.float64), np.empty(16, np.float64)
    check(_capi.load().pcpx_ransac_rigid(_vp(P), len(P), _vp(Q), len(Q), _vp(pr), n, int(hypotheses), int(seed) & 0xFFFFFFFF, _sq(max_distance),
                                         _sq(edge_similarity), _capi.PCPX_RANSAC_REFIT if refit else 0, device, C.byref(found), C.byref(h),
                                         C.byref(score), _vp(inl), _vp(xf), _vp(re) if refit else None))
    out = {"found": bool(found.value), "hypothesis": h.value, "inliers": inl[:score.value].copy(), "transform": xf.reshape(4, 4)}
    if refit:
        out["refit"] = re.reshape(4, 4)
    return out


def ransac_rigid_dev(d_p, np_, d_q, nq, d_pairs, pairs_capacity, hypotheses, max_distance, d_found, d_count=None, d_hypothesis=None, d_score=None,
                     d_inliers=None, d_inlier_count=None, d_transform=None, d_refit=None, seed=0, edge_similarity=0.0, device=None, stream=None):
    """Device form: p (np_, 3) and q (nq, 3) float32, pairs uint32 with room for (pairs_capacity, 2), count one uint64 (the word
    match_correspondences_dev leaves; None: all pairs_capacity pairs), found / hypothesis / score one uint32 each, inliers uint32 with
    room for pairs_capacity, inlier_count one uint64, transform and refit 16 float64 each, as torch tensors or device addresses.  A
    refit array asks for the refit.  Enqueued on `stream` (default: torch's current stream of the tensors' device, else the null
    stream) of `device` (default: the tensors', else 0) with no synchronisation and no read-back."""
    check(_capi.load().pcpx_ransac_rigid_dev(_dptr(d_p), int(np_), _dptr(d_q), int(nq), _dptr(d_pairs), int(pairs_capacity), _dptr(d_count),
                                             int(hypotheses), int(seed) & 0xFFFFFFFF, _sq(max_distance), _sq(edge_similarity),
                                             _capi.PCPX_RANSAC_REFIT if d_refit is not None else 0, _device_of(device, d_p, d_q, d_pairs),
                                             _stream_of(stream, d_p, d_q, d_pairs),
                                             *(_dptr(d) for d in (d_found, d_hypothesis, d_score, d_inliers, d_inlier_count, d_transform, d_refit))))


def rigid_fit(p, q, pairs, positions=None, device=0):
    """The rigid transform minimising the sum of |R p + t - q|^2 over `pairs` (or over pairs[positions]), in float64 by Horn's closed
    form; R is always a proper rotation.  Returns ((4, 4) float64, the root mean square residual); the identity and NaN with fewer
    than three usable pairs."""
    P, Q, pr = _cloud(p, "p"), _cloud(q, "q"), _pair_rows(pairs)
    pos = None if positions is None else np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
    xf = np.empty(16, np.float64)
    rms = C.c_double(0)
    # (the C ABI tells "all pairs" from a list by the pointer: an empty list still needs an address, that of a one-word stand-in)
    stand_in = np.zeros(1, np.uint32)
    pos_ptr = None if pos is None else (_vp(pos) if pos.size else _vp(stand_in))
    check(_capi.load().pcpx_rigid_fit(_vp(P), len(P), _vp(Q), len(Q), _vp(pr), len(pr), pos_ptr, 0 if pos is None else len(pos), device, _vp(xf),
                                      C.byref(rms)))
    return xf.reshape(4, 4), rms.value


def rigid_fit_dev(d_p, np_, d_q, nq, d_pairs, pairs_capacity, d_transform, d_count=None, d_positions=None, positions_capacity=0,
                  d_positions_count=None, d_rms=None, device=None, stream=None):
    """Device form of rigid_fit: positions uint32 with room for positions_capacity and positions_count one uint64 (what
    ransac_rigid_dev leaves as inliers and inlier_count), transform 16 float64, rms one float64.  Enqueued as ransac_rigid_dev."""
    check(_capi.load().pcpx_rigid_fit_dev(_dptr(d_p), int(np_), _dptr(d_q), int(nq), _dptr(d_pairs), int(pairs_capacity), _dptr(d_count),
                                          _dptr(d_positions), int(positions_capacity), _dptr(d_positions_count), _device_of(device, d_p, d_q, d_pairs),
                                          _stream_of(stream, d_p, d_q, d_pairs), _dptr(d_transform), _dptr(d_rms)))
