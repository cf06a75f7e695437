"""A numpy restatement of the keypoint contract of include/pcpx_keypoints.h.  numpy only: no GPU, no package
import.  Sphere membership is the float32 three-rounding rule, from cluster_model.brute_edges (the way tests/subsample_model.py
gets its edges): (src, dst) ordered pairs, the pairs (i, i) included.

    beats(score, j, i)                                  -> j beats i: score_j > score_i, or score_j == score_i and j < i
    local_maxima(n, src, dst, score, ...)               -> keep (bool) over the graph's n vertices; ids: their input indices
    local_maxima_cloud(pts, score, r, ...)              -> keep (bool) by input row; inside: the rows the index holds
    local_maxima_rows(pts, score, rows, r, ...)         -> the verdict for some rows of a large cloud, no list materialised
    local_maxima_two_stage(pts, score, r, ...)          -> keep for a radius whose edge list would be too long
    iss_score(evals, count, g21, g32)                   -> the saliency in float32 from the features' eigenvalues and counts
    iss_saliency_f64(pts, r, g21, g32)                  -> an independent float64 path: eigh of the centred scatter of the brute-force set

The contract: i is kept iff it is a candidate (indexed, score not NaN and >= min_score), no other indexed j in its sphere beats it,
and its sphere holds at least min_neighbours points, itself included."""
import numpy as np

from cluster_model import brute_edges

F = np.float32


def _scores(score):
    """float32, the contract's type -- or float64 left as it is, for the float64 sanity path"""
    score = np.asarray(score)
    return score.reshape(-1) if score.dtype == np.float64 else score.astype(F).reshape(-1)


def beats(score, j, i):
    """elementwise over index arrays j, i; float comparisons, so -0 equals +0 and a NaN on either side is False"""
    score = _scores(score)
    j = np.asarray(j, np.int64)
    i = np.asarray(i, np.int64)
    with np.errstate(invalid="ignore"):
        return (score[j] > score[i]) | ((score[j] == score[i]) & (j < i))


def candidates(score, min_score=-np.inf):
    score = _scores(score)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(score) & (score >= score.dtype.type(min_score))


def local_maxima(n, src, dst, score, min_score=-np.inf, min_neighbours=1, ids=None):
    """keep over the n vertices of the graph (src, dst); score: one float32 per vertex; ids: the input index of every vertex (None:
    vertex v is input row v) -- a graph over the indexed subset of a cloud breaks its ties by the rows it came from.  ids must
    ascend with the vertex number (a subset in input order), so that comparing vertex numbers is comparing input indices."""
    score = _scores(score)
    assert len(score) == n
    if ids is not None:
        ids = np.asarray(ids, np.int64)
        assert (np.diff(ids) > 0).all()
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    count = np.bincount(src, minlength=n)
    count += ~np.isin(np.arange(n), src[src == dst])  # (the centre is in its own sphere whether or not the list names it)
    beaten = np.zeros(n, bool)
    other = src != dst
    beaten[src[other][beats(score, dst[other], src[other])]] = True
    return candidates(score, min_score) & ~beaten & (count >= max(int(min_neighbours), 1))


def local_maxima_cloud(pts, score, r, min_score=-np.inf, min_neighbours=1, inside=None, edges=None):
    """keep by input row.  inside: bool mask of the rows inside the index's voxel grid (None: all); edges: brute_edges(pts[inside], r)
    where the caller has them already."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    score = _scores(score)
    rows = np.arange(len(pts)) if inside is None else np.nonzero(inside)[0]
    src, dst = (brute_edges(pts[rows], r) if edges is None else edges)[:2]
    keep = np.zeros(len(pts), bool)
    keep[rows] = local_maxima(len(rows), src, dst, score[rows], min_score, min_neighbours, ids=rows)
    return keep


def local_maxima_rows(pts, score, rows, r, min_score=-np.inf, min_neighbours=1):
    """The verdict for `rows` alone (every point indexed): each row against the points whose x lies within r and a margin of its
    own -- a superset of what can pass the float32 test."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    score = _scores(score)
    order = np.argsort(pts[:, 0], kind="stable")
    s, key = pts[order], pts[order, 0].astype(np.float64)
    reach = float(r) * (1 + 1e-3) + 8 * float(np.spacing(F(np.abs(key).max() + float(r))))
    r2 = F(r) * F(r)
    cand = candidates(score, min_score)
    out = np.zeros(len(rows), bool)
    for k, i in enumerate(np.asarray(rows, np.int64)):
        if not cand[i]:
            continue
        lo, hi = np.searchsorted(key, [float(pts[i, 0]) - reach, float(pts[i, 0]) + reach])
        d = s[lo:hi] - pts[i][None, :]
        near = order[lo:hi][(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2]
        others = near[near != i]
        out[k] = len(near) >= max(int(min_neighbours), 1) and not beats(score, others, np.full(len(others), i)).any()
    return out


def local_maxima_two_stage(pts, score, r, min_neighbours=1, r_small=None):
    """local_maxima_cloud for a radius whose edge list would be too long: a point that is beaten inside r_small <= r is beaten inside
    r, so only the maxima at r_small (from the edge list) are looked at over the whole radius (local_maxima_rows)."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    assert r_small <= r
    rows = np.nonzero(local_maxima_cloud(pts, score, r_small))[0]
    keep = np.zeros(len(pts), bool)
    keep[rows] = local_maxima_rows(pts, score, rows, r, min_neighbours=min_neighbours)
    return keep


def iss_score(evals, count, g21, g32):
    """saliency in float32: l0 / (float)count where l1 < g21 * l2 and l0 < g32 * l1 (each product and the quotient rounded once),
    NaN elsewhere and where count is 0"""
    ev = np.asarray(evals, F).reshape(-1, 3)
    cnt = np.asarray(count).reshape(-1)
    l0, l1, l2 = ev[:, 0], ev[:, 1], ev[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        ok = (cnt != 0) & (l1 < F(g21) * l2) & (l0 < F(g32) * l1)
        out = l0 / np.maximum(cnt, 1).astype(F)
    assert out.dtype == F
    out[~ok] = F(np.nan)
    return out


def iss_saliency_f64(pts, r, g21, g32, edges=None):
    """float64 throughout and independent of the GPU's eigenvalues: the sphere by the float32 rule, then the centred scatter of the
    set in float64, numpy's eigh, the two strict ratio tests and l0 / count; NaN where a test fails."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    src, dst = (brute_edges(pts, r) if edges is None else edges)[:2]
    p = pts.astype(np.float64)
    count = np.bincount(src, minlength=n).astype(np.float64)
    mean = np.stack([np.bincount(src, p[dst, a], n) for a in range(3)], 1) / count[:, None]
    d = p[dst] - mean[src]
    C = np.empty((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            C[:, a, b] = C[:, b, a] = np.bincount(src, d[:, a] * d[:, b], n)
    w = np.linalg.eigvalsh(C)
    ok = (w[:, 1] < g21 * w[:, 2]) & (w[:, 0] < g32 * w[:, 1])
    return np.where(ok, w[:, 0] / count, np.nan)
