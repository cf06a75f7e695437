"""The contract of include/pcpx_planes.h restated in numpy, float32 line by line and vectorised over the hypotheses: what the GPU
tests compare with bit for bit.

    records(P, rows, normals, origin_row)        -> (rec (C, 3) float32, row (C,) int64, nrm (C, 3) float32 or None, origin (3,) float32)
    slots(hs, seed, C)                           -> (len(hs), 3) the sampled records (register_model's)
    plane_of(x0, x1, x2)                         -> (n (H, 3), m (H,), lc2 (H,)) of explicit triples of records
    hypotheses(rec, hs, seed, axis, min_axis_cos) -> (n, m, valid)
    inlier_mask(n, m, rec, nrm, tau, cosn)       -> (H, C) bool
    ransac(P, T, seed, tau, ...)                 -> Result: best_of(T) -> (found, h, score, inliers, plane (4,) float64)
    plane_fit(P, rows)                           -> (plane (4,) float64, rms) in float64 by numpy.linalg.eigh
    extract(P, T, seed, tau, min_inliers, max_planes, ...) -> (labels, planes, scores)

`rows` are the C rows themselves (the caller cuts the array at min(device count, capacity)); None: all rows in order."""
import numpy as np

from subsample_model import fmix32
from register_model import slots

F = np.float32
NONE = 0xFFFFFFFF


def seed_of_round(seed, r):
    return int(fmix32(np.array([(int(seed) + r) & 0xFFFFFFFF], np.uint64))[0])


def usable(P, row, normals):
    """per listed row: in range, finite coordinates and (with normals) a finite normal; and the gathered coordinates / normals"""
    P = np.asarray(P, F).reshape(-1, 3)
    row = np.asarray(row, np.int64)
    ok = row < len(P)
    x = np.zeros((len(row), 3), F)
    x[ok] = P[row[ok]]
    ok &= np.isfinite(x).all(1)
    nrm = None
    if normals is not None:
        nrm = np.zeros((len(row), 3), F)
        inr = row < len(P)
        nrm[inr] = np.asarray(normals, F).reshape(-1, 3)[row[inr]]
        ok &= np.isfinite(nrm).all(1)
    return ok, x, nrm


def records(P, rows=None, normals=None, origin_row=None):
    P = np.asarray(P, F).reshape(-1, 3)
    row = np.arange(len(P), dtype=np.int64) if rows is None else np.asarray(rows, np.uint32).astype(np.int64)
    ok, x, nrm = usable(P, row, normals)
    origin = np.zeros(3, F)
    if origin_row is None:
        if len(row) and ok[0]:
            origin = x[0].copy()
    else:
        ok_o, x_o, _n = usable(P, np.array([origin_row], np.int64), normals)
        if ok_o[0]:
            origin = x_o[0].copy()
    with np.errstate(all="ignore"):
        rec = (x - origin[None, :]).astype(F)
    bad = ~ok | ~np.isfinite(rec).all(1)
    rec[bad] = 0
    rec[bad, 0] = np.nan
    if nrm is not None:
        nrm[bad] = 0
    return rec, row, nrm, origin


def _dot3(n, x):
    """(n0*x0 + n1*x1) + n2*x2 over the last axis, float32 when both are"""
    return (n[..., 0] * x[..., 0] + n[..., 1] * x[..., 1]) + n[..., 2] * x[..., 2]


def plane_of(x0, x1, x2):
    x0, x1, x2 = (np.asarray(x, F).reshape(-1, 3) for x in (x0, x1, x2))
    with np.errstate(all="ignore"):
        a, b = x1 - x0, x2 - x0
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        lc2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        n = c / np.sqrt(lc2)[:, None]
        m = _dot3(n, x0)
    assert n.dtype == F and m.dtype == F and lc2.dtype == F
    return n, m, lc2


def hypotheses(rec, hs, seed, axis=None, min_axis_cos=0.0):
    hs = np.asarray(hs, np.uint64)
    H = len(hs)
    if len(rec) < 3:
        return np.full((H, 3), np.nan, F), np.full(H, np.nan, F), np.zeros(H, bool)
    sl = slots(hs, seed, len(rec))
    n, m, lc2 = plane_of(rec[sl[:, 0]], rec[sl[:, 1]], rec[sl[:, 2]])
    valid = (sl[:, 0] != sl[:, 1]) & (sl[:, 0] != sl[:, 2]) & (sl[:, 1] != sl[:, 2]) & (lc2 > 0) & (lc2 < np.inf)
    if axis is not None:
        A = np.asarray(axis, F).reshape(3)
        with np.errstate(all="ignore"):
            valid &= np.abs(_dot3(n, A[None, :])) >= F(min_axis_cos)
    return n, m, valid


def inlier_mask(n, m, rec, nrm, tau, cosn=0.0):
    """(H, C) bool; n (H, 3), m (H,)"""
    with np.errstate(all="ignore"):
        e = _dot3(n[:, None, :], rec[None, :, :]) - m[:, None]
        assert e.dtype == F
        out = np.abs(e) <= F(tau)
        if nrm is not None:
            out &= np.abs(_dot3(n[:, None, :], nrm[None, :, :])) >= F(cosn)
    return out


def scores(n, m, rec, nrm, tau, cosn=0.0, chunk=512):
    out = np.zeros(len(n), np.int64)
    if len(rec):
        for a in range(0, len(n), chunk):
            out[a:a + chunk] = inlier_mask(n[a:a + chunk], m[a:a + chunk], rec, nrm, tau, cosn).sum(1)
    return out


def plane64(n, m, origin):
    """the hypothesis as 4 float64: n widened, d = -(m + n . o) in float64"""
    n64, o = n.astype(np.float64), origin.astype(np.float64)
    return np.array([n64[0], n64[1], n64[2], -(float(m) + ((n64[0] * o[0] + n64[1] * o[1]) + n64[2] * o[2]))])


class Result:
    def __init__(self, rec, row, nrm, origin, n, m, valid, score, tau, cosn):
        self.rec, self.row, self.nrm, self.origin, self.n, self.m, self.valid, self.scores, self.tau, self.cosn = rec, row, nrm, origin, n, m, valid, score, tau, cosn

    def best_of(self, T):
        """(found, h, score, inliers (rows), plane) among the first T hypotheses"""
        valid = self.valid[:T]
        if not valid.any():
            return 0, 0, 0, np.zeros(0, np.uint32), np.zeros(4)
        sc = np.where(valid, self.scores[:T], -1)
        h = int(np.argmax(sc))  # (the first of equal ones: the lowest h)
        inl = np.nonzero(inlier_mask(self.n[h:h + 1], self.m[h:h + 1], self.rec, self.nrm, self.tau, self.cosn)[0])[0]
        assert len(inl) == sc[h]
        return 1, h, int(sc[h]), self.row[inl].astype(np.uint32), plane64(self.n[h], self.m[h], self.origin)


def ransac(P, T, seed, tau, rows=None, normals=None, min_normal_cos=0.0, axis=None, min_axis_cos=0.0, origin_row=None):
    rec, row, nrm, origin = records(P, rows, normals, origin_row)
    n, m, valid = hypotheses(rec, np.arange(T, dtype=np.uint64), seed, axis, min_axis_cos)
    return Result(rec, row, nrm, origin, n, m, valid, scores(n, m, rec, nrm, tau, min_normal_cos), tau, min_normal_cos)


def fit_rows(P, rows=None):
    """the usable rows of a fit as float64 (N, 3), in list order"""
    P = np.asarray(P, F).reshape(-1, 3)
    row = np.arange(len(P), dtype=np.int64) if rows is None else np.asarray(rows, np.uint32).astype(np.int64)
    ok, x, _n = usable(P, row, None)
    return x[ok].astype(np.float64)


def sign_rule(n):
    """the component of largest magnitude positive, the lowest index on ties"""
    j = int(np.argmax(np.abs(n)))
    return -n if n[j] < 0 else n


def plane_fit(P, rows=None, like=None):
    """float64: (plane (4,), rms, eigenvalues ascending); `like`: a normal the sign follows (the RANSAC refit)"""
    x = fit_rows(P, rows)
    if len(x) < 3:
        return np.zeros(4), np.nan, np.zeros(3)
    c = x.mean(0)
    d = x - c
    val, vec = np.linalg.eigh(d.T @ d)
    n = vec[:, 0] / np.linalg.norm(vec[:, 0])
    n = sign_rule(n)
    if like is not None and n @ np.asarray(like, np.float64) < 0:
        n = -n
    e = d @ n
    return np.array([n[0], n[1], n[2], -(n @ c)]), float(np.sqrt((e * e).sum() / len(x))), val


def extract(P, T, seed, tau, min_inliers, max_planes, normals=None, min_normal_cos=0.0, axis=None, min_axis_cos=0.0):
    """round r = ransac over the unlabelled rows in ascending order with seed_r and the origin of row 0"""
    P = np.asarray(P, F).reshape(-1, 3)
    labels = np.full(len(P), NONE, np.uint32)
    planes, score_list = [], []
    for r in range(max_planes):
        live = np.nonzero(labels == NONE)[0].astype(np.uint32)
        res = ransac(P, T, seed_of_round(seed, r), tau, live, normals, min_normal_cos, axis, min_axis_cos, origin_row=0)
        found, _h, score, inl, plane = res.best_of(T)
        if not found or score < min_inliers:
            break
        labels[inl] = r
        planes.append(plane)
        score_list.append(score)
    return labels, np.array(planes).reshape(-1, 4), np.array(score_list, np.uint32)
