"""The contract of include/pcpx_shapes.h restated in numpy, float32 (the RANSAC) and float64 (the fits) line by line and vectorised
over the hypotheses: what the GPU tests compare with bit for bit.  Written from the header.

    records(P, N, rows, origin_row)              -> planes_model.records with the normal always present
    hypothesis_of(kind, xa, na, xb, nb)          -> (c (H, 3), u (H, 3), R (H,), lw2 (H,)) of explicit pairs of records
    hypotheses(kind, rec, nrm, hs, seed, gates)  -> (c, u, R, valid)
    inlier_mask(kind, c, u, R, rec, nrm, tau, cosn) -> (H, C) bool; cosn None: no normal gate
    ransac(kind, P, N, T, seed, tau, ...)        -> Result: best_of(T) -> (found, h, score, inliers, model (8,) float64)
    fixed_sum(values)                            -> the column sums of (items, terms) float64 in pcpx_fixed_sum.h's order
    shape_fit(kind, P, N, rows, axis)            -> (model (8,), rms, ok); axis: the cylinder's u given (else numpy.linalg.eigh's)

`rows` are the C rows themselves (the caller cuts the array at min(count, capacity)); None: all rows in order."""
import numpy as np

import planes_model as PM
from register_model import slots

F = np.float32
SPHERE, CYLINDER = "sphere", "cylinder"
FIT_BLOCKS, FIT_THREADS = 64, 256


def records(P, N, rows=None, origin_row=None):
    return PM.records(P, rows, N, origin_row)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], -1)


def across(kind, c, u, x):
    """(e, q) of SCORE for the points x about the shapes (c, u); the shapes' and the points' leading axes broadcast"""
    d = x - c
    if kind == CYLINDER:
        s = _dot3(d, u)
        e = d - s[..., None] * u
    else:
        e = d
    q = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    assert q.dtype == x.dtype
    return e, q


def hypothesis_of(kind, xa, na, xb, nb):
    xa, na, xb, nb = (np.asarray(a, F).reshape(-1, 3) for a in (xa, na, xb, nb))
    with np.errstate(all="ignore"):
        w = _cross(na, nb)
        lw2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
        r = xb - xa
        s = _dot3(_cross(r, nb), w) / lw2
        t = _dot3(_cross(r, na), w) / lw2
        ca = xa + s[:, None] * na
        cb = xb + t[:, None] * nb
        c = F(0.5) * (ca + cb)
        u = w / np.sqrt(lw2)[:, None] if kind == CYLINDER else np.full_like(w, np.nan)
        qa, qb = across(kind, c, u, xa)[1], across(kind, c, u, xb)[1]
        R = F(0.5) * (np.sqrt(qa) + np.sqrt(qb))
    assert c.dtype == F and u.dtype == F and R.dtype == F and lw2.dtype == F
    return c, u, R, lw2


def hypotheses(kind, rec, nrm, hs, seed, radius=(0.0, np.inf), min_normal_sin=0.1, axis=None, min_axis_cos=0.0):
    hs = np.asarray(hs, np.uint64)
    H = len(hs)
    if len(rec) < 2:
        nan = np.full((H, 3), np.nan, F)
        return nan, nan.copy(), np.full(H, np.nan, F), np.zeros(H, bool)
    sl = slots(hs, seed, len(rec))
    c, u, R, lw2 = hypothesis_of(kind, rec[sl[:, 0]], nrm[sl[:, 0]], rec[sl[:, 1]], nrm[sl[:, 1]])
    with np.errstate(all="ignore"):
        valid = (sl[:, 0] != sl[:, 1]) & (lw2 > 0) & (lw2 < np.inf) & (lw2 >= F(min_normal_sin) * F(min_normal_sin))
        valid &= np.isfinite(c).all(1) & np.isfinite(R) & (F(radius[0]) <= R) & (R <= F(radius[1]))
        if axis is not None:
            assert kind == CYLINDER
            valid &= np.abs(_dot3(u, np.asarray(axis, F).reshape(1, 3))) >= F(min_axis_cos)
    return c, u, R, valid


def inlier_mask(kind, c, u, R, rec, nrm, tau, cosn=None):
    """(H, C) bool"""
    with np.errstate(all="ignore"):
        lo = np.maximum(R - F(tau), F(0))
        lo2, hi = lo * lo, R + F(tau)
        hi2 = hi * hi
        e, q = across(kind, c[:, None, :], u[:, None, :], rec[None, :, :])
        out = (lo2[:, None] <= q) & (q <= hi2[:, None])
        if cosn is not None:
            g = _dot3(e, nrm[None, :, :])
            cos2 = F(cosn) * F(cosn)
            assert g.dtype == F
            out &= g * g >= cos2 * q
    return out


def scores(kind, c, u, R, rec, nrm, tau, cosn=None, chunk=256):
    out = np.zeros(len(c), np.int64)
    if len(rec):
        for a in range(0, len(c), chunk):
            out[a:a + chunk] = inlier_mask(kind, c[a:a + chunk], u[a:a + chunk], R[a:a + chunk], rec, nrm, tau, cosn).sum(1)
    return out


def signed_axis(u):
    """the component of largest magnitude positive, the lowest index on ties"""
    big = u[0]
    if abs(u[1]) > abs(big):
        big = u[1]
    if abs(u[2]) > abs(big):
        big = u[2]
    return -u if big < 0 else u


def model64(kind, c, u, R, origin):
    m = np.zeros(8)
    m[:3] = c.astype(np.float64) + origin.astype(np.float64)
    if kind == CYLINDER:
        m[3:6] = signed_axis(u).astype(np.float64)
        m[6] = float(R)
    else:
        m[3] = float(R)
    return m


class Result:
    def __init__(self, kind, rec, row, nrm, origin, c, u, R, valid, score, tau, cosn):
        self.kind, self.rec, self.row, self.nrm, self.origin, self.c, self.u, self.R = kind, rec, row, nrm, origin, c, u, R
        self.valid, self.scores, self.tau, self.cosn = valid, score, tau, cosn

    def best_of(self, T):
        """(found, h, score, inliers (rows), model) among the first T hypotheses"""
        valid = self.valid[:T]
        if not valid.any():
            return 0, 0, 0, np.zeros(0, np.uint32), np.zeros(8)
        sc = np.where(valid, self.scores[:T], -1)
        h = int(np.argmax(sc))  # (the first of equal ones: the lowest h)
        inl = np.nonzero(inlier_mask(self.kind, self.c[h:h + 1], self.u[h:h + 1], self.R[h:h + 1], self.rec, self.nrm, self.tau, self.cosn)[0])[0]
        assert len(inl) == sc[h]
        return 1, h, int(sc[h]), self.row[inl].astype(np.uint32), model64(self.kind, self.c[h], self.u[h], self.R[h], self.origin)


def ransac(kind, P, N, T, seed, tau, rows=None, radius=(0.0, np.inf), min_normal_sin=0.1, min_normal_cos=None, axis=None, min_axis_cos=0.0,
           origin_row=None):
    rec, row, nrm, origin = records(P, N, rows, origin_row)
    c, u, R, valid = hypotheses(kind, rec, nrm, np.arange(T, dtype=np.uint64), seed, radius, min_normal_sin, axis, min_axis_cos)
    return Result(kind, rec, row, nrm, origin, c, u, R, valid, scores(kind, c, u, R, rec, nrm, tau, min_normal_cos), tau, min_normal_cos)


# ---- the fits, float64 ---------------------------------------------------------------------------------------------------------------------
def fixed_sum(values, usable):
    """pcpx_fixed_sum.h's order over the items of a list, (items, terms) float64: thread t of the grid adds its usable items t, t + G,
    ... in ascending order; a block's 256 threads by the tree of offsets 128 ... 1; the 64 blocks in block order"""
    values = np.asarray(values, np.float64)
    items, terms = values.shape
    G = FIT_BLOCKS * FIT_THREADS
    acc = np.zeros((G, terms))
    for a in range(0, items, G):
        part, ok = values[a:a + G], usable[a:a + G]
        acc[:len(part)][ok] = acc[:len(part)][ok] + part[ok]
    tree = acc.reshape(FIT_BLOCKS, FIT_THREADS, terms).copy()
    off = FIT_THREADS // 2
    while off:
        tree[:, :off] = tree[:, :off] + tree[:, off:2 * off]
        off //= 2
    total = np.zeros(terms)
    for b in range(FIT_BLOCKS):
        total = total + tree[b, 0]
    return total


def fit_rows(kind, P, N, rows=None):
    """(x (items, 3) float64, normals (items, 3) float64, usable (items,)) of a fit's list, in list order"""
    P = np.asarray(P, F).reshape(-1, 3)
    row = np.arange(len(P), dtype=np.int64) if rows is None else np.asarray(rows, np.uint32).astype(np.int64)
    ok, x, nrm = PM.usable(P, row, N if kind == CYLINDER else None)
    x = np.where(ok[:, None], x, 0).astype(np.float64)
    nrm = np.zeros_like(x) if nrm is None else np.where(ok[:, None], nrm, 0).astype(np.float64)
    return x, nrm, ok


def _across64(kind, u, y):
    if kind == CYLINDER:
        s = (y[:, 0] * u[0] + y[:, 1] * u[1]) + y[:, 2] * u[2]
        y = y - s[:, None] * u[None, :]
    return y, (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]


def normals_scatter(kind, P, N, rows=None):
    """the 3 x 3 matrix of sum N_a N_b over the usable rows, in the fixed order"""
    _x, nrm, ok = fit_rows(kind, P, N, rows)
    s = fixed_sum(np.stack([nrm[:, 0] * nrm[:, 0], nrm[:, 0] * nrm[:, 1], nrm[:, 0] * nrm[:, 2], nrm[:, 1] * nrm[:, 1], nrm[:, 1] * nrm[:, 2],
                            nrm[:, 2] * nrm[:, 2]], 1), ok)
    return np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])


def shape_fit(kind, P, N=None, rows=None, axis=None, fallback=None):
    """SHAPE FIT: (model (8,), rms, ok).  axis: the cylinder's u as the device found it (its Jacobi sweeps are not restated); None:
    numpy.linalg.eigh's, with the sign rule.  fallback: the model of a degenerate fit (the RANSAC refit's hypothesis); None: zeros."""
    x, nrm, ok = fit_rows(kind, P, N, rows)
    bad = (np.zeros(8) if fallback is None else np.asarray(fallback, np.float64).copy()), np.nan, False
    n = float(ok.sum())
    if n < 4:
        return bad
    with np.errstate(all="ignore"):
        m = fixed_sum(x, ok) / n
        u = np.zeros(3)
        if kind == CYLINDER:
            if axis is None:
                _val, vec = np.linalg.eigh(normals_scatter(kind, P, N, rows))
                axis = PM.sign_rule(vec[:, 0] / np.linalg.norm(vec[:, 0]))
            u = np.asarray(axis, np.float64)
        y, q = _across64(kind, u, x - m[None, :])
        S = fixed_sum(np.stack([y[:, 0] * y[:, 0], y[:, 0] * y[:, 1], y[:, 0] * y[:, 2], y[:, 1] * y[:, 1], y[:, 1] * y[:, 2], y[:, 2] * y[:, 2],
                                y[:, 0] * q, y[:, 1] * q, y[:, 2] * q, q], 1), ok)
        A00, A01, A02, A11, A12, A22 = S[:6]
        b0, b1, b2 = 0.5 * S[6], 0.5 * S[7], 0.5 * S[8]
        if kind == CYLINDER:
            k = 0.5 * ((S[0] + S[3]) + S[5])
            k0, k1, k2 = k * u[0], k * u[1], k * u[2]
            A00, A01, A02 = A00 + k0 * u[0], A01 + k0 * u[1], A02 + k0 * u[2]
            A11, A12 = A11 + k1 * u[1], A12 + k1 * u[2]
            A22 = A22 + k2 * u[2]
        l00 = np.sqrt(A00)
        l10, l20 = A01 / l00, A02 / l00
        p1 = A11 - l10 * l10
        l11 = np.sqrt(p1)
        l21 = (A12 - l20 * l10) / l11
        p2 = A22 - (l20 * l20 + l21 * l21)
        l22 = np.sqrt(p2)
        z0 = b0 / l00
        z1 = (b1 - l10 * z0) / l11
        z2 = (b2 - (l20 * z0 + l21 * z1)) / l22
        c2 = z2 / l22
        c1 = (z1 - l21 * c2) / l11
        c0 = (z0 - (l10 * c1 + l20 * c2)) / l00
        R = np.sqrt(S[9] / n + ((c0 * c0 + c1 * c1) + c2 * c2))
        if not (A00 > 0 and p1 > 0 and p2 > 0 and np.isfinite([c0, c1, c2, R]).all()):
            return bad
        model = np.zeros(8)
        model[:3] = m + np.array([c0, c1, c2])
        if kind == CYLINDER:
            model[3:6], model[6] = u, R
        else:
            model[3] = R
        _e, q2 = _across64(kind, u, x - model[None, :3])
        res = np.sqrt(q2) - R
        rms = np.sqrt(fixed_sum((res * res)[:, None], ok)[0] / n)
    return model, float(rms), True
