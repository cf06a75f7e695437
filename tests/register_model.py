"""The contract of include/pcpx_register.h restated in numpy, float32 line by line and vectorised over the hypotheses: what the GPU
tests compare with bit for bit.

    records(P, Q, pairs)                         -> (rec (C, 6) float32, origins (6,) float32)
    slots(hs, seed, C)                           -> (len(hs), 3) the sampled correspondences
    pose_of(x0, x1, x2, s2)                      -> the triad alignment of explicit triples of records
    hypotheses(rec, hs, seed, s2)                -> (R (H, 3, 3), t (H, 3), valid (H,))
    scores(R, t, rec, tau2)                      -> inliers of every hypothesis (int64)
    ransac(P, Q, pairs, T, seed, tau2, s2)       -> Result: found, h, score, inliers, transform (16 float64), and every hypothesis's
                                                    validity and score (so that a smaller T is a prefix: best_of)
    rigid_fit(P, Q, pairs[, positions])          -> (transform (16,) float64, rms): Horn's closed form in float64

`pairs` are the C correspondences themselves (the caller cuts the array at min(device count, capacity))."""
import numpy as np

from subsample_model import fmix32

F = np.float32
REFIT = 1
GOLDEN = 0x9E3779B9
IDENTITY = np.eye(4).reshape(16)


def _pairs(pairs):
    return np.asarray(pairs, np.uint32).reshape(-1, 2).astype(np.int64)


def usable(P, Q, pairs):
    """per correspondence: both indices in range and all six coordinates finite"""
    P, Q, pr = np.asarray(P, F).reshape(-1, 3), np.asarray(Q, F).reshape(-1, 3), _pairs(pairs)
    ok = (pr[:, 0] < len(P)) & (pr[:, 1] < len(Q))
    six = np.zeros((len(pr), 6), F)
    six[ok, :3], six[ok, 3:] = P[pr[ok, 0]], Q[pr[ok, 1]]
    ok &= np.isfinite(six).all(1)
    return ok, six


def records(P, Q, pairs):
    ok, six = usable(P, Q, pairs)
    origins = six[0].copy() if len(ok) and ok[0] else np.zeros(6, F)
    with np.errstate(all="ignore"):
        rec = (six - origins[None, :]).astype(F)
    bad = ~ok | ~np.isfinite(rec).all(1)
    rec[bad] = 0
    rec[bad, 0] = np.nan
    return rec, origins


def slots(hs, seed, C):
    w = fmix32(np.asarray(hs, np.uint64) ^ np.uint64(int(seed) & 0xFFFFFFFF))
    out = np.empty((len(w), 3), np.int64)
    for s in range(3):
        x = fmix32((w + np.uint64((s + 1) * GOLDEN)) & np.uint64(0xFFFFFFFF))
        out[:, s] = ((x * np.uint64(C)) >> np.uint64(32)).astype(np.int64)  # (x, C < 2^32: the product fits 64 bits)
    return out


def _len2(a):
    return (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def frames(x0, x1, x2):
    """one side: (F (H, 3, 3) with columns u, v, w; la2, lb2, ld2, lc2)"""
    a, b, d = x1 - x0, x2 - x0, x2 - x1
    la2, lb2, ld2 = _len2(a), _len2(b), _len2(d)
    u = a / np.sqrt(la2)[:, None]
    c = _cross(a, b)
    lc2 = _len2(c)
    w = c / np.sqrt(lc2)[:, None]
    v = _cross(w, u)
    return np.stack([u, v, w], 2), la2, lb2, ld2, lc2


def _positive_finite(x):
    return (x > 0) & (x < np.inf)


def pose_of(x0, x1, x2, s2):
    """the triad alignment of explicit triples, records (H, 6) each: (R (H, 3, 3), t (H, 3), ok (H,): every rule of validity but
    "the slots differ")"""
    x0, x1, x2 = (np.asarray(x, F).reshape(-1, 6) for x in (x0, x1, x2))
    H = len(x0)
    s2 = F(s2)
    with np.errstate(all="ignore"):
        Fp, pa, pb, pd, pc = frames(x0[:, :3], x1[:, :3], x2[:, :3])
        Fq, qa, qb, qd, qc = frames(x0[:, 3:], x1[:, 3:], x2[:, 3:])
        R = np.empty((H, 3, 3), F)
        for r in range(3):
            for c in range(3):
                R[:, r, c] = (Fq[:, r, 0] * Fp[:, c, 0] + Fq[:, r, 1] * Fp[:, c, 1]) + Fq[:, r, 2] * Fp[:, c, 2]
        p0, q0 = x0[:, :3], x0[:, 3:]
        t = np.stack([q0[:, r] - ((R[:, r, 0] * p0[:, 0] + R[:, r, 1] * p0[:, 1]) + R[:, r, 2] * p0[:, 2]) for r in range(3)], 1)
        ok = _positive_finite(pa) & _positive_finite(pc) & _positive_finite(qa) & _positive_finite(qc)
        for lp, lq in ((pa, qa), (pb, qb), (pd, qd)):
            ok &= (lp >= s2 * lq) & (lq >= s2 * lp)
    assert R.dtype == F and t.dtype == F
    return R, t, ok


def hypotheses(rec, hs, seed, s2):
    hs = np.asarray(hs, np.uint64)
    H = len(hs)
    if len(rec) < 3:
        return np.full((H, 3, 3), np.nan, F), np.full((H, 3), np.nan, F), np.zeros(H, bool)
    sl = slots(hs, seed, len(rec))
    R, t, ok = pose_of(rec[sl[:, 0]], rec[sl[:, 1]], rec[sl[:, 2]], s2)
    return R, t, ok & (sl[:, 0] != sl[:, 1]) & (sl[:, 0] != sl[:, 2]) & (sl[:, 1] != sl[:, 2])


def inlier_mask(R, t, rec, tau2):
    """(H, C) bool; R (H, 3, 3), t (H, 3)"""
    p, q = rec[None, :, :3], rec[None, :, 3:]
    with np.errstate(all="ignore"):
        d2 = None
        for r in range(3):
            e = (((R[:, r, 0, None] * p[:, :, 0] + R[:, r, 1, None] * p[:, :, 1]) + R[:, r, 2, None] * p[:, :, 2]) + t[:, r, None]) - q[:, :, r]
            assert e.dtype == F
            d2 = e * e if d2 is None else d2 + e * e  # ((e0 e0 + e1 e1) + e2 e2)
        return d2 <= F(tau2)


def scores(R, t, rec, tau2, chunk=1024):
    out = np.zeros(len(R), np.int64)
    if len(rec):
        for a in range(0, len(R), chunk):
            out[a:a + chunk] = inlier_mask(R[a:a + chunk], t[a:a + chunk], rec, tau2).sum(1)
    return out


def transform64(R, t, origins):
    """the hypothesis as 16 float64: R widened, t_abs in float64"""
    R64, t64, o = R.astype(np.float64), t.astype(np.float64), origins.astype(np.float64)
    out = np.eye(4)
    out[:3, :3] = R64
    for r in range(3):
        out[r, 3] = (o[3 + r] + t64[r]) - ((R64[r, 0] * o[0] + R64[r, 1] * o[1]) + R64[r, 2] * o[2])
    return out.reshape(16)


class Result:
    def __init__(self, rec, origins, R, t, valid, score, tau2):
        self.rec, self.origins, self.R, self.t, self.valid, self.scores, self.tau2 = rec, origins, R, t, valid, score, tau2

    def best_of(self, T):
        """(found, h, score, inliers, transform) among the first T hypotheses"""
        valid = self.valid[:T]
        if not valid.any():
            return 0, 0, 0, np.zeros(0, np.uint32), IDENTITY.copy()
        sc = np.where(valid, self.scores[:T], -1)
        h = int(np.argmax(sc))  # (the first of equal ones: the lowest h)
        inl = np.nonzero(inlier_mask(self.R[h:h + 1], self.t[h:h + 1], self.rec, self.tau2)[0])[0].astype(np.uint32)
        assert len(inl) == sc[h]
        return 1, h, int(sc[h]), inl, transform64(self.R[h], self.t[h], self.origins)


def ransac(P, Q, pairs, T, seed, tau2, s2):
    rec, origins = records(P, Q, pairs)
    R, t, valid = hypotheses(rec, np.arange(T, dtype=np.uint64), seed, s2)
    return Result(rec, origins, R, t, valid, scores(R, t, rec, tau2), tau2)


def horn_matrix(H):
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = H
    return np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                     [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                     [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
                     [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz]])


def rotation_of(qw, qx, qy, qz):
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                     [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                     [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])


def fit_pairs(P, Q, pairs, positions=None):
    """the usable pairs of a fit as float64 (p (n, 3), q (n, 3))"""
    ok, six = usable(P, Q, pairs)
    if positions is not None:
        pos = np.asarray(positions, np.int64)
        pos = pos[pos < len(ok)]
        ok, six = ok[pos], six[pos]
    six = six[ok].astype(np.float64)
    return six[:, :3], six[:, 3:]


def rigid_fit(P, Q, pairs, positions=None):
    p, q = fit_pairs(P, Q, pairs, positions)
    if len(p) < 3:
        return IDENTITY.copy(), np.nan
    pbar, qbar = p.mean(0), q.mean(0)
    H = (p - pbar).T @ (q - qbar)
    val, vec = np.linalg.eigh(horn_matrix(H))
    quat = vec[:, np.argmax(val)]
    R = rotation_of(*(quat / np.linalg.norm(quat)))
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, qbar - R @ pbar
    e = p @ R.T + out[:3, 3] - q
    return out.reshape(16), float(np.sqrt((e * e).sum() / len(p)))
