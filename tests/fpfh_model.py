"""The numpy restatement of include/pcpx_descriptors.h: the pair feature and its bins in float32, statement by
statement as the header writes them, the SPFH counts over float32 brute-force spheres, and the FPFH of a point in float64 from
given SPFH rows.  numpy only: no GPU.  Arrays of float32 keep every numpy operation in float32, one rounding each; np.sqrt and /
are correctly rounded."""
import numpy as np

F = np.float32
BINS, SIZE = 11, 33
_K = np.array([1, 3, 5, 7, 9]) * np.pi / 11
COS = np.cos(_K).astype(F)  # PCPX_FPFH_COS_INIT
SIN = np.sin(_K).astype(F)  # PCPX_FPFH_SIN_INIT


def sector_bin(x, y):
    """b1 of the header from float32 arrays x, y (no NaN): 5 +- #{i : COS[i] |y| - SIN[i] x >= 0}, + where y >= 0."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    ay = np.abs(y)
    k = np.zeros(x.shape, np.int64)
    for c, s in zip(COS, SIN):
        k += (c * ay - s * x >= 0)
    return np.where(y >= 0, 5 + k, 5 - k)


def value_bin(f):
    """trunc(min(max((f + 1) * 5.5, 0), 10)) in float32"""
    u = (np.asarray(f, F) + F(1)) * F(5.5)
    return np.minimum(np.maximum(u, F(0)), F(10)).astype(np.int64)


def pair_features(pi, ni, pj, nj):
    """The header's lines for pairs (i, j), arrays of shape (m, 3) float32.  Returns (kept, f3, f2, x, y, swapped): kept = the pair
    is not skipped; the others are float32 and meaningless where kept is False."""
    pi, ni, pj, nj = (np.asarray(a, F).reshape(-1, 3) for a in (pi, ni, pj, nj))
    with np.errstate(all="ignore"):
        dx, dy, dz = pj[:, 0] - pi[:, 0], pj[:, 1] - pi[:, 1], pj[:, 2] - pi[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        ai = (ni[:, 0] * dx + ni[:, 1] * dy) + ni[:, 2] * dz
        aj = (nj[:, 0] * dx + nj[:, 1] * dy) + nj[:, 2] * dz
        swap = np.abs(ai) < np.abs(aj)
        ex, ey, ez = np.where(swap, -dx, dx), np.where(swap, -dy, dy), np.where(swap, -dz, dz)
        a = np.where(swap, -aj, ai)
        ns = np.where(swap[:, None], nj, ni)
        nt = np.where(swap[:, None], ni, nj)
        f3 = a / np.sqrt(d2)
        vx = ey * ns[:, 2] - ez * ns[:, 1]
        vy = ez * ns[:, 0] - ex * ns[:, 2]
        vz = ex * ns[:, 1] - ey * ns[:, 0]
        vv = (vx * vx + vy * vy) + vz * vz
        vl = np.sqrt(vv)
        f2 = ((vx * nt[:, 0] + vy * nt[:, 1]) + vz * nt[:, 2]) / vl
        wx = ns[:, 1] * vz - ns[:, 2] * vy
        wy = ns[:, 2] * vx - ns[:, 0] * vz
        wz = ns[:, 0] * vy - ns[:, 1] * vx
        y = (wx * nt[:, 0] + wy * nt[:, 1]) + wz * nt[:, 2]
        x = ((ns[:, 0] * nt[:, 0] + ns[:, 1] * nt[:, 1]) + ns[:, 2] * nt[:, 2]) * vl
        kept = (d2 != 0) & (vv != 0) & ~(np.isnan(f3) | np.isnan(f2) | np.isnan(x) | np.isnan(y))
    for v in (d2, f3, f2, x, y):
        assert v.dtype == F
    return kept, f3, f2, x, y, swap


def pair_bins(pi, ni, pj, nj):
    """(kept, b1, b2, b3): the three bins (0 .. 10 each) of every pair; meaningless where kept is False."""
    kept, f3, f2, x, y, _ = pair_features(pi, ni, pj, nj)
    safe = lambda v: np.where(kept, v, F(0))
    return kept, sector_bin(safe(x), safe(y)), value_bin(safe(f2)), value_bin(safe(f3))


def sphere(pts, i, r, inside=None):
    """(the indexed points j != i inside i's sphere by the float32 rule, their float32 d2)"""
    d = pts - pts[i][None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    ok = d2 <= F(r) * F(r)
    if inside is not None:
        ok &= inside
    ok[i] = False
    j = np.nonzero(ok)[0]
    return j, d2[j]


def spfh_counts(pts, normals, i, r, inside=None):
    """(count[33] int64, pairs) of point i: over its pairs that are not skipped"""
    j, _ = sphere(pts, i, r, inside)
    count = np.zeros(SIZE, np.int64)
    if len(j) == 0:
        return count, 0
    m = len(j)
    kept, b1, b2, b3 = pair_bins(np.repeat(pts[i][None], m, 0), np.repeat(normals[i][None], m, 0), pts[j], normals[j])
    count[:BINS] = np.bincount(b1[kept], minlength=BINS)
    count[BINS:2 * BINS] = np.bincount(b2[kept], minlength=BINS)
    count[2 * BINS:] = np.bincount(b3[kept], minlength=BINS)
    return count, int(kept.sum())


def spfh_from_counts(count, pairs):
    """float32 (100 * (float)count) / (float)pairs; zeros when pairs = 0"""
    if pairs == 0:
        return np.zeros(SIZE, F)
    return (F(100) * np.asarray(count).astype(F)) / F(pairs)


def spfh(pts, normals, rows, r, inside=None):
    """(spfh float32 (len(rows), 33), pairs uint32) of the given rows; a row outside `inside` gets zeros"""
    pts, normals = np.asarray(pts, F), np.asarray(normals, F)
    out = np.zeros((len(rows), SIZE), F)
    pairs = np.zeros(len(rows), np.uint32)
    for k, i in enumerate(rows):
        if inside is not None and not inside[i]:
            continue
        count, pairs[k] = spfh_counts(pts, normals, i, r, inside)
        out[k] = spfh_from_counts(count, int(pairs[k]))
    return out, pairs


def fpfh_f64(spfh_rows, d2):
    """float64: the contract's FPFH of one point from the SPFH rows (k, 33) of the points of its sphere and their float32 d2 (the
    points at d2 = 0 left out): T[b] = sum spfh_j[b] / d2_j, every block of 11 scaled to sum 100 (0 where the block's sum is 0)."""
    spfh_rows = np.asarray(spfh_rows, np.float64).reshape(-1, SIZE)
    d2 = np.asarray(d2, np.float64)
    use = d2 > 0
    T = (spfh_rows[use] / d2[use][:, None]).sum(0) if use.any() else np.zeros(SIZE)
    out = np.zeros(SIZE)
    for f in range(3):
        blk = T[f * BINS:(f + 1) * BINS]
        s = blk.sum()
        if s > 0:
            out[f * BINS:(f + 1) * BINS] = 100.0 * (blk / s)
    return out


def fpfh(pts, normals, rows, r, inside=None):
    """float64 FPFH (len(rows), 33) of the given rows from the model's own float32 SPFH: for small hand-made sets"""
    pts, normals = np.asarray(pts, F), np.asarray(normals, F)
    out = np.zeros((len(rows), SIZE))
    for k, i in enumerate(rows):
        if inside is not None and not inside[i]:
            continue
        j, d2 = sphere(pts, i, r, inside)
        out[k] = fpfh_f64(spfh(pts, normals, j, r, inside)[0], d2)
    return out


def bound(n_sphere):
    """The relative error bound of a float32 FPFH bin against fpfh_f64: (n + 16) 2^-23"""
    return (n_sphere + 16) * 2.0 ** -23


PLANE_SIGNATURE = np.zeros(SIZE)
PLANE_SIGNATURE[[5, 16, 27]] = 100.0  # a flat neighbourhood with its normals: theta = 0, f2 = 0, f3 = 0
