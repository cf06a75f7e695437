"""The contract of include/pcpx_outliers.h in numpy (no GPU): the mean distance to the k nearest neighbours with the library's
float32 arithmetic and row order, the library's one fixed float64 summation order (csrc/pcpx_fixed_sum.h), and on them the
resolution and the statistical, radius and density filters.  tests/test_outliers_cpu.py checks it on hand-made sets;
tests/test_gpu_outliers.py holds the device to it bit for bit."""
import numpy as np

F = np.float32
FIT_BLOCKS, FIT_THREADS = 64, 256


def _d2(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def mean_knn_distance(pts, k, eps=1e-5, chunk=512):
    """float32 (n,): for every point the mean distance to its k nearest other points -- those outside its eps-box (max |d| >= eps),
    ascending in (d2, index), d = p_j - p_i with three float32 roundings and no FMA; the float32 sum of sqrt(d2) in that order from
    zero, divided by the float32 number found; NaN where nothing is found.  Brute force: small clouds of finite points."""
    pts = np.ascontiguousarray(pts, F)
    n = len(pts)
    out = np.empty(n, F)
    for a in range(0, n, chunk):
        q = pts[a:a + chunk]
        d = pts[None, :, :] - q[:, None, :]
        d2 = _d2(d)
        d2 = np.where(np.abs(d).max(-1) >= F(eps), d2, F(np.inf))
        order = np.lexsort((np.broadcast_to(np.arange(n), d2.shape), d2), axis=1)[:, :k]  # (d2, index)
        v = np.take_along_axis(d2, order, 1)
        found = np.isfinite(v)
        total = np.zeros(len(q), F)
        for j in range(v.shape[1]):
            total = total + np.where(found[:, j], np.sqrt(np.where(found[:, j], v[:, j], F(0))), F(0))
        with np.errstate(invalid="ignore", divide="ignore"):
            out[a:a + chunk] = total / found.sum(1).astype(F)
    return out


def fixed_sum(items64):
    """The float64 sum of the items in the library's one fixed order: thread t of block b adds items (b 256 + t) + j 64 256,
    j = 0, 1, ..., ascending from zero; a block's 256 threads are added by a tree with offsets 128, 64, ..., 1; the 64 block sums are
    added in block order from zero."""
    x = np.asarray(items64, np.float64).reshape(-1)
    grid = FIT_BLOCKS * FIT_THREADS
    rounds = -(-len(x) // grid) if len(x) else 0
    padded = np.zeros(max(rounds, 1) * grid, np.float64)  # (adding +0.0 changes no bit of a sum that started from +0.0)
    padded[:len(x)] = x
    acc = np.zeros(grid, np.float64)
    for row in padded.reshape(-1, grid):
        acc = acc + row
    tree = acc.reshape(FIT_BLOCKS, FIT_THREADS).copy()
    off = FIT_THREADS // 2
    while off > 0:
        tree[:, :off] = tree[:, :off] + tree[:, off:2 * off]
        off //= 2
    total = np.float64(0.0)
    for b in range(FIT_BLOCKS):
        total = total + tree[b, 0]
    return total


def resolution(d, indexed=None):
    """(mean, std, m, usable mask) of the float32 mean distances d: the usable rows are the indexed ones with a finite d."""
    d = np.asarray(d, F)
    usable = np.isfinite(d) if indexed is None else np.isfinite(d) & np.asarray(indexed, bool)
    m = int(usable.sum())
    d64 = d.astype(np.float64)
    s1 = fixed_sum(np.where(usable, d64, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(s1) / np.float64(m)
        e = np.where(usable, d64, mean) - mean
        s2 = fixed_sum(np.where(usable, e * e, 0.0))
        if m >= 2:
            std = np.sqrt(s2 / np.float64(m - 1))
        else:
            std = np.float64(0.0) if m == 1 else np.float64(np.nan)
    return mean, std, m, usable


def statistical(d, indexed=None, std_ratio=2.0):
    """(keep, stats float64 (4,), cut float32): keep = usable and d <= cut in float32, cut = float32(mean + float64(float32 ratio) std)"""
    mean, std, m, usable = resolution(d, indexed)
    with np.errstate(invalid="ignore"):
        cut = F(mean + np.float64(F(std_ratio)) * std)
        keep = usable & (np.asarray(d, F) <= cut)
    return keep, np.array([mean, std, np.float64(cut), m], np.float64), cut


def range_count(pts, indexed, r):
    """uint32 (n,): the indexed points within r of every indexed point, itself included (d2 <= r r in float32); 0 for the others"""
    pts = np.ascontiguousarray(pts, F)
    indexed = np.ones(len(pts), bool) if indexed is None else np.asarray(indexed, bool)
    r2 = F(r) * F(r)
    cnt = np.zeros(len(pts), np.uint32)
    inside = pts[indexed]
    rows = np.nonzero(indexed)[0]
    with np.errstate(invalid="ignore"):
        for a in range(0, len(rows), 512):
            d = inside[None, :, :] - inside[a:a + 512, None, :]
            cnt[rows[a:a + 512]] = (_d2(d) <= r2).sum(1)
    return cnt


def radius(pts, indexed, r, min_neighbours=5):
    """(keep, count): keep = indexed and count >= max(min_neighbours, 1)"""
    cnt = range_count(pts, indexed, r)
    return cnt >= max(int(min_neighbours), 1), cnt


def density(pts, d, indexed=None, radius_scale=1.0, min_neighbours=5):
    """(keep, stats, r float32, count): the radius filter at r = float32(float64(float32 scale) mean); a NaN r keeps nothing"""
    mean, std, m, _usable = resolution(d, indexed)
    with np.errstate(invalid="ignore"):
        r = F(np.float64(F(radius_scale)) * mean)
    keep, cnt = radius(pts, indexed, r, min_neighbours)
    return keep, np.array([mean, std, np.float64(r), m], np.float64), r, cnt
