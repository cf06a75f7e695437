"""The contract of include/pcpx_fps.h in numpy: farthest point sampling by brute force over all pairs, float32 line by line.  It knows
nothing of leaves, buckets or boxes.  numpy only: no GPU, no package import.

    fps(points, m, start=None, stop_radius=0.0, indexed=None) -> Result(rows, count, d2, min_d2, owner)

`indexed` marks the rows inside the index's voxel grid (default: the rows whose three coordinates are finite).  rows and d2 have
`count` entries, min_d2 and owner one per input row.

    pruned(points, m, block, order, ...) -> (Result, evaluations)

is the same selection the way the kernels do it -- blocks of `block` consecutive points of `order`, each with its float32 min / max
box, a block skipped when box_d2 >= its largest D -- for tests/test_fps_cpu.py: the argument the kernels rest on."""
import collections

import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
INF = F(np.inf)
Result = collections.namedtuple("Result", "rows count d2 min_d2 owner")


def d2_to(points, s):
    """d2(i, s) for every row i: fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) on float32 arrays"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = points - s
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        return (dx * dx + dy * dy) + dz * dz


def _indexed(points, indexed):
    finite = np.isfinite(points).all(1)
    return finite if indexed is None else (np.asarray(indexed, bool) & finite)


def _empty(n):
    return Result(np.zeros(0, np.uint32), 0, np.zeros(0, F), np.full(n, INF, F), np.full(n, NONE, np.uint32))


def fps(points, m, start=None, stop_radius=0.0, indexed=None):
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(points)
    inside = _indexed(points, indexed)
    members = np.flatnonzero(inside)
    if m <= 0 or len(members) == 0:
        return _empty(n)
    s = int(members[0]) if start is None else int(start)
    if not (0 <= s < n):
        raise ValueError("start is no input row")
    if not inside[s]:
        return _empty(n)
    stop2 = F(stop_radius) * F(stop_radius)
    P = points[members]
    D = np.full(len(members), INF, F)
    owner = np.full(len(members), NONE, np.uint32)
    rows, d2 = [s], [INF]
    while True:
        t = len(rows) - 1
        now = d2_to(P, points[s])
        closer = now < D  # strict: the earliest sample keeps a tie
        owner[closer] = t
        D = np.where(closer, now, D)
        if t + 1 >= m:
            break
        far = D.max()
        if not far > stop2:
            break
        s = int(members[np.flatnonzero(D == far)[0]])  # (members ascend: the lowest input index)
        rows.append(s)
        d2.append(far)
    min_d2, own = np.full(n, INF, F), np.full(n, NONE, np.uint32)
    min_d2[members], own[members] = D, owner
    return Result(np.array(rows, np.uint32), len(rows), np.array(d2, F), min_d2, own)


def box_d2(lo, hi, q):
    """csrc/pcpx_device.h box_d2, unfused, for every box: the squared distance from q to the box in float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.maximum(np.maximum(lo - q, q - hi), F(0))
        return (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]


def pruned(points, m, block, order, start=None, stop_radius=0.0):
    """the selection by blocks of `block` consecutive points of `order` (a permutation of the indexed rows)"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    order = np.asarray(order, np.int64)
    n, k = len(points), len(order)
    if m <= 0 or k == 0:
        return _empty(n), 0
    nb = -(-k // block)
    pad = nb * block - k
    ids = np.concatenate([order, np.full(pad, -1)]).reshape(nb, block)
    real = ids >= 0
    Q = np.where(real[:, :, None], points[np.where(real, ids, 0)], F(np.nan))
    lo, hi = np.nanmin(Q, 1).astype(F), np.nanmax(Q, 1).astype(F)
    D = np.where(real, INF, F(0)).astype(F)
    owner = np.full((nb, block), NONE, np.uint32)
    bmax = D.max(1)
    stop2 = F(stop_radius) * F(stop_radius)
    s = int(order.min()) if start is None else int(start)
    if s not in set(order.tolist()):
        return _empty(n), 0
    rows, d2, evaluations = [s], [INF], 0
    while True:
        t = len(rows) - 1
        need = np.flatnonzero(box_d2(lo, hi, points[s]) < bmax)
        evaluations += len(need) * block
        for b in need:
            now = d2_to(Q[b], points[s])
            closer = now < D[b]  # (NaN in a slot that holds no point: false)
            owner[b][closer] = t
            D[b] = np.where(closer, now, D[b])
            bmax[b] = D[b][real[b]].max()
        if t + 1 >= m:
            break
        far = bmax.max()
        if not far > stop2:
            break
        s = int(ids[real & (D == far)].min())
        rows.append(s)
        d2.append(far)
    min_d2, own = np.full(n, INF, F), np.full(n, NONE, np.uint32)
    min_d2[ids[real]], own[ids[real]] = D[real], owner[real]
    return Result(np.array(rows, np.uint32), len(rows), np.array(d2, F), min_d2, own), evaluations


def morton_order(points, rows):
    """`rows` in the order of a 10-bit-per-axis Morton code over their box: curve-consecutive points are spatially compact"""
    rows = np.asarray(rows, np.int64)
    if len(rows) == 0:
        return rows
    p = points[rows].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    q = np.clip(((p - lo) / np.maximum(hi - lo, 1e-300) * 1023).astype(np.uint64), 0, 1023)
    code = np.zeros(len(rows), np.uint64)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return rows[np.argsort(code, kind="stable")]
