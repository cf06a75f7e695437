"""The contract of include/pcpx_boundary.h in numpy (no GPU), brute force over all pairs: the sphere of pcpx_range_count_*, the frame
(u, v) of a normal, the sector of a direction by the seven compares, the sector mask as an OR, the longest cyclic run of empty
sectors and its start by counting, and the keep rule.  float32 throughout, one rounding per operation.
tests/test_boundary_cpu.py checks it on hand-made sets; tests/test_gpu_boundary.py holds the device to it bit for bit."""
import numpy as np

F = np.float32
SECTORS = 64
# T_k, k = 1 .. 7: the hexadecimal floats of the header
TANS = np.array([float.fromhex(h) for h in ("0x1.936bb8p-4", "0x1.975f5ep-3", "0x1.36a084p-2", "0x1.a8279ap-2", "0x1.11ab72p-1",
                                            "0x1.561b82p-1", "0x1.a43002p-1")], F)
NO_FRAME = 255


def frames(normals):
    """(has_frame bool (n,), u float32 (n, 3), v float32 (n, 3)); u = v = 0 where there is no frame"""
    n = np.ascontiguousarray(normals, F).reshape(-1, 3)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    has = np.isfinite(n).all(1) & ~(n == 0).all(1)
    with np.errstate(invalid="ignore"):
        ax, ay, az = np.abs(nx), np.abs(ny), np.abs(nz)
        first = (ax <= ay) & (ax <= az)
        second = ~first & (ay <= az)
        zero = np.zeros_like(nx)
        u = np.where(first[:, None], np.stack([zero, -nz, ny], 1), np.where(second[:, None], np.stack([-nz, zero, nx], 1), np.stack([-ny, nx, zero], 1)))
        u = np.where(has[:, None], u, F(0)).astype(F)
        nn = np.where(has[:, None], n, F(0)).astype(F)
        nx, ny, nz = nn[:, 0], nn[:, 1], nn[:, 2]
        ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
        v = np.stack([ny * uz - nz * uy, nz * ux - nx * uz, nx * uy - ny * ux], 1).astype(F)
    return has, u, v


def sector(a, b):
    """the sector 0 .. 63 of every direction (a, b) (float32 arrays; where both are 0 the value means nothing)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(invalid="ignore", over="ignore"):
        fa, fb = np.abs(a), np.abs(b)
        swap = fb > fa
        x, y = np.where(swap, fb, fa), np.where(swap, fa, fb)
        sub = np.zeros(a.shape, np.int64)
        for t in TANS:
            sub += y >= t * x
        q = np.where(swap, 15 - sub, sub)
        return np.where(b < 0, np.where(a < 0, 32 + q, 63 - q), np.where(a < 0, 31 - q, q))


def gap_and_start(masks):
    """(G, start) uint8 arrays of the uint64 masks: the longest cyclic run of zero bits and the lowest start of a run that long"""
    masks = np.asarray(masks, np.uint64).reshape(-1)
    bits = ((masks[:, None] >> np.arange(SECTORS, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    free = ~bits
    run = np.zeros(bits.shape, np.int16)  # run[i, s] = the zero bits from s on, cyclic, at most 64
    alive = np.ones(bits.shape, bool)
    for k in range(SECTORS):
        alive &= np.roll(free, -k, axis=1)
        run += alive
    G = run.max(1)
    starts = free & np.roll(bits, 1, axis=1) & (run == G[:, None])  # bit s clear, bit s - 1 set, a run of G from s
    start = np.where(starts.any(1), starts.argmax(1), 0)  # (the mask 0 and the full mask: no such s, 0)
    return G.astype(np.uint8), start.astype(np.uint8)


def boundary(pts, normals, radius, gap_sectors=16, min_neighbours=1, indexed=None, rows=None, chunk=128):
    """(keep bool, gap uint8 (., 2), count uint32, sectors uint64) of the input rows `rows` (default: all).  indexed: the rows inside
    the voxel grid (default: the rows whose coordinates are all finite)."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    indexed = np.isfinite(pts).all(1) if indexed is None else np.asarray(indexed, bool) & np.isfinite(pts).all(1)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    has, u, v = frames(normals)
    inside = pts[indexed]
    r2 = F(radius) * F(radius)
    count = np.zeros(len(rows), np.uint32)
    sectors = np.zeros(len(rows), np.uint64)
    one = np.uint64(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for at in range(0, len(rows), chunk):
            rr = rows[at:at + chunk]
            live = indexed[rr]
            c = np.where(live[:, None], pts[rr], F(0))
            d = inside[None, :, :] - c[:, None, :]
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            within = (((dx * dx + dy * dy) + dz * dz) <= r2) & live[:, None]
            uu, vv = u[rr][:, None, :], v[rr][:, None, :]
            a = (dx * uu[..., 0] + dy * uu[..., 1]) + dz * uu[..., 2]
            b = (dx * vv[..., 0] + dy * vv[..., 1]) + dz * vv[..., 2]
            directed = within & ~((a == 0) & (b == 0)) & has[rr][:, None]
            s = np.where(directed, sector(a, b), 0).astype(np.uint64)
            count[at:at + chunk] = within.sum(1)
            sectors[at:at + chunk] = np.bitwise_or.reduce(np.where(directed, one << s, np.uint64(0)), axis=1) if inside.size else 0
    G, start = gap_and_start(sectors)
    framed = indexed[rows] & has[rows]
    gap = np.where(framed[:, None], np.stack([G, start], 1), NO_FRAME).astype(np.uint8)
    keep = framed & (count >= max(int(min_neighbours), 1)) & (G >= int(gap_sectors))
    return keep, gap, count, sectors
