"""numpy model of include/pcpx_icp.h: the nearest indexed point under a pose by brute force over all pairs, the point-to-point loop
around a fit step that the caller passes in (the library's own host pcpx_rigid_fit on the GPU box, tests/register_model.py's float64
fit where there is no device), and the point-to-plane step and loop in float64.  Shared by tests/test_icp_cpu.py and
tests/test_gpu_icp.py, with the scenes both use."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
EXHAUSTED, CONVERGED, STARVED, DEGENERATE = range(4)
IDENTITY = np.eye(4)


def pose_of(pose):
    return IDENTITY.copy() if pose is None else np.asarray(pose, np.float64).reshape(4, 4)


def moved64(s, pose):
    """y = T s in float64, each operation rounded on its own, in the header's order; (m, 3) float64"""
    T = pose_of(pose)
    s = np.asarray(s, F).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], 1)


def moved32(s, pose):
    with np.errstate(all="ignore"):
        return moved64(s, pose).astype(F)


def nearest_to(target, y, radius, indexed=None):
    """partner (m,) uint32 and d2 (m,) float32 of the float32 queries y: the smallest (d2, j) with d2 <= radius * radius over the
    indexed rows j of target"""
    x = np.asarray(target, F).reshape(-1, 3)
    y = np.asarray(y, F).reshape(-1, 3)
    r2 = F(radius) * F(radius)
    partner = np.full(len(y), NONE, np.uint32)
    best = np.full(len(y), np.inf, F)
    if len(x) == 0:
        return partner, best
    inside = np.ones(len(x), bool) if indexed is None else np.asarray(indexed, bool)
    chunk = max(1, 2000000 // len(x))
    with np.errstate(all="ignore"):
        for a in range(0, len(y), chunk):
            d = x[None, :, :] - y[a:a + chunk, None, :]
            d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
            ok = (d2 <= r2) & inside[None, :]
            d2 = np.where(ok, d2, F(np.inf))
            j = np.argmin(d2, 1)  # (the first of equal minima: the lowest index)
            has = ok.any(1)
            partner[a:a + chunk] = np.where(has, j, NONE).astype(np.uint32)
            best[a:a + chunk] = np.where(has, d2[np.arange(len(j)), j], F(np.inf))
    return partner, best


def nearest_posed(target, s, pose, radius, indexed=None):
    return nearest_to(target, moved32(s, pose), radius, indexed)


def pairs_of(partner):
    return np.stack([np.arange(len(partner), dtype=np.uint32), partner.astype(np.uint32)], 1)


class Run:
    """what a loop returns: transform (16,), status, iterations, last_count, count and rms (max_iterations entries: 0 and NaN
    beyond the updates made), partner (the last list), poses (T_0 ... as 4 x 4)"""

    def __init__(self, max_iterations, pose):
        self.status, self.iterations, self.last_count = EXHAUSTED, 0, 0
        self.count = np.zeros(max_iterations, np.uint32)
        self.rms = np.full(max_iterations, np.nan)
        self.partner = None
        self.poses = [pose_of(pose)]

    @property
    def transform(self):
        return self.poses[-1].reshape(16)


def icp(target, s, pose, radius, max_iterations, step, min_count=3, indexed=None):
    """the loop of the header; step(T_k (4, 4), partner_k) -> (T_next (4, 4), rms) or None for a degenerate step"""
    run = Run(max_iterations, pose)
    s = np.asarray(s, F).reshape(-1, 3)
    previous = None
    for k in range(max_iterations):
        partner, _d2 = nearest_posed(target, s, run.poses[-1], radius, indexed)
        run.partner, run.last_count = partner, int((partner != NONE).sum())
        if k > 0 and np.array_equal(partner, previous):
            run.status = CONVERGED
            return run
        if run.last_count < min_count:
            run.status = STARVED
            return run
        made = step(run.poses[-1], partner)
        if made is None:
            run.status = DEGENERATE
            return run
        run.poses.append(np.asarray(made[0], np.float64).reshape(4, 4))
        run.count[k], run.rms[k] = run.last_count, made[1]
        run.iterations = k + 1
        previous = partner
    run.status = EXHAUSTED
    return run


def icp_point_to_point(target, s, pose, radius, max_iterations, fit, indexed=None):
    """fit(p, q, pairs) -> (16 or 4 x 4 float64, rms): the least-squares rigid fit over the pairs"""
    target = np.asarray(target, F).reshape(-1, 3)
    s = np.asarray(s, F).reshape(-1, 3)
    return icp(target, s, pose, radius, max_iterations, lambda _T, partner: fit(s, target, pairs_of(partner)), 3, indexed)


# ---- point to plane ------------------------------------------------------------------------------------------------------------------
def box_centre(bbox6):
    b = np.asarray(bbox6, F).astype(np.float64)
    return (b[:3] + b[3:]) / 2.0


def plane_system(target, normals, s, T, partner, o):
    """(A (6, 6), b (6,), sum rho^2, rows) of the header's step"""
    target = np.asarray(target, F).reshape(-1, 3)
    normals = np.asarray(normals, F).reshape(-1, 3)
    has = partner != NONE
    j = partner[has].astype(np.int64)
    n = normals[j].astype(np.float64)
    fine = np.isfinite(n).all(1)
    y = moved64(np.asarray(s, F).reshape(-1, 3)[has], T)[fine]
    x, n = target[j].astype(np.float64)[fine], n[fine]
    rho = ((y - x) * n).sum(1)
    J = np.concatenate([np.cross(y - o, n), n], 1)
    return J.T @ J, -(J * rho[:, None]).sum(0), float((rho * rho).sum()), len(rho)


def cholesky_solve(A, b):
    """x of A x = b, or None by the header's pivot rule"""
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
            if not (d > 2.0 ** -40 * A[j, j] and d < np.inf):
                return None
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                L[i, j] = (A[j, i] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    z = np.zeros(6)
    for i in range(6):
        z[i] = (b[i] - (L[i, :i] * z[:i]).sum()) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (z[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


def cayley(w):
    """the rotation of the unit quaternion (1, w / 2) / |(1, w / 2)|"""
    q = np.array([1.0, w[0] / 2, w[1] / 2, w[2] / 2])
    qw, qx, qy, qz = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                     [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                     [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])


def plane_compose(T, o, x):
    dR = cayley(x[:3])
    out = np.eye(4)
    out[:3, :3] = dR @ T[:3, :3]
    out[:3, 3] = dR @ (T[:3, 3] - o) + o + x[3:]
    return out


def icp_point_to_plane(target, normals, s, pose, radius, max_iterations, bbox6, indexed=None, conditions=None):
    """conditions: a list that gets cond(A) of every step carried out"""
    o = box_centre(bbox6)

    def step(T, partner):
        A, b, ss, rows = plane_system(target, normals, s, T, partner, o)
        x = cholesky_solve(A, b)
        if x is None:
            return None
        if conditions is not None:
            conditions.append(float(np.linalg.cond(A)))
        return plane_compose(T, o, x), np.sqrt(ss / rows)

    return icp(target, s, pose, radius, max_iterations, step, 6, indexed)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rigid(axis, degrees, shift):
    T = np.eye(4)
    T[:3, :3] = rotation(axis, degrees)
    T[:3, 3] = shift
    return T


def surface(n, seed):
    """a curved surface cloud over [-1, 1]^2 and its exact unit normals: (points float32 (n, 3), normals float32 (n, 3))"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    z = 0.3 * np.sin(2.0 * x) * np.cos(1.5 * y) + 0.15 * x * x - 0.1 * y
    zx = 0.6 * np.cos(2.0 * x) * np.cos(1.5 * y) + 0.3 * x
    zy = -0.45 * np.sin(2.0 * x) * np.sin(1.5 * y) - 0.1
    nrm = np.stack([-zx, -zy, np.ones(n)], 1)
    return np.stack([x, y, z], 1).astype(F), (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)


RECOVERY_SEED = 5       # (chosen on the CPU so that the model converges with every partner the true one: tests/test_icp_cpu.py asserts it)
RECOVERY_RADIUS = 0.5
RECOVERY_ITERATIONS = 64


def recovery_scene(seed=RECOVERY_SEED, n=2000, m=500):
    """target, its normals, the rows the source was taken from, the source (those target points moved by the inverse of `truth`),
    truth (4 x 4: source -> target; a 5 degree rotation and a shift of 0.05 of the extent) and the extent"""
    target, normals = surface(n, seed)
    rng = np.random.default_rng(seed + 1000)
    rows = np.sort(rng.choice(n, m, replace=False))
    extent = float(np.linalg.norm(target.max(0).astype(np.float64) - target.min(0)))
    axis = rng.normal(size=3)
    shift = rng.normal(size=3)
    truth = rigid(axis, 5.0, 0.05 * extent * shift / np.linalg.norm(shift))
    inv = np.linalg.inv(truth)
    source = (target[rows].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(F)
    return target, normals, rows, source, truth, extent


def corner_error(T, truth, target):
    """the largest distance between the images of the target box's corners (pulled back to the source frame) under T and truth"""
    lo, hi = target.min(0).astype(np.float64), target.max(0).astype(np.float64)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    inv = np.linalg.inv(truth)
    src = corners @ inv[:3, :3].T + inv[:3, 3]
    T = np.asarray(T, np.float64).reshape(4, 4)
    return float(np.linalg.norm(src @ T[:3, :3].T + T[:3, 3] - corners, axis=1).max())
