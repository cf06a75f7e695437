"""Shared by tests/test_shape_features_cpu.py and tests/test_gpu_shape_features.py (include/pcpx_features.h):
the clouds and sampled rows of the GPU tests, float32 brute-force point sets, the float64 reference of a set's features, a fast
form of the float32 one-pass scatter matrix, and the two hand-made shapes whose geometry is checked on the CPU before the GPU
tests rely on it (a noisy line, a box surface).  numpy only: no GPU."""
import numpy as np

F = np.float32
EPS = float(np.finfo(np.float32).eps)
ROWS = 600  # sampled rows per cloud


def brute_set(pts, c, r):
    """Indices of the points inside the sphere, by the float32 rule of the kernels: (dx dx + dy dy) + dz dz <= r r."""
    d = pts - c[None, :]
    return np.nonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= F(r) * F(r))[0]


def radius_for(pts, k, seed=0):
    """The median distance to the k-th nearest point over a sample: a radius that holds about k points."""
    rng = np.random.default_rng(seed)
    s = pts[rng.choice(len(pts), min(200, len(pts)), replace=False)].astype(np.float64)
    d = np.sqrt(((s[:, None, :] - pts[None, :, :].astype(np.float64)) ** 2).sum(-1))
    return float(np.median(np.sort(d, 1)[:, min(k, len(pts) - 1)]))


CLOUDS = ("uniform", "clustered", "planar", "duplicates")


def cloud(pkg, kind, n=20000):
    """The clouds of tests/test_gpu_range_neighbourhoods.py."""
    rng = np.random.default_rng(11)
    if kind == "uniform":
        return pkg.synthetic.uniform_cloud(n, 5)
    if kind == "clustered":
        return pkg.synthetic.clustered_cloud(n, seed=6)
    g = rng.uniform(0, 1, (n, 2))
    planar = np.concatenate([g, (0.25 + 1e-4 * rng.normal(size=(n, 1)))], 1).astype(F)
    if kind == "planar":
        return planar
    base = rng.uniform(0, 1, (n // 4, 3)).astype(F)
    return base[rng.integers(0, len(base), n)]  # every point ~4 times


def radii(pts):
    return (("r0", 0.0), ("k3", radius_for(pts, 3)), ("k15", radius_for(pts, 15)), ("k200", radius_for(pts, 200)))


def sampled_rows(n, seed=1):
    return np.random.default_rng(seed).choice(n, ROWS, replace=False)


def moved_centres(pts, rows, r, seed=2):
    """The batch form's spheres: the sampled points moved by up to r."""
    return (pts[rows] + np.random.default_rng(seed).uniform(-1, 1, (len(rows), 3)) * r).astype(F)


def line_cloud(n=2000, seed=21):
    """n points along a fixed direction through the unit cube with 1e-4 isotropic noise; returns (points, unit direction)."""
    rng = np.random.default_rng(seed)
    u = np.array([3.0, 2.0, 1.0])
    u /= np.linalg.norm(u)
    t = rng.uniform(0, 1, n)
    return (np.array([0.1, 0.2, 0.3]) + np.outer(t, u) + 1e-4 * rng.normal(size=(n, 3))).astype(F), u


def box_surface(m=63, seed=31):
    """The surface of the unit cube, noise-free: an m x m jittered grid on each of the six faces, kept 0.25 cells away from the
    face's own edges (so no two faces share a point).  Returns (points, face id per point, distance to the nearest edge, cell)."""
    rng = np.random.default_rng(seed)
    h = 1.0 / m
    pts, face = [], []
    for f in range(6):
        axis, side = f // 2, float(f % 2)
        i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
        a = (i.ravel() + 0.5 + rng.uniform(-0.25, 0.25, m * m)) * h
        b = (j.ravel() + 0.5 + rng.uniform(-0.25, 0.25, m * m)) * h
        p = np.empty((m * m, 3))
        p[:, axis] = side
        p[:, (axis + 1) % 3] = a
        p[:, (axis + 2) % 3] = b
        pts.append(p)
        face.append(np.full(m * m, f))
    pts = np.concatenate(pts).astype(F)
    face = np.concatenate(face)
    p64 = pts.astype(np.float64)
    near = np.minimum(p64, 1.0 - p64)  # distance to the two planes of each axis
    edge = np.sort(near, 1)[:, 1]      # on a face one of them is 0: the distance to the nearest edge is the second smallest
    return pts, face, edge, h


def reference_features(P64, q64):
    """float64: (eigenvalues ascending, eigenvectors, surface variation, tr Q about q, tr C) of the set P64 (m x 3), m >= 1."""
    mu = P64.mean(0)
    C = (P64 - mu).T @ (P64 - mu)
    w, v = np.linalg.eigh(C)
    d = P64 - q64
    trq = float((d * d).sum())
    trc = float(np.trace(C))
    sv = max(w[0], 0.0) / w.sum() if w.sum() > 0 else 0.0
    return w, v, sv, trq, trc


def scatter_f32(P, q):
    """The six float32 entries (c00, c10, c11, c20, c21, c22) of C = Q - S (S / n) as the kernel's epilogue forms them: the
    arithmetic of moments_model (tests/test_range_neighbourhoods_cpu.py), with numpy's sequential float32 cumsum for the sums
    (tests/test_shape_features_cpu.py checks that the two agree bit for bit).  n >= 1."""
    P = np.asarray(P, F).reshape(-1, 3)
    d = P - np.asarray(q, F)[None, :]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    last = lambda a: np.cumsum(a, dtype=F)[-1]
    s = [last(x), last(y), last(z)]
    Q = [last(x * x), last(y * x), last(y * y), last(z * x), last(z * y), last(z * z)]
    n = F(len(P))
    m = [F(v / n) for v in s]
    return np.array([Q[0] - s[0] * m[0], Q[1] - s[1] * m[0], Q[2] - s[1] * m[1], Q[3] - s[2] * m[0], Q[4] - s[2] * m[1],
                     Q[5] - s[2] * m[2]], F)


def as_matrix(c):
    c = np.asarray(c, np.float64)
    return np.array([[c[0], c[1], c[3]], [c[1], c[2], c[4]], [c[3], c[4], c[5]]])


def curvature_f32(ev, n):
    """The contract's surface variation from float32 eigenvalues (ascending) and the count: max(l0, 0) / ((l0 + l1) + l2) in float32
    in that order, 0 when the sum is <= 0, NaN for an empty set."""
    if n == 0:
        return F(np.nan)
    l0, l1, l2 = (F(v) for v in ev)
    s = F(F(l0 + l1) + l2)
    return F(max(l0, F(0)) / s) if s > 0 else F(0)


def model_ratio(pts, centres, sets):
    """The worst max_i |lambda_i(model) - lambda_i(float64)| / (eps_f32 tr Q64) over the rows: the model is float64 eigh of the
    float32 one-pass scatter matrix in list order; rows with tr Q64 = 0 must give a zero matrix exactly."""
    worst = 0.0
    for c, s in zip(centres, sets):
        if len(s) == 0:
            continue
        w64, _, _, trq, _ = reference_features(pts[s].astype(np.float64), c.astype(np.float64))
        C = scatter_f32(pts[s], c)
        if trq == 0.0:
            assert not C.any()
            continue
        worst = max(worst, float(np.abs(np.linalg.eigvalsh(as_matrix(C)) - w64).max()) / (EPS * trq))
    return worst
