"""The numpy model of moving least squares projection (include/pcpx_mls.h), shared by tests/test_mls_cpu.py
and tests/test_gpu_mls.py.  The model is the definition: float64 everywhere except what defines the SET -- d = p - q in float32 and
the inside test (dx dx + dy dy) + dz dz <= r r in float32 -- and the width h and k = -1 / (h h), which the contract forms in float32.
A second form, project(..., dtype=float32), accumulates the contract's sums in float32 in a given order: the CPU tests hold it to the error bound
below against the float64 sums.  numpy only: no GPU.

The error bound (the form of DESIGN.md section 16, restated for weighted sums).  Every accumulated sum of m terms carries a relative
error of about m eps of the sum of its terms' magnitudes; S and Q are sums over |d| <= r, so C = Q - S m^T is off by O(eps W r^2) --
scale_c = tr Q64 is that magnitude.  First-order perturbation of the smallest eigenvector turns an error dC into an angle
|dC| / (l1 - l0), and of the plane's offset t = m . n into r times that angle plus eps r.  Hence, with

    kappa1 = 1 + tr Q / (l1 - l0)            (l0 <= l1 <= l2 the eigenvalues of C, Q about the sphere's centre)

    |d displacement| <= K_DISP  eps r kappa1            (order 1)
    angle(normal)    <= K_ANGLE eps kappa1              (order 1)

and for order 2 the system A c = b is solved.  Scaled by its own diagonal, A' = D^-1/2 A D^-1/2 has a unit diagonal and entries of
magnitude <= 1, each carrying a relative float32 error; the solution moves by at most |A'^-1| = 1 / lambda_min(A') times that, and
the system's entries move with the frame (the normal's angle).  growth = 1 / lambda_min(A') is never smaller than one over the
smallest pivot ratio rho -- a pivot of A' is a Schur complement's entry, >= lambda_min(A') --, which is what the contract's refusal
tests; on well-conditioned rows (spheres, planes) it is about three times that.  kappa2 = kappa1 growth.  The coefficients c are
O(1) in units of r (heights over r), so

    |d displacement| <= K_DISP  eps r kappa2
    angle(normal)    <= K_ANGLE eps kappa2
    |dH| r, |dK| r^2 <= K_CURV  eps kappa2 (1 + |H| r + |K| r^2)

The bound applies on rows with l1 > 0 and l0 <= 0.5 l1 (a separated normal).  The constants are measured on the GPU per case and
kept in tests/test_gpu_mls.py."""
import numpy as np

F = np.float32
EPS = float(np.finfo(np.float32).eps)
PIVOT_MIN = 2.0 ** -12
FIT_BAND = (2.0 ** -14, 2.0 ** -10)  # model pivot ratios in this band: the device's fit may differ from the model's


def brute_set(pts, c, r):
    """Indices of the points inside the sphere and their float32 d = p - c, by the float32 rule of the kernels."""
    d = pts - np.asarray(c, F)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= F(r) * F(r)
    s = np.nonzero(inside)[0]
    return s, d[s]


def weight_k(h):
    """k = -1 / (h h) in float32; a width of 0 (a sphere of radius 0 among per-sphere radii) gives k = 0: weight 1."""
    h = F(h)
    return float(F(-1.0) / (h * h)) if h > 0 else 0.0


def width_of(gauss_h, r=None, radius=None):
    """The sphere's width: gauss_h, or gauss_h * r / radius in float32 with one radius per sphere."""
    return F(gauss_h) if r is None else F(F(gauss_h) * F(r)) / F(radius)


def smallest_axis(n):
    a = np.abs(n)
    return int(np.argmin(a))  # (the first minimum: ties to the lowest axis)


def frame(n):
    a = np.zeros(3)
    a[smallest_axis(n)] = 1.0
    U = np.cross(n, a)
    U /= np.linalg.norm(U)
    return U, np.cross(n, U)


def cholesky_pivots(A):
    """The pivots of the Cholesky factorisation of A over their own diagonal entries; stops at the first pivot <= 0 (its ratio is kept)."""
    n = len(A)
    L = np.zeros((n, n))
    ratios = []
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        ratios.append(d / A[j, j] if A[j, j] != 0 else -np.inf)
        if not d > 0:
            break
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[j, i] - L[i, :j] @ L[j, :j]) / L[j, j]
    return np.array(ratios)


class Row:
    """One sphere's result: count, fit, disp (3), normal (3), H, K, and the quantities of the bound: trq, gap = l1 - l0, evals,
    rho = the smallest pivot ratio (inf when no system was formed), growth = 1 / lambda_min of the system scaled to a unit diagonal."""
    __slots__ = ("count", "fit", "disp", "normal", "H", "K", "trq", "gap", "evals", "rho", "growth", "plane_disp", "plane_normal")


def _sums(d, w, dtype, order=None):
    if order is not None:
        d, w = d[order], w[order]
    d = d.astype(dtype)
    w = w.astype(dtype)
    acc = (lambda a: np.cumsum(a, dtype=dtype)[-1]) if dtype == F else (lambda a: a.sum())
    wd = w[:, None] * d
    W = acc(w)
    S = np.array([acc(wd[:, i]) for i in range(3)], dtype)
    Q = np.empty((3, 3), dtype)
    for i in range(3):
        for j in range(i + 1):
            Q[i, j] = Q[j, i] = acc(wd[:, i] * d[:, j])
    return W, S, Q


def project(d32, r, h, order=2, dtype=np.float64, perm=None):
    """The contract on one sphere: d32 the float32 offsets of its points (m x 3), r its radius, h its width.  dtype float64: the
    model; float32: the sums (both walks) accumulated sequentially in float32 in the order `perm`, everything after them in float64."""
    out = Row()
    m = len(d32)
    out.count = m
    out.fit = 0
    out.disp = np.zeros(3)
    out.normal = np.array([0.0, 0.0, 1.0])
    out.plane_disp, out.plane_normal = out.disp, out.normal
    out.H = out.K = np.nan
    out.trq, out.gap, out.evals, out.rho, out.growth = 0.0, 0.0, np.zeros(3), np.inf, 1.0
    if m < 3:
        return out
    d = d32.astype(np.float64)
    k = weight_k(h)
    d2 = (d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2]  # float32, as the kernel's
    if dtype == F:
        w = np.exp(d2 * F(k)).astype(F)
    else:
        w = np.exp(d2.astype(np.float64) * k)
    W, S, Q = _sums(d32, w, dtype, perm)
    if not W > 0:
        return out
    W, S, Q = float(W), S.astype(np.float64), Q.astype(np.float64)
    if dtype == F:
        mean = (S.astype(F) / F(W)).astype(np.float64)
        C = (Q.astype(F) - np.outer(S.astype(F), mean.astype(F)).astype(F)).astype(np.float64)
        C = np.tril(C) + np.tril(C, -1).T  # (the kernel forms the lower triangle: c_ij = q_ij - s_i m_j, i >= j)
    else:
        mean = S / W
        C = Q - np.outer(S, mean)
        C = (C + C.T) / 2
    out.fit = 1
    ev, vec = np.linalg.eigh(C)
    out.evals = ev
    out.trq = float(np.trace(Q))
    out.gap = float(ev[1] - ev[0])
    if not C.any():
        return out  # copies of one point: the centre stays, the solver's normal of a zero matrix
    n = vec[:, 0]
    t = float(mean @ n)
    out.normal = n
    out.disp = t * n
    out.plane_disp, out.plane_normal = out.disp, out.normal
    if order != 2 or m < 6 or r == 0:
        return out
    U, V = frame(n)
    o = t * n
    e = d - o[None, :]
    u, v, z = (e @ U) / r, (e @ V) / r, (e @ n) / r
    B = np.stack([np.ones(m), u, v, u * u, u * v, v * v], 1)
    if dtype == F:
        order_ = perm if perm is not None else np.arange(m)
        B32, w32, z32 = B.astype(F)[order_], w.astype(F)[order_], z.astype(F)[order_]
        A = np.empty((6, 6))
        for i in range(6):
            for j in range(i, 6):
                A[i, j] = A[j, i] = np.cumsum(w32 * B32[:, i] * B32[:, j], dtype=F)[-1]
        rhs = np.array([np.cumsum(w32 * z32 * B32[:, i], dtype=F)[-1] for i in range(6)], np.float64)
    else:
        A = (B * w[:, None]).T @ B
        rhs = (B * w[:, None]).T @ z
    ratios = cholesky_pivots(A)
    out.rho = float(ratios.min())
    scale = 1.0 / np.sqrt(np.where(np.diag(A) > 0, np.diag(A), 1.0))
    lmin = float(np.linalg.eigvalsh(A * np.outer(scale, scale))[0])
    out.growth = 1.0 / lmin if lmin > 0 else np.inf
    if len(ratios) < 6 or not (ratios > PIVOT_MIN).all() or not np.isfinite(ratios).all():
        return out
    c = np.linalg.solve(A, rhs)
    out.fit = 2
    out.disp = o + c[0] * r * n
    nn = n - c[1] * U - c[2] * V
    out.normal = nn / np.linalg.norm(nn)
    hu, hv, huu, huv, hvv = c[1], c[2], 2 * c[3] / r, c[4] / r, 2 * c[5] / r
    g = 1 + hu * hu + hv * hv
    out.K = (huu * hvv - huv * huv) / g ** 2
    out.H = ((1 + hv * hv) * huu - 2 * hu * hv * huv + (1 + hu * hu) * hvv) / (2 * g ** 1.5)
    return out


def project_cloud(pts, centres, r, h, order=2, radii=None):
    """The model's rows for spheres at `centres` (float32 m x 3) over the cloud `pts`; radii: one per sphere, h then scales with it."""
    rows = []
    for i, c in enumerate(centres):
        ri = float(F(r)) if radii is None else float(F(radii[i]))
        hi = width_of(h) if radii is None else width_of(h, radii[i], r)
        if not np.isfinite(c).all():
            rows.append(project(np.zeros((0, 3), F), ri, hi, order))
            continue
        _s, d = brute_set(pts, c, ri)
        rows.append(project(d, ri, hi, order))
    return rows


def kappa(row, order):
    """The bound's condition factor of a row, or None where the bound does not apply (no separated normal)."""
    ev = row.evals
    if row.fit == 0 or not ev[1] > 0 or not ev[0] <= 0.5 * ev[1]:
        return None
    k1 = 1.0 + row.trq / row.gap
    if order == 2 and row.fit == 2:
        return k1 * row.growth
    return k1


def angle(a, b):
    """The angle between two unit vectors up to sign."""
    c = abs(float(np.dot(np.asarray(a, np.float64), np.asarray(b, np.float64))))
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.linalg.norm(np.cross(a64, b64))
    return float(np.arctan2(s, c))


# ---- the clouds of the property tests -------------------------------------------------------------------------------------------
def sphere_cloud(n=4000, noise=0.0, centre=0.0, seed=3):
    """n points on the unit sphere about (centre, centre, centre), moved radially by noise * N(0, 1); float32."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= 1.0 + noise * rng.normal(size=(n, 1))
    return (x + centre).astype(F)


def exact_plane(m=48):
    """Points (i, j, -i - j) / 64, 0 <= i, j < m: exact coordinates on x + y + z = 0."""
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    return (np.stack([i.ravel(), j.ravel(), -i.ravel() - j.ravel()], 1) / 64.0).astype(F)


def property_rows(n, rows=300, seed=3):
    return np.random.default_rng(seed + 1).choice(n, min(rows, n), replace=False)
