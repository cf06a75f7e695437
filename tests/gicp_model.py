"""numpy float64 model of include/pcpx_gicp.h: the plane-to-plane step, every operation in the header's order, inside the loop of
tests/icp_model.py.  `gicp_system_rows` is the per-row form that follows the header line by line; `gicp_system` is the same
arithmetic on whole arrays (tests/test_gicp_cpu.py ties the two, bit for bit per row).  Shared by tests/test_gicp_cpu.py and
tests/test_gpu_gicp.py, with the independent-sampling scene both use."""
import numpy as np

import icp_model as M
from icp_model import F, NONE, box_centre, cholesky_solve, icp, moved64, plane_compose, pose_of  # noqa: F401

FLOOR = 2.0 ** -40
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx, xy, xz, yy, yz, zz


def sym_at(r, c):
    return SYM.index((min(r, c), max(r, c)))


def matrix_of_normal(n, epsilon):
    """the upper triangle (6,) of C = I - (1 - eps) n n^T / q from a float32 normal, or None"""
    n = np.asarray(n, F).astype(np.float64)
    keep = 1.0 - float(F(epsilon))
    with np.errstate(all="ignore"):
        q = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        if not (q > 0.0 and q < np.inf):
            return None
        return np.array([(1.0 if r == c else 0.0) - (keep * (n[r] * n[c])) / q for r, c in SYM])


def matrix_of_six(six):
    c = np.asarray(six, F).astype(np.float64)
    return c if np.isfinite(c).all() else None


def covariances_of_normals(normals, epsilon):
    """(rows, 6) float64: the C of every normal (NaN rows where there is none); its float32 rounding is what the covariance form
    of the tests is fed"""
    normals = np.asarray(normals, F).reshape(-1, 3)
    out = np.full((len(normals), 6), np.nan)
    for i, n in enumerate(normals):
        c = matrix_of_normal(n, epsilon)
        if c is not None:
            out[i] = c
    return out


def _forward(L, a):
    v0 = a[0] / L[0, 0]
    v1 = (a[1] - L[1, 0] * v0) / L[1, 1]
    v2 = ((a[2] - L[2, 0] * v0) - L[2, 1] * v1) / L[2, 2]
    return np.array([v0, v1, v2])


def row_terms(T, o, s_row, x_row, cs, ct):
    """(K (3, 6), z (3,)) of one pair from the upper triangles cs, ct, or None where the factorisation fails"""
    R = T[:3, :3]
    with np.errstate(all="ignore"):
        Mx = np.zeros((3, 3))
        for r in range(3):
            for c in range(3):
                Mx[r, c] = (R[r, 0] * cs[sym_at(0, c)] + R[r, 1] * cs[sym_at(1, c)]) + R[r, 2] * cs[sym_at(2, c)]
        S = np.zeros((3, 3))
        for r in range(3):
            for c in range(r, 3):
                S[r, c] = ct[sym_at(r, c)] + ((Mx[r, 0] * R[c, 0] + Mx[r, 1] * R[c, 1]) + Mx[r, 2] * R[c, 2])
        L = np.zeros((3, 3))
        for j in range(3):
            d = S[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not (d > FLOOR * S[j, j] and d < np.inf):
                return None
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 3):
                v = S[j, i]
                for k in range(j):
                    v = v - L[i, k] * L[j, k]
                L[i, j] = v / L[j, j]
        a, b, c = (float(v) for v in s_row)
        y = np.array([((T[r, 0] * a + T[r, 1] * b) + T[r, 2] * c) + T[r, 3] for r in range(3)])
        e = y - np.asarray(x_row, F).astype(np.float64)
        u = y - o
        J = np.array([[0.0, u[2], -u[1], 1.0, 0.0, 0.0], [-u[2], 0.0, u[0], 0.0, 1.0, 0.0], [u[1], -u[0], 0.0, 0.0, 0.0, 1.0]])
        z = _forward(L, e)
        K = np.stack([_forward(L, J[:, k]) for k in range(6)], 1)
    return K, z


def _matrices(rows, covariances, epsilon):
    rows = np.asarray(rows, F)
    if covariances:
        return [matrix_of_six(r) for r in rows.reshape(-1, 6)]
    return [matrix_of_normal(r, epsilon) for r in rows.reshape(-1, 3)]


def gicp_system_rows(target, target_cov, s, source_cov, T, partner, o, covariances=False, epsilon=1e-3, usable=None):
    """(A (6, 6), b (6,), sum z.z, rows) of the header's step, row by row; usable: a list that gets the usable source rows"""
    target = np.asarray(target, F).reshape(-1, 3)
    s = np.asarray(s, F).reshape(-1, 3)
    cs_all, ct_all = _matrices(source_cov, covariances, epsilon), _matrices(target_cov, covariances, epsilon)
    A, b, ss, rows = np.zeros((6, 6)), np.zeros(6), 0.0, 0
    for i in range(len(s)):
        j = int(partner[i])
        if j == NONE or cs_all[i] is None or ct_all[j] is None:
            continue
        made = row_terms(T, o, s[i], target[j], cs_all[i], ct_all[j])
        if made is None:
            continue
        K, z = made
        for r in range(6):
            for c in range(r, 6):
                A[r, c] += (K[0, r] * K[0, c] + K[1, r] * K[1, c]) + K[2, r] * K[2, c]
                A[c, r] = A[r, c]
            b[r] -= (K[0, r] * z[0] + K[1, r] * z[1]) + K[2, r] * z[2]
        ss += (z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]
        rows += 1
        if usable is not None:
            usable.append(i)
    return A, b, ss, rows


def _matrices_v(rows, covariances, epsilon):
    """(rows, 6) float64 and the mask of the rows that have a matrix"""
    rows = np.asarray(rows, F)
    with np.errstate(all="ignore"):
        if covariances:
            c = rows.reshape(-1, 6).astype(np.float64)
            return c, np.isfinite(c).all(1)
        n = rows.reshape(-1, 3).astype(np.float64)
        keep = 1.0 - float(F(epsilon))
        q = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        c = np.stack([(1.0 if r == k else 0.0) - (keep * (n[:, r] * n[:, k])) / q for r, k in SYM], 1)
        return c, (q > 0.0) & (q < np.inf)


def row_terms_v(T, o, s, x, cs, ct):
    """row_terms on arrays: K (rows, 3, 6), z (rows, 3) and the mask of the rows whose factorisation holds"""
    R = T[:3, :3]
    n = len(s)
    with np.errstate(all="ignore"):
        Mx = np.zeros((n, 3, 3))
        for r in range(3):
            for c in range(3):
                Mx[:, r, c] = (R[r, 0] * cs[:, sym_at(0, c)] + R[r, 1] * cs[:, sym_at(1, c)]) + R[r, 2] * cs[:, sym_at(2, c)]
        S = np.zeros((n, 3, 3))
        for r in range(3):
            for c in range(r, 3):
                S[:, r, c] = ct[:, sym_at(r, c)] + ((Mx[:, r, 0] * R[c, 0] + Mx[:, r, 1] * R[c, 1]) + Mx[:, r, 2] * R[c, 2])
        L = np.zeros((n, 3, 3))
        ok = np.ones(n, bool)
        for j in range(3):
            d = S[:, j, j].copy()
            for k in range(j):
                d = d - L[:, j, k] * L[:, j, k]
            ok &= (d > FLOOR * S[:, j, j]) & (d < np.inf)
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, 3):
                v = S[:, j, i].copy()
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / L[:, j, j]
        s64 = np.asarray(s, F).astype(np.float64)
        y = np.stack([((T[r, 0] * s64[:, 0] + T[r, 1] * s64[:, 1]) + T[r, 2] * s64[:, 2]) + T[r, 3] for r in range(3)], 1)
        e = y - np.asarray(x, F).astype(np.float64)
        u = y - o
        zero, one = np.zeros(n), np.ones(n)
        J = np.stack([np.stack([zero, u[:, 2], -u[:, 1], one, zero, zero], 1), np.stack([-u[:, 2], zero, u[:, 0], zero, one, zero], 1),
                      np.stack([u[:, 1], -u[:, 0], zero, zero, zero, one], 1)], 1)

        def forward(a0, a1, a2):
            v0 = a0 / L[:, 0, 0]
            v1 = (a1 - L[:, 1, 0] * v0) / L[:, 1, 1]
            v2 = ((a2 - L[:, 2, 0] * v0) - L[:, 2, 1] * v1) / L[:, 2, 2]
            return np.stack([v0, v1, v2], 1)

        z = forward(e[:, 0], e[:, 1], e[:, 2])
        K = np.stack([forward(J[:, 0, k], J[:, 1, k], J[:, 2, k]) for k in range(6)], 2)
    return K, z, ok


def gicp_system(target, target_cov, s, source_cov, T, partner, o, covariances=False, epsilon=1e-3, usable=None):
    """gicp_system_rows on whole arrays: the same per-row terms, summed by numpy (so the sums agree to rounding, not to the bit)"""
    target = np.asarray(target, F).reshape(-1, 3)
    s = np.asarray(s, F).reshape(-1, 3)
    cs, has_s = _matrices_v(source_cov, covariances, epsilon)
    ct, has_t = _matrices_v(target_cov, covariances, epsilon)
    partner = np.asarray(partner, np.uint32)
    rows = np.flatnonzero(partner != NONE)
    j = partner[rows].astype(np.int64)
    fine = has_s[rows] & has_t[j]
    rows, j = rows[fine], j[fine]
    K, z, ok = row_terms_v(T, o, s[rows], target[j], cs[rows], ct[j])
    rows, K, z = rows[ok], K[ok], z[ok]
    if usable is not None:
        usable.extend(int(i) for i in rows)
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = ((K[:, 0, r] * K[:, 0, c] + K[:, 1, r] * K[:, 1, c]) + K[:, 2, r] * K[:, 2, c]).sum()
        b[r] = -((K[:, 0, r] * z[:, 0] + K[:, 1, r] * z[:, 1]) + K[:, 2, r] * z[:, 2]).sum()
    ss = float(((z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]) + z[:, 2] * z[:, 2]).sum())
    return A, b, ss, len(rows)


def gicp(target, target_cov, s, source_cov, pose, radius, max_iterations, bbox6, covariances=False, epsilon=1e-3, indexed=None, conditions=None,
         usable=None, system=gicp_system):
    """the loop of the header; conditions: a list that gets cond(A) of every step carried out; usable: a list that gets the number
    of usable rows of every step attempted"""
    o = box_centre(bbox6)

    def step(T, partner):
        A, b, ss, rows = system(target, target_cov, s, source_cov, T, partner, o, covariances, epsilon)
        if usable is not None:
            usable.append(rows)
        x = cholesky_solve(A, b)
        if x is None:
            return None
        if conditions is not None:
            conditions.append(float(np.linalg.cond(A)))
        with np.errstate(all="ignore"):
            return plane_compose(T, o, x), np.sqrt(ss / rows)

    return icp(target, s, pose, radius, max_iterations, step, 3, indexed)


# ---- the independent-sampling scene ----------------------------------------------------------------------------------------------------
SAMPLING_SEED = 3       # (the smallest ratio of the two objectives' errors among seeds 1 - 8; tests/test_gicp_cpu.py asserts the model's facts)
SAMPLING_RADIUS = 0.5
SAMPLING_ITERATIONS = 64


def sampling_scene(seed=SAMPLING_SEED, n=2000, m=500):
    """two independent samplings of one surface: target and its normals, source (its own sample, moved by the inverse of `truth`) and
    its normals in the source frame, truth (4 x 4: source -> target; a 5 degree turn and a shift of 0.05 of the extent), the extent"""
    target, normals = M.surface(n, seed)
    own, own_normals = M.surface(m, seed + 500)
    rng = np.random.default_rng(seed + 1000)
    extent = float(np.linalg.norm(target.max(0).astype(np.float64) - target.min(0)))
    axis = rng.normal(size=3)
    shift = rng.normal(size=3)
    truth = M.rigid(axis, 5.0, 0.05 * extent * shift / np.linalg.norm(shift))
    inv = np.linalg.inv(truth)
    source = (own.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(F)
    source_normals = (own_normals.astype(np.float64) @ inv[:3, :3].T).astype(F)
    return target, normals, source, source_normals, truth, extent
