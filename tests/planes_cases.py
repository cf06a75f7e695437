"""The scenes of the plane-detection tests (tests/test_planes_cpu.py asserts their conditions on the model alone,
tests/test_gpu_planes.py runs them on the GPU): built once, never changed."""
import functools

import numpy as np

import planes_model as M

F = np.float32


@functools.lru_cache(None)
def ties_scene():
    """two 8 x 8 integer grids at z = 0 and z = 3, 64 integer outliers at z >= 5, rows shuffled: every coordinate, difference and
    cross product is a small integer, so many hypotheses hit one of the two grids exactly and tie at 64"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2)
    lo = np.concatenate([g, np.zeros((64, 1))], 1)
    hi = np.concatenate([g, np.full((64, 1), 3.0)], 1)
    out = np.concatenate([rng.integers(0, 8, (64, 2)), rng.integers(5, 40, (64, 1))], 1)
    P = np.concatenate([lo, hi, out]).astype(F)
    P = P[rng.permutation(len(P))]
    P.setflags(write=False)
    return P


TIES = dict(max_distance=0.25, seed=0x1234)
TIES_SHIFT = np.array([2.0 ** 10, -2.0 ** 10, 2.0 ** 10], F)


@functools.lru_cache(None)
def peel_scene():
    """three faces of a box corner on a 1/40 grid (40 x 40 at z = 0, 30 x 30 at x = 0, 20 x 20 at y = 0; the shared edges belong to
    all the faces they lie on) and 500 uniform outliers in [0.05, 1]^3, rows shuffled.  Returns (P, is_outlier)."""
    rng = np.random.default_rng(12)

    def grid(k):
        return np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2) / 40.0

    a, b, c = grid(40), grid(30), grid(20)
    fz = np.concatenate([a, np.zeros((len(a), 1))], 1)
    fx = np.concatenate([np.zeros((len(b), 1)), b], 1)
    fy = np.stack([c[:, 0], np.zeros(len(c)), c[:, 1]], 1)
    out = rng.uniform(0.05, 1.0, (500, 3))
    P = np.concatenate([fz, fx, fy, out]).astype(F)
    is_out = np.concatenate([np.zeros(len(P) - 500, bool), np.ones(500, bool)])
    perm = rng.permutation(len(P))
    P, is_out = P[perm], is_out[perm]
    P.setflags(write=False)
    return P, is_out


PEEL = dict(max_distance=0.004, min_inliers=200, max_planes=6, seed=0x1234)


@functools.lru_cache(None)
def noisy_scene(inlier_fraction):
    """2 000 points in [-1, 1]^3, a fraction of them on a plane with sigma = 0.002.  Returns (P, n_true, d_true)."""
    rng = np.random.default_rng(13)
    n_true = np.array([0.3, -0.5, 0.8])
    n_true /= np.linalg.norm(n_true)
    d_true = 0.1
    k = int(round(2000 * inlier_fraction))
    u = np.cross(n_true, [1.0, 0, 0])
    u /= np.linalg.norm(u)
    v = np.cross(n_true, u)
    ab = rng.uniform(-0.8, 0.8, (k, 2))
    on = ab[:, :1] * u + ab[:, 1:] * v - d_true * n_true + rng.normal(0, 0.002, (k, 1)) * n_true
    off = rng.uniform(-1, 1, (2000 - k, 3))
    P = np.concatenate([on, off]).astype(F)
    P = P[rng.permutation(len(P))]
    P.setflags(write=False)
    return P, n_true, d_true


NOISY = [(0.5, 1024), (0.3, 4096), (0.1, 65536)]
NOISY_ARGS = dict(max_distance=0.01, seed=0x1234)


@functools.lru_cache(None)
def model_run(name, T, shifted=False, frac=None):
    """the model's Result of a scene's single call, computed once"""
    if name == "ties":
        P = ties_scene() + (TIES_SHIFT if shifted else F(0))
        return M.ransac(P.astype(F), T, TIES["seed"], TIES["max_distance"])
    if name == "noisy":
        return M.ransac(noisy_scene(frac)[0], T, NOISY_ARGS["seed"], NOISY_ARGS["max_distance"])
    raise KeyError(name)


@functools.lru_cache(None)
def model_peel(T, max_planes=PEEL["max_planes"], min_inliers=PEEL["min_inliers"]):
    return M.extract(peel_scene()[0], T, PEEL["seed"], PEEL["max_distance"], min_inliers, max_planes)


def fit_sets():
    """(name, points (n, 3) float32) of the plane-fit comparisons: each has an eigenvalue gap l1 - l0 >= 0.1 l2"""
    rng = np.random.default_rng(14)
    sets = []
    for i, (n, shift) in enumerate(((3, 0.0), (50, 0.0), (2000, 0.0), (2000, 500.0), (777, 500.0))):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        u = np.cross(nrm, [0, 0, 1.0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        ab = rng.uniform(-1, 1, (n, 2)) * [1.0, 0.6]
        x = ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0, 0.01 if n > 3 else 0.0, (n, 1)) * nrm + shift
        sets.append(("set%d_n%d_at%g" % (i, n, shift), x.astype(F)))
    return sets
