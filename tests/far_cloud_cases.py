"""Deterministic clouds far from the origin and at other scales, for tests/test_gpu_far_clouds.py and the reference fixture
tests/golden/ref_far.npz (tests/golden/make_reference_golden.py).  numpy only: no GPU, no package import.

Every coordinate is built as offset + i * step with integer i, a power-of-two step and a power-of-two offset, so it is exact in
float32 and the same on every machine.  `utm` is the exception that proves the rule: its design coordinates are on a 0.01 grid
and are then rounded to float32 at the offset, where the spacing is 2^-5 (x), 2^-3 (y) and 2^-16 (z) -- which is what a
georeferenced cloud read into float32 looks like.

    case(name) -> Case(name, points float32 (n, 3), offset float64 (3,), step, radius, rows)
    cap_case(offset, s_over_r) -> (points, centres, radius): spheres whose points sit in a cluster of size s near the rim

`radius` is a sphere radius that holds about 15-40 points, `rows` a fixed sample of query rows for brute-force checks."""
import collections

import numpy as np

import surface_nets_model as M

F = np.float32
Case = collections.namedtuple("Case", "name points offset step radius rows")

NAMES = ("near", "cad_mm", "small", "far_1e3", "utm", "far_plane")
ROWS = 2000  # brute-force rows per case


def _quantise(x, offset, step):
    """offset + round(x / step) * step, exact in float32 (asserted)."""
    i = np.round(np.asarray(x, np.float64) / step)
    p64 = np.asarray(offset, np.float64) + i * step
    p = p64.astype(F)
    assert np.array_equal(p.astype(np.float64), p64), "a coordinate is not exact in float32"
    return p


def _surface(rng, n, centre, radius, noise):
    """n points near a sphere (a closed, curved surface: every neighbourhood has a well-defined normal) with normal noise."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.asarray(centre, np.float64) + v * (radius + noise * rng.normal(size=(n, 1)))


def _rows(n, seed):
    return np.sort(np.random.default_rng(seed).choice(n, min(ROWS, n), replace=False)).astype(np.int64)


def _radius(pts, rows, k):
    """The median distance to the k-th nearest point over 200 of the rows, rounded up to a power-of-two multiple of 1/64 of
    itself (a float32 radius that the tests and the fixture share)."""
    s = pts[rows[:: max(1, len(rows) // 200)]].astype(np.float64)
    p = pts.astype(np.float64)
    d = np.sort(np.sqrt(((s[:, None, :] - p[None, :, :]) ** 2).sum(-1)), 1)[:, min(k, len(pts) - 1)]
    r = float(np.median(d))
    e = 2.0 ** (np.floor(np.log2(r)) - 6)
    return float(F(np.ceil(r / e) * e))


def case(name):
    rng = np.random.default_rng(NAMES.index(name) + 1000)
    if name == "near":  # the regime of the rest of the suite: [0, 1)^3, a sphere surface and a uniform background
        off, step = np.zeros(3), 2.0 ** -16
        x = np.concatenate([_surface(rng, 16000, (0.5, 0.5, 0.5), 0.35, 2e-3), rng.uniform(0, 1, (4000, 3))])
    elif name == "cad_mm":  # millimetres: ~2 * 10^3 across, r > 1 everywhere, d^2 up to ~10^5
        off, step = np.zeros(3), 2.0 ** -6
        x = np.concatenate([_surface(rng, 24000, (1024, 1024, 1024), 600, 0.5), rng.uniform(0, 2048, (8000, 3))])
    elif name == "small":  # 10^-3 across, spacing ~10^-5: the default eps box (1e-5) holds neighbours
        off, step = np.zeros(3), 2.0 ** -17
        x = np.concatenate([_surface(rng, 16000, (5e-4, 5e-4, 5e-4), 3.5e-4, 2e-6), rng.uniform(0, 1e-3, (4000, 3))])
    elif name == "far_1e3":  # DESIGN.md section 16's claim: |q| ~ 10^3, spacing far above the float32 grid (2^-13 there)
        off, step = np.full(3, 2.0 ** 10), 2.0 ** -13
        x = np.concatenate([_surface(rng, 24000, (0.5, 0.5, 0.5), 0.35, 1e-3), rng.uniform(0, 1, (6000, 3))])
    elif name == "utm":  # georeferenced terrain, 30 x 30 (metres), 0.01 design grid rounded to float32 at the offset
        off, step = np.array([2.0 ** 18, 2.0 ** 20, 2.0 ** 7]), None
        n = 100_000
        xy = rng.uniform(0, 30, (n, 2))
        z = 2.0 + 1.5 * np.sin(xy[:, 0] / 4.0) * np.cos(xy[:, 1] / 5.0) + 0.02 * rng.normal(size=n)
        design = np.round(np.column_stack([xy, z]) / 0.01) * 0.01
        p = (off + design).astype(F)  # rounded to the float32 grid at the offset
        assert np.unique(p[:, 1]).size <= 30 / 2.0 ** -3 + 2
        return Case(name, p, off, step, _radius(p, _rows(n, 7), 24), _rows(n, 7))
    elif name == "far_plane":  # 2^16: a 4 x 4 slab, ~10^-2 thick, tilted (z = x / 4 + y / 8): a well-conditioned normal far away
        off, step = np.full(3, 2.0 ** 16), 2.0 ** -7
        n = 50_000
        xy = rng.uniform(0, 4, (n, 2))
        z = 0.25 * xy[:, 0] + 0.125 * xy[:, 1] + rng.uniform(-5e-3, 5e-3, n)
        x = np.column_stack([xy, z])
    else:
        raise ValueError(name)
    p = _quantise(x, off, step)
    rows = _rows(len(p), 7)
    return Case(name, p, off, step, _radius(p, rows, 24), rows)


def plane_normal():
    """far_plane's unit normal (float64)."""
    n = np.array([-0.25, -0.125, 1.0])
    return n / np.linalg.norm(n)


CAP_SIZES = (10.0, 100.0, 1000.0)  # r / s
CAP_OFFSETS = (0.0, 2.0 ** 10)
CAP_RADIUS = 2.0


def cap_case(offset, r_over_s, spheres=64, per=40):
    """(points, centres, radius): `spheres` spheres of radius CAP_RADIUS, 4 r apart so that none reaches another's points; each
    holds `per` points in a flat patch of size s = r / r_over_s (thickness s / 5) centred 0.9 r from its centre.  tr(Q) about
    the centre is ~ n (0.9 r)^2 while lambda1 - lambda0 ~ n s^2 / 12: the one-pass moments' weakest case."""
    rng = np.random.default_rng(int(r_over_s) + int(offset))
    r = CAP_RADIUS
    s = r / r_over_s
    step = 2.0 ** (np.floor(np.log2(s)) - 7) if offset == 0 else 2.0 ** -13  # >= 2^7 steps across the patch; 2^-13 is the grid at 2^10
    g = np.arange(spheres)
    grid = np.column_stack([g % 4, (g // 4) % 4, g // 16]) * 4 * r + r  # 4 x 4 x 4 centres
    centres = _quantise(grid, offset, 2.0 ** -4)
    pts = []
    for c in centres.astype(np.float64):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        e1 = np.cross(u, [1.0, 0.0, 0.0] if abs(u[0]) < 0.9 else [0.0, 1.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(u, e1)
        a, b, t = rng.uniform(-0.5, 0.5, (3, per, 1))
        pts.append(c + 0.9 * r * u + s * (a * e1 + b * e2 + 0.2 * t * u))
    p = _quantise(np.concatenate(pts) - offset, offset, step)
    return p, centres, float(F(r))


FAR_GRID_ORIGIN = 2.0 ** 14


def far_grid():
    """A 24^3 grid at 2^14 with a spacing that is not a power of two (corners lo + i d round there), the sphere field over
    it, the isovalue and a hint on the surface."""
    g = M.grid_dict(FAR_GRID_ORIGIN, FAR_GRID_ORIGIN, FAR_GRID_ORIGIN, 0.03, 0.03, 0.03, 24, 24, 24)
    c = np.array([FAR_GRID_ORIGIN + 0.37, FAR_GRID_ORIGIN + 0.35, FAR_GRID_ORIGIN + 0.33], F)
    p = (M.corner_positions(g) - c).astype(F)
    f = (np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) - F(0.25)).astype(F)
    return g, f, 0.0, (float(c[0]), float(c[1]), float(c[2]) + 0.25)
