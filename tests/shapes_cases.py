"""The scenes of the sphere and cylinder tests (include/pcpx_shapes.h), shared by tests/test_shapes_cpu.py, which
proves on the numpy model alone that each scene is what it is meant to be, and tests/test_gpu_shapes.py, which then compares bits.
Nothing here touches a GPU.  Every hypothesis count a scene needs was found with the model (test_shapes_cpu.py asserts that it
suffices), not guessed."""
import functools

import numpy as np

import shapes_model as M

F = np.float32
KINDS = (M.SPHERE, M.CYLINDER)
SEED = 0x51A9E
ROWS = 2000        # points and listed rows of the count sets
UNROLL = {False: 8, True: 4}  # csrc/pcpx_shapes.hip, unroll_of<NORMALS>(): records of one trip of k_shape_count's loop
BLOCK_HYPOTHESES = 256        # csrc/pcpx_shapes.hip: SH_WAVES wavefronts of 64
TS = (1, 63, 64, 65, BLOCK_HYPOTHESES + 1)
T_MAX = max(TS)
COSN = 0.9
TAU = 0.01
NOISY_T = 1024     # found with the model: test_shapes_cpu.py::test_the_noisy_scenes_recover_their_shape
GATE_T = 512       # found with the model: test_shapes_cpu.py::test_each_gate_changes_the_winner
FAR = np.array([500.0, -3.0, 20.0])


def count_sizes(gated):
    u = UNROLL[gated]
    return (0, 1, 2, 3, u - 1, u, u + 1, 255, 256, 257, 1400)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _noisy_normals(rng, nrm, degrees):
    """unit normals turned by a Gaussian angle of that many degrees, with random signs"""
    t = _unit(np.cross(nrm, rng.normal(size=nrm.shape)))
    a = np.deg2rad(degrees) * rng.normal(size=(len(nrm), 1))
    out = nrm * np.cos(a) + t * np.sin(a)
    return out * rng.choice([-1.0, 1.0], (len(nrm), 1))


def on_sphere(rng, m, centre, radius, sigma=0.0):
    d = _unit(rng.normal(size=(m, 3)))
    return np.asarray(centre) + d * (radius + sigma * rng.normal(size=(m, 1))), d


def on_cylinder(rng, m, point, axis, radius, length, sigma=0.0, arc=2 * np.pi):
    axis = _unit(np.asarray(axis, np.float64))
    a = _unit(np.cross(axis, [0.3, -0.5, 0.8]))
    b = np.cross(axis, a)
    phi, z = rng.uniform(0, arc, (m, 1)), rng.uniform(-length / 2, length / 2, (m, 1))
    d = a * np.cos(phi) + b * np.sin(phi)
    return np.asarray(point) + z * axis + d * (radius + sigma * rng.normal(size=(m, 1))), d


TRUTH = {M.SPHERE: dict(centre=np.array([0.1, -0.2, 0.15]), radius=0.6),
         M.CYLINDER: dict(point=np.array([0.1, -0.2, 0.0]), axis=_unit(np.array([0.2, 0.1, 1.0])), radius=0.4, length=1.6)}


def _shape_points(rng, kind, m, sigma):
    t = TRUTH[kind]
    if kind == M.SPHERE:
        return on_sphere(rng, m, t["centre"], t["radius"], sigma)
    return on_cylinder(rng, m, t["point"], t["axis"], t["radius"], t["length"], sigma)


@functools.lru_cache(maxsize=None)
def count_set(kind, special=False, offset=False):
    """(P, N, rows): 40 % of ROWS points on the kind's TRUTH shape (0.2 % radial noise, 2 degrees of normal noise, random normal signs)
    among uniform outliers with random normals, in random order.  rows: a shuffle with duplicates; special: NaN and +-inf coordinates
    and normals, and rows out of range.  offset: the scene moved by FAR."""
    rng = np.random.default_rng(KINDS.index(kind) + 40 + (7 if special else 0))
    n = ROWS
    on = rng.random(n) < 0.4
    P = rng.uniform(-1, 1, (n, 3))
    N = _unit(rng.normal(size=(n, 3)))
    x, d = _shape_points(rng, kind, int(on.sum()), 0.002 * TRUTH[kind]["radius"])
    P[on], N[on] = x, _noisy_normals(rng, d, 2.0)
    if offset:
        P = P + FAR
    P, N = P.astype(F), N.astype(F)
    rows = rng.permutation(n).astype(np.uint32)
    dup = rng.integers(0, n, 100)
    rows[dup] = rows[(dup + 7) % n]
    if special:
        P[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = np.nan
        P[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = np.inf
        P[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = -np.inf
        N[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = np.nan
        N[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = -np.inf
        rows[rng.integers(0, n, 40)] = n
        rows[rng.integers(0, n, 40)] = 0xFFFFFFFF
        rows[1] = n + 5  # (whatever the draw: an unusable row among the first two)
        P[1, 0] = np.nan
    return P, N, rows


@functools.lru_cache(maxsize=None)
def count_model(kind, gated, special, listed, C, origin_row=None):
    """the model's run of T_MAX hypotheses over the first C rows of the count set (listed: rows[:C] of all ROWS points)"""
    P, N, rows = count_set(kind, special)
    if listed:
        return M.ransac(kind, P, N, T_MAX, SEED, TAU, rows=rows[:C], min_normal_cos=COSN if gated else None, origin_row=origin_row)
    return M.ransac(kind, P[:C], N[:C], T_MAX, SEED, TAU, min_normal_cos=COSN if gated else None, origin_row=origin_row)


# ---- exact ties ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ties_scene(kind):
    """(P, N, tau): integer coordinates and normals that are exactly +-x, +-y or +-z, so every hypothesis from two points of the shape
    whose normals differ is the shape itself, exactly, and they all tie.  Sphere: centre (3, -2, 5), radius 7, its six poles 20 times
    each.  Cylinder: the axis through (3, -2, .) along z, radius 5, its four lines x = 3 +- 5 and y = -2 +- 5 at z = -8 .. 8.  Among
    200 integer outliers with axis normals, in random order."""
    rng = np.random.default_rng(60 + KINDS.index(kind))
    eye = np.eye(3)
    if kind == M.SPHERE:
        c, R = np.array([3.0, -2.0, 5.0]), 7.0
        d = np.concatenate([eye, -eye])
        x, nrm = np.repeat(c + R * d, 20, 0), np.repeat(d, 20, 0)
    else:
        c, R = np.array([3.0, -2.0, 0.0]), 5.0
        d = np.concatenate([eye[:2], -eye[:2]])
        z = np.arange(-8, 9, dtype=np.float64)
        x = np.concatenate([c + R * di + np.outer(z, eye[2]) for di in d])
        nrm = np.repeat(d, len(z), 0)
    nrm = nrm * rng.choice([-1.0, 1.0], (len(nrm), 1))
    out = rng.integers(-12, 13, (200, 3)).astype(np.float64)
    out_n = eye[rng.integers(0, 3, 200)] * rng.choice([-1.0, 1.0], (200, 1))
    P, N = np.concatenate([x, out]), np.concatenate([nrm, out_n])
    order = rng.permutation(len(P))
    return P[order].astype(F), N[order].astype(F), 0.25


SHIFT = np.array([1024.0, -1024.0, 2048.0])


# ---- the gates -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gates_scene(kind, patch=False):
    """(P, N): a large shape of 600 points, only 35 % of them with their true normals (the others' are random), and a small one of
    300 points with true normals, among 300 outliers.  The large one wins by its count; its radius, its normals and (cylinder) its
    axis are not the small one's, so each gate can turn it down.  patch: the large shape's points with true normals (0.05 degrees of
    noise) all lie in one patch of it, across which the normals turn by less than 35 degrees: every hypothesis of the large shape
    comes from two normals whose sine is below 0.6."""
    rng = np.random.default_rng(80 + KINDS.index(kind) + (10 if patch else 0))
    if kind == M.SPHERE:
        big, nb = on_sphere(rng, 600, [0.2, 0.1, -0.1], 0.8, 0.001)
        small, nsm = on_sphere(rng, 300, [-0.3, 0.2, 0.3], 0.3, 0.001)
    else:
        big, nb = on_cylinder(rng, 600, [0.2, 0.1, -0.1], [1.0, 0.0, 0.0], 0.6, 1.8, 0.001)
        small, nsm = on_cylinder(rng, 300, [-0.3, 0.2, 0.3], [0.0, 0.0, 1.0], 0.25, 1.2, 0.001)
    wrong = rng.random(600) >= 0.35
    if patch:
        if kind == M.SPHERE:
            d = _unit(np.array([0.0, 0.0, 1.0]) + 0.2 * rng.uniform(-1, 1, (600, 3)) * [1, 1, 0])  # (within 16 degrees of z)
            part, npart = np.array([0.2, 0.1, -0.1]) + 0.8 * d, d
        else:
            part, npart = on_cylinder(rng, 600, [0.2, 0.1, -0.1], [1.0, 0.0, 0.0], 0.6, 1.8, 0.0, arc=0.5)  # (half a radian)
        big[~wrong], nb[~wrong] = part[~wrong], npart[~wrong]
    nb = _noisy_normals(rng, nb, 0.05 if patch else 1.0)
    nb[wrong] = _unit(rng.normal(size=(int(wrong.sum()), 3)))
    nsm = _noisy_normals(rng, nsm, 1.0)
    P = np.concatenate([big, small, rng.uniform(-1, 1, (300, 3))])
    N = np.concatenate([nb, nsm, _unit(rng.normal(size=(300, 3)))])
    order = rng.permutation(len(P))
    return P[order].astype(F), N[order].astype(F)


GATES = {"radius": dict(radius=(0.2, 0.4)), "normals": dict(min_normal_cos=0.95), "axis": dict(axis=np.array([0, 0, 1], F), min_axis_cos=0.9),
         "sin": dict(min_normal_sin=0.7)}
GATE_RADIUS = {M.SPHERE: (0.8, 0.3), M.CYLINDER: (0.6, 0.25)}  # of the large and of the small shape
GATE_NAMES = {M.SPHERE: ("radius", "normals", "sin"), M.CYLINDER: ("radius", "normals", "axis", "sin")}


def gate_arguments(gate):
    """(patch, keywords) of a gate's run; None: the free run of the plain scene, "free-patch": that of the patch scene"""
    if gate in (None, "free-patch"):
        return gate == "free-patch", {}
    return gate == "sin", GATES[gate]


@functools.lru_cache(maxsize=None)
def gates_model(kind, gate):
    patch, kw = gate_arguments(gate)
    P, N = gates_scene(kind, patch)
    return M.ransac(kind, P, N, GATE_T, SEED, TAU, **kw)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
CHAIN = dict(radius=0.12, T=512, tau=0.01, seed=11, shape_radius=0.5, centre=np.array([0.1, 0.0, -0.2]))  # T: test_shapes_cpu.py::test_the_chain_scene...


@functools.lru_cache(maxsize=None)
def chain_scene():
    """P: 1500 points of a sphere (0.1 % radial noise) and 500 uniform ones, without normals: the chain estimates them"""
    rng = np.random.default_rng(120)
    x, _d = on_sphere(rng, 1500, CHAIN["centre"], CHAIN["shape_radius"], 0.0005)
    P = np.concatenate([x, rng.uniform(-1, 1, (500, 3))])
    return P[rng.permutation(len(P))].astype(F)


# ---- the fits ------------------------------------------------------------------------------------------------------------------------------
FIT_SIZES = (3, 4, 17, 257, 16385, 33000)  # below four rows; a thread's one item; one more than the grid of 64 x 256; two items and a rest


@functools.lru_cache(maxsize=None)
def fit_set(kind, m):
    """(P, N): m points of a cap of the sphere (a third of a cylinder's circumference), 0.2 % radial noise, 3 degrees of normal noise,
    at the offset FAR"""
    rng = np.random.default_rng(100 + m + KINDS.index(kind))
    if kind == M.SPHERE:
        x, d = on_sphere(rng, 3 * m + 10, [0.0, 0.0, 0.0], 0.7, 0.0014)
        keep = np.nonzero(d[:, 2] > 0.3)[0][:m]
        assert len(keep) == m
        x, d = x[keep], d[keep]
    else:
        x, d = on_cylinder(rng, m, [0.0, 0.0, 0.0], TRUTH[kind]["axis"], 0.4, 1.5, 0.0008, arc=2 * np.pi / 3)
    return (x + FAR).astype(F), _noisy_normals(rng, d, 3.0).astype(F)
