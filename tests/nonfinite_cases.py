"""The clouds, queries, radii, boxes and fields of tests/test_nonfinite_cpu.py and tests/test_gpu_nonfinite.py: coordinates and
field values that are NaN or +-inf ("Non-finite coordinates").  Seeded, built once, read-only.

Clouds are derived from the uniform clouds of tests/handle_history_cases.py (c1300: three tree levels, 163 leaves, 21 query
groups; c70; and nine points), by overwriting coordinates of some rows:

    nan_rows       NaN in one random coordinate of min(40, n // 2) rows, rows 0 and n - 1 among them
    inf_rows       the same rows and coordinates with +inf and -inf, alternating
    mixed          both kinds, one row all NaN, one row (+inf, -inf, NaN)
    odd_nans       the NaN bit patterns 0xFFC00000 (sign set), 0x7F800001 (signalling) and 0xFFFFFFFF, through a uint32 view
    survivors_mod  three variants of c1300 whose finite rows number 1280 (= 0 mod 64), 1288 (= 0 mod 8, not 64), 1289 (= 1 mod 8)
    one_finite     65 rows, only row 37 finite
    none_finite    70 rows, every one with a NaN or an infinite coordinate
    inf_axis       c1300 with every x = +inf

A case is (points, finite): `finite` marks the rows with three finite coordinates, the only rows an index holds.  The query sets
are asked of the finite c1300 cloud.  What a kernel must return comes from brute force over the finite rows with the indices
mapped back (`knn_over_finite`, `count_over_finite`, `sphere_lists`, `box_lists`): IEEE comparisons, so a NaN distance is never a
neighbour and +inf is an ordinary value."""
import functools

import numpy as np

import handle_history_cases as Cs

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
ODD_NANS = (0xFFC00000, 0x7F800001, 0xFFFFFFFF)
BASES = {1300: "c1300", 70: "c70"}
SIZES = (1300, 70, 9)
KINDS = ("nan_rows", "inf_rows", "mixed", "odd_nans")
SURVIVORS = {"mod64": 1280, "mod8": 1288, "mod8_plus1": 1289}
ONE_FINITE_ROW = 37


def base(n):
    """the finite cloud of n points every case of that size is derived from"""
    if n in BASES:
        return Cs.inputs(BASES[n])["points"]
    return np.random.default_rng(4000 + n).uniform(0, 1, (n, 3)).astype(F)


def _rows_and_axes(n, count, seed):
    """`count` rows, rows 0 and n - 1 among them, and one axis for each"""
    rng = np.random.default_rng(seed)
    inner = rng.permutation(np.arange(1, n - 1))[:count - 2]
    rows = np.concatenate([[0, n - 1], inner]).astype(np.int64)
    return rows, rng.integers(0, 3, count)


def bad_count(n):
    return min(40, n // 2)


@functools.lru_cache(maxsize=None)
def cloud(kind, n=1300):
    """(points, finite) of a case, by name"""
    pts = base(n).copy() if kind not in ("one_finite", "none_finite") else None
    if kind in KINDS:
        rows, axes = _rows_and_axes(n, bad_count(n), 900 + n)
        if kind == "nan_rows":
            pts[rows, axes] = np.nan
        elif kind == "inf_rows":
            pts[rows, axes] = np.where(np.arange(len(rows)) % 2 == 0, np.inf, -np.inf).astype(F)
        elif kind == "mixed":
            vals = np.array([np.nan, np.inf, -np.inf], F)[np.arange(len(rows)) % 3]
            pts[rows, axes] = vals
            pts[rows[2]] = np.nan
            pts[rows[3]] = np.array([np.inf, -np.inf, np.nan], F)
        else:
            bits = pts.view(np.uint32)
            bits[rows, axes] = np.array(ODD_NANS, np.uint32)[np.arange(len(rows)) % 3]
    elif kind in SURVIVORS:
        assert n == 1300
        rows, axes = _rows_and_axes(n, n - SURVIVORS[kind], 950 + SURVIVORS[kind])
        pts[rows, axes] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(len(rows)) % 3]
    elif kind == "one_finite":
        pts = np.random.default_rng(965).uniform(0, 1, (65, 3)).astype(F)
        rows = np.delete(np.arange(65), ONE_FINITE_ROW)
        pts[rows, np.arange(64) % 3] = np.array([np.nan, -np.inf, np.inf, np.nan], F)[np.arange(64) % 4]
    elif kind == "none_finite":
        pts = np.random.default_rng(970).uniform(0, 1, (70, 3)).astype(F)
        pts[np.arange(70), np.arange(70) % 3] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(70) % 3]
    elif kind == "inf_axis":
        pts[:, 0] = np.inf
    else:
        raise ValueError(kind)
    finite = np.isfinite(pts).all(1)
    pts.setflags(write=False)
    finite.setflags(write=False)
    return pts, finite


def all_clouds():
    """every (kind, n) there is"""
    out = [(kind, n) for kind in KINDS for n in SIZES]
    out += [(kind, 1300) for kind in SURVIVORS] + [("one_finite", 65), ("none_finite", 70), ("inf_axis", 1300)]
    return out


def finite_box(pts, finite):
    """the box an index of the cloud reports: of the finite rows (no finite row: the empty box, as for no point at all)"""
    if not finite.any():
        big = np.finfo(F).max
        return np.array([big] * 3 + [-big] * 3, F)
    sub = pts[finite]
    return np.concatenate([sub.min(0), sub.max(0)]).astype(F)


def twin(pts, finite):
    """(points, voxel grid): the same cloud with every non-finite row moved to a finite place outside the finite rows' box, and that
    box as an explicit grid -- an index of it drops the same rows, for being outside the grid (the contract that was there before)"""
    assert finite.any()
    box = finite_box(pts, finite)
    out = pts.copy()
    out[~finite] = box[3:] + F(1) + np.arange(int((~finite).sum()), dtype=F)[:, None]
    return out, box


# ---- queries ------------------------------------------------------------------------------------------------------------------------
def _bad_queries(rng, count):
    """`count` queries, each with a NaN or an infinite coordinate (every third one both), odd NaN bit patterns among them"""
    q = rng.uniform(-0.1, 1.1, (count, 3)).astype(F)
    vals = np.array([np.nan, np.inf, -np.inf], F)
    for i in range(count):
        q[i, rng.integers(0, 3)] = vals[i % 3]
        if i % 3 == 2 and i % 2 == 0:
            q[i, (int(np.nonzero(np.isinf(q[i]))[0][0]) + 1) % 3] = np.nan
    bits = q.view(np.uint32)
    nan_at = np.argwhere(np.isnan(q))
    for j, (r, a) in enumerate(nan_at[::2]):
        bits[r, a] = ODD_NANS[j % 3]
    return q


@functools.lru_cache(maxsize=None)
def queries(name):
    """a query set over the finite c1300 cloud, by name:
        all_bad    one group of 64, every query non-finite
        first / last / middle   64 queries, entry 0 (and 1) / 63 / 31 non-finite (a kernel orders a batch along its curve before it deals
                   the queries to lanes, so the entry's lane is the kernel's choice; the three sets differ in where the curve puts it)
        many       600 queries (the throughput path at any k), every seventh non-finite
        one_nan / one_inf / one_odd   a single query"""
    rng = np.random.default_rng({"all_bad": 1, "first": 2, "last": 3, "middle": 4, "many": 5, "one_nan": 6, "one_inf": 7, "one_odd": 8}[name])
    if name == "all_bad":
        q = _bad_queries(rng, 64)
    elif name in ("first", "last", "middle"):
        q = rng.uniform(-0.05, 1.05, (64, 3)).astype(F)
        at = {"first": 0, "last": 63, "middle": 31}[name]
        # (NaN and -inf quantise to cell 0 of an axis, +inf to the last one: the first set's entry has the curve's first key and sorts
        #  to lane 0, the second set's sits in the cell (last, 0, 0), where the curve ends; the third is wherever its finite part is)
        q[at] = {"first": [np.nan, np.nan, np.nan], "last": [np.inf, -np.inf, np.nan], "middle": [0.5, np.nan, 0.45]}[name]
        if name == "first":
            q[1] = [-np.inf, 0.3, 0.2]  # (and an infinite query beside it)
    elif name == "many":
        q = rng.uniform(-0.05, 1.05, (600, 3)).astype(F)
        q[::7] = _bad_queries(rng, len(q[::7]))
    elif name == "one_nan":
        q = np.array([[0.4, np.nan, 0.6]], F)
    elif name == "one_inf":
        q = np.array([[0.4, 0.5, -np.inf]], F)
    else:
        q = np.array([[0.4, 0.5, 0.6]], F)
        q.view(np.uint32)[0, 0] = ODD_NANS[0]
    q.setflags(write=False)
    return q


QUERY_SETS = ("all_bad", "first", "last", "middle", "many", "one_nan", "one_inf", "one_odd")


def kinds_of(q):
    """(has a NaN, has an infinite coordinate and no NaN) per query"""
    nan = np.isnan(q).any(1)
    return nan, np.isinf(q).any(1) & ~nan


RADIUS = F(0.09)  # about four points of c1300 to a sphere


@functools.lru_cache(maxsize=None)
def spheres():
    """(centres, radii): 96 spheres over c1300, radii NaN, -1, 0, +inf and ordinary in turn, every fifth centre non-finite"""
    rng = np.random.default_rng(11)
    c = rng.uniform(0, 1, (96, 3)).astype(F)
    c[:20] = base(1300)[rng.permutation(1300)[:20]]  # (centres on points: radius 0 holds them)
    c[4::5] = _bad_queries(rng, len(c[4::5]))
    r = np.array([np.nan, -1.0, 0.0, np.inf, RADIUS, 2 * RADIUS], F)[np.arange(96) % 6]
    c.setflags(write=False)
    r.setflags(write=False)
    return c, r


@functools.lru_cache(maxsize=None)
def boxes():
    """48 boxes over c1300: ordinary ones, a NaN in one bound, (-inf, +inf), half-infinite ones, min above max"""
    rng = np.random.default_rng(12)
    lo = rng.uniform(0, 0.8, (48, 3)).astype(F)
    b = np.concatenate([lo, lo + rng.uniform(0.05, 0.4, (48, 3)).astype(F)], 1)
    for i in range(48):
        what = i % 6
        if what == 1:
            b[i, rng.integers(0, 6)] = np.nan
        elif what == 2:
            b[i, :3], b[i, 3:] = -np.inf, np.inf
        elif what == 3:
            b[i, rng.integers(0, 3)] = -np.inf
        elif what == 4:
            b[i, 3 + rng.integers(0, 3)] = np.inf
        elif what == 5 and i % 12 == 5:
            b[i, 0], b[i, 3] = np.inf, -np.inf
    b.setflags(write=False)
    return b


# ---- what brute force over the finite rows gives ------------------------------------------------------------------------------------
def knn_over_finite(oracle, pts, finite, q, k, eps, threads=16):
    """(idx, cnt, d2) of oracle.knn_bruteforce over the finite rows, the indices those of `pts`"""
    rows = np.nonzero(finite)[0]
    if len(rows) == 0:
        return np.full((len(q), k), NONE, np.uint32), np.zeros(len(q), np.uint32), np.full((len(q), k), np.inf, F)
    idx, cnt, d2 = oracle.knn_bruteforce(np.ascontiguousarray(pts[rows]), q, k, eps, nthreads=threads, want_d2=True)
    live = idx != NONE
    out = np.full(idx.shape, NONE, np.uint32)
    out[live] = rows[idx[live].astype(np.int64)]
    return out, cnt, d2


def _d2(pts, c):
    d = pts - c[None, :]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def sphere_lists(pts, finite, centres, radii):
    """per sphere the ascending rows with d2 <= r * r in float32 (sphere.hpp:27-35), among the finite rows"""
    with np.errstate(invalid="ignore"):
        return [np.nonzero((_d2(pts, c) <= F(r) * F(r)) & finite)[0] for c, r in zip(centres, np.broadcast_to(radii, len(centres)))]


def box_lists(pts, finite, bxs):
    with np.errstate(invalid="ignore"):
        return [np.nonzero(((pts >= b[None, :3]) & (pts <= b[None, 3:])).all(1) & finite)[0] for b in bxs]


def lists_of(off, idx):
    return [np.sort(idx[a:b]) for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64))]


# ---- kd clouds ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kd_case(kind, dims):
    """(points, queries, boxes) of a kd index with `dims` coordinates: 700 points with the rows of `kind` (nan_rows, inf_rows,
    odd_nans) made non-finite in one coordinate, 40 queries of which every fifth is non-finite, 12 boxes"""
    rng = np.random.default_rng(1000 + dims)
    pts = rng.uniform(0, 1, (700, dims)).astype(F)
    rows = rng.permutation(700)[:40]
    axes = rng.integers(0, dims, 40)
    if kind == "nan_rows":
        pts[rows, axes] = np.nan
    elif kind == "inf_rows":
        pts[rows, axes] = np.where(np.arange(40) % 2 == 0, np.inf, -np.inf).astype(F)
    else:
        pts.view(np.uint32)[rows, axes] = np.array(ODD_NANS, np.uint32)[np.arange(40) % 3]
    q = rng.uniform(0, 1, (40, dims)).astype(F)
    q[:10] = np.where(np.isfinite(pts[:10]), pts[:10], F(0.5))
    q[4::5, rng.integers(0, dims, 8)] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(8) % 3]
    lo = rng.uniform(0, 0.3, (12, dims)).astype(F)
    bx = np.concatenate([lo, lo + F(0.6)], 1)
    bx[1, 0] = np.nan
    bx[2, :dims], bx[2, dims:] = -np.inf, np.inf
    bx[3, dims + 1] = np.inf
    for a in (pts, q, bx):
        a.setflags(write=False)
    return pts, q, bx


# ---- distance fields ----------------------------------------------------------------------------------------------------------------
def _sphere(dims, radius=0.7):
    """a grid of exactly dims cubes over [-1, 1]^3 and a sphere's distance at its corners"""
    import surface_nets_model as M
    g = M.grid_dict(-1, -1, -1, F(2) / F(dims[0]), F(2) / F(dims[1]), F(2) / F(dims[2]), *dims)
    return g, M.sphere_field(g, radius).astype(F).copy()


FIELDS = ("nan12", "posinf12", "neginf12", "mixed12", "mixed_33x20x41", "all_nan")


@functools.lru_cache(maxsize=None)
def field(name):
    """(grid, field): a sphere's distance field with corners overwritten -- 40 of a 12^3 grid's with NaN, +inf, -inf or all three,
    150 of a 33 x 20 x 41 grid's (no two extents equal, none a multiple of a kernel's tile) with all three, and a 12^3 field of NaN
    alone.  The corners are drawn near the surface (|f| < 0.25) so that they sit in active cubes."""
    if name == "all_nan":
        g, f = _sphere((12, 12, 12))
        f[:] = np.nan
    else:
        g, f = _sphere((33, 20, 41) if name == "mixed_33x20x41" else (12, 12, 12))
        rng = np.random.default_rng({"nan12": 21, "posinf12": 22, "neginf12": 23, "mixed12": 24, "mixed_33x20x41": 25}[name])
        near = np.nonzero(np.abs(f) < 0.25)[0]
        at = rng.permutation(near)[:150 if name == "mixed_33x20x41" else 40]
        vals = {"nan12": [np.nan], "posinf12": [np.inf], "neginf12": [-np.inf]}.get(name, [np.nan, np.inf, -np.inf])
        f[at] = np.array(vals, F)[np.arange(len(at)) % len(vals)]
    f.setflags(write=False)
    return g, f
