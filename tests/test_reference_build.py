"""CPU tests: every restatement the suite trusts, against a real build of the reference's headers (oracle/pcp_ref.py).

The kernels are compared with the restatements everywhere else (test_gpu_*); here the restatements themselves are pinned to
the reference: oracle/pcp_oracle.cpp's octree kNN and ranges (including the radius > 1 prune quirk), the numpy kd-tree
restatement for K = 1 ... 16, mean neighbour distance, both surface-nets models and WLOP.  Skipped only where the reference's
source is absent and no build of it is at hand."""
import os

import numpy as np
import pytest

import surface_nets_hint_model as H
import surface_nets_model as M
from conftest import knn_rows_equivalent
from oracle import pcp_ref as R

F = np.float32
pytestmark = pytest.mark.skipif(not R.available(), reason="no build of the reference: %s" % R.why_unavailable())
NT = min(16, os.cpu_count() or 1)
POS_TOL = 4e-6       # tests/test_gpu_filters.py: WLOP after one iteration, relative to the cloud's extent
FLIP_FRACTION = 2e-3  # ... and the fraction of rows a range-boundary flip may move beyond it


# ---- clouds ----------------------------------------------------------------------------------------------------------------
def _cloud(name, n, seed=0):
    rng = np.random.default_rng(seed)
    if name == "uniform":
        return rng.random((n, 3)).astype(F)
    if name == "clustered":
        c = rng.random((8, 3))
        return (c[rng.integers(0, 8, n)] + rng.normal(0, 0.01, (n, 3))).astype(F)
    if name == "lattice":  # exact ties: integer / 8 coordinates
        m = int(np.ceil(n ** (1 / 3)))
        g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        return (g[rng.permutation(len(g))] / 8.0).astype(F)
    if name == "duplicates":
        base = rng.random((n // 4, 3)).astype(F)
        return base[rng.integers(0, len(base), n)]
    if name == "slab":
        p = rng.random((n, 3))
        p[:, 2] *= 1e-4
        return p.astype(F)
    if name == "dynamic":  # large dynamic range: a dense core inside a wide shell
        p = rng.normal(0, 1, (n, 3))
        p *= np.where(rng.random(n) < 0.5, 1e-3, 1e3)[:, None]
        return p.astype(F)
    raise ValueError(name)


CLOUDS = ["uniform", "clustered", "lattice", "duplicates", "slab", "dynamic"]


def _queries(pts, n_self, n_out, seed=1):
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(0), pts.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    out = lo - 0.3 * ext + rng.random((n_out, 3)) * 1.6 * ext  # part of it outside the cloud's box
    out[: n_out // 2, 0] = hi[0] + ext[0] * (0.1 + rng.random(n_out // 2))  # surely outside
    return np.concatenate([pts[rng.choice(len(pts), n_self, replace=False)], out.astype(F)]).astype(F)


# ---- octree kNN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloud", CLOUDS)
@pytest.mark.parametrize("n", [700, 3000])
def test_octree_knn_against_reference(oracle, cloud, n):
    pts = _cloud(cloud, n, seed=n)
    q = _queries(pts, 120, 40)
    ref, orc = R.Octree(pts), oracle.Octree(pts)
    assert ref.size() == orc.size() == len(pts)
    assert np.array_equal(ref.voxel_grid(), orc.voxel_grid())
    for k in (1, 2, 15, 16, 17, 32, 33, 40, 70):
        for eps in (0.0, 1e-7, 1e-5, 1e-3):
            ri, rc = ref.knn(q, k, eps)
            for name, (oi, oc) in (("octree", orc.knn(q, k, eps, nthreads=NT)),
                                   ("bruteforce", oracle.knn_bruteforce(pts, q, k, eps, nthreads=NT))):
                ok, why = knn_rows_equivalent(pts, q, ri, rc, oi, oc)
                assert ok, (cloud, n, k, eps, name, why)


@pytest.mark.parametrize("cap,depth", [(1, 21), (4, 3), (32, 21), (200, 2)])
def test_octree_knn_parameters_and_grid(oracle, cap, depth):
    """The explicit constructor (node capacity, depth, a voxel grid that drops points) against the oracle's same arguments."""
    pts = _cloud("uniform", 2500, seed=3)
    grid = np.array([0.1, 0.0, 0.2, 0.9, 0.8, 1.0], F)
    q = _queries(pts, 80, 30)
    for g in (None, grid):
        ref, orc = R.Octree(pts, cap, depth, g), oracle.Octree(pts, cap, depth, g)
        assert ref.size() == orc.size()
        if g is not None:
            assert ref.size() < len(pts)
        for k in (1, 16, 33):
            ri, rc = ref.knn(q, k)
            oi, oc = orc.knn(q, k)
            ok, why = knn_rows_equivalent(pts, q, ri, rc, oi, oc)
            assert ok, (cap, depth, g is not None, k, why)


# ---- octree ranges ---------------------------------------------------------------------------------------------------------
def _brute_sphere(pts, c, r):
    d = pts - np.asarray(c, F)[None, :]
    return np.nonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= F(r) * F(r))[0]


DROP_GRID = np.array([0.1, 0.0, 0.2, 0.9, 0.8, 1.0], F)  # a voxel grid that leaves points of the unit cube out


@pytest.mark.parametrize("grid", [None, DROP_GRID], ids=["bbox", "dropping_grid"])
@pytest.mark.parametrize("cloud", ["uniform", "lattice", "duplicates", "clustered"])
def test_octree_range_sphere_small_radius(oracle, cloud, grid):
    """r <= 1: the reference's sets equal the oracle's, and brute force over the points the tree holds."""
    pts = _cloud(cloud, 4000, seed=7)
    ref, orc = R.Octree(pts, 32, 21, grid), oracle.Octree(pts, 32, 21, grid)
    held = np.arange(len(pts))
    if grid is not None:
        assert ref.size() == orc.size() < len(pts)
        held = np.unique(np.concatenate([ref.range_aabb(grid[:3] - F(1), grid[3:] + F(1))]))
        assert len(held) == ref.size()
    q = _queries(pts, 60, 20)
    for r in (0.0, 1e-6, 0.05, 0.125, 0.3, 1.0):
        for c in q:
            got = ref.range_sphere(c, r)
            assert np.array_equal(got, np.sort(orc.range_sphere(c, r))), (cloud, r)
            assert np.array_equal(got, np.intersect1d(_brute_sphere(pts, c, r), held)), (cloud, r)


@pytest.mark.parametrize("grid", [None, DROP_GRID * F(12)], ids=["bbox", "dropping_grid"])
def test_octree_range_sphere_radius_above_one(oracle, grid):
    """r > 1: the reference prunes boxes against `radius` where it means radius^2 (DESIGN.md 'Semantics'): its sets equal
    the oracle's quirk mode exactly (set_geometric_prune(False), the default), are subsets of brute force, and do drop
    points somewhere -- the documented difference is real, not a reading of it."""
    pts = (_cloud("uniform", 6000, seed=9) * F(12)).astype(F)
    ref = R.Octree(pts, 8, 21, grid)
    oracle.set_geometric_prune(False)
    orc = oracle.Octree(pts, 8, 21, grid)
    assert ref.size() == orc.size() and (grid is None) == (ref.size() == len(pts))
    q = _queries(pts, 60, 20)
    dropped = 0
    for r in (1.0001, 1.5, 2.0, 3.7):
        for c in q:
            got = ref.range_sphere(c, r)
            assert np.array_equal(got, np.sort(orc.range_sphere(c, r))), r
            bf = _brute_sphere(pts, c, r)
            assert np.isin(got, bf).all()
            dropped += len(bf) - len(got)
    assert dropped > 0
    # the same spheres through the per-sphere-radius entry point
    radii = np.resize(np.array([0.0, 1e-6, 0.4, 1.5, 3.7], F), len(q))
    cnt = ref.range_counts(q, radii)
    assert [len(ref.range_sphere(c, r)) for c, r in zip(q, radii)] == cnt.tolist()


@pytest.mark.parametrize("cloud", ["lattice", "duplicates", "uniform"])
def test_octree_range_aabb_faces_inclusive(oracle, cloud):
    """Boxes whose faces pass exactly through points: inclusive on every face, as the oracle."""
    pts = _cloud(cloud, 3000, seed=11)
    rng = np.random.default_rng(5)
    for g in (None, np.array([0.0, 0.0, 0.0, 0.6, 0.7, 0.5], F)):
        ref, orc = R.Octree(pts, 16, 21, g), oracle.Octree(pts, 16, 21, g)
        for _ in range(60):
            a, b = pts[rng.integers(0, len(pts), 2)]
            lo, hi = np.minimum(a, b), np.maximum(a, b)
            got = ref.range_aabb(lo, hi)
            assert np.array_equal(got, np.sort(orc.range_aabb(lo, hi)))
            if g is None:
                assert np.array_equal(got, np.nonzero(((pts >= lo) & (pts <= hi)).all(1))[0])
                assert np.isin(np.nonzero((pts == a).all(1))[0], got).all()  # the corner points are inside


# ---- kd-trees, K = 1 ... 16 ------------------------------------------------------------------------------------------------
def _kd_d2(pts, q):
    acc = np.zeros(len(pts), F)
    for a in range(pts.shape[1]):
        d = pts[:, a] - q[a]
        acc = acc + d * d
    return acc


def _kd_rows_equivalent(pts, qs, ia, ca, ib, cb):
    if not np.array_equal(ca, cb):
        return False, "counts differ"
    for j, q in enumerate(qs):
        c = int(ca[j])
        a, b = ia[j, :c].astype(np.int64), ib[j, :c].astype(np.int64)
        if not np.array_equal(a, b) and not np.array_equal(_kd_d2(pts[a], q), _kd_d2(pts[b], q)):
            return False, "row %d: distance lists differ" % j
    return True, ""


def _kd_cloud(kind, n, K, seed):
    rng = np.random.default_rng(seed)
    if kind == "lattice":
        return rng.integers(0, 3, (n, K)).astype(F) * F(0.25)  # many exact ties and duplicates
    if kind == "duplicates":
        base = rng.random((n // 3, K)).astype(F)
        return base[rng.integers(0, len(base), n)]
    return rng.random((n, K)).astype(F)


@pytest.mark.parametrize("K", list(range(1, 17)))
def test_kd_knn_and_aabb_against_reference(oracle, K):
    for kind in ("uniform", "lattice", "duplicates"):
        pts = _kd_cloud(kind, 1500, K, K)
        rng = np.random.default_rng(K + 100)
        q = np.concatenate([pts[rng.choice(len(pts), 40, replace=False)], rng.random((10, K)).astype(F) * F(1.4) - F(0.2)])
        for params in (None, (12, True, 64), (3, False, 8)):
            t = R.KdTree(pts, params)
            for k in (1, 15, 33):
                for eps in (0.0, 1e-5):
                    ri, rc = t.knn(q, k, eps)
                    bi, bc, _ = oracle.kd_knn_bruteforce(pts, q, k, eps)
                    ok, why = _kd_rows_equivalent(pts, q, ri, rc, bi, bc)
                    assert ok, (kind, params, k, eps, why)
            a, b = pts[rng.integers(0, len(pts), (2, 12))]
            boxes = np.concatenate([np.minimum(a, b), np.maximum(a, b)], 1)  # faces through points
            want = oracle.kd_range_aabb(pts, boxes)
            for bb, w in zip(boxes, want):
                assert np.array_equal(t.range_aabb(bb), w), (kind, params)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 16])
def test_kd_bruteforce_order_is_d2_then_index(oracle, K):
    """The reference breaks ties at equal distance in its heap's order, so it cannot pin kd_knn_bruteforce's tie rule; its
    documented order -- ascending (d2, index), d2 summed axis by axis in float32, eps-box points skipped -- is checked
    exactly here, on a lattice full of ties, against a plain sort of (d2, index) pairs."""
    pts = _kd_cloud("lattice", 400, K, 50 + K)
    q = np.concatenate([pts[:20], np.full((1, K), 0.3, F)])
    for k in (1, 7, 40):
        for eps in (0.0, 1e-5):
            idx, cnt, d2 = oracle.kd_knn_bruteforce(pts, q, k, eps)
            for j, qq in enumerate(q):
                dd = _kd_d2(pts, qq)
                skip = (np.abs(pts - qq) < F(eps)).all(1) if eps > 0 else np.zeros(len(pts), bool)
                want = sorted((float(dd[i]), i) for i in range(len(pts)) if not skip[i])[:k]
                assert int(cnt[j]) == len(want)
                assert idx[j, :cnt[j]].tolist() == [i for _, i in want], (K, k, eps, j)
                assert d2[j, :cnt[j]].tolist() == [d for d, _ in want]


def test_kd_knn_3d_matches_oracle_kdtree(oracle):
    """K = 3: the reference kd-tree against the C++ restatement's KdTree with the parameters it exposes."""
    pts = _cloud("lattice", 3000, seed=2)
    q = _queries(pts, 100, 30)
    for md, cmd, leaf in ((12, False, 64), (12, True, 64), (4, False, 16)):
        ri, rc = R.KdTree(pts, (md, cmd, leaf)).knn(q, 16)
        oi, oc = oracle.KdTree(pts, md, cmd, leaf).knn(q, 16)
        ok, why = knn_rows_equivalent(pts, q, ri, rc, oi, oc)
        assert ok, why


# ---- mean neighbour distance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloud", ["uniform", "lattice", "dynamic"])
@pytest.mark.parametrize("k", [1, 15, 40])
def test_mean_distance_bit_for_bit(oracle, cloud, k):
    pts = _cloud(cloud, 3000, seed=4)
    idx, cnt = oracle.knn_bruteforce(pts, pts, k, nthreads=NT)
    assert cnt.min() > 0
    got = oracle.mean_dist_from_knn(pts, pts, idx, cnt)
    assert np.array_equal(got.view(np.uint32), R.average_distances_to_neighbors(pts, idx, cnt).view(np.uint32))


# ---- surface nets ----------------------------------------------------------------------------------------------------------
def _surface_fields():
    from test_gpu_surface import _fields
    out = list(_fields())
    g, e = _anisotropic()
    out.append(("anisotropic", g, e, 0.0))
    return out


ANISO_CENTRE = (1.675, -0.65, 3.1)


def _anisotropic():
    """dx != dy != dz, a non-zero origin, z the longest axis; an ellipsoid well inside."""
    g = M.grid_dict(0.3, -1.7, 2.1, 0.11, 0.07, 0.05, 25, 30, 40)
    p = M.corner_positions(g) - np.array(ANISO_CENTRE, F)
    e = np.sqrt((p[:, 0] / F(1.1)) ** 2 + (p[:, 1] / F(0.8)) ** 2 + (p[:, 2] / F(0.7)) ** 2) - F(1)
    return g, e.astype(F)


SURFACE_FIELDS = _surface_fields()


def _by_first_vertex(t):
    """The reference emits each cube's triangles together, in its quad order, but walks the cubes in hash-map order: a
    stable sort on the first vertex (the cube's own) gives the models' cube order."""
    return t[np.argsort(t[:, 0], kind="stable")] if len(t) else t


@pytest.mark.parametrize("name,g,field,iso", SURFACE_FIELDS, ids=[f[0] for f in SURFACE_FIELDS])
def test_surface_nets_model_against_reference(name, g, field, iso):
    f = M.sphere_field(g) if field is None else field
    mv, mt = M.surface_nets(f, g, iso)
    if g["sx"] > max(g["sy"], g["sz"]) or g["sy"] > max(g["sx"], g["sz"]):
        # DESIGN.md section 13, 'Every cube once': with x or y strictly longest the reference's swapped loop counters
        # walk cubes outside the grid (f is read there: +1, the sign of these fields beyond the grid, so none is active)
        # and in another order.  The mesh is the same: equal vertices as a set, bit for bit, and equal triangles once the
        # reference's vertex numbers are mapped to the model's.
        rv, rt = R.surface_nets(f, g, iso, outside=1.0)
        assert rv.shape == mv.shape and rt.shape == mt.shape, (name, rv.shape, mv.shape, rt.shape, mt.shape)
        at = {bytes(v): i for i, v in enumerate(mv)}
        assert len(at) == len(mv)
        remap = np.array([at[bytes(v)] for v in rv], np.uint32)
        assert np.array_equal(np.sort(remap), np.arange(len(mv)))
        assert np.array_equal(_by_first_vertex(remap[rt]), mt), "triangles differ"
        return
    rv, rt = R.surface_nets(f, g, iso)
    assert rv.shape == mv.shape and rt.shape == mt.shape, (name, rv.shape, mv.shape, rt.shape, mt.shape)
    assert np.array_equal(rv.view(np.uint32), mv.view(np.uint32)), "vertices differ in bits or order"
    assert np.array_equal(_by_first_vertex(rt), mt), "triangles differ"


def _hint_cases():
    """(name, field, grid, hint): tests/test_gpu_surface_hint.py's cases whose surface stays inside the grid, with hints
    inside, on and outside the surface.  The field is positive on the grid's faces, so the value the reference reads past
    them (+1, the faces' sign) keeps every cube outside the grid inactive, as the model's grid-keyed search assumes."""
    out = []
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (5, 5, 5))
    f = M.sphere_field(g)
    out += [("kat_on", f, g, (0, 0, 0.99)), ("kat_inside", f, g, (0.05, 0.02, 0.0)), ("kat_outside", f, g, (1.2, 1.2, 1.2))]
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (48, 48, 48))
    f = np.minimum(M.sphere_field(g, 0.4, (-0.5, 0, 0)), M.sphere_field(g, 0.3, (0.5, 0.1, 0)))
    out += [("two_spheres_left", f, g, (-0.5, 0, 0.35)), ("two_spheres_right", f, g, (0.5, 0.1, -0.22))]
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (24, 24, 24))
    r = np.sqrt((M.corner_positions(g).astype(F) ** 2).sum(1)).astype(F)
    f = (np.abs(r - F(0.6)) - F(0.15)).astype(F)
    out += [("shells_" + n, f, g, h) for n, h in (("inside", (0.02, 0.01, 0.0)), ("between", (0.6, 0.0, 0.01)),
                                                  ("outside", (0.0, -0.92, 0.0)))]
    g, e = _anisotropic()
    c = ANISO_CENTRE
    out += [("anisotropic_inside", e, g, c), ("anisotropic_on", e, g, (c[0], c[1], c[2] + 0.7))]
    return out


HINT_CASES = _hint_cases()


@pytest.mark.parametrize("name,f,g,hint", HINT_CASES, ids=[c[0] for c in HINT_CASES])
def test_surface_nets_hint_model_against_reference(name, f, g, hint):
    mv, mt, mc, seed = H.surface_nets_hint(f, g, hint)  # seed None: the first search met its bound, the whole grid
    rv, rt = R.surface_nets(f, g, 0.0, hint=hint, outside=1.0)
    assert rv.shape == mv.shape and rt.shape == mt.shape, (name, rv.shape, mv.shape, rt.shape, mt.shape)
    assert np.array_equal(rv.view(np.uint32), mv.view(np.uint32)), "vertices differ in bits or search order"
    assert np.array_equal(_by_first_vertex(rt), _by_first_vertex(mt)), "triangles differ"
    assert len(rt) > 0


# ---- WLOP ------------------------------------------------------------------------------------------------------------------
def _wlop_cloud(uniform_cloud, n, seed):
    rng = np.random.default_rng(seed)
    if uniform_cloud:
        return rng.random((n, 3)).astype(F)
    p = rng.random((n, 3))
    p[: n // 2] *= 0.3  # half the points in a corner eight times denser
    return p.astype(F)


@pytest.mark.parametrize("uniform_cloud", [True, False], ids=["uniform_cloud", "nonuniform_cloud"])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("uniform", [True, False], ids=["wlop", "lop"])
def test_wlop_against_reference(oracle, uniform_cloud, iters, uniform):
    """The oracle's WLOP against the header's own pieces from the same sample.  The sample is the last I points: the
    header writes its densities v_j in shuffled order and reads them by point index (wlop.hpp:371-381 against :338-340),
    which agrees with reading them by point index only when the shuffle left the points in order (DESIGN.md 'Semantics')."""
    n, m = 3000, 1000
    pts = _wlop_cloud(uniform_cloud, n, iters)
    sample = np.arange(n - m, n, dtype=np.uint64)
    h = 0.12
    want = R.wlop_from_sample(pts, sample, 0.45, h, iters, uniform)
    got = oracle.wlop(pts, sample, 0.45, h, iters, uniform=uniform, nthreads=NT)
    assert np.isfinite(want).all() and np.abs(want - pts[sample.astype(np.int64)]).max() > 1e-3
    ext = float((pts.max(0) - pts.min(0)).max())
    d = np.abs(got - want).max(axis=1)
    if iters == 1:
        assert d.max() <= POS_TOL * ext
    else:
        assert float(np.mean(d > POS_TOL * ext)) <= FLIP_FRACTION and d.max() <= 1e-2


def test_lop_any_sample_against_reference(oracle):
    """uniform = false (LOP): every v_j is 1, so any sample agrees with the header."""
    pts = _wlop_cloud(False, 3000, 5)
    sample = np.random.default_rng(6).choice(3000, 800, replace=False).astype(np.uint64)
    want = R.wlop_from_sample(pts, sample, 0.45, 0.12, 1, False)
    got = oracle.wlop(pts, sample, 0.45, 0.12, 1, uniform=False, nthreads=NT)
    assert np.abs(got - want).max() <= POS_TOL


def test_public_wlop_whole_cloud_is_a_permutation(oracle):
    """The public wlop() with I = J (its sample drawn from std::random_device).  LOP: the shuffle only permutes the result,
    so its rows match the oracle's from the identity sample one to one.  WLOP: the header's v_j, written in shuffled order
    and read by point index (DESIGN.md 'Semantics'), move the rows off the oracle's."""
    n = 1200
    pts = _wlop_cloud(True, n, 8)
    for uniform in (False, True):
        want = oracle.wlop(pts, np.arange(n, dtype=np.uint64), 0.45, 0.15, 1, uniform=uniform, nthreads=NT)
        got = R.wlop_public(pts, n, 0.45, 0.15, 1, uniform=uniform)
        d = np.abs(got[:, None, :] - want[None, :, :]).max(2)
        match = d.argmin(1)
        one_to_one = np.array_equal(np.sort(match), np.arange(n)) and d[np.arange(n), match].max() <= POS_TOL
        assert one_to_one == (not uniform), uniform
