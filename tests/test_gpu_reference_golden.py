"""The kernels against outputs recorded from a real build of the reference (tests/golden/ref_*.npz, written by
tests/golden/make_reference_golden.py): kNN (self rows, the latency path <= 512 queries, the batch path), spheres with a scalar
radius and one radius per sphere, boxes, mean neighbour distance, the K-dimensional kd-tree, both surface-nets entry points and
WLOP.  Same rules as tests/test_reference_build.py: ties only at equal distance, radius > 1 as DESIGN.md 'Semantics' states it,
WLOP within the filters' tolerances."""
import os

import numpy as np
import pytest

import surface_nets_hint_model as H
from conftest import GOLDEN, knn_rows_equivalent

pytestmark = pytest.mark.gpu
F = np.float32
POS_TOL = 4e-6        # tests/test_gpu_filters.py
FLIP_FRACTION = 2e-3


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _points(z):
    return (z["points_q"].astype(F) * F(z["scale"])).astype(F)


def _lists(off, idx):
    return [np.sort(idx[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


# ---- kNN and mean distance ---------------------------------------------------------------------------------------------------
def test_knn_self_rows(pkg):
    z = _load("ref_knn.npz")
    pts = _points(z)
    idx, cnt = pkg.LinkedOctree(pts).knn_self(15)
    rows = z["self_rows"].astype(np.int64)
    ok, why = knn_rows_equivalent(pts, pts[rows], idx[rows], cnt[rows], z["self_idx"], z["self_cnt"])
    assert ok, why


FEW_QUERIES_MAX = 512  # csrc/pcpx_api.hip: pcpx_knn_batch takes the latency path (k_knn_few) iff nq <= this and k <= 32


@pytest.mark.parametrize("form,key,k,eps", [("latency", "lat32", 32, 1e-5), ("latency", "lat15", 15, 0.0),
                                            ("batch", "lat33", 33, 1e-5), ("batch", "batch", 16, 0.0)],
                         ids=["latency_k32", "latency_k15", "batch_k33", "batch_k16"])
def test_knn_queries(pkg, form, key, k, eps):
    """300 queries with k = 32 and 15 (the latency path), the same with k = 33 and 1 500 with k = 16 (the batch path)."""
    z = _load("ref_knn.npz")
    pts = _points(z)
    q = z["batch_queries"] if key == "batch" else z["lat_queries"]
    assert (len(q) <= FEW_QUERIES_MAX and k <= 32) == (form == "latency")
    assert z[key + "_idx"].shape == (len(q), k)
    idx, cnt = pkg.LinkedOctree(pts).knn(q, k, eps)
    ok, why = knn_rows_equivalent(pts, q, idx, cnt, z[key + "_idx"], z[key + "_cnt"])
    assert ok, why


def test_mean_knn_distance_self(pkg):
    z = _load("ref_knn.npz")
    got = pkg.LinkedOctree(_points(z)).mean_knn_distance_self(15)
    assert np.array_equal(got.view(np.uint32), z["mean15"].view(np.uint32))


# ---- ranges ------------------------------------------------------------------------------------------------------------------
def _brute(pts, c, r):
    d = pts - c[None, :]
    return np.nonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= F(r) * F(r))[0].astype(np.uint32)


def test_range_sphere_per_sphere_radius(pkg):
    """One radius per sphere, mixing 0, 1e-6, ordinary and > 1 inside every group of 64, over 20 000 points.  r <= 1: the
    reference's sets.  r > 1: the reference's set within the GPU's, the GPU's the geometric answer (brute force)."""
    z = _load("ref_range.npz")
    pts = _points(z)
    c, r = z["centres"], z["radii"]
    assert len(pts) >= 20000
    # co-located blocks of four (radius 0, 1e-6, ordinary, > 1): the kernel's groups of 64, formed after the queries are
    # reordered by their curve key, hold whole blocks, so every group mixes all four kinds
    assert np.array_equal(c[0::4], c[1::4]) and np.array_equal(c[0::4], c[2::4]) and np.array_equal(c[0::4], c[3::4])
    assert (r[0::4] == 0).all() and (r[1::4] == F(1e-6)).all() and (r[2::4] <= 1).all() and (r[2::4] > 0.1).all()
    assert (r[3::4] > 1).all() and len(np.unique(c, axis=0)) == len(c) // 4
    off, idx = pkg.LinkedOctree(pts).range_sphere(c, r)
    got = _lists(off, idx)
    want = _lists(z["per_off"], z["per_idx"])
    above = 0
    for i in range(len(c)):
        if r[i] <= 1:
            assert np.array_equal(got[i], want[i]), (i, r[i])
        else:
            assert np.isin(want[i], got[i]).all(), i
            assert np.array_equal(got[i], _brute(pts, c[i], r[i])), i
            above += len(got[i]) > len(want[i])
    assert above > 0  # the documented difference occurs in this fixture


def test_range_sphere_scalar_radius(pkg):
    z = _load("ref_range.npz")
    pts = _points(z)
    c = z["centres"][:128]
    off, idx = pkg.LinkedOctree(pts).range_sphere(c, float(z["scalar_radius"]))
    for g, w in zip(_lists(off, idx), _lists(z["scalar_off"], z["scalar_idx"])):
        assert np.array_equal(g, w)


def test_range_aabb(pkg):
    z = _load("ref_range.npz")
    off, idx = pkg.LinkedOctree(_points(z)).range_aabb(z["boxes"])
    for g, w in zip(_lists(off, idx), _lists(z["box_off"], z["box_idx"])):
        assert np.array_equal(g, w)


# ---- K-dimensional kd-tree -----------------------------------------------------------------------------------------------------
def _kd_d2(p, q):
    acc = np.zeros(len(p), F)
    for a in range(p.shape[1]):
        d = p[:, a] - q[a]
        acc = acc + d * d
    return acc


def _kd_forms(pkg, pts):
    """(tree, its box query): KdTreeK (exhaustive, any K); for K = 3 also LinkedKdTree, the tree index behind the 3-d API."""
    t = pkg.KdTreeK(pts)
    forms = [(t, t.range_search)]
    if pts.shape[1] == 3:
        t3 = pkg.LinkedKdTree(pts)
        forms.append((t3, t3.range_aabb))
    return forms


@pytest.mark.parametrize("K", [1, 2, 3, 4, 6, 11, 16])
def test_kd_tree_k(pkg, K):
    z = _load("ref_kd.npz")
    pts = (z["k%d_points_q" % K].astype(F) / F(4)).astype(F)
    q = z["k%d_queries" % K]
    for t, boxes in _kd_forms(pkg, pts):
        _check_kd(z, K, pts, q, t, boxes)


def _check_kd(z, K, pts, q, t, boxes):
    for eps, key in ((0.0, ""), (1e-5, "_eps")):
        idx, cnt = t.nearest_neighbours(q, 16, eps)
        assert np.array_equal(cnt, z["k%d_cnt%s" % (K, key)])
        widx = z["k%d_idx%s" % (K, key)]
        for j in range(len(q)):
            c = int(cnt[j])
            a, b = idx[j, :c].astype(np.int64), widx[j, :c].astype(np.int64)
            assert np.array_equal(a, b) or np.array_equal(_kd_d2(pts[a], q[j]), _kd_d2(pts[b], q[j])), (eps, j)
    off, bi = boxes(z["k%d_boxes" % K])
    for g, w in zip(_lists(off, bi), _lists(z["k%d_box_off" % K], z["k%d_box_idx" % K])):
        assert np.array_equal(g, w)


# ---- surface nets ------------------------------------------------------------------------------------------------------------
SURFACE = _load("ref_surface.npz")
CASES = [str(c) for c in SURFACE["cases"]]


def _case(pkg, name):
    z = SURFACE
    gid = str(z[name + "_field"])
    g6, s3 = z[gid + "_grid"], z[gid + "_dims"]
    grid = pkg.surface.grid3d(*[float(v) for v in g6], *[int(v) for v in s3])
    gd = dict(zip(("x", "y", "z", "dx", "dy", "dz"), g6.tolist()))
    gd.update(zip(("sx", "sy", "sz"), [int(v) for v in s3]))
    hint = z[name + "_hint"]
    return z[gid + "_field"], grid, gd, float(z[name + "_iso"]), (None if np.isnan(hint).any() else hint), z[name + "_v"], z[name + "_t"]


def _by_first_vertex(t):
    return t[np.argsort(t[:, 0], kind="stable")] if len(t) else t


@pytest.mark.parametrize("name", CASES)
def test_surface_nets(pkg, name):
    f, grid, gd, iso, hint, rv, rt = _case(pkg, name)
    if hint is None:
        v, t = pkg.surface_nets(f, grid, iso)
        assert v.shape == rv.shape and t.shape == rt.shape
        assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)), "vertices differ in bits or order"
        assert np.array_equal(t, _by_first_vertex(rt)), "triangles differ"
        return
    # the hint overload: the reference's vertices come in search order; keyed by cube, they are the GPU's
    v, t = pkg.surface_nets_from_hint(f, grid, tuple(float(x) for x in hint), iso)
    wv, _ = pkg.surface_nets(f, grid, iso)
    cubes = H.active_cubes(f, gd, iso)
    at = {bytes(x): c for x, c in zip(wv, cubes)}
    rc = np.array([at[bytes(x)] for x in rv], np.int64)
    cv, cc, ct = H.canonical(rv, rt, rc)
    assert v.shape == cv.shape and t.shape == ct.shape, (v.shape, cv.shape, t.shape, ct.shape)
    assert np.array_equal(v.view(np.uint32), cv.view(np.uint32)), "vertices differ in bits or cubes"
    assert np.array_equal(cc[t.astype(np.int64)], ct), "triangles differ"


# ---- WLOP --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("uniform", [True, False], ids=["wlop", "lop"])
def test_wlop(pkg, iters, uniform):
    z = _load("ref_wlop.npz")
    pts = _points(z)
    got = pkg.wlop(pts, mu=float(z["mu"]), h=float(z["h"]), k=iters, uniform=uniform, sample=z["sample"])
    want = z["out_k%d_u%d" % (iters, int(uniform))]
    ext = float((pts.max(0) - pts.min(0)).max())
    d = np.abs(got - want).max(axis=1)
    if iters == 1:
        assert d.max() <= POS_TOL * ext
    else:
        assert float(np.mean(d > POS_TOL * ext)) <= FLIP_FRACTION and d.max() <= 1e-2
