"""Every kernel on clouds and queries with NaN or infinite coordinates ("Non-finite coordinates"; the cases are
in tests/nonfinite_cases.py, what they promise and the reference's part in tests/test_nonfinite_cpu.py).

  1  Indexed clouds.  A row with a NaN or an infinite coordinate is never indexed: size, box, permutation and every *_self form are
     those of the finite rows, against brute force over them -- and, bit for bit, those of the `twin` cloud, whose bad rows lie at
     finite places outside an explicit voxel grid (the dropped-row contract that was there before).
  2  Queries, radii and boxes follow IEEE comparisons, exactly as the oracle's brute force: a NaN query has count 0, an infinite one
     min(k, size) neighbours at d2 = +inf, and the finite queries of the same batch are brute force's.
  3  The kd index drops nothing: oracle.kd_knn_bruteforce and oracle.kd_range_aabb are the definition.
  4  Surface nets and the distance field: the numpy models (and the reference's recorded meshes).

No tolerance is new here: the comparisons are those of the operations' own test files.  Every case prints what it is about to run,
flushed, before it launches anything."""
import os

import numpy as np
import pytest

import handle_history_cases as Cs
import nonfinite_cases as N
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
F = np.float32
NONE = N.NONE
SENT = 7  # what a caller's device arrays hold before a call (handle_history_cases.FILL)
KS = (1, 15, 33)
EPSES = (0.0, 1e-5)
SELF_CLOUDS = [(kind, n) for kind in N.KINDS for n in N.SIZES] + [(kind, 1300) for kind in N.SURVIVORS] + [("one_finite", 65)]
EMPTY_CLOUDS = [("none_finite", 70), ("inf_axis", 1300)]


def _say(*what):
    print(*what, flush=True)


def _ids(cases):
    return ["%s_%d" % c for c in cases]


def _bits(a):
    return Cs.bits(a)


def _torch():
    return pytest.importorskip("torch")


def _up(a):
    t = _torch()
    a = np.ascontiguousarray(a)
    d = t.from_numpy(a.copy() if a.size else np.zeros(1, a.dtype)).to(t.device("cuda", 0))
    t.cuda.synchronize()
    return d


def _out(length, kind):
    t = _torch()
    dtype = {"u32": t.int32, "u64": t.int64, "f32": t.float32}[kind]
    d = t.full((max(int(length), 1),), SENT, dtype=dtype, device=t.device("cuda", 0))
    t.cuda.synchronize()
    return d


def _down(d, length, width=1):
    a = d.cpu().numpy()
    a = a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))[:int(length)]
    return a.reshape(-1, width) if width > 1 else a


_made = {}


def _index(pkg, kind, n):
    """the module's handle on a cloud, and its twin's"""
    if (kind, n) not in _made:
        pts, finite = N.cloud(kind, n)
        ix = pkg.LinkedOctree(pts)
        tw = None
        if finite.any():
            tpts, grid = N.twin(pts, finite)
            tw = pkg.LinkedOctree(tpts, voxel_grid=grid)
        _made[(kind, n)] = (ix, tw)
    return _made[(kind, n)]


def _base_index(pkg):
    if "base" not in _made:
        _made["base"] = pkg.LinkedOctree(N.base(1300))
    return _made["base"]


def _perm(ix, n_in):
    n = ix.size()
    perm, pos = _out(n, "u32"), _out(n_in, "u32")
    ix.perm_dev(perm.data_ptr(), pos.data_ptr())
    ix.synchronize()
    return _down(perm, n), _down(pos, n_in)


# ---- 1. build -------------------------------------------------------------------------------------------------------------------------
def _container(ix, pts, finite, what):
    n_in, rows = len(pts), np.nonzero(finite)[0]
    assert ix.size() == len(rows) and ix.empty() == (len(rows) == 0), what
    box = ix.bbox()
    assert np.isfinite(box).all() and np.array_equal(_bits(box), _bits(N.finite_box(pts, finite))), (what, box)
    perm, pos = _perm(ix, n_in)
    assert np.array_equal(np.sort(perm), rows), what
    assert (pos[~finite] == NONE).all() and np.array_equal(pos[perm.astype(np.int64)], np.arange(len(rows))), what
    return perm


@pytest.mark.parametrize("kind,n", N.all_clouds(), ids=_ids(N.all_clouds()))
def test_build_indexes_the_finite_rows_only(pkg, kind, n):
    t = _torch()
    _say("build", kind, n)
    pts, finite = N.cloud(kind, n)
    ix = pkg.LinkedOctree(pts)
    perm = _container(ix, pts, finite, (kind, n, "host"))
    _say("build", kind, n, "from device memory")
    d_pts = _up(pts)
    dev = pkg.Index.from_device(d_pts.data_ptr(), n, stream=t.cuda.current_stream().cuda_stream)
    assert np.array_equal(_container(dev, pts, finite, (kind, n, "device")), perm)
    if finite.any():  # the twin's order of the finite rows is the same order: the grid comes from the same box
        tpts, grid = N.twin(pts, finite)
        tw = pkg.LinkedOctree(tpts, voxel_grid=grid)
        assert tw.size() == ix.size() and np.array_equal(_perm(tw, n)[0], perm)
        tw.close()
    dev.close()
    ix.close()


def test_bounding_box_keeps_the_reference_rule(pkg):
    """pcpx_bounding_box restates pcp::bounding_box: strict comparisons from +-FLT_MAX, so a NaN is skipped and an infinity taken"""
    _say("bounding_box mixed")
    pts, _finite = N.cloud("mixed", 1300)
    lo = np.where(np.isnan(pts), F(np.inf), pts).min(0)
    hi = np.where(np.isnan(pts), F(-np.inf), pts).max(0)
    got = pkg.bounding_box(pts)
    assert np.array_equal(got, np.concatenate([lo, hi])) and np.isinf(got).any()


def test_rebuild_finite_mixed_finite_on_one_handle(pkg, oracle):
    import test_gpu_parity as TP
    base = N.base(1300)
    mixed, finite = N.cloud("mixed", 1300)
    for form in ("host", "device"):
        _say("rebuild", form)
        ix = pkg.LinkedOctree(base)
        d_base, d_mixed = _up(base), _up(mixed)
        for step, (pts, d_pts, ok) in enumerate(((mixed, d_mixed, finite), (base, d_base, np.ones(1300, bool)), (mixed, d_mixed, finite))):
            _say("rebuild", form, "step", step)
            if form == "host":
                ix.rebuild(pts)
            else:
                ix.rebuild_dev(d_pts.data_ptr(), 1300)
                ix.synchronize()
            _container(ix, pts, ok, (form, step))
            assert 1300 - ix.size() == int((~ok).sum())  # (the outside count)
            gi, gc, gd = ix.knn_self(15, 1e-5, want_d2=True)
            rows = np.nonzero(ok)[0]
            oi, oc, od = N.knn_over_finite(oracle, pts, ok, pts[rows], 15, 1e-5)
            TP._assert_rows_exact(pts, pts[rows], 15, gi[rows], gc[rows], gd[rows], oi, oc, od)
            assert (gc[~ok] == 0).all() and (gi[~ok] == NONE).all()
        ix.close()


@pytest.mark.parametrize("kind,n", EMPTY_CLOUDS, ids=_ids(EMPTY_CLOUDS))
def test_a_cloud_with_no_finite_row_behaves_as_an_empty_one(pkg, kind, n):
    """tests/test_gpu_parity.py::test_knn_empty_and_k0 on it, and the self forms' empty rows"""
    _say("no finite row", kind)
    pts, finite = N.cloud(kind, n)
    ix = pkg.Index(pts)
    assert ix.size() == 0 and ix.empty()
    for q in ([[0, 0, 0], [1, 1, 1]], N.queries("many")):
        for k in (4, 33):
            idx, cnt, d2 = ix.knn(q, k, want_d2=True)
            assert np.all(cnt == 0) and np.all(idx == NONE) and np.isposinf(d2).all()
    idx, cnt = ix.knn_self(15)
    assert (cnt == 0).all() and (idx == NONE).all()
    assert (ix.range_count_self(0.5) == 0).all() and (ix.range_count(N.base(70), np.inf) == 0).all()
    off, lst = ix.range_sphere(N.base(70)[:5], 10.0)
    assert not off.any() and len(lst) == 0
    off, lst = ix.range_aabb(np.array([[-np.inf] * 3 + [np.inf] * 3], F))
    assert not off.any() and len(lst) == 0
    ix.rebuild(N.base(70))  # (and back)
    assert ix.size() == 70
    ix.close()


def test_a_non_finite_voxel_grid_is_refused_in_every_form(pkg):
    _say("grid refusal")
    base = N.base(70)
    d_base = _up(base)
    ix = pkg.LinkedOctree(base)
    for bad in ([0, 0, 0, 1, np.inf, 1], [-np.inf, 0, 0, 1, 1, 1], [0, 0, np.nan, 1, 1, 1], [0, 0, 0, 1, 1, np.nan]):
        grid = np.array(bad, F)
        with pytest.raises(pkg.PcpxError):
            pkg.LinkedOctree(base, voxel_grid=grid)
        with pytest.raises(pkg.PcpxError):
            pkg.Index.from_device(d_base.data_ptr(), 70, voxel_grid=grid)
        with pytest.raises(pkg.PcpxError):
            ix.rebuild(base, voxel_grid=grid)
        with pytest.raises(pkg.PcpxError):
            ix.rebuild_dev(d_base.data_ptr(), 70, voxel_grid=grid)
        assert ix.size() == 70  # (a refused rebuild leaves the handle on its index)
    ix.close()


# ---- 1. self kNN in every form --------------------------------------------------------------------------------------------------------
def _self_rows(pkg, oracle, kind, n, k, eps):
    """(host rows of the handle, brute force over the finite rows): made once per case"""
    key = ("rows", kind, n, k, eps)
    if key not in _made:
        import test_gpu_parity as TP
        pts, finite = N.cloud(kind, n)
        ix, tw = _index(pkg, kind, n)
        rows = np.nonzero(finite)[0]
        gi, gc, gd = ix.knn_self(k, eps, want_d2=True)
        oi, oc, od = N.knn_over_finite(oracle, pts, finite, pts[rows], k, eps)
        TP._assert_rows_exact(pts, pts[rows], k, gi[rows], gc[rows], gd[rows], oi, oc, od)
        assert (gc[~finite] == 0).all() and (gi[~finite] == NONE).all()
        ti, tc, td = tw.knn_self(k, eps, want_d2=True)  # a dropped row is an out-of-grid row, bit for bit
        assert np.array_equal(ti, gi) and np.array_equal(tc, gc) and np.array_equal(_bits(td), _bits(gd))
        _made[key] = (gi, gc, gd)
    return _made[key]


@pytest.mark.parametrize("eps", EPSES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,n", SELF_CLOUDS, ids=_ids(SELF_CLOUDS))
def test_knn_self_host_and_device_forms(pkg, oracle, kind, n, k, eps):
    _say("knn_self", kind, n, k, eps)
    pts, finite = N.cloud(kind, n)
    ix, _tw = _index(pkg, kind, n)
    gi, gc, gd = _self_rows(pkg, oracle, kind, n, k, eps)
    rows, m = np.nonzero(finite)[0], int(finite.sum())
    _say("knn_self_dev", kind, n, k, eps)
    idx, cnt, d2 = _out(n * k, "u32"), _out(n, "u32"), _out(n * k, "f32")
    ix.knn_self_dev(k, eps, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
    ix.synchronize()
    di, dc, dd = _down(idx, n * k, k).reshape(n, k), _down(cnt, n), _down(d2, n * k, k).reshape(n, k)
    assert np.array_equal(di[rows], gi[rows]) and np.array_equal(dc[rows], gc[rows]) and np.array_equal(_bits(dd[rows]), _bits(gd[rows]))
    assert (di[~finite] == SENT).all() and (dc[~finite] == SENT).all() and (dd[~finite] == SENT).all()  # (the caller's bytes)
    if k <= 32:  # (the strided and the curve-order forms are the single-pass kernels')
        stride = k + 1
        _say("knn_self_strided_dev", kind, n, k, eps, stride)
        idx, cnt, d2 = _out(n * stride, "u32"), _out(n, "u32"), _out(n * stride, "f32")
        ix.knn_self_strided_dev(k, eps, stride, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
        ix.synchronize()
        si, sd = _down(idx, n * stride, stride).reshape(n, stride), _down(d2, n * stride, stride).reshape(n, stride)
        assert np.array_equal(si[rows, :k], gi[rows]) and np.array_equal(_bits(sd[rows, :k]), _bits(gd[rows]))
        assert (si[rows, k:] == NONE).all() and np.isposinf(sd[rows, k:]).all() and (si[~finite] == SENT).all()
        _say("knn_self_curve_order_dev", kind, n, k, eps)
        perm = _perm(ix, n)[0].astype(np.int64)
        idx, cnt, d2 = _out(m * k, "u32"), _out(m, "u32"), _out(m * k, "f32")
        ix.knn_self_curve_order_dev(k, eps, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
        ix.synchronize()
        assert np.array_equal(_down(idx, m * k, k).reshape(m, k), gi[perm]) and np.array_equal(_down(cnt, m), gc[perm])
        assert np.array_equal(_bits(_down(d2, m * k, k).reshape(m, k)), _bits(gd[perm]))


@pytest.mark.parametrize("k", (15, 33))
@pytest.mark.parametrize("kind,n", SELF_CLOUDS, ids=_ids(SELF_CLOUDS))
def test_normals_planes_and_mean_distances_of_the_finite_rows(pkg, oracle, kind, n, k):
    import test_gpu_parity as TP
    _say("normals_knn_self", kind, n, k)
    pts, finite = N.cloud(kind, n)
    ix, tw = _index(pkg, kind, n)
    gi, gc, _gd = _self_rows(pkg, oracle, kind, n, k, 1e-5)
    rows = np.nonzero(finite)[0]
    nrm, ni, nc = ix.normals_knn_self(k, want_knn=True)
    assert np.array_equal(ni, gi) and np.array_equal(nc, gc)
    want = oracle.normals_from_knn(pts, gi, gc, nthreads=16)
    if len(rows) > 3:
        assert TP._cos_err(nrm[rows], want[rows]).max() <= TP.COS_TOL
    _say("tangent planes, mean distance", kind, n, k)
    cen, pn = ix.tangent_planes_knn_self(k)
    md = ix.mean_knn_distance_self(k)
    assert np.array_equal(_bits(pn[rows]), _bits(nrm[rows]))
    assert np.array_equal(_bits(cen[rows]), _bits(oracle.centroids_from_knn(pts, gi, gc)[rows]))
    assert np.array_equal(_bits(md[rows]), _bits(oracle.mean_dist_from_knn(pts, pts, gi, gc)[rows]))
    for got, other in ((nrm, tw.normals_knn_self(k)), (cen, tw.tangent_planes_knn_self(k)[0]), (md, tw.mean_knn_distance_self(k))):
        assert np.array_equal(_bits(got), _bits(other))  # (dropped rows: the host forms' empty value, as for a point outside the grid)
    _say("neighbourhoods_self_dev", kind, n, k)
    dn, dc, dm = _out(n * 3, "f32"), _out(n * 3, "f32"), _out(n, "f32")
    ix.neighbourhoods_self_dev(k, 1e-5, dn.data_ptr(), dc.data_ptr(), dm.data_ptr())
    ix.synchronize()
    hn, hc, hm = _down(dn, n * 3, 3).reshape(n, 3), _down(dc, n * 3, 3).reshape(n, 3), _down(dm, n)
    assert np.array_equal(_bits(hn[rows]), _bits(nrm[rows])) and np.array_equal(_bits(hc[rows]), _bits(cen[rows]))
    assert np.array_equal(_bits(hm[rows]), _bits(md[rows]))
    assert (hn[~finite] == SENT).all() and (hc[~finite] == SENT).all() and (hm[~finite] == SENT).all()


# ---- 2. batches of queries ------------------------------------------------------------------------------------------------------------
def _check_batch_rows(oracle, pts, finite, q, k, eps, got, what):
    import test_gpu_parity as TP
    gi, gc, gd = got
    nan, inf = N.kinds_of(q)
    size = int(finite.sum())
    assert (gc[nan] == 0).all() and (gi[nan] == NONE).all() and np.isposinf(gd[nan]).all(), what
    want = min(k, size)
    for r in np.nonzero(inf)[0]:
        ids = gi[r, :want].astype(np.int64)
        assert gc[r] == want and np.isposinf(gd[r]).all() and (gi[r, want:] == NONE).all(), (what, r)
        assert len(set(ids.tolist())) == want and (ids < len(pts)).all() and finite[ids].all(), (what, r)
    rest = ~(nan | inf)
    if rest.any():  # (a bad lane must not disturb its wave)
        oi, oc, od = N.knn_over_finite(oracle, pts, finite, np.ascontiguousarray(q[rest]), k, eps)
        TP._assert_rows_exact(pts, q[rest], k, gi[rest], gc[rest], gd[rest], oi, oc, od)


def _knn_batch_dev(ix, q, k, eps):
    nq = len(q)
    d_q, idx, cnt, d2 = _up(q), _out(nq * k, "u32"), _out(nq, "u32"), _out(nq * k, "f32")
    ix.knn_batch_dev(d_q.data_ptr(), nq, k, eps, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
    ix.synchronize()
    return _down(idx, nq * k, k).reshape(nq, k), _down(cnt, nq), _down(d2, nq * k, k).reshape(nq, k)


@pytest.mark.parametrize("eps", EPSES)
@pytest.mark.parametrize("k", (1, 8, 15, 32, 33))
@pytest.mark.parametrize("name", N.QUERY_SETS)
def test_knn_batch_latency_and_throughput_paths(pkg, oracle, name, k, eps):
    """the host form takes the latency path up to 512 queries and k <= 32, the throughput path beyond; the device form always the
    throughput path (k <= 8, 16, 32 and the multi-pass kernels)"""
    q = N.queries(name)
    for cloud in ("base", "mixed"):
        pts, finite = (N.base(1300), np.ones(1300, bool)) if cloud == "base" else N.cloud("mixed", 1300)
        ix = _base_index(pkg) if cloud == "base" else _index(pkg, "mixed", 1300)[0]
        _say("knn_batch", cloud, name, k, eps, "latency" if len(q) <= 512 and k <= 32 else "throughput")
        _check_batch_rows(oracle, pts, finite, q, k, eps, ix.knn(q, k, eps, want_d2=True), (cloud, name, k, eps, "host"))
        _say("knn_batch_dev", cloud, name, k, eps)
        _check_batch_rows(oracle, pts, finite, q, k, eps, _knn_batch_dev(ix, q, k, eps), (cloud, name, k, eps, "dev"))


@pytest.mark.parametrize("name", N.QUERY_SETS)
def test_kd_knn_batch_with_the_query_sets(pkg, oracle, name):
    q = N.queries(name)
    if "kd3" not in _made:
        _made["kd3"] = pkg.KdTreeK(N.base(1300))
    for k in (1, 15, 70):
        for eps in EPSES:
            _say("kd_knn_batch", name, k, eps)
            idx, cnt, d2 = _made["kd3"].nearest_neighbours(q, k, eps, want_d2=True)
            oi, oc, od = oracle.kd_knn_bruteforce(N.base(1300), q, k, eps)[:3]
            assert np.array_equal(idx, oi) and np.array_equal(cnt, oc) and np.array_equal(_bits(d2), _bits(od)), (name, k, eps)


# ---- ranges ---------------------------------------------------------------------------------------------------------------------------
def _two_clouds(pkg):
    yield "base", N.base(1300), np.ones(1300, bool), _base_index(pkg)
    pts, finite = N.cloud("mixed", 1300)
    yield "mixed", pts, finite, _index(pkg, "mixed", 1300)[0]


@pytest.mark.parametrize("kind,n", SELF_CLOUDS, ids=_ids(SELF_CLOUDS))
def test_range_count_and_lists_self(pkg, oracle, kind, n):
    pts, finite = N.cloud(kind, n)
    ix, tw = _index(pkg, kind, n)
    rows = np.nonzero(finite)[0]
    sub = np.ascontiguousarray(pts[rows])
    for r in (float(N.RADIUS), 0.0, float("inf")):
        _say("range_count_self", kind, n, r)
        want = oracle.range_count_bruteforce(sub, sub, r, nthreads=16)
        got = ix.range_count_self(r)
        assert np.array_equal(got[rows], want) and (got[~finite] == 0).all() and np.array_equal(got, tw.range_count_self(r))
        cnt = _out(n, "u32")
        ix.range_count_self_dev(r, cnt.data_ptr())
        ix.synchronize()
        dev = _down(cnt, n)
        assert np.array_equal(dev[rows], want) and (dev[~finite] == SENT).all()
    _say("range_count_self NaN radius", kind, n)
    assert (ix.range_count_self(float("nan")) == 0).all()
    r = float(N.RADIUS)
    _say("range_lists_self_dev", kind, n, r)
    off = _out(n + 1, "u64")
    total = ix.range_lists_self_dev(r, off.data_ptr())
    idx = _out(total, "u32")
    assert ix.range_lists_self_dev(r, off.data_ptr(), idx.data_ptr(), total) == total
    ix.synchronize()
    lists = N.lists_of(_down(off, n + 1), _down(idx, total))
    want = N.sphere_lists(pts, finite, pts, F(r))
    for i in range(n):
        assert np.array_equal(lists[i], want[i] if finite[i] else np.zeros(0, np.int64)), (kind, n, i)


def test_range_count_batch(pkg, oracle):
    for cloud, pts, finite, ix in _two_clouds(pkg):
        for name in ("many", "all_bad", "one_nan", "one_inf"):
            q = N.queries(name)
            for r in (float(N.RADIUS), 0.0, -1.0, float("inf"), float("nan")):
                _say("range_count_batch", cloud, name, r)
                want = np.array([len(l) for l in N.sphere_lists(pts, finite, q, F(r))], np.uint32)
                assert np.array_equal(ix.range_count(q, r), want), (cloud, name, r)
                if r >= 0:  # (the oracle says the same)
                    assert np.array_equal(want, oracle.range_count_bruteforce(np.ascontiguousarray(pts[finite]), q, r, nthreads=16))


def test_range_sphere_batch_and_single(pkg):
    centres, radii = N.spheres()
    for cloud, pts, finite, ix in _two_clouds(pkg):
        _say("range_sphere_batch per-sphere radii", cloud)
        want = N.sphere_lists(pts, finite, centres, radii)
        got = N.lists_of(*ix.range_sphere(centres, radii))
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), cloud
        assert sum(len(w) == int(finite.sum()) for w in want) >= 8 and sum(0 < len(w) < 50 for w in want) >= 8
        for r in (float(N.RADIUS), float("inf"), float("nan")):
            _say("range_sphere_batch one radius", cloud, r)
            want = N.sphere_lists(pts, finite, centres, F(r))
            got = N.lists_of(*ix.range_sphere(centres, r))
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (cloud, r)
        for i in range(0, 96, 4):  # one sphere per call: the latency form (an infinite radius holds the whole cloud: within its stage)
            _say("range_sphere single", cloud, i, centres[i], radii[i])
            off, idx = ix.range_sphere(centres[i:i + 1], radii[i:i + 1])
            assert np.array_equal(np.sort(idx), N.sphere_lists(pts, finite, centres[i:i + 1], radii[i:i + 1])[0]) and off[1] == len(idx), (cloud, i)


def test_range_aabb_batch_and_single(pkg):
    boxes = N.boxes()
    for cloud, pts, finite, ix in _two_clouds(pkg):
        _say("range_aabb_batch", cloud)
        want = N.box_lists(pts, finite, boxes)
        got = N.lists_of(*ix.range_aabb(boxes))
        assert len(got) == 48 and all(np.array_equal(g, w) for g, w in zip(got, want)), cloud
        assert sum(len(w) == int(finite.sum()) for w in want) == 8
        for i in range(0, 48, 1):
            _say("range_aabb single", cloud, i)
            off, idx = ix.range_aabb(boxes[i:i + 1])
            assert np.array_equal(np.sort(idx), want[i]) and off[1] == len(idx), (cloud, i)


# ---- 3. the kd index ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", (3, 16, 33))
@pytest.mark.parametrize("kind", ("nan_rows", "inf_rows", "odd_nans"))
def test_kd_index_holds_every_row(pkg, oracle, kind, dims):
    """dims 16 is the most a kd index holds (PCPX_KD_MAX_DIMS, include/pcpx.h): 33 coordinates are refused, non-finite or not"""
    pts, q, boxes = N.kd_case(kind, dims)
    _say("kd create", kind, dims)
    if dims > 16:
        with pytest.raises(pkg.PcpxError):
            pkg.KdTreeK(pts)
        return
    tree = pkg.KdTreeK(pts)
    assert tree.size() == 700
    for k in (1, 15, 70):
        for eps in EPSES:
            _say("kd_knn_batch", kind, dims, k, eps)
            idx, cnt, d2 = tree.nearest_neighbours(q, k, eps, want_d2=True)
            oi, oc, od = oracle.kd_knn_bruteforce(pts, q, k, eps)[:3]
            assert np.array_equal(idx, oi) and np.array_equal(cnt, oc) and np.array_equal(_bits(d2), _bits(od)), (kind, dims, k, eps)
    _say("kd_range_aabb_batch", kind, dims)
    got = N.lists_of(*tree.range_search(boxes))
    want = oracle.kd_range_aabb(pts, boxes)
    assert len(got) == len(want) and all(np.array_equal(g, np.sort(w)) for g, w in zip(got, want))
    assert len(want[1]) == 0 and len(want[2]) > 600  # (a NaN bound selects nothing; (-inf, +inf) every row without a NaN)
    tree.close()


# ---- sphere-walk families on `mixed`: each family's own model with inside = finite, and the twin bit for bit ----------------------------
class _Ctx(Cs.Ctx):
    def __init__(self, pkg, ix, I):
        self.pkg, self.ix, self.cloud, self.I = pkg, ix, "mixed", I
        self.n_in, self.n, self.r = len(I["points"]), int(I["inside"].sum()), float(I["radius"][0])


def _mixed_inputs(twin):
    key = ("inputs", twin)
    if key not in _made:
        pts, finite = N.cloud("mixed", 1300)
        I = dict(Cs.inputs("c1300"))
        I["points"], I["inside"] = (N.twin(pts, finite)[0] if twin else pts), finite
        _made[key] = I
    return _made[key]


def _family(pkg, row):
    """(the row's outputs on the mixed cloud, the inputs): checked equal to its twin's, bit for bit"""
    key = ("family", row)
    if key not in _made:
        ix, tw = _index(pkg, "mixed", 1300)
        _say("family", row, "mixed")
        out = {k: np.ascontiguousarray(v) for k, v in Cs.ROWS[row][1](_Ctx(pkg, ix, _mixed_inputs(False))).items()}
        _say("family", row, "twin")
        other = {k: np.ascontiguousarray(v) for k, v in Cs.ROWS[row][1](_Ctx(pkg, tw, _mixed_inputs(True))).items()}
        Cs.same_bits(out, other, (row, "mixed against its twin"))
        _made[key] = out
    return _made[key], _mixed_inputs(False)


def _edges():
    if "edges" not in _made:
        import cluster_model as CM
        I = _mixed_inputs(False)
        sub = np.ascontiguousarray(I["points"][I["inside"]])
        _made["edges"] = (sub, np.nonzero(I["inside"])[0], CM.brute_edges(sub, float(I["radius"][0])))
    return _made["edges"]


def test_family_range_neighbourhoods(pkg, oracle):
    import shape_features_cases as S
    import test_gpu_range_neighbourhoods as TRn
    for row, batch in (("moments_self", False), ("moments_batch", True)):
        out, I = _family(pkg, row)
        pts, inside, r = I["points"], I["inside"], float(I["radius"][0])
        sub, rows, _ = _edges()
        if batch:
            centres, take = I["queries"], np.arange(len(I["queries"]))
            sets = [rows[S.brute_set(sub, c, rr)] for c, rr in zip(centres, I["radii"])]
        else:
            take = np.nonzero(inside)[0][::17]
            centres, sets = pts[take], [rows[S.brute_set(sub, pts[i], r)] for i in take]
            assert (out["counts"][~inside] == 0).all() and np.isnan(out["centroids"][~inside]).all() and np.isnan(out["mean_dist"][~inside]).all()
        extent = float(np.ptp(sub, 0).max())
        TRn._check_rows(oracle, pts, centres, None, sets, out["normals"][take], out["centroids"][take], out["mean_dist"][take], out["counts"][take],
                        extent, row)


def test_family_shape_features(pkg):
    import shape_features_cases as S
    import test_gpu_shape_features as TSf
    out, I = _family(pkg, "features_self")
    pts, inside, r = I["points"], I["inside"], float(I["radius"][0])
    sub, rows, _ = _edges()
    take = np.nonzero(inside)[0][::17]
    sets = [rows[S.brute_set(sub, pts[i], r)] for i in take]
    TSf._check_rows(pts, pts[take], sets, out["evals"][take], out["curvature"][take], out["axes"][take], out["counts"][take], "features mixed", True)
    assert (out["counts"][~inside] == 0).all() and np.isnan(out["curvature"][~inside]).all()


def test_family_cluster(pkg):
    import cluster_model as CM
    for row, min_pts, compact in (("cluster_m1_compact", 1, True), ("cluster_m5_plain_dev", 5, False)):
        out, I = _family(pkg, row)
        inside = I["inside"]
        _sub, rows, (src, dst, cnt) = _edges()
        n = len(inside)
        want, wcore, wn = CM.cluster(len(cnt), src, dst, cnt, min_pts, compact=compact, symmetric=True)
        if not compact:
            live = want != NONE
            want = want.copy()
            want[live] = rows[want[live]]
        if row.endswith("_dev"):  # (the _dev form leaves the caller's bytes at a dropped row)
            full, fcore, fcnt = np.full(n, SENT, np.uint32), np.full(n, SENT, np.uint8), np.full(n, SENT, np.uint32)
        else:
            full, fcore, fcnt = np.full(n, NONE, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        full[rows], fcore[rows], fcnt[rows] = want, wcore, cnt
        assert np.array_equal(out["counts"][rows], fcnt[rows]) and np.array_equal(out["core"][rows], fcore[rows]) and int(out["count"][0]) == wn
        assert np.array_equal(out["labels"][rows], full[rows]) and wn > 1
        if not row.endswith("_dev"):
            assert np.array_equal(out["labels"], full) and np.array_equal(out["counts"], fcnt) and np.array_equal(out["core"], fcore)


def test_family_segment(pkg):
    import segment_model as GM
    out, I = _family(pkg, "segment")
    _sub, _rows, edges = _edges()
    want, wsmooth, wn = GM.segment_cloud(I["points"], I["normals"], float(I["radius"][0]), 0.5, curvature=None, inside=I["inside"], edges=edges,
                                         max_curvature=0.5, min_size=3, oriented=False, compact=True)
    assert np.array_equal(out["smooth"].astype(bool), wsmooth) and int(out["count"][0]) == wn and np.array_equal(out["labels"], want) and wn > 1


def test_family_subsample(pkg):
    import subsample_model as UM
    out, I = _family(pkg, "subsample")
    sub, rows, (src, dst, _cnt) = _edges()
    n = len(I["inside"])
    want_sub, _rounds = UM.rounds_form(len(rows), src, dst, Cs.SUBSAMPLE_SEED, ids=rows)
    own_sub = UM.owners(len(rows), src, dst, UM.pair_d2(sub, src, dst), want_sub)
    want, wown = np.zeros(n, bool), np.full(n, NONE, np.uint32)
    want[rows], wown[rows] = want_sub, rows[own_sub].astype(np.uint32)
    keep = out["keep"].astype(bool)
    assert np.array_equal(keep, want) and np.array_equal(out["kept"], np.nonzero(keep)[0]) and np.array_equal(out["owner"], wown)
    assert 0 < keep.sum() < len(rows)


def test_family_local_maxima(pkg):
    import keypoints_model as KM
    out, I = _family(pkg, "local_maxima")
    _sub, _rows, edges = _edges()
    want = KM.local_maxima_cloud(I["points"], I["score"], float(I["radius"][0]), 0.25, 2, inside=I["inside"], edges=edges)
    assert np.array_equal(out["keep"].astype(bool), want) and np.array_equal(out["kept"], np.nonzero(want)[0]) and 0 < want.sum()


def test_family_fpfh(pkg):
    import fpfh_model as PM
    import test_gpu_fpfh as TFp
    out, I = _family(pkg, "fpfh_all")
    pts, inside, nrm, r = I["points"], I["inside"], I["normals"], float(I["radius"][0])
    rows = np.nonzero(inside)[0][::9]
    want_spfh, want_pairs = PM.spfh(pts, nrm, rows, r, inside)
    assert np.array_equal(out["pairs"][rows], want_pairs) and np.array_equal(_bits(out["spfh"][rows]), _bits(want_spfh))
    assert not out["spfh"][~inside].any() and not out["pairs"][~inside].any()
    TFp._check_fpfh_rows(pts, inside, r, rows, out["fpfh"][rows], out["spfh"], "fpfh mixed")


def test_family_nearest_posed(pkg):
    import icp_model as IM
    out, I = _family(pkg, "nearest_posed")
    want, want_d2 = IM.nearest_posed(I["points"], I["source"], Cs.POSE, 2.0 * float(I["radius"][0]), indexed=I["inside"])
    assert np.array_equal(out["partner"], want) and np.array_equal(_bits(out["d2"]), _bits(want_d2)) and (want != IM.NONE).sum() > 10
    _say("nearest_posed with a non-finite source")
    src = I["source"].copy()
    src[::9] = N.queries("all_bad")[:len(src[::9])]
    ix = _index(pkg, "mixed", 1300)[0]
    partner, d2 = ix.nearest_posed(src, 2.0 * float(I["radius"][0]), Cs.POSE, want_d2=True)
    want, want_d2 = IM.nearest_posed(I["points"], src, Cs.POSE, 2.0 * float(I["radius"][0]), indexed=I["inside"])
    assert np.array_equal(partner, want) and np.array_equal(_bits(d2), _bits(want_d2)) and (partner[::9] == IM.NONE).all()


# ---- filters --------------------------------------------------------------------------------------------------------------------------
def _filter_cloud():
    """tests/test_gpu_filters.py's surface cloud with 30 rows made non-finite (NaN, +inf, -inf, one all NaN)"""
    import test_gpu_filters as TFi
    pts, nrm = TFi._surface_cloud(3000, 7)
    bad = pts.copy()
    rows = np.random.default_rng(31).permutation(3000)[:30]
    bad[rows, np.arange(30) % 3] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(30) % 3]
    bad[rows[0]] = np.nan
    return bad, nrm, np.isfinite(bad).all(1)


@pytest.mark.parametrize("normals_mode", (False, True), ids=("points", "normals"))
def test_bilateral_filters_leave_non_finite_rows_nan(pkg, oracle, normals_mode):
    import test_gpu_filters as TFi
    _say("bilateral", normals_mode)
    bad, nrm, finite = _filter_cloud()
    keep = np.nonzero(finite)[0]
    sigmaf, sigmag = 0.08, 0.02
    if not normals_mode:
        got = pkg.bilateral_filter_points(bad, nrm, sigmaf, sigmag, K=1)
        exp = oracle.bilateral_filter_points(bad[keep], nrm[keep], sigmaf, sigmag, K=1, nthreads=16)
        assert np.isnan(got[~finite]).all() and np.isfinite(got[keep]).all()
        assert np.abs(got[keep] - exp).max() <= TFi.POS_TOL * TFi._extent(bad[keep])
    else:
        got = pkg.bilateral_filter_normals(bad, nrm, sigmaf, sigmag, K=1)
        exp = oracle.bilateral_filter_normals(bad[keep], nrm[keep], sigmaf, sigmag, K=1, nthreads=16)
        assert np.isnan(got[~finite]).all() and np.isfinite(got[keep]).all()
        assert (1.0 - np.sum(got[keep].astype(np.float64) * exp, axis=1)).max() <= TFi.COS_TOL


def test_wlop_with_non_finite_points_and_a_sample_that_names_one(pkg, oracle):
    import test_gpu_filters as TFi
    _say("wlop")
    pts, sample = TFi._wlop_case(2000, 500, 22)
    bad = pts.copy()
    rows = np.random.default_rng(32).permutation(2000)[:24]
    bad[rows, np.arange(24) % 3] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(24) % 3]
    finite = np.isfinite(bad).all(1)
    sample = sample.copy()
    sample[:3] = rows[:3]  # (sample indices that name dropped points: NaN, +inf and -inf rows)
    named = ~finite[sample.astype(np.int64)]
    assert named.sum() >= 3
    got = pkg.wlop(bad, mu=0.45, h=0.25, k=1, uniform=True, sample=sample)
    keep = np.nonzero(finite)[0]
    renumber = np.full(2000, -1, np.int64)
    renumber[keep] = np.arange(len(keep))
    exp = oracle.wlop(np.ascontiguousarray(bad[keep]), renumber[sample[~named].astype(np.int64)].astype(np.uint64), 0.45, 0.25, 1, uniform=True, nthreads=16)
    assert got.shape == (500, 3) and np.isnan(got[named]).all() and np.isfinite(got[~named]).all()
    assert np.abs(got[~named] - exp).max() <= TFi.POS_TOL


# ---- orientation ----------------------------------------------------------------------------------------------------------------------
def test_orientation_with_nan_points_and_nan_normals(pkg, oracle):
    """tests/test_gpu_parity.py::test_device_orientation_equals_the_sequential_search: the host form and the device form against
    oracle.propagate_normal_orientations over the same rows, bit for bit (a NaN normal never flips and flips nothing)"""
    t = _torch()
    for kind, rooted in (("nan_rows", False), ("nan_rows", True), ("mixed", True)):
        # (row 0 of the clouds is not finite: as they are, the search ends at its root, whose row is empty -- when z[0] is NaN every
        #  comparison of the reference's root search is false.  `rooted`: a finite row first and no dropped row above z = 0.9, so
        #  that the root, the first point of largest z, is an indexed point)
        pts, finite = N.cloud(kind, 1300)
        shift = int(rooted)
        if rooted:
            pts = pts.copy()
            j = int(np.nonzero(finite)[0][0])
            pts[[0, j]] = pts[[j, 0]]
            bad = ~np.isfinite(pts).all(1)
            pts[bad, 2] = np.where(pts[bad, 2] > F(0.9), F(0.9), pts[bad, 2])
            finite = np.isfinite(pts).all(1)
            assert (~finite).sum() > 20 and pts[finite, 2].max() > 0.9
        ix = pkg.Index(pts)
        k = 8
        nrm, idx, cnt = ix.normals_knn_self(k, want_knn=True)
        nrm = nrm.copy()
        nrm[np.nonzero(finite)[0][::50]] = np.nan  # (NaN normals at finite points; the dropped rows' normals are zero)
        _say("propagate_normal_orientations", kind)
        host, reached = pkg.propagate_normal_orientations(pts, idx, nrm, cnt)
        ref, ref_reached = oracle.propagate_normal_orientations(pts, idx, cnt, nrm)
        assert reached == ref_reached and np.array_equal(_bits(host), _bits(ref)) and (reached > 1000 if shift else reached >= 1)
        _say("propagate_normal_orientations_dev", kind)
        d_pts, d_idx, d_cnt, d_nrm = _up(pts), _up(idx.view(np.int32)), _up(cnt.view(np.int32)), _up(nrm)
        dev_reached, _levels = pkg.propagate_normal_orientations_dev(d_pts.data_ptr(), 1300, d_idx.data_ptr(), d_cnt.data_ptr(), k, d_nrm.data_ptr())
        t.cuda.synchronize()
        assert dev_reached == reached and np.array_equal(_bits(d_nrm.cpu().numpy()), _bits(host))
        _say("oriented_normals_knn_self refuses dropped rows", kind)
        with pytest.raises(pkg.PcpxError):  # (as for points outside a voxel grid: a row without a neighbourhood)
            ix.oriented_normals_knn_self(k)
        ix.close()


# ---- 4. surface nets and the distance field ---------------------------------------------------------------------------------------------
def _same_vertices(a, b):
    """bit for bit where they are numbers, NaN for NaN where they are not (the sign of a NaN that arithmetic makes is the hardware's)"""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


@pytest.fixture(scope="module")
def recording():
    return np.load(os.path.join(GOLDEN, "ref_nonfinite.npz"))


@pytest.mark.parametrize("name", N.FIELDS)
def test_surface_nets_on_non_finite_fields(pkg, recording, name):
    import surface_nets_hint_model as HM
    import surface_nets_model as M
    import test_gpu_surface as TS
    g, f = N.field(name)
    _say("surface_nets", name)
    wv, wt = M.surface_nets(f, g, 0.0)
    v, t = pkg.surface_nets(f, TS._grid(pkg, g), 0.0)
    assert _same_vertices(v, wv) and np.array_equal(t, wt), name
    rv, rt = recording[name + "_v"], recording[name + "_t"]
    assert _same_vertices(v, rv) and np.array_equal(t, rt[np.argsort(rt[:, 0], kind="stable")] if len(rt) else rt), name
    _say("surface_nets_from_hint", name)
    hint = np.array([0.0, 0.0, 0.7], F)  # (on the sphere)
    mv, mt, mc, mseed = HM.surface_nets_hint(f, g, hint, 0.0, 32768)
    hv, ht, seed = pkg.surface_nets_from_hint(f, TS._grid(pkg, g), hint, with_seed=True)
    assert seed == mseed, (name, seed, mseed)
    if mseed is None:
        assert _same_vertices(hv, mv) and np.array_equal(ht, mt)
    else:
        cv, cc, ct = HM.canonical(mv, mt, mc)
        assert _same_vertices(hv, cv) and ht.shape == ct.shape and np.array_equal(cc[ht.astype(np.int64)], ct)


def test_tangent_plane_field_with_nan_normals(pkg, oracle):
    """tests/test_gpu_surface.py::test_tangent_plane_field_against_brute_force with NaN normals on some planes: a corner whose nearest
    plane has one is NaN, on both sides"""
    import surface_nets_model as M
    import test_gpu_surface as TS
    _say("tangent_plane_sdf")
    pts = N.base(1300)
    ix = _base_index(pkg)
    cen, nrm = ix.tangent_planes_knn_self(10)
    nrm = nrm.copy()
    nrm[::13] = np.nan
    bb = ix.bbox()
    g = M.regular_grid_containing(bb[:3], bb[3:], (12, 12, 12))
    got = ix.tangent_plane_sdf(cen, nrm, TS._grid(pkg, g)).ravel()
    c = M.corner_positions(g)
    kk = 8
    idx, cnt, d2 = oracle.knn_bruteforce(pts, c, kk, eps=1e-5, nthreads=16, want_d2=True)
    assert np.all(cnt > 0)
    with np.errstate(invalid="ignore"):
        cand = np.stack([TS._plane_values(c, cen, nrm, idx[:, q]) for q in range(kk)], axis=1)
    tied = d2 == d2[:, :1]
    same = (_bits(cand) == _bits(got)[:, None]) | (np.isnan(cand) & np.isnan(got)[:, None])  # ("both NaN" counts as equal)
    assert np.all((same & tied).any(1) | tied.all(1)) and np.isnan(got).sum() > 50 and np.isfinite(got).sum() > 1000


def test_reconstruct_surface_refuses_a_cloud_with_dropped_rows(pkg, bunny):
    """The one-call pipeline asks a neighbourhood of every input row: with 20 rows made non-finite it is refused, as it is for
    points outside a voxel grid; on the finite rows alone it equals the host pipeline
    (tests/test_gpu_surface.py::test_reconstruct_surface_matches_host_pipeline)."""
    import surface_nets_model as M
    import test_gpu_surface as TS
    bad = bunny.copy()
    rows = np.random.default_rng(33).permutation(len(bunny))[:20]
    bad[rows, np.arange(20) % 3] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(20) % 3]
    finite = np.isfinite(bad).all(1)
    _say("reconstruct_surface with 20 non-finite rows")
    ix = pkg.Index(bad)
    assert ix.size() == len(bunny) - 20
    with pytest.raises(pkg.PcpxError):
        ix.reconstruct_surface(10, (20, 20, 20))
    ix.close()
    _say("reconstruct_surface on the finite rows")
    kept = np.ascontiguousarray(bad[finite])
    ix = pkg.Index(kept)
    v, t, cen_d, nrm_d, grid = ix.reconstruct_surface(10, (20, 20, 20), want_planes=True)
    cen, nrm = ix.tangent_planes_knn_self(10)
    idx, cnt = ix.knn_self(10)
    nrm_o, _ = pkg.propagate_normal_orientations(kept, idx, nrm, cnt)
    assert np.array_equal(cen_d, cen) and np.array_equal(nrm_d, nrm_o)
    bb = ix.bbox()
    g = M.regular_grid_containing(bb[:3], bb[3:], (20, 20, 20))
    TS._same_mesh((v, t), M.surface_nets(ix.tangent_plane_sdf(cen, nrm_o, grid), g))
    assert len(t) > 100
    ix.close()


def test_close_the_module_handles():
    for key, value in list(_made.items()):
        if key == "base" or key == "kd3":
            value.close()
        elif isinstance(key, tuple) and len(key) == 2 and isinstance(value, tuple):
            for h in value:
                if h is not None and hasattr(h, "close"):
                    h.close()
        del _made[key]
