"""Every kernel on clouds far from the origin and at other scales (tests/far_cloud_cases.py): millimetre CAD extents (r > 1),
a 10^-3 cloud whose neighbours sit inside the default eps box, |q| ~ 10^3, a georeferenced terrain on a coarse float32 grid
(duplicates, equal distances, long runs of equal curve codes), a slab at 2^16, and spheres whose points crowd near the rim.

* kNN in every form against brute force (oracle.knn_bruteforce): counts and d2 bits exact, rows tie-aware equal.
* ranges (counts, lists, boxes) exactly against brute force.
* the fused kNN products against the oracle's restatement of the reference: bit-equal on >= 99.9 % of rows, the rest within
  COS_TOL; the float64 eigh error is printed, not bounded (the reference's float32 two-pass formula is the contract).
* fixed-radius moments against float64 with DESIGN.md section 16's per-row bound: the normal within
  MOMENT_C eps_f32 tr(Q) / (lambda1 - lambda0) radians, Q about the sphere's centre; centroids within
  CENTROID_C eps_f32 (|q|_inf + r); mean distances within 1e-5 relative.
* the tangent-plane field against brute force (bits) and float64 (ulps of the corners), reconstruct_surface against the host
  pipeline, hierarchy simplification against its model, the bilateral filter and WLOP against the oracle."""
import numpy as np
import pytest

import far_cloud_cases as C
import hierarchy_model as HM
import surface_nets_model as M
from conftest import knn_rows_equivalent, normals_vs_float64_eigh

pytestmark = pytest.mark.gpu
F = np.float32
EPS32 = float(np.finfo(F).eps)
KS = (1, 8, 15, 32, 33)
KMAX = 33
FEW_QUERIES_MAX = 512      # csrc/pcpx_api.hip: the latency path takes nq <= 512 and k <= 32
COS_TOL = 1e-4             # tests/test_gpu_output_forms.py
BIT_EQUAL_FRACTION = 0.999  # tests/test_gpu_configs.py::test_config4_clustered_10m_k15_sharded
MOMENT_C = 4.0
CENTROID_C = 4.0
MEAN_TOL = 1e-5            # relative
POS_TOL = 4e-6             # tests/test_gpu_filters.py, times the cloud's magnitude max |p| here
YARD_FACTOR = 4.0

_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = C.case(name)
    return _cases[name]


def _torch():
    return pytest.importorskip("torch")


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ---- kNN ---------------------------------------------------------------------------------------------------------------------
def _check_rows(pts, q, idx, cnt, d2, bi, bc, bd, k, what):
    """GPU rows (idx, cnt, d2) for queries q against brute force at KMAX (its rows of k are the prefixes)."""
    ec = np.minimum(bc, k)
    assert np.array_equal(cnt, ec), what
    live = np.arange(k)[None, :] < ec[:, None]
    assert np.array_equal(np.where(live, d2, 0).view(np.uint32), np.where(live, bd[:, :k], 0).view(np.uint32)), what
    ok, why = knn_rows_equivalent(pts, q, idx, cnt, bi[:, :k], ec)
    assert ok, (what, why)


def _eps_box_drops(pts, q, eps, bc, n_in):
    """Brute force's count is min(KMAX, points outside the eps box |p - q| < eps on all three axes)."""
    inside = np.zeros(len(q), np.int64)
    for j in range(0, len(q), 16):
        d = np.abs(pts[None, :, :] - q[j:j + 16, None, :])
        inside[j:j + 16] = (d < F(eps)).all(-1).sum(1)
    assert np.array_equal(bc, np.minimum(KMAX, n_in - inside))
    return inside


@pytest.mark.parametrize("name", C.NAMES)
def test_knn_every_form(pkg, oracle, name):
    torch = _torch()
    dev = torch.device("cuda", 0)
    c = _case(name)
    pts, rows = c.points, c.rows
    n = len(pts)
    ix = pkg.LinkedOctree(pts)
    rng = np.random.default_rng(3)
    qb = pts[rows].copy()  # batch queries: half on points, half moved by up to a radius
    qb[1::2] = (qb[1::2] + rng.uniform(-1, 1, (len(qb[1::2]), 3)) * F(c.radius)).astype(F)
    qb = qb.astype(F)
    qs = qb[:300]  # latency-sized
    d_pts_q = torch.from_numpy(qb).to(dev)
    perm_t = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ix.perm_dev(perm_t.data_ptr())
    ix.synchronize()
    perm = perm_t.cpu().numpy().astype(np.int64)
    for eps in (0.0, 1e-5):
        bi, bc, bd = oracle.knn_bruteforce(pts, pts[rows], KMAX, eps=eps, nthreads=16, want_d2=True)
        qi, qc, qd = oracle.knn_bruteforce(pts, qb, KMAX, eps=eps, nthreads=16, want_d2=True)
        if name in ("utm", "small") and eps > 0:
            inside = _eps_box_drops(pts, pts[rows], eps, bc, n)
            print("%s eps=%g: %d of %d rows drop more than their own point" % (name, eps, int((inside > 1).sum()), len(rows)))
        for k in KS:
            what = (name, eps, k)
            idx, cnt, d2 = ix.knn_self(k, eps, want_d2=True)
            _check_rows(pts, pts[rows], idx[rows], cnt[rows], d2[rows], bi, bc, bd, k, what + ("self",))
            # device forms: the same rows, bit for bit
            t_idx = torch.full((n, k), -7, dtype=torch.int32, device=dev)
            t_cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
            t_d2 = torch.full((n, k), -7.0, dtype=torch.float32, device=dev)
            ix.knn_self_dev(k, eps, t_idx.data_ptr(), t_cnt.data_ptr(), t_d2.data_ptr())
            ix.synchronize()
            assert np.array_equal(t_idx.cpu().numpy().view(np.uint32), idx) and np.array_equal(t_cnt.cpu().numpy(), cnt.view(np.int32)), what
            assert np.array_equal(t_d2.cpu().numpy().view(np.uint32), d2.view(np.uint32)), what
            if k <= 32:  # (the strided forms take k <= 32)
                stride = k + 3
                s_idx = torch.full((n, stride), -7, dtype=torch.int32, device=dev)
                s_cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
                s_d2 = torch.full((n, stride), -7.0, dtype=torch.float32, device=dev)
                ix.knn_self_strided_dev(k, eps, stride, s_idx.data_ptr(), s_cnt.data_ptr(), s_d2.data_ptr())
                ix.synchronize()
                si, sd = s_idx.cpu().numpy().view(np.uint32), s_d2.cpu().numpy()
                assert np.array_equal(si[:, :k], idx) and np.array_equal(sd[:, :k].view(np.uint32), d2.view(np.uint32)), what
                assert (si[:, k:] == 0xFFFFFFFF).all() and np.isposinf(sd[:, k:]).all(), what
            c_idx = torch.full((n, k), -7, dtype=torch.int32, device=dev)
            c_cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
            c_d2 = torch.full((n, k), -7.0, dtype=torch.float32, device=dev)
            ix.knn_self_curve_order_dev(k, eps, c_idx.data_ptr(), c_cnt.data_ptr(), c_d2.data_ptr())
            ix.synchronize()
            assert np.array_equal(c_idx.cpu().numpy().view(np.uint32), idx[perm]), what
            assert np.array_equal(c_d2.cpu().numpy().view(np.uint32), d2[perm].view(np.uint32)), what
            # batch and latency
            bidx, bcnt, bd2 = ix.knn(qb, k, eps, want_d2=True)
            _check_rows(pts, qb, bidx, bcnt, bd2, qi, qc, qd, k, what + ("batch",))
            lidx, lcnt, ld2 = ix.knn(qs, k, eps, want_d2=True)
            assert (k <= 32) == (len(qs) <= FEW_QUERIES_MAX and k <= 32)
            _check_rows(pts, qs, lidx, lcnt, ld2, qi[:300], qc[:300], qd[:300], k, what + ("latency" if k <= 32 else "batch300",))
            g_idx = torch.full((len(qb), k), -7, dtype=torch.int32, device=dev)
            g_cnt = torch.full((len(qb),), -7, dtype=torch.int32, device=dev)
            g_d2 = torch.full((len(qb), k), -7.0, dtype=torch.float32, device=dev)
            ix.knn_batch_dev(d_pts_q.data_ptr(), len(qb), k, eps, g_idx.data_ptr(), g_cnt.data_ptr(), g_d2.data_ptr())
            ix.synchronize()
            _check_rows(pts, qb, g_idx.cpu().numpy().view(np.uint32), g_cnt.cpu().numpy().view(np.uint32), g_d2.cpu().numpy(),
                        qi, qc, qd, k, what + ("batch_dev",))
    ix.close()


# ---- ranges ------------------------------------------------------------------------------------------------------------------
def _brute_set(pts, c, r):
    d = pts - c[None, :]
    return np.nonzero(_d2(pts, c[None, :]) <= F(r) * F(r))[0] if d.size else np.zeros(0, np.int64)


def _lists(off, idx):
    return [np.sort(idx[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


@pytest.mark.parametrize("name", C.NAMES)
def test_ranges_exact(pkg, oracle, name):
    c = _case(name)
    pts, rows, r = c.points, c.rows, c.radius
    if name == "cad_mm":
        assert r > 1
    ix = pkg.LinkedOctree(pts)
    cnt = ix.range_count_self(r)
    assert np.array_equal(cnt[rows], oracle.range_count_bruteforce(pts, pts[rows], r, nthreads=16))
    rng = np.random.default_rng(4)
    q = (pts[rows] + rng.uniform(-1, 1, (len(rows), 3)) * F(r)).astype(F)
    assert np.array_equal(ix.range_count(q, r), oracle.range_count_bruteforce(pts, q, r, nthreads=16))
    sub = q[:400]
    for radius in (r, np.where(np.arange(len(sub)) % 3 == 0, F(0), np.where(np.arange(len(sub)) % 3 == 1, F(r), F(2 * r))).astype(F)):
        off, idx = ix.range_sphere(sub, radius)
        rr = np.broadcast_to(np.asarray(radius, F), (len(sub),))
        for i, got in enumerate(_lists(off, idx)):
            assert np.array_equal(got, _brute_set(pts, sub[i], rr[i])), (name, i)
    a, b = pts[rng.integers(0, len(pts), (2, 200))]
    span = (np.abs(a - b) % F(4 * r)).astype(F)
    boxes = np.concatenate([np.minimum(a, b), (np.minimum(a, b) + span).astype(F)], 1).astype(F)
    off, idx = ix.range_aabb(boxes)
    for i, got in enumerate(_lists(off, idx)):
        want = np.nonzero(((pts >= boxes[i, :3]) & (pts <= boxes[i, 3:])).all(1))[0]
        assert np.array_equal(got, want), (name, i)
    ix.close()


# ---- fused kNN products --------------------------------------------------------------------------------------------------------
def _bits_mostly_equal(got, want, what):
    """>= BIT_EQUAL_FRACTION of rows bit-equal; returns the mask of rows that are not."""
    g, w = np.asarray(got), np.asarray(want)
    rows_eq = (g.view(np.uint32) == w.view(np.uint32)).reshape(len(g), -1).all(1) | (np.isnan(g).reshape(len(g), -1).all(1) & np.isnan(w).reshape(len(w), -1).all(1))
    frac = float(rows_eq.mean())
    assert frac >= BIT_EQUAL_FRACTION, (what, frac)
    return ~rows_eq, frac


@pytest.mark.parametrize("name", C.NAMES)
@pytest.mark.parametrize("k", [8, 15, 32])
def test_knn_products_against_the_oracle(pkg, oracle, name, k):
    c = _case(name)
    pts = c.points
    ix = pkg.LinkedOctree(pts)
    nrm, idx, cnt = ix.normals_knn_self(k, want_knn=True)
    on = oracle.normals_from_knn(pts, idx, cnt, nthreads=16)
    bad, frac = _bits_mostly_equal(nrm, on, (name, k, "normals"))
    cos = np.abs((nrm[bad].astype(np.float64) * on[bad].astype(np.float64)).sum(1))
    assert (1 - cos).max(initial=0) <= COS_TOL, (name, k)
    # the same rows handed back: normals_from_knn
    assert np.array_equal(ix.normals_from_knn(idx, cnt).view(np.uint32), nrm.view(np.uint32))
    cen, tn = ix.tangent_planes_knn_self(k)
    assert np.array_equal(tn.view(np.uint32), nrm.view(np.uint32))
    _bits_mostly_equal(cen, oracle.centroids_from_knn(pts, idx, cnt), (name, k, "centroids"))
    _bits_mostly_equal(ix.mean_knn_distance_self(k)[:, None], oracle.mean_dist_from_knn(pts, pts, idx, cnt)[:, None], (name, k, "mean"))
    # estimate_normal over explicit sets: the batch form and the single-set form
    rows = c.rows[:400]
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum(cnt[rows])
    sets = np.concatenate([pts[idx[r, : cnt[r]].astype(np.int64)] for r in rows])
    assert np.array_equal(pkg.estimate_normals_batch(sets, off).view(np.uint32), nrm[rows].view(np.uint32))
    for r in rows[:20]:
        assert np.array_equal(pkg.estimate_normal(pts[idx[r, : cnt[r]].astype(np.int64)]), nrm[r])
    worst, ill = normals_vs_float64_eigh(pts, idx[c.rows], cnt[c.rows], nrm[c.rows])
    print("%s k=%d: bit-equal %.5f; float64 eigh worst 1-|cos| %.2e, ill-conditioned %.3f" % (name, k, frac, worst, ill))
    if name == "far_plane":  # the reference's mean of coordinates at 2^16 (float32 step 2^-7) costs it the slab's normal
        off = 1 - np.abs(nrm.astype(np.float64) @ C.plane_normal())
        print("far_plane k=%d: rows whose normal is off the slab's by 1-|cos| > 1e-3: %.3f" % (k, float((off > 1e-3).mean())))
    ix.close()


# ---- fixed-radius moments ----------------------------------------------------------------------------------------------------
def _moment_rows(oracle, pts, centres, radii, sets, nrm, cen, md, cnt, label, ref_check=False):
    """Per-row bounds against float64; returns the worst ratio observed / bound of (normal, centroid, mean distance)."""
    worst = [0.0, 0.0, 0.0]
    conditioned = ref_worse = 0
    for i, s in enumerate(sets):
        n = len(s)
        assert cnt[i] == n, (label, i, int(cnt[i]), n)
        if n == 0:
            continue
        P = pts[s].astype(np.float64)
        q = centres[i].astype(np.float64)
        r = float(radii[i])
        mu = P.mean(0)
        cb = CENTROID_C * EPS32 * (np.abs(q).max() + r)
        ce = np.abs(cen[i].astype(np.float64) - mu).max()
        worst[1] = max(worst[1], ce / cb)
        assert ce <= cb, (label, i, ce, cb)
        d = P - q
        m64 = np.sqrt((d * d).sum(1)).mean()
        if m64 > 0:
            worst[2] = max(worst[2], abs(md[i] - m64) / (MEAN_TOL * m64))
        assert abs(md[i] - m64) <= MEAN_TOL * m64 or (m64 == 0 and md[i] == 0), (label, i, md[i], m64)
        if n < 3:
            continue
        w, v = np.linalg.eigh((P - mu).T @ (P - mu))
        if not (w[0] <= 0.5 * w[1]) or w[1] <= 1e-9 * w[2]:
            continue
        conditioned += 1
        g = nrm[i].astype(np.float64)
        angle = np.arctan2(np.linalg.norm(np.cross(g, v[:, 0])), abs(g @ v[:, 0]))
        bound = MOMENT_C * EPS32 * float((d * d).sum()) / (w[1] - w[0])
        worst[0] = max(worst[0], angle / bound)
        assert angle <= bound, (label, i, angle, bound, n)
        if ref_check:
            ref_err = 1 - abs(float(oracle.estimate_normal(pts[s]).astype(np.float64) @ v[:, 0]))
            if ref_err > 1e-6:
                ref_worse += 1
                assert 1 - abs(float(g @ v[:, 0])) / np.linalg.norm(g) < ref_err, (label, i, ref_err)
    print("%s: %d rows, %d conditioned, %d where the reference's two-pass normal is off by > 1e-6; worst observed / bound: "
          "normal %.3f, centroid %.3f, mean distance %.3f" % (label, len(sets), conditioned, ref_worse, *worst))
    return worst, conditioned, ref_worse


@pytest.mark.parametrize("name", C.NAMES)
def test_range_moments_against_float64(pkg, oracle, name):
    c = _case(name)
    pts, rows, r = c.points, c.rows, c.radius
    ix = pkg.LinkedOctree(pts)
    nrm, cen, md, cnt = ix.range_neighbourhoods_self(r, normals=True, centroids=True, mean_dist=True, counts=True)
    assert np.array_equal(cnt[rows], oracle.range_count_bruteforce(pts, pts[rows], r, nthreads=16))
    sets = [_brute_set(pts, pts[i], r) for i in rows]
    radii = np.full(len(rows), r)
    _, conditioned, ref_worse = _moment_rows(oracle, pts, pts[rows], radii, sets, nrm[rows], cen[rows], md[rows], cnt[rows],
                                             name + " self", ref_check=name in ("far_1e3", "utm", "far_plane"))
    assert conditioned >= len(rows) // 2
    rng = np.random.default_rng(5)
    q = (pts[rows] + rng.uniform(-1, 1, (len(rows), 3)) * F(r)).astype(F)
    bn, bc, bm, bk = ix.range_neighbourhoods(q, r, normals=True, centroids=True, mean_dist=True, counts=True)
    _moment_rows(oracle, pts, q, radii, [_brute_set(pts, x, r) for x in q], bn, bc, bm, bk, name + " batch")
    ix.close()


@pytest.mark.parametrize("offset", C.CAP_OFFSETS, ids=["origin", "2^10"])
@pytest.mark.parametrize("r_over_s", C.CAP_SIZES, ids=["s=r/10", "s=r/100", "s=r/1000"])
def test_range_moments_on_rim_caps(pkg, oracle, offset, r_over_s):
    pts, centres, r = C.cap_case(offset, r_over_s)
    ix = pkg.LinkedOctree(pts)
    nrm, cen, md, cnt = ix.range_neighbourhoods(centres, r, normals=True, centroids=True, mean_dist=True, counts=True)
    sets = [_brute_set(pts, x, r) for x in centres]
    assert all(len(s) == len(pts) // len(centres) for s in sets)
    _, conditioned, _ = _moment_rows(oracle, pts, centres, np.full(len(centres), r), sets, nrm, cen, md, cnt,
                                     "cap offset=%g r/s=%g" % (offset, r_over_s))
    assert conditioned >= len(centres) // 2
    ix.close()


# ---- tangent-plane field and surface reconstruction ----------------------------------------------------------------------------
def _grid(pkg, g):
    return pkg.surface.grid3d(g["x"], g["y"], g["z"], g["dx"], g["dy"], g["dz"], g["sx"], g["sy"], g["sz"])


def _plane_values(cx, cen, nrm, j):
    op = (cx - cen[j]).astype(F)
    return (nrm[j, 0] * op[..., 0] + nrm[j, 1] * op[..., 1]) + nrm[j, 2] * op[..., 2]


FIELD_ULPS = 4.0  # |field - float64 dot(c - o, n)| in ulps of max |corner coordinate|


@pytest.mark.parametrize("name", ["far_1e3", "utm"])
@pytest.mark.parametrize("eps", [1e-5, 0.0])
def test_tangent_plane_field(pkg, oracle, name, eps):
    """Bits against the float32 brute force of the example's definition (the nearest point's plane), and the value against
    float64's dot(c - o_j, n_j) with the same j and the exact corner lo + i d: within FIELD_ULPS ulps of the corner's largest
    coordinate (the corner and c - o are rounded once each at that magnitude; n is a unit vector)."""
    pts = _case(name).points
    ix = pkg.Index(pts)
    cen, nrm = ix.tangent_planes_knn_self(10)
    bb = ix.bbox()
    ext = bb[3:] - bb[:3]
    g = M.regular_grid_containing(bb[:3] - F(0.1) * ext, bb[3:] + F(0.1) * ext, (20, 20, 20))
    got = ix.tangent_plane_sdf(cen, nrm, _grid(pkg, g), eps=eps).ravel()
    cx = M.corner_positions(g)
    kk = 8
    idx, cnt, d2 = oracle.knn_bruteforce(pts, cx, kk, eps=eps, nthreads=16, want_d2=True)
    cand = np.stack([_plane_values(cx, cen, nrm, idx[:, q]) for q in range(kk)], axis=1)
    tied = d2 == d2[:, :1]
    hit = (cand.view(np.uint32) == got.view(np.uint32)[:, None]) & tied
    all_tied = tied.all(1)
    assert np.all(hit.any(1) | all_tied), "%d corners differ" % int((~(hit.any(1) | all_tied)).sum())
    # float64 of the same definition at the chosen point
    sel = hit.any(1)
    j = idx[sel, np.argmax(hit[sel], 1)].astype(np.int64)
    s = np.array([g["sx"] + 1, g["sy"] + 1, g["sz"] + 1])
    lin = np.nonzero(sel)[0]
    ii = np.stack([lin % s[0], (lin // s[0]) % s[1], lin // (s[0] * s[1])], 1).astype(np.float64)
    exact = np.array([g["x"], g["y"], g["z"]], np.float64) + ii * np.array([g["dx"], g["dy"], g["dz"]], np.float64)
    v64 = ((exact - cen[j].astype(np.float64)) * nrm[j].astype(np.float64)).sum(1)
    ulp = np.spacing(F(np.abs(cx).max())).astype(np.float64)
    err = np.abs(got[sel].astype(np.float64) - v64) / ulp
    print("%s eps=%g: field vs float64: worst %.2f ulps of %.3g" % (name, eps, err.max(), ulp))
    assert err.max() <= FIELD_ULPS


@pytest.mark.parametrize("name", ["far_1e3", "utm"])
def test_reconstruct_surface_matches_host_pipeline(pkg, name):
    pts = _case(name).points
    ix = pkg.Index(pts)
    dims = 24
    v, t, cen_d, nrm_d, grid = ix.reconstruct_surface(10, (dims, dims, dims), want_planes=True)
    cen, nrm = ix.tangent_planes_knn_self(10)
    idx, cnt = ix.knn_self(10)
    nrm_o, _ = pkg.propagate_normal_orientations(pts, idx, nrm, cnt)
    assert np.array_equal(cen_d, cen) and np.array_equal(nrm_d, nrm_o)
    bb = ix.bbox()
    g = M.regular_grid_containing(bb[:3], bb[3:], (dims, dims, dims))
    for a in ("x", "y", "z", "dx", "dy", "dz", "sx", "sy", "sz"):
        assert getattr(grid, a) == g[a], a
    field = ix.tangent_plane_sdf(cen, nrm_o, grid)
    wv, wt = M.surface_nets(field, g)
    assert v.shape == wv.shape and t.shape == wt.shape
    assert np.array_equal(v.view(np.uint32), wv.view(np.uint32)) and np.array_equal(t, wt)
    assert len(t) > 100


# ---- hierarchy simplification --------------------------------------------------------------------------------------------------
HIER_THRESHOLDS = {"f": 1e-9, "var": 1e-9, "gap": 1e-6, "sign": 1e-9, "d2": 1e-9}  # tests/test_gpu_hierarchy.py
HIER_CASES = [("far_1e3", 32, 1.0 / 3.0), ("far_1e3", 10 ** 4, 0.1), ("utm", 10 ** 4, 0.1), ("utm", 10 ** 4, 0.02)]


@pytest.mark.parametrize("name,cluster_size,var_max", HIER_CASES)
def test_hierarchy_simplification(pkg, name, cluster_size, var_max):
    """tests/test_gpu_hierarchy.py::_check: the model's decision margins first, then the kept indices equal, in order."""
    pts = _case(name).points
    r = HM.hierarchy(pts, cluster_size, var_max)
    low = {k: r["margins"][k] for k in HIER_THRESHOLDS if r["margins"][k] < HIER_THRESHOLDS[k]}
    assert not low, "case too close to a decision for exact parity: %s" % low
    out, idx = pkg.hierarchy_simplification(pts, cluster_size, var_max, return_indices=True)
    assert np.array_equal(idx, r["idx"])
    assert np.array_equal(out, pts[idx.astype(np.int64)])


# ---- filters ---------------------------------------------------------------------------------------------------------------------
def _magnitude(pts):
    return float(np.abs(pts).max())


def test_bilateral_filter_far(pkg, oracle):
    """far_1e3's points with their k = 15 normals, one iteration: |gpu - oracle| <= POS_TOL max|p| (test_gpu_filters.py's
    tolerance, whose _extent is already the magnitude max|p|; 1.2e-4 = one float32 step at 2^10, so ~33 steps) and the float64
    yardstick's ratio as there."""
    pts = _case("far_1e3").points
    nrm = pkg.LinkedOctree(pts).normals_knn_self(15)
    sf = 0.02
    got = pkg.bilateral_filter_points(pts, nrm, sf, sf / 4.0, K=1)
    exp = oracle.bilateral_filter_points(pts, nrm, sf, sf / 4.0, K=1, nthreads=16)
    yard = oracle.bilateral_filter_points(pts, nrm, sf, sf / 4.0, K=1, f64_yardstick=True, nthreads=16)
    mag = _magnitude(pts)
    err, e_gpu, e_orc = np.abs(got - exp).max(), np.abs(got - yard).max(), np.abs(exp - yard).max()
    print("bilateral far_1e3: |gpu-oracle| %.2e |gpu-f64| %.2e |oracle-f64| %.2e (magnitude %.1f)" % (err, e_gpu, e_orc, mag))
    assert err <= POS_TOL * mag
    assert e_gpu <= YARD_FACTOR * max(e_orc, 1e-7 * mag)
    assert np.abs(got - pts).max() > 0


@pytest.mark.parametrize("uniform", [True, False], ids=["wlop", "lop"])
def test_wlop_far(pkg, oracle, uniform):
    """far_1e3, one iteration, 5 000 of the points as the sample: the tolerances of test_gpu_filters.py::test_wlop_one_iteration
    times the magnitude max|p| (POS_TOL there is absolute on a cloud of magnitude 1)."""
    pts = _case("far_1e3").points
    sample = np.random.default_rng(21).permutation(len(pts))[-5000:].astype(np.uint64)
    h = 0.05
    got = pkg.wlop(pts, mu=0.45, h=h, k=1, uniform=uniform, sample=sample)
    exp = oracle.wlop(pts, sample, 0.45, h, 1, uniform=uniform, nthreads=16)
    yard = oracle.wlop(pts, sample, 0.45, h, 1, uniform=uniform, f64_yardstick=True, nthreads=16)
    mag = _magnitude(pts)
    err, e_gpu, e_orc = np.abs(got - exp).max(), np.abs(got - yard).max(), np.abs(exp - yard).max()
    print("wlop far_1e3 uniform=%s: |gpu-oracle| %.2e |gpu-f64| %.2e |oracle-f64| %.2e" % (uniform, err, e_gpu, e_orc))
    assert err <= POS_TOL * mag
    assert e_gpu <= YARD_FACTOR * max(e_orc, 1e-7 * mag)
    assert np.abs(got - pts[sample.astype(np.int64)]).max() > 1e-3


# ---- the reference's own outputs at the new offsets and scales (tests/golden/ref_far.npz) ----------------------------------------
def _far():
    import os
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "ref_far.npz"))


def _sha(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


@pytest.mark.parametrize("name,eps", [("far_1e3", 1e-5), ("utm", 1e-5), ("utm", 0.0), ("small", 1e-5), ("small", 0.0)])
def test_reference_far_knn(pkg, oracle, name, eps):
    """The reference's octree rows (k = 15) at |q| ~ 10^3, on the coarse utm grid and at 10^-3: tie-aware equal, and the
    reference's own rows are brute force's."""
    z = _far()
    pts = _case(name).points
    assert np.array_equal(_sha(pts), z[name + "_sha"]), "tests/far_cloud_cases.py no longer builds the recorded cloud"
    key = "knn_%s_eps%d" % (name, int(eps > 0))
    rows = z[key + "_rows"].astype(np.int64)
    idx, cnt = pkg.LinkedOctree(pts).knn_self(15, eps)
    ok, why = knn_rows_equivalent(pts, pts[rows], idx[rows], cnt[rows], z[key + "_idx"], z[key + "_cnt"])
    assert ok, why
    bi, bc = oracle.knn_bruteforce(pts, pts[rows], 15, eps=eps, nthreads=16)
    ok, why = knn_rows_equivalent(pts, pts[rows], bi, bc, z[key + "_idx"], z[key + "_cnt"])
    assert ok, why


@pytest.mark.parametrize("name", ["cad_mm", "utm"])
def test_reference_far_range_lists(pkg, name):
    """One radius per sphere.  r <= 1: the reference's sets.  r > 1: the reference prunes boxes with d^2 <= r (DESIGN.md
    section 10), so its set is within the GPU's, and the GPU's is the geometric answer; at cad_mm (r ~ 40, d^2 ~ 10^3) the
    difference shows on most spheres."""
    z = _far()
    pts = _case(name).points
    assert np.array_equal(_sha(pts), z[name + "_sha"])
    c, r = z["range_%s_centres" % name], z["range_%s_radii" % name]
    off, idx = pkg.LinkedOctree(pts).range_sphere(c, r)
    got, want = _lists(off, idx), _lists(z["range_%s_off" % name], z["range_%s_idx" % name])
    above = 0
    for i in range(len(c)):
        brute = _brute_set(pts, c[i], r[i])
        assert np.array_equal(got[i], brute), (name, i)
        if r[i] <= 1:
            assert np.array_equal(got[i], want[i]), (name, i, r[i])
        else:
            assert np.isin(want[i], got[i]).all(), (name, i)
            above += len(got[i]) > len(want[i])
    print("%s: %d of %d spheres with r > 1 where the reference under-reports" % (name, above, int((r > 1).sum())))
    assert above > 0


def test_reference_far_surface_nets(pkg):
    """Both surface-nets overloads on a grid at 2^14 with spacing 0.03: vertices bit-equal to the reference's, triangles
    equal (tests/test_gpu_reference_golden.py::test_surface_nets's rules), and to the numpy restatement."""
    import surface_nets_hint_model as H
    z = _far()
    g, f, iso, hint = C.far_grid()
    assert np.array_equal(_sha(f), z["grid_field_sha"])
    grid = _grid(pkg, g)
    rv, rt = z["grid_v"], z["grid_t"]
    v, t = pkg.surface_nets(f, grid, iso)
    assert v.shape == rv.shape and t.shape == rt.shape and len(t) > 100
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)), "vertices differ in bits or order"
    assert np.array_equal(t, rt[np.argsort(rt[:, 0], kind="stable")]), "triangles differ"
    mv, mt = M.surface_nets(f, g, iso)
    assert np.array_equal(v.view(np.uint32), mv.view(np.uint32)) and np.array_equal(t, mt)
    hv, ht = pkg.surface_nets_from_hint(f, grid, hint, iso)
    cubes = H.active_cubes(f, g, iso)
    at = {bytes(x): cb for x, cb in zip(v, cubes)}
    rc = np.array([at[bytes(x)] for x in z["grid_hint_v"]], np.int64)
    cv, cc, ct = H.canonical(z["grid_hint_v"], z["grid_hint_t"], rc)
    assert hv.shape == cv.shape and ht.shape == ct.shape
    assert np.array_equal(hv.view(np.uint32), cv.view(np.uint32)) and np.array_equal(cc[ht.astype(np.int64)], ct)
