"""k_knn's epilogue reads each neighbour's leaf record once for the fused normal: the coordinates gathered in the row's final order
(after the tie repair), held by the lane, and used by both the centroid and the scatter sums (csrc/pcpx_query.hip, knn_group).
What can go wrong there, case by case:

* a neighbour's coordinates must follow its id through the tie repair -- integer lattices, where every row has exact d2 ties;
* `ok` masking of rows with fewer than k neighbours, the found = 0 contract (mean distance and centroid NaN), lanes of a group
  that hold no query, and a last group with fewer than 64 valid lanes;
* coincident points, with eps = 0 and with an eps-box;
* every kernel (KCAP 8 / 16 / 32) in both sentinel forms (k = KCAP - 1 and k = KCAP), and one k > 32, which takes the multi-pass
  path the change does not touch;
* every output form, which must give the same bits;
* 40 000 points: 625 query groups, every row compared.

Rows are checked against a numpy brute force in ascending (d2, index) order -- counts and the bits of d2 exactly, indices exactly
except among points exactly as far as the k-th (which of those a row holds is left to the implementation, tests/test_gpu_parity.py)
-- and normals three ways: bit for bit against the explicit-row kernel (pcpx_normals_from_knn) on the returned rows, which is
"the normal recomputed from the returned ids"; against a float64 eigh of the returned row within the 1e-4 cosine of
tests/test_gpu_parity.py, leaving out the rows that conftest.normals_vs_float64_eigh calls ill-conditioned (relative eigenvalue
gap < 1e-3); and, for centroid and mean distance, against the same float32 sums formed in numpy in row order."""
import numpy as np
import pytest

from conftest import normals_vs_float64_eigh

pytestmark = pytest.mark.gpu

COS_TOL = 1e-4  # tests/test_gpu_parity.py
INVALID = np.uint32(0xFFFFFFFF)
SENT = -7


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _brute(pts, queries, k, eps):
    """(idx, cnt, d2) of every query's k nearest points outside its eps-box, ascending in (d2, index); float32 arithmetic in the
    kernel's order."""
    pts, queries = np.asarray(pts, np.float32), np.asarray(queries, np.float32)
    nq, n = len(queries), len(pts)
    idx = np.full((nq, k), INVALID, np.uint32)
    d2o = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.uint32)
    for a in range(0, nq, 1024):
        q = queries[a:a + 1024]
        d = pts[None, :, :] - q[:, None, :]
        d2 = _d2(d, np.float32(0))
        d2 = np.where(np.abs(d).max(-1) >= np.float32(eps), d2, np.float32(np.inf))  # inside the eps-box: excluded
        # the keys up to each row's k-th smallest d2 (a partition, not a sort of the whole row), then (d2, index) order among those
        kk = min(k, n)
        thr = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        r, c = np.nonzero(d2 <= thr[:, None])
        v = d2[r, c]
        o = np.lexsort((c, v, r))
        r, c, v = r[o], c[o], v[o]
        rank = np.arange(len(r)) - np.searchsorted(r, np.arange(len(q)))[r]
        keep = (rank < k) & np.isfinite(v)
        idx[a + r[keep], rank[keep]] = c[keep]
        d2o[a + r[keep], rank[keep]] = v[keep]
        cnt[a:a + 1024] = np.bincount(r[keep], minlength=len(q))
    return idx, cnt, d2o


def _brute_by_cells(pts, k, eps, cells):
    """_brute(pts, pts, ...) for a cloud in the unit cube, a cell of a cells^3 grid at a time against the points of the 27 cells
    round it.  Exact where a query's k-th distance stays below the cell width (asserted): a point outside those cells is farther
    than that along some axis.  Candidates are taken in ascending index order, so ties are ordered by index as in _brute."""
    n = len(pts)
    cell = np.minimum((pts * cells).astype(np.int64), cells - 1)
    idx = np.full((n, k), INVALID, np.uint32)
    d2o = np.full((n, k), np.inf, np.float32)
    cnt = np.zeros(n, np.uint32)
    for c in np.ndindex(cells, cells, cells):
        mine = np.nonzero((cell == c).all(1))[0]
        if len(mine) == 0:
            continue
        near = np.nonzero((np.abs(cell - np.array(c)) <= 1).all(1))[0]
        i, m, d = _brute(pts[near], pts[mine], k, eps)
        assert (m == k).all() and (d[:, -1] <= np.float32(0.9 / cells) ** 2).all()
        idx[mine], cnt[mine], d2o[mine] = near[i].astype(np.uint32), m, d
    return idx, cnt, d2o


def _check_rows(pts, queries, k, got, want, what):
    gi, gc, gd = got
    bi, bc, bd = want
    assert np.array_equal(gc, bc), what
    valid = np.arange(k)[None, :] < bc[:, None]
    assert np.array_equal(gd[valid].view(np.uint32), bd[valid].view(np.uint32)), what
    assert (gi[~valid] == INVALID).all(), what
    r, c = np.nonzero((gi != bi) & valid)
    if len(r):  # only among points exactly as far as the row's k-th; each really is that far; no point twice; (d2, index) order
        assert (bd[r, c] == bd[r, bc[r] - 1]).all(), what
        assert np.array_equal(_d2(pts[gi[r, c].astype(np.int64)], np.asarray(queries, np.float32)[r]).view(np.uint32), bd[r, c].view(np.uint32)), what
    rising = (gd[:, 1:] > gd[:, :-1]) | ((gd[:, 1:] == gd[:, :-1]) & (gi[:, 1:] > gi[:, :-1]))
    assert rising[valid[:, 1:]].all(), what


def _row_sums(pts, queries, gi, gc):
    """(centroid, mean distance) of each returned row as the kernel forms them: float32 sums from zero in row order, divided by
    the float32 count (0 / 0 = NaN for an empty row)."""
    k = gi.shape[1]
    s = np.zeros((len(gi), 3), np.float32)
    dist = np.zeros(len(gi), np.float32)
    for j in range(k):
        ok = j < gc
        p = pts[np.where(ok, gi[:, j], 0).astype(np.int64)]
        s = s + np.where(ok[:, None], p, np.float32(0))
        dist = dist + np.where(ok, np.sqrt(_d2(p, queries)), np.float32(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        fn = gc.astype(np.float32)
        return s / fn[:, None], dist / fn


def _check_normals(ix, pts, gi, gc, nrm, what, eigh_rows=600):
    """The fused normals against the explicit-row kernel on the same rows (bits) and against float64 eigh (1e-4 cosine)."""
    some = np.nonzero(gc > 0)[0]
    if len(some):
        again = ix.normals_from_knn(gi[some], gc[some])
        assert np.array_equal(again.view(np.uint32), nrm[some].view(np.uint32)), what
    full = np.nonzero(gc >= 3)[0]
    full = full[:: max(1, len(full) // eigh_rows)]
    if len(full):
        worst, ill = normals_vs_float64_eigh(pts, gi[full], gc[full], nrm[full])
        print("%s: max 1-|cos| vs float64 eigh %.2e over %d rows, ill-conditioned fraction %.3f" % (what, worst, len(full), ill))
        assert worst <= COS_TOL, what


def _self_case(pkg, pts, k, eps, what, want=None, eigh_rows=600):
    """Host entry points on one cloud: rows (with d2), fused normals with rows, tangent planes, mean distances."""
    pts = np.ascontiguousarray(pts, np.float32)
    ix = pkg.Index(pts)
    gi, gc, gd = ix.knn_self(k, eps, want_d2=True)
    _check_rows(pts, pts, k, (gi, gc, gd), want or _brute(pts, pts, k, eps), what)
    nrm, ni, nc = ix.normals_knn_self(k, eps, want_knn=True)
    assert np.array_equal(ni, gi) and np.array_equal(nc, gc), what
    _check_normals(ix, pts, gi, gc, nrm, what, eigh_rows)
    cen, pn = ix.tangent_planes_knn_self(k, eps)
    md = ix.mean_knn_distance_self(k, eps)
    wc, wm = _row_sums(pts, pts, gi, gc)
    assert np.array_equal(pn.view(np.uint32), nrm.view(np.uint32)), what
    assert np.array_equal(cen, wc, equal_nan=True) and np.array_equal(md, wm, equal_nan=True), what
    empty = gc == 0
    assert np.isnan(md[empty]).all() and np.isnan(cen[empty]).all(), what
    ix.close()
    return gi, gc, nrm


def _lattice(side):
    g = np.arange(side, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return pts[np.random.default_rng(side).permutation(len(pts))]


@pytest.mark.parametrize("k", [15, 16])
@pytest.mark.parametrize("side", [6, 9])
def test_integer_lattice_coordinates_follow_ids_through_the_tie_repair(pkg, side, k):
    pts = _lattice(side)  # 216 points: four groups; 729: twelve, the last with 25 valid lanes
    gi, gc, nrm = _self_case(pkg, pts, k, 1e-5, ("lattice", side, k))
    assert (gc == k).all()
    # every row does contain runs of exactly equal d2 (or the case would be vacuous)
    d2 = _d2(pts[gi.astype(np.int64)], pts[:, None, :])
    assert ((d2[:, 1:] == d2[:, :-1]).sum(1) >= 5).all()


@pytest.mark.parametrize("n,k", [(1, 15), (9, 15), (9, 7), (64 * 3 + 5, 15), (64 * 3 + 5, 32), (20, 31)])
def test_fewer_than_k_neighbours_and_partly_filled_groups(pkg, n, k):
    pts = np.random.default_rng(n + k).random((n, 3), dtype=np.float32)
    gi, gc, nrm = _self_case(pkg, pts, k, 1e-5, ("few", n, k))
    assert (gc == min(k, n - 1)).all()


@pytest.mark.parametrize("eps", [0.0, 1e-5])
@pytest.mark.parametrize("k", [8, 15])
def test_coincident_points(pkg, eps, k):
    rng = np.random.default_rng(5)
    base = rng.random((700, 3), dtype=np.float32)
    pts = np.concatenate([base, base[:300], base[:300], base[:40] + np.float32(3e-6), rng.random((200, 3), dtype=np.float32)])
    pts = pts[rng.permutation(len(pts))]
    _self_case(pkg, pts, k, eps, ("coincident", eps, k))


@pytest.fixture(scope="module")
def cloud3k(pkg):
    pts = pkg.synthetic.uniform_cloud(3000 + 37, 11)
    return pts, {}


def _brute3k(cloud3k, k, eps=1e-5):
    pts, cache = cloud3k
    if eps not in cache:
        cache[eps] = _brute(pts, pts, 40, eps)  # once per eps: the rows of a smaller k are its prefixes
    i, c, d = cache[eps]
    return i[:, :k].copy(), np.minimum(c, k).astype(np.uint32), d[:, :k].copy()


@pytest.mark.parametrize("k", [7, 8, 15, 16, 31, 32, 40])
def test_every_kernel_and_both_sentinel_forms(pkg, cloud3k, k):
    _self_case(pkg, cloud3k[0], k, 1e-5, ("kernels", k), want=_brute3k(cloud3k, k))


@pytest.mark.parametrize("k", [15, 16, 7, 32])
def test_every_output_form_gives_the_same_bits(pkg, cloud3k, k):
    torch = pytest.importorskip("torch")
    pts = cloud3k[0]
    n, eps, dev = len(pts), 1e-5, torch.device("cuda", 0)
    kcap = 8 if k <= 8 else 16 if k <= 16 else 32
    d_pts = torch.from_numpy(pts).to(dev)
    ix = pkg.Index.from_device(d_pts.data_ptr(), n)
    full = lambda shape, dtype: torch.full(shape, SENT, dtype=dtype, device=dev)
    # rows only, packed, with d2: against brute force
    idx, cnt, d2 = full((n, k), torch.int32), full((n,), torch.int32), full((n, k), torch.float32)
    ix.knn_self_dev(k, eps, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
    # normals with packed rows; normals only
    nrm, ni, nc = full((n, 3), torch.float32), full((n, k), torch.int32), full((n,), torch.int32)
    ix.normals_knn_self_dev(k, eps, nrm.data_ptr(), ni.data_ptr(), nc.data_ptr())
    only = full((n, 3), torch.float32)
    ix.normals_knn_self_dev(k, eps, only.data_ptr())
    # rows at pitch KCAP with normals
    sn, si, sc = full((n, 3), torch.float32), full((n, kcap), torch.int32), full((n,), torch.int32)
    ix.normals_knn_self_strided_dev(k, eps, kcap, sn.data_ptr(), si.data_ptr(), sc.data_ptr())
    # curve order (by_position) with normals
    cn, ci, cc, cd = full((n, 3), torch.float32), full((n, k), torch.int32), full((n,), torch.int32), full((n, k), torch.float32)
    ix.knn_self_curve_order_dev(k, eps, ci.data_ptr(), cc.data_ptr(), cd.data_ptr(), cn.data_ptr())
    perm = full((n,), torch.int32)
    ix.perm_dev(perm.data_ptr())
    # centroids + normals, mean distance + normals
    n1, cen = full((n, 3), torch.float32), full((n, 3), torch.float32)
    ix.neighbourhoods_self_dev(k, eps, n1.data_ptr(), cen.data_ptr(), None)
    n2, md = full((n, 3), torch.float32), full((n,), torch.float32)
    ix.neighbourhoods_self_dev(k, eps, n2.data_ptr(), None, md.data_ptr())
    ix.synchronize()
    gi, gc, gd = idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32), d2.cpu().numpy()
    _check_rows(pts, pts, k, (gi, gc, gd), _brute3k(cloud3k, k), ("forms", k))
    assert torch.equal(ni, idx) and torch.equal(nc, cnt)
    for other in (only, sn, n1, n2):
        assert torch.equal(other.view(torch.int32), nrm.view(torch.int32)), k
    assert torch.equal(si[:, :k], idx) and torch.equal(sc, cnt) and bool((si[:, k:] == -1).all())
    p = perm.long()
    assert torch.equal(ci, idx[p]) and torch.equal(cc, cnt[p]) and torch.equal(cd, d2[p])
    assert torch.equal(cn.view(torch.int32), nrm[p].view(torch.int32))
    wc, wm = _row_sums(pts, pts, gi, gc)
    assert np.array_equal(cen.cpu().numpy(), wc) and np.array_equal(md.cpu().numpy(), wm)
    _check_normals(ix, pts, gi, gc, nrm.cpu().numpy(), ("forms", k), eigh_rows=300)
    ix.close()


@pytest.mark.parametrize("k", [8, 15, 16, 32])
def test_batch_queries_not_in_the_cloud(pkg, cloud3k, k):
    pts = cloud3k[0]
    rng = np.random.default_rng(k)
    q = np.concatenate([rng.random((777, 3), dtype=np.float32) * np.float32(1.4) - np.float32(0.2), pts[:50] + np.float32(2e-6)])
    ix = pkg.Index(pts)
    for eps in (0.0, 1e-5):
        got = ix.knn(q, k, eps, want_d2=True)
        _check_rows(pts, q, k, got, _brute(pts, q, k, eps), ("batch", k, eps))
    ix.close()


def test_many_groups_every_row(pkg):
    """40 000 points = 625 query groups on the persistent waves (a wave that finishes early takes another: the next group's seed
    phase must find its LDS column as the compaction wants it); every row against brute force."""
    pts = pkg.synthetic.uniform_cloud(40_000, 13)
    assert pts.min() >= 0.0 and pts.max() <= 1.0
    _self_case(pkg, pts, 15, 1e-5, ("many groups", 15), want=_brute_by_cells(pts, 15, 1e-5, 8), eigh_rows=500)
