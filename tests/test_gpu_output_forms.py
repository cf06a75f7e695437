"""The device-resident output contract around the kNN rows, in every form of the kernel (include/pcpx.h):

* strided rows (pcpx_knn_self_strided_dev, pcpx_normals_knn_self_strided_dev): entries k .. row_stride of an answered row are
  0xFFFFFFFF / +inf, whatever the kernel form -- the deferred eps-box test (NZ = 1 or 0) or the per-candidate one (a planar
  cloud picks it on its own, pcpx_debug_eps_test_mode(2) forces it) -- and whatever the caller's buffer held there;
* slices of the curve order [sorted_first, sorted_first + sorted_count): exactly those positions are answered, on a whole-cloud
  handle as on a rank-local one; the rows of every other point keep what the caller put there;
* the fused per-neighbourhood products (pcpx_neighbourhoods_self_dev) and estimate_normal over explicit point sets
  (pcpx_estimate_normals_batch, what estimate_normals runs for a user knn map).

Rows are checked against brute force (oracle.knn_bruteforce, want_d2=True): counts and the bits of d2 exactly, indices exactly
except among points exactly as far as the k-th (the reference leaves those ties to the implementation).  Every other form must
then equal the packed rows of the same handle bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -7          # what the caller's buffers hold before a call
KMAX = 64          # brute force once per cloud and eps at this k; the rows of a smaller k are its prefixes ((d2, index) order)
EPSES = (0.0, 1e-5, 0.05)
STRIDE_KS = (1, 3, 7, 8, 12, 15, 16, 20, 31, 32)
COS_TOL = 1e-4
GAP_TOL = 1e-3


def _torch():
    return pytest.importorskip("torch")


def _kcap(k):
    return 8 if k <= 8 else 16 if k <= 16 else 32


def _strides(k):
    return sorted(s for s in {k, k + 1, _kcap(k), 40} if s >= k)


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _make_cloud(pkg, kind):
    """(points, voxel grid or None) of each cloud."""
    rng = np.random.default_rng(len(kind))
    if kind == "clustered":
        return pkg.synthetic.clustered_cloud(60_000, 71), np.array([0, 0, 0, 1, 1, 1], np.float32)
    if kind == "planar":  # z = 0: a box of zero volume, the automatic choice is the per-candidate form
        xy = pkg.synthetic.uniform_cloud(40_000, 72)[:, :2]
        return np.concatenate([xy, np.zeros((len(xy), 1), np.float32)], 1), None
    if kind == "tiny":  # fewer points than k
        return pkg.synthetic.uniform_cloud(20, 73), None
    if kind == "outside":  # points outside the voxel grid have no row
        return rng.uniform(-0.15, 1.15, (20_000, 3)).astype(np.float32), np.array([0, 0, 0, 1, 1, 1], np.float32)
    if kind == "duplicates":  # every point three times: exact ties everywhere, and points equal to their query
        base = pkg.synthetic.uniform_cloud(15_000, 74)
        pts = np.concatenate([base, base, base])
        return pts[rng.permutation(len(pts))], None
    raise ValueError(kind)


class Cloud:
    """One cloud, one whole-cloud handle (modes are switched on it), brute force rows by eps, packed GPU rows by (mode, eps, k)."""

    def __init__(self, pkg, oracle, torch, kind):
        self.kind, self.torch, self.oracle = kind, torch, oracle
        self.dev = torch.device("cuda", 0)
        self.pts, self.grid = _make_cloud(pkg, kind)
        self.n = len(self.pts)
        self.inside = np.ones(self.n, bool) if self.grid is None else np.all((self.pts >= self.grid[:3]) & (self.pts <= self.grid[3:]), 1)
        self.d_pts = torch.from_numpy(self.pts).to(self.dev)
        self.ix = pkg.Index.from_device(self.d_pts.data_ptr(), self.n, voxel_grid=self.grid)
        assert self.ix.size() == int(self.inside.sum())
        self._bf, self._packed = {}, {}

    def full(self, shape, value, dtype):
        return self.torch.full(shape, value, dtype=dtype, device=self.dev)

    def brute(self, eps):
        """(idx n x KMAX uint32 input indices, cnt, d2) of brute force over the indexed points; rows of the other points unused."""
        if eps not in self._bf:
            sel = np.nonzero(self.inside)[0]
            p = self.pts[sel]
            i, c, d = self.oracle.knn_bruteforce(p, p, KMAX, eps=eps, nthreads=16, want_d2=True)
            idx = np.full((self.n, KMAX), 0xFFFFFFFF, np.uint32)
            cnt = np.zeros(self.n, np.uint32)
            d2 = np.full((self.n, KMAX), np.inf, np.float32)
            ok = i != 0xFFFFFFFF
            idx[sel] = np.where(ok, sel[np.minimum(i, len(sel) - 1)], 0xFFFFFFFF)
            cnt[sel], d2[sel] = c, d
            self._bf[eps] = (idx, cnt, d2)
        return self._bf[eps]

    def packed(self, mode, eps, k):
        """Packed rows (knn_self_dev: idx, cnt, d2) and input-order normals (normals_knn_self_dev, plain form) as device tensors,
        checked against brute force once."""
        key = (mode, eps, k)
        if key not in self._packed:
            t, n = self.torch, self.n
            self.ix.debug_eps_test_mode(mode)
            self.ix.debug_set("gather_outputs", 0)
            idx, cnt, d2 = self.full((n, k), SENT, t.int32), self.full((n,), SENT, t.int32), self.full((n, k), float(SENT), t.float32)
            self.ix.knn_self_dev(k, eps, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
            nrm = self.full((n, 3), float(SENT), t.float32)
            ni, nc = self.full((n, k), SENT, t.int32), self.full((n,), SENT, t.int32)
            self.ix.normals_knn_self_dev(k, eps, nrm.data_ptr(), ni.data_ptr(), nc.data_ptr())
            self.ix.synchronize()
            self.ix.debug_set("gather_outputs", 1)
            assert t.equal(ni, idx) and t.equal(nc, cnt), key
            self.check_rows(idx, cnt, d2, eps, k, key)
            self._packed[key] = (idx, cnt, d2, nrm)
        return self._packed[key]

    def check_rows(self, idx, cnt, d2, eps, k, what):
        bi, bc, bd = self.brute(eps)
        gi, gc, gd = idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy(), d2.cpu().numpy()
        out = ~self.inside
        assert (gc[out] == SENT).all() and (gi[out] == np.uint32(SENT & 0xFFFFFFFF)).all() and (gd[out] == SENT).all(), what
        gi, gc, gd = gi[self.inside], gc[self.inside].astype(np.uint32), gd[self.inside]
        ei, ec, ed = bi[self.inside, :k], np.minimum(bc[self.inside], k), bd[self.inside, :k]
        assert np.array_equal(gc, ec), what
        assert np.array_equal(gd.view(np.uint32), ed.view(np.uint32)), what
        r, c = np.nonzero(gi != ei)
        if len(r):  # only among points exactly as far as the row's k-th, and each such point really is that far
            assert (c < ec[r]).all() and (ed[r, c] == ed[r, ec[r] - 1]).all(), what
            q = self.pts[np.nonzero(self.inside)[0][r]]
            p = self.pts[gi[r, c].astype(np.int64)]
            assert np.array_equal(_d2(p, q).view(np.uint32), ed[r, c].view(np.uint32)), what
            s = np.sort(np.where(np.arange(k) < gc[:, None], gi, np.arange(k, dtype=np.uint32) + np.uint32(0xFFFFFF00)), 1)
            assert (s[:, 1:] != s[:, :-1]).all(), what  # no point twice in a row

    def close(self):
        self.ix.debug_eps_test_mode(0)
        self.ix.close()


@pytest.fixture(scope="module")
def clouds(pkg, oracle):
    torch = _torch()
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Cloud(pkg, oracle, torch, kind)
        return made[kind]

    yield get
    for c in made.values():
        c.close()


# ---- strided rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["clustered", "planar", "tiny", "outside", "duplicates"])
def test_strided_rows_are_padded_to_the_stride_in_every_kernel_form(clouds, kind):
    cl = clouds(kind)
    t, n = cl.torch, cl.n
    answered = t.from_numpy(cl.inside).to(cl.dev)
    failures = []
    for mode in (0, 1, 2):
        for eps in EPSES:
            for k in STRIDE_KS:
                idx, cnt, d2, nrm = cl.packed(mode, eps, k)
                cl.ix.debug_eps_test_mode(mode)
                for stride in _strides(k):
                    col = t.arange(stride, device=cl.dev)[None, :]
                    pad = (col >= cnt[:, None]) & answered[:, None]  # [cnt, stride) of an answered row
                    for form in ("d2", "no_d2", "normals0", "normals1"):
                        si = cl.full((n, stride), SENT, t.int32)
                        sc = cl.full((n,), SENT, t.int32)
                        sd = cl.full((n, stride), float(SENT), t.float32)
                        sn = cl.full((n, 3), float(SENT), t.float32)
                        if form in ("d2", "no_d2"):
                            cl.ix.knn_self_strided_dev(k, eps, stride, si.data_ptr(), sc.data_ptr(), sd.data_ptr() if form == "d2" else None)
                        else:
                            cl.ix.debug_set("gather_outputs", int(form[-1]))
                            cl.ix.normals_knn_self_strided_dev(k, eps, stride, sn.data_ptr(), si.data_ptr(), sc.data_ptr())
                        cl.ix.synchronize()
                        ok = t.equal(si[:, :k], idx) and t.equal(sc, cnt)
                        ok = ok and bool((si[pad] == -1).all()) and bool((si[~answered] == SENT).all())
                        if form == "d2":
                            ok = ok and t.equal(sd[:, :k], d2) and bool(t.isinf(sd[pad]).all()) and bool((sd[~answered] == SENT).all())
                        elif form == "no_d2":
                            ok = ok and bool((sd == SENT).all())
                        else:
                            ok = ok and t.equal(sn, nrm)
                        if not ok:
                            failures.append((mode, eps, k, stride, form))
    cl.ix.debug_set("gather_outputs", 1)
    cl.ix.debug_eps_test_mode(0)
    assert not failures, "%d cases (mode, eps, k, stride, form) differ, first %s" % (len(failures), failures[:12])


def test_strided_rows_refuse_a_stride_below_k(clouds, pkg):
    cl = clouds("clustered")
    t = cl.torch
    si, sc = cl.full((cl.n, 16), SENT, t.int32), cl.full((cl.n,), SENT, t.int32)
    for k, stride in ((15, 14), (33, 40)):
        with pytest.raises(pkg.PcpxError):
            cl.ix.knn_self_strided_dev(k, 1e-5, stride, si.data_ptr(), sc.data_ptr())
        with pytest.raises(pkg.PcpxError):
            cl.ix.normals_knn_self_strided_dev(k, 1e-5, stride, si.data_ptr(), si.data_ptr(), sc.data_ptr())
    cl.ix.synchronize()
    assert bool((si == SENT).all()) and bool((sc == SENT).all())


# ---- slices of the curve order -----------------------------------------------------------------------------------------------
def _perm(cl):
    t = cl.torch
    perm = cl.full((cl.ix.size(),), -1, t.int32)
    cl.ix.perm_dev(perm.data_ptr())
    cl.ix.synchronize()
    return perm.long()


def _slice_handles(pkg, cl, k):
    """(name, handle, first, count) of a whole-cloud and a rank-local handle; each slice starts at a multiple of 64 and its
    length is not one."""
    yield "whole", cl.ix, 64 * 97, 20_000 + 45
    loc = pkg.Index.from_device(cl.d_pts.data_ptr(), cl.n, voxel_grid=cl.grid, shard=(1, 3), k_hint=k)
    try:
        si = loc.shard_info()
        assert si["shard_first"] % 64 == 0 and si["shard_count"] > 1000
        yield "rank-local", loc, si["shard_first"] + 128, si["shard_count"] - 128 - 29
    finally:
        loc.close()


@pytest.mark.parametrize("k", [8, 15, 32, 40])
def test_a_slice_answers_exactly_its_positions(pkg, clouds, k):
    cl = clouds("clustered")
    t, n = cl.torch, cl.n
    idx, cnt, d2, nrm = cl.packed(0, 1e-5, k)
    perm = _perm(cl)
    for name, h, first, count in _slice_handles(pkg, cl, k):
        rows = t.zeros(n, dtype=t.bool, device=cl.dev)
        rows[perm[first:first + count]] = True
        what = (name, k, first, count)
        # input-order rows
        i2, c2, d22 = cl.full((n, k), SENT, t.int32), cl.full((n,), SENT, t.int32), cl.full((n, k), float(SENT), t.float32)
        h.knn_self_dev(k, 1e-5, i2.data_ptr(), c2.data_ptr(), d22.data_ptr(), first=first, count=count)
        h.synchronize()
        assert int((c2 != SENT).sum()) == count, what
        assert t.equal(c2 != SENT, rows), what
        assert t.equal(i2[rows], idx[rows]) and t.equal(c2[rows], cnt[rows]) and t.equal(d22[rows], d2[rows]), what
        assert bool((i2[~rows] == SENT).all()) and bool((d22[~rows] == SENT).all()), what
        # input-order normals, plain and through the gather-form permute
        for gather in (0, 1):
            h.debug_set("gather_outputs", gather)
            n2, c3 = cl.full((n, 3), float(SENT), t.float32), cl.full((n,), SENT, t.int32)
            i3 = cl.full((n, k), SENT, t.int32)
            h.normals_knn_self_dev(k, 1e-5, n2.data_ptr(), i3.data_ptr(), c3.data_ptr(), first=first, count=count)
            h.synchronize()
            assert t.equal(c3 != SENT, rows), what + (gather,)
            assert t.equal(n2[rows], nrm[rows]) and bool((n2[~rows] == SENT).all()), what + (gather,)
        h.debug_set("gather_outputs", 1)
        # rows at curve positions
        if k <= 32:
            i4, c4 = cl.full((n, k), SENT, t.int32), cl.full((n,), SENT, t.int32)
            h.knn_self_curve_order_dev(k, 1e-5, i4.data_ptr(), c4.data_ptr(), first=first, count=count)
            h.synchronize()
            pos = t.zeros(n, dtype=t.bool, device=cl.dev)
            pos[first:first + count] = True
            assert t.equal(c4 != SENT, pos), what
            assert t.equal(i4[first:first + count], idx[perm[first:first + count]]), what
            assert bool((i4[~pos] == SENT).all()), what


def test_a_slice_counts_exactly_its_positions(pkg, clouds, oracle):
    cl = clouds("clustered")
    t, n, radius = cl.torch, cl.n, 0.02
    want = t.from_numpy(oracle.range_count_bruteforce(cl.pts, cl.pts, radius, nthreads=16).astype(np.int32)).to(cl.dev)
    perm = _perm(cl)
    for name, h, first, count in _slice_handles(pkg, cl, 8):
        rows = t.zeros(n, dtype=t.bool, device=cl.dev)
        rows[perm[first:first + count]] = True
        for gather in (0, 1):
            h.debug_set("gather_counts", gather)
            c = cl.full((n,), SENT, t.int32)
            h.range_count_self_dev(radius, c.data_ptr(), first, count)
            h.synchronize()
            assert int((c != SENT).sum()) == count and t.equal(c != SENT, rows), (name, gather)
            assert t.equal(c[rows], want[rows]), (name, gather)
        h.debug_set("gather_counts", 1)
        c = cl.full((n,), SENT, t.int32)
        h.range_count_self_curve_order_dev(radius, c.data_ptr(), first, count)
        h.synchronize()
        assert int((c != SENT).sum()) == count and bool((c[first:first + count] != SENT).all()), name
        assert t.equal(c[first:first + count], want[perm[first:first + count]]), name


# ---- fused per-neighbourhood products ----------------------------------------------------------------------------------------
def _eigh_check(pts, idx, nrm):
    """float64 eigh of the centred scatter matrix of full rows against the float32 normals: (max 1-|cos| over well-conditioned
    rows, their number)."""
    nb = pts[idx.astype(np.int64)].astype(np.float64)
    v = nb - nb.mean(axis=1, keepdims=True)
    w, vec = np.linalg.eigh(np.einsum("rki,rkj->rij", v, v))
    well = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300) >= GAP_TOL
    err = 1.0 - np.abs((vec[:, :, 0] * nrm.astype(np.float64)).sum(1))
    return float(err[well].max()) if well.any() else 0.0, int(well.sum())


@pytest.mark.parametrize("k", [1, 2, 3, 8, 15, 16, 24, 32, 33, 40, 64])
def test_neighbourhood_products_against_the_oracle(pkg, clouds, oracle, k):
    cl = clouds("clustered")
    t, n = cl.torch, cl.n
    perm = _perm(cl)
    first, count = 64 * 211, 9_000 + 13
    rows = t.zeros(n, dtype=t.bool, device=cl.dev)
    rows[perm[first:first + count]] = True
    for mode in (0, 2):
        idx, cnt, _, _ = cl.packed(mode, 1e-5, k)
        cl.ix.debug_eps_test_mode(mode)
        outs = [cl.full((n, 3), float(SENT), t.float32), cl.full((n, 3), float(SENT), t.float32), cl.full((n,), float(SENT), t.float32)]
        cl.ix.neighbourhoods_self_dev(k, 1e-5, *[o.data_ptr() for o in outs])
        cl.ix.synchronize()
        for which in range(3):  # each output on its own gives the same bits
            alone = cl.full(outs[which].shape, float(SENT), t.float32)
            ptrs = [None, None, None]
            ptrs[which] = alone.data_ptr()
            cl.ix.neighbourhoods_self_dev(k, 1e-5, *ptrs)
            cl.ix.synchronize()
            assert t.equal(alone, outs[which]), (mode, k, which)
        # a slice: its rows as above, every other row as the caller left it
        sl = [cl.full(o.shape, float(SENT), t.float32) for o in outs]
        cl.ix.neighbourhoods_self_dev(k, 1e-5, *[o.data_ptr() for o in sl], first=first, count=count)
        cl.ix.synchronize()
        for a, b in zip(sl, outs):
            assert t.equal(a[rows], b[rows]) and bool((a[~rows] == SENT).all()), (mode, k)
        # against the oracle on the GPU's own rows
        nrm, cen, md = (o.cpu().numpy() for o in outs)
        gi, gc = idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
        assert np.array_equal(cen.view(np.uint32), oracle.centroids_from_knn(cl.pts, gi, gc).view(np.uint32)), (mode, k)
        assert np.array_equal(md.view(np.uint32), oracle.mean_dist_from_knn(cl.pts, cl.pts, gi, gc).view(np.uint32)), (mode, k)
        if k >= 3:
            on = oracle.normals_from_knn(cl.pts, gi, gc, nthreads=16)
            cos = np.abs((nrm.astype(np.float64) * on.astype(np.float64)).sum(1))
            assert (1.0 - cos).max() <= COS_TOL, (mode, k, (1.0 - cos).max())
            full = np.nonzero(gc == k)[0][::7]
            err, nwell = _eigh_check(cl.pts, gi[full], nrm[full])
            assert nwell > len(full) // 2 and err <= COS_TOL, (mode, k, err, nwell)
        else:  # one or two points span no plane: a unit normal, across the pair's direction
            assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-5), (mode, k)
            if k == 2:
                dirs = cl.pts[gi[:, 1].astype(np.int64)].astype(np.float64) - cl.pts[gi[:, 0].astype(np.int64)]
                dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
                assert np.abs((dirs * nrm).sum(1)).max() <= 1e-3, (mode, k)
    cl.ix.debug_eps_test_mode(0)


@pytest.mark.parametrize("k", [8, 40])
def test_an_empty_neighbourhood_has_nan_mean_distance(clouds, k):
    cl = clouds("clustered")
    t, n = cl.torch, cl.n
    md, cen = cl.full((n,), float(SENT), t.float32), cl.full((n, 3), float(SENT), t.float32)
    cl.ix.neighbourhoods_self_dev(k, 10.0, None, cen.data_ptr(), md.data_ptr())  # every point lies inside every eps-box
    cl.ix.synchronize()
    assert bool(t.isnan(md).all()) and bool(t.isnan(cen).all())


# ---- estimate_normal over explicit point sets ---------------------------------------------------------------------------------
def test_estimate_normals_batch_equals_the_oracle_row_by_row(pkg, oracle):
    rng = np.random.default_rng(9)
    sizes = [0, 1, 2, 3, 7, 63, 64, 65, 1000, 4097] + rng.integers(0, 40, 300).tolist() + [0, 5, 0]
    base = 11  # the offsets start here, not at 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64) + np.uint64(base)
    pts = np.empty((int(off[-1]) + 6, 3), np.float32)
    pts[:] = rng.uniform(-5, 5, pts.shape)  # (points before offsets[0] and after the last row belong to no row)
    for r, m in enumerate(sizes):  # each row a noisy tilted patch somewhere
        a = int(off[r])
        e = rng.normal(size=(3, 3))
        pts[a:a + m] = (rng.uniform(-1, 1, (m, 3)) * [1.0, 0.6, 0.02]) @ e + rng.uniform(-20, 20, 3)
    got = pkg.estimate_normals_batch(pts, off)
    assert got.shape == (len(sizes), 3)
    for r, m in enumerate(sizes):
        want = oracle.estimate_normal(pts[int(off[r]):int(off[r + 1])])
        if m == 0:
            assert np.array_equal(got[r], want, equal_nan=True), (r, got[r], want)
        else:
            assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (r, m, got[r], want)
    with pytest.raises(pkg.PcpxError):
        pkg.estimate_normals_batch(pts, np.array([3, 9, 8, 12], np.uint64))
    assert pkg.estimate_normals_batch(pts, np.array([7], np.uint64)).shape == (0, 3)
