"""The k <= 16 kernels merge their seed leaves into the best-list in registers, in a loop of their own in front of the buffered
seed loop (csrc/pcpx_query.hip, knn_group: direct_seed_loop); the cloud's last leaf, with its NaN padding, still goes through the
buffer.  These are the clouds and calls where that split has an edge:

* n = 8 ... 3 000: a seed range clamped at either end of the cloud, fewer leaves than the range, a last leaf with 1 ... 7 padding
  slots (n = 9, 17, 63, 65, 97) or none (8, 64, 96, 200, 3 000), which is then the only leaf the buffered loop sees;
* k = 9, 15 (a sentinel slot in the list: the NZ = 1 kernels) and 16 (NZ = 0), rows packed and at a pitch of 16;
* 20 coincident points and a lattice with exact d2 ties, eps = 0 and 1e-5: the deferred eps-box drop inside a direct leaf (at
  eps = 1e-5 a query's own point and its 19 twins are dropped from the leaf's sorted keys; at eps = 0 they stay) and the tie repair;
* an eps that is large against the spacing of the points: the launcher picks the per-candidate kernels, which have no direct leaves;
* batch queries -- near the cloud, outside its box, one with a NaN coordinate -- and a self slice that ends inside a group (a slice starts at a group's first
  position: pcpx_knn_self_strided_dev takes no other);
* the same question twice on one handle.  The second launch hands the groups out by the first one's times and takes long groups
  apart, which needs 512 groups: that one cloud has 36 000 points;
* pcpx_knn_group_costs_dev: the event-counting kernels keep the buffered seed leaves (a fold per seed leaf is due only when a lane
  holds three keys, which a direct leaf cannot tell), so the event table is the one of before --
  tests/golden/seed_direct_group_costs.json holds the tables of the build before the change.

Rows are compared with brute force as in tests/test_gpu_walk_paths.py (check_rows: counts and the bits of d2 exactly, indices
exactly except among points exactly as far as the row's k-th)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_walk_paths import check_rows

pytestmark = pytest.mark.gpu

KMAX = 16
KS = (9, 15, 16)
SIZES = (8, 9, 17, 63, 64, 65, 96, 97, 200, 3000)
EPS_LARGE = 0.02  # 3 eps^2 against 0.01 x (the spacing of 3 000 points in the unit cube)^2 = 4.8e-5: per-candidate kernels


def _make(pkg, kind):
    if kind.startswith("uniform"):
        return pkg.synthetic.uniform_cloud(int(kind[7:]), 300 + len(kind))
    if kind == "coincident":  # 20 copies of one point, scattered over the input order
        base = pkg.synthetic.uniform_cloud(2980, 91)
        pts = np.concatenate([base, np.repeat(base[1234:1235], 20, 0)])
        return pts[np.random.default_rng(6).permutation(len(pts))]
    if kind == "lattice":  # 12^3 points on a grid of 1/16: every d2 is exact and most are shared by many pairs
        g = np.arange(12, dtype=np.float32) / np.float32(16)
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return pts[np.random.default_rng(7).permutation(len(pts))]
    raise ValueError(kind)


class Case:
    def __init__(self, pkg, oracle, kind):
        self.pts = _make(pkg, kind)
        self.ix = pkg.Index(self.pts)
        self.oracle = oracle
        self._brute = {}
        n = len(self.pts)
        rng = np.random.default_rng(n + 1)
        near = self.pts[rng.integers(0, n, 100)] + rng.normal(0, 1e-3, (100, 3)).astype(np.float32)
        lo, hi = self.pts.min(0), self.pts.max(0)
        outside = (hi + (0.1 + rng.random((45, 3))) * (hi - lo + 1)).astype(np.float32)
        outside[::2] = (lo - (0.1 + rng.random((23, 3))) * (hi - lo + 1)).astype(np.float32)
        self.queries = np.concatenate([near, outside, self.pts[: min(n, 40)]]).astype(np.float32)  # (no multiple of 64)

    def brute(self, eps, batch=False):
        key = (eps, batch)
        if key not in self._brute:
            q = self.queries if batch else self.pts
            self._brute[key] = self.oracle.knn_bruteforce(self.pts, q, KMAX, eps=eps, nthreads=16, want_d2=True)
        return self._brute[key]


@pytest.fixture(scope="module")
def cases(pkg, oracle):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Case(pkg, oracle, kind)
        return made[kind]

    yield get
    for c in made.values():
        c.ix.close()


@pytest.mark.parametrize("n", SIZES)
def test_self_rows_at_every_size(cases, n):
    cs = cases("uniform%d" % n)
    for eps in (0.0, 1e-5):
        for k in KS:
            check_rows(cs.pts, cs.pts, cs.ix.knn_self(k, eps, want_d2=True), cs.brute(eps), k, (n, "self", k, eps))


@pytest.mark.parametrize("n", SIZES)
def test_batch_rows_at_every_size(cases, n):
    cs = cases("uniform%d" % n)
    for eps in (0.0, 1e-5):
        for k in KS:
            check_rows(cs.pts, cs.queries, cs.ix.knn(cs.queries, k, eps, want_d2=True), cs.brute(eps, True), k, (n, "batch", k, eps))


def test_a_nan_query_has_an_empty_row(cases):
    cs = cases("uniform3000")
    q = cs.queries.copy()
    q[[3, 70, 130], [0, 1, 2]] = np.nan
    ok = ~np.isnan(q).any(1)
    bi, bc, bd = cs.brute(1e-5, True)
    for k in KS:
        gi, gc, gd = cs.ix.knn(q, k, 1e-5, want_d2=True)
        assert (gc[~ok] == 0).all(), k
        check_rows(cs.pts, q[ok], (gi[ok], gc[ok], gd[ok]), (bi[ok], bc[ok], bd[ok]), k, ("nan", k))


@pytest.mark.parametrize("kind", ["coincident", "lattice"])
@pytest.mark.parametrize("eps", [0.0, 1e-5])
def test_coincident_points_and_exact_ties(cases, kind, eps):
    cs = cases(kind)
    for k in KS:
        check_rows(cs.pts, cs.pts, cs.ix.knn_self(k, eps, want_d2=True), cs.brute(eps), k, (kind, "self", k, eps))
        check_rows(cs.pts, cs.queries, cs.ix.knn(cs.queries, k, eps, want_d2=True), cs.brute(eps, True), k, (kind, "batch", k, eps))


def test_a_large_eps_takes_the_per_candidate_kernels(cases):
    cs = cases("uniform3000")
    for k in KS:
        check_rows(cs.pts, cs.pts, cs.ix.knn_self(k, EPS_LARGE, want_d2=True), cs.brute(EPS_LARGE), k, ("eps_each", "self", k))
        check_rows(cs.pts, cs.queries, cs.ix.knn(cs.queries, k, EPS_LARGE, want_d2=True), cs.brute(EPS_LARGE, True), k, ("eps_each", "batch", k))


def _strided_self(torch, ix, n, k, eps, pitch, first=0, count=None):
    dev = torch.device("cuda", 0)
    idx = torch.full((n, pitch), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((n, pitch), -7.0, dtype=torch.float32, device=dev)
    kw = {} if count is None else dict(first=first, count=count)
    ix.knn_self_strided_dev(k, eps, pitch, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr(), **kw)
    ix.synchronize()
    return idx.cpu().numpy(), cnt.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("kind", ["uniform97", "uniform3000", "coincident"])
def test_rows_at_a_pitch_of_16_and_a_slice_that_ends_inside_a_group(pkg, cases, kind):
    torch = pytest.importorskip("torch")
    cs = cases(kind)
    n, dev = len(cs.pts), torch.device("cuda", 0)
    d_pts = torch.from_numpy(cs.pts).to(dev)
    ix = pkg.Index.from_device(d_pts.data_ptr(), n)
    try:
        perm = torch.full((n,), -1, dtype=torch.int32, device=dev)
        ix.perm_dev(perm.data_ptr())
        ix.synchronize()
        perm = perm.long().cpu().numpy()
        first = 64 if n > 200 else 0                 # (the call wants a slice to start at a group's first position) ...
        count = 64 * 4 + 30 if n > 200 else n - 9    # ... and this one ends 30 lanes into a group (the small cloud: 24 into its second)
        rows = np.zeros(n, bool)
        rows[perm[first:first + count]] = True
        bi, bc, bd = cs.brute(1e-5)
        for k in KS:
            for pitch in (k, 16):
                gi, gc, gd = _strided_self(torch, ix, n, k, 1e-5, pitch)
                assert (gi[:, k:] == -1).all() and np.isposinf(gd[:, k:]).all(), (kind, k, pitch)  # (an answered row's padding)
                check_rows(cs.pts, cs.pts, (gi[:, :k].view(np.uint32), gc.view(np.uint32), gd[:, :k]), (bi, bc, bd), k, (kind, "pitch", k, pitch))
                gi, gc, gd = _strided_self(torch, ix, n, k, 1e-5, pitch, first, count)
                assert (gc[~rows] == -7).all() and (gi[~rows] == -7).all() and (gd[~rows] == -7).all(), (kind, k, pitch)
                assert (gi[rows][:, k:] == -1).all() and np.isposinf(gd[rows][:, k:]).all(), (kind, k, pitch)
                check_rows(cs.pts, cs.pts[rows], (gi[rows][:, :k].view(np.uint32), gc[rows].view(np.uint32), gd[rows][:, :k]),
                           (bi[rows], bc[rows], bd[rows]), k, (kind, "slice", k, pitch))
    finally:
        ix.close()


def test_the_same_question_twice_on_one_handle(pkg, oracle):
    """(the second launch runs in the order recorded by the first, with its longest groups taken apart: k_make_order wants 512 groups)"""
    pts = pkg.synthetic.clustered_cloud(36_000, 47)
    ix = pkg.Index(pts)
    try:
        brute = oracle.knn_bruteforce(pts, pts, KMAX, eps=1e-5, nthreads=16, want_d2=True)
        for k in (15, 16):
            first = ix.knn_self(k, 1e-5, want_d2=True)
            check_rows(pts, pts, first, brute, k, ("first", k))
            for _ in range(2):
                again = ix.knn_self(k, 1e-5, want_d2=True)
                assert all(np.array_equal(a, b) for a, b in zip(first, again)), k
    finally:
        ix.close()


def test_group_costs_are_those_of_the_buffered_seed_loop(pkg):
    with open(os.path.join(GOLDEN, "seed_direct_group_costs.json")) as f:
        golden = json.load(f)
    for entry in golden["tables"]:
        make = pkg.synthetic.clustered_cloud if entry["cloud"] == "clustered" else pkg.synthetic.uniform_cloud
        ix = pkg.Index(make(entry["n"], entry["seed"]))
        try:
            ev = ix.knn_group_costs(entry["k"], entry["eps"], entry["group_stride"])
        finally:
            ix.close()
        assert np.array_equal(ev, np.array(entry["events"], np.uint32)), (entry["cloud"], entry["k"])
