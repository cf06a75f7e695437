"""k_knn starts every walk round of a self-query group inside the height-2 ancestor of the group's own points, with the siblings of
its ancestors pending that pass one wave-wide box-to-box test (WalkerT::start_path, csrc/pcpx_device.h; the lanes' nodes:
csrc/pcpx_path_start.h; the bound: csrc/pcpx_box_bound.h).  These are the trees and calls where that start has an edge:

* depths 2, 3, 4, 5 and 7 (lanes 4 ... 4 depth - 1 stand for a node), a partly padded last leaf;
* cloud ends where the last group's height-2 ancestor has one, two or three real last-level nodes (padding siblings in the lanes of
  height 1, a padding node as the second half of the wave's box) and where the last group has 1 ... 8 points;
* 30 coincident points and a far outlier, eps 0 and 1e-5: finite growing caps, then the uncapped round -- every round starts anew;
* a cloud translated by 1e6 and one scaled by 1e-6;
* k = 1, 8, 15, 16, 32: the three KCAP kernels; slices that end inside a group, a slice of one query (a slice that starts inside a
  group of its tree is what a rank-local index asks: the last case);
* the same question twice on a clustered cloud (the second launch takes long groups apart into eight-lane parts);
* a rank-local index for each of 8 ranks.

Rows are checked against brute force with the comparison of tests/test_gpu_walk_paths.py (oracle.knn_bruteforce at k = 32, once per
cloud; the rows of a smaller k are its prefixes)."""
import numpy as np
import pytest

from test_gpu_walk_paths import KMAX, KS, _make, check_rows

pytestmark = pytest.mark.gpu

# n -> what its end looks like (a height-2 node spans 128 points = two groups, a last-level node 32 points)
ENDS = {1024 + r: "one real last-level node, last group of %d" % r for r in range(1, 9)}
ENDS.update({1024 + 40: "two real last-level nodes", 1024 + 64 + 1: "three, last group of 1", 1024 + 64 + 5: "three, last group of 5",
             1024 + 64 + 8: "three, last group of 8", 1024 + 100: "four, the last partly filled"})
CLOUDS = (["uniform%d" % n for n in (100, 128, 400, 512, 2000, 2056, 70001)]  # depths 2, 2, 3, 3, 4, 5, 7
          + ["uniform%d" % n for n in sorted(ENDS)] + ["shells", "shells_eps0", "far", "tiny"])


def _cloud(pkg, kind):
    if kind == "tiny":
        return pkg.synthetic.uniform_cloud(3_000, 83) * np.float32(1e-6), 0.0
    return _make(pkg, kind)


class Case:
    def __init__(self, pkg, oracle, kind):
        self.pts, self.eps = _cloud(pkg, kind)
        self.ix = pkg.Index(self.pts)
        self.brute = oracle.knn_bruteforce(self.pts, self.pts, KMAX, eps=self.eps, nthreads=16, want_d2=True)


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


def test_the_clouds_have_the_depths_they_are_meant_to_have():
    def depth(n):
        leaves, d = (n + 7) // 8, 0
        while 4 ** d < leaves:
            d += 1
        return 2 if d == 1 else d
    assert [depth(n) for n in (100, 128, 400, 512, 2000, 2056, 70001)] == [2, 2, 3, 3, 4, 5, 7]
    assert 70001 % 8 == 1 and all(depth(n) == 4 for n in ENDS)


@pytest.mark.parametrize("kind", CLOUDS)
def test_self_rows_equal_brute_force_at_every_k(cases, kind):
    cs = cases(kind)
    for k in KS:
        check_rows(cs.pts, cs.pts, cs.ix.knn_self(k, cs.eps, want_d2=True), cs.brute, k, (kind, k))


@pytest.mark.parametrize("kind", ["uniform2056", "uniform1093", "shells"])
def test_slices_that_end_inside_a_group(pkg, cases, kind):
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
        bi, bc, bd = cs.brute
        # (a slice starts at a group's first position -- pcpx_knn_self_dev refuses any other -- and ends 6 lanes into a later group;
        #  inside its first group; after one query; with the cloud.  A slice that STARTS inside a group is what a rank-local index
        #  asks of its own tree: test_rank_local_indexes_of_eight_ranks.)
        last = (n - 1) // 64 * 64
        for first, count in ((64 * 3, 64 * 5 + 6), (64 * 2, 30), (64 * 7, 1), (last - 64, n - last + 64)):
            rows = np.zeros(n, bool)
            rows[perm[first:first + count]] = True
            for k in KS:
                idx = torch.full((n, k), -7, dtype=torch.int32, device=dev)
                cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
                d2 = torch.full((n, k), -7.0, dtype=torch.float32, device=dev)
                ix.knn_self_dev(k, cs.eps, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr(), first=first, count=count)
                ix.synchronize()
                gi, gc, gd = idx.cpu().numpy(), cnt.cpu().numpy(), d2.cpu().numpy()
                assert (gc[~rows] == -7).all() and (gi[~rows] == -7).all() and (gd[~rows] == -7).all(), (kind, first, count, k)
                check_rows(cs.pts, cs.pts[rows], (gi[rows].view(np.uint32), gc[rows].view(np.uint32), gd[rows]), (bi[rows], bc[rows], bd[rows]), k,
                           (kind, first, count, k))
    finally:
        ix.close()


@pytest.fixture(scope="module")
def clustered(pkg, oracle):
    """(points, grid, sampled rows, their brute-force rows at k = 15) of the 200 k clustered cloud the last two tests share.  Brute
    force over all 200 k rows takes the oracle ten seconds and more; every row is compared between the launches (or with the
    whole-cloud index's), and one row in eight, drawn at random, with brute force."""
    pts = pkg.synthetic.clustered_cloud(200_000, 84)
    grid = np.concatenate([pts.min(0), pts.max(0)]).astype(np.float32)
    sel = np.sort(np.random.default_rng(84).choice(len(pts), 25_000, replace=False))
    return pts, grid, sel, oracle.knn_bruteforce(pts, pts[sel], 15, eps=1e-5, nthreads=16, want_d2=True)


def _check_sampled(pts, sel, got, brute, k, what):
    idx, cnt, d2 = (a.cpu().numpy() for a in got)
    check_rows(pts, pts[sel], (idx[sel].view(np.uint32), cnt[sel].view(np.uint32), d2[sel]), brute, k, what)


def _ask(torch, ix, n, k, **kw):
    dev = torch.device("cuda", 0)
    idx = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    d2 = torch.full((n, k), float("inf"), dtype=torch.float32, device=dev)
    ix.knn_self_dev(k, 1e-5, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr(), **kw)
    ix.synchronize()
    return idx, cnt, d2


def test_the_same_question_twice(pkg, clustered):
    """the second launch hands the groups out by the first one's recorded times, the long ones as eight-lane parts"""
    torch = pytest.importorskip("torch")
    pts, grid, sel, brute = clustered
    n, k = len(pts), 15
    d_pts = torch.from_numpy(pts).to(torch.device("cuda", 0))
    ix = pkg.Index.from_device(d_pts.data_ptr(), n, voxel_grid=grid)
    try:
        first = _ask(torch, ix, n, k)
        second = _ask(torch, ix, n, k)
        for a, b in zip(first, second):
            assert torch.equal(a, b)
        _check_sampled(pts, sel, second, brute, k, "twice")
    finally:
        ix.close()


def test_rank_local_indexes_of_eight_ranks(pkg, clustered):
    torch = pytest.importorskip("torch")
    pts, grid, sel, brute = clustered
    n, k, world = len(pts), 15, 8
    d_pts = torch.from_numpy(pts).to(torch.device("cuda", 0))
    whole = pkg.Index.from_device(d_pts.data_ptr(), n, voxel_grid=grid)
    try:
        widx, wcnt, wd2 = _ask(torch, whole, n, k)
    finally:
        whole.close()
    idx = torch.full_like(widx, -1)
    cnt = torch.zeros_like(wcnt)
    d2 = torch.full_like(wd2, float("inf"))
    ix, covered = None, 0
    try:
        for rank in range(world):
            kw = dict(voxel_grid=grid, shard=(rank, world), k_hint=k)
            if ix is None:
                ix = pkg.Index.from_device(d_pts.data_ptr(), n, **kw)
            else:
                ix.rebuild_dev(d_pts.data_ptr(), n, **kw)
            first, count = pkg.shard_range(ix.size(), rank, world)
            ix.knn_self_dev(k, 1e-5, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr(), first, count)
            ix.synchronize()
            covered += count
    finally:
        if ix is not None:
            ix.close()
    assert covered == n
    assert torch.equal(cnt, wcnt) and torch.equal(idx, widx) and torch.equal(d2, wd2)
    _check_sampled(pts, sel, (idx, cnt, d2), brute, k, "ranks")
