"""k_knn's walk expands every popped node, whatever its height, through one path (WalkerT::pop_scaled / expand_any,
csrc/pcpx_device.h): the level's first heap id, the climb from the last expanded node and the place of the child mask -- pending
bits or the leaf loop -- all come from the popped bit's number.  These are the trees and calls where that arithmetic has an edge:

* depth 0 (n <= 8: no walk at all), depth 2 (the smallest real tree -- the build makes no depth 1: the root's children are
  last-level nodes, so the first pop already climbs zero levels), depths 3 and 4 with padding nodes at every level;
* a last leaf that is partly NaN padding; a group whose last-level nodes lie wholly inside its seed range (every leaf of the
  walk skipped); a slice that ends inside a group;
* a clustered cloud with 30 coincident points and one far outlier: lanes that fail the first round's cap go round again, and
  every round starts the walk at the root;
* a cloud translated by 1e6 (coordinates on a grid of 1/16: ties everywhere);
* k = 1, 8, 15, 16, 32: the three KCAP kernels, which load the child boxes in two ways (k <= 8: seven words per box; above: two
  64-byte loads), self and batch queries.

Rows are checked against brute force (oracle.knn_bruteforce at k = 32, once per cloud and eps; the rows of a smaller k are its
prefixes): counts and the bits of d2 exactly, indices exactly except among points exactly as far as the row's k-th, which the
reference leaves to the implementation -- the comparison of tests/test_gpu_output_forms.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KMAX = 32
KS = (1, 8, 15, 16, 32)


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _make(pkg, kind):
    """(points, eps) of each cloud."""
    if kind.startswith("uniform"):  # uniform<n>
        return pkg.synthetic.uniform_cloud(int(kind[7:]), 100 + len(kind)), 1e-5
    if kind.startswith("shells"):  # lanes on 30 coincident points never fill a row inside the first cap; the outlier's row is all far away
        base = pkg.synthetic.clustered_cloud(20_000 - 31, 81)
        pts = np.concatenate([base, np.repeat(base[777:778], 30, 0), np.array([[40.0, -35.0, 60.0]], np.float32)])
        pts = pts[np.random.default_rng(5).permutation(len(pts))]
        return pts, (0.0 if kind == "shells_eps0" else 1e-5)
    if kind == "far":
        return pkg.synthetic.uniform_cloud(3_000, 82) + np.float32(1e6), 1e-5
    raise ValueError(kind)


CLOUDS = ("uniform1", "uniform5", "uniform8",                         # depth 0
          "uniform9", "uniform17", "uniform33", "uniform128",         # depth 2
          "uniform139", "uniform519",                                 # 8 * 17 + 3, 8 * 65 - 1: padding nodes, a partly padded last leaf
          "uniform300", "uniform640", "uniform1003",                  # last-level nodes inside the seed range; a partly padded last leaf
          "shells", "shells_eps0", "far")


class Case:
    def __init__(self, pkg, oracle, kind):
        self.kind = kind
        self.pts, self.eps = _make(pkg, kind)
        self.ix = pkg.Index(self.pts)
        self.oracle = oracle
        self._self = None
        n = len(self.pts)
        rng = np.random.default_rng(n)
        near = self.pts[rng.integers(0, n, 150)] + rng.normal(0, 1e-3, (150, 3)).astype(np.float32)
        lo, hi = self.pts.min(0), self.pts.max(0)
        anywhere = (lo - 0.3 * (hi - lo + 1) + rng.random((150 + 37, 3)) * 1.6 * (hi - lo + 1)).astype(np.float32)
        self.queries = np.concatenate([near, anywhere, self.pts[: min(n, 64)]]).astype(np.float32)  # (not a multiple of 64)
        self._batch = None

    def brute_self(self):
        if self._self is None:
            self._self = self.oracle.knn_bruteforce(self.pts, self.pts, KMAX, eps=self.eps, nthreads=16, want_d2=True)
        return self._self

    def brute_batch(self):
        if self._batch is None:
            self._batch = self.oracle.knn_bruteforce(self.pts, self.queries, KMAX, eps=self.eps, nthreads=16, want_d2=True)
        return self._batch


def check_rows(pts, queries, got, brute, k, what):
    gi, gc, gd = got
    bi, bc, bd = brute
    ei, ec, ed = bi[:, :k], np.minimum(bc, k), bd[:, :k]
    assert np.array_equal(gc, ec), what
    live = np.arange(k)[None, :] < ec[:, None]
    assert np.array_equal(gd.view(np.uint32)[live], ed.view(np.uint32)[live]), what
    r, c = np.nonzero((gi != ei) & live)
    if len(r):  # only among points exactly as far as the row's k-th, and each such point really is that far
        assert (ed[r, c] == ed[r, ec[r] - 1]).all(), what
        assert np.array_equal(_d2(pts[gi[r, c].astype(np.int64)], queries[r]).view(np.uint32), ed[r, c].view(np.uint32)), what
        s = np.sort(np.where(live, gi, np.arange(k, dtype=np.uint32) + np.uint32(0xFFFFFF00)), 1)
        assert (s[:, 1:] != s[:, :-1]).all(), what  # no point twice in a row


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


@pytest.mark.parametrize("kind", CLOUDS)
def test_self_rows_equal_brute_force_at_every_k(cases, kind):
    cs = cases(kind)
    for k in KS:
        check_rows(cs.pts, cs.pts, cs.ix.knn_self(k, cs.eps, want_d2=True), cs.brute_self(), k, (kind, "self", k))


@pytest.mark.parametrize("kind", CLOUDS)
def test_batch_rows_equal_brute_force_at_every_k(cases, kind):
    cs = cases(kind)
    for k in KS:
        check_rows(cs.pts, cs.queries, cs.ix.knn(cs.queries, k, cs.eps, want_d2=True), cs.brute_batch(), k, (kind, "batch", k))


@pytest.mark.parametrize("kind", ["uniform1003", "shells"])
def test_a_slice_that_ends_inside_a_group(pkg, cases, kind):
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
        first, count = 64 * 3, 64 * 5 + 23  # ends 23 lanes into a group
        rows = np.zeros(n, bool)
        rows[perm[first:first + count]] = True
        for k in KS:
            idx = torch.full((n, k), -7, dtype=torch.int32, device=dev)
            cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
            d2 = torch.full((n, k), -7.0, dtype=torch.float32, device=dev)
            ix.knn_self_dev(k, cs.eps, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr(), first=first, count=count)
            ix.synchronize()
            gi, gc, gd = idx.cpu().numpy(), cnt.cpu().numpy(), d2.cpu().numpy()
            assert (gc[~rows] == -7).all() and (gi[~rows] == -7).all() and (gd[~rows] == -7).all(), (kind, k)
            bi, bc, bd = cs.brute_self()
            check_rows(cs.pts, cs.pts[rows], (gi[rows].view(np.uint32), gc[rows].view(np.uint32), gd[rows]), (bi[rows], bc[rows], bd[rows]), k, (kind, "slice", k))
    finally:
        ix.close()
