"""k_knn prunes nodes with a fused box bound against a slackened tau (csrc/pcpx_box_bound.h).  That may not change a row (nor may
any rearrangement of the leaf loop these clouds were also run against): every cloud here is checked, every row of it, against a numpy
brute force that forms d2 in float32 in the reference's association and orders by (d2, index) -- counts and the bits of d2
exactly, indices entry for entry except among points exactly as far as the k-th -- and the fused normals against the explicit-row
kernel (bits) and a float64 eigh (the 1e-4 cosine of tests/test_gpu_epilogue_once.py, whose checks these are).

* integer lattices scaled by 2^-3 (exact arithmetic) and by 0.1 (inexact), k = 8, 15, 16, 32: the three kernels in both sentinel
  forms, points on box faces and corners, exact ties everywhere -- a query's k-th neighbour sits ON the nearest corner of its box;
* a cloud offset by 1e4 with a spacing of 1e-2 (ten ulps of a coordinate), and one scaled by 1e-18, whose squared distances are
  subnormal or underflow (FLT_MIN is then all the slack there is);
* n = 1, 63, 65, 257: partly filled groups, trees made mostly of padding nodes, whose NaN poison enters as the FMA's addend;
* two dense clusters far apart and a few dozen isolated points: groups whose first walk round is capped and that go round again
  (the later rounds' shell, lane-per-query leaves after packed ones)."""
import numpy as np
import pytest

from conftest import normals_vs_float64_eigh
from test_gpu_epilogue_once import COS_TOL, _brute, _check_rows, _self_case

pytestmark = pytest.mark.gpu

_cache = {}


def _reference(name, pts, eps, kmax):
    """The brute-force rows of a cloud once, at the largest k asked of it: a smaller k's rows are their prefixes."""
    if name not in _cache:
        _cache[name] = _brute(pts, pts, kmax, eps)
    return _cache[name]


def _prefix(ref, k):
    i, c, d = ref
    return i[:, :k].copy(), np.minimum(c, k).astype(np.uint32), d[:, :k].copy()


def _lattice(scale):
    g = np.arange(12, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * np.float32(scale)
    return np.ascontiguousarray(pts[np.random.default_rng(12).permutation(len(pts))])


@pytest.mark.parametrize("k", [8, 15, 16, 32])
@pytest.mark.parametrize("scale", [0.125, 0.1])
def test_lattice_points_on_box_faces_and_corners(pkg, scale, k):
    pts = _lattice(scale)
    want = _prefix(_reference(("lattice", scale), pts, 1e-5, 32), k)
    gi, gc, _ = _self_case(pkg, pts, k, 1e-5, ("lattice", scale, k), want=want, eigh_rows=300)
    assert (gc == k).all()
    if scale == 0.125:  # (exact arithmetic: the lattice's ties are exact ties of d2 in every row)
        assert (want[2][:, 1:] == want[2][:, :-1]).any(1).all()


def test_cloud_far_from_the_origin(pkg, oracle):
    """Rows as everywhere.  Normals: a coordinate's float32 step here is a tenth of the spacing, and the reference's own float32
    arithmetic (the mean of the coordinates, the scatter matrix) is then far from a float64 eigh of the same rows -- measured on
    this cloud: 1 - |cos| up to 1.3e-1; the rows are what they were before the fused bound and the normal is a function of the row
    (tests/test_gpu_far_clouds.py prints that figure for its clouds and asserts nothing about it either).  So the 1e-4 cosine is
    asked against the reference's arithmetic restated on the host (oracle.normals_from_knn), and the bits against the explicit-row
    kernel on the returned rows."""
    rng = np.random.default_rng(41)
    pts = (np.float32(1e4) + rng.random((4096, 3), dtype=np.float32) * np.float32(0.16)).astype(np.float32)  # 16^3 cells of 1e-2
    ix = pkg.Index(pts)
    gi, gc, gd = ix.knn_self(15, 1e-5, want_d2=True)
    _check_rows(pts, pts, 15, (gi, gc, gd), _brute(pts, pts, 15, 1e-5), "offset 1e4")
    nrm, ni, nc = ix.normals_knn_self(15, 1e-5, want_knn=True)
    assert np.array_equal(ni, gi) and np.array_equal(nc, gc)
    assert np.array_equal(ix.normals_from_knn(gi, gc).view(np.uint32), nrm.view(np.uint32))
    ix.close()
    rows = np.nonzero(gc >= 3)[0]
    on = oracle.normals_from_knn(pts, gi[rows], gc[rows], nthreads=16)
    off = 1.0 - np.abs((nrm[rows].astype(np.float64) * on.astype(np.float64)).sum(1))
    worst, ill = normals_vs_float64_eigh(pts, gi[rows[::13]], gc[rows[::13]], nrm[rows[::13]])
    print("offset 1e4: max 1-|cos| vs the reference's float32 arithmetic %.2e over %d rows (bit-equal %.4f); vs float64 eigh %.2e"
          % (off.max(), len(rows), float((nrm[rows].view(np.uint32) == on.view(np.uint32)).all(1).mean()), worst))
    assert off.max() <= COS_TOL


def test_cloud_whose_squares_underflow(pkg):
    rng = np.random.default_rng(42)
    pts = rng.random((2048, 3), dtype=np.float32) * np.float32(1e-18)
    ix = pkg.Index(pts)  # (rows only: a scatter matrix of 1e-38s is no normal to check)
    gi, gc, gd = ix.knn_self(15, 0.0, want_d2=True)
    ix.close()
    want = _brute(pts, pts, 15, 0.0)
    assert (want[2][:, -1] < np.float32(1e-36)).all() and (want[2][:, 1] > 0).any()
    _check_rows(pts, pts, 15, (gi, gc, gd), want, "scale 1e-18")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("k", [8, 15, 32])
def test_partly_filled_groups_and_padding_nodes(pkg, n, k):
    pts = np.random.default_rng(n).random((n, 3), dtype=np.float32)
    gi, gc, _ = _self_case(pkg, pts, k, 1e-5, ("padding", n, k), want=_prefix(_reference(("padding", n), pts, 1e-5, 32), k))
    assert (gc == min(k, n - 1)).all()


@pytest.mark.parametrize("k", [8, 15, 32])
def test_clusters_far_apart_take_later_rounds(pkg, k):
    rng = np.random.default_rng(43)
    a = rng.normal(0.0, 1e-3, (1500, 3)) + np.array([0.1, 0.1, 0.1])
    b = rng.normal(0.0, 1e-3, (1450, 3)) + np.array([0.9, 0.8, 0.9])
    lone = rng.random((50, 3))
    pts = np.concatenate([a, b, lone]).astype(np.float32)
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    if k == 15:  # (the diagnostic build exists for this kernel) the case is about later rounds: some group does take one
        ix = pkg.Index(pts)
        stats = ix.debug_knn_stats(15, 1e-5)
        ix.close()
        print("later rounds: %d groups, %d lanes" % (stats["second_round_groups"], stats["lanes_in_later_rounds"]))
        assert stats["second_round_groups"] > 0 and stats["sparse_leaves"] > 0
    _self_case(pkg, pts, k, 1e-5, ("clusters", k), want=_prefix(_reference("clusters", pts, 1e-5, 32), k), eigh_rows=300)
