"""The eigen-solver of the normals (csrc/pcpx_eig3.h) is shaped for a wave: its lanes no longer branch apart, and the float
operations each lane keeps are those of the branching form (tests/test_eig3_cpu.py compares the two on the host).  Here the
kernels that compile it are compared with each other and with the CPU oracle, bit for bit:

* the fused normals of the kNN kernel, k = 3, 8, 15, 16, 32, on free, planar, collinear, coincident and lattice clouds of 16 ... 3 000
  points, one cloud at 1e6 and one of 1e-6 (at eps = 0: a row leaves out what lies within eps of its point, the point itself
  included, and at the default eps that is this whole cloud), 20 places of five coincident points each, 100 points in one place
  (every row is empty) and a cloud of 16 points (every row of k = 16 and 32 has fewer than k neighbours), against the
  oracle's normals over the same rows (pcp::estimate_normal per row), against estimate_normal on single rows, and against
  normals_from_knn (k_normals) over the rows handed back;
* the radius normals and the shape features (the moments form, C = Q - S S^T / n about the query) against the fused normals and
  the eigenvalues of normals_from_knn.  The two forms round differently in general, so this takes rows where they form the same
  matrix exactly: interior points of a sheared integer lattice, whose shells are symmetric about them (S = 0, the mean is the
  point itself, every product and sum an exact small integer), with the radius between two shells and k the number of other
  points inside (the sphere holds the point itself, the row does not: it adds nothing to either matrix).  The shear makes the
  matrices full, so the solver rotates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
KS = (3, 8, 15, 16, 32)


def _bits_equal(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _clouds():
    rng = np.random.default_rng(20260117)
    free = rng.uniform(-1, 1, (3000, 3)).astype(F)
    uv = rng.uniform(-1, 1, (2000, 2)).astype(F)
    planar = np.stack([uv[:, 0], uv[:, 1], F(0.3) * uv[:, 0] - F(0.2) * uv[:, 1] + F(0.1)], 1).astype(F)
    t = rng.uniform(-1, 1, (500, 1)).astype(F)
    collinear = (t * np.array([[0.6, -0.3, 0.74]], F) + np.array([[0.1, 0.2, -0.3]], F)).astype(F)
    coincident = np.repeat(free[:20], 5, 0)
    one_place = np.tile(np.array([[0.25, -0.5, 0.125]], F), (100, 1))
    g = np.arange(12, dtype=F)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    return {"free": free, "planar": planar, "collinear": collinear, "coincident": coincident, "one_place": one_place, "lattice": lattice,
            "at_1e6": (free[:1000] * F(1e6)).astype(F), "of_1e-6": (free[1000:2000] * F(1e-6)).astype(F), "sixteen": free[:16].copy()}


CLOUDS = _clouds()
EPS = {"of_1e-6": 0.0}
EXPECTED_COUNT = {"one_place": lambda k: 0, "sixteen": lambda k: min(k, 15)}  # (a row never holds its own point)
_indices = {}


def _index(pkg, name):
    if name not in _indices:
        _indices[name] = pkg.LinkedOctree(CLOUDS[name])
    return _indices[name]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_fused_normals_equal_the_oracle_and_k_normals_bit_for_bit(pkg, oracle, name, k):
    pts = CLOUDS[name]
    ix = _index(pkg, name)
    nrm, idx, cnt = ix.normals_knn_self(k, EPS.get(name, 1e-5), want_knn=True)
    assert (cnt == EXPECTED_COUNT.get(name, lambda k: k)(k)).all()
    want = oracle.normals_from_knn(pts, idx, cnt, nthreads=16)
    differ = ~_bits_equal(nrm, want).all(1)
    print("%s k=%d: %d rows, %d differ from the oracle" % (name, k, len(pts), int(differ.sum())))
    assert not differ.any(), (name, k, np.nonzero(differ)[0][:5], nrm[differ][:5], want[differ][:5])
    for r in range(0, len(pts), max(1, len(pts) // 25)):
        one = oracle.estimate_normal(pts[idx[r, : cnt[r]].astype(np.int64)])
        assert _bits_equal(nrm[r], one).all(), (name, k, r)
    again, ev = ix.normals_from_knn(idx, cnt, want_evals=True)
    assert _bits_equal(again, nrm).all(), (name, k)
    _, oev = oracle.normals_from_knn(pts, idx, cnt, nthreads=16, want_evals=True)
    assert _bits_equal(ev, oev).all(), (name, k)


def _sheared_lattice():
    basis = np.array([[2, 1, 0], [0, 2, 1], [1, 0, 3]], np.int64)
    g = np.arange(9)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return (ijk @ basis).astype(F), ijk


def _shells(pts, centre):
    """(squared radius between this shell and the next, points inside, the centre among them) for the centre's neighbourhood,
    nearest shells first."""
    d2 = np.sort(((pts.astype(np.int64) - pts[centre].astype(np.int64)) ** 2).sum(1))
    out = []
    for i in range(1, 34):  # (up to 33 points inside: k <= 32)
        if d2[i] > d2[i - 1]:
            out.append((0.5 * (float(d2[i]) + float(d2[i - 1])), i))
    return out


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -10])
def test_radius_normals_and_shape_features_equal_the_fused_normals_where_both_forms_are_exact(pkg, scale):
    ints, ijk = _sheared_lattice()
    pts = (ints * F(scale)).astype(F)
    centre = int(np.nonzero((ijk == 4).all(1))[0][0])
    ix = pkg.LinkedOctree(pts)
    checked = 0
    for r2, inside in _shells(ints, centre):
        k = inside - 1  # the row leaves the point itself out
        if k < 3:
            continue
        radius = float(np.sqrt(r2)) * scale
        rn, rc = ix.range_neighbourhoods_self(radius, normals=True, counts=True)
        fe, fnrm, fc = ix.shape_features_self(radius, evals=True, curvature=False, normals=True, counts=True)
        nrm, idx, cnt = ix.normals_knn_self(k, want_knn=True)
        _, ev = ix.normals_from_knn(idx, cnt, want_evals=True)
        # rows whose sphere holds exactly the kNN row, symmetric about the point
        nb = ints[idx.astype(np.int64)].astype(np.int64) - ints[:, None, :].astype(np.int64)
        rows = (rc == inside) & (cnt == k) & ((nb ** 2).sum(2).max(1) < r2) & (nb.sum(1) == 0).all(1)
        assert rows[centre] and np.array_equal(rc, fc)
        assert _bits_equal(fnrm, rn).all()
        assert _bits_equal(rn[rows], nrm[rows]).all(), (scale, k)
        assert _bits_equal(fe[rows], ev[rows]).all(), (scale, k)
        off_diagonal = np.stack([(nb[rows][:, :, a] * nb[rows][:, :, b]).sum(1) for a, b in ((0, 1), (1, 2), (0, 2))], 1)
        assert (off_diagonal != 0).any(1).all()  # not a diagonal matrix: the solver has rotations to do
        print("scale %g k=%d: %d rows" % (scale, k, int(rows.sum())))
        checked += int(rows.sum())
    ix.close()
    assert checked >= 100
