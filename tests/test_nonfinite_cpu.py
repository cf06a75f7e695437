"""CPU tests of the non-finite cases (tests/nonfinite_cases.py; DESIGN.md section 10, "Non-finite coordinates"): what the generators
promise, and the yardsticks of tests/test_gpu_nonfinite.py against a real build of the reference where the reference defines
anything --

  * a cloud with NaN coordinates: the reference's octree leaves those rows out, and its kNN, sphere and box results are brute force
    over the finite rows (the contract's rule 1 is the reference's there);
  * a cloud with an infinite coordinate: the reference stops on an assertion, in a child process (rule 1 is this project's there);
  * queries: the reference returns k arbitrary points for a NaN query (its answer depends on the shape of its tree), so nothing is
    compared; for an infinite one it returns k points, as the IEEE rule says;
  * surface nets: the numpy model against the reference on fields with NaN, +inf and -inf corners, and the recording
    tests/golden/ref_nonfinite.npz, which the GPU tests read, against both.

The sign of a NaN that arithmetic makes (inf - inf, 0 x inf) is the hardware's choice -- x86 makes a negative one, gfx950 a positive
one -- so vertices are compared bit for bit where they are numbers and NaN for NaN where they are not (`same_vertices`)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nonfinite_cases as N
import surface_nets_model as M
from conftest import GOLDEN, ROOT, knn_rows_equivalent
from oracle import pcp_ref as R

F = np.float32
NT = min(16, os.cpu_count() or 1)
needs_reference = pytest.mark.skipif(not R.available(), reason="no build of the reference: %s" % R.why_unavailable())


def same_vertices(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def by_first_vertex(t):
    """tests/test_reference_build.py: the reference walks its cubes in hash-map order"""
    return t[np.argsort(t[:, 0], kind="stable")] if len(t) else t


# ---- the generators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", N.all_clouds(), ids=["%s_%d" % c for c in N.all_clouds()])
def test_clouds_are_what_they_say(kind, n):
    pts, finite = N.cloud(kind, n)
    assert pts.dtype == F and pts.shape == (n, 3) and np.array_equal(finite, np.isfinite(pts).all(1))
    bad = np.nonzero(~finite)[0]
    if kind in N.KINDS:
        assert len(bad) == N.bad_count(n) and 0 in bad and n - 1 in bad and (n != 1300 or len(bad) == 40)
        assert np.array_equal(pts[finite], N.base(n)[finite])  # (the finite rows are the base cloud's)
        nan, inf = np.isnan(pts[bad]), np.isinf(pts[bad])
        if kind in ("nan_rows", "odd_nans"):
            assert (nan.sum(1) == 1).all() and not inf.any()
        elif kind == "inf_rows":
            assert (inf.sum(1) == 1).all() and not nan.any() and (pts[bad] == np.inf).any() and (pts[bad] == -np.inf).any()
        else:
            assert nan.all(1).sum() == 1 and any(np.array_equal(r, [np.inf, -np.inf, np.nan], equal_nan=True) for r in pts[bad])
            assert nan.any() and (pts[bad] == np.inf).any() and (pts[bad] == -np.inf).any()
        if kind == "odd_nans":
            bits = pts.view(np.uint32)[np.isnan(pts)]
            assert set(bits.tolist()) == set(N.ODD_NANS) if n > 9 else set(bits.tolist()) <= set(N.ODD_NANS)
    elif kind in N.SURVIVORS:
        s = int(finite.sum())
        assert s == N.SURVIVORS[kind] and {"mod64": s % 64 == 0, "mod8": s % 8 == 0 and s % 64 != 0, "mod8_plus1": s % 8 == 1}[kind]
    elif kind == "one_finite":
        assert n == 65 and np.nonzero(finite)[0].tolist() == [N.ONE_FINITE_ROW]
    elif kind == "none_finite":
        assert not finite.any() and np.isnan(pts).any() and np.isinf(pts).any()
    else:
        assert (pts[:, 0] == np.inf).all() and np.isfinite(pts[:, 1:]).all() and not finite.any()
    box = N.finite_box(pts, finite)
    assert np.isfinite(box).all() and (finite.any() == bool((box[:3] <= box[3:]).all()))
    if finite.any():
        tw, grid = N.twin(pts, finite)
        assert np.isfinite(tw).all() and np.array_equal(((tw >= grid[:3]) & (tw <= grid[3:])).all(1), finite)


def test_the_base_cloud_has_the_shape_the_cases_count_on():
    import handle_history_cases as Cs
    s = Cs.statistics("c1300")
    assert (s["n"], s["leaf_slots"] // Cs.LEAF, s["groups"]) == (1300, 163, 21)
    assert np.isfinite(N.base(1300)).all() and np.isfinite(N.base(70)).all() and N.base(9).shape == (9, 3)


@pytest.mark.parametrize("name", N.QUERY_SETS)
def test_query_sets_are_what_they_say(name):
    q = N.queries(name)
    nan, inf = N.kinds_of(q)
    bad = nan | inf
    if name == "all_bad":
        assert len(q) == 64 and bad.all() and nan.sum() >= 16 and inf.sum() >= 16
        bits = set(q.view(np.uint32)[np.isnan(q)].tolist())
        assert set(N.ODD_NANS) <= bits and 0x7FC00000 in bits
    elif name in ("first", "last", "middle"):
        at = {"first": [0, 1], "last": [63], "middle": [31]}[name]
        assert len(q) == 64 and np.nonzero(bad)[0].tolist() == at and nan[at[0]]
    elif name == "many":
        assert len(q) == 600 > 512 and np.array_equal(np.nonzero(bad)[0], np.arange(0, 600, 7)) and nan.any() and inf.any()
    else:
        assert len(q) == 1 and bad.all() and (name == "one_inf") == bool(inf[0])
        assert name != "one_odd" or q.view(np.uint32)[0, 0] == N.ODD_NANS[0]


def test_spheres_boxes_and_fields_are_what_they_say():
    c, r = N.spheres()
    assert len(c) == len(r) == 96 and np.isnan(r).sum() == 16 and (r == -1).sum() == 16 and (r == 0).sum() == 16 and np.isposinf(r).sum() == 16
    assert not np.isfinite(c[4::5]).all(1).any() and np.isfinite(np.delete(c, np.arange(4, 96, 5), 0)).all()
    b = N.boxes()
    assert len(b) == 48 and np.isnan(b).any(1).sum() == 8 and (np.isneginf(b[:, :3]).all(1) & np.isposinf(b[:, 3:]).all(1)).sum() == 8
    pts = N.base(1300)
    every = np.ones(1300, bool)
    lists = N.box_lists(pts, every, b)
    assert all(len(l) == 0 for l, bb in zip(lists, b) if np.isnan(bb).any()) and sum(len(l) == 1300 for l in lists) == 8
    sl = N.sphere_lists(pts, every, c, r)
    ok = np.isfinite(c).all(1)
    assert all(len(l) == 0 for l, rr in zip(sl, r) if np.isnan(rr)) and all(len(l) == 1300 for l, rr, o in zip(sl, r, ok) if np.isinf(rr) and o)
    on_points = [i for i in range(20) if r[i] == 0 and ok[i]]  # (a centre on a point: radius 0 holds it)
    assert len(on_points) >= 2 and all(len(sl[i]) >= 1 for i in on_points) and any(1 < len(l) < 1300 for l in sl)
    for name in N.FIELDS:
        g, f = N.field(name)
        assert f.shape == ((g["sx"] + 1) * (g["sy"] + 1) * (g["sz"] + 1),) and f.dtype == F
        want = {"nan12": (40, 0, 0), "posinf12": (0, 40, 0), "neginf12": (0, 0, 40), "mixed12": (14, 13, 13), "mixed_33x20x41": (50, 50, 50),
                "all_nan": (f.size, 0, 0)}[name]
        assert (int(np.isnan(f).sum()), int(np.isposinf(f).sum()), int(np.isneginf(f).sum())) == want, name
    g, _ = N.field("mixed_33x20x41")
    assert (g["sx"], g["sy"], g["sz"]) == (33, 20, 41) and N.field("nan12")[0]["sx"] == 12


def test_kd_cases_are_what_they_say():
    for kind in ("nan_rows", "inf_rows", "odd_nans"):
        for dims in (3, 16, 33):
            pts, q, bx = N.kd_case(kind, dims)
            assert pts.shape == (700, dims) and q.shape == (40, dims) and bx.shape == (12, 2 * dims)
            assert (~np.isfinite(pts)).any(1).sum() == 40 and (~np.isfinite(q)).any(1).sum() == 8
            assert np.isnan(pts).any() == (kind != "inf_rows")


def test_kd_restatements_skip_a_nan_pair_and_keep_infinity(oracle):
    """the definition of rule 3 -- a pair whose distance is NaN is skipped, +inf is a value, ties in index order"""
    for kind in ("nan_rows", "inf_rows", "odd_nans"):
        pts, q, bx = N.kd_case(kind, 16)
        idx, cnt, d2 = oracle.kd_knn_bruteforce(pts, q, 15, 1e-5)[:3]
        bad_q = ~np.isfinite(q).all(1)
        assert not np.isnan(d2).any() and (cnt[np.isnan(q).any(1)] == 0).all() and (cnt[~bad_q] == 15).all()
        assert np.isposinf(d2[np.isinf(q).any(1) & ~np.isnan(q).any(1)]).all()
        lists = oracle.kd_range_aabb(pts, bx)
        assert len(lists[1]) == 0 and len(lists[2]) == int((~np.isnan(pts).any(1)).sum())


# ---- the oracle states the IEEE rule (it is the definition of rule 2 and is not changed) ---------------------------------------------
def test_the_oracle_states_the_ieee_rule(oracle):
    pts = N.base(1300)
    q = N.queries("all_bad")
    nan, inf = N.kinds_of(q)
    for k in (1, 15, 33):
        idx, cnt, d2 = oracle.knn_bruteforce(pts, q, k, 1e-5, nthreads=NT, want_d2=True)
        assert (cnt[nan] == 0).all() and (idx[nan] == N.NONE).all() and np.isposinf(d2[nan]).all()
        assert (cnt[inf] == k).all() and np.isposinf(d2[inf]).all() and all(len(set(r.tolist())) == k for r in idx[inf])
    assert (oracle.range_count_bruteforce(pts, q, 0.3, nthreads=NT) == 0).all()
    assert (oracle.range_count_bruteforce(pts, q[inf], np.inf, nthreads=NT) == 1300).all()
    assert (oracle.range_count_bruteforce(pts, pts[:5], np.nan, nthreads=NT) == 0).all()


# ---- NaN points: the reference ----------------------------------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("kind,n", [(k, n) for k in ("nan_rows", "odd_nans") for n in N.SIZES], ids=lambda v: str(v))
def test_reference_octree_leaves_nan_rows_out(oracle, kind, n):
    pts, finite = N.cloud(kind, n)
    t = R.Octree(pts)
    assert t.size() == int(finite.sum()) < n
    # pcp::bounding_box skips a NaN coordinate, not its row: the reference's grid is the box of the finite COORDINATES and holds the
    # finite rows' box, which is what an index of this project reports -- no query result depends on it
    grid, box = t.voxel_grid(), N.finite_box(pts, finite)
    assert np.array_equal(grid, np.concatenate([np.where(np.isnan(pts), F(np.inf), pts).min(0), np.where(np.isnan(pts), F(-np.inf), pts).max(0)])) and (grid[:3] <= box[:3]).all() and (grid[3:] >= box[3:]).all()
    q = np.ascontiguousarray(N.base(1300)[:200])
    for k in (1, 15, 33):
        for eps in (0.0, 1e-5):
            ri, rc = t.knn(q, k, eps)
            bi, bc, _ = N.knn_over_finite(oracle, pts, finite, q, k, eps, NT)
            ok, why = knn_rows_equivalent(pts, q, ri, rc, bi, bc)
            assert ok, (kind, n, k, eps, why)
            assert finite[ri[ri != N.NONE].astype(np.int64)].all()


@needs_reference
def test_reference_ranges_over_nan_rows_are_brute_force_over_the_finite_rows():
    pts, finite = N.cloud("nan_rows", 1300)
    t = R.Octree(pts)
    centres, radii = N.spheres()
    want = N.sphere_lists(pts, finite, centres, radii)
    quirk = 0
    for c, r, w in zip(centres, radii, want):
        if not np.isfinite(c).all():
            continue
        got = np.sort(t.range_sphere(c, r))
        if r < 0:  # (the reference prunes boxes against `radius` where it means radius^2, DESIGN.md 'Semantics': a subset)
            assert np.isin(got, w).all()
            quirk += len(w) - len(got)
        else:
            assert np.array_equal(got, w), (c, r)
    assert quirk > 0
    for b, w in zip(N.boxes(), N.box_lists(pts, finite, N.boxes())):
        assert np.array_equal(np.sort(t.range_aabb(b[:3], b[3:])), w), b


@needs_reference
def test_reference_answers_an_infinite_query_with_k_points_at_infinity():
    pts, finite = N.cloud("nan_rows", 1300)
    q = N.queries("all_bad")
    _nan, inf = N.kinds_of(q)
    idx, cnt = R.Octree(pts).knn(q[inf], 15, 1e-5)
    assert (cnt == 15).all() and finite[idx.astype(np.int64)].all() and all(len(set(r.tolist())) == 15 for r in idx)


@needs_reference
def test_reference_stops_on_a_cloud_with_an_infinite_coordinate():
    """In a child process: the insertion's assertion (linked_octree_node.hpp:89) ends it.  Nothing defines this case but this project's
    own rule: such a row is never indexed."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import nonfinite_cases as N\nfrom oracle import pcp_ref as R\n"
            "print(R.Octree(N.cloud('inf_rows', 1300)[0]).size())\n") % (ROOT, os.path.join(ROOT, "tests"))
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert done.returncode in (-6, 134), (done.returncode, done.stdout, done.stderr[-400:])
    assert "Assertion" in done.stderr or "assert" in done.stderr.lower(), done.stderr[-400:]


# ---- surface nets: the model, the reference, the recording -------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("name", N.FIELDS)
def test_surface_nets_model_against_reference_on_non_finite_fields(name):
    g, f = N.field(name)
    mv, mt = M.surface_nets(f, g, 0.0)
    rv, rt = R.surface_nets(f, g, 0.0)
    assert same_vertices(rv, mv), name
    assert np.array_equal(by_first_vertex(rt), mt), name
    if name == "all_nan":
        assert len(mv) == 0 and len(mt) == 0
    else:
        assert np.isnan(mv).any() and len(mt) > 500


@pytest.fixture(scope="module")
def recording():
    return np.load(os.path.join(GOLDEN, "ref_nonfinite.npz"))


def _sha(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def test_the_recording_is_of_these_inputs_and_agrees_with_the_models(oracle, recording):
    """without the reference: the recorded inputs are the generators', the recorded outputs what the yardsticks of the GPU tests give"""
    q = np.ascontiguousarray(N.base(1300)[:200])
    centres, radii = N.spheres()
    ok = np.isfinite(centres).all(1)
    listed = ok & np.isfinite(radii)
    assert np.array_equal(recording["sphere_rows"], np.nonzero(ok)[0]) and np.array_equal(recording["sphere_listed"], np.nonzero(listed)[0])
    for kind in ("nan_rows", "odd_nans"):
        pts, finite = N.cloud(kind, 1300)
        assert np.array_equal(recording[kind + "_sha"], _sha(pts)) and int(recording[kind + "_size"]) == int(finite.sum())
        bi, bc, _ = N.knn_over_finite(oracle, pts, finite, q, 15, 1e-5, NT)
        good, why = knn_rows_equivalent(pts, q, recording[kind + "_idx"], recording[kind + "_cnt"], bi, bc)
        assert good, why
        want = N.sphere_lists(pts, finite, centres, radii)
        got = N.lists_of(recording[kind + "_sphere_off"], recording[kind + "_sphere_idx"])
        for i, lst in zip(np.nonzero(listed)[0], got):
            assert np.array_equal(lst, want[i]) if radii[i] >= 0 else np.isin(lst, want[i]).all(), i
        for i, c in zip(np.nonzero(ok)[0], recording[kind + "_sphere_cnt"]):
            assert c == len(want[i]) or radii[i] < 0, i
        for lst, w in zip(N.lists_of(recording[kind + "_box_off"], recording[kind + "_box_idx"]), N.box_lists(pts, finite, N.boxes())):
            assert np.array_equal(lst, w)
    for name in N.FIELDS:
        g, f = N.field(name)
        assert np.array_equal(recording[name + "_sha"], _sha(f)), name
        mv, mt = M.surface_nets(f, g, 0.0)
        assert same_vertices(recording[name + "_v"], mv) and np.array_equal(by_first_vertex(recording[name + "_t"]), mt), name


@needs_reference
def test_the_recording_regenerates_byte_for_byte(tmp_path, recording):
    """tests/golden/make_reference_golden.py's nonfinite(), written elsewhere: the same bytes as the committed file"""
    sys.path.insert(0, GOLDEN)
    try:
        import make_reference_golden as G
    finally:
        sys.path.remove(GOLDEN)
    here = G.HERE
    G.HERE = str(tmp_path)
    try:
        size = G.nonfinite()
    finally:
        G.HERE = here
    with open(os.path.join(GOLDEN, "ref_nonfinite.npz"), "rb") as a, open(str(tmp_path / "ref_nonfinite.npz"), "rb") as b:
        assert a.read() == b.read()
    assert size <= G.MAX_FILE
