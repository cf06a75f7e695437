"""Every sphere walk on lattices, where points and leaf boxes lie exactly at r ("The rim"; the cases are in
tests/rim_cases.py, what they rest on in tests/test_rim_cpu.py).

Each fixed-radius operation walks the index with its own copy of the inside test sq3(dx, dy, dz) <= r2 and of the prune test
box_d2(b, q) <= r2.  On random float32 clouds d2 == r2 has a probability of about 1e-7 per pair, so a `<` for a `<=`, an r2 formed in
double, a need() that drops a leaf whose box lies at exactly r2 or a rule on distances would pass every other test.  Here between a
fifth and four fifths of the pairs inside lie at exactly r, and the reference is integer arithmetic on the lattice.

Every row runs on the three clouds and the four radii, on a fresh index.  What a row compares exactly it compares with the integer
rule and with the operation's own model; no tolerance is new: eigenvalues, centroids, FPFH and MLS rows go through the comparators
of the operations' own test files."""
import numpy as np
import pytest

import handle_history_cases as Cs
import keypoints_model as KM
import rim_cases as R

pytestmark = pytest.mark.gpu
F = np.float32
CASES = R.all_cases()
IDS = ["%s-%s" % c for c in CASES]
rim = pytest.mark.parametrize("cloud,rname", CASES, ids=IDS)


class _Ctx(Cs.Ctx):
    """what the _dev callers of tests/handle_history_cases.py take"""

    def __init__(self, pkg, ix, c):
        self.pkg, self.ix, self.cloud, self.I = pkg, ix, c.cloud, c.I
        self.n_in, self.n, self.r = c.n, c.n, c.r


def _fresh(pkg, c):
    ix = pkg.LinkedOctree(c.pts)
    assert ix.size() == c.n and ix.n_in == c.n
    return ix


def _exact(row, got, want, what):
    """the outputs a row compares bit for bit: every one the table names, and no other"""
    spec = R.ROWS[row]
    assert sorted(got) == sorted(spec.exact + spec.fixed), (what, sorted(got))
    for name, a in got.items():
        w = want[name]
        a = np.ascontiguousarray(a)
        a = a.astype(w.dtype) if a.dtype.kind in "bu" and w.dtype.kind in "bu" and a.dtype.itemsize <= w.dtype.itemsize else a
        if not R.same(a, w):
            assert a.shape == w.shape and a.dtype == w.dtype, (what, name, a.shape, w.shape, a.dtype, w.dtype)
            bad = np.flatnonzero((Cs.bits(a) != Cs.bits(w)).reshape(len(w), -1).any(1))
            raise AssertionError((what, name, len(bad), bad[:8].tolist(), a[bad[:8]].tolist(), w[bad[:8]].tolist()))


# ---- counts, lists, radius outliers --------------------------------------------------------------------------------------------------------
@rim
def test_counts(pkg, cloud, rname):
    import outliers_model as OM
    c = R.case(cloud, rname)
    want = R.ROWS["counts"].model(c, "contract")
    ix = _fresh(pkg, c)
    got = {"self": ix.range_count_self(c.r), "absent": ix.range_count(R.at(cloud, R.absent(cloud)), c.r)}
    dev = Cs.ROWS["count_self_dev"][1](_Ctx(pkg, ix, c))  # range_count_self_dev and range_count_self_curve_order_dev
    assert np.array_equal(dev["cnt"], want["self"]), (c, "range_count_self_dev")
    assert np.array_equal(np.sort(dev["perm"]), np.arange(c.n)) and np.array_equal(dev["cnt_by_position"], want["self"][dev["perm"].astype(np.int64)]), c
    for name, at_least in zip(("keep_interior", "keep_median"), R.outlier_bounds(c)):
        kept, keep, cnt = ix.radius_outliers(c.r, at_least, want_keep=True, want_counts=True)
        kept0, keep0 = ix.radius_outliers(c.r, at_least, want_keep=True)  # (no counts: the at-least form, a walk that stops at the bound)
        mkeep, mcnt = OM.radius(c.pts, None, c.r, at_least)
        assert np.array_equal(cnt, want["self"]) and np.array_equal(cnt, mcnt) and np.array_equal(mkeep, want[name]), (c, name)
        assert np.array_equal(keep0, want[name]), (c, name, "at-least form", at_least, np.flatnonzero(keep0 != want[name])[:8].tolist())
        assert np.array_equal(kept, np.flatnonzero(want[name])) and np.array_equal(kept0, kept), (c, name)
        got[name] = keep
    assert want["keep_median"].any() and not want["keep_median"].all()
    _exact("counts", got, want, c)
    ix.close()


@rim
def test_lists(pkg, cloud, rname):
    c = R.case(cloud, rname)
    want = R.ROWS["lists"].model(c, "contract")
    ix = _fresh(pkg, c)
    ctx = _Ctx(pkg, ix, c)
    dev = Cs.ROWS["lists_self_dev"][1](ctx)
    pos = ctx.out(c.n, "u32")
    ctx.ready()
    ix.perm_dev(None, pos.data_ptr())
    ctx.drain()
    position_of = ctx.down(pos, c.n).astype(np.int64)
    off = dev["offsets"].astype(np.int64)
    for i in range(c.n):  # each list in tree order (include/pcpx.h): walk order, then point order inside a leaf
        at = position_of[dev["idx"][off[i]:off[i + 1]].astype(np.int64)]
        assert (np.diff(at) > 0).all(), (c, i, at.tolist())
    boff, bidx = ix.range_sphere(c.I["centres"], R.mixed_radii(cloud, rname))
    got = {"offsets": dev["offsets"], "idx": R.sorted_lists(dev["offsets"], dev["idx"]), "batch_offsets": boff, "batch_idx": R.sorted_lists(boff, bidx)}
    _exact("lists", got, want, c)
    ix.close()


# ---- neighbourhoods and shape features -------------------------------------------------------------------------------------------------------
def _moments_check(oracle, c, centres, radii, sets, nrm, cen, md, cnt, label):
    """the comparator of the operation's own file; far from the origin that of tests/test_gpu_far_clouds.py"""
    if c.cloud.endswith("far"):
        import test_gpu_far_clouds as TFar
        TFar._moment_rows(oracle, c.pts, centres, radii, sets, nrm, cen, md, cnt, label)
    else:
        import test_gpu_range_neighbourhoods as TRn
        TRn._check_rows(oracle, c.pts, centres, radii, sets, nrm, cen, md, cnt, float(np.ptp(c.pts, 0).max()), label)


@rim
def test_range_neighbourhoods(pkg, oracle, cloud, rname):
    c = R.case(cloud, rname)
    want = R.ROWS["neighbourhoods"].model(c, "contract")
    ix = _fresh(pkg, c)
    nrm, cen, md, cnt = ix.range_neighbourhoods_self(c.r, normals=True, centroids=True, mean_dist=True, counts=True)
    radii = R.mixed_radii(cloud, rname)
    bn, bc, bm, bk = ix.range_neighbourhoods(c.I["centres"], radii, normals=True, centroids=True, mean_dist=True, counts=True)
    _exact("neighbourhoods", {"counts_self": cnt, "counts_batch": bk}, want, c)
    _moments_check(oracle, c, c.pts, np.full(c.n, c.r, F), c.sets(), nrm, cen, md, cnt, "%r self" % c)
    _moments_check(oracle, c, c.I["centres"], radii, c.batch_sets(), bn, bc, bm, bk, "%r batch" % c)
    ix.close()


@rim
def test_shape_features(pkg, cloud, rname):
    import test_gpu_shape_features as TSf
    c = R.case(cloud, rname)
    want = R.ROWS["features"].model(c, "contract")
    ix = _fresh(pkg, c)
    ev, sv, nrm, ax, cnt = ix.shape_features_self(c.r, normals=True, axes=True, counts=True)
    radii = R.mixed_radii(cloud, rname)
    bev, bsv, bnrm, bax, bcnt = ix.shape_features(c.I["centres"], radii, normals=True, axes=True, counts=True)
    _exact("features", {"counts_self": cnt, "counts_batch": bcnt}, want, c)
    snrm = ix.range_neighbourhoods_self(c.r, normals=True)
    bsnrm = ix.range_neighbourhoods(c.I["centres"], radii, normals=True)
    assert np.array_equal(TSf._bits(nrm), TSf._bits(snrm)) and np.array_equal(TSf._bits(bnrm), TSf._bits(bsnrm)), c
    TSf._check_rows(c.pts, c.pts, c.sets(), ev, sv, ax, cnt, "%r self" % c, True)
    TSf._check_rows(c.pts, c.I["centres"], c.batch_sets(), bev, bsv, bax, bcnt, "%r batch" % c, False)
    ix.close()


# ---- cluster, segment, subsample -----------------------------------------------------------------------------------------------------------
@rim
def test_cluster(pkg, cloud, rname):
    c = R.case(cloud, rname)
    want = R.ROWS["cluster"].model(c, "contract")
    ix = _fresh(pkg, c)
    for form in ("host", "dev"):
        got = {}
        for name, compact in R.CLUSTER_FORMS:
            min_pts = R.cluster_min_pts(name, rname)
            if form == "host":
                lab, count, core, counts = ix.cluster(c.r, min_pts, compact, want_core=True, want_counts=True)
                count = np.array([count], np.uint64)
            else:
                d = Cs._cluster_dev(_Ctx(pkg, ix, c), min_pts, compact)
                lab, count, core, counts = d["labels"], d["count"], d["core"], d["counts"]
            tag = R.cluster_tag(name, compact)
            got["labels" + tag], got["count" + tag] = lab, count
            if name != "m1":
                got["core" + tag] = np.asarray(core).astype(np.uint8)
            else:
                assert np.asarray(core).all(), (c, form, tag)  # (a sphere holds its centre)
            assert np.array_equal(counts, want["counts"]), (c, form, tag)
        got["counts"] = counts
        _exact("cluster", got, want, (c, form))
    ix.close()


@rim
def test_segment(pkg, cloud, rname):
    c = R.case(cloud, rname)
    want = R.ROWS["segment"].model(c, "contract")
    ix = _fresh(pkg, c)
    lab, count, smooth = ix.segment(c.I["normals"], c.r, min_cos=R.MIN_COS[rname], want_smooth=True)
    assert smooth.all()
    glab, gcount, gsmooth = ix.segment(c.I["normals"], c.r, min_cos=R.MIN_COS[rname], curvature=c.I["curvature"], max_curvature=R.MAX_CURVATURE,
                                       min_size=R.MIN_SIZE, want_smooth=True)  # (not every point smooth: k_segment_border runs)
    assert 0 < gsmooth.sum() < c.n and (glab[~gsmooth.astype(bool)] != R.NONE).any()
    _exact("segment", {"labels": lab, "count": np.array([count], np.uint64), "gated_labels": glab, "gated_count": np.array([gcount], np.uint64),
                       "gated_smooth": gsmooth.astype(np.uint8)}, want, c)
    ix.close()


@rim
def test_subsample(pkg, cloud, rname):
    c = R.case(cloud, rname)
    want = R.ROWS["subsample"].model(c, "contract")
    ix = _fresh(pkg, c)
    kept, keep, owner = ix.subsample(c.r, R.SUBSAMPLE_SEED, want_keep=True, want_owner=True)
    keep = keep.astype(bool)
    assert np.array_equal(kept, np.flatnonzero(keep))
    d = R.d2_int(c.g, c.g[keep])  # by integers: no two kept rows within the bound, every dropped row within it of a kept one
    assert ((d[keep] <= c.bound()).sum(1) == 1).all() and (d[~keep] <= c.bound()).any(1).all(), c
    assert (d[np.arange(c.n), np.searchsorted(kept, owner)] <= c.bound()).all() and keep[owner.astype(np.int64)].all(), c
    _exact("subsample", {"keep": keep.astype(np.uint8), "owner": owner}, want, c)
    ix.close()


# ---- keypoints, descriptors ----------------------------------------------------------------------------------------------------------------
@rim
def test_local_maxima(pkg, cloud, rname):
    c = R.case(cloud, rname)
    want = R.ROWS["local_maxima"].model(c, "contract")
    ix = _fresh(pkg, c)
    kept, keep = ix.local_maxima(c.I["score"], c.r, min_score=R.MIN_SCORE, min_neighbours=R.MAXIMA_MIN_NEIGHBOURS, want_keep=True)
    assert np.array_equal(kept, np.flatnonzero(keep)) and 0 < len(kept) < c.n
    _exact("local_maxima", {"keep": keep.astype(np.uint8)}, want, c)
    ix.close()


@rim
def test_iss_keypoints(pkg, cloud, rname):
    """as tests/test_gpu_keypoints.py::test_iss_exact_layer: the saliency is the model's float32 arithmetic on the eigenvalues and
    counts of shape_features_self at the salient radius, the kept set the model's maxima of it over the integer edges"""
    c = R.case(cloud, rname)
    salient, non_max = R.iss_radii(c)
    ix = _fresh(pkg, c)
    evals, cnt = ix.shape_features_self(salient, evals=True, curvature=False, counts=True)
    assert np.array_equal(cnt, R.case(cloud, R.ISS_SALIENT[rname]).counts()), c
    kept, keep, sal = ix.iss_keypoints(salient, non_max, R.ISS_GAMMA, R.ISS_GAMMA, R.ISS_MIN_NEIGHBOURS, want_saliency=True, want_keep=True)
    want_sal = KM.iss_score(evals, cnt, R.ISS_GAMMA, R.ISS_GAMMA)
    nan = np.isnan(want_sal)
    assert np.array_equal(np.isnan(sal), nan) and np.array_equal(Cs.bits(sal[~nan]), Cs.bits(want_sal[~nan])) and 0 < (~nan).sum(), c
    want = KM.local_maxima_cloud(c.pts, sal, non_max, min_neighbours=R.ISS_MIN_NEIGHBOURS, edges=c.edges())
    assert np.array_equal(keep, want) and np.array_equal(kept, np.flatnonzero(want)), (c, np.flatnonzero(keep != want)[:8].tolist())
    ix.close()


@rim
def test_fpfh(pkg, cloud, rname):
    import test_gpu_fpfh as TFp
    c = R.case(cloud, rname)
    want = R.fpfh_rows(c)
    ix = _fresh(pkg, c)
    inside = np.ones(c.n, bool)
    fpfh, spfh, pairs = ix.fpfh(c.I["normals"], c.r, want_spfh=True)
    assert np.array_equal(pairs, want["pairs"]), (c, np.flatnonzero(pairs != want["pairs"])[:8].tolist())
    assert np.array_equal(Cs.bits(spfh), Cs.bits(want["spfh"])), c
    worst = TFp._check_fpfh_rows(c.pts, inside, c.r, np.arange(c.n), fpfh, spfh, "%r all" % c)
    rows = c.I["rows"]
    sub, sub_spfh, sub_pairs = ix.fpfh(c.I["normals"], c.r, rows=rows, want_spfh=True)
    at = rows.astype(np.int64)
    _exact("fpfh", {"spfh": sub_spfh[at], "pairs": sub_pairs[at]}, R.ROWS["fpfh"].model(c, "contract"), (c, "subset"))
    worst = max(worst, TFp._check_fpfh_rows(c.pts, inside, c.r, at, sub, spfh, "%r subset" % c))
    print("%r: worst |fpfh - F| / bound %.3f" % (c, worst))
    ix.close()


# ---- registration, MLS, boundary -------------------------------------------------------------------------------------------------------------
@rim
def test_nearest_posed(pkg, cloud, rname):
    c = R.case(cloud, rname)
    want = R.ROWS["nearest_posed"].model(c, "contract")  # (the integers, and icp_model: ties to the lowest index)
    ix = _fresh(pkg, c)
    got = {}
    for name, pose in R.POSES.items():
        got["partner_" + name], got["d2_" + name] = ix.nearest_posed(c.I["source"], c.r, pose, want_d2=True)
        at_bound = want["d2_" + name] == F(c.bound() * R.S * R.S)  # (partners at exactly the bound, and sources with none)
        assert at_bound.sum() >= 8 and (want["partner_" + name] == R.NONE).sum() >= 8, (c, name)
    _exact("nearest_posed", got, want, c)
    ix.close()


@rim
def test_mls_project_self(pkg, cloud, rname):
    """counts exact on every row; the fit words exact and the rest within the bounds of tests/test_gpu_mls.py on every row whose
    normal the contract defines (rim_cases.mls_tie: a symmetric lattice neighbourhood has none, and the quadric's fit follows it)"""
    import test_gpu_mls as TM
    c = R.case(cloud, rname)
    model = R.mls_rows(c)
    tie = np.array([R.mls_tie(m) for m in model])
    rows = np.flatnonzero(~tie)
    assert len(rows) >= (0.9 if cloud != "full9" else 0.25) * c.n
    ix = _fresh(pkg, c)
    for order in (1, 2):
        got = ix.mls_project_self(c.r, R.GAUSS_H, order, **TM.ALL)
        cnt, fit = got[4], got[5]
        assert np.array_equal(cnt, c.counts()), (c, order)
        want_fit = np.array([min(m.fit, order) for m in model], np.uint32)
        assert np.array_equal(fit[rows], want_fit[rows]), (c, order, rows[fit[rows] != want_fit[rows]][:8].tolist())
        assert ((fit[tie] >= 1) & (fit[tie] <= order)).all() and all(np.isfinite(a[tie]).all() for a in got[:3]), (c, order)
        TM._check(c.pts, c.pts[rows], [a[rows] for a in got], [model[i] for i in rows], c.r, order, "%r" % c)
    ix.close()


@rim
def test_boundary(pkg, cloud, rname):
    import test_gpu_boundary as TB
    c = R.case(cloud, rname)
    want = R.ROWS["boundary"].model(c, "contract")
    ix = _fresh(pkg, c)
    got = {}
    for which in R.BOUNDARY_NORMALS:
        out = TB.check(ix, c.pts, c.I[which], c.r, what="%r %s" % (c, which))  # (boundary_model, bit for bit)
        assert np.array_equal(out[2], c.counts()), (c, which)
        got.update({"%s_%s" % (name, which): a for name, a in zip(R.BOUNDARY_NAMES, out)})
    _exact("boundary", got, want, c)
    ix.close()


# ---- farthest points -----------------------------------------------------------------------------------------------------------------------
def test_farthest_points_stop_at_exactly_the_stop_radius(pkg):
    """full9, stop_radius 2 S: the selection goes on while D > 4 S^2 and ends with points at D == 4 S^2 left (tests/test_rim_cpu.py)"""
    import test_gpu_fps as TF
    pts, m, want = R.fps_case()
    ix = pkg.Index(pts)
    got = TF.check_all(ix, want, m, start=R.FPS_START, stop_radius=R.FPS_STOP, switches=TF.FEWER, what="rim")
    assert len(got["rows"]) == want.count < m and got["min_d2"].max() == F(R.FPS_STOP) * F(R.FPS_STOP)
    ix.close()
