"""What tests/test_gpu_rim.py rests on, asserted on the CPU ("The rim"; the cases are in tests/rim_cases.py).

  1  The float32 models say what the integers say: cluster_model.brute_edges and the other models' sphere tests equal the integer
     rule on every cloud at every radius, and the table of radii is what rim_cases' header states.
  2  The rim is populated: the share of the pairs inside that lie at exactly r.
  3  So are the box edges: (centre, leaf) pairs whose tight leaf box is at exactly fl(r r) by the formula of box_d2 while the leaf
     holds a point inside the sphere -- a prune test that drops what lies AT r2 loses a neighbour there.
  4  Teeth: every row's model answers differently under every wrong rule that differs from the contract at the radius, on every
     cloud, and each output the GPU test compares exactly changes on at least one (cloud, radius).
  5  The farthest-point case ends at D == stop2 exactly."""
import numpy as np
import pytest

import build_model as BM
import cluster_model as CM
import fpfh_model as PM
import fps_model as FM
import mls_model as MM
import outliers_model as OM
import rim_cases as R
import shape_features_cases as SF

F = np.float32
SS = F(R.S * R.S)
CASES = R.all_cases()
IDS = ["%s-%s" % c for c in CASES]
RIM_SHARE = {"s": 0.75, "sqrt3_s": 0.25, "3s": 0.20}
BOX_EDGES = 100


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_of_radii():
    r = {name: R.radius(name) for name in R.RADII}
    assert all(v.dtype == F for v in r.values())
    assert r["s"] * r["s"] == SS and r["sqrt3_s"] * r["sqrt3_s"] == F(3) * SS and r["3s"] * r["3s"] == F(9) * SS
    assert F(1) * SS < r["sqrt2_s"] * r["sqrt2_s"] < F(2) * SS and np.sqrt(F(2) * SS) == r["sqrt2_s"]
    assert float(r["sqrt3_s"]) ** 2 < 3 * R.S * R.S  # (r^2 itself is below 3 s^2: only its float32 rounding reaches it)
    table = {name: tuple(R.bound(name, rule) for rule in R.RULES) for name in R.RADII}
    assert table == {"s": (1, 0, 1, 1), "sqrt2_s": (1, 1, 1, 2), "sqrt3_s": (3, 2, 2, 3), "3s": (9, 8, 9, 9)}, table
    for name in R.RADII:
        assert R.bound(name) == int(np.floor(float(r[name] * r[name]) / (R.S * R.S)))
        assert any(R.bound(name, rule) != R.bound(name) for rule in R.WRONG), name  # (every radius is separated by some wrong rule)
    for k, factor in R.EQUIVALENT.items():  # no lattice distance between an equivalent radius' square and its bound: every rule agrees
        assert all(R.bound(float(F(factor) * F(R.S)), rule) == k for rule in R.RULES), (k, factor)
    assert {R.bound(name, rule) for name in R.RADII for rule in R.WRONG if R.bound(name, rule) != R.bound(name)} == set(R.EQUIVALENT)
    assert [R.interior_count(k) for k in (1, 3, 9)] == [7, 27, 123]


@pytest.mark.parametrize("cloud", R.CLOUDS)
def test_the_clouds(cloud):
    g, pts = R.sites(cloud), R.points(cloud)
    assert len(g) == {"full9": 729, "thin12": R.THIN_KEPT, "thin12far": R.THIN_KEPT}[cloud] and pts.dtype == F
    assert len(np.unique(g, axis=0)) == len(g) and not np.array_equal(g, g[np.lexsort(g.T[::-1])])  # (distinct sites, rows permuted)
    both = np.concatenate([g, R.absent(cloud)])
    assert len(np.unique(both, axis=0)) == len(both)  # (an absent site holds no point)
    d = pts[:, None, :] - pts[None, :, :]  # every d, d2 and with it every box distance is exact in float32: the integers are the contract
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert np.array_equal(d2.astype(np.float64), R.d2_int(g, g) * (R.S * R.S))
    if cloud == "thin12far":
        assert np.array_equal(g, R.sites("thin12")) and np.array_equal(pts.astype(np.float64), R.points("thin12").astype(np.float64) + R.FAR_SHIFT)


@pytest.mark.parametrize("cloud,rname", CASES, ids=IDS)
def test_the_float32_models_equal_the_integer_rule(cloud, rname):
    c = R.case(cloud, rname)
    src, dst, cnt = c.edges()
    bs, bd, bc = CM.brute_edges(c.pts, c.r)
    order = np.lexsort((bd, bs))
    assert np.array_equal(bs[order], src) and np.array_equal(bd[order], dst) and np.array_equal(bc, cnt)
    assert np.array_equal(OM.range_count(c.pts, None, c.r), cnt)
    sets = c.sets()
    for i in range(0, c.n, 11):
        assert np.array_equal(SF.brute_set(c.pts, c.pts[i], c.r), sets[i]) and np.array_equal(MM.brute_set(c.pts, c.pts[i], c.r)[0], sets[i])
        assert np.array_equal(PM.sphere(c.pts, i, c.r)[0], sets[i][sets[i] != i])
    bsets, radii = c.batch_sets(), R.mixed_radii(cloud, rname)
    assert len(set(radii.tolist())) == 4
    for i in range(0, len(bsets), 11):
        assert np.array_equal(SF.brute_set(c.pts, c.I["centres"][i], radii[i]), bsets[i])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloud,rname", [c for c in CASES if c[1] in RIM_SHARE], ids=[i for i, c in zip(IDS, CASES) if c[1] in RIM_SHARE])
def test_rim_share(cloud, rname):
    share = R.rim_share(R.case(cloud, rname))
    print("%s %s: %.3f of the pairs inside are at exactly r" % (cloud, rname, share))
    assert share >= RIM_SHARE[rname]


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def box_edges(c):
    """the (centre, leaf) pairs with box_d2 == fl(r r) and a member of the leaf inside the sphere, over the cloud's own points as centres"""
    pts = c.pts
    m = BM.Model(pts, np.concatenate([pts.min(0), pts.max(0)]))
    assert m.n == c.n
    perm = m.perm.astype(np.int64)
    leaf_of = np.arange(c.n) // BM.LEAF
    lo = np.stack([np.minimum.reduceat(pts[perm, a], np.arange(0, c.n, BM.LEAF)) for a in range(3)], 1)
    hi = np.stack([np.maximum.reduceat(pts[perm, a], np.arange(0, c.n, BM.LEAF)) for a in range(3)], 1)
    assert np.array_equal(lo.view(np.uint32), m.nodes[BM.level_start(m.depth):][:m.nleaves, :3])  # (the model's leaf boxes)
    assert np.array_equal(hi.view(np.uint32), m.nodes[BM.level_start(m.depth):][:m.nleaves, 3:6])
    inside = R.d2_int(c.g, c.g[perm]) <= c.bound()  # (centre, position)
    holds = np.zeros((c.n, m.nleaves), bool)
    rows, pos = np.nonzero(inside)
    holds[rows, leaf_of[pos]] = True
    r2 = F(c.r) * F(c.r)
    at_r2 = np.stack([FM.box_d2(lo, hi, q) == r2 for q in pts])
    return int((at_r2 & holds).sum())


@pytest.mark.parametrize("cloud,rname", [c for c in CASES if c[1] in RIM_SHARE], ids=[i for i, c in zip(IDS, CASES) if c[1] in RIM_SHARE])
def test_box_edges(cloud, rname):
    count = box_edges(R.case(cloud, rname))
    print("%s %s: %d (centre, leaf) pairs with the leaf's box at exactly r2 and a neighbour in the leaf" % (cloud, rname, count))
    assert count >= BOX_EDGES


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(R.ROWS))
def test_teeth(row):
    model, exact, fixed = R.ROWS[row]
    changed = {name: [] for name in exact}
    for cloud, rname in CASES:
        c = R.case(cloud, rname)
        want = model(c, "contract")
        assert sorted(want) == sorted(exact + fixed), (row, sorted(want))
        for rule in R.differing_rules(row, rname):
            got = model(c, rule)
            differ = [name for name in exact if not R.same(got[name], want[name])]
            assert differ, (row, cloud, rname, rule, "the wrong rule changes nothing")
            assert all(R.same(got[name], want[name]) for name in fixed)
            for name in differ:
                changed[name].append((cloud, rname, rule))
    print(row, {name: len(v) for name, v in changed.items()})
    assert all(changed.values()), (row, [name for name, v in changed.items() if not v])


@pytest.mark.parametrize("rname", list(RIM_SHARE))
def test_each_kernel_of_a_row_has_teeth(rname):
    """Where an operation walks the spheres in more than one kernel, a `<` in ONE of them must show while the others keep the
    contract -- else the rows would be red for the whole operation and blind to a slip in a single copy.  On thin12, at the three
    radii where `<` and `<=` differ: cluster's hook (core to core) and border (non-core to core) kernels in the sparse form,
    segment's hook (smooth to smooth) and border kernels in the curvature-gated form, subsample's round kernel and owner search."""
    import segment_model as GM
    import subsample_model as UM
    c = R.case("thin12", rname)
    src, dst, cnt = c.edges()
    every = np.ones(c.n, bool)
    min_pts = R.SPARSE_MIN_PTS[rname]
    core = cnt >= min_pts
    want = CM.cluster(c.n, src, dst, cnt, min_pts, compact=False, symmetric=True)[0]
    for name, a, b in (("hook", core, core), ("border", ~core, core)):
        s, d, _ = R.without_rim(c, a, b)
        changed = int((CM.cluster(c.n, s, d, cnt, min_pts, compact=False, symmetric=True)[0] != want).sum())
        print("cluster %s %s: %d labels hang on pairs at exactly r" % (rname, name, changed))
        assert changed > 0, ("cluster", name)
    kw = dict(curvature=c.I["curvature"], max_curvature=R.MAX_CURVATURE, min_size=R.MIN_SIZE)
    want, smooth, _ = GM.segment_cloud(c.pts, c.I["normals"], c.r, R.MIN_COS[rname], edges=(src, dst, cnt), **kw)
    for name, a, b in (("hook", smooth, smooth), ("border", ~smooth, smooth)):
        changed = int((GM.segment_cloud(c.pts, c.I["normals"], c.r, R.MIN_COS[rname], edges=R.without_rim(c, a, b), **kw)[0] != want).sum())
        print("segment %s %s: %d labels hang on pairs at exactly r" % (rname, name, changed))
        assert changed > 0, ("segment", name)
    keep = UM.rounds_form(c.n, src, dst, R.SUBSAMPLE_SEED)[0]
    s, d, _ = R.without_rim(c, every, every)
    assert (UM.rounds_form(c.n, s, d, R.SUBSAMPLE_SEED)[0] != keep).any(), "subsample round"
    assert (UM.owners(c.n, s, d, UM.pair_d2(c.pts, s, d), keep) != UM.owners(c.n, src, dst, UM.pair_d2(c.pts, src, dst), keep)).any(), "subsample owner"


def test_mls_fit_words_are_clear_of_the_pivot_band():
    """tests/test_gpu_mls.py lets the device's fit word differ from the model's where the model's smallest pivot ratio lies in
    mls_model.FIT_BAND; the rim test asks the words exactly, so no row of its cases may lie there -- except the rows whose normal
    the contract leaves open (rim_cases.mls_tie), which the rim test holds to their counts alone"""
    for cloud, rname in CASES:
        rows = R.mls_rows(R.case(cloud, rname), "contract")
        rho = np.array([m.rho for m in rows if not R.mls_tie(m)])
        assert not ((rho >= MM.FIT_BAND[0]) & (rho <= MM.FIT_BAND[1])).any(), (cloud, rname)
        # a tie is a tie: the relative gap of the two smallest eigenvalues is rounding noise or far above it, nothing in between
        gap = np.array([m.gap / m.evals[2] for m in rows if m.count >= 6])
        tie = np.array([R.mls_tie(m) for m in rows if m.count >= 6])
        assert (gap[tie] <= 1e-9).all() and (gap[~tie] >= 1e-5).all(), (cloud, rname)
        assert (~tie).sum() + sum(m.count < 6 for m in rows) >= (0.9 if cloud != "full9" else 0.25) * len(rows), (cloud, rname)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_farthest_point_case_ends_at_the_stop_distance():
    pts, m, want = R.fps_case()
    stop2 = F(R.FPS_STOP) * F(R.FPS_STOP)
    assert stop2 == F(4) * SS and 1 < want.count < m
    assert want.min_d2.max() == stop2 and (want.d2[1:] > stop2).all()  # (a `>=` in the stop rule would go on from here)
    assert (want.min_d2 == stop2).sum() > 10
    longer = FM.fps(pts, m, start=R.FPS_START, stop_radius=float(F(1.9) * F(R.S)))
    assert longer.count > want.count
