"""Every operation on a used, poisoned handle as on a fresh one ("Handle history"; the table, the clouds and the
sequences are in tests/handle_history_cases.py, what they promise is checked on the CPU in tests/test_handle_history_cpu.py).

  A  each row's result on a fresh handle is right: the comparison and the tolerance of the operation's own test file, at this
     table's clouds (no tolerance is new here; everything below is equality of bits with that result)
  B  each row after the handle has run it once and `debug_set("poison", byte)` has filled every byte that is scratch by contract,
     for 0x00, 0x55 and 0xFF
  C  the recordings tests/golden/host_forms.npz and tests/golden/fit_bits.npz again, after a 0xFF fill
  D  six seeded sequences of 24 rows on one handle, with rebuilds, switches and fills in between
  E  a handle built from a closed handle's filled blocks, and two live handles called alternately on two streams

Every case prints what it is about to run, flushed, before it launches anything: should a filled word ever be used as an index and
fault, the last line says where to read."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import handle_history_cases as Cs
import host_forms_cases as HF
import fit_bits_cases as FB

pytestmark = pytest.mark.gpu
F = np.float32
BYTES = (0x00, 0x55, 0xFF)
NONE = np.uint32(0xFFFFFFFF)
ROWS = list(Cs.ROWS)


def _say(*what):
    print(*what, flush=True)


_used = {}


def _handle(pkg, cloud):
    """the module's one long-lived handle on a cloud: whatever ran on it before is its history"""
    if cloud not in _used:
        _used[cloud] = Cs.build(pkg, cloud)
    return _used[cloud]


def _home(row):
    return Cs.HOME[Cs.ROWS[row][0]]


def _poison(ix, byte, free=False):
    """the fill, and that it was one: something was filled, the handle's own scratch block was inside it, and for the rows without
    a handle the device's pool and finished leases were reached"""
    ix.debug_set("poison", byte)
    filled, shared, cache = (ix.debug_get(k) for k in ("poisoned_bytes", "poisoned_shared_bytes", "poisoned_cache_bytes"))
    assert filled > 0 and filled - shared - cache >= ix.debug_get("scratch_bytes") >= 0, (filled, shared, cache)
    if free:
        assert shared > 0, (filled, shared, cache)
    return filled


def test_poison_takes_a_byte_and_changes_no_state(pkg):
    _say("poison: arguments and flags")
    ix = Cs.build(pkg, "c1300")
    for bad in (-1, 256, 1 << 40):
        with pytest.raises(pkg.PcpxError):
            ix.debug_set("poison", bad)
    before = Cs.run(pkg, ix, "c1300", "count_self_dev")
    state = ix.debug_get("schedule_state")
    assert _poison(ix, 0xFF) >= ix.debug_get("scratch_bytes")
    assert ix.debug_get("schedule_state") == state and ix.size() == 1300
    assert np.array_equal(ix.bbox(), Cs.build(pkg, "c1300").bbox())
    Cs.same_bits(Cs.run(pkg, ix, "c1300", "count_self_dev"), before, "after the fill")
    ix.close()


# ---- A: the fresh result is right ---------------------------------------------------------------------------------------------------------
def _brute(cloud, r):
    """(inside, the indexed points, brute_edges among them): made once per cloud and radius"""
    import cluster_model as CM
    key = (cloud, float(r))
    if key not in _brute.made:
        I = Cs.inputs(cloud)
        _brute.made[key] = (I["inside"], I["points"][I["inside"]], CM.brute_edges(I["points"][I["inside"]], r))
    return _brute.made[key]


_brute.made = {}


def _knn_rows(oracle, out, pts, queries, k, width=None):
    import test_gpu_parity as TP
    oi, oc, od = oracle.knn_bruteforce(pts, queries, k, Cs.EPS, nthreads=16, want_d2=True)
    TP._assert_rows_exact(pts, queries, k, out["idx"][:, :k], out["cnt"], out["d2"][:, :k], oi, oc, od)
    if width and width > k:  # (tests/test_gpu_far_clouds.py: the padding of a strided row)
        assert (out["idx"][:, k:] == NONE).all() and np.isposinf(out["d2"][:, k:]).all()
    return oi, oc


def _normals_of_rows(oracle, pts, idx, cnt, nrm):
    import test_gpu_parity as TP
    assert TP._cos_err(nrm, oracle.normals_from_knn(pts, idx, cnt, nthreads=16)).max() <= TP.COS_TOL


def _a_knn_dev(pkg, oracle, out, I, k, width=None):
    _knn_rows(oracle, out, I["points"], I["points"], k, width)


def _a_knn_curve(pkg, oracle, out, I, k):
    pts, perm = I["points"], out["perm"].astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(len(pts))) and np.array_equal(out["position_of"][perm], np.arange(len(pts)))
    _knn_rows(oracle, out, pts, pts[perm], k)
    _normals_of_rows(oracle, pts, out["idx"], out["cnt"], out["normals"])  # (row p is input point perm[p]: the normal of its own rows)


def _a_count_self_dev(pkg, oracle, out, I, r):
    inside, sub, _ = _brute("c5000g", r)
    want = oracle.range_count_bruteforce(sub, sub, r, nthreads=16)
    rows = np.nonzero(inside)[0]
    assert np.array_equal(out["cnt"][rows], want) and (out["cnt"][~inside] == Cs.FILL).all()
    assert np.array_equal(np.sort(out["perm"]), rows)
    assert np.array_equal(out["cnt_by_position"], out["cnt"][out["perm"].astype(np.int64)])


def _lists_of(off, idx):
    return [idx[a:b] for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64))]


def _a_lists_self(pkg, oracle, out, I, r):
    pts, inside = I["points"], I["inside"]
    sub_rows = np.nonzero(inside)[0]
    lists = _lists_of(out["offsets"], out["idx"])
    assert len(lists) == len(pts) and all(len(lists[i]) == 0 for i in np.nonzero(~inside)[0])
    _inside, sub, (src, dst, cnt) = _brute("c5000g", r)
    assert np.array_equal(np.diff(out["offsets"].astype(np.int64))[sub_rows], cnt)
    order = np.lexsort((dst, src))
    want = np.split(sub_rows[dst[order]], np.cumsum(cnt.astype(np.int64))[:-1])
    for i, w in zip(sub_rows, want):
        assert np.array_equal(np.sort(lists[i]), w), i


def _a_batch_lists(pkg, oracle, out, I, kind):
    pts, inside = I["points"], I["inside"]
    lists = _lists_of(out["offsets"], out["idx"])
    for q, got in enumerate(lists):
        if kind == "sphere":
            d = pts - I["queries"][q][None, :]
            r = I["radii"][q]
            ok = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r * r
        else:
            b = I["boxes"][q]
            ok = ((pts >= b[None, :3]) & (pts <= b[None, 3:])).all(1)
        assert np.array_equal(got, np.nonzero(ok & inside)[0]), (kind, q)


def _a_normals_knn(pkg, oracle, out, I, k):
    pts = I["points"]
    _oi, _oc = oracle.knn_bruteforce(pts, pts, k, Cs.EPS, nthreads=16)[:2]
    import conftest
    ok, why = conftest.knn_rows_equivalent(pts, pts, out["idx"], out["cnt"], _oi, _oc)
    assert ok, why
    _normals_of_rows(oracle, pts, out["idx"], out["cnt"], out["normals"])
    worst, ill = conftest.normals_vs_float64_eigh(pts, out["idx"][::9], out["cnt"][::9], out["normals"][::9])
    import test_gpu_parity as TP
    assert worst <= TP.COS_TOL, (worst, ill)


def _a_neighbourhoods(pkg, oracle, out, I, k, rows):
    pts = I["points"]
    gi, gc = rows["idx"], rows["cnt"]  # (the GPU's own rows of the same k, as tests/test_gpu_output_forms.py takes them)
    assert np.array_equal(Cs.bits(out["centroids"]), Cs.bits(oracle.centroids_from_knn(pts, gi, gc)))
    assert np.array_equal(Cs.bits(out["mean_dist"]), Cs.bits(oracle.mean_dist_from_knn(pts, pts, gi, gc)))
    _normals_of_rows(oracle, pts, gi, gc, out["normals"])


def _a_oriented(pkg, oracle, out, I, k):
    import test_gpu_parity as TP
    pts = I["points"]
    ix, nrm, idx, cnt, host, host_reached = TP._host_orientation(pkg, pts, k)
    ix.close()
    assert np.array_equal(out["idx"], idx) and np.array_equal(out["cnt"], cnt) and int(out["reached"][0]) == host_reached
    assert np.array_equal(Cs.bits(out["normals"]), Cs.bits(host))
    ref, ref_reached = oracle.propagate_normal_orientations(pts, idx, cnt, nrm)
    assert ref_reached == host_reached and np.array_equal(Cs.bits(host), Cs.bits(ref))


def _a_reconstruct(pkg, oracle, out, I):
    """tests/test_gpu_surface.py::test_reconstruct_surface_matches_host_pipeline at this cloud"""
    import surface_nets_model as SM
    import test_gpu_surface as TS
    pts, k, dims = I["points"], Cs.RECONSTRUCT_K, Cs.RECONSTRUCT_DIMS
    ix = pkg.Index(pts)
    cen, nrm = ix.tangent_planes_knn_self(k)
    idx, cnt = ix.knn_self(k)
    nrm_o, _ = pkg.propagate_normal_orientations(pts, idx, nrm, cnt)
    assert np.array_equal(out["centroids"], cen) and np.array_equal(out["normals"], nrm_o)
    bb = ix.bbox()
    g = SM.regular_grid_containing(bb[:3], bb[3:], (dims, dims, dims))
    field = ix.tangent_plane_sdf(cen, nrm_o, TS._grid(pkg, g))
    ix.close()
    want = SM.surface_nets(field, g)
    TS._same_mesh((out["host_vertices"], out["host_triangles"]), want)
    TS._same_mesh((out["vertices"], out["triangles"]), want)
    assert out["counts"].tolist() == [len(want[0]), len(want[1])] and len(want[1]) > 0


def _a_hint(pkg, oracle, out, I):
    """tests/test_gpu_surface_hint.py::_against_model over this row's own field and hint"""
    import surface_nets_model as SM
    import surface_nets_hint_model as HM
    import test_gpu_surface_hint as TH
    ix = pkg.Index(I["points"])
    bb = ix.bbox()
    ix.close()
    g = SM.regular_grid_containing(bb[:3], bb[3:], (Cs.RECONSTRUCT_DIMS,) * 3)
    f = out["field"]
    mv, mt, mc, mseed = HM.surface_nets_hint(f, g, out["hint"], 0.0, 32768)
    v, t, seed = out["vertices"], out["triangles"], None if int(out["seed"][0]) < 0 else int(out["seed"][0])
    assert seed == mseed
    if mseed is None:
        TH._bytes_equal((v, t), (mv, mt))
        return
    cv, cc, ct = HM.canonical(mv, mt, mc)
    assert v.shape == cv.shape and t.shape == ct.shape
    assert np.array_equal(v.view(np.uint32), cv.view(np.uint32)) and np.array_equal(cc[t.astype(np.int64)], ct)


def _a_cluster(pkg, oracle, out, I, r, min_pts, compact):
    """tests/test_gpu_cluster.py::_check"""
    import cluster_model as CM
    inside, _sub, (src, dst, cnt) = _brute("c5000g", r)
    n, rows = len(inside), np.nonzero(inside)[0]
    want, wcore, wn = CM.cluster(len(cnt), src, dst, cnt, min_pts, compact=compact, symmetric=True)
    if not compact:
        live = want != NONE
        want = want.copy()
        want[live] = rows[want[live]]
    full, fcore, fcnt = np.full(n, NONE, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    full[rows], fcore[rows], fcnt[rows] = want, wcore, cnt
    assert np.array_equal(out["counts"], fcnt) and np.array_equal(out["core"], fcore) and int(out["count"][0]) == wn
    assert np.array_equal(out["labels"], full)
    assert wn > 1


def _a_segment(pkg, oracle, out, I, r, curvature):
    import segment_model as GM
    inside, _sub, edges = _brute("c5000g", r)
    want, wsmooth, wn = GM.segment_cloud(I["points"], I["normals"], r, 0.5, curvature=I["curvature"] if curvature else None, inside=inside, edges=edges,
                                         max_curvature=0.5, min_size=3, oriented=False, compact=True)
    assert np.array_equal(out["smooth"].astype(bool), wsmooth) and int(out["count"][0]) == wn and np.array_equal(out["labels"], want)
    assert wn > 1


def _a_subsample(pkg, oracle, out, I, r):
    """tests/test_gpu_subsample.py::_check"""
    import subsample_model as UM
    inside, sub, (src, dst, _cnt) = _brute("c5000g", r)
    n, rows = len(inside), np.nonzero(inside)[0]
    want_sub, _rounds = UM.rounds_form(len(rows), src, dst, Cs.SUBSAMPLE_SEED, ids=rows)
    assert np.array_equal(UM.greedy(len(rows), src, dst, Cs.SUBSAMPLE_SEED, ids=rows), want_sub)
    own_sub = UM.owners(len(rows), src, dst, UM.pair_d2(sub, src, dst), want_sub)
    want, wown = np.zeros(n, bool), np.full(n, NONE, np.uint32)
    want[rows], wown[rows] = want_sub, rows[own_sub].astype(np.uint32)
    keep = out["keep"].astype(bool)
    assert np.array_equal(keep, want) and np.array_equal(out["kept"], np.nonzero(keep)[0]) and np.array_equal(out["owner"], wown)
    assert 0 < keep.sum() < len(rows)


def _a_local_maxima(pkg, oracle, out, I, r):
    import keypoints_model as KM
    inside, _sub, edges = _brute("c5000g", r)
    want = KM.local_maxima_cloud(I["points"], I["score"], r, 0.25, 2, inside=inside, edges=edges)
    assert np.array_equal(out["keep"].astype(bool), want) and np.array_equal(out["kept"], np.nonzero(want)[0]) and 0 < want.sum()


def _a_iss(pkg, oracle, out, I, r, features):
    """tests/test_gpu_keypoints.py::test_iss_exact_layer: the saliency is, bit for bit and NaN for NaN, the model's float32 arithmetic on
    the eigenvalues and counts of shape_features_self at the salient radius, and the kept set the model's maxima of that saliency"""
    import keypoints_model as KM
    inside, _sub, _ = _brute("c5000g", r)
    sal, want_sal = out["saliency"], KM.iss_score(features["evals"], features["counts"], 0.975, 0.975)
    nan = np.isnan(want_sal)
    assert np.array_equal(np.isnan(sal), nan) and np.array_equal(Cs.bits(sal[~nan]), Cs.bits(want_sal[~nan])) and 0 < (~nan).sum()
    non_max = float(F(1.5 * r))
    _i, _s, edges = _brute("c5000g", non_max)
    want = KM.local_maxima_cloud(I["points"], sal, non_max, min_neighbours=2, inside=inside, edges=edges)
    assert np.array_equal(out["keep"].astype(bool), want) and np.array_equal(out["kept"], np.nonzero(want)[0])


def _a_fpfh(pkg, oracle, out, I, r, subset):
    """tests/test_gpu_fpfh.py::test_spfh_exact_and_fpfh_within_the_bound on sampled rows"""
    import fpfh_model as PM
    import test_gpu_fpfh as TFp
    pts, inside, nrm, n = I["points"], I["inside"], I["normals"], len(I["points"])
    fpfh, spfh, pairs = out["fpfh"], out["spfh"], out["pairs"]
    described = I["rows"] if subset else np.arange(n, dtype=np.uint32)
    take = np.arange(0, len(described), max(1, len(described) // 150))
    rows = described[take]
    real = rows < n
    assert not fpfh[take][~real].any()  # (a row >= n_in: zeros)
    rows, got = rows[real].astype(np.int64), fpfh[take][real]
    want_spfh, want_pairs = PM.spfh(pts, nrm, rows, r, inside)
    assert np.array_equal(pairs[rows], want_pairs) and np.array_equal(Cs.bits(spfh[rows]), Cs.bits(want_spfh))
    assert not spfh[~inside].any() and not pairs[~inside].any()
    if subset:  # (tests/test_gpu_fpfh.py::test_subset_is_the_whole: the SPFH that the described rows' spheres hold, zeros elsewhere)
        whole = Cs.fresh(pkg, "c5000g", "fpfh_all")
        assert np.array_equal(Cs.bits(fpfh[:-1]), Cs.bits(whole["fpfh"][described[:-1].astype(np.int64)]))
        full_spfh = whole["spfh"]
    else:
        full_spfh = spfh
    TFp._check_fpfh_rows(pts, inside, r, rows, got, full_spfh, "fpfh")


def _spheres(I, batch, r):
    import shape_features_cases as S
    pts, inside = I["points"], I["inside"]
    sub, rows = pts[inside], np.nonzero(inside)[0]
    if batch:
        centres, radii = I["queries"], I["radii"]
        sets = [rows[S.brute_set(sub, c, rr)] for c, rr in zip(centres, radii)]
        return centres, sets, np.arange(len(centres))
    take = np.arange(0, len(pts), 17)
    sets = [rows[S.brute_set(sub, pts[i], r)] if inside[i] else np.zeros(0, np.int64) for i in take]
    return pts[take], sets, take


def _a_moments(pkg, oracle, out, I, r, batch):
    import test_gpu_range_neighbourhoods as TRn
    pts = I["points"]
    centres, sets, take = _spheres(I, batch, r)
    extent = float(np.ptp(pts, 0).max())
    TRn._check_rows(oracle, pts, centres, None, sets, out["normals"][take], out["centroids"][take], out["mean_dist"][take], out["counts"][take], extent,
                    "moments batch=%d" % batch)


def _a_features(pkg, oracle, out, I, r, batch, moments):
    import test_gpu_shape_features as TSf
    pts = I["points"]
    centres, sets, take = _spheres(I, batch, r)
    TSf._check_rows(pts, centres, sets, out["evals"][take], out["curvature"][take], out["axes"][take], out["counts"][take], "features batch=%d" % batch,
                    not batch)
    assert np.array_equal(out["counts"], moments["counts"]) and np.array_equal(Cs.bits(out["normals"]), Cs.bits(moments["normals"]))


def _a_nearest(pkg, oracle, out, I, r):
    import icp_model as IM
    want, want_d2 = IM.nearest_posed(I["points"], I["source"], Cs.POSE, 2.0 * r, indexed=I["inside"])
    assert np.array_equal(out["partner"], want) and np.array_equal(Cs.bits(out["d2"]), Cs.bits(want_d2)) and (want != IM.NONE).sum() > 10


def _run_of(out, prefix=""):
    w = out[prefix + "words"]
    done = int(w[1])
    return {"transform": out[prefix + "transform"], "status": int(w[0]), "iterations": done, "last_count": int(w[2]), "count": out[prefix + "count"][:done],
            "rms": out[prefix + "rms"][:done], "partner": out[prefix + "partner"]}


def _a_icp_point(pkg, oracle, out, I, r):
    """tests/test_gpu_icp.py::test_loop_equals_its_replay_from_public_parts"""
    import icp_model as IM
    import test_gpu_icp as TI
    want = IM.icp_point_to_point(I["points"], I["source"], None, 2.0 * r, Cs.ICP_ITERATIONS, TI._fit_of(pkg), indexed=I["inside"])
    TI._same_run(_run_of(out), want, "icp point")
    TI._same_run(_run_of(out, "dev_"), want, "icp point dev")
    done = int(out["dev_words"][1])
    assert (out["dev_count"][done:] == 0).all() and np.isnan(out["dev_rms"][done:]).all() and done >= 1


def _a_icp_plane(pkg, oracle, out, I, r, bbox):
    """tests/test_gpu_icp.py::test_plane_loop_follows_the_float64_model"""
    import icp_model as IM
    import test_gpu_icp as TI
    pts, conditions = I["points"], []
    want = IM.icp_point_to_plane(pts, I["normals"], I["source"], None, 2.0 * r, Cs.ICP_ITERATIONS, bbox, indexed=I["inside"], conditions=conditions)
    assert max(conditions) <= 1e4 and want.iterations >= 1
    extent = float(np.linalg.norm(pts.max(0).astype(np.float64) - pts.min(0)))
    for prefix in ("", "dev_"):
        got = _run_of(out, prefix)
        assert (got["status"], got["iterations"], got["last_count"]) == (want.status, want.iterations, want.last_count)
        assert np.array_equal(got["partner"], want.partner) and np.array_equal(got["count"], want.count[:want.iterations])
        assert np.abs(TI._corners_moved(got["transform"], pts) - TI._corners_moved(want.poses[want.iterations], pts)).max() / extent <= 1e-9
        assert np.abs(got["rms"] - want.rms[:want.iterations]).max() <= 1e-9 * extent
    assert np.array_equal(Cs.bits(out["transform"]), Cs.bits(out["dev_transform"]))


def _a_bilateral(pkg, oracle, out, normals_mode):
    import test_gpu_filters as TFi
    pts, nrm = Cs.filter_cloud()
    B = Cs.BILATERAL
    got = out["out"]
    if not normals_mode:  # test_bilateral_points_one_iteration
        exp = oracle.bilateral_filter_points(pts, nrm, B["sigmaf"], B["sigmag"], K=B["K"], nthreads=16)
        yard = oracle.bilateral_filter_points(pts, nrm, B["sigmaf"], B["sigmag"], K=B["K"], f64_yardstick=True, nthreads=16)
        ext = TFi._extent(pts)
        assert np.abs(got - exp).max() <= TFi.POS_TOL * ext
        assert np.abs(got - yard).max() <= TFi.YARD_FACTOR * max(np.abs(exp - yard).max(), 1e-7 * ext) and np.abs(got - pts).max() > 1e-4
    else:  # test_bilateral_normals
        exp = oracle.bilateral_filter_normals(pts, nrm, B["sigmaf"], B["sigmag"], K=B["K"], nthreads=16)
        yard = oracle.bilateral_filter_normals(pts, nrm, B["sigmaf"], B["sigmag"], K=B["K"], f64_yardstick=True, nthreads=16)
        assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
        c, cg, co = (1.0 - np.sum(a.astype(np.float64) * b, axis=1) for a, b in ((got, exp), (got, yard), (exp, yard)))
        assert c.max() <= TFi.COS_TOL and cg.max() <= max(TFi.YARD_FACTOR * co.max(), 1e-6)


def _a_wlop(pkg, oracle, out):
    """tests/test_gpu_filters.py::test_wlop_one_iteration"""
    import test_gpu_filters as TFi
    pts, sample = Cs.wlop_case()
    W = Cs.WLOP
    exp = oracle.wlop(pts, sample, W["mu"], W["h"], W["k"], uniform=True, nthreads=16)
    yard = oracle.wlop(pts, sample, W["mu"], W["h"], W["k"], uniform=True, f64_yardstick=True, nthreads=16)
    got = out["out"]
    assert got.shape == (W["I"], 3) and np.abs(got - exp).max() <= TFi.POS_TOL
    assert np.abs(got - yard).max() <= TFi.YARD_FACTOR * max(np.abs(exp - yard).max(), 1e-7) and np.abs(got - pts[sample.astype(np.int64)]).max() > 1e-3


def _a_hierarchy(pkg, oracle, out):
    """tests/test_gpu_hierarchy.py::_check"""
    import hierarchy_model as YM
    import test_gpu_hierarchy as TY
    H = Cs.HIERARCHY
    pts = pkg.synthetic.uniform_cloud(H["n"], H["seed"])
    r = YM.hierarchy(pts, H["cluster_size"], H["var_max"])
    TY._assert_margins(r)
    assert np.array_equal(out["idx"], r["idx"]) and np.array_equal(out["points"], np.asarray(pts, F)[out["idx"].astype(np.int64)])


def _a_match(pkg, oracle, out):
    import match_model as MM
    import test_gpu_match as TM
    kf, kr = TM._model_keys("fpfh", Cs.MATCH_DIMS, False)
    m, n = Cs.MATCH_M, Cs.MATCH_N
    fwd = MM.two_smallest(kf[:m, :n])
    TM._same((out["idx"], out["d2"], out["second_idx"], out["second_d2"]), fwd, "match")
    TM._same_pairs((out["pairs"], out["pairs_d2"]), MM.keep_pairs(fwd, MM.two_smallest(kr[:n, :m])[0], 1.0), "match mutual")
    assert len(out["pairs"]) > 0


def _a_ransac_rigid(pkg, oracle, out):
    import register_model as RM
    import test_gpu_register as TR
    R = Cs.RANSAC
    P, Q, pairs, tau = TR._set(R["kind"])
    w = out["words"]
    got = {"found": int(w[0]), "h": int(w[1]), "score": int(w[2]), "ninl": int(w[3]), "inliers": out["inliers"], "xf": out["xf"]}
    TR._same(got, RM.ransac(P, Q, pairs[:R["C"]], R["T"], TR.SEED, TR._sq(tau), TR._sq(R["s"])).best_of(R["T"]), "ransac rigid")
    assert (out["rest"] == -1).all()
    fit, _rms = RM.rigid_fit(P, Q, pairs[:R["C"]], out["inliers"])
    assert np.abs(out["refit"].reshape(-1) - np.asarray(fit).reshape(-1)).max() <= 1e-9  # (test_gpu_register.py: the refit is the fit over the inliers)


def _a_fits(pkg, oracle, out):
    import planes_model as PM
    import test_gpu_register as TR
    S = Cs.fit_pairs()
    TR._check_fit(out["rigid"].reshape(4, 4), float(out["rigid_rms"][0]), S["P"], S["Q"], S["pairs"], None, "fits")
    x = Cs.fit_set()  # (tests/test_gpu_planes.py::test_plane_fit_matches_the_float64_eigenvectors)
    want, rms, val = PM.plane_fit(x)
    assert val[1] - val[0] >= 0.1 * val[2]
    got, got_rms = out["plane"], float(out["plane_rms"][0])
    extent = float(np.abs(x.astype(np.float64)).max())
    assert max(np.abs(got[:3] - want[:3]).max(), abs(got[3] - want[3]) / extent) <= 1e-9
    assert abs(np.linalg.norm(got[:3]) - 1) <= 1e-12 and got[np.argmax(np.abs(got[:3]))] > 0 and abs(got_rms - rms) <= 1e-9 * extent + 1e-6 * rms


def _a_ransac_plane(pkg, oracle, out):
    import planes_model as PM
    import test_gpu_planes as TPl
    L = Cs.PLANE
    P, tau, kw = TPl._model_args(L["kind"], L["C"], L["variant"])
    w = out["words"]
    got = {"found": int(w[0]), "h": int(w[1]), "score": int(w[2]), "ninl": int(w[3]), "inliers": out["inliers"], "plane": out["plane"]}
    TPl._same(got, PM.ransac(P, L["T"], TPl.SEED, tau, **kw).best_of(L["T"]), "ransac plane")
    assert (out["rest"] == -1).all()


def _a_extract(pkg, oracle, out):
    """tests/test_gpu_planes.py::test_extract_planes_peels_the_box_corner"""
    import planes_cases as PC
    labels, planes, scores = PC.model_peel(Cs.PEEL_T)
    assert scores.tolist() == [1650, 889, 361]
    assert np.array_equal(out["labels"], labels) and out["scores"].tolist() == scores.tolist() and np.array_equal(Cs.bits(out["planes"]), Cs.bits(planes))
    for r, axis in enumerate((2, 0, 1)):
        assert abs(abs(out["refits"][r][axis]) - 1) <= 1e-9 and out["refits"][r][:3] @ out["planes"][r][:3] > 0


def _a_kd(pkg, oracle, out):
    pts, q = Cs.kd_sets()
    oi, oc, od = oracle.kd_knn_bruteforce(pts, q, Cs.KD_K, Cs.EPS)[:3]
    assert np.array_equal(out["idx"], oi) and np.array_equal(out["cnt"], oc) and np.array_equal(Cs.bits(out["d2"]), Cs.bits(od))


def _check(pkg, oracle, row, out):
    cloud = _home(row)
    I = Cs.inputs(cloud)
    r = float(I["radius"][0])
    if row in ("knn_dev_k8", "knn_dev_k32", "knn_dev_k40"):
        return _a_knn_dev(pkg, oracle, out, I, int(row.rsplit("k", 1)[1]))
    if row == "knn_strided_k15":
        return _a_knn_dev(pkg, oracle, out, I, 15, 16)
    if row == "knn_curve_k8":
        return _a_knn_curve(pkg, oracle, out, I, 8)
    if row == "knn_batch_k8":
        return _knn_rows(oracle, out, I["points"], I["many_queries"], 8)
    if row == "knn_one_k8":
        return _knn_rows(oracle, out, I["points"], I["queries"][:1], 8)
    if row == "count_batch":
        sub = I["points"][I["inside"]]
        assert np.array_equal(out["cnt"], oracle.range_count_bruteforce(sub, I["queries"], r, nthreads=16))
        return None
    if row == "count_self_dev":
        return _a_count_self_dev(pkg, oracle, out, I, r)
    if row == "lists_self_dev":
        return _a_lists_self(pkg, oracle, out, I, r)
    if row in ("sphere_batch", "aabb_batch"):
        return _a_batch_lists(pkg, oracle, out, I, row.split("_")[0])
    if row in ("normals_knn_dev", "normals_knn_gather_dev"):
        return _a_normals_knn(pkg, oracle, out, I, 15)
    if row == "neighbourhoods_dev":
        return _a_neighbourhoods(pkg, oracle, out, I, 15, Cs.fresh(pkg, cloud, "normals_knn_dev"))
    if row == "oriented_normals":
        return _a_oriented(pkg, oracle, out, I, 8)
    if row == "reconstruct_dev":
        return _a_reconstruct(pkg, oracle, out, I)
    if row == "surface_hint":
        return _a_hint(pkg, oracle, out, I)
    if row == "cluster_m1_compact":
        return _a_cluster(pkg, oracle, out, I, r, 1, True)
    if row == "cluster_m5_plain_dev":
        return _a_cluster(pkg, oracle, out, I, r, 5, False)
    if row in ("segment", "segment_curvature"):
        return _a_segment(pkg, oracle, out, I, r, row == "segment_curvature")
    if row == "subsample":
        return _a_subsample(pkg, oracle, out, I, r)
    if row == "local_maxima":
        return _a_local_maxima(pkg, oracle, out, I, r)
    if row == "iss":
        return _a_iss(pkg, oracle, out, I, r, Cs.fresh(pkg, cloud, "features_self"))
    if row in ("fpfh_all", "fpfh_subset"):
        return _a_fpfh(pkg, oracle, out, I, r, row == "fpfh_subset")
    if row in ("moments_self", "moments_batch"):
        return _a_moments(pkg, oracle, out, I, r, row == "moments_batch")
    if row in ("features_self", "features_batch"):
        return _a_features(pkg, oracle, out, I, r, row == "features_batch", Cs.fresh(pkg, cloud, row.replace("features", "moments")))
    if row == "nearest_posed":
        return _a_nearest(pkg, oracle, out, I, r)
    if row == "icp_point":
        return _a_icp_point(pkg, oracle, out, I, r)
    if row == "icp_plane":
        ix = Cs.build(pkg, cloud)
        bbox = ix.bbox()
        ix.close()
        return _a_icp_plane(pkg, oracle, out, I, r, bbox)
    if row in ("bilateral_points", "bilateral_normals"):
        return _a_bilateral(pkg, oracle, out, row == "bilateral_normals")
    return {"wlop": _a_wlop, "hierarchy": _a_hierarchy, "match": _a_match, "ransac_rigid_dev": _a_ransac_rigid, "fits": _a_fits,
            "ransac_plane_dev": _a_ransac_plane, "extract_planes": _a_extract, "kd_knn": _a_kd}[row](pkg, oracle, out)


@pytest.mark.parametrize("row", ROWS)
def test_a_fresh_result_is_right(pkg, oracle, row):
    pytest.importorskip("torch")
    _say("A", row, _home(row))
    _check(pkg, oracle, row, Cs.fresh(pkg, _home(row), row))


# ---- B: poison ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", BYTES, ids=["0x%02X" % b for b in BYTES])
@pytest.mark.parametrize("row", ROWS)
def test_b_same_bits_after_poison(pkg, row, byte):
    pytest.importorskip("torch")
    _say("B", row, "0x%02X" % byte)
    cloud, free = _home(row), Cs.ROWS[row][0] == "free"
    want = Cs.fresh(pkg, cloud, row)
    ix = _handle(pkg, cloud)
    Cs.run(pkg, ix, cloud, row)  # (so that the scratch has its size)
    _poison(ix, byte, free)
    Cs.same_bits(Cs.run(pkg, ix, cloud, row), want, (row, "0x%02X" % byte))


# ---- C: the recordings under poison -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_forms():
    return np.load(os.path.join(GOLDEN, "host_forms.npz"))


@pytest.fixture(scope="module")
def fit_bits():
    return np.load(os.path.join(GOLDEN, "fit_bits.npz"))


def _equals_recording(name, got, fixture, bits):
    assert sorted(got) == sorted(k.split("/", 1)[1] for k in fixture.files if k.startswith(name + "/") and not k.endswith("/crc")), name
    for key, a in got.items():
        want = fixture[name + "/" + key]
        a = np.ascontiguousarray(a)
        assert a.dtype == want.dtype and a.shape == want.shape, (name, key, a.dtype, want.dtype, a.shape, want.shape)
        assert np.array_equal(bits(a), bits(want)), (name, key)


@pytest.mark.parametrize("name", HF.CASES)
def test_c_host_forms_equal_their_recording_after_poison(pkg, host_forms, name):
    pytest.importorskip("torch")
    _say("C host_forms", name)
    assert np.array_equal(HF.crc(name), host_forms[name + "/crc"]), "inputs differ from the recording's: %s" % name
    ix = HF.index(pkg, HF.split(name)[0])
    for run in (HF.run_host, HF.run_dev):
        assert ix.debug_set("poison", 0xFF) is None and ix.debug_get("poisoned_bytes") > 0
        got = run(pkg, name)
        if got is not None:  # (a batch form has no _dev form)
            _equals_recording(name, got, host_forms, HF.bits)


@pytest.mark.parametrize("name", FB.CASES)
def test_c_fit_bits_equal_their_recording_after_poison(pkg, fit_bits, name):
    pytest.importorskip("torch")
    _say("C fit_bits", name)
    assert np.array_equal(FB.crc(name), fit_bits[name + "/crc"]), "inputs differ from the recording's: %s" % name
    FB.run(pkg, name)  # (so that the device's pool and its leases have their sizes)
    _poison(_handle(pkg, "c70"), 0xFF, free=True)
    _equals_recording(name, FB.run(pkg, name), fit_bits, FB.bits)


# ---- D: interleavings ---------------------------------------------------------------------------------------------------------------------
_states = {}


def _sequence(pkg, seed):
    """runs the seed's sequence once; the schedule_state after every step"""
    if seed in _states:
        return _states[seed]
    first, steps = Cs.plans()[seed]
    _say("D", seed, "on", first)
    ix = Cs.build(pkg, first)
    states = []
    for i, (actions, cloud, row) in enumerate(steps):
        _say("D", seed, "step", i, actions, cloud, row)
        want = Cs.fresh(pkg, cloud, row)
        for a in actions:
            if a[0] == "rebuild":
                Cs.rebuild(ix, a[1])
            elif a[0] == "poison":
                _poison(ix, a[1])
            elif a[1] == "eps_test_mode":
                ix.debug_eps_test_mode(a[2])
            else:
                ix.debug_set(a[1], a[2])
        Cs.same_bits(Cs.run(pkg, ix, cloud, row), want, (seed, i, cloud, row))
        states.append(ix.debug_get("schedule_state"))
    ix.close()
    _states[seed] = states
    return states


@pytest.mark.parametrize("seed", Cs.SEQUENCE_SEEDS)
def test_d_every_step_of_a_sequence_equals_the_fresh_result(pkg, seed):
    pytest.importorskip("torch")
    assert len(_sequence(pkg, seed)) == Cs.STEPS  # (no step is skipped or caught: a step that differs ends the sequence there)


def test_d_the_sequences_cover_the_table_and_reach_the_recorded_order(pkg):
    """every row occurs, after at least three different rows; every kind of rebuild occurs (properties of the plans, asserted without
    a GPU too: tests/test_handle_history_cpu.py); and a repeated self-kNN was handed out by its recorded order"""
    pytest.importorskip("torch")
    occur, follows, moves = Cs.coverage()
    assert occur == set(Cs.ROWS) and all(len(v) >= 3 for v in follows.values()) and moves == set(Cs.TRANSITIONS)
    states = [s for seed in Cs.SEQUENCE_SEEDS for s in _sequence(pkg, seed)]
    assert len(states) == len(Cs.SEQUENCE_SEEDS) * Cs.STEPS and 2 in states, states


# ---- E: recycled blocks -------------------------------------------------------------------------------------------------------------------
RECYCLED = ("knn_dev_k8", "knn_dev_k40", "knn_curve_k8", "knn_batch_k8", "knn_one_k8", "cluster_m1_compact", "cluster_m5_plain_dev", "subsample")


def _container(ix):
    return {"size": np.array([ix.size()], np.uint64), "bbox": ix.bbox()}


@pytest.mark.parametrize("byte", (0x00, 0xFF), ids=["0x00", "0xFF"])
def test_e_a_handle_built_from_filled_blocks(pkg, byte):
    """build, query, close; fill the idle index blocks through a second handle; build a handle of the same size from them"""
    pytest.importorskip("torch")
    _say("E recycled", "0x%02X" % byte)
    other = _handle(pkg, "c70")
    first = Cs.build(pkg, "c5000")
    want = {row: Cs.run(pkg, first, "c5000", row) for row in RECYCLED}  # (knn_curve_k8 holds perm and position_of)
    want["container"] = _container(first)
    first.close()
    other.debug_set("poison", byte)
    assert other.debug_get("poisoned_cache_bytes") >= 5000 * 12, "the closed handle's blocks were idle and were filled"
    again = Cs.build(pkg, "c5000")
    Cs.same_bits(_container(again), want["container"], "container")
    for row in RECYCLED:
        _say("E recycled", row)
        Cs.same_bits(Cs.run(pkg, again, "c5000", row), want[row], (row, byte))
        Cs.same_bits(want[row], Cs.fresh(pkg, "c5000", row), (row, "first build"))
    again.close()


def test_e_two_live_handles_called_alternately(pkg):
    """the first handle's calls on its own stream, the second's (made on torch's stream, so are its leased _dev calls) on torch's"""
    torch = pytest.importorskip("torch")
    _say("E two handles")
    a = Cs.build(pkg, "c5000")
    d_pts = Cs.on_device("c5000")
    b = pkg.Index.from_device(d_pts.data_ptr(), 5000, stream=torch.cuda.current_stream().cuda_stream)
    for row in RECYCLED + ("icp_point", "nearest_posed", "count_self_dev", "lists_self_dev"):
        want = Cs.fresh(pkg, "c5000", row)
        for name, ix in (("own stream", a), ("torch's stream", b), ("own stream", a), ("torch's stream", b)):
            _say("E two handles", row, name)
            Cs.same_bits(Cs.run(pkg, ix, "c5000", row), want, (row, name))
    _poison(a, 0xFF)
    for row in ("icp_point", "knn_dev_k40", "cluster_m5_plain_dev"):
        _say("E two handles after a fill", row)
        Cs.same_bits(Cs.run(pkg, b, "c5000", row), Cs.fresh(pkg, "c5000", row), (row, "after the other handle's fill"))
    torch.cuda.synchronize()
    b.close()
    a.close()
