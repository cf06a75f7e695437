"""FPFH descriptors on the GPU (include/pcpx_descriptors.h) against the numpy model of the contract
(tests/fpfh_model.py) over float32 brute-force spheres.  The SPFH and the pair counts are compared bit for bit; the FPFH against
the float64 value of the contract's sums over the GPU's own SPFH, within the derived bound (n + 16) 2^-23 per bin; a subset call
against the whole-cloud call bit for bit.

The worst observed |fpfh - F| / ((n + 16) 2^-23 F) per case is printed by test_spfh_exact_and_fpfh_within_the_bound (0.126 over all
of them on an MI355X; DESIGN.md section 22 has the figure per cloud)."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import far_cloud_cases
import fpfh_model as M
import shape_features_cases as S

pytestmark = pytest.mark.gpu
F = np.float32
CASES = S.CLOUDS + ("far", "grid")
NEIGHBOURS = (0, 3, 15, 60)  # radius_for(pts, k): a radius that holds about k points
NORMALS = ("random", "gpu")
_clouds, _normals = {}, {}


def _capi():
    return importlib.import_module("point-cloud-processing_amd._capi")


def _cloud(pkg, name):
    """(points, inside the voxel grid, index, {k: radius}); made once"""
    if name not in _clouds:
        grid = None
        if name == "far":
            pts = far_cloud_cases.case("far_1e3").points
        elif name == "grid":  # the voxel grid drops the points beyond x = 0.6
            pts = pkg.synthetic.uniform_cloud(30000, 9)
            pts = pts[np.abs(pts[:, 0] - 0.6) > 1e-3]  # (no point near the grid's face)
            grid = np.array([-0.01, -0.01, -0.01, 0.6, 1.01, 1.01], F)
        else:
            pts = S.cloud(pkg, name)
        inside = pts[:, 0] < 0.6 if grid is not None else np.ones(len(pts), bool)
        ix = pkg.LinkedOctree(pts, voxel_grid=grid) if grid is not None else pkg.LinkedOctree(pts)
        assert ix.size() == int(inside.sum())
        radii = {k: (S.radius_for(pts[inside], k) if k else 0.0) for k in NEIGHBOURS}
        _clouds[name] = (pts, inside, ix, radii)
    return _clouds[name]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _cloud_normals(pkg, name, kind):
    """random unit vectors (these reach every bin), or the GPU's own PCA normals at the radius of about 15 points"""
    if (name, kind) not in _normals:
        pts, _inside, ix, radii = _cloud(pkg, name)
        if kind == "random":
            nrm = _unit(np.random.default_rng(77), len(pts))
        else:
            nrm = ix.shape_features_self(radii[15], evals=False, curvature=False, normals=True)
        _normals[(name, kind)] = np.ascontiguousarray(nrm, F)
    return _normals[(name, kind)]


def _check_fpfh_rows(pts, inside, r, rows, fpfh, spfh, label):
    """fpfh: the GPU's rows for `rows`; spfh: the GPU's SPFH by input row.  Returns the worst |fpfh - F| / bound."""
    worst = 0.0
    assert np.isfinite(fpfh).all() and (fpfh >= 0).all(), label
    for got, i in zip(fpfh.astype(np.float64), rows):
        if not inside[i]:
            assert not got.any(), (label, i)
            continue
        j, d2 = M.sphere(pts, i, r, inside)
        want = M.fpfh_f64(spfh[j], d2)
        rel = M.bound(len(j) + 1)  # the sphere's count: the centre too
        assert (got[want == 0] == 0).all(), (label, i)
        err = np.abs(got - want)
        assert (err <= rel * want).all(), (label, i, float((err[want > 0] / (rel * want[want > 0])).max()))
        if (want > 0).any():
            worst = max(worst, float((err[want > 0] / (rel * want[want > 0])).max()))
        sums, want_sums = got.reshape(3, 11).sum(1), want.reshape(3, 11).sum(1)
        assert ((want_sums == 0) | (np.abs(sums - 100.0) <= rel * 100.0)).all() and (sums[want_sums == 0] == 0).all(), (label, i, sums)
    return worst


@pytest.mark.parametrize("kind", NORMALS)
@pytest.mark.parametrize("k", NEIGHBOURS)
@pytest.mark.parametrize("name", CASES)
def test_spfh_exact_and_fpfh_within_the_bound(pkg, name, k, kind):
    pts, inside, ix, radii = _cloud(pkg, name)
    r, nrm = radii[k], _cloud_normals(pkg, name, kind)
    fpfh, spfh, pairs = ix.fpfh(nrm, r, want_spfh=True)
    assert fpfh.shape == spfh.shape == (len(pts), 33) and pairs.shape == (len(pts),) and pairs.dtype == np.uint32
    rows = S.sampled_rows(len(pts))
    want_spfh, want_pairs = M.spfh(pts, nrm, rows, r, inside)
    label = "%s k%d %s" % (name, k, kind)
    assert np.array_equal(pairs[rows], want_pairs), (label, np.nonzero(pairs[rows] != want_pairs)[0][:10])
    assert np.array_equal(spfh[rows].view(np.uint32), want_spfh.view(np.uint32)), label
    assert not fpfh[~inside].any() and not spfh[~inside].any() and not pairs[~inside].any()
    worst = _check_fpfh_rows(pts, inside, r, rows, fpfh[rows], spfh, label)
    print("%s: r = %.5g, %d points, mean pairs %.1f, bins reached %d of 33, worst |fpfh - F| / bound = %.3f" % (
        label, r, len(pts), float(want_pairs.mean()), int((want_spfh.sum(0) > 0).sum()), worst))
    if k == 0:
        assert not fpfh.any() and not spfh.any() and not pairs.any()  # radius 0: zeros everywhere
    elif k >= 15 and kind == "random" and name != "duplicates":
        assert (want_spfh.sum(0) > 0).all()  # (random normals reach every bin)


def test_subset_is_the_whole(pkg):
    pts, inside, ix, radii = _cloud(pkg, "uniform")
    n, r, nrm = len(pts), radii[15], _cloud_normals(pkg, "uniform", "random")
    whole, spfh, pairs = ix.fpfh(nrm, r, want_spfh=True)
    keypoints = ix.iss_keypoints(radii[60], radii[15], 0.975, 0.975, 5)
    assert len(keypoints) > 1
    rng = np.random.default_rng(4)
    for label, rows in (("300 random rows", rng.choice(n, 300, replace=False)), ("the ISS keypoints", keypoints), ("one row", np.array([n // 3]))):
        rows = rows.astype(np.uint32)
        sub, sub_spfh, sub_pairs = ix.fpfh(nrm, r, rows=rows, want_spfh=True)
        assert sub.shape == (len(rows), 33)
        assert np.array_equal(sub.view(np.uint32), whole[rows].view(np.uint32)), label
        defined = np.zeros(n, bool)  # the points that some described row's sphere holds
        for i in rows:
            defined[M.sphere(pts, i, r)[0]] = True
            defined[i] = True
        assert np.array_equal(sub_spfh[defined].view(np.uint32), spfh[defined].view(np.uint32)), label
        assert np.array_equal(sub_pairs[defined], pairs[defined]), label
        assert not sub_spfh[~defined].any() and not sub_pairs[~defined].any(), label
        assert np.array_equal(ix.fpfh(nrm, r, rows=rows).view(np.uint32), sub.view(np.uint32)), label  # (without the optional outputs)
        print("%s: %d described, %d SPFH needed of %d" % (label, len(rows), int(defined.sum()), n))


def test_subset_edges_on_a_grid_that_drops_points(pkg):
    pts, inside, ix, radii = _cloud(pkg, "grid")
    n, r, nrm = len(pts), radii[15], _cloud_normals(pkg, "grid", "random")
    whole = ix.fpfh(nrm, r)
    out_row, in_row = int(np.nonzero(~inside)[0][0]), int(np.nonzero(inside)[0][0])
    rows = np.array([in_row, n, out_row, 0xFFFFFFFF, n + 7, int(np.nonzero(inside)[0][-1])], np.uint32)
    sub = ix.fpfh(nrm, r, rows=rows)
    assert not sub[[1, 2, 3, 4]].any()  # an entry >= n_in, a row outside the grid
    assert np.array_equal(sub[[0, 5]].view(np.uint32), whole[rows[[0, 5]]].view(np.uint32)) and sub[0].any()
    sub, spfh, pairs = ix.fpfh(nrm, r, rows=np.zeros(0, np.uint32), want_spfh=True)  # m = 0
    assert sub.shape == (0, 33) and not spfh.any() and not pairs.any()
    zero, spfh, pairs = ix.fpfh(nrm, 0.0, rows=rows, want_spfh=True)
    assert not zero.any() and not spfh.any() and not pairs.any()


@pytest.mark.parametrize("n", (1, 2, 65, 129))
def test_small_clouds_against_the_model(pkg, n):
    pts = pkg.synthetic.uniform_cloud(1000, 8)[:n]
    nrm = _unit(np.random.default_rng(n), n)
    ix = pkg.LinkedOctree(pts)
    inside = np.ones(n, bool)
    for r in (0.0, 0.2, 2.0):
        fpfh, spfh, pairs = ix.fpfh(nrm, r, want_spfh=True)
        want_spfh, want_pairs = M.spfh(pts, nrm, np.arange(n), r)
        assert np.array_equal(pairs, want_pairs) and np.array_equal(spfh.view(np.uint32), want_spfh.view(np.uint32)), (n, r)
        _check_fpfh_rows(pts, inside, r, np.arange(n), fpfh, spfh, "n = %d r = %g" % (n, r))
        assert n > 1 or not fpfh.any()
        rows = np.arange(n - 1, -1, -2).astype(np.uint32)
        assert np.array_equal(ix.fpfh(nrm, r, rows=rows).view(np.uint32), fpfh[rows].view(np.uint32))


def test_special_normals(pkg):
    """NaN, zero and non-unit normals are handled by the skip rule, bit for bit as the model has it; duplicates are skipped pairs."""
    pts, inside, ix, radii = _cloud(pkg, "duplicates")
    n, r = len(pts), radii[15]
    rng = np.random.default_rng(12)
    nrm = _unit(rng, n)
    nrm[rng.uniform(size=n) < 0.1] = np.nan
    nrm[rng.uniform(size=n) < 0.1] = 0
    nrm[rng.uniform(size=n) < 0.1] *= F(3)
    fpfh, spfh, pairs = ix.fpfh(nrm, r, want_spfh=True)
    rows = S.sampled_rows(n)
    want_spfh, want_pairs = M.spfh(pts, nrm, rows, r)
    assert np.array_equal(pairs[rows], want_pairs) and np.array_equal(spfh[rows].view(np.uint32), want_spfh.view(np.uint32))
    counts = ix.range_count_self(r)
    assert (pairs[rows] < counts[rows] - 1).any() and (pairs[np.isnan(nrm[:, 0])] == 0).all()  # (skipped pairs; a NaN normal: all of them)
    _check_fpfh_rows(pts, inside, r, rows, fpfh[rows], spfh, "special normals")


def test_refusals_and_empty(pkg):
    capi = _capi()
    empty = pkg.LinkedOctree(np.zeros((0, 3), F))
    assert empty.fpfh(np.zeros((0, 3), F), 0.1).shape == (0, 33)
    assert not empty.fpfh(np.zeros((0, 3), F), 0.1, rows=np.array([0, 5], np.uint32)).any()
    n = 5000
    ix = pkg.LinkedOctree(pkg.synthetic.uniform_cloud(n, 2))
    nrm = _unit(np.random.default_rng(1), n)
    for bad in (-0.01, float("nan")):
        with pytest.raises(pkg.PcpxError) as e:
            ix.fpfh(nrm, bad)
        assert e.value.status == capi.PCPX_ERR_INVALID
    with pytest.raises(ValueError):
        ix.fpfh(nrm[:-1], 0.1)
    out, rows = np.empty((n, 33), F), np.arange(4, dtype=np.uint32)
    lib, h, a, o, w = ix._lib, ix._h, nrm.ctypes.data, out.ctypes.data, rows.ctypes.data
    for fn in (lib.pcpx_fpfh_self, lib.pcpx_fpfh_self_dev):
        for flags in (1, 2, 0x80000000):
            assert fn(h, a, 0.01, None, 0, flags, o, None, None) == capi.PCPX_ERR_INVALID
        assert fn(h, None, 0.01, None, 0, 0, o, None, None) == capi.PCPX_ERR_INVALID     # NULL normals
        assert fn(h, a, 0.01, None, 0, 0, None, None, None) == capi.PCPX_ERR_INVALID     # NULL output
        assert fn(h, a, 0.01, None, 4, 0, o, None, None) == capi.PCPX_ERR_INVALID        # rows NULL with m > 0
        assert fn(h, a, -1.0, w, 4, 0, o, None, None) == capi.PCPX_ERR_INVALID
    shard = pkg.Index(pkg.synthetic.uniform_cloud(50_000, 3), shard=(1, 4), k_hint=15)
    with pytest.raises(pkg.PcpxError) as e:
        shard.fpfh(np.zeros((shard.n_in, 3), F), 0.05)
    assert e.value.status == capi.PCPX_ERR_UNSUPPORTED
    assert shard._lib.pcpx_fpfh_self_dev(shard._h, a, 0.05, None, 0, 0, o, None, None) == capi.PCPX_ERR_UNSUPPORTED


def test_pipeline_on_the_box_surface(pkg):
    """normals -> ISS keypoints -> descriptors at the keypoints with only the kept count read back in between; the descriptors of a
    face's interior are the plane signature.  The PCA normals are turned outwards on the device first: orientation is the caller's."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    pts, _face, edge, _h = S.box_surface()
    n = len(pts)
    r = S.radius_for(pts, 30)
    ix = pkg.LinkedOctree(pts)
    d_pts = torch.from_numpy(pts).to(dev)
    d_normals = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_rows = torch.zeros(n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ix.shape_features_self_dev(r, d_normals=d_normals.data_ptr())
    ix.iss_keypoints_dev(r, 0.55, d_keep, d_kept_rows=d_rows, d_kept_count=d_count)
    ix.synchronize()
    outward = torch.sign((d_normals * (d_pts - 0.5)).sum(1, keepdim=True))
    d_normals = (d_normals * torch.where(outward == 0, torch.ones_like(outward), outward)).contiguous()
    torch.cuda.synchronize()
    m = int(d_count.cpu()[0])  # the one read-back
    assert m > 0
    d_fpfh = torch.full((m, 33), -1.0, dtype=torch.float32, device=dev)
    ix.profile_begin()
    ix.fpfh_dev(d_normals, r, d_fpfh, d_rows=d_rows, m=m)
    ix.synchronize()
    profile = ix.profile_end()
    assert profile["range"][0] == 1 and all(v[0] == 0 for k, v in profile.items() if k != "range"), profile
    kept, fpfh, normals = d_rows[:m].cpu().numpy().astype(np.int64), d_fpfh.cpu().numpy(), d_normals.cpu().numpy()
    counts = ix.range_count_self(r)
    assert np.isfinite(fpfh).all() and (fpfh >= 0).all()
    assert (np.abs(fpfh.astype(np.float64).sum(1) - 300.0) <= 3 * 100.0 * M.bound(counts[kept])).all()
    assert np.array_equal(fpfh.view(np.uint32), ix.fpfh(normals, r, rows=kept.astype(np.uint32)).view(np.uint32))  # host form = device form
    # a whole-cloud call: a point farther than 3 r from every edge sees, through its neighbours' neighbours' normals, one plane only
    d_all = torch.full((n, 33), -1.0, dtype=torch.float32, device=dev)
    ix.fpfh_dev(d_normals, r, d_all)
    ix.synchronize()
    whole = d_all.cpu().numpy()
    assert np.array_equal(whole[kept].view(np.uint32), fpfh.view(np.uint32))
    flat = edge > 3 * r
    assert flat.sum() > 1000
    on = M.PLANE_SIGNATURE > 0
    assert not whole[flat][:, ~on].any()
    assert (np.abs(whole[flat][:, on].astype(np.float64) - 100.0) <= 100.0 * M.bound(counts[flat])[:, None]).all()
    print("box surface: %d keypoints described, %d face-interior rows with the plane signature" % (m, int(flat.sum())))


def test_cpp_fpfh_through_octree_and_kdtree(tmp_path, pkg):
    assert os.path.exists(_capi().LIB_PATH)  # (the package's build made it)
    inc, pkgdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "point-cloud-processing_amd")
    exe = str(tmp_path / "fpfh_shape")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", inc, os.path.join(ROOT, "tests", "cpp", "fpfh_shape.cpp"),
                    "-o", exe, "-L", pkgdir, "-lpcpx", "-Wl,-rpath," + pkgdir, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], check=True)
    pts, _ = pkg.ply.read_ply(os.path.join(GOLDEN, "stanford_bunny.ply"))
    ix = pkg.LinkedOctree(pts)
    r = float(F(2.0 * float(np.mean(ix.mean_knn_distance_self(15)))))
    nrm = np.ascontiguousarray(ix.shape_features_self(r, evals=False, curvature=False, normals=True), F)
    rows = np.random.default_rng(6).choice(len(pts), 500, replace=False).astype(np.uint32)
    ply, rows_path, prefix = str(tmp_path / "cloud.ply"), str(tmp_path / "rows.u32"), str(tmp_path / "fpfh")
    pkg.ply.write_ply(ply, pts, nrm)
    rows.tofile(rows_path)
    res = subprocess.run([exe, ply, rows_path, repr(r), prefix], capture_output=True, text=True, timeout=900)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["points"] == len(pts) and out["rows"] == 500 and out["containers_agree"] and out["subset_is_whole"] and out["written"]
    whole = ix.fpfh(nrm, r)
    assert whole.any()
    assert np.fromfile(prefix + ".all.f32", F).tobytes() == whole.tobytes()
    assert np.fromfile(prefix + ".rows.f32", F).tobytes() == whole[rows].tobytes()
