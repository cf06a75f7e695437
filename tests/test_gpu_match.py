"""GPU tests of descriptor matching (include/pcpx_match.h).  Everything is compared with the numpy model of the
contract (tests/match_model.py) bit for bit -- indices, the bits of every d2, the correspondence lists -- with no tolerance and no
row left out, over every shape at which the code takes another path: m around a wavefront, n around the plan's segment boundaries
for two and three segments, every compiled width.  The model's m x n keys are computed once per (data, dims) on the largest shape;
a smaller shape is a prefix of both sets, so its keys are a corner of that matrix."""
import functools
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import match_model as M

pytestmark = pytest.mark.gpu
F = np.float32
MS = (0, 1, 63, 64, 65, 1000)
DIMS = (1, 3, 16, 33, 36, 64)
WIDTH_DIMS = (5, 8, 17, 24, 37)  # the compiled widths that DIMS does not reach: 8 and 24 at their smallest and largest dims, 48 at its smallest
KINDS = ("ties", "random", "fpfh", "special")


def _capi():
    return importlib.import_module("point-cloud-processing_amd._capi")


@functools.lru_cache(maxsize=None)
def _boundary_ns(pkg_plan, m, dims):
    """n with 2 and with 3 segments whose last segment is one row (a boundary at n - 1), full (at n) and one row short (at n + 1), read from
    the plan"""
    found = {}
    for n in range(1, 2100):
        p = pkg_plan(m, n, dims)
        seg, rows = p["segments"], p["segment_rows"]
        last = n - (seg - 1) * rows
        kind = "one" if last == 1 else "full" if last == rows else "short" if last == rows - 1 else None
        if seg in (2, 3) and kind:
            found.setdefault((seg, kind), n)
    assert sorted(found) == sorted((s, k) for s in (2, 3) for k in ("one", "full", "short")), found
    return tuple(sorted(found.values()))


def _ns(pkg, m, dims):
    return (0, 1, 2, 63) + _boundary_ns(pkg.match_plan, max(m, 1), dims)


@functools.lru_cache(maxsize=None)
def _sets(kind, dims):
    """(src (1000, dims), tgt (n_max, dims)): every shape of the tests is a prefix of both"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + dims)
    m, n = max(MS), 1600
    if kind == "ties":  # small integers: equal d2 across different targets is the rule
        return rng.integers(0, 4, (m, dims)).astype(F), rng.integers(0, 4, (n, dims)).astype(F)
    if kind == "random":
        return rng.normal(size=(m, dims)).astype(F), rng.normal(size=(n, dims)).astype(F)

    def fpfh_like(rows):  # three blocks that each sum to 100 (the first two empty below three columns)
        out = np.zeros((rows, dims))
        cuts = [0, dims // 3, 2 * dims // 3, dims]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if b > a:
                g = rng.gamma(0.5, size=(rows, b - a))
                out[:, a:b] = 100.0 * g / g.sum(1, keepdims=True)
        return out.astype(F)
    if kind == "fpfh":
        return fpfh_like(m), fpfh_like(n)
    out = []
    for rows in (m, n):  # FPFH-like rows, some entries NaN or +-inf, some rows all +0 / -0, some rows copies of others
        a = fpfh_like(rows)
        a[rng.random(a.shape) < 0.01] = np.nan
        a[rng.random(a.shape) < 0.01] = np.inf
        a[rng.random(a.shape) < 0.01] = -np.inf
        zero = rng.random(rows) < 0.1
        a[zero] = np.where(rng.random((int(zero.sum()), dims)) < 0.5, F(0.0), F(-0.0))
        out.append(a)
    out[1][5:40] = out[0][5:40]  # exact matches
    out[0][0], out[1][0] = 0.0, 0.0  # (whatever the draw: zero rows at the start of both sets, so the smallest shapes have them)
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def _model_keys(kind, dims, skip):
    src, tgt = _sets(kind, dims)
    return M.keys(src, tgt, skip), M.keys(tgt, src, skip)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "d2", "second_idx", "second_d2")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


def _same_pairs(got, want, what):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (what, got[0][:5].tolist(), want[0][:5].tolist())
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


@pytest.mark.parametrize("dims", DIMS + WIDTH_DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_match_equals_the_model_on_every_shape(pkg, kind, dims):
    src, tgt = _sets(kind, dims)
    for skip in ((False, True) if kind == "special" else (False,)):
        kf, kr = _model_keys(kind, dims, skip)
        if kind == "ties":  # the tie-breaking rule is what this data is for
            _i1, d1, _i2, d2 = M.two_smallest(kf)
            assert (d1 == d2).mean() >= 0.1, (d1 == d2).mean()
        if kind == "special" and dims > 1:
            assert np.isnan(src).any() and np.isinf(tgt).any() and M.zero_rows(src).any() and M.zero_rows(tgt).any()
        shapes = 0
        for m in MS:
            for n in _ns(pkg, m, dims):
                what = (kind, dims, skip, m, n)
                fwd = M.two_smallest(kf[:m, :n])
                _same(pkg.match_nearest(src[:m], tgt[:n], skip_zero_rows=skip), fwd, what)
                back = M.two_smallest(kr[:n, :m])[0]
                _same_pairs(pkg.match_correspondences(src[:m], tgt[:n], 1.0, True, skip), M.keep_pairs(fwd, back, 1.0), what + ("mutual",))
                ratio = 0.8 if kind != "ties" else 1.0  # (on the integer sets the ratio test is the tie test: d2_best <= d2_second always)
                r2 = float(F(ratio) * F(ratio))
                _same_pairs(pkg.match_correspondences(src[:m], tgt[:n], ratio, False, skip), M.keep_pairs(fwd, None, r2), what + ("ratio",))
                shapes += 1
        assert shapes == len(MS) * 10


def test_match_result_does_not_depend_on_the_split(pkg):
    """a case the plan cuts into three segments, against the same rows matched chunk by chunk by separate calls and merged on the host"""
    for kind, dims in (("ties", 33), ("special", 36), ("random", 3)):
        src, tgt = _sets(kind, dims)
        m = 65
        n = max(_boundary_ns(pkg.match_plan, m, dims))
        assert pkg.match_plan(m, n, dims)["segments"] >= 3
        whole = pkg.match_nearest(src[:m], tgt[:n])
        cuts = [0, 1, 100, 500, 777, 1200, n]  # (not the plan's cuts; every chunk is a call with one segment)
        assert all(pkg.match_plan(m, b - a, dims)["segments"] == 1 for a, b in zip(cuts[:-1], cuts[1:]))
        parts = [pkg.match_nearest(src[:m], tgt[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        _same(M.merge_chunks(parts, cuts[:-1]), whole, (kind, dims))
        _same(whole, M.two_smallest(_model_keys(kind, dims, False)[0][:m, :n]), (kind, dims))


@pytest.mark.parametrize("dims", [d for d in DIMS if d <= 16])
def test_match_agrees_with_the_kd_search(pkg, dims):
    """code this feature does not touch: pcpx_kd_knn_batch(k = 2, eps = 0) returns the same two indices and the same d2 bits"""
    for kind in ("ties", "random"):
        src, tgt = _sets(kind, dims)
        m, n = 1000, max(_boundary_ns(pkg.match_plan, 1000, dims))
        kd = pkg.KdTreeK(tgt[:n])
        idx, cnt, d2 = kd.nearest_neighbours(src[:m], 2, eps=0.0, want_d2=True)
        kd.close()
        assert (cnt == 2).all()
        _same(pkg.match_nearest(src[:m], tgt[:n]), (idx[:, 0], d2[:, 0], idx[:, 1], d2[:, 1]), (kind, dims))


def test_match_mutual_is_symmetric(pkg):
    """on tie-free data the mutual correspondences of (src, tgt) are those of (tgt, src) transposed; on tie-heavy data both equal the
    model (where a tie makes the two directions choose differently)"""
    for dims in (3, 33):
        src, tgt = _sets("random", dims)
        m, n = 1000, 1537
        fwd = M.two_smallest(_model_keys("random", dims, False)[0][:m, :n])
        assert (fwd[1] != fwd[3]).all()  # tie-free
        a, da = pkg.match_correspondences(src[:m], tgt[:n], 1.0, True)
        b, db = pkg.match_correspondences(tgt[:n], src[:m], 1.0, True)
        assert len(a) > 0
        order = np.argsort(b[:, 1], kind="stable")
        assert np.array_equal(a, b[order][:, ::-1]) and np.array_equal(da.view(np.uint32), db[order].view(np.uint32))
        src, tgt = _sets("ties", dims)
        kf, kr = _model_keys("ties", dims, False)
        for (s, t, k1, k2) in ((src[:m], tgt[:n], kf[:m, :n], kr[:n, :m]), (tgt[:n], src[:m], kr[:n, :m], kf[:m, :n])):
            _same_pairs(pkg.match_correspondences(s, t, 1.0, True), M.keep_pairs(M.two_smallest(k1), M.two_smallest(k2)[0], 1.0), dims)


def test_match_dev_calls_on_two_streams(pkg):
    """the device forms wait for nothing and keep their scratch until their stream has passed them: calls queued on two streams, and
    twice on one, before anything is waited for"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    dims, m, n = 33, 1000, 1537
    src, tgt = _sets("fpfh", dims)
    want = M.two_smallest(_model_keys("fpfh", dims, False)[0][:m, :n])
    d_src, d_tgt = torch.from_numpy(src[:m]).to(dev), torch.from_numpy(tgt[:n]).to(dev)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = []
    for s in (streams[0], streams[1], streams[0]):
        with torch.cuda.stream(s):
            o = (torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.float32, device=dev),
                 torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.float32, device=dev))
            pkg.match_nearest_dev(d_src, m, d_tgt, n, dims, *o)
            outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
        got = (o[0].cpu().numpy().view(np.uint32), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32), o[3].cpu().numpy())
        _same(got, want, "dev")


def test_match_chained_on_the_device_after_fpfh(pkg):
    """normals -> FPFH of 2 000 rows of a 20 000-point cloud (Index.fpfh_dev) -> a device-side permutation of those descriptors plus
    2 000 distractor rows as the target -> match_correspondences_dev, with one read-back: the count.  Against the model on the
    downloaded descriptors."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    pts = pkg.synthetic.uniform_cloud(20000, 11)
    ix = pkg.LinkedOctree(pts)
    r = float(F(2.5 * float(np.mean(ix.mean_knn_distance_self(15)))))
    m, extra = 2000, 2000
    gen = torch.Generator(device="cpu").manual_seed(5)
    d_normals = torch.zeros((len(pts), 3), dtype=torch.float32, device=dev)
    d_rows = torch.randperm(len(pts), generator=gen)[:m].to(torch.int32).to(dev)
    d_fpfh = torch.full((m, 33), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ix.shape_features_self_dev(r, d_normals=d_normals.data_ptr())
    ix.fpfh_dev(d_normals, r, d_fpfh, d_rows=d_rows, m=m)
    ix.synchronize()
    perm = torch.randperm(m + extra, generator=gen).to(dev)
    distractors = torch.rand((extra, 33), generator=gen).to(dev)
    distractors = 100.0 * distractors / distractors.reshape(extra, 3, 11).sum(-1).repeat_interleave(11, dim=1)
    d_tgt = torch.cat([d_fpfh, distractors])[perm].contiguous()
    d_pairs = torch.zeros((m, 2), dtype=torch.int32, device=dev)
    d_d2 = torch.zeros(m, dtype=torch.float32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    pkg.match_correspondences_dev(d_fpfh, m, d_tgt, m + extra, 33, d_pairs, d_d2, d_count, max_ratio=0.9, mutual=True, skip_zero_rows=True)
    count = int(d_count.cpu()[0])  # the one read-back (it waits for the stream)
    src, tgt = d_fpfh.cpu().numpy(), d_tgt.cpu().numpy()
    assert src.any() and count > m // 2
    want = M.correspondences(src, tgt, float(F(0.9) * F(0.9)), M.MUTUAL | M.SKIP_ZERO_ROWS)
    got = (d_pairs.cpu().numpy().view(np.uint32)[:count], d_d2.cpu().numpy()[:count])
    _same_pairs(got, want, "chain")
    # every kept source found its own descriptor where the permutation put it, at distance 0
    inverse = torch.argsort(perm).cpu().numpy()
    exact = got[1] == 0
    assert exact.any() and np.array_equal(got[0][exact, 1], inverse[got[0][exact, 0]].astype(np.uint32))


def test_cpp_match_program(tmp_path, pkg):
    assert os.path.exists(_capi().LIB_PATH)  # (the package's build made it)
    inc, pkgdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "point-cloud-processing_amd")
    exe = str(tmp_path / "match_shape")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", inc, os.path.join(ROOT, "tests", "cpp", "match_shape.cpp"),
                    "-o", exe, "-L", pkgdir, "-lpcpx", "-Wl,-rpath," + pkgdir, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["overloads_agree"] and out["dims"] == 5
    src = np.array(out["src"], np.uint32).view(F).reshape(-1, 5)
    tgt = np.array(out["tgt"], np.uint32).view(F).reshape(-1, 5)
    assert M.zero_rows(src).sum() == 1 and M.zero_rows(tgt).sum() == 2

    def nearest_of(entry):
        return (np.array(entry["index"], np.uint32), np.array(entry["d2"], np.uint32).view(F), np.array(entry["second_index"], np.uint32),
                np.array(entry["second_d2"], np.uint32).view(F))

    def pairs_of(entry):
        a = np.array(entry, np.uint32).reshape(-1, 3)
        return np.ascontiguousarray(a[:, :2]), np.ascontiguousarray(a[:, 2]).view(F)
    _same(nearest_of(out["nearest"]), M.nearest(src, tgt), "nearest")
    _same(nearest_of(out["nearest_skip_zero_rows"]), M.nearest(src, tgt, True), "skip")
    _same(nearest_of(out["nearest_no_targets"]), M.nearest(src, tgt[:0]), "no targets")
    _same_pairs(pairs_of(out["mutual_skip_zero_rows"]), M.correspondences(src, tgt, 1.0, M.MUTUAL | M.SKIP_ZERO_ROWS), "mutual")
    _same_pairs(pairs_of(out["ratio_075"]), M.correspondences(src, tgt, float(F(0.75) * F(0.75)), 0), "ratio")
    # the hand-made answers: sources 1 and 4 are copies and tie at targets 0 and 1 (the lower index wins, and target 0's best source is
    # the lower of the copies); source 2 has an exact match; source 0 is a zero row
    assert out["nearest"]["index"] == [3, 0, 2, 4, 0, 5] and out["nearest_skip_zero_rows"]["index"] == [0xFFFFFFFF, 0, 2, 4, 0, 5]
    assert [p[:2] for p in out["mutual_skip_zero_rows"]] == [[1, 0], [2, 2], [3, 4], [5, 5]]
