"""GPU tests of sphere and cylinder detection (include/pcpx_shapes.h).  Everything is compared with the numpy
model of the contract (tests/shapes_model.py) bit for bit -- found, the winning hypothesis, its score, the inlier rows, the 8 float64
of the model, the sphere fit -- except the cylinder fit's axis, whose Jacobi sweeps the model does not restate: that is compared with
numpy.linalg.eigh within an angle derived from the eigenvalue gap, and fed back to the model for everything after it.  What the
scenes are is proved on the model in tests/test_shapes_cpu.py; here only bits are compared."""
import functools
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import exact_buffers as EB
import shapes_cases as Cs
import shapes_model as M
import stream_order as SO

pytestmark = pytest.mark.gpu
F = np.float32
POISON = 7


def _torch():
    return pytest.importorskip("torch")


def _dev(a):
    t = _torch()
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
    return t.from_numpy(a.copy() if a.size else np.zeros(1, a.dtype)).to(t.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def _count_on_device(kind, special):
    P, N, rows = Cs.count_set(kind, special)
    return _dev(P), _dev(N), _dev(rows)


def _outputs(room, refit=True):
    t = _torch()
    dev = t.device("cuda", 0)
    return {"found": t.full((1,), POISON, dtype=t.int32, device=dev), "h": t.full((1,), POISON, dtype=t.int32, device=dev),
            "score": t.full((1,), POISON, dtype=t.int32, device=dev), "inliers": t.full((max(room, 1),), -1, dtype=t.int32, device=dev),
            "ninl": t.full((1,), -1, dtype=t.int64, device=dev), "model": t.full((8,), 7.0, dtype=t.float64, device=dev),
            "refit": t.full((8,), 7.0, dtype=t.float64, device=dev) if refit else None}


def _launch(pkg, kind, d_P, d_N, n, T, tau, d_rows=None, capacity=0, count=None, refit=False, seed=Cs.SEED, stream=None, **gates):
    """one ransac_shape_dev call; returns the device arrays (read them after a synchronisation)"""
    out = _outputs(capacity if d_rows is not None else n)
    out["count"] = None if count is None else _dev(np.array([count], np.uint64))
    prm = pkg.shape_params(kind, T, tau, seed, refit=refit, on_device=True, **gates)
    pkg.ransac_shape_dev(d_P, n, d_N, prm, out["found"], d_rows=d_rows, rows_capacity=capacity, d_rows_count=out["count"], d_hypothesis=out["h"],
                         d_score=out["score"], d_inliers=out["inliers"], d_inlier_count=out["ninl"], d_model=out["model"],
                         d_refit=out["refit"] if refit else None, stream=stream)
    return out


def _read(out):
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "count"}
    n = int(got["ninl"][0])
    return {"found": int(got["found"][0]), "h": int(got["h"].view(np.uint32)[0]), "score": int(got["score"].view(np.uint32)[0]), "ninl": n,
            "inliers": got["inliers"].view(np.uint32)[:max(n, 0)], "rest": got["inliers"][max(n, 0):], "model": got["model"], "refit": got.get("refit")}


def _same(got, want, what):
    found, h, score, inl, model = want
    assert (got["found"], got["h"], got["score"], got["ninl"]) == (found, h, score, score), (what, got["found"], got["h"], got["score"], got["ninl"], want[:3])
    assert np.array_equal(got["inliers"], inl), what
    assert np.array_equal(got["model"].view(np.uint64), model.view(np.uint64)), (what, got["model"].tolist(), model.tolist())
    assert (got["rest"] == -1).all(), what  # (nothing is written beyond the inliers)


def _bits(*arrays):
    return [None if a is None else np.ascontiguousarray(a).view(np.uint8).tobytes() for a in arrays]


def _all_bits(got):
    return (got["found"], got["h"], got["score"], got["ninl"]) + tuple(_bits(got["inliers"], got["model"], got["refit"]))


# ---- every shape of the count loop ----------------------------------------------------------------------------------------------------------
ORIGIN_ROW = 5


@pytest.mark.parametrize("special", [False, True], ids=["finite", "special"])
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("kind", Cs.KINDS)
def test_ransac_equals_the_model_on_every_shape_of_the_loop(pkg, kind, gated, special):
    """all rows with the origin defaulted; and a list with repeated (special: out-of-range, non-finite) rows, room for 300 more than
    the count, the count on the device and the origin row given"""
    t = _torch()
    d_P, d_N, d_rows = _count_on_device(kind, special)
    gates = dict(min_normal_cos=Cs.COSN) if gated else {}
    calls = []
    for T in Cs.TS:
        for C in Cs.count_sizes(gated):
            calls.append(((T, C, False), _launch(pkg, kind, d_P, d_N, C, T, Cs.TAU, **gates)))
            calls.append(((T, C, True), _launch(pkg, kind, d_P, d_N, Cs.ROWS, T, Cs.TAU, d_rows=d_rows, capacity=C + 300, count=C, origin_row=ORIGIN_ROW, **gates)))
    t.cuda.synchronize()
    found_some = 0
    for (T, C, listed), out in calls:
        model = Cs.count_model(kind, gated, special, listed, C, ORIGIN_ROW if listed else None)
        got = _read(out)
        _same(got, model.best_of(T), (kind, gated, special, T, C, listed))
        assert got["found"] == (1 if model.valid[:T].any() else 0)
        found_some += got["found"]
    assert len(calls) == 2 * 5 * 11 and found_some > len(calls) // 2
    assert pkg.shape_plan(64, 1400)["segments"] >= 3 and pkg.shape_plan(64, 1700)["segments"] >= 3  # (several segments were among them)
    if special:
        P, N, rows = Cs.count_set(kind, True)
        assert np.isnan(P).any() and np.isinf(P).any() and np.isnan(N).any() and np.isinf(N).any() and (rows >= Cs.ROWS).any() and len(np.unique(rows)) < len(rows)


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("kind", Cs.KINDS)
def test_the_result_does_not_depend_on_the_split(pkg, kind, gated):
    t = _torch()
    d_P, d_N, d_rows = _count_on_device(kind, False)
    gates = dict(min_normal_cos=Cs.COSN) if gated else {}
    C, caps = 1400, (1400, 1700, 2000)
    plans = {(pkg.shape_plan(64, cap)["segments"], pkg.shape_plan(64, cap)["segment_rows"]) for cap in caps}
    assert len(plans) >= 2, plans
    outs = [_launch(pkg, kind, d_P, d_N, Cs.ROWS, 64, Cs.TAU, d_rows=d_rows, capacity=cap, count=C, refit=True, **gates) for cap in caps]
    outs.append(_launch(pkg, kind, d_P, d_N, Cs.ROWS, 64, Cs.TAU, d_rows=d_rows, capacity=C, refit=True, **gates))  # (no count: the capacity)
    t.cuda.synchronize()
    got = [_read(o) for o in outs]
    want = Cs.count_model(kind, gated, False, True, C).best_of(64)
    for g in got:
        _same(g, want, (kind, gated))
        assert _all_bits(g) == _all_bits(got[0])
    assert got[0]["found"] and got[0]["refit"][6 if kind == M.CYLINDER else 3] > 0


# ---- exact ties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 4096])
@pytest.mark.parametrize("kind", Cs.KINDS)
def test_exact_ties_go_to_the_lowest_hypothesis_and_survive_a_shift(pkg, kind, T):
    P, N, tau = Cs.ties_scene(kind)
    fn = pkg.ransac_sphere if kind == M.SPHERE else pkg.ransac_cylinder
    res = M.ransac(kind, P, N, T, Cs.SEED, tau)
    want = res.best_of(T)
    tied = np.nonzero(res.valid & (res.scores == want[2]))[0]
    assert len(tied) >= 2 and want[1] == tied[0]
    got = fn(P, N, T, tau, seed=Cs.SEED, refit=False)
    assert (int(got["found"]), got["hypothesis"]) == want[:2] and np.array_equal(got["inliers"], want[3])
    assert np.array_equal(got["model"].view(np.uint64), want[4].view(np.uint64))
    far = fn((P.astype(np.float64) + Cs.SHIFT).astype(F), N, T, tau, seed=Cs.SEED, refit=False)
    assert far["hypothesis"] == got["hypothesis"] and np.array_equal(far["inliers"], got["inliers"])
    moved = want[4].copy()
    moved[:3] += Cs.SHIFT
    assert np.array_equal(far["model"].view(np.uint64), moved.view(np.uint64))


# ---- the gates ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Cs.KINDS)
def test_the_gates_change_the_answer(pkg, kind):
    fn = pkg.ransac_sphere if kind == M.SPHERE else pkg.ransac_cylinder
    at = 6 if kind == M.CYLINDER else 3
    radii = {}
    for gate in (None, "free-patch") + Cs.GATE_NAMES[kind]:
        patch, kw = Cs.gate_arguments(gate)
        P, N = Cs.gates_scene(kind, patch)
        got = fn(P, N, Cs.GATE_T, Cs.TAU, seed=Cs.SEED, refit=False, **kw)
        want = Cs.gates_model(kind, gate).best_of(Cs.GATE_T)
        assert (int(got["found"]), got["hypothesis"]) == want[:2] and np.array_equal(got["inliers"], want[3]), gate
        assert np.array_equal(got["model"].view(np.uint64), want[4].view(np.uint64)), gate
        radii[gate] = got["model"][at]
    big, small = Cs.GATE_RADIUS[kind]
    assert all(abs(r - (big if g in (None, "free-patch") else small)) < 0.02 for g, r in radii.items()), radii


# ---- the signs of the normals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("kind", Cs.KINDS)
def test_the_signs_of_the_normals_change_no_bit_on_the_device(pkg, kind, gated):
    t = _torch()
    P, N, _rows = Cs.count_set(kind)
    rng = np.random.default_rng(17)
    gates = dict(min_normal_cos=Cs.COSN) if gated else {}
    if kind == M.CYLINDER:
        gates.update(axis=(0, 0, 1), min_axis_cos=0.5)
    d_P = _dev(P)
    outs = [_launch(pkg, kind, d_P, _dev(N * s), Cs.ROWS, 257, Cs.TAU, refit=True, **gates)
            for s in [np.ones((len(N), 1), F)] + [rng.choice([-1.0, 1.0], (len(N), 1)).astype(F) for _ in range(3)]]
    t.cuda.synchronize()
    got = [_read(o) for o in outs]
    assert got[0]["found"] and got[0]["score"] > 500
    for g in got[1:]:
        assert _all_bits(g) == _all_bits(got[0])


# ---- far from the origin; nothing found -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Cs.KINDS)
def test_a_far_scene_is_recovered_through_its_origin_row(pkg, kind):
    """(that the model's answer is the shape: tests/test_shapes_cpu.py::test_the_noisy_scenes_recover_their_shape)"""
    P, N, _rows = Cs.count_set(kind, False, True)
    fn = pkg.ransac_sphere if kind == M.SPHERE else pkg.ransac_cylinder
    got = fn(P, N, Cs.NOISY_T, Cs.TAU, seed=Cs.SEED, refit=True, origin_row=3)
    want = M.ransac(kind, P, N, Cs.NOISY_T, Cs.SEED, Cs.TAU, origin_row=3).best_of(Cs.NOISY_T)
    assert (int(got["found"]), got["hypothesis"]) == want[:2] and np.array_equal(got["inliers"], want[3]) and len(want[3]) > 600
    assert np.array_equal(got["model"].view(np.uint64), want[4].view(np.uint64))
    at = 6 if kind == M.CYLINDER else 3
    assert abs(got["refit"][at] - Cs.TRUTH[kind]["radius"]) <= 4 * Cs.TAU and np.abs(got["refit"][:3] - Cs.FAR).max() < 2.0


@pytest.mark.parametrize("kind", Cs.KINDS)
def test_nothing_found_gives_zeros_and_leaves_the_refit_alone(pkg, kind):
    t = _torch()
    P, N, _rows = Cs.count_set(kind)
    d_P, d_same = _dev(P), _dev(np.tile(np.array([[0.0, 0.6, 0.8]], F), (len(N), 1)))  # parallel normals: no hypothesis is valid
    plain = _launch(pkg, kind, d_P, d_same, Cs.ROWS, 257, Cs.TAU)
    refit = _launch(pkg, kind, d_P, d_same, Cs.ROWS, 257, Cs.TAU, refit=True)
    bounds = _launch(pkg, kind, d_P, _dev(N), Cs.ROWS, 257, Cs.TAU, refit=True, radius=(50.0, 60.0))
    one = _launch(pkg, kind, d_P, _dev(N), 1, 257, Cs.TAU, refit=True)
    t.cuda.synchronize()
    for out in (plain, refit, bounds, one):
        got = _read(out)
        _same(got, (0, 0, 0, np.zeros(0, np.uint32), np.zeros(8)), kind)
    assert (plain["refit"].cpu().numpy() == 7.0).all()  # (not passed: the caller's)
    for out in (refit, bounds, one):
        assert not out["refit"].cpu().numpy().any()


# ---- exact-size buffers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Cs.KINDS)
def test_nothing_outside_the_documented_extents_is_written(pkg, kind):
    t = _torch()
    P, N, rows = Cs.count_set(kind, True)
    C, cap = 1400, 1700
    arena = EB.Arena("cuda:0", 4 << 20)
    d_P, d_N = arena.take("points", P.size, "f32", data=P), arena.take("normals", N.size, "f32", data=N)
    d_rows, d_count = arena.take("rows", cap, "u32", data=rows[:cap]), arena.take("count", 1, "u64", data=np.array([C], np.uint64))
    out = {k: arena.take(k, n, kind_) for k, n, kind_ in (("found", 1, "u32"), ("h", 1, "u32"), ("score", 1, "u32"), ("inliers", cap, "u32"), ("ninl", 1, "u64"),
                                                          ("model", 8, "f64"), ("refit", 8, "f64"))}
    fit = {k: arena.take("fit " + k, n, kind_) for k, n, kind_ in (("model", 8, "f64"), ("rms", 1, "f64"), ("status", 1, "u32"))}
    t.cuda.synchronize()
    prm = pkg.shape_params(kind, 257, Cs.TAU, Cs.SEED, refit=True, on_device=True, min_normal_cos=Cs.COSN)
    pkg.ransac_shape_dev(d_P, Cs.ROWS, d_N, prm, out["found"], d_rows=d_rows, rows_capacity=cap, d_rows_count=d_count, d_hypothesis=out["h"], d_score=out["score"],
                         d_inliers=out["inliers"], d_inlier_count=out["ninl"], d_model=out["model"], d_refit=out["refit"])
    pkg.shape_fit_dev(kind, d_P, Cs.ROWS, fit["model"], d_normals=d_N, d_rows=out["inliers"], rows_capacity=cap, d_rows_count=out["ninl"], d_rms=fit["rms"],
                      d_status=fit["status"])
    t.cuda.synchronize()
    arena.check("%s ransac and fit" % kind)
    want = M.ransac(kind, P, N, 257, Cs.SEED, Cs.TAU, rows=rows[:C], min_normal_cos=Cs.COSN).best_of(257)
    ninl = int(out["ninl"].cpu().numpy().view(np.uint64)[0])
    assert want[0] and ninl == want[2] and np.array_equal(out["inliers"].cpu().numpy().view(np.uint32)[:ninl], want[3])
    EB.Arena.untouched(out["inliers"], np.arange(cap) >= ninl, "the inliers beyond their count")
    assert np.array_equal(out["model"].cpu().numpy().view(np.uint64), want[4].view(np.uint64))
    assert np.array_equal(fit["model"].cpu().numpy().view(np.uint64), out["refit"].cpu().numpy().view(np.uint64))  # the refit is the fit over the inliers
    assert int(fit["status"].cpu().numpy()[0]) == 0


# ---- the fits -------------------------------------------------------------------------------------------------------------------------------
def _fit_dev(pkg, kind, d_P, n, d_N=None, d_rows=None, capacity=0, d_count=None, stream=None):
    t = _torch()
    dev = t.device("cuda", 0)
    out = {"model": t.full((8,), 7.0, dtype=t.float64, device=dev), "rms": t.full((1,), 7.0, dtype=t.float64, device=dev),
           "status": t.full((1,), POISON, dtype=t.int32, device=dev)}
    pkg.shape_fit_dev(kind, d_P, n, out["model"], d_normals=d_N, d_rows=d_rows, rows_capacity=capacity, d_rows_count=d_count, d_rms=out["rms"],
                      d_status=out["status"], stream=stream)
    return out


def _fit_read(out):
    return out["model"].cpu().numpy(), float(out["rms"].cpu().numpy()[0]), int(out["status"].cpu().numpy()[0]) == 0


def _same_fit(got, want, what):
    assert got[2] == want[2], what
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), (what, got[0].tolist(), want[0].tolist())
    assert np.array([got[1]]).view(np.uint64)[0] == np.array([want[1]]).view(np.uint64)[0], (what, got[1], want[1])


def test_the_sphere_fit_equals_the_model_to_the_bit(pkg):
    t = _torch()
    rng = np.random.default_rng(31)
    outs = []
    for m in Cs.FIT_SIZES:
        P, _N = Cs.fit_set(M.SPHERE, m)
        rows = rng.integers(0, m + 2, 2 * m + 7).astype(np.uint32)  # (repeated rows, and rows out of range)
        d_P = _dev(P)
        outs.append((m, None, _fit_dev(pkg, M.SPHERE, d_P, m)))
        outs.append((m, rows[:m + 3], _fit_dev(pkg, M.SPHERE, d_P, m, d_rows=_dev(rows), capacity=len(rows), d_count=_dev(np.array([m + 3], np.uint64)))))
    t.cuda.synchronize()
    for m, rows, out in outs:
        P, _N = Cs.fit_set(M.SPHERE, m)
        want = M.shape_fit(M.SPHERE, P, None, rows)
        _same_fit(_fit_read(out), want, (m, rows is not None))
        if rows is None:
            _same_fit(pkg.sphere_fit(P), want, (m, "host form"))
    P = np.full((20, 3), np.nan, F)
    P[:3] = [[1, 2, 3], [1, 2, 3], [1, 2, 3]]
    got = pkg.sphere_fit(P)
    assert not got[2] and not got[0].any() and np.isnan(got[1])


def test_the_cylinder_fit_equals_the_model_given_its_axis(pkg):
    """The axis is the Jacobi eigenvector of a float64 matrix: within 1e-13 / gap of numpy.linalg.eigh's, gap = (l1 - l0) / l2, the
    bound tests/test_planes_cpu.py holds pcpx_plane_fit.h to.  With the device's axis given to the model, every other bit is the
    model's."""
    t = _torch()
    outs = []
    for m in Cs.FIT_SIZES:
        P, N = Cs.fit_set(M.CYLINDER, m)
        outs.append((m, _fit_dev(pkg, M.CYLINDER, _dev(P), m, d_N=_dev(N))))
    t.cuda.synchronize()
    for m, out in outs:
        P, N = Cs.fit_set(M.CYLINDER, m)
        got = _fit_read(out)
        if m < 4:
            _same_fit(got, M.shape_fit(M.CYLINDER, P, N), m)
            continue
        val, vec = np.linalg.eigh(M.normals_scatter(M.CYLINDER, P, N))
        gap = (val[1] - val[0]) / val[2]
        u = got[0][3:6]
        assert gap > 1e-3 and abs(np.linalg.norm(u) - 1) <= 1e-15 and u[np.argmax(np.abs(u))] > 0, (m, gap)
        assert np.abs(u - M.PM.sign_rule(vec[:, 0])).max() <= 1e-13 / gap, (m, gap, u, vec[:, 0])
        want = M.shape_fit(M.CYLINDER, P, N, axis=u)
        _same_fit(got, want, m)
        _same_fit(pkg.cylinder_fit(P, N), want, (m, "host form"))


@pytest.mark.parametrize("kind", Cs.KINDS)
def test_the_refit_is_the_fit_over_the_inliers_and_the_host_form_is_the_device_form(pkg, kind):
    t = _torch()
    P, N, rows = Cs.count_set(kind)
    d_P, d_N = _dev(P), _dev(N)
    out = _launch(pkg, kind, d_P, d_N, Cs.ROWS, 257, Cs.TAU, d_rows=_dev(rows), capacity=Cs.ROWS, refit=True)
    fit = _fit_dev(pkg, kind, d_P, Cs.ROWS, d_N=d_N, d_rows=out["inliers"], capacity=Cs.ROWS, d_count=out["ninl"])
    t.cuda.synchronize()
    got, fitted = _read(out), _fit_read(fit)
    assert got["found"] and fitted[2] and np.array_equal(fitted[0].view(np.uint64), got["refit"].view(np.uint64))
    fn = pkg.ransac_sphere if kind == M.SPHERE else pkg.ransac_cylinder
    host = fn(P, N, 257, Cs.TAU, seed=Cs.SEED, rows=rows, refit=True)
    assert (int(host["found"]), host["hypothesis"], len(host["inliers"])) == (got["found"], got["h"], got["score"])
    assert _bits(host["inliers"], host["model"], host["refit"]) == _bits(got["inliers"], got["model"], got["refit"])
    _same(got, Cs.count_model(kind, False, False, True, Cs.ROWS).best_of(257), kind)
    if kind == M.SPHERE:
        want = M.shape_fit(kind, P, N, got["inliers"])
        assert np.array_equal(want[0].view(np.uint64), got["refit"].view(np.uint64))
    fit_host = (pkg.sphere_fit(P, rows=got["inliers"]) if kind == M.SPHERE else pkg.cylinder_fit(P, N, rows=got["inliers"]))
    _same_fit(fit_host, fitted, (kind, "host fit"))


# ---- streams --------------------------------------------------------------------------------------------------------------------------------
def _held_line():
    import test_gpu_stream_order as TSO  # (the session's one calibrated, independent stream and its delay)
    return TSO._line()


@pytest.mark.parametrize("kind", Cs.KINDS)
def test_the_device_form_on_a_held_stream_returns_at_once_and_gives_the_same_bits(pkg, kind):
    t = _torch()
    P, N, rows = Cs.count_set(kind)
    C, cap = 1400, 1700
    prm = pkg.shape_params(kind, 257, Cs.TAU, Cs.SEED, refit=True, on_device=True)

    def run(c):
        d_P, d_N, d_rows, d_count = c.up(P), c.up(N), c.up(rows[:cap]), c.up(np.array([C], np.uint64))
        o = {k: c.out(n, kind_) for k, n, kind_ in (("found", 1, "u32"), ("h", 1, "u32"), ("score", 1, "u32"), ("inliers", cap, "u32"), ("ninl", 1, "u64"),
                                                    ("model", 8, "f64"), ("refit", 8, "f64"), ("fit", 8, "f64"), ("rms", 1, "f64"), ("status", 1, "u32"))}
        c.ready()
        pkg.ransac_shape_dev(d_P, Cs.ROWS, d_N, prm, o["found"], d_rows=d_rows, rows_capacity=cap, d_rows_count=d_count, d_hypothesis=o["h"], d_score=o["score"],
                             d_inliers=o["inliers"], d_inlier_count=o["ninl"], d_model=o["model"], d_refit=o["refit"], device=0, stream=c.stream)
        pkg.shape_fit_dev(kind, d_P, Cs.ROWS, o["fit"], d_normals=d_N, d_rows=o["inliers"], rows_capacity=cap, d_rows_count=o["ninl"], d_rms=o["rms"],
                          d_status=o["status"], device=0, stream=c.stream)
        c.drain()
        return {k: c.down(v) for k, v in o.items()}

    line = _held_line()
    plain_ctx = SO.Held(pkg, None, "c70", SO.HeldLine(t, line.stream, 0))  # (the same stream, idle: the drained run, and the warm-up)
    plain = run(plain_ctx)
    assert plain_ctx.finish() == []
    held = SO.Held(pkg, None, "c70", line)
    got = run(held)
    late = held.finish()
    assert held.returned_before_release, "the calls waited for their stream: they returned after %.1f ms" % (1e3 * held.call_seconds)
    assert SO.differing_bits(got, plain) == [] and late == []
    want = M.ransac(kind, P, N, 257, Cs.SEED, Cs.TAU, rows=rows[:C]).best_of(257)
    assert int(got["found"][0]) == 1 and int(got["h"][0]) == want[1] and int(got["ninl"][0]) == want[2]
    assert np.array_equal(got["model"].view(np.uint64), want[4].view(np.uint64)) and np.array_equal(got["fit"], got["refit"])


@pytest.mark.parametrize("kind", Cs.KINDS)
def test_two_calls_on_two_streams_give_equal_bits(pkg, kind):
    t = _torch()
    d_P, d_N, d_rows = _count_on_device(kind, False)
    t.cuda.synchronize()
    streams = [t.cuda.Stream(device=t.device("cuda", 0)) for _ in range(2)]
    outs = []
    for _ in range(3):
        for s in streams:
            with t.cuda.stream(s):
                outs.append(_launch(pkg, kind, d_P, d_N, Cs.ROWS, 257, Cs.TAU, d_rows=d_rows, capacity=Cs.ROWS, refit=True, stream=s.cuda_stream))
    t.cuda.synchronize()
    got = [_read(o) for o in outs]
    _same(got[0], Cs.count_model(kind, False, False, True, Cs.ROWS).best_of(257), kind)
    assert all(_all_bits(g) == _all_bits(got[0]) for g in got)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def test_normals_ransac_and_fit_chain_with_one_wait(pkg):
    t = _torch()
    P = Cs.chain_scene()
    n = len(P)
    dev = t.device("cuda", 0)
    s = t.cuda.Stream(device=dev)
    d_P = _dev(P)
    t.cuda.synchronize()
    ix = pkg.Index.from_device(d_P.data_ptr(), n, stream=s.cuda_stream)
    prm = pkg.shape_params("sphere", Cs.CHAIN["T"], Cs.CHAIN["tau"], Cs.CHAIN["seed"], on_device=True)
    with t.cuda.stream(s):
        d_N = t.full((n, 3), 7.0, dtype=t.float32, device=dev)
        out = _outputs(n, refit=False)
        fit = {"model": t.full((8,), 7.0, dtype=t.float64, device=dev), "rms": t.full((1,), 7.0, dtype=t.float64, device=dev),
               "status": t.full((1,), POISON, dtype=t.int32, device=dev)}
        ix.range_neighbourhoods_self_dev(Cs.CHAIN["radius"], d_normals=d_N.data_ptr())
        pkg.ransac_shape_dev(d_P, n, d_N, prm, out["found"], d_hypothesis=out["h"], d_score=out["score"], d_inliers=out["inliers"], d_inlier_count=out["ninl"],
                             d_model=out["model"], device=0, stream=s.cuda_stream)
        pkg.shape_fit_dev("sphere", d_P, n, fit["model"], d_rows=out["inliers"], rows_capacity=n, d_rows_count=out["ninl"], d_rms=fit["rms"],
                          d_status=fit["status"], device=0, stream=s.cuda_stream)
    s.synchronize()  # the one wait
    N = d_N.cpu().numpy()
    got = _read(out)
    want = M.ransac(M.SPHERE, P, N, Cs.CHAIN["T"], Cs.CHAIN["seed"], Cs.CHAIN["tau"]).best_of(Cs.CHAIN["T"])
    _same(got, want, "chain")
    assert got["score"] >= 1400 and abs(got["model"][3] - Cs.CHAIN["shape_radius"]) <= 0.01
    _same_fit(_fit_read(fit), M.shape_fit(M.SPHERE, P, None, got["inliers"]), "chain fit")
    assert np.linalg.norm(_fit_read(fit)[0][:3] - Cs.CHAIN["centre"]) <= 0.005


# ---- the C++ program ------------------------------------------------------------------------------------------------------------------------
def test_cpp_shapes_program(tmp_path, pkg):
    capi = importlib.import_module("point-cloud-processing_amd._capi")
    assert os.path.exists(capi.LIB_PATH)  # (the package's build made it)
    inc, pkgdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "point-cloud-processing_amd")
    exe = str(tmp_path / "shapes_shape")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", inc, os.path.join(ROOT, "tests", "cpp", "shapes_shape.cpp"),
                    "-o", exe, "-L", pkgdir, "-lpcpx", "-Wl,-rpath," + pkgdir, "-Wl,-rpath-link,/opt/rocm/lib", "-pthread"], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["calls_agree"]
    P = np.array(out["p"], np.uint32).view(F).reshape(-1, 3)
    N = np.array(out["n"], np.uint32).view(F).reshape(-1, 3)
    tau = float(np.array([out["max_distance"]], np.uint32).view(F)[0])
    T, seed = out["hypotheses"], out["seed"]

    def same(entry, want, what):
        assert (entry["found"], entry["hypothesis"]) == want[:2] and entry["inliers"] == want[3].tolist(), what
        assert np.array_equal(np.array(entry["model"], np.uint64), want[4].view(np.uint64)), what
    ball, pipe = M.ransac(M.SPHERE, P, N, T, seed, tau).best_of(T), M.ransac(M.CYLINDER, P, N, T, seed, tau).best_of(T)
    same(out["ball"], ball, "ball")
    same(out["plain"], ball, "plain")
    same(out["pipe"], pipe, "pipe")
    same(out["one_row"], M.ransac(M.SPHERE, P, N, T, seed, tau, rows=np.array([5], np.uint32)).best_of(T), "one row")
    # the generated shapes: the ball of radius 0.5 about (0.25, -0.5, 1), the pipe of radius 0.25 along z through (-1, 1, .)
    refit = np.array(out["ball"]["refit"], np.uint64).view(np.float64)
    assert len(out["ball"]["inliers"]) >= 290 and np.abs(refit[:4] - [0.25, -0.5, 1.0, 0.5]).max() <= 1e-6
    assert np.array_equal(refit.view(np.uint64), M.shape_fit(M.SPHERE, P, None, np.array(out["ball"]["inliers"], np.uint32))[0].view(np.uint64))
    refit = np.array(out["pipe"]["refit"], np.uint64).view(np.float64)
    assert len(out["pipe"]["inliers"]) >= 290 and np.abs(refit[[0, 1, 3, 4, 5, 6]] - [-1.0, 1.0, 0.0, 0.0, 1.0, 0.25]).max() <= 1e-6
