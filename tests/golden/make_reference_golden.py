"""Regenerates tests/golden/ref_*.npz: inputs and the reference's own outputs (a real build of its headers, oracle/pcp_ref.py)
for the GPU tests in tests/test_gpu_reference_golden.py, which cannot build the reference themselves.

    python tests/golden/make_reference_golden.py

Deterministic (fixed seeds, sequential reference calls, no timestamps in the archives): a second run writes the same bytes.
Clouds are stored as small integers with a power-of-two scale, so every coordinate is exact in float32 and compresses well."""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import far_cloud_cases as FC  # noqa: E402
import nonfinite_cases as NF  # noqa: E402
import surface_nets_model as M  # noqa: E402
from oracle import pcp_ref as R  # noqa: E402

F = np.float32
MAX_FILE = 256 * 1024


def _save(name, **arrays):
    """np.savez_compressed with a fixed timestamp on every member (byte-identical reruns)."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size <= MAX_FILE, (name, size)
    print("%-24s %7d bytes" % (name, size))
    return size


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, (np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32))


def knn():
    """5 000 points on a 1/1024 lattice (exact ties); self rows, a latency-sized batch (<= 512 queries, k <= 32, and the same
    queries with k = 33) and a large batch."""
    rng = np.random.default_rng(101)
    q = rng.integers(0, 1024, (5000, 3)).astype(np.uint16)
    pts = q.astype(F) / F(1024)
    t = R.Octree(pts)
    self_rows = np.sort(rng.choice(len(pts), 600, replace=False)).astype(np.uint32)
    out = dict(points_q=q, scale=np.float32(1 / 1024), self_rows=self_rows)
    out["self_idx"], out["self_cnt"] = t.knn(pts[self_rows], 15)
    lat = (rng.integers(-100, 1124, (300, 3)).astype(F) / F(1024)).astype(F)
    lat[:100] = pts[rng.choice(len(pts), 100, replace=False)]
    out["lat_queries"] = lat
    # k <= 32 with <= 512 queries: pcpx_knn_batch's latency path (k_knn_few); k = 33 on the same queries: the batch path
    out["lat32_idx"], out["lat32_cnt"] = t.knn(lat, 32, 1e-5)
    out["lat15_idx"], out["lat15_cnt"] = t.knn(lat, 15, 0.0)
    out["lat33_idx"], out["lat33_cnt"] = t.knn(lat, 33, 1e-5)
    big = (rng.random((1500, 3)) * 1.2 - 0.1).astype(F)
    out["batch_queries"] = big
    out["batch_idx"], out["batch_cnt"] = t.knn(big, 16, 0.0)
    # mean neighbour distance over the reference's own self rows, every point
    idx, cnt = t.knn(pts, 15)
    out["mean15"] = R.average_distances_to_neighbors(pts, idx, cnt)
    return _save("ref_knn.npz", **out)


def ranges():
    """20 000 points in [0, 8)^3; spheres with one radius each, every group of 64 mixing radius 0, tiny, ordinary and > 1;
    boxes through points."""
    rng = np.random.default_rng(202)
    q = rng.integers(0, 8 * 1024, (20000, 3)).astype(np.uint16)
    pts = q.astype(F) / F(1024)
    t = R.Octree(pts)
    # four spheres at every centre, radii 0, 1e-6, ordinary and > 1: co-located queries share their curve key, so however
    # the queries are reordered into groups of 64, every group holds all four kinds
    locs = pts[rng.choice(len(pts), 64, replace=False)].copy()
    locs[50:] = (rng.random((14, 3)) * 8).astype(F)
    kinds = np.array([0.0, 1e-6, 0.2, 1.3], F)
    centres = np.repeat(locs, 4, axis=0).astype(F)
    radii = np.tile(kinds, len(locs)).astype(F)
    radii[2::8] = F(0.45)  # a second ordinary radius and a second one above 1
    radii[3::8] = F(2.5)
    per_lists = [t.range_sphere(c, r) for c, r in zip(centres, radii)]
    scalar_r = F(0.3)
    sc_lists = [t.range_sphere(c, scalar_r) for c in centres[:128]]
    a, b = pts[rng.integers(0, len(pts), (2, 128))]
    boxes = np.concatenate([np.minimum(a, b), np.minimum(a, b) + (np.abs(a - b) % F(1.5))], 1).astype(F)
    bx_lists = [t.range_aabb(bb[:3], bb[3:]) for bb in boxes]
    out = dict(points_q=q, scale=np.float32(1 / 1024), centres=centres, radii=radii, scalar_radius=scalar_r, boxes=boxes)
    out["per_off"], out["per_idx"] = _csr(per_lists)
    out["scalar_off"], out["scalar_idx"] = _csr(sc_lists)
    out["box_off"], out["box_idx"] = _csr(bx_lists)
    return _save("ref_range.npz", **out)


KD_DIMS = (1, 2, 3, 4, 6, 11, 16)


def kd():
    rng = np.random.default_rng(303)
    out = {}
    for K in KD_DIMS:
        qz = rng.integers(0, 6, (1500, K)).astype(np.uint8)  # a coarse lattice: ties and duplicates
        pts = qz.astype(F) / F(4)
        t = R.KdTree(pts)
        queries = np.concatenate([pts[rng.choice(len(pts), 60, replace=False)], (rng.random((20, K)) * 1.6 - 0.1).astype(F)])
        idx, cnt = t.knn(queries, 16, 0.0)
        idx5, cnt5 = t.knn(queries, 16, 1e-5)
        a, b = pts[rng.integers(0, len(pts), (2, 24))]
        boxes = np.concatenate([np.minimum(a, b), np.maximum(a, b)], 1).astype(F)
        off, bi = _csr([t.range_aabb(bb) for bb in boxes])
        for key, v in (("points_q", qz), ("queries", queries), ("idx", idx), ("cnt", cnt), ("idx_eps", idx5), ("cnt_eps", cnt5),
                       ("boxes", boxes), ("box_off", off), ("box_idx", bi)):
            out["k%d_%s" % (K, key)] = v
    return _save("ref_kd.npz", **out)


def _anisotropic():
    g = M.grid_dict(0.3, -1.7, 2.1, 0.11, 0.07, 0.05, 18, 22, 30)
    p = M.corner_positions(g) - np.array([1.29, -0.93, 2.85], F)
    return g, (np.sqrt((p[:, 0] / F(0.8)) ** 2 + (p[:, 1] / F(0.6)) ** 2 + (p[:, 2] / F(0.55)) ** 2) - F(1)).astype(F)


def _grid_arr(g):
    return np.array([g[n] for n in ("x", "y", "z", "dx", "dy", "dz")], F), np.array([g[n] for n in ("sx", "sy", "sz")], np.uint64)


def surface():
    """Whole-grid meshes (z longest or cubes: the reference meshes every grid cube once there) and hint-seeded ones."""
    cases = []
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (5, 5, 5))
    cases.append(("sphere5", g, M.sphere_field(g), 0.0, None))
    cases.append(("sphere5_hint_on", g, M.sphere_field(g), 0.0, (0, 0, 0.99)))
    cases.append(("sphere5_hint_outside", g, M.sphere_field(g), 0.0, (1.2, 1.2, 1.2)))
    g, f = _anisotropic()
    cases.append(("aniso", g, f, 0.0, None))
    cases.append(("aniso_iso", g, f, -0.3, None))
    cases.append(("aniso_hint_on", g, f, 0.0, (1.29, -0.93, 2.85 + 0.55)))
    g = M.regular_grid_containing((-1, -1, -1), (1, 1, 1), (24, 24, 24))
    r = np.sqrt((M.corner_positions(g).astype(F) ** 2).sum(1)).astype(F)
    shells = (np.abs(r - F(0.6)) - F(0.15)).astype(F)
    cases.append(("shells", g, shells, 0.0, None))
    for n, h in (("inside", (0.02, 0.01, 0.0)), ("between", (0.6, 0.0, 0.01)), ("outside", (0.0, -0.92, 0.0))):
        cases.append(("shells_hint_" + n, g, shells, 0.0, h))
    out = {}
    fields = {}
    for name, g, f, iso, hint in cases:
        gid = next((k for k, v in fields.items() if v[0] is f), None)
        if gid is None:
            gid = "f%d" % len(fields)
            fields[gid] = (f, g)
            out[gid + "_field"] = f
            out[gid + "_grid"], out[gid + "_dims"] = _grid_arr(g)
        v, t = R.surface_nets(f, g, iso, hint=hint, outside=None if hint is None else 1.0)
        out[name + "_field"] = np.array(gid)
        out[name + "_iso"] = np.float32(iso)
        out[name + "_hint"] = np.full(3, np.nan, F) if hint is None else np.asarray(hint, F)
        out[name + "_v"], out[name + "_t"] = v, t
    out["cases"] = np.array([c[0] for c in cases])
    return _save("ref_surface.npz", **out)


def wlop():
    rng = np.random.default_rng(404)
    q = rng.integers(0, 4096, (3000, 3)).astype(np.uint16)
    q[:1500] //= 4  # half the points in a corner, 64 times denser: non-uniform
    pts = q.astype(F) / F(4096)
    sample = np.arange(2000, 3000, dtype=np.uint64)  # the last I: the header's v_j order agrees (DESIGN.md 'Semantics')
    out = dict(points_q=q, scale=np.float32(1 / 4096), sample=sample, h=np.float32(0.12), mu=np.float32(0.45))
    for iters in (1, 3):
        for uniform in (True, False):
            out["out_k%d_u%d" % (iters, int(uniform))] = R.wlop_from_sample(pts, sample, 0.45, 0.12, iters, uniform)
    return _save("ref_wlop.npz", **out)


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


FAR_KNN = (("far_1e3", 1e-5), ("utm", 1e-5), ("utm", 0.0), ("small", 1e-5), ("small", 0.0))
FAR_RANGE = ("cad_mm", "utm")
def far():
    """The clouds of tests/far_cloud_cases.py are rebuilt by the test (only their SHA-256 is stored): octree kNN rows at
    far_1e3, utm and small (eps 1e-5 and 0); lists of spheres with one radius each at cad_mm (r > 1 throughout) and utm (r
    <= 1 and > 1); both surface-nets overloads on a grid at 2^14."""
    out = {}
    for name, eps in FAR_KNN:
        c = FC.case(name)
        key = "knn_%s_eps%d" % (name, int(eps > 0))
        rows = c.rows[:500].astype(np.uint32)
        out[name + "_sha"] = _sha(c.points)
        out[key + "_rows"] = rows
        out[key + "_idx"], out[key + "_cnt"] = R.Octree(c.points).knn(c.points[rows], 15, eps)
    for name in FAR_RANGE:
        c = FC.case(name)
        rng = np.random.default_rng(505)
        out[name + "_sha"] = _sha(c.points)
        centres = c.points[c.rows[:128]].copy()
        centres[64:] = (centres[64:] + rng.uniform(-1, 1, (64, 3)) * F(c.radius)).astype(F)
        radii = np.tile(np.array([c.radius, 2 * c.radius, 1.5, 0.75 * c.radius], F), 32)
        t = R.Octree(c.points)
        out["range_%s_centres" % name], out["range_%s_radii" % name] = centres.astype(F), radii
        out["range_%s_off" % name], out["range_%s_idx" % name] = _csr([t.range_sphere(x, r) for x, r in zip(centres, radii)])
    g, f, iso, hint = FC.far_grid()
    out["grid_v"], out["grid_t"] = R.surface_nets(f, g, iso)
    out["grid_hint_v"], out["grid_hint_t"] = R.surface_nets(f, g, iso, hint=hint, outside=1.0)
    out["grid_field_sha"] = _sha(f)
    return _save("ref_far.npz", **out)


NONFINITE_CLOUDS = ("nan_rows", "odd_nans")  # (a cloud with an infinite coordinate stops the reference on an assertion: not recorded)
NONFINITE_QUERIES = 200


def nonfinite():
    """The clouds and fields of tests/nonfinite_cases.py are rebuilt by the test (only their SHA-256 is stored).  Clouds of 1 300 points
    with NaN coordinates in 40 rows: the octree's size, kNN rows at k = 15 for the first 200 points of the finite base cloud, the
    counts of the case's spheres (radii NaN, -1, 0, +inf among them), the lists of those with a finite radius, and the lists of its
    boxes.  Distance fields with NaN, +inf and -inf corners: the whole-grid mesh."""
    out = {}
    q = np.ascontiguousarray(NF.base(1300)[:NONFINITE_QUERIES])
    centres, radii = NF.spheres()
    ok = np.isfinite(centres).all(1)  # (the reference is asked what it defines: finite centres; any radius)
    listed = ok & np.isfinite(radii)
    out["sphere_rows"], out["sphere_listed"] = np.nonzero(ok)[0].astype(np.uint32), np.nonzero(listed)[0].astype(np.uint32)
    for kind in NONFINITE_CLOUDS:
        pts, _finite = NF.cloud(kind, 1300)
        t = R.Octree(pts)
        out[kind + "_sha"] = _sha(pts)
        out[kind + "_size"] = np.uint64(t.size())
        out[kind + "_idx"], out[kind + "_cnt"] = t.knn(q, 15, 1e-5)
        out[kind + "_sphere_cnt"] = np.array([len(t.range_sphere(c, r)) for c, r in zip(centres[ok], radii[ok])], np.uint32)
        out[kind + "_sphere_off"], out[kind + "_sphere_idx"] = _csr([np.sort(t.range_sphere(c, r)) for c, r in zip(centres[listed], radii[listed])])
        out[kind + "_box_off"], out[kind + "_box_idx"] = _csr([np.sort(t.range_aabb(b[:3], b[3:])) for b in NF.boxes()])
    for name in NF.FIELDS:
        g, f = NF.field(name)
        out[name + "_sha"] = _sha(f)
        out[name + "_v"], out[name + "_t"] = R.surface_nets(f, g, 0.0)
    return _save("ref_nonfinite.npz", **out)


def main():
    if not R.available():
        sys.exit("no build of the reference: %s" % R.why_unavailable())
    total = knn() + ranges() + kd() + surface() + wlop() + far() + nonfinite()
    print("%-24s %7d bytes" % ("total", total))
    assert total <= 1536 * 1024


if __name__ == "__main__":
    main()
