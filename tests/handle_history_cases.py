"""The cases of tests/test_gpu_handle_history.py: one table of operations, the clouds they run on and the comparison of each with
its model.  What is tested is not an operation but what a call FINDS: every entry point keeps state between calls -- in the handle
(one scratch block that every operation lays out for itself and that only grows, the k > 32 pass keys, the gather scratch and
the input-index table with its flag, two work-queue counter sets, the recorded schedule, the staging pool), in the device (the
shared pool and the leased blocks a later _dev call takes over) and in the process (the cache that hands a destroyed index's
blocks, contents and all, to the next index) -- and the content of scratch is unspecified, so every row must give the same bits
after any earlier call and after `debug_set("poison", byte)` has filled all of it.

The clouds are seeded, float32, in the unit cube, the smallest at which the shared pieces can go wrong:

    c70     70 points: two query groups, the last leaf part full
    c1300   1 300 points: a second scan tile, partly filled
    c1300b  as many other points (a rebuild to the same size)
    c5000   5 000 points: several scan tiles, inner tree nodes
    c5000g  5 000 points of which 40 are exact copies of others, under the voxel grid of host_forms_cases.GRID, which drops the
            points beyond x = 0.6: n < n_in, the rows outnumber the leaf slots
    c33000  33 000 points: 516 query groups, the first size (512 groups) at which a self-kNN launch records its groups' times and a
            repeated one is handed out by them -- no smaller cloud reaches schedule_state 2; only the kNN rows run on it
    c0      no point (a rebuild to an empty cloud and back)

A radius holds about eight points (the formula of host_forms_cases.inputs).  DESIGN.md section 10 leaves open which of several
points that tie exactly with the k-th distance a kNN row keeps, so the rows that rest on a kNN set run only on the clouds of
KNN_CLOUDS, and `knn_ties` (asserted on the CPU, tests/test_handle_history_cpu.py) finds no query of them whose k-th and (k+1)-th
squared distances are equal, for any k used.  Seeded inputs, built once, never changed; only the public Python API is called.

A row is a callable over a Ctx (the package, a handle, its cloud's inputs) that returns a dict of numpy arrays, compared by their
bits.  Where a contract leaves an order open the row returns the canonical form it names: the sphere and box lists of the batch
forms are "in unspecified order" (include/pcpx.h, conventions), so each list is sorted; every other output
-- range_lists_self_dev's lists in tree order, the surface-nets meshes in ascending cube index (DESIGN.md sections 13 and 15), the
hierarchy's points in breadth-first cluster order (section 14) -- has its order fixed by its contract and is compared as it
comes."""
import functools

import numpy as np

import host_forms_cases as H

F = np.float32
EPS = 1e-5
FILL = 7
GRID = H.GRID
SIZES = {"c0": 0, "c70": 70, "c1300": 1300, "c1300b": 1300, "c5000": 5000, "c5000g": 5000, "c33000": 33000}
SEEDS = {"c0": 2000, "c70": 2070, "c1300": 3300, "c1300b": 3301, "c5000": 7000, "c5000g": 7001, "c33000": 35000}
KNN_CLOUDS = ("c70", "c1300", "c1300b", "c5000", "c33000")
DUPLICATES = 40
QUERIES = 37          # the batch forms' spheres, boxes and the latency path's queries
BATCH_QUERIES = 600   # pcpx_knn_batch takes the latency path up to 512 queries: the general path needs more
SOURCE = 200          # rows of the moved source of nearest_posed and icp
KS = (8, 15, 32, 40)  # every k a kNN row uses
SCAN_TILE, LEAF, GROUP = 1024, 8, 64  # csrc/pcpx_scan.h, csrc/pcpx_internal.h


def gridded(cloud):
    return cloud.endswith("g")


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _rigid(axis, degrees, shift):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    T[:3, 3] = shift
    return T


POSE = _rigid([0.3, -1.0, 0.5], 2.0, [0.004, -0.003, 0.002])  # (the source is the cloud's own points moved by its inverse)


@functools.lru_cache(maxsize=None)
def inputs(cloud):
    """the input arrays of a cloud, by name"""
    n = SIZES[cloud]
    rng = np.random.default_rng(SEEDS[cloud])
    pts = rng.uniform(0, 1, (n, 3)).astype(F)
    if gridded(cloud):
        pts[np.abs(pts[:, 0] - 0.6) < 1e-3, 0] = F(0.5)  # (no point near the grid's face)
        rows = rng.permutation(n)
        pts[rows[:DUPLICATES]] = pts[rows[DUPLICATES:2 * DUPLICATES]]
    inside = pts[:, 0] < 0.6 if gridded(cloud) else np.ones(n, bool)
    radius = F(min(0.7, (1.91 / max(n, 1)) ** (1.0 / 3.0)))  # 4/3 pi r^3 n = 8
    rows = np.concatenate([np.arange(n - 1, -1, -2), [n + 3]]).astype(np.uint32)  # every other row, descending, and one >= n_in
    inv = np.linalg.inv(POSE)
    take = rng.permutation(n)[:min(SOURCE, n)]
    source = (pts[take].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3] + rng.normal(0, 0.1 * float(radius), (len(take), 3))).astype(F)
    centres = rng.uniform(-0.1, 1.1, (QUERIES, 3)).astype(F)
    half = (radius * rng.uniform(0.5, 1.5, (QUERIES, 3))).astype(F)
    d = {"points": pts, "inside": inside, "radius": np.array([radius], F), "normals": _unit(rng, n), "curvature": rng.uniform(0, 1, n).astype(F),
         "score": (np.floor(rng.uniform(0, 16, n)) / 16).astype(F),  # (ties: the lower row wins)
         "rows": rows, "queries": centres, "radii": (radius * rng.uniform(0.5, 1.5, QUERIES)).astype(F),
         "boxes": np.concatenate([centres - half, centres + half], 1).astype(F),
         "many_queries": rng.uniform(-0.05, 1.05, (BATCH_QUERIES, 3)).astype(F), "source": source}
    for a in d.values():
        a.setflags(write=False)
    return d


def statistics(cloud):
    """what the description above promises of a cloud: (n_in, n, leaf slots, scan tiles of the rows, query groups)"""
    I = inputs(cloud)
    n_in, n = len(I["points"]), int(I["inside"].sum())
    return {"n_in": n_in, "n": n, "leaf_slots": -(-n // LEAF) * LEAF, "tiles": -(-n_in // SCAN_TILE), "last_tile": n_in % SCAN_TILE,
            "groups": -(-n // GROUP), "last_leaf": n % LEAF}


def knn_ties(oracle, cloud, threads=16):
    """the number of (query, k) whose k-th and (k + 1)-th squared distances are equal, by float32 brute force on the CPU, over every
    query a kNN row asks on this cloud and every k of KS"""
    I = inputs(cloud)
    pts = I["points"]
    ties = 0
    for q in (pts, I["many_queries"], I["queries"]):
        k1 = min(max(KS) + 1, len(pts))
        _idx, cnt, d2 = oracle.knn_bruteforce(pts, q, k1, eps=EPS, nthreads=threads, want_d2=True)
        for k in KS:
            both = cnt > k
            ties += int((d2[both, k - 1] == d2[both, k]).sum())
    return ties


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def build(pkg, cloud):
    """a fresh handle on the cloud"""
    I = inputs(cloud)
    ix = pkg.LinkedOctree(I["points"], voxel_grid=GRID) if gridded(cloud) else pkg.LinkedOctree(I["points"])
    assert ix.size() == int(I["inside"].sum())
    return ix


@functools.lru_cache(maxsize=None)
def on_device(cloud):
    """the cloud's points as a device array (at least one row: an empty tensor has no address)"""
    import torch
    pts = inputs(cloud)["points"]
    t = torch.from_numpy(pts.copy() if len(pts) else np.zeros((1, 3), F)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def rebuild(ix, cloud):
    """rebuild_dev of a handle to the cloud"""
    ix.rebuild_dev(on_device(cloud).data_ptr(), SIZES[cloud], voxel_grid=GRID if gridded(cloud) else None)
    ix.synchronize()
    assert ix.size() == int(inputs(cloud)["inside"].sum())


class Ctx:
    """what a row gets: the package, a handle and its cloud's inputs, and the device arrays of a _dev call"""
    stream = None  # what a row passes to a call that takes a stream (tests/stream_order.py: the stream it holds)

    def __init__(self, pkg, ix, cloud):
        self.pkg, self.ix, self.cloud, self.I = pkg, ix, cloud, inputs(cloud)
        self.n_in, self.n, self.r = SIZES[cloud], int(self.I["inside"].sum()), float(self.I["radius"][0])

    @staticmethod
    def torch():
        import torch
        return torch

    def up(self, a):
        t = self.torch()
        a = np.ascontiguousarray(a).reshape(-1)
        a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
        d = t.from_numpy(a.copy() if len(a) else np.zeros(1, a.dtype)).to(t.device("cuda", 0))
        t.cuda.synchronize(0)  # (torch's stream is not the handle's; device 0 by number: a caller's thread may have another current)
        return d

    def out(self, length, kind):
        """a device array of `length` entries of kind "u32", "u64", "u8", "f32" or "f64", filled with FILL"""
        t = self.torch()
        dtype = {"u32": t.int32, "u64": t.int64, "u8": t.uint8, "f32": t.float32, "f64": t.float64}[kind]
        return t.full((max(int(length), 1),), FILL, dtype=dtype, device=t.device("cuda", 0))

    def ready(self):
        self.torch().cuda.synchronize(0)  # (the fills are on torch's stream, a handle's call on its own)

    def drain(self):
        """after the calls on the handle: its stream is drained before an output is looked at"""
        self.ix.synchronize()

    def down(self, d, length=None, width=1):
        """after the handle's stream is drained: the array on the host, unsigned, cut to `length` entries, `width` to a row"""
        a = d.cpu().numpy()
        a = a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))
        a = a if length is None else a[:int(length)]
        return a.reshape(-1, width) if width > 1 else a


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------
# kNN
def _knn_dev(c, k, stride=0):
    w = stride or k
    idx, cnt, d2 = c.out(c.n_in * w, "u32"), c.out(c.n_in, "u32"), c.out(c.n_in * w, "f32")
    c.ready()
    if stride:
        c.ix.knn_self_strided_dev(k, EPS, stride, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
    else:
        c.ix.knn_self_dev(k, EPS, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr())
    c.drain()
    return {"idx": c.down(idx, c.n_in * w, w), "cnt": c.down(cnt, c.n_in), "d2": c.down(d2, c.n_in * w, w)}


def _knn_curve(c, k):
    idx, cnt, d2, nrm = c.out(c.n * k, "u32"), c.out(c.n, "u32"), c.out(c.n * k, "f32"), c.out(c.n * 3, "f32")
    perm, pos = c.out(c.n, "u32"), c.out(c.n_in, "u32")
    c.ready()
    c.ix.knn_self_curve_order_dev(k, EPS, idx.data_ptr(), cnt.data_ptr(), d2.data_ptr(), nrm.data_ptr())
    c.ix.perm_dev(perm.data_ptr(), pos.data_ptr())
    c.drain()
    return {"idx": c.down(idx, c.n * k, k), "cnt": c.down(cnt, c.n), "d2": c.down(d2, c.n * k, k), "normals": c.down(nrm, c.n * 3, 3),
            "perm": c.down(perm, c.n), "position_of": c.down(pos, c.n_in)}


def _knn_host(c, queries, k):
    idx, cnt, d2 = c.ix.knn(queries, k, EPS, want_d2=True)
    return {"idx": idx, "cnt": cnt, "d2": d2}


# ranges
def _count_dev(c):
    cnt, pos = c.out(c.n_in, "u32"), c.out(c.n_in, "u32")  # (at curve positions: the first n entries)
    perm = c.out(c.n, "u32")
    c.ready()
    c.ix.range_count_self_dev(c.r, cnt.data_ptr())
    c.ix.range_count_self_curve_order_dev(c.r, pos.data_ptr())
    c.ix.perm_dev(perm.data_ptr())
    c.drain()
    # (input order: the rows of the points outside the grid are the caller's, here FILL)
    return {"cnt": c.down(cnt, c.n_in), "cnt_by_position": c.down(pos, c.n), "perm": c.down(perm, c.n)}


def _lists_dev(c):
    off = c.out(c.n_in + 1, "u64")
    c.ready()
    total = c.ix.range_lists_self_dev(c.r, off.data_ptr())
    idx = c.out(total, "u32")
    c.ready()
    assert c.ix.range_lists_self_dev(c.r, off.data_ptr(), idx.data_ptr(), total) == total
    c.drain()
    return {"offsets": c.down(off, c.n_in + 1), "idx": c.down(idx, total)}


def _sorted_lists(off, idx):
    """each list ascending: the batch forms' lists are in unspecified order (include/pcpx.h)"""
    out = idx.copy()
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        out[a:b] = np.sort(idx[a:b])
    return {"offsets": off, "idx": out}


# normals
def _normals_dev(c, k, gather):
    nrm, idx, cnt = c.out(c.n_in * 3, "f32"), c.out(c.n_in * k, "u32"), c.out(c.n_in, "u32")
    c.ready()
    if gather:
        c.ix.debug_set("gather_outputs", 1)
    c.ix.normals_knn_self_dev(k, EPS, nrm.data_ptr(), idx.data_ptr(), cnt.data_ptr())
    c.drain()
    if gather:
        c.ix.debug_set("gather_outputs", 0)
    return {"normals": c.down(nrm, c.n_in * 3, 3), "idx": c.down(idx, c.n_in * k, k), "cnt": c.down(cnt, c.n_in)}


def _neighbourhoods_dev(c, k):
    nrm, cen, md = c.out(c.n_in * 3, "f32"), c.out(c.n_in * 3, "f32"), c.out(c.n_in, "f32")
    c.ready()
    c.ix.neighbourhoods_self_dev(k, EPS, nrm.data_ptr(), cen.data_ptr(), md.data_ptr())
    c.drain()
    return {"normals": c.down(nrm, c.n_in * 3, 3), "centroids": c.down(cen, c.n_in * 3, 3), "mean_dist": c.down(md, c.n_in)}


def _oriented(c, k):
    nrm, idx, cnt, reached = c.ix.oriented_normals_knn_self(k, EPS, want_knn=True)
    return {"normals": nrm, "idx": idx, "cnt": cnt, "reached": np.array([reached], np.uint64)}


# reconstruction
RECONSTRUCT_K, RECONSTRUCT_DIMS = 8, 12  # (a k of KS: knn_ties covers it)


def _reconstruct(c):
    v, t, cen, nrm, grid = c.ix.reconstruct_surface(RECONSTRUCT_K, (RECONSTRUCT_DIMS,) * 3, EPS, want_planes=True)
    return {"vertices": v, "triangles": t, "centroids": cen, "normals": nrm}


def _reconstruct_dev(c):
    import ctypes as C
    S = c.pkg.surface
    first = _reconstruct(c)  # (the host form: it sizes the mesh)
    V, T = len(first["vertices"]), len(first["triangles"])
    dv, dt = c.out(V * 3, "f32"), c.out(T * 3, "u32")
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    d = np.array([RECONSTRUCT_DIMS] * 3, np.uint64)
    c.ready()
    S.check(S._capi.load().pcpx_reconstruct_surface_dev(c.ix._h, RECONSTRUCT_K, EPS, d.ctypes.data_as(S._capi.u64p), 0.0, C.c_void_p(dv.data_ptr()), V,
                                                        C.c_void_p(dt.data_ptr()), T, C.byref(nv), C.byref(nt), None, None, None))
    c.drain()
    return {"counts": np.array([nv.value, nt.value], np.uint64), "vertices": c.down(dv, V * 3, 3), "triangles": c.down(dt, T * 3, 3),
            "host_vertices": first["vertices"], "host_triangles": first["triangles"], "centroids": first["centroids"], "normals": first["normals"]}


def _hint(c):
    """the example's `graph` variant: the field of the handle's tangent planes, meshed from the densest point's neighbourhood"""
    pts = c.I["points"]
    cen, nrm = c.ix.tangent_planes_knn_self(RECONSTRUCT_K, EPS)
    bb = c.ix.bbox()
    grid = c.pkg.regular_grid_containing(bb[:3], bb[3:], (RECONSTRUCT_DIMS,) * 3)
    field = c.ix.tangent_plane_sdf(cen, nrm, grid, EPS)
    hint = c.ix.surface_hint(pts, RECONSTRUCT_K, EPS)
    v, t, seed = c.pkg.surface_nets_from_hint(field, grid, hint, with_seed=True)
    return {"field": field, "hint": hint, "vertices": v, "triangles": t, "seed": np.array([-1 if seed is None else seed], np.int64)}


# clustering, segmentation, sampling, keypoints, descriptors: the forms of host_forms_cases on this table's clouds
def _cluster(c, min_pts, compact):
    lab, count, core, counts = c.ix.cluster(c.r, min_pts, compact, want_core=True, want_counts=True)
    return {"labels": lab, "count": np.array([count], np.uint64), "core": core.astype(np.uint8), "counts": counts}


def _cluster_dev(c, min_pts, compact):
    lab, core, counts, count = c.out(c.n_in, "u32"), c.out(c.n_in, "u8"), c.out(c.n_in, "u32"), c.out(1, "u64")
    c.ready()
    c.ix.cluster_dev(c.r, lab.data_ptr(), min_pts, compact, core.data_ptr(), counts.data_ptr(), count.data_ptr())
    c.drain()
    return {"labels": c.down(lab, c.n_in), "count": c.down(count, 1), "core": c.down(core, c.n_in), "counts": c.down(counts, c.n_in)}


def _segment(c, curvature):
    lab, count, smooth = c.ix.segment(c.I["normals"], c.r, min_cos=0.5, curvature=c.I["curvature"] if curvature else None, max_curvature=0.5,
                                      min_size=3, want_smooth=True)
    return {"labels": lab, "count": np.array([count], np.uint64), "smooth": smooth.astype(np.uint8)}


SUBSAMPLE_SEED = 5


def _subsample(c):
    kept, keep, owner = c.ix.subsample(c.r, SUBSAMPLE_SEED, want_keep=True, want_owner=True)
    return {"kept": kept, "keep": keep.astype(np.uint8), "owner": owner}


def _local_maxima(c):
    kept, keep = c.ix.local_maxima(c.I["score"], c.r, min_score=0.25, min_neighbours=2, want_keep=True)
    return {"kept": kept, "keep": keep.astype(np.uint8)}


def _iss(c):
    kept, keep, saliency = c.ix.iss_keypoints(c.r, 1.5 * c.r, min_neighbours=2, want_saliency=True, want_keep=True)
    return {"kept": kept, "keep": keep.astype(np.uint8), "saliency": saliency}


def _fpfh(c, subset):
    fpfh, spfh, pairs = c.ix.fpfh(c.I["normals"], c.r, rows=c.I["rows"] if subset else None, want_spfh=True)
    return {"fpfh": fpfh, "spfh": spfh, "pairs": pairs}


def _moments(c, batch):
    if batch:
        got = c.ix.range_neighbourhoods(c.I["queries"], c.I["radii"], normals=True, centroids=True, mean_dist=True, counts=True)
    else:
        got = c.ix.range_neighbourhoods_self(c.r, normals=True, centroids=True, mean_dist=True, counts=True)
    return dict(zip(("normals", "centroids", "mean_dist", "counts"), got))


def _features(c, batch):
    if batch:
        got = c.ix.shape_features(c.I["queries"], c.I["radii"], normals=True, axes=True, counts=True)
    else:
        got = c.ix.shape_features_self(c.r, normals=True, axes=True, counts=True)
    return dict(zip(("evals", "curvature", "normals", "axes", "counts"), got))


# registration against the handle's cloud
ICP_ITERATIONS = 4


def _nearest(c, pose):
    partner, d2 = c.ix.nearest_posed(c.I["source"], 2.0 * c.r, pose, want_d2=True)
    return {"partner": partner, "d2": d2}


def _icp(c, plane):
    got = c.ix.icp(c.I["source"], 2.0 * c.r, None, ICP_ITERATIONS, normals=c.I["normals"] if plane else None, want_partner=True)
    out = {"transform": got["transform"].reshape(16), "words": np.array([got["status"], got["iterations"], got["last_count"]], np.uint32),
           "count": got["count"], "rms": got["rms"], "partner": got["partner"]}
    # the _dev loop: its scratch is a lease of the device's pool on the handle's stream; beyond the updates made its traces hold 0 and NaN
    m = len(c.I["source"])
    src, nrm, xf, words = c.up(c.I["source"]), c.up(c.I["normals"]) if plane else None, c.out(16, "f64"), [c.out(1, "u32") for _ in range(3)]
    count, rms, partner = c.out(ICP_ITERATIONS, "u32"), c.out(ICP_ITERATIONS, "f64"), c.out(m, "u32")
    c.ready()
    c.ix.icp_dev(src, m, 2.0 * c.r, xf, max_iterations=ICP_ITERATIONS, d_normals=nrm, d_status=words[0], d_iterations=words[1], d_last_count=words[2],
                 d_count=count, d_rms=rms, d_partner=partner)
    c.drain()
    out.update({"dev_transform": c.down(xf, 16), "dev_words": np.concatenate([c.down(w, 1) for w in words]), "dev_count": c.down(count, ICP_ITERATIONS),
                "dev_rms": c.down(rms, ICP_ITERATIONS), "dev_partner": c.down(partner, m)})
    return out


# ---- the rows without a handle: their scratch is the device's pool and its leases; they take the cloud's arrays as plain inputs -------
BILATERAL = dict(n=3000, seed=7, sigmaf=0.08, sigmag=0.02, K=1)  # (a case of tests/test_gpu_filters.py: one round has no boundary flips)
WLOP = dict(n=2000, I=500, seed=22, mu=0.45, h=0.25, k=1)


def filter_cloud():
    import test_gpu_filters as TF
    return TF._surface_cloud(BILATERAL["n"], BILATERAL["seed"])


def _bilateral(c, normals_mode):
    f = c.pkg.bilateral_filter_normals if normals_mode else c.pkg.bilateral_filter_points
    pts, nrm = filter_cloud()
    return {"out": f(pts, nrm, BILATERAL["sigmaf"], BILATERAL["sigmag"], K=BILATERAL["K"])}


def wlop_case():
    import test_gpu_filters as TF
    return TF._wlop_case(WLOP["n"], WLOP["I"], WLOP["seed"])


def _wlop(c):
    pts, sample = wlop_case()
    return {"out": c.pkg.wlop(pts, mu=WLOP["mu"], h=WLOP["h"], k=WLOP["k"], uniform=True, sample=sample)}


HIERARCHY = dict(n=1000, seed=42, cluster_size=5, var_max=1.0 / 3.0)  # (uniform_1e3 of tests/test_gpu_hierarchy.py)


def _hierarchy(c):
    pts = c.pkg.synthetic.uniform_cloud(HIERARCHY["n"], HIERARCHY["seed"])
    out, idx = c.pkg.hierarchy_simplification(pts, HIERARCHY["cluster_size"], HIERARCHY["var_max"], return_indices=True)
    return {"points": out, "idx": idx}


MATCH_DIMS, MATCH_M, MATCH_N = 33, 65, 1000


def match_sets():
    import test_gpu_match as TM
    src, tgt = TM._sets("fpfh", MATCH_DIMS)
    return src[:MATCH_M], tgt[:MATCH_N]


def _match(c):
    out = dict(zip(("idx", "d2", "second_idx", "second_d2"), c.pkg.match_nearest(*match_sets())))
    out["pairs"], out["pairs_d2"] = c.pkg.match_correspondences(*match_sets(), 1.0, True)
    return out


RANSAC = dict(kind="noisy", C=1400, T=1024, s=0.9)


def _ransac_rigid(c):
    import test_gpu_register as TR
    out = TR._launch(c.pkg, RANSAC["kind"], RANSAC["C"], RANSAC["T"], RANSAC["s"], refit=True)  # (on torch's stream: a queued lease)
    c.ready()
    got = TR._read(out)
    return {"words": np.array([got["found"], got["h"], got["score"], got["ninl"]], np.int64), "inliers": got["inliers"], "rest": got["rest"],
            "xf": got["xf"], "refit": got["refit"]}


def fit_set():
    import planes_cases
    return planes_cases.fit_sets()[2][1]


def fit_pairs():
    import fit_bits_cases
    return fit_bits_cases.inputs("fit_all_n16385")  # (a clean set: the first size where a thread of the sums adds two items)


def _fits(c):
    S = fit_pairs()
    xf, rms = c.pkg.rigid_fit(S["P"], S["Q"], S["pairs"])
    plane, prms = c.pkg.plane_fit(fit_set())
    return {"rigid": xf.reshape(16), "rigid_rms": np.array([rms]), "plane": plane, "plane_rms": np.array([prms])}


PLANE = dict(kind="noisy", variant="all", C=1000, T=1024)


def _ransac_plane(c):
    import test_gpu_planes as TP
    out = TP._launch(c.pkg, PLANE["kind"], PLANE["variant"], PLANE["C"], PLANE["C"], PLANE["T"], refit=True)
    c.ready()
    got = TP._read(out)
    return {"words": np.array([got["found"], got["h"], got["score"], got["ninl"]], np.int64), "inliers": got["inliers"], "rest": got["rest"],
            "plane": got["plane"], "refit": got["refit"]}


PEEL_T = 256


def _extract_planes(c):
    import planes_cases as PC
    got = c.pkg.extract_planes(PC.peel_scene()[0], PEEL_T, PC.PEEL["max_distance"], PC.PEEL["min_inliers"], PC.PEEL["max_planes"], seed=PC.PEEL["seed"],
                               refit=True)
    return {"labels": got["labels"], "planes": got["planes"], "scores": got["scores"], "refits": got["refits"]}


KD_DIMS, KD_K = 6, 5
_kd = {}


def kd_sets():
    rng = np.random.default_rng(61)
    return rng.uniform(0, 1, (1300, KD_DIMS)).astype(F), rng.uniform(0, 1, (QUERIES, KD_DIMS)).astype(F)


def _kd_knn(c):
    if "tree" not in _kd:
        _kd["tree"] = c.pkg.KdTreeK(kd_sets()[0])
    idx, cnt, d2 = _kd["tree"].nearest_neighbours(kd_sets()[1], KD_K, EPS, want_d2=True)
    return {"idx": idx, "cnt": cnt, "d2": d2}


# name -> (family, callable).  Families: "knn" rows rest on a kNN set (KNN_CLOUDS only: no ties, every point indexed); "any" rows run
# on every cloud; "free" rows take no handle.
ROWS = {
    "knn_dev_k8": ("knn", lambda c: _knn_dev(c, 8)),
    "knn_dev_k32": ("knn", lambda c: _knn_dev(c, 32)),
    "knn_dev_k40": ("knn", lambda c: _knn_dev(c, 40)),  # (the multi-pass form: Index::d_multi)
    "knn_strided_k15": ("knn", lambda c: _knn_dev(c, 15, 16)),
    "knn_curve_k8": ("knn", lambda c: _knn_curve(c, 8)),
    "knn_batch_k8": ("knn", lambda c: _knn_host(c, c.I["many_queries"], 8)),
    "knn_one_k8": ("knn", lambda c: _knn_host(c, c.I["queries"][:1], 8)),  # (the latency path)
    "count_batch": ("any", lambda c: {"cnt": c.ix.range_count(c.I["queries"], c.r)}),
    "count_self_dev": ("any", _count_dev),  # (both orders)
    "lists_self_dev": ("any", _lists_dev),
    "sphere_batch": ("any", lambda c: _sorted_lists(*c.ix.range_sphere(c.I["queries"], c.I["radii"]))),
    "aabb_batch": ("any", lambda c: _sorted_lists(*c.ix.range_aabb(c.I["boxes"]))),
    "normals_knn_dev": ("knn", lambda c: _normals_dev(c, 15, False)),
    "normals_knn_gather_dev": ("knn", lambda c: _normals_dev(c, 15, True)),
    "neighbourhoods_dev": ("knn", lambda c: _neighbourhoods_dev(c, 15)),
    "oriented_normals": ("knn", lambda c: _oriented(c, 8)),
    "reconstruct_dev": ("knn", _reconstruct_dev),  # (the host form sizes the mesh first)
    "surface_hint": ("knn", _hint),
    "cluster_m1_compact": ("any", lambda c: _cluster(c, 1, True)),
    "cluster_m5_plain_dev": ("any", lambda c: _cluster_dev(c, 5, False)),
    "segment": ("any", lambda c: _segment(c, False)),
    "segment_curvature": ("any", lambda c: _segment(c, True)),
    "subsample": ("any", _subsample),
    "local_maxima": ("any", _local_maxima),
    "iss": ("any", _iss),
    "fpfh_all": ("any", lambda c: _fpfh(c, False)),
    "fpfh_subset": ("any", lambda c: _fpfh(c, True)),
    "moments_self": ("any", lambda c: _moments(c, False)),
    "moments_batch": ("any", lambda c: _moments(c, True)),
    "features_self": ("any", lambda c: _features(c, False)),
    "features_batch": ("any", lambda c: _features(c, True)),
    "nearest_posed": ("any", lambda c: _nearest(c, POSE)),
    "icp_point": ("any", lambda c: _icp(c, False)),  # (host and _dev forms)
    "icp_plane": ("any", lambda c: _icp(c, True)),
    "bilateral_points": ("free", lambda c: _bilateral(c, False)),
    "bilateral_normals": ("free", lambda c: _bilateral(c, True)),
    "wlop": ("free", _wlop),
    "hierarchy": ("free", _hierarchy),
    "match": ("free", _match),  # (nearest and correspondences)
    "ransac_rigid_dev": ("free", _ransac_rigid),
    "fits": ("free", _fits),  # (rigid_fit and plane_fit)
    "ransac_plane_dev": ("free", _ransac_plane),
    "extract_planes": ("free", _extract_planes),
    "kd_knn": ("free", _kd_knn),
}
HOME = {"knn": "c5000", "any": "c5000g", "free": "c70"}  # the cloud of groups A and B
EMPTY_OK = ("cluster_m1_compact", "cluster_m5_plain_dev", "segment", "subsample", "local_maxima", "iss", "fpfh_all", "moments_self",
            "features_self")  # the rows that run on the empty cloud (the early returns of host_forms_cases' n0)
LARGE_OK = ("knn_dev_k8", "knn_curve_k8", "count_self_dev")  # the rows that run on c33000


def runs_on(row, cloud):
    family = ROWS[row][0]
    if cloud == "c0":
        return row in EMPTY_OK
    if cloud == "c33000":
        return row in LARGE_OK
    return family != "knn" or cloud in KNN_CLOUDS


def run(pkg, ix, cloud, row):
    """the row's outputs on the handle (which holds the cloud): a dict of contiguous numpy arrays"""
    assert runs_on(row, cloud), (row, cloud)
    return {k: np.ascontiguousarray(v) for k, v in ROWS[row][1](Ctx(pkg, ix, cloud)).items()}


_fresh = {}


def fresh(pkg, cloud, row):
    """the row's outputs on a handle that did nothing else before, made once"""
    cloud = HOME["free"] if ROWS[row][0] == "free" else cloud
    if (cloud, row) not in _fresh:
        ix = build(pkg, cloud)
        _fresh[(cloud, row)] = run(pkg, ix, cloud, row)
        ix.close()
    return _fresh[(cloud, row)]


def same_bits(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key, a in got.items():
        w = want[key]
        assert a.dtype == w.dtype and a.shape == w.shape, (what, key, a.dtype, w.dtype, a.shape, w.shape)
        bad = np.nonzero((bits(a) != bits(w)).reshape(-1))[0]
        assert len(bad) == 0, (what, key, len(bad), bad[:8].tolist(), a.reshape(-1)[bad[:8]].tolist(), w.reshape(-1)[bad[:8]].tolist())


# ---- the sequences of group D: six seeds, 24 rows each on one handle, with what lies between them ---------------------------------------
SEQUENCE_SEEDS = (17, 18, 19, 20, 21, 22)  # (chosen on the CPU so that the coverage holds: tests/test_handle_history_cpu.py)
STEPS = 24
# seed -> the cloud the handle is made on, and {step: the cloud it is rebuilt to before that step's row}
ROUTES = {
    17: ("c1300", {5: "c5000", 10: "c5000g", 15: "c70", 20: "c1300b"}),
    18: ("c5000g", {6: "c0", 8: "c5000g", 14: "c5000", 19: "c1300"}),
    19: ("c70", {4: "c1300", 9: "c1300b", 14: "c33000", 18: "c5000"}),
    20: ("c5000", {6: "c5000g", 12: "c0", 14: "c70", 19: "c5000g"}),
    21: ("c33000", {4: "c1300", 10: "c5000g", 16: "c5000"}),
    22: ("c5000g", {5: "c1300b", 10: "c5000", 15: "c70", 20: "c5000g"}),
}
SWITCHES = {"long_groups_first": (0, 1), "gather_outputs": (0, 1), "eps_test_mode": (0, 1, 2)}
REPEATS = 3  # a cloud of 512 groups or more begins with the same self-kNN this many times: recorded, ordered, handed out by the order
TRANSITIONS = ("grow", "shrink", "same_size", "to_empty", "from_empty", "grid_on", "grid_off")


def transitions(a, b):
    """what a rebuild from cloud a to cloud b is"""
    na, nb = SIZES[a], SIZES[b]
    out = set()
    if nb == 0:
        out.add("to_empty")
    elif na == 0:
        out.add("from_empty")
    elif nb > na:
        out.add("grow")
    elif nb < na:
        out.add("shrink")
    elif a != b:
        out.add("same_size")
    if gridded(b) and not gridded(a):
        out.add("grid_on")
    if gridded(a) and not gridded(b) and nb > 0:
        out.add("grid_off")
    return out


@functools.lru_cache(maxsize=None)
def plans():
    """seed -> (first cloud, the steps); a step is (the actions before its row, the cloud it runs on, the row), an action ("rebuild",
    cloud), ("set", switch, value) or ("poison", byte).  Made for all seeds at once: a row is drawn among those that run on the handle's
    cloud and have been seen after the fewest different rows so far, so that the six sequences together reach the coverage that
    tests/test_handle_history_cpu.py asserts."""
    seen = {r: set() for r in ROWS}  # row -> the rows it has followed
    out = {}
    for seed in SEQUENCE_SEEDS:
        rng = np.random.default_rng(seed)
        cloud, route = ROUTES[seed]
        state = {"long_groups_first": 1, "gather_outputs": 0, "eps_test_mode": 0}
        steps, prev, forced = [], None, REPEATS if cloud == "c33000" else 0
        for i in range(STEPS):
            actions = []
            if i in route:
                cloud = route[i]
                actions.append(("rebuild", cloud))
                if cloud == "c33000":
                    forced = REPEATS
                    if not state["long_groups_first"]:
                        state["long_groups_first"] = 1
                        actions.append(("set", "long_groups_first", 1))
            if forced:
                row = "knn_dev_k8"
                forced -= 1
            else:
                if i % 4 == 1:
                    name = list(SWITCHES)[int(rng.integers(len(SWITCHES)))]
                    others = [v for v in SWITCHES[name] if v != state[name]]
                    state[name] = others[int(rng.integers(len(others)))]
                    actions.append(("set", name, state[name]))
                if i % 6 == 3:
                    actions.append(("poison", (0x00, 0x55, 0xFF)[int(rng.integers(3))]))
                can = [r for r in ROWS if runs_on(r, cloud)]
                new = [r for r in can if prev not in seen[r]] or can
                least = min(len(seen[r]) for r in new)
                pool = [r for r in new if len(seen[r]) == least]
                row = pool[int(rng.integers(len(pool)))]
            if prev is not None:
                seen[row].add(prev)
            steps.append((tuple(actions), cloud, row))
            prev = row
        out[seed] = (ROUTES[seed][0], tuple(steps))
    return out


def coverage():
    """(rows that occur, row -> the rows it follows, the rebuild transitions) over the six sequences"""
    occur, follows, moves = set(), {r: set() for r in ROWS}, set()
    for first, steps in plans().values():
        cloud, prev = first, None
        for actions, at, row in steps:
            for a in actions:
                if a[0] == "rebuild":
                    moves |= transitions(cloud, a[1])
                    cloud = a[1]
            assert at == cloud and runs_on(row, cloud)
            occur.add(row)
            if prev is not None:
                follows[row].add(prev)
            prev = row
    return occur, follows, moves
