"""The cases that pin the outputs of the handle family's host-pointer forms and of their _dev forms (tests/test_gpu_host_forms.py;
the fixture tests/golden/host_forms.npz is written by tests/golden/make_host_forms.py): clustering, segmentation, subsampling, local
maxima, ISS keypoints, FPFH, and the range-neighbourhood and shape-feature forms.  Every output is deterministic, so it is compared
by its bits.  What is pinned is the staging around the kernels -- which arrays are staged, where each array lies in the handle's
scratch, what is copied back -- so the clouds are the smallest at which each path of it runs, none of them a workload:

    n0    no point: the early returns and what they write
    n1    one point
    n7    under one leaf: the leaf slots, not the rows, size the shared words
    n70   two query groups, the last leaf part full
    grid  300 points of which an explicit voxel grid drops those beyond x = 0.6: the rows of the outside points are preset, the rows
          outnumber the leaf slots, and the two range forms run their empty-rows kernels

A radius holds about eight points.  A case is "<cloud>.<operation>"; its recording holds every optional output, and `asks(op)`
lists the other subsets of them: an offset that depends on which outputs exist shows as a difference there.  Seeded inputs, built
once, never changed; only the public Python API is called."""
import functools
import itertools
import zlib

import numpy as np

F = np.float32
CLOUDS = {"n0": 0, "n1": 1, "n7": 7, "n70": 70, "grid": 300}
GRID = np.array([-0.01, -0.01, -0.01, 0.6, 1.01, 1.01], F)
QUERIES = 37
FILL = 7  # what a _dev output holds before the call

# operation -> (required outputs, optional outputs); "kept" is the list of kept rows, cut at the count
OUTPUTS = {
    "cluster": (("labels",), ("core", "counts", "count")),
    "segment": (("labels",), ("smooth", "count")),
    "subsample": (("keep",), ("owner", "kept", "count")),
    "local_maxima": (("keep",), ("kept", "count")),
    "iss": (("keep",), ("kept", "count", "saliency")),
    "fpfh": (("fpfh",), ("spfh", "pairs")),
    "rn": ((), ("normals", "centroids", "mean_dist", "counts")),
    "sf": ((), ("evals", "curvature", "normals", "axes", "counts")),
}
# operation -> its parameter sets, by name
PARAMS = {
    "cluster": {"m%d_%s" % (m, "c" if c else "r"): dict(min_pts=m, compact=c) for m in (1, 4) for c in (True, False)},
    "segment": {"%s_s%d_%s" % ("k" if k else "a", s, "o" if o else "u"): dict(curvature=k, min_size=s, oriented=o, compact=not o)
                for k in (True, False) for s in (1, 3) for o in (True, False)},
    "subsample": {"s5": dict(seed=5)},
    "local_maxima": {"m2": dict(min_neighbours=2)},
    "iss": {"m2": dict(min_neighbours=2)},
    "fpfh": {"all": dict(rows=None), "subset": dict(rows="some"), "none": dict(rows="none")},
    "rn": {"self": dict(), "batch_radii": dict(radii=True), "batch_one": dict(radii=False), "batch_none": dict(radii=False, nq=0)},
    "sf": {"self": dict(), "batch_radii": dict(radii=True), "batch_one": dict(radii=False), "batch_none": dict(radii=False, nq=0)},
}
# (a batch form needs an indexed point for its walk; without queries it returns before it looks)
CASES = ["%s.%s_%s" % (c, op, p) for c in CLOUDS for op in OUTPUTS for p in PARAMS[op] if not (c == "n0" and p in ("batch_radii", "batch_one"))]


def split(name):
    cloud, rest = name.split(".")
    op = next(o for o in sorted(OUTPUTS, key=len, reverse=True) if rest.startswith(o + "_"))
    return cloud, op, rest[len(op) + 1:]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


@functools.lru_cache(maxsize=None)
def inputs(cloud):
    """the input arrays of a cloud, by name"""
    n = CLOUDS[cloud]
    rng = np.random.default_rng(1000 + n)
    pts = rng.uniform(0, 1, (n, 3)).astype(F)
    if cloud == "grid":
        pts[np.abs(pts[:, 0] - 0.6) < 1e-3, 0] = F(0.5)  # (no point near the grid's face)
    radius = F(min(0.7, (1.91 / max(n, 1)) ** (1.0 / 3.0)))  # 4/3 pi r^3 n = 8
    rows = np.concatenate([np.arange(n - 1, -1, -2), [n + 3]]).astype(np.uint32)  # every other row, descending, and one >= n_in
    d = {"points": pts, "radius": np.array([radius], F), "normals": _unit(rng, n), "curvature": rng.uniform(0, 1, n).astype(F),
         "score": (np.floor(rng.uniform(0, 16, n)) / 16).astype(F),  # (ties: the lower row wins)
         "rows": rows, "queries": rng.uniform(-0.1, 1.1, (QUERIES, 3)).astype(F),
         "radii": (radius * rng.uniform(0.5, 1.5, QUERIES)).astype(F)}
    for a in d.values():
        a.setflags(write=False)
    return d


def crc(name):
    """CRC32 of the bytes of the input arrays of the case's cloud, in the order of their names"""
    c = 0
    for key, a in sorted(inputs(split(name)[0]).items()):
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.array([c], np.uint32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.kind == "f" else a


_indices = {}


def index(pkg, cloud):
    if cloud not in _indices:
        pts = inputs(cloud)["points"]
        _indices[cloud] = pkg.LinkedOctree(pts, voxel_grid=GRID) if cloud == "grid" else pkg.LinkedOctree(pts)
        if cloud == "grid":
            assert 0 < _indices[cloud].size() == int((pts[:, 0] < 0.6).sum()) < len(pts)
    return _indices[cloud]


def asks(op, dev):
    """the subsets of the optional outputs that the form can be asked for, the full one first"""
    required, optional = OUTPUTS[op]
    if dev or op in ("rn", "sf"):
        sets = [frozenset(c) for k in range(len(optional), -1, -1) for c in itertools.combinations(optional, k)]
        return [s for s in sets if s or required]
    host = {"cluster": ("core", "counts"), "segment": ("smooth",), "subsample": ("owner",), "local_maxima": (), "iss": ("saliency",)}
    if op == "fpfh":
        return [frozenset(optional), frozenset()]
    always = frozenset(optional) - frozenset(host[op])  # (the package's host methods always ask for these)
    return [always | frozenset(c) for k in range(len(host[op]), -1, -1) for c in itertools.combinations(host[op], k)]


def _fpfh_rows(I, p):
    return {None: None, "some": I["rows"], "none": np.zeros(0, np.uint32)}[p["rows"]]


def _spheres(I, p):
    nq = p.get("nq", QUERIES)
    return I["queries"][:nq], (I["radii"][:nq] if p["radii"] else float(I["radius"][0]))


def run_host(pkg, name, ask=None):
    """the asked outputs of a case from the host-pointer form: a dict of numpy arrays"""
    cloud, op, pname = split(name)
    I, ix, p = inputs(cloud), index(pkg, cloud), PARAMS[op][pname]
    ask = asks(op, False)[0] if ask is None else ask
    r = float(I["radius"][0])
    if op == "cluster":
        got = ix.cluster(r, p["min_pts"], p["compact"], want_core="core" in ask, want_counts="counts" in ask)
        out = {"labels": got[0], "count": np.array([got[1]], np.uint64)}
        rest = list(got[2:])
        if "core" in ask:
            out["core"] = rest.pop(0).astype(np.uint8)
        if "counts" in ask:
            out["counts"] = rest.pop(0)
        return out
    if op == "segment":
        got = ix.segment(I["normals"], r, min_cos=0.5, curvature=I["curvature"] if p["curvature"] else None, max_curvature=0.5,
                         min_size=p["min_size"], oriented=p["oriented"], compact=p["compact"], want_smooth="smooth" in ask)
        out = {"labels": got[0], "count": np.array([got[1]], np.uint64)}
        if "smooth" in ask:
            out["smooth"] = got[2].astype(np.uint8)
        return out
    if op == "subsample":
        got = ix.subsample(r, p["seed"], want_keep=True, want_owner="owner" in ask)
        out = {"kept": got[0], "count": np.array([len(got[0])], np.uint64), "keep": got[1].astype(np.uint8)}
        if "owner" in ask:
            out["owner"] = got[2]
        return out
    if op == "local_maxima":
        kept, keep = ix.local_maxima(I["score"], r, min_score=0.25, min_neighbours=p["min_neighbours"], want_keep=True)
        return {"kept": kept, "count": np.array([len(kept)], np.uint64), "keep": keep.astype(np.uint8)}
    if op == "iss":
        got = ix.iss_keypoints(r, 1.5 * r, min_neighbours=p["min_neighbours"], want_saliency="saliency" in ask, want_keep=True)
        out = {"kept": got[0], "count": np.array([len(got[0])], np.uint64), "keep": got[1].astype(np.uint8)}
        if "saliency" in ask:
            out["saliency"] = got[2]
        return out
    if op == "fpfh":
        got = ix.fpfh(I["normals"], r, rows=_fpfh_rows(I, p), want_spfh="spfh" in ask)
        return {"fpfh": got[0], "spfh": got[1], "pairs": got[2]} if "spfh" in ask else {"fpfh": got}
    keys = [k for k in OUTPUTS[op][1] if k in ask]
    flags = {k: k in ask for k in OUTPUTS[op][1]}
    if pname == "self":
        got = ix.range_neighbourhoods_self(r, **flags) if op == "rn" else ix.shape_features_self(r, **flags)
    else:
        q, radius = _spheres(I, p)
        got = ix.range_neighbourhoods(q, radius, **flags) if op == "rn" else ix.shape_features(q, radius, **flags)
    return dict(zip(keys, got if len(keys) > 1 else (got,)))


def run_dev(pkg, name, ask=None, count=None):
    """the asked outputs of a case from the _dev form (the batch forms have none: None).  count: where the kept rows are asked for
    without their count, the number of them that the call wrote"""
    import torch
    cloud, op, pname = split(name)
    if pname.startswith("batch"):
        return None
    I, ix, p = inputs(cloud), index(pkg, cloud), PARAMS[op][pname]
    ask = asks(op, True)[0] if ask is None else ask
    r, n, dev = float(I["radius"][0]), CLOUDS[cloud], torch.device("cuda", 0)
    kinds = {"labels": (torch.int32, 1), "core": (torch.uint8, 1), "counts": (torch.int32, 1), "count": (torch.int64, 0), "smooth": (torch.uint8, 1),
             "keep": (torch.uint8, 1), "owner": (torch.int32, 1), "kept": (torch.int32, 1), "saliency": (torch.float32, 1), "spfh": (torch.float32, 33),
             "pairs": (torch.int32, 1), "normals": (torch.float32, 3), "centroids": (torch.float32, 3), "mean_dist": (torch.float32, 1),
             "evals": (torch.float32, 3), "curvature": (torch.float32, 1), "axes": (torch.float32, 3)}
    rows = _fpfh_rows(I, p) if op == "fpfh" else None
    d = {}
    for key in OUTPUTS[op][0] + tuple(k for k in OUTPUTS[op][1] if k in ask):
        dtype, width = (torch.float32, 33) if key == "fpfh" else kinds[key]
        length = 1 if width == 0 else (len(rows) if key == "fpfh" and rows is not None else n) * width
        d[key] = torch.full((max(length, 1),), FILL, dtype=dtype, device=dev)  # (an empty tensor has no address)

    def up(a):
        a = np.ascontiguousarray(a).reshape(-1)
        a = a.view(np.int32) if a.dtype == np.uint32 else a
        t = torch.from_numpy(a.copy() if len(a) else np.zeros(1, a.dtype)).to(dev)
        torch.cuda.synchronize()  # (torch's stream is not the index's)
        return t

    ptr = lambda key: d[key].data_ptr() if key in d else None
    torch.cuda.synchronize()  # (the fills above are on torch's stream, the call below is on the index's own)
    if op == "cluster":
        ix.cluster_dev(r, ptr("labels"), p["min_pts"], p["compact"], ptr("core"), ptr("counts"), ptr("count"))
    elif op == "segment":
        d_normals, d_curv = up(I["normals"]), up(I["curvature"])
        ix.segment_dev(d_normals.data_ptr(), r, ptr("labels"), min_cos=0.5, d_curvature=d_curv.data_ptr() if p["curvature"] else None,
                       max_curvature=0.5, min_size=p["min_size"], oriented=p["oriented"], compact=p["compact"], d_smooth=ptr("smooth"),
                       d_segment_count=ptr("count"))
    elif op == "subsample":
        ix.subsample_dev(r, ptr("keep"), p["seed"], ptr("owner"), ptr("kept"), ptr("count"))
    elif op == "local_maxima":
        d_score = up(I["score"])
        ix.local_maxima_dev(d_score, r, ptr("keep"), min_score=0.25, min_neighbours=p["min_neighbours"], d_kept_rows=ptr("kept"),
                            d_kept_count=ptr("count"))
    elif op == "iss":
        ix.iss_keypoints_dev(r, 1.5 * r, ptr("keep"), min_neighbours=p["min_neighbours"], d_kept_rows=ptr("kept"), d_kept_count=ptr("count"),
                             d_saliency=ptr("saliency"))
    elif op == "fpfh":
        d_normals = up(I["normals"])
        d_rows = up(rows) if rows is not None else None
        ix.fpfh_dev(d_normals, r, ptr("fpfh"), d_rows, 0 if rows is None else len(rows), ptr("spfh"), ptr("pairs"))
    elif op == "rn":
        ix.range_neighbourhoods_self_dev(r, ptr("normals"), ptr("centroids"), ptr("mean_dist"), ptr("counts"))
    else:
        ix.shape_features_self_dev(r, ptr("evals"), ptr("curvature"), ptr("normals"), ptr("axes"), ptr("counts"))
    ix.synchronize()
    out = {}
    for key, t in d.items():
        dtype, width = (torch.float32, 33) if key == "fpfh" else kinds[key]
        a = t.cpu().numpy()
        a = a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))
        length = 1 if width == 0 else (len(rows) if key == "fpfh" and rows is not None else n) * width
        a = a[:length]
        out[key] = a.reshape(-1, width) if width > 1 else a
    if "kept" in out:  # nothing is written beyond the count
        count = int(out["count"][0]) if "count" in out else count
        assert (out["kept"][count:] == FILL).all(), name
        out["kept"] = out["kept"][:count]
    return out
