"""The cases that pin the bits of the float64 fits (tests/test_gpu_fit_bits.py; the fixture tests/golden/fit_bits.npz is written
by tests/golden/make_fit_bits.py).  Every result bit of a fit depends on one fixed order of additions -- a thread adds its items a
grid stride apart in ascending order, 256 threads are added by a fixed tree, 64 blocks in block order -- so the sizes are the
smallest at which each part of that order can go wrong: 257 is the first size where a second block has an item, 16 385 the first
where a thread adds two, 33 000 gives three trips to some threads and two to others.  Seeded inputs, built once, never changed; only
the public Python API is called."""
import functools
import zlib

import numpy as np

import icp_model
import planes_cases

F = np.float32
FIT_SIZES = (3, 17, 255, 257, 16384, 16385, 33000)
LIST_SIZES = (16385, 33000)
DEV_CAPACITY, DEV_COUNT = 17000, 16385  # the device-side count is smaller than the capacity
OFFSET = np.array([500.0, -3.0, 20.0])  # far from the origin: the sums are not trivially exact
RANSAC_RIGID = dict(C=1535, T=4096, s=0.9)
RANSAC_PLANE = dict(frac=0.5, T=1024)
PEEL_T = 1024
ICP_PLANE = dict(target=4000, source=16385, radius=0.5, iterations=3)

CASES = (["fit_all_n%d" % n for n in FIT_SIZES] + ["fit_list_n%d" % n for n in LIST_SIZES] +
         ["fit_dev", "ransac_rigid", "ransac_plane", "extract_planes", "icp_plane", "icp_point"])


def _rotation(rng):
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return A * np.sign(np.linalg.det(A))


def _pairs_set(n, seed):
    """P uniform in a 2 x 4 x 1 box at OFFSET, Q its rigidly moved noisy copy, pairs (n, 2): P row k with the Q row that belongs to it"""
    rng = np.random.default_rng(seed)
    P = (rng.uniform(-1, 1, (n, 3)) * [1.0, 2.0, 0.5] + OFFSET).astype(F)
    A, t = _rotation(rng), rng.uniform(-1, 1, 3)
    Q = (P.astype(np.float64) @ A.T + t + rng.normal(0, 0.01, (n, 3))).astype(F)
    pairs = np.stack([np.arange(n), rng.permutation(n)], 1).astype(np.uint32)
    Qp = np.empty_like(Q)
    Qp[pairs[:, 1]] = Q
    return rng, P, Qp, pairs


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the input arrays of a case, by name"""
    if name.startswith("fit_all_n"):
        _rng, P, Q, pairs = _pairs_set(int(name[len("fit_all_n"):]), 100)
        return _frozen({"P": P, "Q": Q, "pairs": pairs})
    if name.startswith("fit_list_n"):
        n = int(name[len("fit_list_n"):])
        rng, P, Q, pairs = _pairs_set(n, 200)
        # a shuffled half of the items, one position out of range and one row with a NaN coordinate: the skipped-item path
        lst = rng.permutation(n)[:n // 2].astype(np.uint32)
        lst[100] = n + 7
        P[lst[200], 1] = np.nan
        assert pairs[lst[200], 0] == lst[200]
        return _frozen({"P": P, "Q": Q, "pairs": pairs, "list": lst})
    if name == "fit_dev":
        rng, P, Q, pairs = _pairs_set(DEV_CAPACITY, 300)
        return _frozen({"P": P, "Q": Q, "pairs": pairs, "rows": rng.permutation(DEV_CAPACITY).astype(np.uint32)})
    if name == "ransac_rigid":
        import test_gpu_register as R  # (its "noisy" set)
        P, Q, pairs, tau = R._set("noisy")
        return _frozen({"P": P.copy(), "Q": Q.copy(), "pairs": pairs[:RANSAC_RIGID["C"]].copy(), "tau": np.array([tau]), "seed": np.array([R.SEED])})
    if name == "ransac_plane":
        return _frozen({"P": planes_cases.noisy_scene(RANSAC_PLANE["frac"])[0].copy()})
    if name == "extract_planes":
        return _frozen({"P": planes_cases.peel_scene()[0].copy()})
    if name == "icp_plane":
        target, normals = icp_model.surface(ICP_PLANE["target"], 31)
        rng = np.random.default_rng(32)
        inv = np.linalg.inv(icp_model.rigid([0.2, 1.0, -0.4], 3.0, [0.02, -0.03, 0.01]))
        on = target[rng.integers(0, len(target), ICP_PLANE["source"])].astype(np.float64) + rng.normal(0, 0.003, (ICP_PLANE["source"], 3))
        return _frozen({"target": target, "normals": normals, "source": (on @ inv[:3, :3].T + inv[:3, 3]).astype(F)})
    if name == "icp_point":
        target, _normals, _rows, source, _truth, _extent = icp_model.recovery_scene()
        return _frozen({"target": target.copy(), "source": source.copy()})
    raise KeyError(name)


def crc(name):
    """CRC32 of the input arrays' bytes, in the order of their names"""
    c = 0
    for key, a in sorted(inputs(name).items()):
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.array([c], np.uint32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _fit_pair(pkg, P, Q, pairs, lst=None):
    xf, rms = pkg.rigid_fit(P, Q, pairs, lst)
    plane, prms = pkg.plane_fit(P, lst)
    return {"rigid": xf.reshape(16), "rigid_rms": np.array([rms]), "plane": plane, "plane_rms": np.array([prms])}


def _fit_dev(pkg, I):
    import torch
    dev = torch.device("cuda", 0)
    d_P, d_Q = torch.from_numpy(I["P"].copy()).to(dev), torch.from_numpy(I["Q"].copy()).to(dev)
    d_pairs, d_rows = torch.from_numpy(I["pairs"].view(np.int32).copy()).to(dev), torch.from_numpy(I["rows"].view(np.int32).copy()).to(dev)
    d_count = torch.tensor([DEV_COUNT], dtype=torch.int64).to(dev)
    d_xf, d_rms, d_plane, d_prms = (torch.full((k,), 7.0, dtype=torch.float64, device=dev) for k in (16, 1, 4, 1))
    pkg.rigid_fit_dev(d_P, DEV_CAPACITY, d_Q, DEV_CAPACITY, d_pairs, DEV_CAPACITY, d_xf, d_count=d_count, d_rms=d_rms)
    pkg.plane_fit_dev(d_P, DEV_CAPACITY, d_plane, d_rows=d_rows, rows_capacity=DEV_CAPACITY, d_rows_count=d_count, d_rms=d_prms)
    torch.cuda.synchronize()
    out = {"rigid": d_xf.cpu().numpy(), "rigid_rms": d_rms.cpu().numpy(), "plane": d_plane.cpu().numpy(), "plane_rms": d_prms.cpu().numpy()}
    # the host forms over the same prefix
    xf, rms = pkg.rigid_fit(I["P"], I["Q"], I["pairs"][:DEV_COUNT])
    plane, prms = pkg.plane_fit(I["P"], I["rows"][:DEV_COUNT])
    out.update({"host_rigid": xf.reshape(16), "host_rigid_rms": np.array([rms]), "host_plane": plane, "host_plane_rms": np.array([prms])})
    return out


def _extract(pkg, P):
    import torch
    first = pkg.extract_planes(P, PEEL_T, planes_cases.PEEL["max_distance"], planes_cases.PEEL["min_inliers"], planes_cases.PEEL["max_planes"],
                               seed=planes_cases.PEEL["seed"], refit=True)
    found = len(first["planes"])
    rounds = found + 2  # two dead rounds: the fit's gated launches run and must leave the zeroed entries alone
    got = pkg.extract_planes(P, PEEL_T, planes_cases.PEEL["max_distance"], planes_cases.PEEL["min_inliers"], rounds, seed=planes_cases.PEEL["seed"], refit=True)
    out = {"found": np.array([found], np.uint32), "labels": got["labels"], "planes": got["planes"], "scores": got["scores"], "refits": got["refits"]}
    # the device form keeps the entries of the dead rounds
    dev = torch.device("cuda", 0)
    prm = pkg.planes.plane_params(PEEL_T, planes_cases.PEEL["max_distance"], seed=planes_cases.PEEL["seed"], refit=True, min_inliers=planes_cases.PEEL["min_inliers"],
                                  max_planes=rounds)
    d_P = torch.from_numpy(P.copy()).to(dev)
    d_labels, d_count = torch.full((len(P),), 5, dtype=torch.int32, device=dev), torch.full((1,), 5, dtype=torch.int32, device=dev)
    d_planes, d_refits = (torch.full((rounds, 4), 7.0, dtype=torch.float64, device=dev) for _ in range(2))
    d_scores = torch.full((rounds,), 5, dtype=torch.int32, device=dev)
    pkg.extract_planes_dev(d_P, len(P), prm, d_labels, d_count, d_planes=d_planes, d_refits=d_refits, d_scores=d_scores)
    torch.cuda.synchronize()
    out.update({"dev_count": d_count.cpu().numpy().view(np.uint32), "dev_labels": d_labels.cpu().numpy().view(np.uint32),
                "dev_planes": d_planes.cpu().numpy(), "dev_refits": d_refits.cpu().numpy(), "dev_scores": d_scores.cpu().numpy().view(np.uint32)})
    return out


def _icp(pkg, target, source, radius, iterations, normals=None):
    ix = pkg.Index(target)
    got = ix.icp(source, radius, None, iterations, normals=normals)
    ix.close()
    return {"transform": got["transform"].reshape(16), "words": np.array([got["status"], got["iterations"], got["last_count"]], np.uint32),
            "count": got["count"], "rms": got["rms"]}


def run(pkg, name):
    """the outputs of a case on the GPU: a dict of numpy arrays"""
    I = inputs(name)
    if name.startswith("fit_all_n"):
        return _fit_pair(pkg, I["P"], I["Q"], I["pairs"])
    if name.startswith("fit_list_n"):
        return _fit_pair(pkg, I["P"], I["Q"], I["pairs"], I["list"])
    if name == "fit_dev":
        return _fit_dev(pkg, I)
    if name == "ransac_rigid":
        got = pkg.ransac_rigid(I["P"], I["Q"], I["pairs"], RANSAC_RIGID["T"], float(I["tau"][0]), seed=int(I["seed"][0]), edge_similarity=RANSAC_RIGID["s"],
                               refit=True)
        return {"words": np.array([got["found"], got["hypothesis"], len(got["inliers"])], np.uint32), "inliers": got["inliers"],
                "transform": got["transform"].reshape(16), "refit": got["refit"].reshape(16)}
    if name == "ransac_plane":
        got = pkg.ransac_plane(I["P"], RANSAC_PLANE["T"], refit=True, **planes_cases.NOISY_ARGS)
        return {"words": np.array([got["found"], got["hypothesis"], len(got["inliers"])], np.uint32), "inliers": got["inliers"], "plane": got["plane"],
                "refit": got["refit"]}
    if name == "extract_planes":
        return _extract(pkg, I["P"])
    if name == "icp_plane":
        return _icp(pkg, I["target"], I["source"], ICP_PLANE["radius"], ICP_PLANE["iterations"], I["normals"])
    if name == "icp_point":
        return _icp(pkg, I["target"], I["source"], icp_model.RECOVERY_RADIUS, icp_model.RECOVERY_ITERATIONS)
    raise KeyError(name)
