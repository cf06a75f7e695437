#!/usr/bin/env python3
"""Boundary points (include/pcpx_boundary.h) on one device: the uniform cloud of section 16 at --n points
(r = 0.01 at 10 M, scaled by (10 M / n)^(1/3) for another n: ~42 neighbours) and the Stanford bunny (at its median 20th-neighbour
distance), the normals those of range_neighbourhoods_self_dev at the same radius.  The variants ALTERNATE in one process
(a, b, c, a, b, c, ...), each call timed by a pair of device events after warm-up; beside every median stands the spread of the same
code in that run (the medians of its even and of its odd calls).
  boundary_dev          keep + kept rows + count, and the same with gap, counts and sector masks written as well
  the count walk        pcpx_range_count_self_dev at the same radius: the same spheres, the pair test alone
  the features walk     pcpx_shape_features_self_dev (eigenvalues and curvature) at the same radius: the moments per accepted pair
  the path it replaces  range lists on the host (range_sphere over all points) and the numpy model over the lists, host clock; at
                        --baseline-n points (the lists of 10 M points at ~42 neighbours are 424 M entries) and on the bunny
No rate is asserted anywhere: the ratios to the count walk are what the run records.
python tools/boundary_rate.py [--n N] [--baseline-n N] [--rounds R] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import boundary_model as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=float, default=10e6)
ap.add_argument("--baseline-n", type=float, default=1e6)
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_boundary.json"))
a = ap.parse_args()
pkg = importlib.import_module("point-cloud-processing_amd")
dev = torch.device("cuda", 0)
F = np.float32


def alternating(variants, rounds=a.rounds):
    """{name: fn} -> {name: {median, min, max, same-code spread}} in milliseconds: two warm-up calls each, then `rounds` rounds of
    every variant in turn, each call between two events"""
    names = list(variants)
    for _ in range(2):
        for name in names:
            variants[name]()
    torch.cuda.synchronize()
    events = {name: [] for name in names}
    for _ in range(rounds):
        for name in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            variants[name]()
            e1.record()
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for name in names:
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in events[name]])
        med = float(np.median(ms))
        out[name] = {"median_ms": round(med, 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
                     "same code, even against odd calls_%": round(100.0 * abs(float(np.median(ms[0::2])) - float(np.median(ms[1::2]))) / med, 2)}
    return out


def from_lists(pts, nrm, off, idx, gap_sectors):
    """the model's keep mask from materialised range lists: what a caller had to do on the host"""
    counts = np.diff(off.astype(np.int64))
    centre = np.repeat(np.arange(len(pts)), counts)
    has, u, v = M.frames(nrm)
    d = pts[idx] - pts[centre]
    uu, vv = u[centre], v[centre]
    a_ = (d[:, 0] * uu[:, 0] + d[:, 1] * uu[:, 1]) + d[:, 2] * uu[:, 2]
    b_ = (d[:, 0] * vv[:, 0] + d[:, 1] * vv[:, 1]) + d[:, 2] * vv[:, 2]
    directed = ~((a_ == 0) & (b_ == 0))
    bit = np.where(directed, np.uint64(1) << M.sector(a_, b_).astype(np.uint64), np.uint64(0))
    masks = np.bitwise_or.reduceat(bit, off[:-1].astype(np.int64))  # (every list holds its centre: none is empty)
    G, _start = M.gap_and_start(masks)
    return has & (G >= gap_sectors)


def measure(name, pts, r, baseline):
    n = len(pts)
    d_pts = torch.from_numpy(pts).to(dev)
    ix = pkg.Index.from_device(d_pts.data_ptr(), n)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ix.range_neighbourhoods_self_dev(r, d_normals=nrm.data_ptr())
    ix.synchronize()
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    rows = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    gap = torch.empty(2 * n, dtype=torch.uint8, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    sec = torch.empty(n, dtype=torch.int64, device=dev)
    evals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    curv = torch.empty(n, dtype=torch.float32, device=dev)
    t = alternating({
        "pcpx_range_count_self_dev": lambda: ix.range_count_self_dev(r, cnt.data_ptr()),
        "pcpx_shape_features_self_dev (eigenvalues, curvature)": lambda: ix.shape_features_self_dev(r, evals.data_ptr(), curv.data_ptr()),
        "boundary_dev (keep, kept rows, count)": lambda: ix.boundary_dev(nrm, r, keep, 16, 5, d_kept_rows=rows, d_kept_count=total),
        "boundary_dev (every output)": lambda: ix.boundary_dev(nrm, r, keep, 16, 5, d_kept_rows=rows, d_kept_count=total, d_gap=gap, d_count=cnt,
                                                               d_sectors=sec),
    })
    count_ms = t["pcpx_range_count_self_dev"]["median_ms"]
    out = {"points": n, "radius": r, "mean count at the radius": round(float(cnt.double().mean().item()), 2), "kept": int(total.item()),
           "device events, alternating": t,
           "boundary / count walk": round(t["boundary_dev (keep, kept rows, count)"]["median_ms"] / count_ms, 4),
           "boundary (every output) / count walk": round(t["boundary_dev (every output)"]["median_ms"] / count_ms, 4),
           "features walk / count walk": round(t["pcpx_shape_features_self_dev (eigenvalues, curvature)"]["median_ms"] / count_ms, 4)}
    ix.profile_begin()
    ix.boundary_dev(nrm, r, keep, 16, 5, d_kept_rows=rows, d_kept_count=total)
    ix.synchronize()
    out["the index's own profile of one call (launches, ms)"] = {k: v for k, v in ix.profile_end().items() if v[0]}
    if baseline:
        h_nrm = nrm.cpu().numpy()
        t0 = time.perf_counter()
        off, idx = ix.range_sphere(pts, r)
        t1 = time.perf_counter()
        want = from_lists(pts, h_nrm, off, idx, 16) & (np.diff(off.astype(np.int64)) >= 5)
        t2 = time.perf_counter()
        kept = ix.boundary(h_nrm, r, 16, 5)
        t3 = time.perf_counter()
        out["the path it replaces, host clock"] = {"list entries": int(off[-1]), "range lists to the host_ms": round(1e3 * (t1 - t0), 1),
                                                  "numpy over the lists_ms": round(1e3 * (t2 - t1), 1),
                                                  "Index.boundary (host arrays, one call)_ms": round(1e3 * (t3 - t2), 2),
                                                  "same kept rows": bool(np.array_equal(np.flatnonzero(want), kept))}
    print(name, json.dumps(out), flush=True)
    ix.close()
    return out


res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
       "timing": "device events round each call, variants alternating in one process, medians; milliseconds", "clouds": {}}
n = int(a.n)
res["clouds"]["uniform, %d points" % n] = measure("uniform", pkg.synthetic.uniform_cloud(n, 43), float(F(0.01 * (10e6 / n) ** (1.0 / 3.0))), False)
torch.cuda.empty_cache()
m = int(a.baseline_n)
res["clouds"]["uniform, %d points (with the path it replaces)" % m] = measure(
    "uniform, baseline", pkg.synthetic.uniform_cloud(m, 43), float(F(0.01 * (10e6 / m) ** (1.0 / 3.0))), True)
bunny = pkg.ply.read_ply(os.path.join(ROOT, "tests", "golden", "stanford_bunny.ply"))[0]
ix = pkg.Index(bunny)
sample = bunny[np.random.default_rng(1).choice(len(bunny), 2000, replace=False)]
r_bunny = float(np.median(np.sqrt(ix.knn(sample, 20, 0.0, want_d2=True)[2][:, 19])))
ix.close()
res["clouds"]["bunny, %d points" % len(bunny)] = measure("bunny", bunny, r_bunny, True)

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
