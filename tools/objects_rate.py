#!/usr/bin/env python3
"""Objects from labels (include/pcpx_objects.h) on one device: --n uniform points in the unit cube, device
arrays, four kinds of labels:
  (a) clusters      Index.cluster_dev at a radius below the percolation threshold (r = 0.65 of the mean spacing): many small clusters
  (b) groups of 64  the owners of voxel_grid_dev at the leaf that holds 64 points on average
  (c) one label     every row under the label 0
  (d) 40 % and small  a random 40 % of the rows under one label, the others under their owner of (b)
For each: label_objects_dev with the counts alone (the grouping), with counts and centroids, with the AABB beside them (what the
minima and maxima add to the pass that sums), with the covariance, and with every output; beside them the
yardstick, voxel_grid_dev (centroids and counts) on the same points at a leaf that gives the same mean group size -- for (c) and
(d) one cell, the case the tree exists for.  The variants ALTERNATE in one process (a, b, c, a, b, c, ...), each call timed by a
pair of device events after warm-up; beside every median stands the spread of the same code in that run (the medians of its even
and of its odd calls).  The path it replaces -- the labels to the host, np.unique, np.add.at -- by the host's clock, once, on (b).
No rate is asserted anywhere: the ratios are what the run records.
python tools/objects_rate.py [--n N] [--rounds R] [--out FILE] [--no-host]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=float, default=10e6)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_objects.json"))
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
pkg = importlib.import_module("point-cloud-processing_amd")
dev = torch.device("cuda", 0)
F = np.float32
NOISE = 0xFFFFFFFF


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


n = int(a.n)
pts = pkg.synthetic.uniform_cloud(n, 43)
d_pts = torch.from_numpy(pts).to(dev)
spacing = (1.0 / n) ** (1.0 / 3.0)
count = torch.zeros(1, dtype=torch.int64, device=dev)
vcount = torch.zeros(1, dtype=torch.int64, device=dev)
o = {"labels": torch.empty(n, dtype=torch.int32, device=dev), "counts": torch.empty(n, dtype=torch.int32, device=dev),
     "first": torch.empty(n, dtype=torch.int32, device=dev), "offsets": torch.empty(n + 1, dtype=torch.int32, device=dev),
     "rows": torch.empty(n, dtype=torch.int32, device=dev), "centroid": torch.empty((n, 3), dtype=torch.float64, device=dev),
     "cov": torch.empty((n, 6), dtype=torch.float64, device=dev), "aabb": torch.empty((n, 6), dtype=torch.float32, device=dev),
     "obb": torch.empty((n, 15), dtype=torch.float64, device=dev), "object": torch.empty(n, dtype=torch.int32, device=dev),
     "skipped": torch.zeros(1, dtype=torch.int64, device=dev)}
v_xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
v_counts = torch.empty(n, dtype=torch.int32, device=dev)
prm = pkg.objects.objects_params(NOISE, on_device=True)


def voxel(leaf, owner=None):
    pkg.voxel_grid_dev(d_pts, n, pkg.voxel.voxel_params(leaf, origin=(0.0, 0.0, 0.0)), n, vcount, d_xyz=v_xyz, d_counts=v_counts, d_owner=owner)


def measure(name, d_labels, leaf):
    variants = {
        "label_objects_dev (counts)": lambda: pkg.label_objects_dev(d_pts, d_labels, n, prm, n, count, d_counts=o["counts"]),
        "label_objects_dev (counts, centroids)": lambda: pkg.label_objects_dev(d_pts, d_labels, n, prm, n, count, d_counts=o["counts"],
                                                                                 d_centroid=o["centroid"]),
        "label_objects_dev (counts, centroids, AABB)": lambda: pkg.label_objects_dev(d_pts, d_labels, n, prm, n, count, d_counts=o["counts"],
                                                                                       d_centroid=o["centroid"], d_aabb=o["aabb"]),
        "label_objects_dev (counts, centroids, AABB, covariance)": lambda: pkg.label_objects_dev(
            d_pts, d_labels, n, prm, n, count, d_counts=o["counts"], d_centroid=o["centroid"], d_aabb=o["aabb"], d_cov=o["cov"]),
        "label_objects_dev (every output)": lambda: pkg.label_objects_dev(
            d_pts, d_labels, n, prm, n, count, d_labels_out=o["labels"], d_counts=o["counts"], d_first_row=o["first"], d_offsets=o["offsets"],
            d_rows=o["rows"], d_centroid=o["centroid"], d_cov=o["cov"], d_aabb=o["aabb"], d_obb=o["obb"], d_object_of_row=o["object"],
            d_skipped=o["skipped"]),
        "voxel_grid_dev (centroids, counts), leaf %.6g" % leaf: lambda: voxel(leaf),
    }
    t = alternating(variants)
    torch.cuda.synchronize()
    S, V = int(count.item()), int(vcount.item())
    sizes = o["counts"][:S].to(torch.int64)
    yard = t["voxel_grid_dev (centroids, counts), leaf %.6g" % leaf]["median_ms"]
    out = {"objects": S, "mean members": round(float(sizes.double().mean().item()), 2), "largest object": int(sizes.max().item()),
           "skipped rows": int(o["skipped"].item()), "the yardstick's cells": V, "the yardstick's mean members": round(n / max(V, 1), 2),
           "device events, alternating": t,
           "centroids / voxel_grid_dev": round(t["label_objects_dev (counts, centroids)"]["median_ms"] / yard, 4),
           "every output / voxel_grid_dev": round(t["label_objects_dev (every output)"]["median_ms"] / yard, 4)}
    print(name, json.dumps(out), flush=True)
    return out


res = {"device": torch.cuda.get_device_name(0), "points": n, "rounds": a.rounds, "plan": pkg.objects_plan(n),
       "timing": "device events round each call, variants alternating in one process, medians; milliseconds", "cases": {}}

# (b) first: its owners are the labels of (b) and the small labels of (d)
leaf64 = float(F((64.0 / n) ** (1.0 / 3.0)))
owner64 = torch.empty(n, dtype=torch.int32, device=dev)
voxel(leaf64, owner64)
torch.cuda.synchronize()
res["cases"]["(b) groups of 64: the owners of voxel_grid_dev at leaf %.6g" % leaf64] = b = measure("(b)", owner64, leaf64)

# (a) clusters below the percolation threshold
ix = pkg.Index.from_device(d_pts.data_ptr(), n)
radius = float(F(0.65 * spacing))
d_clusters = torch.empty(n, dtype=torch.int32, device=dev)
ix.cluster_dev(radius, d_clusters.data_ptr(), min_pts=1, compact=True)
ix.synchronize()
ix.close()
clusters = int(d_clusters.max().item()) + 1
leaf_a = float(F((n / clusters / n) ** (1.0 / 3.0)))  # the leaf whose cells hold as many points as a cluster on average
res["cases"]["(a) Index.cluster_dev, radius %.6g (%d clusters)" % (radius, clusters)] = measure("(a)", d_clusters, leaf_a)

# (c) one label
zeros = torch.zeros(n, dtype=torch.int32, device=dev)
res["cases"]["(c) one label holding every row"] = c = measure("(c)", zeros, 2.0)

# (d) 40 % under one label, the others small
g = torch.Generator(device=dev)
g.manual_seed(7)
big = torch.rand(n, device=dev, generator=g) < 0.4
mixed = torch.where(big, torch.zeros_like(owner64), owner64 + 1)
res["cases"]["(d) 40 % of the rows under one label, the others in groups of 64"] = d = measure("(d)", mixed, 2.0)

key = "label_objects_dev (counts, centroids)"
res["(c) against (b), centroids"] = round(c["device events, alternating"][key]["median_ms"] / b["device events, alternating"][key]["median_ms"], 4)
res["(d) against (b), centroids"] = round(d["device events, alternating"][key]["median_ms"] / b["device events, alternating"][key]["median_ms"], 4)

if not a.no_host:
    t0 = time.perf_counter()
    h_labels = owner64.cpu().numpy().view(np.uint32)
    t1 = time.perf_counter()
    uniq, inverse, h_counts = np.unique(h_labels, return_inverse=True, return_counts=True)
    t2 = time.perf_counter()
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inverse, pts)
    centroid = sums / h_counts[:, None]
    t3 = time.perf_counter()
    pkg.label_objects_dev(d_pts, owner64, n, prm, n, count, d_counts=o["counts"], d_centroid=o["centroid"])
    torch.cuda.synchronize()
    S = int(count.item())
    res["the path it replaces on (b), host clock"] = {
        "labels to the host_ms": round(1e3 * (t1 - t0), 1), "np.unique_ms": round(1e3 * (t2 - t1), 1), "np.add.at and the division_ms": round(1e3 * (t3 - t2), 1),
        "total_ms": round(1e3 * (t3 - t0), 1), "same counts": bool(S == len(uniq) and np.array_equal(o["counts"][:S].cpu().numpy().view(np.uint32), h_counts)),
        "largest centroid difference": float(np.abs(o["centroid"][:S].cpu().numpy() - centroid).max()) if S == len(uniq) else None}

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
