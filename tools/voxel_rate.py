#!/usr/bin/env python3
"""Voxel-grid downsampling (include/pcpx_voxel.h) on one device, in one run, on the seeded 10 M-point uniform
and clustered clouds of sections 16-18, at the leaves that give about 4, 16 and 64 points per occupied cell (found by bisection on the
call's own count).  Per case the device form: device-synchronised host clocks of single calls after a warm-up (median, min, max) for
the count alone (keys, the two sorts, the scan), for centroids and counts, and for every output with three attribute columns.  For
the middle leaf also what a user had before this call existed -- download, np.unique(axis=0, return_inverse=True) on the cell triples,
np.add.at, upload -- and, for context, Index.subsample at a radius of the leaf with the number of points it keeps.
Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/voxel_rate.py --trace-run
    python tools/voxel_rate.py --summarise DIR --kernels-out profiles/r21_voxel_kernels.json
python tools/voxel_rate.py [--points N] [--reps R] [--out FILE] [--no-host]"""
import argparse
import csv
import glob
import importlib
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_voxel.json"))
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--summarise", default=None)
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r21_voxel_kernels.json"))
ap.add_argument("--no-host", action="store_true", help="skip the composed host route and the subsample")
a = ap.parse_args()
PER_CELL = (4, 16, 64)
CLOUDS = (("uniform", 43), ("clustered", 44))
TRACE_CALLS = 3
KERNELS = r"\b(k_voxel_[a-z_]+|k_sort_[a-z_]+|k_scan_[a-z_]+)"


def summarise():
    """kernel_trace.csv of the traced run -> per case (the order of the traced run) the mean milliseconds of every kernel by name over
    the calls after the warm-up one, and the sorts' share.  A call begins at its k_voxel_begin."""
    rows = []
    for f in glob.glob(os.path.join(a.summarise, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        m = re.search(KERNELS, r["Kernel_Name"].replace("pcpx::(anonymous namespace)::", ""))
        if not m:
            continue
        name, ms = m.group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        if name == "k_voxel_begin":
            calls.append({"first": int(r["Start_Timestamp"]), "last": 0, "kernels": {}})
        if calls:
            k = calls[-1]["kernels"].setdefault(name, [0.0, 0])
            k[0] += ms
            k[1] += 1
            calls[-1]["last"] = int(r["End_Timestamp"])
    # (the bisection's calls come first in every case and have no per-voxel kernels: a traced case is its last 1 + TRACE_CALLS calls
    #  with k_voxel_chunks)
    full = [c for c in calls if "k_voxel_chunks" in c["kernels"]]
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own: tools/voxel_rate.py --trace-run); milliseconds per call "
                   "(and launches per call) of the call with every output and three attribute columns, mean over %d calls after one warm-up "
                   "call" % TRACE_CALLS, "cases": []}
    names = ["%s, about %d per cell" % (cloud, per) for cloud, _seed in CLOUDS for per in PER_CELL]
    for c, name in enumerate(names):
        group = full[c * (1 + TRACE_CALLS) + 1:(c + 1) * (1 + TRACE_CALLS)]
        if not group:
            continue
        kernels = {k: [round(float(np.mean([g["kernels"].get(k, [0.0, 0])[0] for g in group])), 4), group[0]["kernels"][k][1]] for k in group[0]["kernels"]}
        total = sum(v[0] for v in kernels.values())
        sorts = sum(v[0] for k, v in kernels.items() if k.startswith("k_sort_"))
        out["cases"].append({"case": name, "kernels": kernels, "all kernels of the call": round(total, 4), "the two sorts": round(sorts, 4),
                             "the sorts' share": round(sorts / total, 3),
                             "first kernel's start to last kernel's end": round(float(np.mean([(g["last"] - g["first"]) * 1e-6 for g in group])), 4)})
    with open(a.kernels_out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if a.summarise:
    summarise()
    sys.exit(0)

import torch  # noqa: E402

pkg = importlib.import_module("point-cloud-processing_amd")
capi = importlib.import_module("point-cloud-processing_amd._capi")
dev = torch.device("cuda", 0)
n = a.points


def times(fn, reps):
    """device-synchronised milliseconds of single calls after two warm-up calls: (median, min, max)"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(out)), 3), "min": round(min(out), 3), "max": round(max(out), 3)}


def host_route(d_P, d_Q, leaf):
    """download, cell triples, np.unique(axis=0, return_inverse=True), np.add.at, upload: (seconds, cells)"""
    t0 = time.perf_counter()
    P, Q = d_P.cpu().numpy(), d_Q.cpu().numpy()
    cells = np.floor((P - P.min(0)) / np.float32(leaf)).astype(np.int64)
    _u, inverse = np.unique(cells, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    V = int(inverse.max()) + 1
    sums = np.zeros((V, 6))
    np.add.at(sums, inverse, np.concatenate([P, Q], 1).astype(np.float64))
    counts = np.bincount(inverse, minlength=V)
    mean = (sums / counts[:, None]).astype(np.float32)
    d_out = torch.from_numpy(mean).to(dev)
    torch.cuda.synchronize()
    del d_out
    return time.perf_counter() - t0, V


res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "library": os.path.basename(capi.LIB_PATH), "points": n, "plan": pkg.voxel_plan(n),
       "cases": {}}
for cloud, seed in CLOUDS:
    P = pkg.synthetic.uniform_cloud(n, seed) if cloud == "uniform" else pkg.synthetic.clustered_cloud(n, seed)
    d_P = torch.from_numpy(P).to(dev)
    d_Q = torch.from_numpy(np.random.default_rng(seed).random((n, 3), dtype=np.float32)).to(dev)
    del P
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    d_xyz = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    d_mean = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    d_counts = torch.zeros(n, dtype=torch.int32, device=dev)
    d_rows = torch.zeros(n, dtype=torch.int32, device=dev)
    d_owner = torch.zeros(n, dtype=torch.int32, device=dev)
    d_keys = torch.zeros(n, dtype=torch.int64, device=dev)

    def count_only(leaf):
        pkg.voxel_grid_dev(d_P, n, pkg.voxel.voxel_params(leaf), 0, d_count)

    def centroids(leaf):
        pkg.voxel_grid_dev(d_P, n, pkg.voxel.voxel_params(leaf), n, d_count, d_xyz=d_xyz, d_counts=d_counts)

    def everything(leaf):
        pkg.voxel_grid_dev(d_P, n, pkg.voxel.voxel_params(leaf, attr_columns=3), n, d_count, d_attrs=d_Q, d_xyz=d_xyz, d_mean=d_mean, d_counts=d_counts,
                           d_keys=d_keys, d_rows=d_rows, d_owner=d_owner)

    for per in PER_CELL:
        lo, hi = 1e-4, 1.0  # the leaf with n / V = per, by bisection on the call's own count (V falls as the leaf grows)
        for _ in range(24):
            leaf = float(np.sqrt(lo * hi))
            count_only(leaf)
            V = int(d_count.cpu()[0])
            lo, hi = (leaf, hi) if n / max(V, 1) < per else (lo, leaf)
        leaf = float(np.float32(np.sqrt(lo * hi)))
        if a.trace_run:
            for _ in range(1 + TRACE_CALLS):
                everything(leaf)
            torch.cuda.synchronize()
            continue
        case = "%s, about %d per cell" % (cloud, per)
        out = {"leaf": leaf, "count only_ms": times(lambda: count_only(leaf), a.reps), "centroids and counts_ms": times(lambda: centroids(leaf), a.reps),
               "every output, 3 attribute columns_ms": times(lambda: everything(leaf), a.reps)}
        out["voxels"] = int(d_count.cpu()[0])
        out["points per voxel"] = round(n / max(out["voxels"], 1), 2)
        if per == PER_CELL[1] and not a.no_host:
            sec, V = host_route(d_P, d_Q, leaf)
            out["host route (download, np.unique, np.add.at, upload)_ms"] = round(sec * 1e3, 1)
            out["host route's cells"] = V
            out["host route over every output"] = round(sec * 1e3 / out["every output, 3 attribute columns_ms"]["median"], 1)
            t0 = time.perf_counter()
            ix = pkg.Index.from_device(d_P.data_ptr(), n, device=0)
            ix.synchronize()
            build_ms = (time.perf_counter() - t0) * 1e3
            d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_kept = torch.zeros(1, dtype=torch.int64, device=dev)
            t0 = time.perf_counter()
            ix.subsample_dev(leaf, d_keep.data_ptr(), d_kept_count=d_kept.data_ptr())
            ix.synchronize()
            out["Index.subsample at radius = leaf"] = {"index build_ms": round(build_ms, 3), "subsample_ms": round((time.perf_counter() - t0) * 1e3, 3),
                                                      "kept": int(d_kept.cpu()[0])}
            ix.close()
            del d_keep
        print(case, json.dumps(out), flush=True)
        res["cases"][case] = out
    del d_P, d_Q, d_xyz, d_mean, d_counts, d_rows, d_owner, d_keys
    torch.cuda.empty_cache()

if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
