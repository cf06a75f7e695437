#!/usr/bin/env python3
"""FPFH descriptors (pcpx_fpfh_self_dev) on one device, in one run on the seeded clouds of section 16 at --n
points: uniform at r = 0.01, clustered (synthetic.py) at r = 0.0023 (radii scaled by (10 M / n)^(1/3) for another n), with seeded
random unit normals.  Beside each case, from the same run and on the same box:
  - the floor: the count form on the same cloud at the same radius (pcpx_range_count_self_dev: one walk);
  - (a) fpfh_dev of the whole cloud;
  - (b) fpfh_dev of 1 % of the rows, drawn at random;
  - the composed route as the library offered it before: pcpx_range_lists_self_dev on the device, the lists' download, and a host
    loop over the lists -- the arithmetic of tests/fpfh_model.py, vectorised over all list entries at once.  The host part is timed
    on a cloud of --host-n points (<= 1 M) of the same kind with the radius scaled to the same mean count, and scaled to n by list
    entries (and said so in the output).
Call times are device-synchronised host clocks over --reps calls after warm-up.
Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fpfh_rate.py --trace-run
    python tools/fpfh_rate.py --summarise DIR --kernels-out profiles/r16_fpfh_kernels.json
python tools/fpfh_rate.py [--n N] [--host-n M] [--reps R] [--out FILE] [--no-composed]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=float, default=10e6)
ap.add_argument("--host-n", type=float, default=1e6)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_fpfh.json"))
ap.add_argument("--no-composed", action="store_true")
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--summarise", default=None)
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r16_fpfh_kernels.json"))
a = ap.parse_args()
n = int(a.n)
CASES = (("uniform", 0.01), ("clustered", 0.0023))
NORMAL_SEED, ROWS_SEED = 5, 6
TRACE_CALLS = 3
KERNELS = r"\b(k_fpfh_[a-z_]+|k_spfh|k_fpfh|k_invert_perm\w*|k_range<true, false>)"
STEPS = ("floor: count form", "(a) whole cloud", "(b) 1 % of the rows")


def summarise():
    """kernel_trace.csv of the traced run -> per case and per step (floor, a, b; the order of the traced run) the mean milliseconds of
    every kernel by name over the calls after the warm-up one.  The floor's k_range launches stand alone; a descriptor call begins
    at k_fpfh_prep."""
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
        if name == "k_range<true, false>":
            calls.append({"step": "floor", "kernels": {name: ms}})
        elif name == "k_fpfh_prep":
            calls.append({"step": "fpfh", "kernels": {name: ms}})
        elif calls:
            calls[-1]["kernels"][name] = calls[-1]["kernels"].get(name, 0.0) + ms
    per_case = len(STEPS) * (1 + TRACE_CALLS)
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own: tools/fpfh_rate.py --trace-run); milliseconds, mean over "
                   "%d calls after one warm-up call" % TRACE_CALLS, "n": n, "cases": []}
    for c, (kind, r10) in enumerate(CASES):
        mine = calls[c * per_case:(c + 1) * per_case]
        per = {"case": "%s, r = %g" % (kind, r10)}
        for s, label in enumerate(STEPS):
            group = mine[s * (1 + TRACE_CALLS) + 1:(s + 1) * (1 + TRACE_CALLS)]
            if not group:
                continue
            kernels = {k: round(float(np.mean([g["kernels"].get(k, 0.0) for g in group])), 4) for k in group[0]["kernels"]}
            per[label] = {"kernels": kernels, "all kernels of the call": round(sum(kernels.values()), 4)}
        floor = per.get(STEPS[0], {}).get("all kernels of the call")
        whole = per.get(STEPS[1], {}).get("kernels", {})
        if floor:
            per["count walks: k_spfh / floor"] = round(whole.get("k_spfh", 0.0) / floor, 2)
            per["count walks: k_fpfh / floor"] = round(whole.get("k_fpfh", 0.0) / floor, 2)
        out["cases"].append(per)
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


def make_cloud(kind, m):
    return pkg.synthetic.uniform_cloud(m, 43) if kind == "uniform" else pkg.synthetic.clustered_cloud(m)


def make_normals(m):
    v = np.random.default_rng(NORMAL_SEED).standard_normal((m, 3), dtype=np.float32)
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), np.float32)


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / reps, 3)


def host_fpfh(pts, nrm, offs, ind):
    """float32 FPFH of every point from its neighbour list (the point itself included in it), all list entries at once"""
    import fpfh_model as M
    m = len(pts)
    src = np.repeat(np.arange(m), np.diff(offs).astype(np.int64))
    dst = ind.astype(np.int64)
    other = src != dst
    src, dst = src[other], dst[other]
    kept, b1, b2, b3 = M.pair_bins(pts[src], nrm[src], pts[dst], nrm[dst])
    count = np.zeros(m * 33, np.int64)
    for base, b in ((0, b1), (11, b2), (22, b3)):
        count += np.bincount(src[kept] * 33 + base + b[kept], minlength=m * 33)
    pairs = np.bincount(src[kept], minlength=m)
    spfh = np.where(pairs[:, None] > 0, np.float32(100) * count.reshape(m, 33).astype(np.float32) / np.maximum(pairs, 1)[:, None].astype(np.float32),
                    np.float32(0)).astype(np.float32)
    d = pts[dst] - pts[src]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    far = d2 > 0
    src, dst, w = src[far], dst[far], np.float32(1) / d2[far]
    T = np.zeros((m, 33), np.float32)
    for b in range(33):
        T[:, b] = np.bincount(src, weights=spfh[dst, b] * w, minlength=m)
    T = T.reshape(m, 3, 11)
    S = T.sum(2, keepdims=True)
    return (T * np.where(S > 0, np.float32(100) / np.where(S > 0, S, 1), 0)).reshape(m, 33).astype(np.float32)


def composed(kind, r, mean_count):
    """lists on the device at n and their download; the host loop at host_n with the radius scaled to the same mean count"""
    res = {}
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    total = IX.range_lists_self_dev(r, off.data_ptr())
    res["list entries"] = total
    try:
        if total > 1_000_000_000:  # (4 GB of indices and more: neither kept on the device nor sent to the host here)
            raise RuntimeError("not run: %d list entries" % total)
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        res["lists on the device (pcpx_range_lists_self_dev)_ms"] = timed(lambda: IX.range_lists_self_dev(r, off.data_ptr(), idx.data_ptr(), total), 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_idx = idx.cpu()
        h_off = off.cpu()
        res["download of the lists (%.2f GB)_ms" % (total * 4e-9 + n * 8e-9)] = round((time.perf_counter() - t0) * 1e3, 1)
        del idx, h_idx, h_off
    except RuntimeError as e:
        res["lists at n failed"] = str(e)[:200]
    torch.cuda.empty_cache()
    m = min(int(a.host_n), 1_000_000, max(50_000, int(1e7 / max(mean_count, 1.0))))  # (at most ~10 M list entries on the host)
    pts = make_cloud(kind, m)
    nrm = make_normals(m)
    ix = pkg.LinkedOctree(pts)
    rm = float(np.float32(r * (n / m) ** (1.0 / 3.0)))
    offs, ind = ix.range_sphere(pts, rm)
    res["host part: points"] = m
    res["host part: radius (same mean count)"] = rm
    res["host part: list entries"] = int(len(ind))
    t0 = time.perf_counter()
    got = host_fpfh(pts, nrm, offs, ind)
    ms = (time.perf_counter() - t0) * 1e3
    want = ix.fpfh(nrm, rm)
    res["host part: largest |host - device| (of 100)"] = float(np.abs(got - want).max())
    res["host loop (numpy, vectorised over the list entries)_ms"] = round(ms, 1)
    res["host loop, scaled to n by list entries_ms"] = round(ms * total / max(1, len(ind)), 1)
    ix.close()
    return res


res = {"device": torch.cuda.get_device_name(0), "n": n, "reps": a.reps, "library": os.path.basename(capi.LIB_PATH), "cases": {}}
for kind, r10 in CASES:
    r = float(np.float32(r10 * (10e6 / n) ** (1.0 / 3.0)))
    pts = make_cloud(kind, n)
    d_pts = torch.from_numpy(pts).to(dev)
    IX = pkg.Index.from_device(d_pts.data_ptr(), n)
    case = "%s %d points, r = %.6g" % (kind, n, r)
    d_normals = torch.from_numpy(make_normals(n)).to(dev)
    m = max(1, n // 100)
    d_rows = torch.from_numpy(np.random.default_rng(ROWS_SEED).choice(n, m, replace=False).astype(np.int32)).to(dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    d_fpfh = torch.empty((n, 33), dtype=torch.float32, device=dev)
    floor_fn = lambda: IX.range_count_self_dev(r, cnt.data_ptr())  # noqa: E731
    whole = lambda: IX.fpfh_dev(d_normals, r, d_fpfh)  # noqa: E731
    some = lambda: IX.fpfh_dev(d_normals, r, d_fpfh, d_rows=d_rows, m=m)  # noqa: E731
    if a.trace_run:
        for fn in (floor_fn, whole, some):
            for _ in range(1 + TRACE_CALLS):
                fn()
        torch.cuda.synchronize()
    else:
        out = {"radius": r}
        floor_fn()
        torch.cuda.synchronize()
        out["mean count"] = round(float(cnt.double().mean().item()), 2)
        floor = out["floor: count form (pcpx_range_count_self_dev)_ms"] = timed(floor_fn, a.reps)
        for label, fn in (("(a) whole cloud", whole), ("(b) 1 %% of the rows (%d)" % m, some)):
            ms = timed(fn, a.reps)
            out[label] = {"call_ms": ms, "ratio to the floor": round(ms / floor, 2)}
        if not a.no_composed:
            out["composed route"] = composed(kind, r, out["mean count"])
            lists = out["composed route"].get("lists on the device (pcpx_range_lists_self_dev)_ms")
            down = [v for k, v in out["composed route"].items() if k.startswith("download")]
            if lists is not None and down:
                tot = lists + down[0] + out["composed route"]["host loop, scaled to n by list entries_ms"]
                out["composed route end to end_ms (lists + download at n, host part scaled)"] = round(tot, 1)
                out["composed / fused (a)"] = round(tot / out["(a) whole cloud"]["call_ms"], 1)
        print(case, json.dumps(out), flush=True)
        res["cases"][case] = out
    IX.close()
    del d_pts, IX, d_normals, d_fpfh
    torch.cuda.empty_cache()
if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
