#!/usr/bin/env python3
"""Keypoints (pcpx_local_maxima_self_dev, pcpx_iss_keypoints_self_dev) on one device, in one run on the seeded
clouds of section 16 at --n points: uniform at r = 0.01, clustered (synthetic.py) at r = 0.0023 (radii scaled by (10 M / n)^(1/3)
for another n).  Beside each case, from the same run and on the same box:
  - the floor: the count form on the same cloud at the same radius (pcpx_range_count_self_dev: one walk);
  - (a) local_maxima_dev (keep + kept rows + count) on a seeded random score with every point a candidate;
  - (b) the same with 10 % candidates (min_score at the score's 90th percentile);
  - (c) iss_keypoints_dev with both radii = r, and what it is made of: shape_features_self_dev (evals + counts) at r plus the floor;
  - the composed route as the library offered it before: pcpx_range_lists_self_dev on the device, the lists' download, and the host
    loop of tests/keypoints_model.py.  The host part is timed on a cloud of --host-n points (<= 1 M) of the same kind with the
    radius scaled to the same mean count, and scaled to n by list entries (and said so in the output).
Call times are device-synchronised host clocks over --reps calls after warm-up.
Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/keypoints_rate.py --trace-run
    python tools/keypoints_rate.py --summarise DIR --kernels-out profiles/r15_keypoints_kernels.json
python tools/keypoints_rate.py [--n N] [--host-n M] [--reps R] [--out FILE] [--no-composed]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_keypoints.json"))
ap.add_argument("--no-composed", action="store_true")
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--summarise", default=None)
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r15_keypoints_kernels.json"))
a = ap.parse_args()
n = int(a.n)
CASES = (("uniform", 0.01), ("clustered", 0.0023))
SCORE_SEED = 5
TRACE_CALLS = 3
KERNELS = r"\b(k_maxima_[a-z_]+|k_local_maxima|k_iss_score|k_scan_[a-z_]+|k_range_features<true>|k_range<true, false>)"


def summarise():
    """kernel_trace.csv of the traced run -> per case and per step (floor, a, b, c; the order of the traced run) the mean milliseconds
    of every kernel by name over the calls after the warm-up one.  A case begins at the k_range launches of the floor."""
    rows = []
    for f in glob.glob(os.path.join(a.summarise, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = []
    for r in rows:
        m = re.search(KERNELS, r["Kernel_Name"].replace("pcpx::(anonymous namespace)::", ""))
        if m:
            seq.append((m.group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    # split into calls: the floor's k_range launches stand alone; a local-maxima call begins at k_maxima_prep, an ISS call at
    # k_range_features and takes the k_maxima_prep that follows it
    calls = []
    for name, ms in seq:
        if name == "k_range<true, false>":
            calls.append({"step": "floor", "kernels": {name: ms}})
        elif name == "k_range_features<true>":
            calls.append({"step": "iss", "kernels": {name: ms}})
        elif name == "k_maxima_prep" and not (calls and calls[-1]["step"] == "iss" and "k_maxima_prep" not in calls[-1]["kernels"]):
            calls.append({"step": "maxima", "kernels": {name: ms}})
        elif calls:
            calls[-1]["kernels"][name] = calls[-1]["kernels"].get(name, 0.0) + ms
    per_case = 4 * (1 + TRACE_CALLS)
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own: tools/keypoints_rate.py --trace-run); milliseconds, mean "
                   "over %d calls after one warm-up call" % TRACE_CALLS, "n": n, "cases": []}
    for c, (kind, r10) in enumerate(CASES):
        mine = calls[c * per_case:(c + 1) * per_case]
        per = {"case": "%s, r = %g" % (kind, r10)}
        for s, label in enumerate(("floor: count form", "(a) every point a candidate", "(b) 10 % candidates", "(c) ISS")):
            group = mine[s * (1 + TRACE_CALLS) + 1:(s + 1) * (1 + TRACE_CALLS)]
            if not group:
                continue
            kernels = {k: round(float(np.mean([g["kernels"].get(k, 0.0) for g in group])), 4) for k in group[0]["kernels"]}
            per[label] = {"kernels": kernels, "all kernels of the call": round(sum(kernels.values()), 4)}
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


def make_score(m):
    return np.random.default_rng(SCORE_SEED).random(m, dtype=np.float32)


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / reps, 3)


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
    m = min(int(a.host_n), 1_000_000, max(50_000, int(4e7 / max(mean_count, 1.0))))  # (at most ~40 M list entries on the host)
    import cluster_model as CM
    import keypoints_model as M
    pts = make_cloud(kind, m)
    score = make_score(m)
    ix = pkg.LinkedOctree(pts)
    rm = float(np.float32(r * (n / m) ** (1.0 / 3.0)))
    offs, ind = ix.range_sphere(pts, rm)
    res["host part: points"] = m
    res["host part: radius (same mean count)"] = rm
    res["host part: list entries"] = int(len(ind))
    t0 = time.perf_counter()
    src, dst, _ = CM.edges_from_lists(offs, ind)
    keep = M.local_maxima(m, src, dst, score)
    ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(np.nonzero(keep)[0], ix.local_maxima(score, rm))
    res["host loop (numpy model)_ms"] = round(ms, 1)
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
    score = make_score(n)
    p90 = float(np.quantile(score, 0.9))
    d_score = torch.from_numpy(score).to(dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    evals = torch.empty(3 * n, dtype=torch.float32, device=dev)
    floor_fn = lambda: IX.range_count_self_dev(r, cnt.data_ptr())  # noqa: E731
    every = lambda: IX.local_maxima_dev(d_score, r, keep, d_kept_rows=kept, d_kept_count=total)  # noqa: E731
    tenth = lambda: IX.local_maxima_dev(d_score, r, keep, min_score=p90, d_kept_rows=kept, d_kept_count=total)  # noqa: E731
    iss = lambda: IX.iss_keypoints_dev(r, r, keep, d_kept_rows=kept, d_kept_count=total)  # noqa: E731
    features = lambda: IX.shape_features_self_dev(r, d_evals=evals.data_ptr(), d_counts=cnt.data_ptr())  # noqa: E731
    if a.trace_run:
        for fn in (floor_fn, every, tenth, iss):
            for _ in range(1 + TRACE_CALLS):
                fn()
        torch.cuda.synchronize()
    else:
        out = {"radius": r}
        floor_fn()
        torch.cuda.synchronize()
        out["mean count"] = round(float(cnt.double().mean().item()), 2)
        floor = out["floor: count form (pcpx_range_count_self_dev)_ms"] = timed(floor_fn, a.reps)
        for label, fn in (("(a) every point a candidate", every), ("(b) 10 % candidates", tenth), ("(c) ISS, both radii = r", iss)):
            ms = timed(fn, a.reps)
            torch.cuda.synchronize()
            out[label] = {"call (keep + kept rows + count)_ms": ms, "kept": int(total.item()), "ratio to the floor": round(ms / floor, 2)}
        fms = out["shape_features_self_dev (evals + counts) at r_ms"] = timed(features, a.reps)
        out["(c) ISS, both radii = r"]["features + floor_ms"] = round(fms + floor, 3)
        out["(c) ISS, both radii = r"]["ratio to features + floor"] = round(out["(c) ISS, both radii = r"]["call (keep + kept rows + count)_ms"] / (fms + floor), 2)
        if not a.no_composed:
            out["composed route"] = composed(kind, r, out["mean count"])
            lists = out["composed route"].get("lists on the device (pcpx_range_lists_self_dev)_ms")
            down = [v for k, v in out["composed route"].items() if k.startswith("download")]
            if lists is not None and down:
                tot = lists + down[0] + out["composed route"]["host loop, scaled to n by list entries_ms"]
                out["composed route end to end_ms (lists + download at n, host part scaled)"] = round(tot, 1)
                out["composed / fused (a)"] = round(tot / out["(a) every point a candidate"]["call (keep + kept rows + count)_ms"], 1)
        print(case, json.dumps(out), flush=True)
        res["cases"][case] = out
    IX.close()
    del d_pts, IX
    torch.cuda.empty_cache()
if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
