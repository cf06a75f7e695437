#!/usr/bin/env python3
"""RANSAC rigid registration from correspondences (include/pcpx_register.h) on one device, in one run, on seeded
noisy sets (a cloud in [-1, 1]^3, 30 % inliers with noise sigma = 0.002, tau = 0.01, edge similarity 0.9): hypotheses x
correspondences = 100 000 x 1 000, 1 000 000 x 10 000 and 4 000 000 x 1 000.  Per case the device form with every output and the
refit (device-synchronised host clocks over --reps calls after a warm-up), the pair tests per second of the call, and what it found.
Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/register_rate.py --trace-run
    python tools/register_rate.py --summarise DIR --kernels-out profiles/r18_register_kernels.json
python tools/register_rate.py [--reps R] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_register.json"))
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--summarise", default=None)
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r18_register_kernels.json"))
a = ap.parse_args()
CASES = ((100_000, 1_000), (1_000_000, 10_000), (4_000_000, 1_000))  # (hypotheses, correspondences)
TRACE_CALLS = 3
TAU, SIMILARITY, SEED = 0.01, 0.9, 0x1234
KERNELS = r"\b(k_reg_[a-z_]+|k_ransac_[a-z_]+|k_fit_[a-z_]+|k_fixed_[a-z_]+(?:<\w+>)?|k_scan_[a-z_]+)"


def summarise():
    """kernel_trace.csv of the traced run -> per case (the order of the traced run) the mean milliseconds of every kernel by name over
    the calls after the warm-up one.  A call begins at its k_reg_pack."""
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
        if name == "k_reg_pack":
            calls.append({})
        if calls:
            k = calls[-1].setdefault(name, [0.0, 0])
            k[0] += ms
            k[1] += 1
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own: tools/register_rate.py --trace-run); milliseconds per call "
                   "(and launches per call), mean over %d calls after one warm-up call" % TRACE_CALLS, "cases": []}
    for c, (T, C) in enumerate(CASES):
        group = calls[c * (1 + TRACE_CALLS) + 1:(c + 1) * (1 + TRACE_CALLS)]
        if not group:
            continue
        kernels = {k: [round(float(np.mean([g.get(k, [0.0, 0])[0] for g in group])), 4), group[0][k][1]] for k in group[0]}
        count_ms = kernels.get("k_ransac_count", [0.0])[0]
        out["cases"].append({"case": "%d x %d" % (T, C), "kernels": kernels, "all kernels of the call": round(sum(v[0] for v in kernels.values()), 4),
                             "pair tests per second of k_ransac_count": round(T * C / (count_ms * 1e-3), 0) if count_ms else None})
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


def noisy_set(C, seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1, 1, (C, 3)).astype(np.float32)
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    A *= np.sign(np.linalg.det(A))
    Q = (P.astype(np.float64) @ A.T + rng.uniform(-1, 1, 3) + rng.normal(0, 0.002, (C, 3))).astype(np.float32)
    true = rng.random(C) < 0.3
    Q[~true] = rng.uniform(-2, 2, (int((~true).sum()), 3)).astype(np.float32)
    pairs = np.stack([np.arange(C), np.arange(C)], 1).astype(np.int32)
    return P, Q, pairs, int(true.sum())


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / reps, 3)


res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "library": os.path.basename(capi.LIB_PATH), "max_distance": TAU,
       "edge_similarity": SIMILARITY, "cases": {}}
for T, C in CASES:
    P, Q, pairs, true = noisy_set(C, 19)
    d_P, d_Q, d_pairs = (torch.from_numpy(x).to(dev) for x in (P, Q, pairs))
    d_count = torch.tensor([C], dtype=torch.int64).to(dev)
    d_small = torch.zeros(3, dtype=torch.int32, device=dev)
    d_inl = torch.zeros(C, dtype=torch.int32, device=dev)
    d_ninl = torch.zeros(1, dtype=torch.int64, device=dev)
    d_xf = torch.zeros((2, 16), dtype=torch.float64, device=dev)

    def call(refit=True):
        pkg.ransac_rigid_dev(d_P, C, d_Q, C, d_pairs, C, T, TAU, d_small[0:1], d_count=d_count, d_hypothesis=d_small[1:2], d_score=d_small[2:3],
                             d_inliers=d_inl, d_inlier_count=d_ninl, d_transform=d_xf[0], d_refit=d_xf[1] if refit else None, seed=SEED,
                             edge_similarity=SIMILARITY)
    if a.trace_run:
        for _ in range(1 + TRACE_CALLS):
            call()
        torch.cuda.synchronize()
        continue
    case = "%d x %d" % (T, C)
    ms = timed(call, a.reps)
    small = d_small.cpu().numpy()
    out = {"plan": pkg.ransac_plan(T, C), "call_ms": ms, "pair tests per second": round(T * C / (ms * 1e-3), 0),
           "call without the refit_ms": timed(lambda: call(False), a.reps), "true inliers": true, "found": int(small[0]), "hypothesis": int(small[1]),
           "inliers": int(small[2])}
    print(case, json.dumps(out), flush=True)
    res["cases"][case] = out
    del d_P, d_Q, d_pairs
    torch.cuda.empty_cache()
if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
