#!/usr/bin/env python3
"""Generalized ICP (include/pcpx_gicp.h) beside point to plane on one device, in one run, on the scene of
tools/icp_rate.py: a source of 10^6 points of a curved surface with Gaussian noise of half a mean spacing, turned by 5 degrees and
shifted by 0.05 of the extent, against targets of 10^6 and 10^7 points of that surface, from a first pose that is off by half a mean
spacing in angle (radians) and in place, the radius three mean spacings, a fixed number of rounds (the output says whether the loop
was still running at the last of them).  The normals of both clouds are the unoriented PCA normals of range_neighbourhoods_self_dev
over that radius, one walk each (timed once per cloud, not part of the calls).  Per target, device-synchronised host clocks:
  * Index.gicp_dev (from normals, epsilon 1e-3) and Index.icp_dev with the target's normals (point to plane), one call of each in
    turn, at two round counts; the cost of a round from their difference; the ratio of the two calls.
Medians and ranges over --reps calls after a warm-up.  Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gicp_rate.py --trace-run
python tools/gicp_rate.py [--reps R] [--targets N,N] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--source", type=int, default=1_000_000)
ap.add_argument("--targets", default="1000000,10000000")
ap.add_argument("--rounds", default="4,10")
ap.add_argument("--epsilon", type=float, default=1e-3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_gicp.json"))
ap.add_argument("--trace-run", action="store_true")
a = ap.parse_args()
ROUNDS = tuple(int(v) for v in a.rounds.split(","))

import torch  # noqa: E402

pkg = importlib.import_module("point-cloud-processing_amd")
capi = importlib.import_module("point-cloud-processing_amd._capi")
dev = torch.device("cuda", 0)


def surface(n, seed):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    z = 0.3 * np.sin(2.0 * x) * np.cos(1.5 * y) + 0.15 * x * x - 0.1 * y
    return np.stack([x, y, z], 1).astype(np.float32)


def rigid(axis, radians, shift):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(radians) * K + (1 - np.cos(radians)) * (K @ K)
    T[:3, 3] = shift
    return T


def alternating(variants, reps):
    """{name: spread} of several calls, one call of each in turn, each device-synchronised; the first round warms up"""
    ms = {name: [] for name, _ in variants}
    for r in range(reps + 1):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for name, v in ms.items()}


def normals_of(ix, n, radius):
    """(device normals (n, 3), milliseconds of the walk)"""
    d = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ix.range_neighbourhoods_self_dev(radius, d_normals=d.data_ptr())
    ix.synchronize()
    return d, round((time.perf_counter() - t0) * 1e3, 3)


res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "library": os.path.basename(capi.LIB_PATH), "source points": a.source,
       "rounds": list(ROUNDS), "epsilon": a.epsilon, "what": "milliseconds per call, device-synchronised host clocks, median and range", "targets": {}}
truth = rigid([0.3, -1.0, 0.5], np.deg2rad(5.0), 0.05 * 2.9 * np.array([0.6, -0.64, 0.48]))
inv = np.linalg.inv(truth)
for n in (int(v) for v in a.targets.split(",")):
    target = surface(n, 31)
    rows = np.random.default_rng(32).choice(n, a.source, replace=n < a.source)
    spacing = float(np.sqrt(4.0 / n))  # (the surface covers about four square units)
    noise = np.random.default_rng(33).normal(0.0, 0.5 * spacing, (a.source, 3))
    source = ((target[rows].astype(np.float64) + noise) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    ix, sx = pkg.Index(target), pkg.Index(source)
    radius = 3.0 * spacing
    m = len(source)
    start = rigid([1.0, 2.0, -1.0], 0.5 * spacing, 0.5 * spacing * np.array([0.48, 0.6, -0.64])) @ truth
    d_start = torch.from_numpy(start.reshape(16).copy()).to(dev)
    d_S = torch.from_numpy(source).to(dev)
    d_nt, target_ms = normals_of(ix, n, radius)
    d_ns, source_ms = normals_of(sx, m, radius)
    sx.close()
    d_xf = torch.zeros(16, dtype=torch.float64, device=dev)
    d_words = torch.zeros(3, dtype=torch.int32, device=dev)
    d_partner = torch.zeros(m, dtype=torch.int32, device=dev)
    d_rms = torch.zeros(max(ROUNDS), dtype=torch.float64, device=dev)

    def gicp(rounds):
        ix.gicp_dev(d_S, m, radius, d_xf, d_source_normals=d_ns, d_normals=d_nt, epsilon=a.epsilon, d_pose=d_start, max_iterations=rounds,
                    d_status=d_words[0:1], d_iterations=d_words[1:2], d_last_count=d_words[2:3], d_rms=d_rms, d_partner=d_partner)
        ix.synchronize()

    def plane(rounds):
        ix.icp_dev(d_S, m, radius, d_xf, d_pose=d_start, max_iterations=rounds, d_normals=d_nt, d_status=d_words[0:1], d_iterations=d_words[1:2],
                   d_last_count=d_words[2:3], d_rms=d_rms, d_partner=d_partner)
        ix.synchronize()

    if a.trace_run:
        for fn in (gicp, plane):
            for _ in range(3):
                fn(ROUNDS[0])
        torch.cuda.synchronize()
        ix.close()
        continue
    out = {"radius": radius, "mean spacing": spacing, "normals of the target_ms": target_ms, "normals of the source_ms": source_ms}
    for rounds in ROUNDS:
        both = alternating([("gicp", lambda: gicp(rounds)), ("point to plane", lambda: plane(rounds))], a.reps)
        for name, fn in (("gicp", gicp), ("point to plane", plane)):  # the words and the residual of one more call of each
            fn(rounds)
            words = d_words.cpu().numpy()
            both[name].update({"status": int(words[0]), "updates": int(words[1]), "partners": int(words[2]),
                               "last rms": float(d_rms.cpu().numpy()[max(int(words[1]), 1) - 1])})
        both["gicp / point to plane"] = round(both["gicp"]["median_ms"] / both["point to plane"]["median_ms"], 3)
        out["%d rounds" % rounds] = both
    lo, hi = ROUNDS[0], ROUNDS[-1]
    # (meaningful only where "updates" equals the rounds in both: a stopped round costs next to nothing)
    for name in ("gicp", "point to plane"):
        out["one round of %s_ms" % name] = round((out["%d rounds" % hi][name]["median_ms"] - out["%d rounds" % lo][name]["median_ms"]) / (hi - lo), 3)
    print(n, json.dumps(out), flush=True)
    res["targets"][str(n)] = out
    ix.close()
    del d_S, d_nt, d_ns
    torch.cuda.empty_cache()
if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
