#!/usr/bin/env python3
"""Iterative closest point (include/pcpx_icp.h) on one device, in one run: a source of 10^6 points of a curved
surface, turned by 5 degrees and shifted by 0.05 of the extent, against targets of 10^6 and 10^7 points of that surface, from a first
pose that is off by half a mean spacing in angle (radians) and in place -- what a RANSAC refit leaves --, the source with Gaussian
noise of half a mean spacing (without it the partner lists repeat after four rounds and the loop stops), the radius three mean
spacings, a fixed number of rounds (the output says whether the loop was still running at the last of them).  Per target, device-synchronised host clocks:
  * the whole call (Index.icp_dev, point to point) at two round counts, and the cost of a round from their difference;
  * beside it what a caller had to compose before this call existed, per round: the moved source (torch), pcpx_knn_batch_dev with
    k = 1 -- which sorts the queries again on every call --, the pair list (torch) and pcpx_rigid_fit_dev;
  * the two A/Bs of the call, their variants alternating in one job: the source sorted once against sorted again in every round
    ("icp_resort"), and a lane starting from its previous partner against from nothing ("icp_previous_start");
  * the nearest partners alone (Index.nearest_posed_dev: the sort and one launch of k_nearest_posed).
Medians and ranges over --reps calls after a warm-up.  Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/icp_rate.py --trace-run
python tools/icp_rate.py [--reps R] [--targets N,N] [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_icp.json"))
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


def spread(fn, reps):
    """milliseconds of fn() per call: median, minimum, maximum over reps calls, each device-synchronised"""
    ms = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:  # (the first call warms up)
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def alternating(variants, reps):
    """{name: spread} of several variants of a call, one call of each in turn"""
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


res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "library": os.path.basename(capi.LIB_PATH), "source points": a.source,
       "rounds": list(ROUNDS), "what": "milliseconds per call, device-synchronised host clocks, median and range", "targets": {}}
truth = rigid([0.3, -1.0, 0.5], np.deg2rad(5.0), 0.05 * 2.9 * np.array([0.6, -0.64, 0.48]))
inv = np.linalg.inv(truth)
for n in (int(v) for v in a.targets.split(",")):
    target = surface(n, 31)
    rows = np.random.default_rng(32).choice(n, a.source, replace=n < a.source)
    spacing = float(np.sqrt(4.0 / n))  # (the surface covers about four square units)
    noise = np.random.default_rng(33).normal(0.0, 0.5 * spacing, (a.source, 3))
    source = ((target[rows].astype(np.float64) + noise) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    ix = pkg.Index(target)
    radius = 3.0 * spacing
    m = len(source)
    start = rigid([1.0, 2.0, -1.0], 0.5 * spacing, 0.5 * spacing * np.array([0.48, 0.6, -0.64])) @ truth
    d_start = torch.from_numpy(start.reshape(16).copy()).to(dev)
    d_S = torch.from_numpy(source).to(dev)
    d_T = torch.from_numpy(target).to(dev)
    d_xf = torch.zeros(16, dtype=torch.float64, device=dev)
    d_words = torch.zeros(3, dtype=torch.int32, device=dev)
    d_partner = torch.zeros(m, dtype=torch.int32, device=dev)
    d_d2 = torch.zeros(m, dtype=torch.float32, device=dev)
    d_idx = torch.zeros(m, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(m, dtype=torch.int32, device=dev)
    d_rms = torch.zeros(1, dtype=torch.float64, device=dev)
    rows_m = torch.arange(m, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream()

    def call(rounds):
        ix.icp_dev(d_S, m, radius, d_xf, d_pose=d_start, max_iterations=rounds, d_status=d_words[0:1], d_iterations=d_words[1:2], d_last_count=d_words[2:3],
                   d_partner=d_partner)
        ix.synchronize()

    def composed(rounds):
        """the parent commit's way, with no stopping rule (reading one back would cost a round trip per round)"""
        pose = d_start.reshape(4, 4)
        for _ in range(rounds):
            y = (d_S.double() @ pose[:3, :3].T + pose[:3, 3]).float().contiguous()
            stream.synchronize()  # (the index has a stream of its own)
            ix.knn_batch_dev(y.data_ptr(), m, 1, 0.0, d_idx.data_ptr(), d_cnt.data_ptr(), d_d2.data_ptr())
            ix.synchronize()
            pairs = torch.stack([rows_m, d_idx], 1).contiguous()
            pkg.rigid_fit_dev(d_S, m, d_T, n, pairs, m, d_xf, d_rms=d_rms)
            pose = d_xf.reshape(4, 4)
        stream.synchronize()

    def nearest():
        ix.nearest_posed_dev(d_S, m, radius, d_partner, d_pose=d_start, d_d2=d_d2)
        ix.synchronize()

    if a.trace_run:
        for fn in (lambda: call(ROUNDS[0]), nearest, lambda: composed(2)):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ix.close()
        continue
    out = {"radius": radius, "mean spacing": spacing}
    for rounds in ROUNDS:
        out["call, %d rounds" % rounds] = spread(lambda: call(rounds), a.reps)
        words = d_words.cpu().numpy()
        out["call, %d rounds" % rounds].update({"status": int(words[0]), "updates": int(words[1]), "partners": int(words[2])})
    lo, hi = ROUNDS[0], ROUNDS[-1]
    # (meaningful only where "updates" equals the rounds in both: a stopped round costs next to nothing)
    out["one round of the call_ms"] = round((out["call, %d rounds" % hi]["median_ms"] - out["call, %d rounds" % lo]["median_ms"]) / (hi - lo), 3)
    out["nearest partners alone (sort + k_nearest_posed)"] = spread(nearest, a.reps)
    out["composed from public parts, %d rounds" % lo] = spread(lambda: composed(lo), a.reps)
    out["composed from public parts, %d rounds" % hi] = spread(lambda: composed(hi), a.reps)
    out["one round of the composition_ms"] = round((out["composed from public parts, %d rounds" % hi]["median_ms"] -
                                                    out["composed from public parts, %d rounds" % lo]["median_ms"]) / (hi - lo), 3)

    def with_knob(name, value, rounds):
        def fn():
            ix.debug_set(name, value)
            call(rounds)
        return fn
    out["A/B sort once | sort every round, %d rounds" % hi] = alternating([("once", with_knob("icp_resort", 0, hi)), ("every round", with_knob("icp_resort", 1, hi))],
                                                                          a.reps)
    ix.debug_set("icp_resort", 0)
    out["A/B start from nothing | from the previous partner, %d rounds" % hi] = alternating(
        [("nothing", with_knob("icp_previous_start", 0, hi)), ("previous partner", with_knob("icp_previous_start", 1, hi))], a.reps)
    ix.debug_set("icp_previous_start", -1)
    print(n, json.dumps(out), flush=True)
    res["targets"][str(n)] = out
    ix.close()
    del d_S, d_T
    torch.cuda.empty_cache()
if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
