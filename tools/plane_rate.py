#!/usr/bin/env python3
"""Plane detection (include/pcpx_planes.h) on one device, in one run, on seeded scenes (a cloud in [-1, 1]^3,
30 % of it on a plane with noise sigma = 0.002, tau = 0.01): hypotheses x points = 10 000 x 1 000 000, 100 000 x 1 000 000 and
1 000 000 x 100 000, and extract_planes of six planes on 1 000 000 points.  Per case the device form with every output and the refit:
device-synchronised times of single calls after a warm-up (median, min, max), the point tests per second, what it found -- and the
same scoring as torch's dense form on the same box (hypotheses x points product, abs() <= tau, row sums, chunked to fit), which is
what a user had before this call existed.
Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/plane_rate.py --trace-run
    python tools/plane_rate.py --summarise DIR --kernels-out profiles/r20_plane_kernels.json
python tools/plane_rate.py [--reps R] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_plane.json"))
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--summarise", default=None)
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r20_plane_kernels.json"))
ap.add_argument("--no-torch", action="store_true", help="skip the dense torch form")
a = ap.parse_args()
CASES = ((10_000, 1_000_000), (100_000, 1_000_000), (1_000_000, 100_000))  # (hypotheses, points)
PEEL = dict(points=1_000_000, hypotheses=1024, planes=6, min_inliers=50_000)
TRACE_CALLS = 3
TAU, SEED = 0.01, 0x1234
# vector instructions of one record in k_plane_count's loop, counted in the disassembly, and the estimate from them
VALU_PER_RECORD, CLOCK_GHZ, SIMDS = 8, 2.4, 1024
ESTIMATE = SIMDS * CLOCK_GHZ * 1e9 / (VALU_PER_RECORD * 2) * 64
KERNELS = r"\b(k_plane_[a-z_]+|k_ransac_[a-z_]+|k_reg_[a-z_]+|k_pfit_[a-z_]+|k_fixed_[a-z_]+|k_scan_[a-z_]+)"


def summarise():
    """kernel_trace.csv of the traced run -> per case (the order of the traced run) the mean milliseconds of every kernel by name over
    the calls after the warm-up one.  A call begins at its k_plane_begin."""
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
        if name == "k_plane_begin":
            calls.append({})
        if calls:
            k = calls[-1].setdefault(name, [0.0, 0])
            k[0] += ms
            k[1] += 1
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own: tools/plane_rate.py --trace-run); milliseconds per call "
                   "(and launches per call), mean over %d calls after one warm-up call" % TRACE_CALLS, "cases": []}
    names = ["%d x %d" % c for c in CASES] + ["extract %d planes of %d points, %d hypotheses a round" % (PEEL["planes"], PEEL["points"], PEEL["hypotheses"])]
    for c, name in enumerate(names):
        group = calls[c * (1 + TRACE_CALLS) + 1:(c + 1) * (1 + TRACE_CALLS)]
        if not group:
            continue
        kernels = {k: [round(float(np.mean([g.get(k, [0.0, 0])[0] for g in group])), 4), group[0][k][1]] for k in group[0]}
        case = {"case": name, "kernels": kernels, "all kernels of the call": round(sum(v[0] for v in kernels.values()), 4)}
        count_ms = kernels.get("k_plane_count", [0.0])[0]
        if c < len(CASES) and count_ms:
            rate = CASES[c][0] * CASES[c][1] / (count_ms * 1e-3)
            case["point tests per second of k_plane_count"] = round(rate, 0)
            case["of the issue-rate estimate"] = round(rate / ESTIMATE, 3)
        out["cases"].append(case)
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


def noisy_scene(n, seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1, 1, (n, 3))
    on = rng.random(n) < 0.3
    nrm = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    P[on] -= ((P[on] @ nrm) + 0.1)[:, None] * nrm
    P[on] += rng.normal(0, 0.002, (int(on.sum()), 1)) * nrm
    return P.astype(np.float32), int((np.abs(P @ nrm + 0.1) <= TAU).sum())


def box_scene(n, seed):
    """the six faces of the cube [-1, 1]^3, a seventh of the points each, and a seventh inside it"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1, 1, (n, 3))
    face = rng.integers(0, 7, n)
    for f in range(6):
        P[face == f, f // 2] = (1.0 if f % 2 else -1.0) + rng.normal(0, 0.002, int((face == f).sum()))
    return P.astype(np.float32)


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
    return round(float(np.median(out)), 3), round(min(out), 3), round(max(out), 3)


def dense_scores(d_P, d_n, d_m, tau, chunk_bytes=1 << 30):
    """the parent's route: inliers of every hypothesis (n (T, 3), m (T,)) by a dense product, chunked to about chunk_bytes of floats"""
    T, n = len(d_n), len(d_P)
    chunk = max(1, chunk_bytes // (4 * n))
    out = torch.empty(T, dtype=torch.int64, device=d_P.device)
    Pt = d_P.t().contiguous()
    for t0 in range(0, T, chunk):
        e = d_n[t0:t0 + chunk] @ Pt - d_m[t0:t0 + chunk, None]
        out[t0:t0 + chunk] = (e.abs() <= tau).sum(1)
    return out


res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "library": os.path.basename(capi.LIB_PATH), "max_distance": TAU,
       "issue-rate estimate": {"vector instructions per record": VALU_PER_RECORD, "point tests per second": ESTIMATE,
                               "formula": "1 024 SIMDs x 2.4 GHz / (instructions x 2 cycles) x 64"}, "cases": {}}
for T, n in CASES:
    P, true = noisy_scene(n, 26)
    d_P = torch.from_numpy(P).to(dev)
    d_small = torch.zeros(3, dtype=torch.int32, device=dev)
    d_inl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ninl = torch.zeros(1, dtype=torch.int64, device=dev)
    d_planes = torch.zeros((2, 4), dtype=torch.float64, device=dev)

    def call(refit=True):
        prm = pkg.planes.plane_params(T, TAU, SEED, refit)
        pkg.ransac_plane_dev(d_P, n, prm, d_small[0:1], d_hypothesis=d_small[1:2], d_score=d_small[2:3], d_inliers=d_inl, d_inlier_count=d_ninl,
                             d_plane=d_planes[0], d_refit=d_planes[1] if refit else None)
    if a.trace_run:
        for _ in range(1 + TRACE_CALLS):
            call()
        torch.cuda.synchronize()
        continue
    case = "%d x %d" % (T, n)
    med, lo, hi = times(call, a.reps)
    small = d_small.cpu().numpy()
    out = {"plan": pkg.plane_plan(T, n), "call_ms": {"median": med, "min": lo, "max": hi}, "point tests per second": round(T * n / (med * 1e-3), 0),
           "of the issue-rate estimate": round(T * n / (med * 1e-3) / ESTIMATE, 3), "call without the refit_ms": times(lambda: call(False), a.reps)[0],
           "points truly within max_distance": true, "found": int(small[0]), "hypothesis": int(small[1]), "inliers": int(small[2])}
    if not a.no_torch:
        rng = np.random.default_rng(1)
        nn = rng.normal(size=(T, 3))
        d_n = torch.from_numpy((nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(np.float32)).to(dev)
        d_m = torch.from_numpy(rng.uniform(-1, 1, T).astype(np.float32)).to(dev)
        tmed, tlo, thi = times(lambda: dense_scores(d_P, d_n, d_m, TAU), 3)
        out["torch dense scoring_ms"] = {"median": tmed, "min": tlo, "max": thi}
        out["torch over this call"] = {"median": round(tmed / med, 2), "min": round(tlo / hi, 2), "max": round(thi / lo, 2)}
        del d_n, d_m
    print(case, json.dumps(out), flush=True)
    res["cases"][case] = out
    del d_P, d_inl
    torch.cuda.empty_cache()

# plane after plane
n, T = PEEL["points"], PEEL["hypotheses"]
d_P = torch.from_numpy(box_scene(n, 27)).to(dev)
d_labels = torch.zeros(n, dtype=torch.int32, device=dev)
d_count = torch.zeros(1, dtype=torch.int32, device=dev)
d_planes = torch.zeros((2, PEEL["planes"], 4), dtype=torch.float64, device=dev)
d_scores = torch.zeros(PEEL["planes"], dtype=torch.int32, device=dev)


def peel():
    prm = pkg.planes.plane_params(T, TAU, SEED, True, min_inliers=PEEL["min_inliers"], max_planes=PEEL["planes"])
    pkg.extract_planes_dev(d_P, n, prm, d_labels, d_count, d_planes=d_planes[0], d_refits=d_planes[1], d_scores=d_scores)


if a.trace_run:
    for _ in range(1 + TRACE_CALLS):
        peel()
    torch.cuda.synchronize()
else:
    med, lo, hi = times(peel, a.reps)
    out = {"points": n, "hypotheses a round": T, "plan": pkg.plane_plan(T, n, max_planes=PEEL["planes"]), "call_ms": {"median": med, "min": lo, "max": hi},
           "planes": int(d_count.cpu()[0]), "scores": d_scores.cpu().numpy().tolist(),
           "largest |component| of each refit normal": np.abs(d_planes[1].cpu().numpy()[:, :3]).max(1).round(6).tolist()}
    print("extract", json.dumps(out), flush=True)
    res["extract_planes"] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
