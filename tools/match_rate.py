#!/usr/bin/env python3
"""Descriptor matching (include/pcpx_match.h) on one device, in one run, on seeded FPFH-like sets (three blocks
of 11 bins that each sum to 100) at dims = 33: 100 000 x 100 000, 1 000 x 1 000 000 and 10 000 x 10 000 rows.  Per case the device
forms of nearest, of correspondences without and with the mutual test (device-synchronised host clocks over --reps calls after a
warm-up), pairs per second of the nearest call, and from the same run on the same box:
  - at dims = 16 (the first 16 columns) and the same counts, with m capped at --kd-m so that it finishes in seconds:
    pcpx_kd_knn_batch(k = 2, eps = 0), a host-form call, beside the host form of match_nearest on the same rows (both upload their
    queries and download their rows; the kd index is built before the clock starts) -- and whether the two agree bit for bit;
  - the chunked torch.cdist + topk(2) route on the same device tensors at dims = 33 (a different arithmetic: how many best indices
    differ is reported).
Kernel times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/match_rate.py --trace-run
    python tools/match_rate.py --summarise DIR --kernels-out profiles/r17_match_kernels.json
python tools/match_rate.py [--reps R] [--kd-m M] [--out FILE]"""
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
ap.add_argument("--kd-m", type=int, default=10000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_match.json"))
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--summarise", default=None)
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r17_match_kernels.json"))
a = ap.parse_args()
CASES = ((100_000, 100_000), (1_000, 1_000_000), (10_000, 10_000))
DIMS = 33
TRACE_CALLS = 3
STEPS = ("nearest", "correspondences", "correspondences, mutual")
KERNELS = r"\b(k_match_[a-z_]+|k_match<\d+, \d+>|k_scan_[a-z_]+)"


def summarise():
    """kernel_trace.csv of the traced run -> per case and step (the order of the traced run) the mean milliseconds of every kernel by
    name over the calls after the warm-up one.  A call begins at its first k_match_pack (it packs the sources, then the targets)."""
    rows = []
    for f in glob.glob(os.path.join(a.summarise, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, packs = [], 0
    for r in rows:
        m = re.search(KERNELS, r["Kernel_Name"].replace("pcpx::(anonymous namespace)::", ""))
        if not m:
            continue
        name, ms = m.group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        if name == "k_match_pack":
            packs += 1
            if packs % 2 == 1:
                calls.append({})
        if calls:
            k = calls[-1].setdefault(name, [0.0, 0])
            k[0] += ms
            k[1] += 1
    per_case = len(STEPS) * (1 + TRACE_CALLS)
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own: tools/match_rate.py --trace-run); milliseconds per call "
                   "(and launches per call), mean over %d calls after one warm-up call" % TRACE_CALLS, "dims": DIMS, "cases": []}
    for c, (m, n) in enumerate(CASES):
        mine = calls[c * per_case:(c + 1) * per_case]
        per = {"case": "%d x %d" % (m, n)}
        for s, label in enumerate(STEPS):
            group = mine[s * (1 + TRACE_CALLS) + 1:(s + 1) * (1 + TRACE_CALLS)]
            if not group:
                continue
            kernels = {k: [round(float(np.mean([g.get(k, [0.0, 0])[0] for g in group])), 4), group[0][k][1]] for k in group[0]}
            per[label] = {"kernels": kernels, "all kernels of the call": round(sum(v[0] for v in kernels.values()), 4)}
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


def fpfh_like(rows, seed):
    g = np.random.default_rng(seed).gamma(0.5, size=(rows, 3, 11)).astype(np.float32)
    return np.ascontiguousarray((np.float32(100) * g / g.sum(2, keepdims=True)).reshape(rows, 33), np.float32)


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / reps, 3)


def cdist_top2(d_src, d_tgt):
    """nearest and second nearest by torch: cdist over chunks of the sources, topk(2) of each chunk"""
    step = max(1, (1 << 28) // d_tgt.shape[0])
    idx = [torch.cdist(d_src[i:i + step], d_tgt).topk(2, dim=1, largest=False).indices for i in range(0, d_src.shape[0], step)]
    return torch.cat(idx)


res = {"device": torch.cuda.get_device_name(0), "dims": DIMS, "reps": a.reps, "library": os.path.basename(capi.LIB_PATH), "cases": {}}
for m, n in CASES:
    src, tgt = fpfh_like(m, 17), fpfh_like(n, 18)
    d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    d_idx = torch.empty(m, dtype=torch.int32, device=dev)
    d_d2, d_d22 = torch.empty(m, dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.float32, device=dev)
    d_pairs = torch.empty((m, 2), dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    nearest = lambda: pkg.match_nearest_dev(d_src, m, d_tgt, n, DIMS, d_idx, d_d2, None, d_d22)  # noqa: E731
    corr = lambda: pkg.match_correspondences_dev(d_src, m, d_tgt, n, DIMS, d_pairs, d_d2, d_count, max_ratio=0.9, mutual=False)  # noqa: E731
    mutual = lambda: pkg.match_correspondences_dev(d_src, m, d_tgt, n, DIMS, d_pairs, d_d2, d_count, max_ratio=0.9, mutual=True)  # noqa: E731
    if a.trace_run:
        for fn in (nearest, corr, mutual):
            for _ in range(1 + TRACE_CALLS):
                fn()
        torch.cuda.synchronize()
        continue
    case = "%d x %d" % (m, n)
    out = {"plan": pkg.match_plan(m, n, DIMS)}
    ms = timed(nearest, a.reps)
    out["nearest"] = {"call_ms": ms, "pairs per second": round(m * n / (ms * 1e-3), 0)}
    out["correspondences (ratio 0.9)"] = {"call_ms": timed(corr, a.reps), "kept": int(d_count.cpu()[0])}
    out["correspondences (ratio 0.9, mutual)"] = {"call_ms": timed(mutual, a.reps), "kept": int(d_count.cpu()[0])}
    # the cdist route, same tensors
    nearest()
    torch.cuda.synchronize()
    ours = d_idx.cpu().numpy().view(np.uint32)
    theirs = cdist_top2(d_src, d_tgt)[:, 0].cpu().numpy().astype(np.uint32)
    out["torch.cdist + topk(2), chunked"] = {"call_ms": timed(lambda: cdist_top2(d_src, d_tgt), max(1, a.reps // 3)),
                                             "best indices that differ from the exact ones": int((ours != theirs).sum())}
    # the kd search at 16 columns, host forms of both, m capped
    mk = min(m, a.kd_m)
    s16, t16 = np.ascontiguousarray(src[:mk, :16]), np.ascontiguousarray(tgt[:, :16])
    kd = pkg.KdTreeK(t16)
    kd_fn = lambda: kd.nearest_neighbours(s16, 2, eps=0.0, want_d2=True)  # noqa: E731
    ours_fn = lambda: pkg.match_nearest(s16, t16)  # noqa: E731
    ki, _kc, kd2 = kd_fn()
    oi, od, oi2, od2 = ours_fn()
    same = bool(np.array_equal(ki[:, 0], oi) and np.array_equal(ki[:, 1], oi2) and np.array_equal(kd2[:, 0].view(np.uint32), od.view(np.uint32)) and
                np.array_equal(kd2[:, 1].view(np.uint32), od2.view(np.uint32)))
    kd_ms, ours_ms = timed(kd_fn, max(1, a.reps // 3)), timed(ours_fn, a.reps)
    d_s16, d_t16 = torch.from_numpy(s16).to(dev), torch.from_numpy(t16).to(dev)
    dev16 = timed(lambda: pkg.match_nearest_dev(d_s16, mk, d_t16, n, 16, d_idx, d_d2, None, d_d22), a.reps)
    out["dims = 16, %d x %d" % (mk, n)] = {"pcpx_kd_knn_batch(k = 2, eps = 0), host form_ms": kd_ms, "match_nearest, host form_ms": ours_ms,
                                          "kd / match (host forms)": round(kd_ms / ours_ms, 1), "match_nearest_dev_ms": dev16,
                                          "same indices and d2 bits": same}
    kd.close()
    print(case, json.dumps(out), flush=True)
    res["cases"][case] = out
    del d_src, d_tgt, d_s16, d_t16
    torch.cuda.empty_cache()
if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
