#!/usr/bin/env python3
"""Poisson-disk subsampling (pcpx_subsample_self_dev) on one device, in one run on the seeded clouds of
sections 16 and 17 at --n points: uniform at r = 0.01 and r = 0.0071, clustered (synthetic.py) at r = 0.0023 (radii scaled by
(10 M / n)^(1/3) for another n).  Beside each case, from the same run:
  - the count form on the same cloud (pcpx_range_count_self_dev: one walk -- the floor);
  - the call with keep + kept rows + count, and with owners too; the rounds it issued;
  - the composed route as the library offered it before: pcpx_range_lists_self_dev on the device, the lists' download, and the
    sequential greedy loop of tests/subsample_model.py on the host.  The host part is timed on a cloud of --host-n points of the
    same kind with the radius scaled to the same mean count and scaled to n by list entries (and said so in the output).
Call times are device-synchronised host clocks over --reps calls after warm-up.
The library under test is PCPX_LIB (default: the package's libpcpx.so); --label names it in the output.  How many rounds go between
two reads of the decided counter (PCPX_SUBSAMPLE_ROUND_BATCH of include/pcpx_subsample.h) was chosen by running this on builds with
the constant at 1, 2 and 4.
Kernel times -- every round of a call on its own -- come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/subsample_rate.py --trace-run
    python tools/subsample_rate.py --summarise DIR --kernels-out profiles/r12_subsample_kernels.json
python tools/subsample_rate.py [--n N] [--host-n M] [--reps R] [--out FILE] [--no-composed] [--label TEXT]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_subsample.json"))
ap.add_argument("--no-composed", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--summarise", default=None)
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r12_subsample_kernels.json"))
a = ap.parse_args()
n = int(a.n)
CASES = (("uniform", 0.01), ("uniform", 0.0071), ("clustered", 0.0023))
SEED = 0
TRACE_CALLS = 3


def summarise():
    """kernel_trace.csv of the traced run -> per case: the count form, and per call (mean over the calls after the warm-up one) every
    round's milliseconds in order and the other kernels' by name.  A call begins at k_subsample_init; a case at the k_range launches
    before it."""
    rows = []
    for f in glob.glob(os.path.join(a.summarise, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases, cur = [], None
    for r in rows:
        m = re.search(r"\b(k_subsample_[a-z_]+|k_scan_[a-z_]+|k_range<true, false>)", r["Kernel_Name"].replace("pcpx::(anonymous namespace)::", ""))
        if not m:
            continue
        name, ms = m.group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        if name.startswith("k_range"):
            if cur is None or cur["calls"]:
                cur = {"count": [], "calls": []}
                cases.append(cur)
            cur["count"].append(ms)
            continue
        if name == "k_subsample_init":
            cur["calls"].append({"rounds": [], "others": {}})
        call = cur["calls"][-1]
        if name == "k_subsample_round":
            call["rounds"].append(ms)
        else:
            call["others"][name] = call["others"].get(name, 0.0) + ms
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own: tools/subsample_rate.py --trace-run); milliseconds, mean over "
                   "%d calls after one warm-up call; each case: the calls without owners, then the calls with.  'every round' lists the round "
                   "LAUNCHES the call issued, a multiple of PCPX_SUBSAMPLE_ROUND_BATCH (include/pcpx_subsample.h) of the traced library: "
                   "the trailing ones may run over a cloud that is decided already and return after one load per group" % TRACE_CALLS,
           "n": n, "cases": []}
    for (kind, r10), c in zip(CASES, cases):
        per = {"case": "%s, r = %g" % (kind, r10), "count form k_range": round(float(np.mean(c["count"][1:])), 4)}
        for label, calls in (("keep + kept rows", c["calls"][1:1 + TRACE_CALLS]), ("with owners", c["calls"][2 + TRACE_CALLS:])):
            rounds = np.array([k["rounds"] for k in calls])
            others = {k: round(float(np.mean([q["others"][k] for q in calls])), 4) for k in calls[0]["others"]}
            per[label] = {"rounds": int(rounds.shape[1]), "every round": [round(float(v), 4) for v in rounds.mean(0)],
                          "all rounds": round(float(rounds.sum(1).mean()), 4), "other kernels": others,
                          "all kernels of the call": round(float(rounds.sum(1).mean()) + sum(others.values()), 4)}
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
    """lists on the device at n and their download; the host greedy loop at host_n with the radius scaled to the same mean count"""
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
    m = min(int(a.host_n), max(50_000, int(4e7 / max(mean_count, 1.0))))  # (at most ~40 M list entries on the host)
    import cluster_model as CM
    import subsample_model as M
    pts = make_cloud(kind, m)
    ix = pkg.LinkedOctree(pts)
    rm = float(np.float32(r * (n / m) ** (1.0 / 3.0)))
    offs, ind = ix.range_sphere(pts, rm)
    res["host part: points"] = m
    res["host part: radius (same mean count)"] = rm
    res["host part: list entries"] = int(len(ind))
    t0 = time.perf_counter()
    src, dst, _ = CM.edges_from_lists(offs, ind)
    keep = M.greedy(m, src, dst, SEED)
    ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(np.nonzero(keep)[0], ix.subsample(rm, SEED))
    res["host greedy loop (numpy model)_ms"] = round(ms, 1)
    res["host greedy loop, scaled to n by list entries_ms"] = round(ms * total / max(1, len(ind)), 1)
    ix.close()
    return res


res = {"device": torch.cuda.get_device_name(0), "n": n, "reps": a.reps, "library": a.label or os.path.basename(capi.LIB_PATH),
       "rounds between two reads of the counter": a.label or capi.PCPX_SUBSAMPLE_ROUND_BATCH,
       "rounds": "the round launches the call issued: a multiple of the line above, the last of them possibly over a decided cloud", "cases": {}}
last_kind = None
for kind, r10 in CASES:
    r = float(np.float32(r10 * (10e6 / n) ** (1.0 / 3.0)))
    if kind != last_kind:
        if last_kind is not None:
            IX.close()
            del d_pts
            torch.cuda.empty_cache()
        pts = make_cloud(kind, n)
        d_pts = torch.from_numpy(pts).to(dev)
        IX = pkg.Index.from_device(d_pts.data_ptr(), n)
        last_kind = kind
    case = "%s %d points, r = %.6g" % (kind, n, r)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    own = torch.empty(n, dtype=torch.int32, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    plain = lambda: IX.subsample_dev(r, keep.data_ptr(), seed=SEED, d_kept_rows=kept.data_ptr(), d_kept_count=total.data_ptr())  # noqa: E731
    owners = lambda: IX.subsample_dev(r, keep.data_ptr(), seed=SEED, d_owner=own.data_ptr(), d_kept_rows=kept.data_ptr(),  # noqa: E731
                                      d_kept_count=total.data_ptr())
    if a.trace_run:
        for fn in (lambda: IX.range_count_self_dev(r, cnt.data_ptr()), plain, owners):
            for _ in range(1 + TRACE_CALLS):
                fn()
        torch.cuda.synchronize()
        continue
    out = {"radius": r}
    IX.range_count_self_dev(r, cnt.data_ptr())
    torch.cuda.synchronize()
    out["mean count"] = round(float(cnt.double().mean().item()), 2)
    floor = out["count form (pcpx_range_count_self_dev)_ms"] = timed(lambda: IX.range_count_self_dev(r, cnt.data_ptr()), a.reps)
    out["rounds"] = plain()
    ms = timed(plain, a.reps)
    torch.cuda.synchronize()
    out["kept"] = int(total.item())
    out["call (keep + kept rows + count)_ms"] = ms
    out["ratio to the count form"] = round(ms / floor, 2)
    out["per round, call / rounds_ms"] = round(ms / out["rounds"], 3)
    ms = timed(owners, a.reps)
    out["call with owners_ms"] = ms
    out["with owners: ratio to the count form"] = round(ms / floor, 2)
    if not a.no_composed:
        out["composed route"] = composed(kind, r, out["mean count"])
        lists = out["composed route"].get("lists on the device (pcpx_range_lists_self_dev)_ms")
        down = [v for k, v in out["composed route"].items() if k.startswith("download")]
        if lists is not None and down:
            tot = lists + down[0] + out["composed route"]["host greedy loop, scaled to n by list entries_ms"]
            out["composed route end to end_ms (lists + download at n, host part scaled)"] = round(tot, 1)
            out["composed / fused"] = round(tot / out["call (keep + kept rows + count)_ms"], 1)
    print(case, json.dumps(out), flush=True)
    res["cases"][case] = out
if not a.trace_run:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
