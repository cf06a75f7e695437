#!/usr/bin/env python3
"""Outlier removal (include/pcpx_outliers.h) on one device, on the seeded clouds of section 16 at --n points:
uniform (r = 0.01 at 10 M, scaled by (10 M / n)^(1/3) for another n) and clustered (synthetic.py, at the median 42nd-neighbour
distance).  Every comparison is between variants that ALTERNATE in one process (a, b, a, b, ...), each call timed by a pair of
device events after warm-up; beside every median stands the spread of the same code in that run (the medians of its even and of its
odd calls).
  statistical   the whole call (keep + kept rows + count + mean distances) beside pcpx_neighbourhoods_self_dev (mean distance
                only) at the same k: the difference is the tail (two sums, the cut, keep, scan, compact).  Its bytes -- the n floats
                read three times, the mask written and read three times, the scan's places written and read, the kept rows -- over
                that time, beside a device-to-device copy of as many bytes in the same run.
  radius        the at-least form (no counts asked for) against the count form (counts asked for), min_neighbours 2, 5, 16.
  density       the same two forms behind the resolution at k = 15, radius_scale 2.
  host baseline the composition through the host calls that existed before (mean_knn_distance_self, numpy, range_count_self,
                numpy) beside density_outliers (host arrays) and density_outliers_dev, host clock, device-synchronised.
python tools/outlier_removal_rate.py [--n N] [--rounds R] [--out FILE] [--clouds uniform,clustered]"""
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
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_outliers.json"))
ap.add_argument("--clouds", default="uniform,clustered")
a = ap.parse_args()
n = int(a.n)
pkg = importlib.import_module("point-cloud-processing_amd")
dev = torch.device("cuda", 0)


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


def host_timed(fn, reps=2):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / reps, 2)


res = {"device": torch.cuda.get_device_name(0), "n": n, "rounds": a.rounds,
       "timing": "device events round each call, variants alternating in one process, medians; milliseconds", "clouds": {}}
for kind in a.clouds.split(","):
    pts = pkg.synthetic.uniform_cloud(n, 43) if kind == "uniform" else pkg.synthetic.clustered_cloud(n)
    d_pts = torch.from_numpy(pts).to(dev)
    ix = pkg.Index.from_device(d_pts.data_ptr(), n)
    if kind == "uniform":
        r = float(np.float32(0.01 * (10e6 / n) ** (1.0 / 3.0)))
    else:
        sample = pts[np.random.default_rng(1).choice(n, 2000, replace=False)]
        r = float(np.median(np.sqrt(ix.knn(sample, 42, 0.0, want_d2=True)[2][:, 41])))
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    rows = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    out = {"radius": r}

    # ---- statistical: the whole call beside the neighbour search alone
    for k in (15, 32):
        t = alternating({
            "pcpx_neighbourhoods_self_dev (mean distance only)": lambda: ix.neighbourhoods_self_dev(k, 1e-5, d_meandist=dist.data_ptr()),
            "statistical_outliers_dev (keep + rows + count + mean distances)":
                lambda: ix.statistical_outliers_dev(keep, k, 2.0, d_kept_rows=rows, d_kept_count=total, d_mean_dist=dist, d_stats=stats),
        })
        kept = int(total.item())
        tail_ms = t["statistical_outliers_dev (keep + rows + count + mean distances)"]["median_ms"] - \
            t["pcpx_neighbourhoods_self_dev (mean distance only)"]["median_ms"]
        # n floats x 3 (two sums, keep), mask written once and read by the scan twice and the compaction once, places written and read
        tail_bytes = n * (3 * 4 + 1 + 3 * 1 + 2 * 4) + 4 * kept
        src = torch.empty(tail_bytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = alternating({"copy": lambda: dst.copy_(src)}, rounds=6)["copy"]["median_ms"]  # (reads and writes tail_bytes in all)
        del src, dst
        t["tail (the difference of the medians)_ms"] = round(tail_ms, 4)
        t["tail bytes"] = tail_bytes
        t["tail GB/s"] = round(tail_bytes / max(tail_ms, 1e-6) * 1e-6, 1)
        t["device-to-device copy moving as many bytes_ms"] = round(copy, 4)
        t["copy GB/s"] = round(tail_bytes / copy * 1e-6, 1)
        t["tail / whole call_%"] = round(100.0 * tail_ms / t["statistical_outliers_dev (keep + rows + count + mean distances)"]["median_ms"], 2)
        t["kept"] = kept
        t["stats (mean, std, cut, usable)"] = stats.cpu().tolist()
        out["statistical k = %d, ratio 2" % k] = t
        print(kind, k, json.dumps(t), flush=True)

    # ---- radius: the at-least form against the count form
    for at_least in (2, 5, 16):
        t = alternating({
            "count form (counts asked for)": lambda: ix.radius_outliers_dev(r, keep, at_least, d_kept_rows=rows, d_kept_count=total, d_count=cnt),
            "at-least form": lambda: ix.radius_outliers_dev(r, keep, at_least, d_kept_rows=rows, d_kept_count=total),
        })
        t["at-least / count"] = round(t["at-least form"]["median_ms"] / t["count form (counts asked for)"]["median_ms"], 4)
        t["kept"] = int(total.item())
        out["radius, min_neighbours = %d" % at_least] = t
        print(kind, "radius", at_least, json.dumps(t), flush=True)
    out["mean count at the radius"] = round(float(cnt.double().mean().item()), 2)
    t = alternating({"pcpx_range_count_self_dev": lambda: ix.range_count_self_dev(r, cnt.data_ptr())})
    out["floor: the count walk alone"] = t["pcpx_range_count_self_dev"]

    # ---- density: the same two forms behind the resolution
    t = alternating({
        "count form (counts asked for)": lambda: ix.density_outliers_dev(keep, 15, 2.0, 5, d_kept_rows=rows, d_kept_count=total, d_count=cnt, d_stats=stats),
        "at-least form": lambda: ix.density_outliers_dev(keep, 15, 2.0, 5, d_kept_rows=rows, d_kept_count=total, d_stats=stats),
    })
    t["kept"] = int(total.item())
    t["stats (mean, std, radius, usable)"] = stats.cpu().tolist()
    out["density k = 15, scale 2, min_neighbours = 5"] = t
    print(kind, "density", json.dumps(t), flush=True)

    # ---- the host composition that existed before, beside the one call
    def composed():
        md = ix.mean_knn_distance_self(15)
        radius = np.float32(2.0) * np.mean(md, dtype=np.float32)
        return np.flatnonzero(ix.range_count_self(radius) >= 5)

    out["host baseline"] = {
        "mean_knn_distance_self + numpy + range_count_self + numpy_ms": host_timed(composed),
        "density_outliers (host arrays, one call)_ms": host_timed(lambda: ix.density_outliers(15, 2.0, 5)),
        "density_outliers_dev (device arrays, one call)_ms": host_timed(
            lambda: ix.density_outliers_dev(keep, 15, 2.0, 5, d_kept_rows=rows, d_kept_count=total), reps=5),
    }
    print(kind, "host", json.dumps(out["host baseline"]), flush=True)
    res["clouds"]["%s, %d points" % (kind, n)] = out
    ix.close()
    del d_pts, ix, keep, rows, dist, cnt
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
