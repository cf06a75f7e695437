#!/usr/bin/env python3
"""Moving least squares projection (pcpx_mls_project_self_dev) on one device, in one run on the seeded clouds
of tools/range_neighbourhoods_rate.py:
  (a) 10 M uniform points, r = 0.01 (~42 neighbours);
  (b) the same cloud at the radius that holds ~15 points;
  (c) the clustered cloud of synthetic.py at the radius of its median 42nd-neighbour distance.
Per case, with gauss_h = r / 2:
  the floor: pcpx_range_neighbourhoods_self_dev, normals + centroids (the unweighted moments walk);
  order 1 (one walk with a weight per neighbour) with points + normals, and with every output;
  order 2 (the second walk and the 6 x 6 solve) with points + normals, and with every output;
and on (a) the existing denoiser: one round of the bilateral points loop (bilateral_filter_points, a host-pointer call: its time
includes the copies of the cloud and the normals to the device and of the points back).
Call times are device-synchronised host clocks over `reps` calls after warm-up; "range_kernel_ms (events)" is the index's own
event profile.  Kernel times come from a run of its own under the profiler, then summarised:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mls_rate.py --no-bilateral --out DIR/traced.json
    python tools/mls_rate.py --summarise DIR [--kernels-out FILE]
python tools/mls_rate.py [--n N] [--reps R] [--out FILE] [--no-bilateral]"""
import argparse
import csv
import glob
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=float, default=10e6)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_mls.json"))
ap.add_argument("--no-bilateral", action="store_true")
ap.add_argument("--summarise", default=None, help="directory of a traced run: write the kernels' times per case and step")
ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "r22_mls_kernels.json"))
a = ap.parse_args()
n = int(a.n)
CASES = ("(a) uniform r=0.01", "(b) uniform ~15 neighbours", "(c) clustered ~42 neighbours (median)")
STEPS = ("order 1: points + normals", "order 1: every output", "order 2: points + normals", "order 2: every output")
FLOOR = "floor: moments form, normals + centroids (pcpx_range_neighbourhoods_self_dev)"


def summarise():
    """kernel_trace.csv of the traced run -> per case and step the mean milliseconds of k_range_moments, k_mls_plane and k_mls_poly
    over the `reps` launches after the two warm-up ones (the launches of a kernel come in the run's order: case, step, call)."""
    rows = []
    for f in glob.glob(os.path.join(a.summarise, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = {"k_range_moments<true, 1>": [], "k_mls_plane<true>": [], "k_mls_poly<true>": []}
    for r in rows:
        for name in ms:
            if name + "(" in r["Kernel_Name"]:
                ms[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    per = 2 + a.reps
    assert len(ms["k_range_moments<true, 1>"]) == 3 * per and len(ms["k_mls_plane<true>"]) == 12 * per and len(ms["k_mls_poly<true>"]) == 6 * per, \
        {k: len(v) for k, v in ms.items()}
    mean = lambda v, call: round(float(np.mean(v[call * per + 2:(call + 1) * per])), 4)
    out = {"what": "kernel times from rocprofv3 --kernel-trace (a run of its own); milliseconds, mean over %d launches after two warm-up "
                   "ones" % a.reps, "n": n, "cases": {}}
    for c, case in enumerate(CASES):
        res = {FLOOR: {"k_range_moments<true, 1>": mean(ms["k_range_moments<true, 1>"], c)}}
        for s, step in enumerate(STEPS):
            res[step] = {"k_mls_plane<true>": mean(ms["k_mls_plane<true>"], 4 * c + s)}
            if s >= 2:
                res[step]["k_mls_poly<true>"] = mean(ms["k_mls_poly<true>"], 2 * c + s - 2)
        out["cases"][case] = res
    with open(a.kernels_out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if a.summarise:
    summarise()
    sys.exit(0)

import torch  # noqa: E402

pkg = importlib.import_module("point-cloud-processing_amd")
dev = torch.device("cuda", 0)


def timed(fn, reps=a.reps, ix=None):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    if ix is not None:
        ix.profile_begin()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {"call_ms": round((time.perf_counter() - t0) * 1e3 / reps, 3)}
    if ix is not None:
        out["range_kernel_ms (events)"] = round(ix.profile_end()["range"][1] / reps, 3)
    return out


def cloud_index(pts):
    d_pts = torch.from_numpy(pts).to(dev)
    return d_pts, pkg.Index.from_device(d_pts.data_ptr(), len(pts))


def self_forms(ix, r, label):
    f3 = lambda: torch.empty((n, 3), dtype=torch.float32, device=dev)
    P, D, nrm, cen = f3(), f3(), f3(), f3()
    cv = torch.empty((n, 2), dtype=torch.float32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    fit = torch.empty(n, dtype=torch.int32, device=dev)
    res = {"radius": r, "gauss_h": r / 2}
    res[FLOOR] = timed(
        lambda: ix.range_neighbourhoods_self_dev(r, d_normals=nrm.data_ptr(), d_centroids=cen.data_ptr()), ix=ix)
    every = dict(d_points=P.data_ptr(), d_displacements=D.data_ptr(), d_normals=nrm.data_ptr(), d_curvatures=cv.data_ptr(),
                 d_counts=cnt.data_ptr(), d_fit=fit.data_ptr())
    for order in (1, 2):
        res["order %d: points + normals" % order] = timed(
            lambda: ix.mls_project_self_dev(r, None, order, d_points=P.data_ptr(), d_normals=nrm.data_ptr()), ix=ix)
        res["order %d: every output" % order] = timed(lambda: ix.mls_project_self_dev(r, None, order, **every), ix=ix)
        res["order %d: fits 0 / 1 / 2" % order] = [int((fit == v).sum().item()) for v in (0, 1, 2)]
    res["mean_neighbours"] = round(float(cnt.double().mean().item()), 2)
    res["checksum displacement norm sum (order 2)"] = round(float(D.double().norm(dim=1).sum().item()), 6)
    print(label, json.dumps(res), flush=True)
    return res, nrm


res = {"device": torch.cuda.get_device_name(0), "n": n, "reps": a.reps}
pts = pkg.synthetic.uniform_cloud(n, 43)
d_pts, ix = cloud_index(pts)
res[CASES[0]], d_nrm = self_forms(ix, 0.01, "(a)")
if not a.no_bilateral:
    nrm = d_nrm.cpu().numpy()
    res["(a) bilateral points loop, one round (host-pointer call, sigmaf = r, sigmag = r / 2)"] = timed(
        lambda: pkg.filters.bilateral_filter_points(pts, nrm, sigmaf=0.01, sigmag=0.005, K=1), reps=3)
    print("bilateral", json.dumps(res["(a) bilateral points loop, one round (host-pointer call, sigmaf = r, sigmag = r / 2)"]), flush=True)
r15 = (15.0 / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)
res[CASES[1]], _ = self_forms(ix, float(np.float32(r15)), "(b)")
ix.close()
del d_pts, d_nrm
torch.cuda.empty_cache()
pts = pkg.synthetic.clustered_cloud(n)
d_pts, ix = cloud_index(pts)
sample = pts[np.random.default_rng(1).choice(n, 2000, replace=False)]
_, _, d2 = ix.knn(sample, 42, 0.0, want_d2=True)
res[CASES[2]], _ = self_forms(ix, float(np.median(np.sqrt(d2[:, 41]))), "(c)")
ix.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
