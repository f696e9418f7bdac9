"""PCLKeypoint on a KITTI-shaped scan: ``kitti_like_scan(120000)`` at radius 1.0 (salient 1.0 / non-max 0.7 for the PCL-rule ISS).

Whole calls: wall milliseconds (host clock around a call that ends in a device synchronise) and device milliseconds (pcr_timer_*, HIP
events on the context's stream) of ``keypointHarris3D`` (is_nms False / True / True with refine), ``keypointIss``,
``estimate_normals_radius`` and, as the yardstick of the same neighbourhood structure, ``iss_keypoints`` (pcr_iss) at the same radius --
from a cloud already on the device, medians over --reps after two warm-up calls, the calls alternating within every repetition.
Beside them, once, on the same machine's host: the NumPy restatement (tests/harris_checks.py) with SciPy's cKDTree.

Kernels: per-kernel times come from a profiler run of their own,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o st -- python scripts/harris_bench.py --prof
    python scripts/harris_bench.py --fold-stats DIR/**/st_kernel_stats.csv
which adds every pass's average to the JSON, with nanoseconds per (row, neighbour) pair visited -- sum over rows of |N(p_i)| pairs per
pass -- next to pcr_iss's two passes.  Writes profiles/harris_bench.json.

    python scripts/harris_bench.py [--reps 10] [--no-host] [--out profiles/harris_bench.json]
"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcp = importlib.import_module("point-cloud-process_amd")
from tests import harris_checks as hc  # noqa: E402

WARMUP = 2
N, RADIUS, NON_MAX, THRESHOLD, GAMMA, MIN_NB = 120_000, 1.0, 0.7, 0.001, 0.975, 5
KERNELS = {   # pass -> (substring of the kernel's name, radius whose pairs it visits)
    "harris_position_covariance": ("harris_poscov_kernel<false>", "radius"),
    "iss_pcl_scatter": ("harris_poscov_kernel<true>", "radius"),
    "harris_normal_covariance": ("harris_response_kernel", "radius"),
    "suppression": ("harris_suppress_kernel", None),   # both detectors' launches; candidates only walk their ball
    "refine": ("harris_refine_kernel", None),
    "pcr_iss_count": ("iss_count_kernel", "radius"),
    "pcr_iss_weighted_scatter": ("iss_cov_kernel", "radius"),
}


def calls(dc, ctx):
    return {
        "keypointHarris3D": lambda: pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, ctx=ctx),
        "keypointHarris3D_nms": lambda: pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, ctx=ctx),
        "keypointHarris3D_nms_refine": lambda: pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, is_refine=True, ctx=ctx),
        "keypointIss": lambda: pcp.keypointIss(dc, RADIUS, NON_MAX, GAMMA, GAMMA, MIN_NB, ctx=ctx),
        "estimate_normals_radius": lambda: pcp.estimate_normals_radius(dc, RADIUS, ctx=ctx),
        "iss_keypoints_pcr_iss": lambda: pcp.iss_keypoints(dc, radius=RADIUS, non_max_radius=RADIUS, ctx=ctx),
    }


def stats(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "reps": int(len(v))}


def fold_stats(paths, out_path):
    with open(out_path) as f:
        out = json.load(f)
    rows = []
    for p in paths:
        with open(p) as f:
            rows += list(csv.DictReader(f))
    kernels = {}
    for key, (needle, pairs_of) in KERNELS.items():
        hit = [r for r in rows if needle in r["Name"]]
        if not hit:
            continue
        calls_n = sum(int(r["Calls"]) for r in hit)
        avg_us = sum(float(r["TotalDurationNs"]) for r in hit) / calls_n / 1e3
        kernels[key] = {"kernel": needle, "launches": calls_n, "avg_us": avg_us, "min_us": min(float(r["MinNs"]) for r in hit) / 1e3,
                        "max_us": max(float(r["MaxNs"]) for r in hit) / 1e3}
        if pairs_of:
            kernels[key]["ns_per_pair"] = 1e3 * avg_us / out["pairs_within_radius"]
    out["kernels"] = kernels
    out["kernels_source"] = "rocprofv3 --kernel-trace --stats, a run of its own (scripts/harris_bench.py --prof)"
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for key, v in kernels.items():
        print(key, json.dumps(v), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--prof", action="store_true", help="three calls of each kind and nothing else (the profiler's run)")
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy / cKDTree restatement")
    ap.add_argument("--fold-stats", nargs="+", metavar="CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harris_bench.json"))
    a = ap.parse_args()
    if a.fold_stats:
        return fold_stats(a.fold_stats, a.out)
    points = np.ascontiguousarray(pcp.synthetic.kitti_like_scan(N)[:, :3], dtype=np.float64)
    ctx = pcp.default_context()
    dc = pcp.DeviceCloud.upload(points, ctx)
    todo = calls(dc, ctx)
    if a.prof:
        for _ in range(3):
            for fn in todo.values():
                fn()
        dc.free()
        return
    _, det = pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, return_details=True, ctx=ctx)
    out = {"device": ctx.device_info(), "n": int(len(points)), "radius": RADIUS, "non_max_radius": NON_MAX, "threshold": THRESHOLD, "gamma": GAMMA,
           "min_neighbors": MIN_NB, "warmup": WARMUP, "pairs_within_radius": int(det["counts"].astype(np.int64).sum()),
           "neighbours_median": float(np.median(det["counts"])), "neighbours_max": int(det["counts"].max())}
    wall = {k: [] for k in todo}
    dev = {k: [] for k in todo}
    results = {}
    for rep in range(a.reps + WARMUP):
        for key, fn in todo.items():
            ctx.sync()
            t0 = time.perf_counter()
            ctx.timer_start()
            results[key] = fn()          # (returns after its read-back: the device is idle)
            d = ctx.timer_stop_ms()
            w = 1e3 * (time.perf_counter() - t0)
            if rep >= WARMUP:
                wall[key].append(w)
                dev[key].append(d)
    out["wall_ms"] = {k: stats(v) for k, v in wall.items()}
    out["device_ms"] = {k: stats(v) for k, v in dev.items()}
    out["keypoints"] = {"harris_nms": int(len(results["keypointHarris3D_nms"])), "iss_pcl": int(len(results["keypointIss"])),
                        "pcr_iss": int(len(results["iss_keypoints_pcr_iss"]))}
    for k in todo:
        print(k, "wall", json.dumps(out["wall_ms"][k]), "device", json.dumps(out["device_ms"][k]), flush=True)
    dc.free()
    if not a.no_host:
        t0 = time.perf_counter()
        ref = hc.harris3d(points, RADIUS, THRESHOLD, nms=True)
        t_h = time.perf_counter() - t0
        print("host restatement, Harris with suppression: %.1f s" % t_h, flush=True)
        t0 = time.perf_counter()
        ref_i = hc.iss_pcl(points, RADIUS, NON_MAX, GAMMA, GAMMA, MIN_NB)
        t_i = time.perf_counter() - t0
        print("host restatement, PCL-rule ISS: %.1f s" % t_i, flush=True)
        got = pcp.keypointHarris3D(points, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, return_indices=True, ctx=ctx)[1]
        got_i = pcp.keypointIss(points, RADIUS, NON_MAX, GAMMA, GAMMA, MIN_NB, return_indices=True, ctx=ctx)[1]
        out["host_restatement"] = {"what": "tests/harris_checks.py: SciPy cKDTree ball queries + NumPy per row, one run, same machine's host",
                                   "harris_nms_s": t_h, "iss_pcl_s": t_i, "harris_keypoints": int(len(ref["rows"])), "iss_keypoints": int(len(ref_i["rows"])),
                                   "harris_rows_differing_from_device": int(len(np.setxor1d(got, ref["rows"]))),
                                   "harris_contested_rows": int((ref["contested"] & ref["candidates"]).sum()),
                                   "iss_rows_differing_from_device": int(len(np.setxor1d(got_i, ref_i["rows"])))}
        print(json.dumps(out["host_restatement"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
