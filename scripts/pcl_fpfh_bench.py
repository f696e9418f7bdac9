"""PCL-rule FPFH33 at keypoint positions on a KITTI-shaped scan: ``kitti_like_scan(120000)`` at radius 1.0, the Harris bench's case.

Keypoint sets: the Harris-3D keypoints of the scan (radius 1.0, threshold 0.001, suppressed), the same refined (coordinates that are
no cloud rows), and 400 / 1 600 / 6 400 rows drawn at random.  Normals: ``estimate_normals_knn(k=10)``, timed on its own.
Per set, from a cloud already on the device, medians over --reps after two warm-up calls:
    wall_ms     host clock around ``fpfh33_with_normal`` -- host normals and keypoints in, float32 rows out, ends in a synchronise
    device_ms   HIP events around the same call (pcr_timer_*)
    stage_ms    HIP events between the stages of pcr_fpfh_pcl (pcr_profile_*): mark, compact, SPFH, FPFH
For context, no target (it follows Open3D's rules: hybrid neighbourhood capped at max_nn = 100, own SPFH added):
``compute_fpfh_at_rows`` at the same rows, where the keypoints are rows.  And once, on the same machine's host, the NumPy / cKDTree
restatement (tests/pcl_fpfh_checks.py) of the 400-row set, with the largest difference between the two.

    python scripts/pcl_fpfh_bench.py [--reps 10] [--no-host] [--out profiles/pcl_fpfh_bench.json]

("sizing" in the committed profiles/pcl_fpfh_bench.json is the one measurement of a retired A/B build that read M back and sized the SPFH
block by it: DESIGN.md section 3.6.0.1.  A fresh run of this script does not write it.)
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcp = importlib.import_module("point-cloud-process_amd")
from tests import pcl_fpfh_checks as pf  # noqa: E402

WARMUP = 2
N, RADIUS, THRESHOLD, K_NORMALS, MAX_NN = 120_000, 1.0, 0.001, 10, 100
STAGES = ("mark", "compact", "spfh", "fpfh")


def stats(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "reps": int(len(v))}


def timed(ctx, fn, reps):
    """-> (wall stats, device stats, stage medians or None, last result)"""
    L = pcp._lib
    wall, dev, stage = [], [], []
    res = None
    for rep in range(reps + WARMUP):
        L.check(L.lib().pcr_profile_enable(ctx.handle, 1), ctx.handle)      # (zeroes the stage sums)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        res = fn()
        d = ctx.timer_stop_ms()
        w = 1e3 * (time.perf_counter() - t0)
        ms = (C.c_double * 4)()
        passes = C.c_int()
        L.check(L.lib().pcr_profile_read(ctx.handle, ms, C.byref(passes)), ctx.handle)
        if rep >= WARMUP:
            wall.append(w)
            dev.append(d)
            if passes.value == 1:
                stage.append(list(ms))
    L.check(L.lib().pcr_profile_enable(ctx.handle, 0), ctx.handle)
    st = {s: float(np.median([r[i] for r in stage])) for i, s in enumerate(STAGES)} if stage else None
    return stats(wall), stats(dev), st, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy / cKDTree restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcl_fpfh_bench.json"))
    a = ap.parse_args()
    points = np.ascontiguousarray(pcp.synthetic.kitti_like_scan(N)[:, :3], dtype=np.float64)
    ctx = pcp.default_context()
    dc = pcp.DeviceCloud.upload(points, ctx)
    out = {"device": ctx.device_info(), "library": os.path.basename(pcp._lib.LIB_PATH), "n": int(len(points)), "radius": RADIUS, "normals_k": K_NORMALS, "warmup": WARMUP,
           "what": "wall_ms: host in, host out; device_ms: HIP events around the call; stage_ms: HIP events between the stages of pcr_fpfh_pcl"}
    w, d, _, nrm = timed(ctx, lambda: pcp.estimate_normals_knn(dc, K_NORMALS, ctx=ctx), a.reps)
    out["estimate_normals_knn"] = {"wall_ms": w, "device_ms": d}
    print("estimate_normals_knn", json.dumps(out["estimate_normals_knn"]), flush=True)
    harris, harris_rows = pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, return_indices=True, ctx=ctx)
    refined = pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, is_refine=True, ctx=ctx)
    rng = np.random.default_rng(0)
    sets = {"harris": (points[harris_rows], harris_rows), "harris_refined": (refined[:, :3].astype(np.float64), None)}
    for m in (400, 1600, 6400):
        rows = rng.choice(len(points), m, replace=False)
        sets["random_%d" % m] = (points[rows], rows)
    out["sets"] = {}
    results = {}
    for name, (kp, rows) in sets.items():
        w, d, st, (f, info) = timed(ctx, lambda: pcp.fpfh33_with_normal(dc, nrm, kp, RADIUS, ctx=ctx, return_info=True), a.reps)
        results[name] = (f, info)
        counts = info["counts"]
        e = {"m": int(len(kp)), "n_spfh": info["n_spfh"], "ball_median": float(np.median(counts)), "ball_max": int(counts.max()), "ball_min": int(counts.min()),
             "nan_rows": int(np.isnan(f).any(axis=1).sum()), "wall_ms": w, "device_ms": d, "stage_ms": st}
        if st and info["n_spfh"]:
            e["spfh_us_per_row"] = 1e3 * st["spfh"] / info["n_spfh"]
            e["fpfh_us_per_keypoint"] = 1e3 * st["fpfh"] / len(kp)
        if rows is not None:
            try:
                w2, d2, _, (_, info2) = timed(ctx, lambda: pcp.compute_fpfh_at_rows(dc, rows, nrm, RADIUS, MAX_NN, ctx=ctx, return_info=True), a.reps)
                e["context_compute_fpfh_at_rows"] = {"what": "Open3D rules, max_nn = %d: other values, context only" % MAX_NN, "n_spfh": info2["n_spfh"], "wall_ms": w2, "device_ms": d2}
            except pcp._lib.PcrError as err:
                e["context_compute_fpfh_at_rows"] = {"refused": str(err)}
        out["sets"][name] = e
        print(name, json.dumps(e), flush=True)
    dc.free()
    if not a.no_host:
        kp = sets["random_400"][0]
        t0 = time.perf_counter()
        ref = pf.fpfh33(points, nrm, kp, RADIUS)
        t_h = time.perf_counter() - t0
        f, info = results["random_400"]
        both = ~np.isnan(ref["values"]).any(axis=1)
        out["host_restatement"] = {"what": "tests/pcl_fpfh_checks.py on the random_400 set: SciPy cKDTree ball queries + NumPy, one run, same machine's host",
                                   "seconds": t_h, "n_spfh": int(ref["n_spfh"]), "counts_equal": bool(np.array_equal(ref["counts"], info["counts"])),
                                   "n_spfh_equal": bool(ref["n_spfh"] == info["n_spfh"]),
                                   "max_abs_difference_float32_rows": float(np.abs(f[both] - ref["values"][both].astype(np.float32)).max()),
                                   "clean_share": float((ref["margin"] > 1e-9).mean())}
        print(json.dumps(out["host_restatement"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
