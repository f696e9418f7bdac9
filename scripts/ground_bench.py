"""Ground removal ahead of DBSCAN (Cluster_dbscan/clustering.py:36-95, 158-160) on a 120 000-point kitti_like_scan: device
milliseconds (pcr_timer_*, HIP events on the context's stream) and wall milliseconds of ground_segmentation on a resident cloud and of
segment_and_cluster, beside plain DBSCAN on the whole scan; the reference's NumPy loop (35 x n Python iterations) once on the host.
Every timed call gets the same triples (np.random.seed before it).  Writes profiles/ground_bench.json.

    python scripts/ground_bench.py [--n 120000] [--reps 10] [--no-host-loop] [--out profiles/ground_bench.json]
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcp = importlib.import_module("point-cloud-process_amd")


def reference_loop(data, tau=0.6, trials=35, ratio=0.5):
    """What clustering.py:50-83 computes, at its cost: float32 arithmetic, one interpreter iteration per point and trial, one draw of
    three rows per trial (a degenerate triple gives a NaN normal, no inliers, and is not redrawn)."""
    total = data.shape[0]
    top, kept = 0, None
    for _ in range(trials):
        tri = data[np.random.randint(0, total, size=3)]
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm = np.cross(tri[0] - tri[1], tri[0] - tri[2])
            nrm = nrm / np.linalg.norm(nrm)
        outside = []
        for i in range(total):
            if not math.fabs(np.dot(data[i] - tri[0], nrm)) < tau:
                outside.append(i)
        inside = total - len(outside)
        if inside > top:
            top, kept = inside, outside
            if top / total > ratio:
                break
    return data[kept]


def timed(ctx, fn, reps, seed):
    """-> (device ms, wall ms) per repetition; the first call (arena growth, code load) is not reported."""
    dev, wall, last = [], [], None
    for rep in range(reps + 1):
        np.random.seed(seed)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        last = fn()
        d = ctx.timer_stop_ms()
        w = 1e3 * (time.perf_counter() - t0)
        if rep:
            dev.append(d)
            wall.append(w)
    return np.array(dev), np.array(wall), last


def stats(dev, wall):
    return {"device_ms_median": float(np.median(dev)), "device_ms_min": float(dev.min()), "device_ms_max": float(dev.max()),
            "wall_ms_median": float(np.median(wall)), "wall_ms_min": float(wall.min()), "reps": int(len(dev))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=120_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_bench.json"))
    a = ap.parse_args()
    scan = np.ascontiguousarray(pcp.synthetic.kitti_like_scan(a.n, seed=0)[:, :3], dtype=np.float32)
    ctx = pcp.default_context()
    out = {"device": ctx.device_info(), "n": int(len(scan)), "tau": 0.6, "N": 35, "ratio": 0.5, "np_random_seed": a.seed, "runs": {}}
    dc = pcp.DeviceCloud.upload(scan, ctx)

    def ground_resident():
        seg = pcp.ground_segmentation(dc)
        m = seg.n
        seg.free()
        return m

    def pipeline_resident():
        seg, labels = pcp.segment_and_cluster(dc)
        seg.free()
        return labels

    def dbscan_whole():
        clus = pcp.DBSCAN(0.5, 10, ctx=ctx)
        clus.fit(dc)
        return clus.predict()

    np.random.seed(a.seed)
    _, info = pcp.ground_segmentation(scan, return_info=True)
    out["best_hyp"], out["evaluated"] = info["best_hyp"], info["evaluated"]
    out["n_inliers"], out["n_outliers"] = info["n_inliers"], info["n_outliers"]
    dev, wall, m = timed(ctx, ground_resident, a.reps, a.seed)
    out["runs"]["ground_segmentation_resident"] = stats(dev, wall)
    dev, wall, _ = timed(ctx, lambda: pcp.ground_segmentation(scan), a.reps, a.seed)
    out["runs"]["ground_segmentation_host_array"] = stats(dev, wall)   # upload + step + row list back + host gather
    dev, wall, labels = timed(ctx, pipeline_resident, a.reps, a.seed)
    out["runs"]["segment_and_cluster_resident"] = dict(stats(dev, wall), clusters=int(labels.max() + 1), points_clustered=int(len(labels)))
    dev, wall, labels = timed(ctx, dbscan_whole, max(1, a.reps // 3), a.seed)
    out["runs"]["dbscan_whole_scan"] = dict(stats(dev, wall), clusters=int(labels.max() + 1), points_clustered=int(len(labels)))
    for k, v in out["runs"].items():
        print(k, json.dumps(v), flush=True)
    if not a.no_host_loop:
        np.random.seed(a.seed)
        t0 = time.perf_counter()
        ref = reference_loop(scan)
        out["reference_numpy_loop_s"] = time.perf_counter() - t0
        out["reference_outliers"] = int(len(ref))
        print("reference loop", out["reference_numpy_loop_s"], "s,", len(ref), "outliers; device:", m, flush=True)
    dc.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
