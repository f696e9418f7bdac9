"""Label match (Final_Project/scripts/extract.py:514-566) on the labelled scene of scripts/objects_bench.py: 28 658 labelled points in
44 objects of 5 to 10 000 points plus noise rows, 20 labels -- 14 drawn round objects, 6 over empty space.  Device milliseconds
(pcr_timer_*, HIP events on the context's stream: upload of the records, the one launch, the read-back) and wall milliseconds of
``ObjectBatch.match_labels`` alone, wall milliseconds of ``match_labels`` from a cloud already on the device (grouping included), and
beside them, on the same box's host, the reference-shaped loop: per label a radius query (SciPy ``cKDTree.query_ball_point`` standing in
for Open3D's tree, built once per frame and timed apart), three ``np.dot``, the box mask, ``np.unique`` and ``max``.  Two calls of each
kind warm up and are not reported; the sides alternate within every repetition; medians of the repetitions.  The two sides' k, object
ids and counts are compared.  Writes profiles/label_match_bench.json.

    python scripts/label_match_bench.py [--reps 20] [--out profiles/label_match_bench.json] [--kernel-stats <rocprofv3 kernel_stats.csv>]

--kernel-stats: merge the row of label_match_kernel from a ``rocprofv3 --kernel-trace --stats`` run OF ITS OWN into the JSON (the
timings above are taken with the profiler off).
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
pcp = importlib.import_module("point-cloud-process_amd")
from kitti_boxes_bench import calibration, stats  # noqa: E402
from objects_bench import planted_scene  # noqa: E402

WARMUP = 2
N_ON_OBJECTS, N_EMPTY = 14, 6


def make_labels(points, ids, param, seed=3):
    """-> a frame with read_label's columns: boxes of 1.2 x the extent of every third object at a random yaw, then boxes over empty space."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    counts = np.bincount(ids[ids >= 0])
    rows = []
    for o in np.argsort(-counts)[::3][:N_ON_OBJECTS]:
        P = points[ids == o]
        centre, ext = P.mean(axis=0), 1.2 * (P.max(axis=0) - P.min(axis=0))
        l = w = max(ext[0], ext[1])
        rows.append((centre, ext[2], w, l, rng.uniform(-np.pi, np.pi)))
    for _ in range(N_EMPTY):
        rows.append((np.array([rng.uniform(100, 120), rng.uniform(-20, 20), 0.0]), 1.5, 1.6, 3.9, rng.uniform(-np.pi, np.pi)))
    out = []
    for centre, h, w, l, ry in rows:
        c = pcp.transform_to_cam(centre[None, :], param)[0]
        out.append(["Car", 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, h, w, l, c[0], c[1] + h / 2, c[2], ry, centre[0], centre[1], centre[2],
                    np.linalg.norm(0.5 * np.asarray([h, w, l]))])
    return pd.DataFrame(out, columns=pcp.extract.LABEL_COLUMNS + ["vx", "vy", "vz", "radius"])


def host_loop(tree, points, object_ids, param, df_label):
    """extract.py:514-566 at its cost -> (seconds, [(k, object id or -1, N)])."""
    t0 = time.perf_counter()
    R0, Tr = param["R0_rect"], param["Tr_velo_to_cam"]
    out = []
    for _, label in df_label.iterrows():
        center_velo = np.asarray([label["vx"], label["vy"], label["vz"]])
        center_cam = np.asarray([label["cx"], label["cy"], label["cz"]])
        dims = np.asarray([label["length"], label["height"], label["width"]])
        idx = np.asarray(tree.query_ball_point(center_velo, label["radius"]), dtype=np.int64)
        if len(idx) == 0:
            out.append((0, -1, 0))
            continue
        X_velo, object_ids_ = points[idx], object_ids[idx]
        X_cam = np.dot(R0, (np.dot(Tr[:, 0:3], X_velo.T).T + Tr[:, 3]).T).T
        cos_ry, sin_ry = np.cos(label["ry"]), np.sin(label["ry"])
        R = np.asarray([[cos_ry, 0.0, sin_ry], [0.0, 1.0, 0.0], [-sin_ry, 0.0, cos_ry]])
        X_obj = np.dot(R.T, (X_cam - center_cam).T).T
        X_obj[:, 1] += label["height"] / 2
        idx_obj = np.all(np.logical_and(X_obj >= -dims / 2, X_obj <= dims / 2), axis=1)
        if idx_obj.sum() == 0:
            out.append((len(idx), -1, 0))
            continue
        found, counts = np.unique(object_ids_[idx_obj], return_counts=True)
        object_id_, _ = max(zip(found, counts), key=lambda x: x[1])
        idx_object = idx[object_ids_ == object_id_]
        points[idx_object].mean(axis=0)
        out.append((len(idx), int(object_id_), len(idx_object)))
    return time.perf_counter() - t0, out


def kernel_row(path):
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "label_match_kernel" in row.get("Name", ""):
                return {key: (float(v) if v.replace(".", "", 1).isdigit() else v) for key, v in row.items()}
    raise SystemExit(f"{path}: no row for label_match_kernel")


def main():
    from scipy.spatial import cKDTree

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_match_bench.json"))
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            out = json.load(f)
        out["rocprofv3_kernel_stats"] = kernel_row(a.kernel_stats)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out["rocprofv3_kernel_stats"]))
        return
    points, _, ids = planted_scene()
    points64 = points.astype(np.float64)
    param = calibration()
    ctx = pcp.default_context()
    df = make_labels(points64, ids, param)
    records = pcp.label_records(df)
    labelled = np.flatnonzero(ids >= 0)
    P_lab, ids_lab = points64[labelled], ids[labelled]      # a noise row belongs to no object of the library: the host loop sees the labelled rows
    counts = np.bincount(ids[ids >= 0])
    out = {"device": ctx.device_info(), "n": int(len(ids)), "labelled": int(len(labelled)), "objects": int(len(counts)), "object_size_min": int(counts.min()),
           "object_size_max": int(counts.max()), "labels": int(len(df)), "labels_on_objects": N_ON_OBJECTS, "warmup": WARMUP, "ms": {}}
    dc = pcp.DeviceCloud.upload(points, ctx)
    batch = pcp.ObjectBatch(dc, ids)
    t = {"match_labels_device": [], "match_labels_wall": [], "match_labels_from_device_cloud_wall": [], "host_tree_build_wall": [], "host_loop_wall": []}
    m = host = None
    for rep in range(a.reps + WARMUP):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        m = batch.match_labels(param, records)
        d = ctx.timer_stop_ms()
        w = [1e3 * (time.perf_counter() - t0)]
        t0 = time.perf_counter()
        pcp.match_labels(dc, ids, df, param)       # (returns after the read-back: the device is idle)
        w.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        tree = cKDTree(P_lab)
        w.append(1e3 * (time.perf_counter() - t0))
        s, host = host_loop(tree, P_lab, ids_lab, param, df)
        if rep >= WARMUP:
            for key, v in zip(t, [d] + w + [1e3 * s]):
                t[key].append(v)
    out["ms"] = {key: stats(v) for key, v in t.items()}
    device_side = list(zip(m["k"].tolist(), m["object_id"].tolist(), m["count"].tolist()))
    out["labels_with_an_object"] = int((m["object_id"] >= 0).sum())
    out["rows_in_spheres"] = int(m["k"].sum())
    out["selected_rows"] = int(m["count"].sum())
    out["labels_differing_from_host_loop"] = int(sum(a_ != b_ for a_, b_ in zip(device_side, host)))
    batch.free()
    dc.free()
    for key, v in out["ms"].items():
        print(key, json.dumps(v), flush=True)
    print("labels differing from the host loop:", out["labels_differing_from_host_loop"], "of", len(df), "; with an object:", out["labels_with_an_object"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
