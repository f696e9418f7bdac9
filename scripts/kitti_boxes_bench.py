"""KITTI label rows (Final_Project/scripts/detect.py:56-194) on the labelled scene of scripts/objects_bench.py: 28 658 labelled points
in 44 objects of 5 to 10 000 points plus noise rows.  Device milliseconds (pcr_timer_*, HIP events on the context's stream) and wall
milliseconds of ``ObjectBatch.kitti_boxes`` alone, wall milliseconds of ``to_kitti_eval_format`` end to end (grouping, the box kernel,
the DataFrame) from a cloud already on the device and from host arrays, and beside them, on the same box's host, the reference-shaped
NumPy loop: per object a mask over the whole cloud, three ``np.dot``, ``np.cov``, ``np.linalg.eig``, the min / max.  Every object is
predicted (classes cycle through cyclist, pedestrian, vehicle).  Two calls of each kind warm up and are not reported; the sides
alternate within every repetition.  The device's numbers are compared with the host loop's.  Writes profiles/kitti_boxes_bench.json.

    python scripts/kitti_boxes_bench.py [--reps 20] [--out profiles/kitti_boxes_bench.json]
"""
import argparse
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
from objects_bench import planted_scene  # noqa: E402

WARMUP = 2
DECODER = {0: "cyclist", 1: "pedestrian", 2: "vehicle", 3: "misc"}


def calibration():
    """A calibration of KITTI's shape: the camera looks along the sensor's x axis."""
    c, s = np.cos(0.01), np.sin(0.01)
    rot = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return {"P2": np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]),
            "R0_rect": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]]),
            "Tr_velo_to_cam": np.hstack([rot, np.array([[-0.004], [-0.076], [-0.272]])])}


def host_loop(points, object_ids, param, predictions, decoder):
    """detect.py:91-167 at its cost, in NumPy (the Open3D box is a min / max here) -> (seconds, {object_id: 11 numbers})."""
    t0 = time.perf_counter()
    R0, Tr, P2 = param["R0_rect"], param["Tr_velo_to_cam"], param["P2"]
    out = {}
    for class_id in predictions:
        if decoder[class_id] == "misc":
            continue
        for object_id in predictions[class_id]:
            X_velo = points[object_ids == object_id]
            X_cam = np.dot(R0, (np.dot(Tr[:, 0:3], X_velo.T).T + Tr[:, 3]).T).T
            X_pixel = np.dot(P2[:, 0:3], X_cam.T).T + P2[:, 3]
            X_pixel = (X_pixel[:, :2].T / X_pixel[:, 2]).T
            top_left, bottom_right = X_pixel.min(axis=0), X_pixel.max(axis=0)
            c_center = X_cam.mean(axis=0)
            X_cam_centered = X_cam - c_center
            eigenvalues, eigenvectors = np.linalg.eig(np.cov(X_cam_centered[:, [0, 2]], rowvar=False, bias=True))
            eigenvectors = eigenvectors[:, eigenvalues.argsort()[::-1]]
            ry = np.arctan2(-eigenvectors[0][1], eigenvectors[0][0])
            cos_ry, sin_ry = np.cos(-ry), np.sin(-ry)
            R = np.asarray([[cos_ry, 0.0, sin_ry], [0.0, 1.0, 0.0], [-sin_ry, 0.0, cos_ry]])
            X_obj = np.dot(R.T, X_cam_centered.T).T
            extent = X_obj.max(axis=0) - X_obj.min(axis=0)
            out[int(object_id)] = [f"{v:.2f}" for v in (top_left[0], top_left[1], bottom_right[0], bottom_right[1], extent[1], extent[0], extent[2],
                                                         c_center[0], c_center[1], c_center[2], ry)]
    return time.perf_counter() - t0, out


def stats(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "reps": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_boxes_bench.json"))
    a = ap.parse_args()
    points, _, ids = planted_scene()
    points64 = points.astype(np.float64)
    param = calibration()
    ctx = pcp.default_context()
    counts = np.bincount(ids[ids >= 0])
    predictions = {c: {} for c in range(4)}
    for o in range(len(counts)):
        predictions[o % 3][o] = 0.5 + 0.01 * (o % 40)
    out = {"device": ctx.device_info(), "n": int(len(ids)), "labelled": int((ids >= 0).sum()), "objects": int(len(counts)),
           "object_size_min": int(counts.min()), "object_size_max": int(counts.max()), "lds_rows": int(pcp.detection.LDS_ROWS),
           "objects_on_chip": int((counts <= pcp.detection.LDS_ROWS).sum()), "warmup": WARMUP,
           "record_bytes_read": int(32 * (counts.sum() + 2 * counts[counts > pcp.detection.LDS_ROWS].sum())), "ms": {}}
    dc = pcp.DeviceCloud.upload(points, ctx)
    batch = pcp.ObjectBatch(dc, ids)
    t = {"kitti_boxes_device": [], "kitti_boxes_wall": [], "to_kitti_eval_format_device_cloud_wall": [], "to_kitti_eval_format_host_arrays_wall": [],
         "host_loop_wall": []}
    boxes = label = host = None
    for rep in range(a.reps + WARMUP):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        boxes = batch.kitti_boxes(param)
        d = ctx.timer_stop_ms()
        w = [1e3 * (time.perf_counter() - t0)]
        for arg in (dc, points):
            t0 = time.perf_counter()
            label = pcp.to_kitti_eval_format(arg, ids, param, predictions, DECODER)   # (returns after the read-back: the device is idle)
            w.append(1e3 * (time.perf_counter() - t0))
        s, host = host_loop(points64, ids, param, predictions, DECODER)
        if rep >= WARMUP:
            for key, v in zip(t, [d] + w + [1e3 * s]):
                t[key].append(v)
    out["ms"] = {key: stats(v) for key, v in t.items()}
    # the same rows on both sides
    fields = ("left", "top", "right", "bottom", "height", "width", "length", "cx", "cy", "cz", "ry")
    order = [o for c in predictions if DECODER[c] != "misc" for o in predictions[c]]
    differing = sum(label[f][r] != host[o][i] for r, o in enumerate(order) for i, f in enumerate(fields))
    out["label_strings"] = int(len(order) * len(fields))
    out["label_strings_differing_from_host_loop"] = int(differing)
    out["boxes_finite"] = bool(np.isfinite(boxes).all())
    batch.free()
    dc.free()
    for key, v in out["ms"].items():
        print(key, json.dumps(v), flush=True)
    print("label strings differing from the host loop:", differing, "of", out["label_strings"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
