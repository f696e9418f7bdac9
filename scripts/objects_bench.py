"""Object batches (Final_Project/scripts/detect.py:269-354) on a KITTI-shaped labelled scene: about 30 000 labelled points in planted
objects of 5 to 10 000 points plus noise rows.  Device milliseconds (pcr_timer_*, HIP events on the context's stream) and wall
milliseconds of the three device steps -- grouping + statistics (ObjectBatch), resampling weights, pack -- and of preprocess_device as a
whole, beside the reference's host loop over objects (SciPy pdist + squareform + column mean, then np.random.choice and the gather),
timed once.  Every timed call gets the same draws (np.random.seed before it); the first call of each kind is not reported.  The device's
weights are compared with the host loop's bit for bit.  Writes profiles/objects_bench.json.

    python scripts/objects_bench.py [--reps 10] [--no-host-loop] [--out profiles/objects_bench.json]
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
pcp = importlib.import_module("point-cloud-process_amd")

SIZES = [10_000, 5_000, 2_500, 1_800, 1_200] + [800, 650, 500, 420, 350, 300] * 2 + [200, 150, 120, 90, 64, 40, 25, 12, 5] * 3
CONFIG = {"max_radius_distance": 75.0, "num_sample_points": 64, "batch_size": 16}


def planted_scene(seed=0, n_noise=6_000):
    """-> (points float32 (n,3), normals float64 (n,3), object_ids int64 (n,)): anisotropic blobs (walls, cars, poles) between 3 and
    70 m from the sensor, rows shuffled."""
    rng = np.random.default_rng(seed)
    pts, ids = [], []
    for o, n in enumerate(SIZES):
        ang, r = rng.uniform(-np.pi, np.pi), rng.uniform(3.0, 70.0)
        extent = np.array([0.4, 0.4, 0.5]) * max(1.0, (n / 200.0) ** 0.5) * rng.uniform(0.5, 2.0, size=3)
        pts.append(np.array([r * np.cos(ang), r * np.sin(ang), rng.uniform(-1.5, 0.5)]) + rng.normal(scale=extent, size=(n, 3)))
        ids += [o] * n
    pts.append(np.column_stack([rng.uniform(-80, 80, n_noise), rng.uniform(-80, 80, n_noise), rng.uniform(-2, 2, n_noise)]))
    ids += [-1] * n_noise
    points = np.concatenate(pts).astype(np.float32)
    ids = np.array(ids, dtype=np.int64)
    order = rng.permutation(len(ids))
    nrm = rng.normal(size=(len(ids), 3))
    return np.ascontiguousarray(points[order]), np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)), ids[order]


def host_loop(points, normals, object_ids, config):
    """detect.py:284-320 at its cost -> (seconds in pdist + squareform + mean, seconds in all, weights per kept object)."""
    import scipy.spatial.distance

    t_pd, t0, weights = 0.0, time.perf_counter(), {}
    for object_id in range(max(object_ids) + 1):
        mask = object_ids == object_id
        if mask.sum() <= 4:
            continue
        centre = np.mean(points[mask], axis=0)[:2]
        if np.sqrt((centre * centre).sum()) > config["max_radius_distance"]:
            continue
        points_, normals_ = np.copy(points[mask]), np.copy(normals[mask])
        n = len(points_)
        t1 = time.perf_counter()
        w = scipy.spatial.distance.squareform(scipy.spatial.distance.pdist(points_, "euclidean")).mean(axis=0)
        t_pd += time.perf_counter() - t1
        weights[object_id] = w.copy()
        w /= w.sum()
        idx = np.random.choice(np.arange(n), size=(config["num_sample_points"],), replace=config["num_sample_points"] > n, p=w)
        np.hstack((points_[idx] - points_.mean(axis=0), normals_[idx]))
    return t_pd, time.perf_counter() - t0, weights


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
            "wall_ms_median": float(np.median(wall)), "wall_ms_min": float(wall.min()), "wall_ms_max": float(wall.max()), "reps": int(len(dev))}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.json"))
    a = ap.parse_args()
    points, normals, ids = planted_scene()
    points64 = points.astype(np.float64)
    ctx = pcp.default_context()
    counts = np.bincount(ids[ids >= 0])
    out = {"device": ctx.device_info(), "n": int(len(ids)), "labelled": int((ids >= 0).sum()), "objects": int(len(counts)),
           "object_size_min": int(counts.min()), "object_size_max": int(counts.max()), "config": CONFIG, "np_random_seed": a.seed,
           "distance_terms": int((counts.astype(np.int64) ** 2).sum()), "runs": {}}
    dc = pcp.DeviceCloud.upload(points, ctx)
    batch = pcp.ObjectBatch(dc, ids)
    st = batch.stats()
    keep = pcp.objects.select(st["count"], st["mean"], CONFIG["max_radius_distance"])
    out["kept_objects"] = int(keep.sum())
    out["kept_distance_terms"] = int((counts[keep].astype(np.int64) ** 2).sum())

    def build():
        b = pcp.ObjectBatch(dc, ids)
        b.free()

    S = CONFIG["num_sample_points"]
    kept = np.flatnonzero(keep)
    slots = np.concatenate([kept, np.full(-len(kept) % CONFIG["batch_size"], kept[0])])
    idx = np.stack([np.arange(S) % counts[o] for o in slots])
    X = torch.empty((len(slots), S, 6), dtype=torch.float32, device=f"cuda:{ctx.device}")
    torch.cuda.synchronize()

    dev, wall, _ = timed(ctx, build, a.reps, a.seed)
    out["runs"]["group_and_stats"] = stats(dev, wall)
    dev, wall, w_dev = timed(ctx, lambda: batch.weights(keep), a.reps, a.seed)
    out["runs"]["weights"] = dict(stats(dev, wall), distance_terms_per_s=out["kept_distance_terms"] / (1e-3 * float(np.median(dev))))
    dev, wall, _ = timed(ctx, lambda: batch.pack(slots, idx, X.data_ptr(), normals), a.reps, a.seed)
    out["runs"]["pack"] = dict(stats(dev, wall), slots=int(len(slots)))
    dev, wall, res = timed(ctx, lambda: pcp.preprocess_device(dc, ids, CONFIG, normals=normals), a.reps, a.seed)
    out["runs"]["preprocess_device"] = dict(stats(dev, wall), batch=list(res[0].shape), N=int(res[2]))
    for k, v in out["runs"].items():
        print(k, json.dumps(v), flush=True)
    if not a.no_host_loop:
        np.random.seed(a.seed)
        t_pd, t_all, w_host = host_loop(points64, normals, ids, CONFIG)
        out["host_loop_s"] = t_all
        out["host_pdist_squareform_mean_s"] = t_pd
        same = all(np.array_equal(w_dev[batch.offsets[o]:batch.offsets[o + 1]], w) for o, w in w_host.items())
        out["weights_bit_equal_to_scipy"] = bool(same and sorted(w_host) == kept.tolist())
        print("host loop", t_all, "s, of which pdist + squareform + mean", t_pd, "s; weights bit-equal:", out["weights_bit_equal_to_scipy"], flush=True)
    batch.free()
    dc.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
