"""Point-to-plane refinement (refine_registration, Registration/main.py:87-95) on a 120 000-point perturbed_pair: device and
wall milliseconds per iteration and per call, beside pcr_icp's per-iteration time on the same pair and box.  The target normals
come from estimate_normals_hybrid (radius 2 * voxel_size, 30 neighbours); the gate is 0.4 * voxel_size (main.py:88), voxel_size 2.0
(main.py:196).  Writes profiles/p2plane_bench.json.

    python scripts/p2plane_bench.py [--n 120000] [--reps 10] [--out profiles/p2plane_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=120_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--voxel-size", type=float, default=2.0)   # main.py:196
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2plane_bench.json"))
    a = ap.parse_args()
    src, tgt, T_true = pcp.synthetic.perturbed_pair(a.n, seed=0)
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    ctx = pcp.default_context()
    gate = 0.4 * a.voxel_size   # main.py:88
    t0 = time.perf_counter()
    normals = pcp.estimate_normals_hybrid(tgt, radius=2.0 * a.voxel_size, max_nn=30, ctx=ctx)
    normals_ms = 1e3 * (time.perf_counter() - t0)
    out = {"device": ctx.device_info(), "n_source": int(len(src)), "n_target": int(len(tgt)), "max_correspondence_distance": gate,
           "normals_hybrid_ms": normals_ms, "runs": {}}
    for kind in ("grid", "brute"):
        index = pcp.TargetIndex(tgt, kind=kind, ctx=ctx).set_normals(normals)
        sd = pcp.DeviceCloud.upload(src, ctx).prepare(index)
        rows = []
        for rep in range(a.reps + 1):   # the first call (arena growth, code load) is not reported
            ctx.sync()
            t0 = time.perf_counter()
            r = pcp.icp_point2plane_device(sd, index, np.eye(4), max_correspondence_distance=gate)
            wall = 1e3 * (time.perf_counter() - t0)
            if rep:
                rows.append((r["device_ms"], wall, r["nn_launches"]))
        dev, wall, passes = (np.array(c, dtype=np.float64) for c in zip(*rows))
        err = float(np.abs(r["T"] - T_true).max())
        # pcr_icp on the same pair: composed-transform mode, the same number of passes, the gate on the squared distance
        p2p_rows = []
        for rep in range(a.reps + 1):
            s2 = pcp.DeviceCloud.upload(src, ctx).prepare(index)
            ctx.sync()
            q = pcp.icp_device(s2, index, np.eye(4), mode="total", max_iter=int(passes[-1]), min_iter=int(passes[-1]), r_thres=-1.0, t_thres=-1.0,
                               max_d2=gate * gate)
            s2.free()
            if rep:
                p2p_rows.append(q["device_ms"] / max(q["nn_launches"], 1))
        out["runs"][kind] = {
            "iterations": int(r["iters"]), "passes": int(passes[-1]), "fitness": r["fitness"], "inlier_rmse": r["inlier_rmse"], "status": int(r["status"]),
            "max_abs_T_minus_truth": err,
            "device_ms_per_call_median": float(np.median(dev)), "wall_ms_per_call_median": float(np.median(wall)),
            "device_ms_per_pass_median": float(np.median(dev / passes)), "device_ms_per_pass_min": float((dev / passes).min()),
            "wall_ms_per_pass_median": float(np.median(wall / passes)),
            "pcr_icp_device_ms_per_pass_median": float(np.median(p2p_rows)),
        }
        print(kind, json.dumps(out["runs"][kind]), flush=True)
        sd.free()
        index.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
