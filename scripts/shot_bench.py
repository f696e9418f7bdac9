"""SHOT352 at keypoint positions on a KITTI-shaped scan: ``kitti_like_scan(120000)`` at radius 1.0, the case of pcl_fpfh_bench.py.

Keypoint sets: the Harris-3D keypoints of the scan (radius 1.0, threshold 0.001, suppressed) and 400 / 1 600 / 6 400 rows drawn at
random (the same draws as pcl_fpfh_bench.py).  Normals: ``estimate_normals_knn(k=10)``.  Per set, from a cloud already on the device,
medians over --reps after two warm-up calls:
    wall_ms     host clock around ``shot352_with_normal`` -- host normals and keypoints in, float32 rows out, ends in a synchronise
    device_ms   HIP events around the same call (pcr_timer_*)
    stage_ms    HIP events between the stages of pcr_shot352 (pcr_profile_*): frames, histogram
and beside them ``fpfh33_with_normal`` at the same set, and ``shot_lrf`` alone.  The tie walk: the keypoints whose sign count is
balanced for either sign of a final axis are counted on the host from the device's frames, and the frames stage is timed on those
keypoints alone and on as many others.  Once, on the same machine's host, the NumPy restatement (tests/shot_checks.py) of the Harris
set, with the largest difference between the two.

    python scripts/shot_bench.py [--reps 10] [--no-host] [--out profiles/shot_bench.json]
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
from tests import shot_checks as sc  # noqa: E402

WARMUP = 2
N, RADIUS, THRESHOLD, K_NORMALS = 120_000, 1.0, 0.001, 10
STAGES = ("frames", "histogram")


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


def balanced(points, kp, frames):
    """Per keypoint: whether the sign count of its x or z axis is balanced for the final axis or for its negative (the tie walk ran)."""
    out = np.zeros(len(kp), dtype=bool)
    for i, b in enumerate(pf.balls(points, kp, RADIUS)):
        if len(b) < 5:
            continue
        v = points[b] - kp[i]
        for a in (frames[i, 0], frames[i, 2]):
            t = (v[:, 0] * a[0] + v[:, 1] * a[1]) + v[:, 2] * a[2]
            pos, neg, zero = int((t > 0).sum()), int((t < 0).sum()), int((t == 0).sum())
            out[i] |= pos + zero == neg or neg + zero == pos
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shot_bench.json"))
    a = ap.parse_args()
    points = np.ascontiguousarray(pcp.synthetic.kitti_like_scan(N)[:, :3], dtype=np.float64)
    ctx = pcp.default_context()
    dc = pcp.DeviceCloud.upload(points, ctx)
    out = {"device": ctx.device_info(), "library": os.path.basename(pcp._lib.LIB_PATH), "n": int(len(points)), "radius": RADIUS, "normals_k": K_NORMALS, "warmup": WARMUP,
           "what": "wall_ms: host in, host out; device_ms: HIP events around the call; stage_ms: HIP events between the stages of pcr_shot352 (frames, histogram)"}
    nrm = pcp.estimate_normals_knn(dc, K_NORMALS, ctx=ctx)
    harris, harris_rows = pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, return_indices=True, ctx=ctx)
    rng = np.random.default_rng(0)
    sets = {"harris": points[harris_rows]}
    for m in (400, 1600, 6400):
        sets["random_%d" % m] = points[rng.choice(len(points), m, replace=False)]
    out["sets"] = {}
    results = {}
    for name, kp in sets.items():
        w, d, st, (f, info) = timed(ctx, lambda: pcp.shot352_with_normal(dc, nrm, kp, RADIUS, ctx=ctx, return_info=True), a.reps)
        results[name] = (f, info)
        counts = info["counts"]
        e = {"m": int(len(kp)), "ball_median": float(np.median(counts)), "ball_max": int(counts.max()), "ball_min": int(counts.min()),
             "nan_rows": int(np.isnan(f).any(axis=1).sum()), "wall_ms": w, "device_ms": d, "stage_ms": st}
        if st:
            e["frames_us_per_keypoint"] = 1e3 * st["frames"] / len(kp)
            e["histogram_us_per_keypoint"] = 1e3 * st["histogram"] / len(kp)
            e["histogram_ns_per_neighbour"] = 1e6 * st["histogram"] / max(int(counts.sum()), 1)
        w2, d2, _, _ = timed(ctx, lambda: pcp.shot_lrf(dc, kp, RADIUS, ctx=ctx), a.reps)
        e["shot_lrf"] = {"wall_ms": w2, "device_ms": d2}
        w3, d3, _, _ = timed(ctx, lambda: pcp.fpfh33_with_normal(dc, nrm, kp, RADIUS, ctx=ctx), a.reps)
        e["fpfh33_with_normal"] = {"wall_ms": w3, "device_ms": d3}
        tie = balanced(points, kp, info["frames"])
        e["tie_keypoints"] = int(tie.sum())
        k = int(min(tie.sum(), (~tie).sum()))
        if k:
            for label, sel in (("ties_only", np.flatnonzero(tie)[:k]), ("no_ties_same_count", np.flatnonzero(~tie)[:k])):
                sub = np.ascontiguousarray(kp[sel])
                _, d4, _, (_, c4) = timed(ctx, lambda: pcp.shot_lrf(dc, sub, RADIUS, ctx=ctx, return_counts=True), a.reps)
                e["shot_lrf_" + label] = {"m": k, "ball_median": float(np.median(c4)), "device_ms": d4}
        out["sets"][name] = e
        print(name, json.dumps(e), flush=True)
    dc.free()
    if not a.no_host:
        kp = sets["harris"]
        f, info = results["harris"]
        t0 = time.perf_counter()
        ref = sc.shot352(points, nrm, kp, RADIUS, frames=info["frames"])
        t_h = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref_lrf = sc.lrf(points, kp, RADIUS)
        t_l = time.perf_counter() - t0
        both = ~np.isnan(ref["values"]).any(axis=1)
        good = (ref_lrf["gap"] > 1e-3) & (ref_lrf["sign_margin"] > 1e-9) & (ref_lrf["counts"] >= 5)
        dots = np.einsum("kij,kij->ki", info["frames"][good], ref_lrf["frames"][good])
        out["host_restatement"] = {"what": "tests/shot_checks.py on the harris set: SciPy cKDTree ball queries + NumPy, one run, same machine's host; the histogram from the device's frames",
                                   "histogram_seconds": t_h, "frames_seconds": t_l, "counts_equal": bool(np.array_equal(ref["counts"], info["counts"])),
                                   "max_abs_difference_float32_rows": float(np.abs(f[both] - ref["values"][both].astype(np.float32)).max(initial=0.0)),
                                   "well_conditioned_share": float(good.mean()), "smallest_frame_row_dot": float(dots.min(initial=1.0))}
        print(json.dumps(out["host_restatement"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
