"""K-Means fit (include/pcr.h: pcr_kmeans_fit) on a resident cloud: device milliseconds per iteration (pcr_kmeans_result.device_ms, HIP
events around the loop and the final pass, divided by the passes run: iterations + 1) and GB/s over the 32-byte records, for
k = 3, 8 and 32 at 120 000 and 1 000 000 points.  Beside each: the NumPy restatement on the host (tests/kmeans_checks.step, timed on
at most 200 000 of the points and scaled to n) and the Gaussian mixture's device milliseconds per EM iteration at the same (n, k),
measured in the same process (pcp.GMM, tol = -inf so that every run does max_iter iterations; two passes per iteration plus one).
The data are k broad, overlapping Gaussian blobs at lidar range, so that Lloyd's iteration does not settle within the iterations timed
(tolerance 0; the iterations actually run are recorded), the initial centres k data rows.  Writes profiles/kmeans_bench.json.

    python scripts/kmeans_bench.py [--reps 7] [--iters 20] [--no-host] [--no-gmm] [--out profiles/kmeans_bench.json]
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
from tests import kmeans_checks  # noqa: E402

HOST_POINTS = 200_000


def blobs(n, k, seed=0):
    rng = np.random.default_rng(seed)
    centres = np.column_stack([rng.uniform(-60, 60, k), rng.uniform(-60, 60, k), rng.uniform(-2, 2, k)])
    pts = centres[rng.integers(0, k, n)] + rng.normal(size=(n, 3)) * np.array([15.0, 20.0, 1.0])
    return pts, pts[rng.choice(n, k, replace=False)].copy()


def host_iteration_ms(data, centres0):
    """One tests/kmeans_checks.step (NumPy float64) on at most HOST_POINTS points -> ms scaled to len(data), points timed."""
    m = min(len(data), HOST_POINTS)
    t0 = time.perf_counter()
    kmeans_checks.step(data[:m], centres0)
    return 1e3 * (time.perf_counter() - t0) * len(data) / m, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-gmm", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.json"))
    a = ap.parse_args()
    ctx = pcp.default_context()
    out = {"device": ctx.device_info(), "max_iter": a.iters, "bytes_per_point_per_pass": 32, "runs": []}
    for n in (120_000, 1_000_000):
        for k in (3, 8, 32):
            data, c0 = blobs(n, k, seed=n + k)
            dc = pcp.DeviceCloud.upload(data, ctx)
            dev, wall, model = [], [], None
            for rep in range(a.reps + 1):     # the first call (arena growth, code load) is not reported
                ctx.sync()
                t0 = time.perf_counter()
                model = pcp.K_Means(k, tolerance=0.0, max_iter=a.iters).fit(dc, centers_init=c0, labels=False)
                w = 1e3 * (time.perf_counter() - t0)
                if rep:
                    dev.append(model.device_ms_)
                    wall.append(w)
            dev, wall = np.array(dev), np.array(wall)
            passes = model.n_iter_ + 1
            run = {"n": n, "k": k, "iterations_run": model.n_iter_, "passes": passes, "fit_device_ms_median": float(np.median(dev)),
                   "fit_device_ms_min": float(dev.min()), "fit_device_ms_max": float(dev.max()), "iteration_device_ms_median": float(np.median(dev)) / passes,
                   "fit_wall_ms_median": float(np.median(wall)), "reps": a.reps, "GB_per_s_streamed": 32.0 * n * passes / (np.median(dev) * 1e-3) / 1e9,
                   "inertia": model.inertia_}
            if not a.no_gmm:
                try:
                    g = []
                    for rep in range(a.reps + 1):
                        mix = pcp.GMM(k, max_iter=a.iters, tol=-np.inf).fit(dc, means_init=c0)
                        if rep:
                            g.append(mix.device_ms_)
                    run["gmm_em_iteration_device_ms_median"] = float(np.median(g)) / mix.n_iter_
                    run["gmm_iterations_run"] = mix.n_iter_
                except np.linalg.LinAlgError as e:
                    run["gmm_em_iteration_device_ms_median"] = None
                    run["gmm_note"] = str(e)
            if not a.no_host:
                run["host_numpy_iteration_ms"], run["host_points_timed"] = host_iteration_ms(data, c0)
            dc.free()
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
