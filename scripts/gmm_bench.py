"""Gaussian-mixture fit (Cluster_KMeans_GMM/GMM.py:23-63) on a resident cloud: device milliseconds per EM iteration and per fit
(pcr_gmm_result.device_ms, HIP events around the whole loop) and wall milliseconds per fit, for k = 3 and k = 8 at 120 000 and
1 000 000 points; beside each the NumPy log-domain restatement on the host (tests/gmm_checks.fit_log, a few iterations timed) as the CPU
baseline.  The data are k Gaussian blobs at lidar range, the initial means k data rows, max_iter iterations with tol = -inf so that
every run does the same work.  Writes profiles/gmm_bench.json.

    python scripts/gmm_bench.py [--reps 7] [--iters 20] [--host-iters 4] [--no-host] [--out profiles/gmm_bench.json]
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
from tests import gmm_checks  # noqa: E402


def blobs(n, k, seed=0):
    rng = np.random.default_rng(seed)
    centres = np.column_stack([rng.uniform(-60, 60, k), rng.uniform(-60, 60, k), rng.uniform(-2, 2, k)])
    pts = centres[rng.integers(0, k, n)] + rng.normal(size=(n, 3)) * np.array([1.5, 2.0, 0.4])
    return pts, pts[rng.choice(n, k, replace=False)].copy()


def host_iteration_ms(data, means0, iters):
    """tests/gmm_checks.fit_log (NumPy float64, log domain) for a fixed number of iterations -> ms per iteration."""
    t0 = time.perf_counter()
    r = gmm_checks.fit_log(data, means0, max_iter=iters, tol=-np.inf)
    assert r["n_iter"] == iters
    return 1e3 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=4)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_bench.json"))
    a = ap.parse_args()
    ctx = pcp.default_context()
    out = {"device": ctx.device_info(), "iters_per_fit": a.iters, "passes_per_fit": 2 * a.iters + 1, "bytes_per_point_per_pass": 32, "runs": []}
    for n in (120_000, 1_000_000):
        for k in (3, 8):
            data, means0 = blobs(n, k, seed=n + k)
            dc = pcp.DeviceCloud.upload(data, ctx)
            dev, wall, model = [], [], None
            for rep in range(a.reps + 1):     # the first call (arena growth, code load) is not reported
                ctx.sync()
                t0 = time.perf_counter()
                model = pcp.GMM(k, max_iter=a.iters, tol=-np.inf).fit(dc, means_init=means0)
                w = 1e3 * (time.perf_counter() - t0)
                if rep:
                    dev.append(model.device_ms_)
                    wall.append(w)
            assert model.n_iter_ == a.iters
            dev, wall = np.array(dev), np.array(wall)
            run = {"n": n, "k": k, "fit_device_ms_median": float(np.median(dev)), "fit_device_ms_min": float(dev.min()), "fit_device_ms_max": float(dev.max()),
                   "iteration_device_ms_median": float(np.median(dev)) / a.iters, "fit_wall_ms_median": float(np.median(wall)), "reps": a.reps,
                   "GB_per_s_streamed": 32.0 * n * (2 * a.iters + 1) / (np.median(dev) * 1e-3) / 1e9, "nll": model.nll_}
            if not a.no_host:
                run["host_numpy_iteration_ms"] = host_iteration_ms(data, means0, a.host_iters)
                run["host_numpy_fit_ms"] = run["host_numpy_iteration_ms"] * a.iters   # (iterations cost the same: extrapolated)
                run["host_iters_timed"] = a.host_iters
            dc.free()
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
