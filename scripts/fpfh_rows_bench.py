"""FPFH at chosen rows against the full pass, on the GPU box -> profiles/fpfh_rows_bench.json.

The 120 000-point synthetic scan, down-sampled and described the way preprocess_point_cloud does it at voxel 0.5 and at 2.0 (normals
2 voxels / 30 neighbours, FPFH 5 voxels / 100 neighbours), and the scan itself with the voxel-0.5 radii.  Keypoints: the rows
keypointHarris3D(is_nms=True) keeps (radius 2.5 voxels, as ransac_init), the first 400 of them, and seeded random rows at growing m up
to the whole cloud -- the rows pass computes the lists of its rows twice (once for the list, once for the SPFH) and must lose where
m * max_nn approaches n; the sweep shows where.  Both passes go through their host entry points on a resident DeviceCloud (normals
in, descriptors out), timed by the host clock around calls that end in a stream synchronise, after a warm-up, alternating.

--parent-lib PATH: a libpcr.so built from the parent commit.  The full pass alone is then timed in fresh processes that alternate
between this tree's library and that one (--runs of each), and both medians with the spread of the per-run medians are recorded:
the full pass shares spfh_body / fpfh_body with the rows pass and must not have become slower."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_NN = 100
VOXELS = (0.5, 2.0)
RAW = "scan_at_full_resolution_voxel_0.5_radii"


def scan():
    import pcp_amd as pcp

    return pcp.synthetic.kitti_like_scan(120_000, seed=4).astype(np.float64)


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def full_only(reps):
    """Child process: median ms of compute_fpfh_feature on the voxel-0.5 and the voxel-2.0 down-sample and on the scan itself (the
    configurations of main()), one JSON line."""
    import torch  # noqa: F401  (one HIP runtime per process, before the library is looked at)
    import ctypes

    from importlib import import_module

    L = import_module("point-cloud-process_amd._lib")
    if not hasattr(ctypes.CDLL(L.LIB_PATH), "pcr_fpfh_rows"):
        L.SIGNATURES.pop("pcr_fpfh_rows")               # the parent's library
    import pcp_amd as pcp

    ctx = pcp.default_context()
    pts, res = scan(), {"lib": L.LIB_PATH}
    for name, voxel in [(str(v), v) for v in VOXELS] + [(RAW, 0.5)]:
        down = pts if name == RAW else pcp.voxel_down_sample(pts, voxel, ctx=ctx)
        nrm = pcp.estimate_normals_hybrid(down, 2 * voxel, 30, ctx=ctx)
        cloud = pcp.DeviceCloud.upload(down, ctx)
        call = lambda: pcp.compute_fpfh_feature(cloud, nrm, 5 * voxel, MAX_NN, ctx=ctx)  # noqa: E731
        for _ in range(3):
            call()
        ms = [timed(call) for _ in range(reps)]
        res[name] = {"n": len(down), "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "digest": float(np.abs(call().data).sum())}
        cloud.free()
    print(json.dumps(res), flush=True)


def scratch_full(n):
    return n * (12 * MAX_NN + 268)


def scratch_rows(n, m, table):
    bound = min(n, m * (MAX_NN + 1))
    return 12 * m * MAX_NN + 4 * m + (8 if table else 4) * n + 268 * bound


def config(pcp, ctx, name, pts, voxel, reps, out):
    radius = 5 * voxel
    n = len(pts)
    nrm = pcp.estimate_normals_hybrid(pts, 2 * voxel, 30, ctx=ctx)
    cloud = pcp.DeviceCloud.upload(pts, ctx)
    kp = np.asarray(pcp.keypointHarris3D(cloud, radius=2.5 * voxel, nms_threshold=0.001, is_nms=True, return_indices=True, ctx=ctx)[1], dtype=np.int64)
    rng = np.random.default_rng(12)
    sets = {"harris": kp, "harris_first_400": kp[:400]}
    for m in (100, 400, 1600, 6400, 25600):
        if m < n:
            sets[f"random_{m}"] = rng.choice(n, m, replace=False)
    sets["every_row"] = np.arange(n)
    full_call = lambda: pcp.compute_fpfh_feature(cloud, nrm, radius, MAX_NN, ctx=ctx)  # noqa: E731
    full = full_call().data
    table = n > 4096                                     # HYBRID_BRUTE_MAX: above it the search goes through a grid index
    res = {"n": n, "voxel": voxel, "fpfh_radius": radius, "max_nn": MAX_NN, "harris_keypoints": len(kp), "scratch_bytes_full": scratch_full(n), "rows": {}}
    for tag, rows in sets.items():
        if len(rows) == 0:
            continue
        rows_call = lambda: pcp.compute_fpfh_at_rows(cloud, rows, nrm, radius, MAX_NN, ctx=ctx, return_info=True)  # noqa: E731
        f, info = rows_call()
        assert np.array_equal(f.data, full[:, rows]), tag               # faster and different is not faster
        full_call()
        t_full, t_rows = [], []
        for _ in range(reps):                                           # alternating
            t_full.append(timed(full_call))
            t_rows.append(timed(rows_call))
        r = {"m": len(rows), "m_max_nn_over_n": len(rows) * MAX_NN / n, "n_spfh": info["n_spfh"], "n_spfh_over_n": info["n_spfh"] / n,
             "full_ms_median": float(np.median(t_full)), "full_ms_min": float(min(t_full)), "full_ms_max": float(max(t_full)),
             "rows_ms_median": float(np.median(t_rows)), "rows_ms_min": float(min(t_rows)), "rows_ms_max": float(max(t_rows)),
             "scratch_bytes_rows": scratch_rows(n, len(rows), table)}
        r["rows_over_full"] = r["rows_ms_median"] / r["full_ms_median"]
        r["rows_pass_loses"] = bool(r["rows_over_full"] > 1.0)
        res["rows"][tag] = r
        print(name, tag, json.dumps(r), flush=True)
    cloud.free()
    out[name] = res


def against_parent(parent_lib, runs, reps):
    here = {"new": None, "parent": parent_lib}
    got = {"new": [], "parent": []}
    for run in range(runs):
        for which in (("new", "parent") if run % 2 == 0 else ("parent", "new")):
            env = dict(os.environ)
            env.pop("PCR_LIB_PATH", None)
            if here[which]:
                env["PCR_LIB_PATH"] = os.path.abspath(here[which])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--full-only", "--reps", str(reps)], env=env, capture_output=True,
                               text=True, timeout=600, check=True)
            got[which].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("full pass", which, got[which][-1], flush=True)
    out = []
    for voxel in [str(v) for v in VOXELS] + [RAW]:
        res = {"config": voxel if voxel == RAW else "voxel_" + voxel, "n": got["new"][0][voxel]["n"], "runs_each": runs, "calls_per_run": reps}
        assert len({g[voxel]["digest"] for g in got["new"] + got["parent"]}) == 1   # the same descriptors from both libraries
        for which, g in got.items():
            med = [x[voxel]["median_ms"] for x in g]
            res[which] = {"run_medians_ms": med, "median_ms": float(np.median(med)), "spread_ms": float(max(med) - min(med))}
        res["new_minus_parent_ms"] = res["new"]["median_ms"] - res["parent"]["median_ms"]
        res["within_spread"] = bool(res["new_minus_parent_ms"] <= max(res["new"]["spread_ms"], res["parent"]["spread_ms"]))
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--full-only", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-raw", action="store_true", help="skip the scan at full resolution")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_rows_bench.json"))
    a = ap.parse_args()
    if a.full_only:
        return full_only(a.reps)
    import pcp_amd as pcp

    ctx = pcp.default_context()
    pts = scan()
    out = {"device": ctx.device_info().get("name", ""), "timing": "host clock around host-in / host-out calls that end in a stream synchronise; ms; "
           f"{a.reps} alternating calls of each pass after warm-up", "configs": {}}
    for voxel in VOXELS:
        config(pcp, ctx, f"voxel_{voxel}", pcp.voxel_down_sample(pts, voxel, ctx=ctx), voxel, a.reps, out["configs"])
    if not a.no_raw:
        config(pcp, ctx, RAW, pts, 0.5, max(3, a.reps // 5), out["configs"])
    if a.parent_lib:
        out["full_pass_against_parent"] = against_parent(a.parent_lib, a.runs, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
