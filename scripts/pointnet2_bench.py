"""PointNet++ ops (include/pcr.h: pcr_pn2_*) through pointnet2_utils, each beside the same op written with torch device ops -- what a
user of this hardware had before, since the reference's kernels are CUDA only:

  furthest point sampling  B in {1, 16, 64} x N in {1024, 4096, 16384, 120000}, m = N / 8 capped at 1024: microseconds per call and per
                           pick.  The torch version is the usual loop (one distance pass, one minimum, one arg-max per pick); it is timed
                           over its first TORCH_PICKS picks and reported per pick.
  ball query               the (radius, nsample) pairs of the reference's multi-scale classifier (pointnet2_msg_cls.py:17-30) at its
                           two levels, B = 16, points in the unit ball, centres by furthest point sampling.  torch: the full distance
                           matrix, indices outside the ball replaced by N, a sort, the first nsample.
  three_nn                 n = 4096 unknown, m = 1024 known, B = 16.  torch: distance matrix + topk(3).

Times are HIP events around `reps` back-to-back calls on the current stream after `warmup` calls of the same shape, the median of
`rounds` such windows.  Writes profiles/pointnet2_bench.json.

    python scripts/pointnet2_bench.py [--rounds 5] [--out profiles/pointnet2_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcp = importlib.import_module("point-cloud-process_amd")
u = pcp.pointnet2_utils

TORCH_PICKS = 64


def window_us(fn, reps, warmup, rounds):
    """median over `rounds` of (HIP-event time of `reps` calls) / reps, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        out.append(1e3 * t0.elapsed_time(t1) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def torch_fps(xyz, m):
    B, N, _ = xyz.shape
    temp = torch.full((B, N), 1e10, device=xyz.device)
    idx = torch.zeros((B, m), dtype=torch.int64, device=xyz.device)
    rows = torch.arange(B, device=xyz.device)
    far = torch.zeros(B, dtype=torch.int64, device=xyz.device)
    for j in range(1, m):
        d = ((xyz - xyz[rows, far].unsqueeze(1)) ** 2).sum(-1)
        temp = torch.minimum(temp, d)
        far = temp.argmax(dim=1)
        idx[:, j] = far
    return idx


def torch_ball_query(radius, nsample, xyz, new_xyz):
    B, N, _ = xyz.shape
    d2 = torch.cdist(new_xyz, xyz) ** 2
    idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat(B, new_xyz.shape[1], 1)
    idx[d2 >= radius * radius] = N
    idx = idx.sort(dim=-1).values[:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, idx.shape[2])
    idx = torch.where(idx == N, first, idx)
    return torch.where(idx == N, torch.zeros_like(idx), idx)


def torch_three_nn(unknown, known):
    d, i = torch.cdist(unknown, known).topk(3, dim=2, largest=False)
    return d, i


def unit_ball(rng, B, N):
    p = rng.normal(size=(B, N, 3))
    p *= (rng.uniform(size=(B, N, 1)) ** (1 / 3)) / np.linalg.norm(p, axis=2, keepdims=True)
    return torch.from_numpy(p.astype(np.float32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet2_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "torch_fps_picks_timed": TORCH_PICKS, "fps": [], "ball_query": [], "three_nn": []}

    for B in (1, 16, 64):
        for N in (1024, 4096, 16384, 120000):
            m = min(N // 8, 1024)
            xyz = torch.from_numpy(rng.normal(size=(B, N, 3)).astype(np.float32)).cuda()
            ours = u.furthest_point_sample(xyz, m)
            same = bool(torch.equal(ours.long()[:, :TORCH_PICKS], torch_fps(xyz, min(m, TORCH_PICKS))))
            reps = max(2, min(50, int(2e5 / (m * max(1.0, N / 4096)))))
            med, lo, hi = window_us(lambda: u.furthest_point_sample(xyz, m), reps, 3, a.rounds)
            tp = min(m, TORCH_PICKS)
            tmed, _, _ = window_us(lambda: torch_fps(xyz, tp), 2, 1, max(3, a.rounds // 2))
            run = {"B": B, "N": N, "m": m, "call_us": med, "call_us_min": lo, "call_us_max": hi, "pick_us": med / m, "torch_pick_us": tmed / (tp - 1),
                   "speedup_per_pick": (tmed / (tp - 1)) / (med / m), "same_first_picks_as_torch_loop": same}
            out["fps"].append(run)
            print(json.dumps(run), flush=True)

    levels = ((1024, 512, ((0.1, 16), (0.2, 32), (0.4, 128))), (512, 128, ((0.2, 32), (0.4, 64), (0.8, 128))))
    for N, npoint, pairs in levels:
        xyz = unit_ball(rng, 16, N)
        centres = u.gather_operation(xyz.transpose(1, 2).contiguous(), u.furthest_point_sample(xyz, npoint)).transpose(1, 2).contiguous()
        for radius, nsample in pairs:
            same = bool(torch.equal(u.ball_query(radius, nsample, xyz, centres).long(), torch_ball_query(radius, nsample, xyz, centres)))
            med, lo, hi = window_us(lambda: u.ball_query(radius, nsample, xyz, centres), 200, 20, a.rounds)
            tmed, _, _ = window_us(lambda: torch_ball_query(radius, nsample, xyz, centres), 20, 3, a.rounds)
            run = {"B": 16, "N": N, "npoint": npoint, "radius": radius, "nsample": nsample, "call_us": med, "call_us_min": lo, "call_us_max": hi,
                   "torch_call_us": tmed, "speedup": tmed / med, "same_as_torch": same}
            out["ball_query"].append(run)
            print(json.dumps(run), flush=True)

    unknown, known = unit_ball(rng, 16, 4096), unit_ball(rng, 16, 1024)
    same = bool(torch.equal(u.three_nn(unknown, known)[1].long(), torch_three_nn(unknown, known)[1]))
    med, lo, hi = window_us(lambda: u.three_nn(unknown, known), 200, 20, a.rounds)
    tmed, _, _ = window_us(lambda: torch_three_nn(unknown, known), 20, 3, a.rounds)
    run = {"B": 16, "n": 4096, "m": 1024, "call_us": med, "call_us_min": lo, "call_us_max": hi, "torch_call_us": tmed, "speedup": tmed / med,
           "same_indices_as_torch": same}
    out["three_nn"].append(run)
    print(json.dumps(run), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
