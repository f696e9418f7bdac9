"""The fixed-order PointNet++ gradients (include/pcr.h: pcr_pn2_inverse_index, pcr_pn2_*_grad) beside the composed scatter_add_ path
they can replace, on the same device, the same tensors, warm:

  ops     the groupings of the reference's two classifiers (pointnet2_ssg_cls.py, pointnet2_msg_cls.py) at both levels with centres,
          at B = 8 x 64 points (the reference's training batch: KITTI objects resampled to 64 points) and at B = 8 x 1024 points, the
          gather of the centres, and one feature-propagation interpolation.  Per shape: the inverse-index build alone, the ordered sum
          alone (index already built), both together, and torch's scatter_add_ composition; the bytes the sum kernel moves (every
          point tile stages the cloud's terms, every channel tile walks the slot lists) against the algorithmic minimum (terms and
          idx read once, the output written once).
  steps   one training step (forward, backward, Adam) of both classifiers at both batch shapes with the switch on and off, the two
          alternating.
  fit     how many epochs of pointnet2_train.train_and_eval the SSG classifier needs on the synthetic two-shape set
          (tests/pointnet2_grad_checks.py: write_shapes_dataset, seed 0, batch 8) until every training batch of an epoch is classified correctly,
          with the switch off (torch's path) and on.  tests/test_gpu_pointnet2_train.py trains for twice the first number.

Times are HIP events around `reps` back-to-back calls on the current stream after warm-up calls of the same shape, the median of
`rounds` such windows.  Writes profiles/pointnet2_grad_bench.json.

    python scripts/pointnet2_grad_bench.py [--rounds 5] [--skip-fit] [--out profiles/pointnet2_grad_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pn2 = importlib.import_module("point-cloud-process_amd.pointnet2_ops")
from tests.pointnet2_grad_checks import write_shapes_dataset  # noqa: E402
u = pn2.pointnet2_utils

GRAD_CT, GRAD_POINTS = 8, 256     # pcr_pointnet2_grad.hip: channels and points per workgroup


def window_us(fn, reps, warmup, rounds):
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
    return float(np.median(out))


def cloud(rng, B, N):
    """Points on a sphere of radius 0.5 with a little noise: an object's surface, as the classifier sees it."""
    p = rng.normal(size=(B, N, 3))
    p *= 0.5 / np.linalg.norm(p, axis=2, keepdims=True)
    return torch.from_numpy((p + rng.normal(scale=0.01, size=p.shape)).astype(np.float32)).cuda()


def time_op(name, grad, idx, n, rounds, weight=None):
    """grad / idx / weight as scatter_rows_ordered takes them."""
    B, C = grad.shape[:2]
    K = int(np.prod(idx.shape[1:]))

    def build():
        if hasattr(idx, "_pcr_inverse_index"):
            del idx._pcr_inverse_index
        u.inverse_index(idx, n)

    def composed():
        if weight is None:
            return u._scatter_rows(grad.reshape(B, C, -1), idx.reshape(B, -1), n)
        return u._scatter_rows((grad.unsqueeze(-1) * weight.unsqueeze(1)).reshape(B, C, K), idx.reshape(B, K), n)

    def both():
        build()
        u.scatter_rows_ordered(grad, idx, n, weight=weight)

    ordered = u.scatter_rows_ordered(grad, idx, n, weight=weight)
    old = composed()
    scale = old.abs().max().clamp_min(1e-30)
    build_us = window_us(build, 50, 5, rounds)
    u.inverse_index(idx, n)
    sum_us = window_us(lambda: u.scatter_rows_ordered(grad, idx, n, weight=weight), 50, 5, rounds)
    both_us = window_us(both, 50, 5, rounds)
    composed_us = window_us(composed, 50, 5, rounds)
    point_tiles, channel_tiles = -(-n // GRAD_POINTS), -(-C // GRAD_CT)
    term_bytes = 4 * B * C * grad[0, 0].numel() + (4 * B * K if weight is not None else 0)
    minimum = term_bytes + 4 * B * K + 4 * B * C * n
    moved = point_tiles * (4 * B * C * K + (4 * B * K if weight is not None else 0)) + channel_tiles * 4 * B * (K + n + 1) + 4 * B * C * n
    run = {"op": name, "B": B, "C": C, "n": n, "slots_per_cloud": K, "slots_per_point": K / n, "inverse_index_us": build_us, "ordered_sum_us": sum_us,
           "index_and_sum_us": both_us, "scatter_add_us": composed_us, "scatter_add_over_index_and_sum": composed_us / both_us,
           "sum_bytes_moved": moved, "bytes_minimum": minimum, "sum_GBps_of_moved": moved / sum_us * 1e-3,
           "max_abs_difference_over_max_abs": float((ordered - old).abs().max() / scale),
           "two_ordered_runs_equal": bool(torch.equal(ordered, u.scatter_rows_ordered(grad, idx, n, weight=weight)))}
    print(json.dumps(run), flush=True)
    return run


def ops(rounds):
    rng = np.random.default_rng(0)
    runs = []
    msg = {1: ((0.1, 16), (0.2, 32), (0.4, 128)), 2: ((0.2, 32), (0.4, 64), (0.8, 128))}
    ssg = {1: ((0.2, 64),), 2: ((0.4, 64),)}
    for N in (64, 1024):
        xyz = cloud(rng, 8, N)
        level_xyz, npoints, feat_c = {1: xyz}, {1: 512, 2: 128}, {1: (3,), 2: (128, 320)}
        picks = u.furthest_point_sample(xyz, 512)
        level_xyz[2] = u.gather_operation(xyz.transpose(1, 2).contiguous(), picks).transpose(1, 2).contiguous()
        runs.append(time_op(f"gather 8x{N} centres", torch.randn((8, 3, 512), device="cuda"), picks, N, rounds))
        for level in (1, 2):
            pts = level_xyz[level]
            n = pts.shape[1]
            centres = u.gather_operation(pts.transpose(1, 2).contiguous(), u.furthest_point_sample(pts, npoints[level])).transpose(1, 2).contiguous()
            for radius, nsample in sorted(set(msg[level] + ssg[level])):
                idx = u.ball_query(radius, nsample, pts, centres)
                for C in feat_c[level]:
                    grad = torch.randn((8, C, npoints[level], nsample), device="cuda")
                    runs.append(time_op(f"group 8x{N} level {level} r={radius} nsample={nsample}", grad, idx, n, rounds))
    unknown, known = cloud(rng, 8, 1024), cloud(rng, 8, 256)
    dist, idx = u.three_nn(unknown, known)
    recip = 1.0 / (dist + 1e-8)
    weight = (recip / recip.sum(dim=2, keepdim=True)).contiguous()
    runs.append(time_op("three_interpolate 8x1024 from 256", torch.randn((8, 256, 1024), device="cuda"), idx, 256, rounds, weight=weight))
    return runs


def steps(rounds):
    rng = np.random.default_rng(1)
    runs = []
    for name in ("PointNet2ClassificationSSG", "PointNet2ClassificationMSG"):
        for N in (64, 1024):
            torch.manual_seed(0)
            model = getattr(pn2, name)(num_classes=4, input_channels=3).cuda().train()
            optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
            normals = rng.normal(size=(8, N, 3)).astype(np.float32)
            batch = torch.cat([cloud(rng, 8, N), torch.from_numpy(normals).cuda()], dim=2)
            labels = torch.from_numpy(rng.integers(0, 4, size=8)).cuda()

            def step(fixed):
                optimizer.zero_grad()
                with u.fixed_order_gradients(fixed):
                    loss = torch.nn.functional.cross_entropy(model(batch), labels)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
                optimizer.step()

            times = {True: [], False: []}
            for fixed in (True, False):
                window_us(lambda: step(fixed), 2, 2, 1)
            for _ in range(rounds):
                for fixed in (True, False):
                    times[fixed].append(window_us(lambda: step(fixed), 5, 0, 1))
            run = {"model": name, "B": 8, "N": N, "step_ms_fixed_order": float(np.median(times[True])) * 1e-3,
                   "step_ms_scatter_add": float(np.median(times[False])) * 1e-3}
            run["scatter_add_over_fixed_order"] = run["step_ms_scatter_add"] / run["step_ms_fixed_order"]
            print(json.dumps(run), flush=True)
            runs.append(run)
    return runs


class Scalars:
    """What train_one_epoch reports, kept by name."""

    def __init__(self):
        self.seen = {}

    def add_scalar(self, name, value, step):
        self.seen.setdefault(name, []).append(float(value))


def epochs_to_fit(fixed_order, max_epochs=40, seed=0):
    """The first epoch (counted from 1) in which every training batch is classified correctly, or None within max_epochs."""
    train = pn2.pointnet2_train
    with tempfile.TemporaryDirectory() as root:
        write_shapes_dataset(root, seed=seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        config = argparse.Namespace(batch_size=8, workers=0, lr=0.003, weight_decay=0.0, epochs=max_epochs + 1, ckpt_save_interval=10 ** 9, resume="false")
        loaders = pn2.resampled_dataset.KITTIPCDClsDataset_Wrapper(root, config).get_dataloader()
        model = pn2.PointNet2ClassificationSSG(num_classes=2, input_channels=3)
        log = Scalars()
        train.train_and_eval(model, loaders[0], loaders[1], log, root, None, config, fixed_order=fixed_order)
        per_epoch = len(loaders[0])
    acc = np.array(log.seen["train_acc"]).reshape(max_epochs, per_epoch)
    full = np.flatnonzero((acc == 1.0).all(axis=1))
    return (int(full[0]) + 1 if len(full) else None), acc.min(axis=1).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet2_grad_bench.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if not a.skip_fit:
        out["fit"] = {}
        for fixed in (False, True):
            first, worst = epochs_to_fit(fixed)
            out["fit"]["fixed_order" if fixed else "scatter_add"] = {"epochs_until_every_training_batch_is_right": first, "worst_batch_accuracy_per_epoch": worst}
            print(json.dumps(out["fit"]), flush=True)
    out["ops"] = ops(a.rounds)
    out["steps"] = steps(a.rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
