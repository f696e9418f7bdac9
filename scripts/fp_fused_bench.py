"""Feature propagation for inference: ``fused_forward`` (three_nn, the weights, then one kernel, include/pcr.h: pcr_pn2_fp_mlp) beside
``forward`` (three_nn, three_interpolate, concatenation, 1x1 convolutions, batch norm, ReLU as torch ops) of the SAME module in the
same process, B = 8 clouds of N = 4096 points:

  modules  every decoder module of both segmentation networks on the tensors it sees inside its network (recorded from one unfused
           forward): SSG 4096 <- 1024 <- 256 <- 64 <- 16 points, MSG the same; the two deepest MSG modules are 512 wide, which the
           kernel declines, so their ``fused_forward`` runs forward's torch ops;
  routed   the in-range modules that ``fused_forward`` hands to forward because the kernel was measured slower
           (PointnetFPModule.FUSED_MAX_K0_WIDE), with the route lifted: the kernel beside forward, for the record;
  head     ``fused_head`` (one propagated_mlp call without known points) beside ``fc_lyaer`` on the (B, 128, N) decoder output;
  models   the whole forward of both networks, ``fused=True`` beside ``fused=False``.

Every entry: the neighbour search is part of both paths.  A sample is the HIP-event time of `reps` back-to-back calls divided by
`reps`, after `warmup` calls; the two paths are sampled alternately, `samples` (>= 20) each; reported are the median with the
smallest and the largest sample of its window and the quartiles, the peak-allocation delta (torch.cuda.max_memory_allocated) of
one call of each path, and the largest difference of the two outputs.  Eval mode, no grad, seeded weights and running statistics.
Writes profiles/fp_fused_bench.json.

    python scripts/fp_fused_bench.py [--samples 25] [--out profiles/fp_fused_bench.json]
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
models = pcp.pointnet2_models

B, N = 8, 4096


def window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def window(v):
    q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
    return {"median_ms": med, "min_ms": float(min(v)), "max_ms": float(max(v)), "q1_ms": q1, "q3_ms": q3}


def peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    del out
    return int(delta)


def compare(name, fused, plain, samples, reps, warmup, extra):
    for _ in range(warmup):
        fused()
        plain()
    torch.cuda.synchronize()
    a, b = fused(), plain()
    diff = float((a - b).abs().max())
    scale = float(b.abs().max())
    del a, b
    tf, tp = [], []
    for _ in range(samples):
        tf.append(window_ms(fused, reps))
        tp.append(window_ms(plain, reps))
    run = dict(extra, name=name, samples=samples, reps_per_sample=reps, fused=window(tf), forward=window(tp),
               fused_peak_alloc_bytes=peak_delta(fused), forward_peak_alloc_bytes=peak_delta(plain), max_abs_difference=diff, max_abs_output=scale)
    run["speedup_median"] = run["forward"]["median_ms"] / run["fused"]["median_ms"]
    # the README's box-to-box spread: a fused path more than 10 % slower than forward must not be the default
    run["fused_within_10_percent"] = bool(run["fused"]["median_ms"] <= 1.10 * run["forward"]["median_ms"])
    print(json.dumps(run), flush=True)
    return run


def randomise_bn(module, gen):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)


def unit_ball(rng, n):
    p = rng.normal(size=(B, n, 3))
    p *= (rng.uniform(size=(B, n, 1)) ** (1 / 3)) / np.linalg.norm(p, axis=2, keepdims=True)
    return torch.from_numpy(p.astype(np.float32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp_fused_bench.json"))
    a = ap.parse_args()
    if a.samples < 20:
        ap.error("--samples must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("fp_fused_bench needs a GPU: there is nothing to measure on the host")
    rng = np.random.default_rng(0)
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "N": N, "modules": [], "routed": [], "head": [], "models": []}

    with torch.no_grad():
        ssg, msg = models.PointNet2SemSegSSG(), models.PointNet2SemSegMSG()
        for model in (ssg, msg):
            randomise_bn(model, gen)
            model.cuda().eval()
        pc = torch.cat([unit_ball(rng, N), torch.rand(B, N, 6, generator=gen).cuda()], dim=-1)
        for tag, model in (("ssg", ssg), ("msg", msg)):
            seen = {}
            hooks = [fp.register_forward_hook(lambda mod, args, result, _i=i: seen.__setitem__(_i, args)) for i, fp in enumerate(model.FP_modules)]
            head_in = []
            hooks.append(model.fc_lyaer.register_forward_hook(lambda mod, args, result: head_in.append(args[0])))
            model(pc, fused=False)
            for h in hooks:
                h.remove()
            for i, fp in enumerate(model.FP_modules):
                args = seen[i]
                convs = [c for c in fp.mlp if isinstance(c, torch.nn.Conv2d)]
                spec = [convs[0].in_channels] + [c.out_channels for c in convs]
                n, m = int(args[0].shape[1]), int(args[1].shape[1])
                flop = 2 * B * n * sum(k * w for k, w in zip(spec[:-1], spec[1:]))
                declined = max(spec[1:]) > 256
                out["modules"].append(compare(f"{tag}.FP_modules.{i}", lambda: fp.fused_forward(*args), lambda: fp.forward(*args), a.samples, 10, 5,
                                              {"spec": spec, "n": n, "m": m, "mlp_flop": flop, "kernel_declines": declined}))
                if not declined and not fp._kernel_takes():
                    # in range, but routed to forward because the kernel was measured slower: the kernel itself, for the record
                    fp.FUSED_MAX_K0_WIDE = 1024
                    assert fp._kernel_takes()
                    out["routed"].append(compare(f"{tag}.FP_modules.{i} (kernel)", lambda: fp.fused_forward(*args), lambda: fp.forward(*args), a.samples, 10, 5,
                                                 {"spec": spec, "n": n, "m": m, "mlp_flop": flop}))
                    del fp.FUSED_MAX_K0_WIDE
            x = head_in[0]
            out["head"].append(compare(f"{tag}.fc_lyaer", lambda: model.fused_head(x), lambda: model.fc_lyaer(x), a.samples, 10, 5,
                                       {"spec": [128, 128, model.num_classes], "n": N}))
            out["models"].append(compare(f"{tag} forward", lambda: model(pc, fused=True), lambda: model(pc, fused=False), a.samples, 5, 3, {}))

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
