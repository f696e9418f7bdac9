"""bench.py's batch256 tight leg (256 x 20 000-point pairs, thresholds 1e-3, at most 30 iterations) run repeatedly through the per-pair
path (PCR_BATCH_PER_PAIR=1) and the fused batch, on 8 contexts and on 1: pairs whose T or iteration count differ from the FIRST
per-pair run on 8 contexts, as (pair, iters, iters, n_assoc, n_assoc, max |dT|).  Says which path varies from run to run when
bench.py's results_bitwise_equal_to_fused is false.  A/B: PCR_LIB_PATH.  Recorded: profiles/grid_build_tight_leg_bits.txt"""
import importlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("point-cloud-process_amd")
batch = importlib.import_module("point-cloud-process_amd.batch")
pairs = [(s, t, None) for s, t, _ in pkg.synthetic.registration_batch_6f(256, 20000, seed=1000)]
kw = dict(mode="total", max_iter=30, r_thres=1e-3, t_thres=1e-3)
def run(per_pair, streams):
    if per_pair: os.environ["PCR_BATCH_PER_PAIR"] = "1"
    try:
        return batch.register_batch(pairs, device=0, streams=streams, **kw)
    finally:
        os.environ.pop("PCR_BATCH_PER_PAIR", None)
def diff(a, b):
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        if not (np.array_equal(x["T"], y["T"]) and x["iters"] == y["iters"]):
            out.append((i, x["iters"], y["iters"], x["n_assoc"], y["n_assoc"], float(np.abs(x["T"] - y["T"]).max())))
    return out
ref = run(True, 8)
print("lib", os.path.basename(os.environ.get("PCR_LIB_PATH", "in-tree")), flush=True)
for tag, pp, st, reps in (("per-pair x8ctx", True, 8, 4), ("per-pair x1ctx", True, 1, 2), ("fused x8ctx", False, 8, 10), ("fused x1ctx", False, 1, 3), ("fused x8ctx", False, 8, 6)):
    for r in range(reps):
        d = diff(ref, run(pp, st))
        print(tag, r, "pairs differing from the first per-pair run:", len(d), d[:4], flush=True)
