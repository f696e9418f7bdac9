"""The mechanism of the query curve, free of timing noise, on the 120 000-point bench pair: candidates per query that the tile kernel's
filter evaluates (its own counters, as bench.py --full reports them under roofline_valu), the queue items of every pass of one 30-pass
call (ctx.pass_log()), and what upload + lay-out cost, for PCR_QUERY_CURVE=morton and for the default curve.  With PCR_LIB_PATH set to
a build from before the curve both columns are that build's Morton lay-out.  Recorded: profiles/query_curve_pass.txt"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
pcp = importlib.import_module("point-cloud-process_amd")
N = int(os.environ.get("N", 120000))
src, tgt, _ = pcp.synthetic.perturbed_pair(N, seed=0)
ctx = pcp.default_context()
index = pcp.TargetIndex(tgt)
for curve in ("morton", None):
    os.environ.pop("PCR_QUERY_CURVE", None) if curve is None else os.environ.__setitem__("PCR_QUERY_CURVE", curve)
    pairs, mean_c = bench.filter_pairs_per_pass(pcp, 0, src, tgt, 0.0)
    setup = []
    for _ in range(7):
        ctx.sync()
        t0 = time.perf_counter()
        sd = pcp.DeviceCloud.upload(src).prepare(index)
        ctx.sync()
        setup.append(1e3 * (time.perf_counter() - t0))
        sd.free()
    sd = pcp.DeviceCloud.upload(src).prepare(index)
    os.environ["PCR_PASS_INLINE"] = "0"     # the two-launch variant of the pass logs its items
    r = pcp.icp_device(sd, index, np.eye(4), mode="total", max_iter=30, r_thres=-1, t_thres=-1, min_iter=30)
    del os.environ["PCR_PASS_INLINE"]
    items = ctx.pass_log()["items"]
    sd.free()
    print("%-8s lib %s | candidates per query %.1f | items: pass 1 %d, seeded passes mean %.0f (min %d, max %d) | upload + lay-out ms median %.3f min %.3f | n_assoc %d" % (
        curve or "default", os.path.basename(os.environ.get("PCR_LIB_PATH", "in-tree")), mean_c, items[0], np.mean(items[1:]), min(items[1:]), max(items[1:]),
        np.median(setup), min(setup), r["n_assoc"]))
    print("         items per pass", items)
