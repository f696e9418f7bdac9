"""What the queue items of a seeded ICP pass are, on the 120 000-point bench pair (two-launch variant, so that every counter is of
the LAST pass of the call; diagnostic build: scripts/build_variant.sh diag "-DPCR_WT_DIAG -DPCR_PASS_DIAG=1",
PCR_LIB_PATH=scripts/bin/libpcr_diag.so): items, why the tiles left them open (as scripts/why_open.py), how many carry a candidate
(a seeded query's real point and ball) and the descent's cycles and start level for both kinds, blocks with open queries; then the
items of every pass of one 30-pass call.  PCR_PASS_GATE_LB=0 for the pass without carried gate bounds.  Recorded:
profiles/gate_bounds_pass.txt"""
import ctypes as C, importlib, os, sys
import numpy as np
os.environ["PCR_DEBUG_STAMPS"] = "1"
os.environ["PCR_PASS_INLINE"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pcp = importlib.import_module("point-cloud-process_amd")
L = pcp._lib
src, tgt, _ = pcp.synthetic.perturbed_pair(120000, seed=0)
ctx = pcp.default_context()
index = pcp.TargetIndex(tgt)
for it in (2, 5, 20):
    sd = pcp.DeviceCloud.upload(src).prepare(index)
    r = pcp.icp_device(sd, index, np.eye(4), mode="total", max_iter=it, r_thres=-1, t_thres=-1, min_iter=it)
    buf = np.zeros(1 << 19, dtype=np.uint64)
    L.check(L.lib().pcr_debug_read(ctx.handle, buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size))
    why = buf[(1 << 15):(1 << 15) + 5].astype(np.int64)
    total = int(buf[(1 << 19) - 8])
    hb = buf[(1 << 17):(1 << 17) + 4 * min(total, 60000)].reshape(-1, 4).astype(np.int64)
    cand = hb[:, 3] & 1
    lvl = (hb[:, 3] >> 8) - 1
    cyc = hb[:, 0].astype(float)
    nb = (120000 + 127) // 128
    blk = buf[:nb * 4].reshape(nb, 4).astype(np.int64)
    print(os.environ.get("TAG"), "pass", it, "items", total, "open by reason [clamped/none, level, too many points, ambiguous, ball out of box]", why.tolist())
    print("   with a candidate", int(cand.sum()), "without", int((1 - cand).sum()),
          "| descent cycles pct 50/90/max: with", np.percentile(cyc[cand == 1], [50, 90, 100]).round(0).tolist() if cand.any() else None,
          "without", np.percentile(cyc[cand == 0], [50, 90, 100]).round(0).tolist() if (cand == 0).any() else None)
    print("   start level of the descent (with candidate):", np.bincount(lvl[cand == 1] + 1).tolist() if cand.any() else None, "(without):", np.bincount(lvl[cand == 0] + 1).tolist() if (cand == 0).any() else None)
    print("   blocks (4 tiles) with open queries", int((blk[:, 3] > 0).sum()), "of", nb, "| open per such block pct 50/90/max", np.percentile(blk[blk[:, 3] > 0, 3], [50, 90, 100]).tolist())
    sd.free()
sd = pcp.DeviceCloud.upload(src).prepare(index)
r = pcp.icp_device(sd, index, np.eye(4), mode="total", max_iter=30, r_thres=-1, t_thres=-1, min_iter=30)
print("items per pass", ctx.pass_log()["items"])
sd.free()
