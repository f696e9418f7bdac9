"""Per-wave timeline of the one-kernel ICP pass (PCR_DEBUG_STAMPS=1): when a wave's tile ended, when its moments were in,
when it left the work queue, how many items it served, polls and lost compare-and-swaps; 100-MHz real-time stamps.
Needs scripts/build_variant.sh pdiag "-DPCR_PASS_DIAG=1" and PCR_LIB_PATH=scripts/bin/libpcr_pdiag.so: the product build compiles the stamps out."""
import ctypes as C, importlib, os, sys
import numpy as np
os.environ["PCR_DEBUG_STAMPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pcp = importlib.import_module("point-cloud-process_amd")
L = pcp._lib
N = int(os.environ.get("N", 120000))
src, tgt, Tt = pcp.synthetic.perturbed_pair(N, seed=0)
ctx = pcp.default_context()
index = pcp.TargetIndex(tgt, kind="grid", cell=float(os.environ.get("CELL", 0)))
sd = pcp.DeviceCloud.upload(src).prepare(index)
it = int(os.environ.get("ITERS", 4))
r = pcp.icp_device(sd, index, np.eye(4), mode="total", max_iter=it, r_thres=-1, t_thres=-1, min_iter=it)
nw = (N + 127) // 128 * 4
buf = np.zeros((1 << 19) + nw * 8, dtype=np.uint64)
L.check(L.lib().pcr_debug_read(ctx.handle, buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size))
w = buf[(1 << 19):].reshape(nw, 8).astype(np.int64)
t0 = w[:, 0].min()
us = lambda c: (c - t0) / 100.0
pc = lambda v: np.percentile(v, [50, 90, 99, 100]).round(1)
print("waves", nw, "(last pass of", it, ")")
print("start      us pct 50/90/99/max", pc(us(w[:, 0])))
print("tile end   us", pc(us(w[:, 1])), " tile duration", pc((w[:, 1] - w[:, 0]) / 100.0))
print("moments in us", pc(us(w[:, 2])), " duration", pc((w[:, 2] - w[:, 1]) / 100.0))
print("queue exit us", pc(us(w[:, 3])), " duration", pc((w[:, 3] - w[:, 2]) / 100.0))
print("ticket     us", pc(us(w[:, 7])), " duration", pc((w[:, 7] - w[:, 3]) / 100.0))
print("finishing wave: first sum in %.2f, sums exchanged %.2f, Procrustes done %.2f, state written %.2f us" % tuple((int(buf[(1 << 19) - k]) - t0) / 100.0 for k in (4, 3, 2, 1)))
print("items total", w[:, 4].sum(), "per wave max", w[:, 4].max(), "waves with items", (w[:, 4] > 0).sum())
print("polls total", (w[:, 5] & 0xffffffff).sum(), "max", (w[:, 5] & 0xffffffff).max(), " lost CAS total", (w[:, 5] >> 32).sum())
pairs = w[:, 6] & ((1 << 40) - 1); passes = (w[:, 6] >> 40) & 0xff; unres = (w[:, 6] >> 48)
dur = (w[:, 1] - w[:, 0]) / 100.0
print("tile duration by passes:", {int(k): (int((passes == k).sum()), round(float(np.median(dur[passes == k])), 1), round(float(dur[passes == k].max()), 1)) for k in np.unique(passes)})
staged = pairs / 32.0
for lo, hi in [(0, 193), (193, 385), (385, 577), (577, 769), (769, 1e9)]:
    m = (staged >= lo) & (staged < hi)
    if m.any():
        print("  staged points (sum over passes) in [%d, %d): %5d waves, duration median %.1f p90 %.1f max %.1f, unresolved mean %.1f" % (lo, min(hi, 99999), m.sum(), np.median(dur[m]), np.percentile(dur[m], 90), dur[m].max(), unres[m].mean()))
o = np.argsort(-dur)[:12]
print("slowest tiles (us, passes, staged, unresolved):", [(round(float(dur[i]), 1), int(passes[i]), int(staged[i]), int(unres[i])) for i in o])
hb = buf[(1 << 17):(1 << 17) + 240000].reshape(-1, 4)
hb = hb[hb[:, 0] > 0]
if len(hb):
    print("hard items", len(hb), "cycles pct", pc(hb[:, 0].astype(float)), " start offset (wave clock / 16) pct", pc((hb[:, 1] & np.uint64(0xffffffff)).astype(float)))
nb = (N + 127) // 128
ph = buf[(1 << 16):(1 << 16) + nb * 8].reshape(nb, 8).astype(np.float64)
if ph.sum() > 0:   # -DPCR_WT_DIAG build: phase cycles of wave 0 of every block (shader clock)
    names = ["load+xform", "cube+level", "directory", "prefix", "staging", "filter", "merge+verify", "-"]
    print("wave-0 tile phases, cycles (sum over passes/rounds): median / p90 / max")
    for i, nm in enumerate(names[:7]):
        print("   %-14s %8.0f %8.0f %8.0f" % (nm, np.median(ph[:, i]), np.percentile(ph[:, i], 90), ph[:, i].max()))
    print("   total median %.0f" % np.median(ph.sum(axis=1)))
    tot = ph.sum(axis=1)
    heavy = tot >= np.percentile(tot, 97)
    print("the heaviest 3 %% of these waves (%d): mean cycles per phase" % heavy.sum(), {nm: int(ph[heavy, i].mean()) for i, nm in enumerate(names[:7])}, "total", int(tot[heavy].mean()))
# per queue group (wave id after the XCD remap, mod 32): items served and when the group's last wave left
nblk = nw // 4
per = nblk >> 3; main = per << 3
raw = np.arange(nw)
blk = raw // 4
blk2 = np.where(blk < main, (blk & 7) * per + (blk >> 3), blk)
wid = blk2 * 4 + (raw & 3)
grp = wid % 32
it_g = np.bincount(grp, weights=w[:, 4], minlength=32)
ex_g = np.array([us(w[grp == g, 3]).max() for g in range(32)])
last_tile_g = np.array([us(w[grp == g, 1]).max() for g in range(32)])
print("items per group min/median/max", int(it_g.min()), int(np.median(it_g)), int(it_g.max()), "| group's last queue exit us min/median/max %.1f %.1f %.1f" % (ex_g.min(), np.median(ex_g), ex_g.max()),
      "| last tile end per group min/max %.1f %.1f" % (last_tile_g.min(), last_tile_g.max()))
busy = w[:, 4] > 0
print("waves that served items: exit us pct 50/90/99/max", pc(us(w[busy, 3])), " idle ones:", pc(us(w[~busy, 3])))
# ---- when the last contribution to the accumulators LANDED (where a finish by the last lander starts), from the stamps above.
# Tiles: "moments in" is taken behind the reply of the done-add, which was issued in front of the 19 moment atomics: their
# acknowledgement follows within one round trip.  Items: pass_serve_item stamps its start (shader clock / 16, from the serving wave's
# start) and its duration in its slot, group + 32 * index; a group's slots of THIS pass are the first `items served by the group`
# ones (the block is not zeroed per pass).  The shader clock is calibrated against the real-time stamps of the tiles (per block:
# longest start -> moments-in span in both clocks); the serving wave is not recorded, so its start is taken as the median one.
RT_US = 1.4   # one returning atomic inside the launch (scripts/atomic_rt.hip: 0.7 us unloaded, about 1.4 loaded)
blk_cyc = buf[:nblk * 4].reshape(nblk, 4)[:, 0].astype(np.float64)
blk_rt = (w[:, 2] - w[:, 0]).reshape(nblk, 4).max(axis=1).astype(np.float64)
ok = (blk_cyc > 0) & (blk_rt > 0)
cyc_per_us = float(np.median(blk_cyc[ok] / blk_rt[ok])) * 100.0 if ok.any() else 0.0
item_end = []
rows = []   # items of THIS pass: start, duration (us on the serving wave's clock), with candidate, descent steps, points scanned
full = buf[(1 << 17):(1 << 17) + 240000].reshape(-1, 4)
for g in range(32):
    for k in range(int(it_g[g])):
        e = full[g + 32 * k]
        if g + 32 * k < 59999 and e[0] > 0 and cyc_per_us > 0:
            item_end.append((float(int(e[1]) & 0xffffffff) * 16.0 + float(e[0])) / cyc_per_us)
            rows.append((float(int(e[1]) & 0xffffffff) * 16.0 / cyc_per_us, float(e[0]) / cyc_per_us, int(e[3]) & 1, int(e[1]) >> 32, int(e[2]) & 0xffffffff))
if rows:
    # ("hard items" above counts every record in the block, the unseeded first pass's included: these are the last pass's alone)
    rw = np.array(rows)
    print("items of this pass by start (us after the serving wave's start): count, with a candidate, duration median / max, points scanned median, last end")
    for lo, hi in [(0, 8), (8, 12), (12, 15), (15, 18), (18, 99)]:
        m = (rw[:, 0] >= lo) & (rw[:, 0] < hi)
        if m.any():
            print("   %2d-%2d: %5d items, %5d with a candidate, duration %.2f / %.2f us, points %d, last end %.2f" % (lo, hi, m.sum(), rw[m, 2].sum(), np.median(rw[m, 1]), rw[m, 1].max(), np.median(rw[m, 4]), (rw[m, 0] + rw[m, 1]).max()))
    for c, nm in ((1, "with a candidate"), (0, "without one")):
        m = rw[:, 2] == c
        if m.any():
            print("   %-17s %5d items, duration pct 50/90/99/max" % (nm, m.sum()), pc(rw[m, 1]).round(2), "us, descent steps median %d, points median %d" % (np.median(rw[m, 3]), np.median(rw[m, 4])))
    o = np.argsort(-(rw[:, 0] + rw[:, 1]))[:8]
    print("   the last to end (start, duration, candidate, steps, points):", [(round(float(rw[i, 0]), 1), round(float(rw[i, 1]), 1), int(rw[i, 2]), int(rw[i, 3]), int(rw[i, 4])) for i in o])
start_med = float(np.median(us(w[:, 0])))
# (the wave that writes the poison takes its "moments in" stamp behind those stores: a tile's span is capped at the 99th percentile)
span = w[:, 2] - w[:, 1]
last_tile_in = float(us(w[:, 1] + np.minimum(span, int(np.percentile(span, 99)))).max())
last_item_in = start_med + max(item_end) if item_end else 0.0
first_sum = (int(buf[(1 << 19) - 4]) - t0) / 100.0
print("shader clock %.0f cycles per us | last tile's moments issued %.2f us, last item's %.2f us (%d items stamped) -> last contribution acknowledged about %.2f us (+ one round trip of %.1f us); the finishing wave's first sum in %.2f us"
      % (cyc_per_us, last_tile_in, last_item_in, len(item_end), max(last_tile_in, last_item_in) + RT_US, RT_US, first_sum))
# ---- who finished (a library with the landed counts, PCR_PASS_DIAG build; zeros with an older one)
kind = int(buf[(1 << 19) - 6])
if kind:
    names = {1: "the last lander, a tile wave", 2: "the last lander, an item server", 3: "the last leaver (fall-back)"}
    print("finished by %s: chosen at %.2f us, first sum in %.2f, Procrustes done %.2f, state written %.2f us; last exit (ticket) %.2f us"
          % (names.get(kind, "?"), (int(buf[(1 << 19) - 5]) - t0) / 100.0, first_sum, (int(buf[(1 << 19) - 2]) - t0) / 100.0, (int(buf[(1 << 19) - 1]) - t0) / 100.0, float(us(w[:, 7]).max())))
else:
    print("finished by the last leaver (no landed counts in this library); last exit (ticket) %.2f us" % float(us(w[:, 7]).max()))
print("passes finished by the last lander %d, by the last leaver %d, passes with a give-up %d (whole process)" % (int(buf[(1 << 19) - 15]), int(buf[(1 << 19) - 14]), int(buf[(1 << 19) - 16])))
