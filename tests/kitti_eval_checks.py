"""The KITTI evaluation rules of include/pcr.h ("KITTI evaluation") restated in NumPy, for the tests and scripts/kitti_eval_bench.py.

The ground overlap is written differently from the device's: here the FIRST box's quad is the subject, it is cut by the half-planes
``n . p <= d`` of the SECOND box (outward normals, a growing Python list of vertices), and both quads are taken relative to the midpoint
of the two centres; the device clips the second quad by the first one's edges, relative to the first centre, with cross products in
fixed-size arrays.  Cleaning, matching, thresholds and AP are direct loops; the mode-2 matching carries one row of state per threshold,
so a frame costs one pass over its labels.

What arithmetic can tip is reported, not hidden: ``stats["closest"]`` is the smallest |o - MIN_OVERLAP| over the overlaps a matching read,
``stats["gap"]`` the smallest difference between the two largest competing overlaps in mode 2.  Scores, heights, occlusion and truncation
are compared as data."""
import numpy as np

COLUMNS = ["type", "truncated", "occluded", "alpha", "left", "top", "right", "bottom", "height", "width", "length", "cx", "cy", "cz", "ry", "score"]
CLASSES = ["car", "pedestrian", "cyclist"]
METRICS = ["image", "ground", "3d"]
DIFFICULTIES = ["easy", "moderate", "hard"]
MIN_OVERLAP = np.array([[0.7, 0.5, 0.5]] * 3)     # [metric][class]
MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0.0, 1.0, 2.0)
MAX_TRUNCATION = (0.15, 0.30, 0.50)
N_SAMPLES = 41
MAX_DET, MAX_GT = 256, 128


# ------------------------------------------------------------------ overlaps
def _ratio(inter, a, b, criterion):
    return inter / ((a + b) - inter) if criterion < 0 else (inter / a if criterion == 0 else inter / b)


def _quad(l, w, ry, ox, oz):
    c, s = np.cos(ry), np.sin(ry)
    return [(c * x + s * z + ox, -s * x + c * z + oz) for x, z in ((l / 2, w / 2), (-l / 2, w / 2), (-l / 2, -w / 2), (l / 2, -w / 2))]


def _cut(poly, n, d):
    """The part of `poly` with n . p <= d."""
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        sp = n[0] * p[0] + n[1] * p[1] - d
        sq = n[0] * q[0] + n[1] * q[1] - d
        if sp <= 0:
            out.append(p)
        if (sp <= 0) != (sq <= 0):
            t = sp / (sp - sq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def ground_intersection(a, b):
    """Area of the intersection of the ground rectangles of two rows."""
    mx, mz = (a[11] + b[11]) / 2, (a[13] + b[13]) / 2
    subject = _quad(a[10], a[9], a[14], a[11] - mx, a[13] - mz)
    clip = _quad(b[10], b[9], b[14], b[11] - mx, b[13] - mz)
    for i in range(4):
        if len(subject) < 3:
            return 0.0
        p, q = clip[i], clip[(i + 1) % 4]
        n = (q[1] - p[1], -(q[0] - p[0]))           # outward for a counter-clockwise quad
        subject = _cut(subject, n, n[0] * p[0] + n[1] * p[1])
    if len(subject) < 3:
        return 0.0
    x, z = np.array([v[0] for v in subject]), np.array([v[1] for v in subject])
    twice = 0.0
    for i in range(len(x)):
        j = (i + 1) % len(x)
        twice += x[i] * z[j] - x[j] * z[i]
    return max(0.5 * twice, 0.0)


def box_overlap(a, b, metric, criterion=-1):
    """One pair; `metric` 0 image, 1 ground, 2 3-D; `criterion` -1 union, 0 the first box, 1 the second."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if metric == 0:
        if not (np.isfinite(a[4:8]).all() and np.isfinite(b[4:8]).all()):
            return 0.0
        w = min(a[6], b[6]) - max(a[4], b[4])
        h = min(a[7], b[7]) - max(a[5], b[5])
        if w <= 0 or h <= 0:
            return 0.0
        return float(_ratio(w * h, (a[6] - a[4]) * (a[7] - a[5]), (b[6] - b[4]) * (b[7] - b[5]), criterion))
    used = [9, 10, 11, 13, 14] + ([8, 12] if metric == 2 else [])
    if not (np.isfinite(a[used]).all() and np.isfinite(b[used]).all()):
        return 0.0
    if a[9] <= 0 or a[10] <= 0 or b[9] <= 0 or b[10] <= 0:
        return 0.0
    # (a shortcut that changes no value: two rectangles whose centres are further apart than their half diagonals together are disjoint)
    if np.hypot(a[11] - b[11], a[13] - b[13]) > 0.5 * (np.hypot(a[9], a[10]) + np.hypot(b[9], b[10])) * (1 + 1e-9) + 1e-9:
        return 0.0
    inter = ground_intersection(a, b)
    if not inter > 0:
        return 0.0
    if metric == 1:
        return float(_ratio(inter, a[10] * a[9], b[10] * b[9], criterion))
    if a[8] <= 0 or b[8] <= 0:
        return 0.0
    hh = min(a[12], b[12]) - max(a[12] - a[8], b[12] - b[8])
    if hh <= 0:
        return 0.0
    return float(_ratio(inter * hh, (a[8] * a[10]) * a[9], (b[8] * b[10]) * b[9], criterion))


def overlap_matrices(det, gt, criterion=-1, dontcare_first=False):
    """-> (3, nd, ng).  `dontcare_first`: the column of a DontCare label holds the criterion-0 overlap (what the matching reads)."""
    det, gt = np.asarray(det, dtype=np.float64).reshape(-1, 16), np.asarray(gt, dtype=np.float64).reshape(-1, 16)
    out = np.zeros((3, len(det), len(gt)))
    for g in range(len(gt)):
        c = 0 if (dontcare_first and gt[g, 0] == 5.0) else criterion
        for d in range(len(det)):
            for m in range(3):
                out[m, d, g] = box_overlap(det[d], gt[g], m, c)
    return out


# ------------------------------------------------------------------ cleaning
def gt_flags(gt, cls, dif):
    """0 counted, 1 ignored, -1 absent, 2 don't care."""
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 16)
    t, h2d = gt[:, 0], gt[:, 7] - gt[:, 5]
    ignored = (gt[:, 2] > MAX_OCCLUSION[dif]) | (gt[:, 1] > MAX_TRUNCATION[dif]) | (h2d < MIN_HEIGHT[dif])
    f = np.full(len(gt), -1, dtype=np.int64)
    f[t == cls] = np.where(ignored, 1, 0)[t == cls]
    if cls == 0:
        f[t == 3.0] = 1
    if cls == 1:
        f[t == 4.0] = 1
    f[t == 5.0] = 2
    return f


def det_flags(det, cls, dif):
    det = np.asarray(det, dtype=np.float64).reshape(-1, 16)
    f = np.where(det[:, 7] - det[:, 5] < MIN_HEIGHT[dif], 1, 0).astype(np.int64)
    f[det[:, 0] != cls] = -1
    return f


# ------------------------------------------------------------------ matching
def new_stats():
    return {"closest": np.inf, "gap": np.inf, "ignored_assignments": 0, "replaced_ignored": 0, "dontcare_removed": 0, "fn": 0, "score_ties": 0}


def _note_closest(stats, o, mask, min_ov):
    if mask.any():
        stats["closest"] = min(stats["closest"], float(np.abs(o[mask] - min_ov).min()))


def first_mode(ov, df, gf, score, min_ov, stats=None):
    """-> (emitted scores in emission order, tp, fn)."""
    stats = stats if stats is not None else new_stats()
    assigned = np.zeros(len(df), dtype=bool)
    emitted, tp, fn = [], 0, 0
    for g in range(len(gf)):
        if gf[g] not in (0, 1):
            continue
        live = (df >= 0) & ~assigned
        _note_closest(stats, ov[:, g], live, min_ov)
        elig = live & (ov[:, g] > min_ov)
        if not elig.any():
            fn += int(gf[g] == 0)
            stats["fn"] += int(gf[g] == 0)
            continue
        s = np.where(elig, score, -np.inf)
        cand = int(np.argmax(s))                      # the first maximum: a later equal score does not replace it
        stats["score_ties"] += int((s == s[cand]).sum() > 1)
        assigned[cand] = True
        if gf[g] == 0 and df[cand] == 0:
            tp += 1
            emitted.append(score[cand])
        else:
            stats["ignored_assignments"] += 1
    return np.asarray(emitted, dtype=np.float64), tp, fn


def second_mode(ov, df, gf, score, min_ov, thresholds, stats=None):
    """-> tp, fp, fn, one entry per threshold (int64).  Column g of `ov` is the criterion-0 overlap where gf[g] == 2."""
    stats = stats if stats is not None else new_stats()
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    K, nd = len(t), len(df)
    assigned = np.zeros((K, nd), dtype=bool)
    tp, fp, fn = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    if K == 0:
        return tp, fp, fn
    if nd == 0:                                                   # no detection: every counted label is missed
        n = int((np.asarray(gf) == 0).sum())
        stats["fn"] += n * K
        return tp, fp, fn + n
    scanned = (df >= 0)[None, :] & ~(score[None, :] < t[:, None])
    counted = (df == 0)[None, :] & (score[None, :] >= t[:, None])
    for g in range(len(gf)):
        if gf[g] not in (0, 1):
            continue
        o = ov[:, g]
        live = scanned & ~assigned
        _note_closest(stats, o, live.any(axis=0), min_ov)
        elig = live & (o > min_ov)[None, :]
        e0, e1 = elig & (df == 0)[None, :], elig & (df == 1)[None, :]
        has0, has1 = e0.any(axis=1), e1.any(axis=1)
        o0 = np.where(e0, o[None, :], -np.inf)
        c0, c1 = np.argmax(o0, axis=1), np.argmax(e1, axis=1)     # the largest overlap (first on a tie); the first flag-1 detection
        if nd >= 2:
            top = np.sort(o0, axis=1)[:, -2:]
            both = np.isfinite(top[:, 0])
            if both.any():
                stats["gap"] = min(stats["gap"], float((top[both, 1] - top[both, 0]).min()))
        first0 = np.argmax(e0, axis=1)
        stats["replaced_ignored"] += int((has0 & has1 & (c1 < first0)).sum())
        cand = np.where(has0, c0, np.where(has1, c1, -1))
        cand_ignored = ~has0 & has1
        found = cand >= 0
        rows = np.nonzero(found)[0]
        assigned[rows, cand[rows]] = True
        if gf[g] == 0:
            fn += ~found
            tp += found & ~cand_ignored
            stats["fn"] += int((~found).sum())
            stats["ignored_assignments"] += int((found & cand_ignored).sum())
        else:
            stats["ignored_assignments"] += int(found.sum())
    fp += (counted & ~assigned).sum(axis=1)
    for g in range(len(gf)):
        if gf[g] != 2:
            continue
        o = ov[:, g]
        live = counted & ~assigned
        _note_closest(stats, o, live.any(axis=0), min_ov)
        hit = live & (o > min_ov)[None, :]
        assigned |= hit
        fp -= hit.sum(axis=1)
        stats["dontcare_removed"] += int(hit.sum())
    return tp, fp, fn


# ------------------------------------------------------------------ thresholds and AP
def pick_thresholds(scores_desc, n_gt):
    v = np.asarray(scores_desc, dtype=np.float64)
    out, current = [], 0.0
    for i in range(len(v)):
        if len(out) >= N_SAMPLES:
            break
        l = (i + 1) / n_gt
        r = (i + 2) / n_gt if i < len(v) - 1 else l
        if (r - current) < (current - l) and i < len(v) - 1:
            continue
        out.append(v[i])
        current += 1 / 40
    return np.asarray(out, dtype=np.float64)


def curves(tp, fp, fn):
    """-> precision[41] (with the running maximum from the right), recall[41], ap11, ap40; the sums run in index order."""
    precision, recall = np.zeros(N_SAMPLES), np.zeros(N_SAMPLES)
    for k in range(len(tp)):
        a, b, c = int(tp[k]), int(fp[k]), int(fn[k])
        recall[k] = a / (a + c) if a + c else 0.0
        precision[k] = a / (a + b) if a + b else 0.0
    for k in range(N_SAMPLES - 2, -1, -1):
        precision[k] = max(precision[k], precision[k + 1])
    s11 = 0.0
    for k in range(0, N_SAMPLES, 4):
        s11 += precision[k]
    s40 = 0.0
    for k in range(1, N_SAMPLES):
        s40 += precision[k]
    return precision, recall, 100.0 * (s11 / 11.0), 100.0 * (s40 / 40.0)


def frame_overlaps(gt_frames, det_frames):
    return [overlap_matrices(d, g, -1, dontcare_first=True) for g, d in zip(gt_frames, det_frames)]


def match_all(gt_frames, det_frames, cls, dif, metric, mode, thresholds=None, min_overlap=None, overlaps=None, stats=None):
    """The staged call over all frames: mode 1 -> (scores descending, tp, fn, n_gt); mode 2 -> (tp, fp, fn) per threshold."""
    mo = MIN_OVERLAP if min_overlap is None else np.asarray(min_overlap, dtype=np.float64)
    overlaps = overlaps if overlaps is not None else frame_overlaps(gt_frames, det_frames)
    stats = stats if stats is not None else new_stats()
    if mode == 1:
        scores, tp, fn, n_gt = [], 0, 0, 0
    else:
        K = len(thresholds)
        tp, fp, fn = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    for g, d, ov in zip(gt_frames, det_frames, overlaps):
        g, d = np.asarray(g, dtype=np.float64).reshape(-1, 16), np.asarray(d, dtype=np.float64).reshape(-1, 16)
        gf, df = gt_flags(g, cls, dif), det_flags(d, cls, dif)
        if mode == 1:
            s, a, c = first_mode(ov[metric], df, gf, d[:, 15], mo[metric][cls], stats)
            scores.append(s)
            tp += a
            fn += c
            n_gt += int((gf == 0).sum())
        else:
            a, b, c = second_mode(ov[metric], df, gf, d[:, 15], mo[metric][cls], thresholds, stats)
            tp += a
            fp += b
            fn += c
    if mode == 1:
        scores = np.sort(np.concatenate(scores) if scores else np.zeros(0))[::-1]
        return scores, tp, fn, n_gt
    return tp, fp, fn


def evaluate(gt_frames, det_frames, min_overlap=None, overlaps=None, stats=None):
    """-> {class: {metric: {difficulty: cell}}}, a cell holding the fields of pcr_kitti_eval_cell."""
    overlaps = overlaps if overlaps is not None else frame_overlaps(gt_frames, det_frames)
    stats = stats if stats is not None else new_stats()
    out = {}
    for c, cname in enumerate(CLASSES):
        for m, mname in enumerate(METRICS):
            for d, dname in enumerate(DIFFICULTIES):
                scores, _, _, n_gt = match_all(gt_frames, det_frames, c, d, m, 1, None, min_overlap, overlaps, stats)
                thr = pick_thresholds(scores, n_gt) if n_gt else np.zeros(0)
                tp, fp, fn = match_all(gt_frames, det_frames, c, d, m, 2, thr, min_overlap, overlaps, stats)
                precision, recall, ap11, ap40 = curves(tp, fp, fn)
                pad = lambda a, dt: np.concatenate([np.asarray(a, dtype=dt), np.zeros(N_SAMPLES - len(a), dtype=dt)])   # noqa: E731
                out.setdefault(cname, {}).setdefault(mname, {})[dname] = {
                    "n_gt": int(n_gt), "n_thresholds": len(thr), "thresholds": pad(thr, np.float64), "tp": pad(tp, np.int64), "fp": pad(fp, np.int64),
                    "fn": pad(fn, np.int64), "precision": precision, "recall": recall, "ap11": ap11, "ap40": ap40}
    return out


# ------------------------------------------------------------------ frames
_SIZE = {0: (1.5, 1.6, 3.9), 1: (1.7, 0.6, 0.8), 2: (1.7, 0.6, 1.8), 3: (2.0, 1.9, 5.0), 4: (1.3, 0.6, 0.8), 6: (3.0, 2.5, 8.0)}   # h, w, l
_DET_CLASS = {0: 0, 1: 1, 2: 2, 3: 0, 4: 1, 6: 0}
_HEIGHT_2D = (18.0, 24.5, 25.0, 25.5, 33.0, 39.5, 40.0, 40.5, 60.0, 90.0)
_TRUNCATION = (0.0, 0.0, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.6)


def dontcare_row(left, top, right, bottom):
    return np.array([5.0, -1.0, -1.0, -10.0, left, top, right, bottom, -1.0, -1.0, -1.0, -1000.0, -1000.0, -1000.0, -10.0, 0.0])


def make_frame(rng, n_labels, n_det, spread=1.0):
    """One frame -> (gt (n,16), det (m,16)): labels of every type code with occlusion 0-3, truncation around the three limits and 2-D
    heights around 25 and 40; detections that are jittered copies of labels (centre, size, ry, score; some twice, some with the same
    score, some with a flat 2-D box) plus false positives, some of them inside a DontCare region; about `n_det` detections."""
    gt = []
    n_dc = 1 + int(rng.integers(0, 2)) if n_labels >= 3 else 0
    for _ in range(max(n_labels - n_dc, 0)):
        t = int(rng.choice([0, 0, 0, 1, 1, 2, 2, 3, 4, 6]))
        h, w, l = np.asarray(_SIZE[t]) * rng.uniform(0.9, 1.1, size=3)
        h2 = float(rng.choice(_HEIGHT_2D)) if rng.random() < 0.7 else float(np.round(rng.uniform(20, 120), 2))
        w2 = float(np.round(h2 * rng.uniform(0.5, 2.0), 2))
        left, top = float(np.round(rng.uniform(0, 1100), 2)), float(np.round(rng.uniform(100, 250), 2))
        gt.append([t, float(rng.choice(_TRUNCATION)), float(rng.integers(0, 4)), -10.0, left, top, left + w2, top + h2, h, w, l,
                   rng.uniform(-20, 20) * spread, rng.uniform(1.4, 1.9), rng.uniform(5, 60) * spread, rng.uniform(-np.pi, np.pi), 0.0])
    dcs = []
    for _ in range(n_dc):
        left, top = float(np.round(rng.uniform(0, 1000), 2)), float(np.round(rng.uniform(100, 250), 2))
        dcs.append(dontcare_row(left, top, left + 128.0, top + 64.0))
    det = []

    def copy_of(row, flat=False, score=None):
        d = np.array(row, dtype=np.float64)
        d[0] = _DET_CLASS[int(row[0])]
        d[1], d[2], d[3] = -1.0, -1.0, -10.0
        d[8:11] *= rng.uniform(0.93, 1.07, size=3)
        d[11:14] += rng.normal(0, 0.12, size=3)
        d[14] += rng.normal(0, 0.06)
        d[4:8] += rng.uniform(-0.03, 0.03, size=4) * (row[7] - row[5])
        if flat:
            d[7] = d[5] + 20.0                      # under every height limit: flag 1 at every difficulty
        d[15] = float(np.round(rng.uniform(0.05, 1.0), 2)) if score is None else score
        return d

    budget = n_det
    for row in gt:
        if budget <= 0 or rng.random() < 0.2:
            continue                                # a miss
        twice = budget >= 2 and rng.random() < 0.35
        if twice and rng.random() < 0.5:
            det.append(copy_of(row, flat=True))     # a flat copy in front of the good one
            budget -= 1
            twice = False
        first = copy_of(row)
        det.append(first)
        budget -= 1
        if twice:
            det.append(copy_of(row, score=first[15] if rng.random() < 0.5 else None))
            budget -= 1
    while budget > 0:                               # false positives
        t = int(rng.choice([0, 1, 2]))
        h, w, l = np.asarray(_SIZE[t]) * rng.uniform(0.9, 1.1, size=3)
        if dcs and rng.random() < 0.5:
            dc = dcs[int(rng.integers(0, len(dcs)))]
            left, top, h2 = dc[4] + 16.0, dc[5] + 4.0, 48.0
        else:
            left, top, h2 = float(np.round(rng.uniform(0, 1100), 2)), float(np.round(rng.uniform(100, 250), 2)), float(np.round(rng.uniform(20, 100), 2))
        det.append(np.array([t, -1.0, -1.0, -10.0, left, top, left + 0.75 * h2, top + h2, h, w, l, rng.uniform(-20, 20) * spread, rng.uniform(1.4, 1.9),
                             rng.uniform(5, 60) * spread, rng.uniform(-np.pi, np.pi), float(np.round(rng.uniform(0.05, 1.0), 2))]))
        budget -= 1
    gt = [np.asarray(r, dtype=np.float64) for r in gt] + dcs
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 16)
    det = np.asarray(det, dtype=np.float64).reshape(-1, 16)
    return gt[rng.permutation(len(gt))], det[rng.permutation(len(det))]


def make_frames(seed, n_frames, n_labels=10, n_det=15, vary=True):
    """-> (gt_frames, det_frames): lists of (n,16) arrays; with `vary` the sizes are drawn around the given ones."""
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    for _ in range(n_frames):
        nl = int(rng.integers(max(n_labels // 2, 1), n_labels + 1)) if vary else n_labels
        nd = int(rng.integers(max(n_det // 2, 1), n_det + 1)) if vary else n_det
        g, d = make_frame(rng, nl, nd)
        gts.append(g)
        dets.append(d)
    return gts, dets


def ragged(frames):
    """list of (n,16) -> (rows (N,16), first (F+1,) int64)."""
    first = np.zeros(len(frames) + 1, dtype=np.int64)
    for i, f in enumerate(frames):
        first[i + 1] = first[i] + len(f)
    rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 16) for f in frames]) if frames else np.zeros((0, 16))
    return np.ascontiguousarray(rows.reshape(-1, 16)), first


def box(cx=0.0, cz=0.0, l=1.0, w=1.0, ry=0.0, h=1.0, cy=0.0, rect=(0.0, 0.0, 1.0, 1.0), type=0.0, score=0.0):
    """A row from its 3-D box and 2-D rectangle (left, top, right, bottom)."""
    return np.array([type, 0.0, 0.0, -10.0, rect[0], rect[1], rect[2], rect[3], h, w, l, cx, cy, cz, ry, score])


def special_pairs():
    """(name, a, b, {(metric, criterion): the value known in closed form}).  The extents are powers of two and the offsets dyadic with
    ry = 0 wherever the table says "exact": every product, quotient of the clip and sum is then exact in binary64, so ANY correct order
    of operations yields the same bits, and the final quotient is one correctly rounded division."""
    out = []
    a = box(0, 0, 4, 2, 0, h=2, cy=1, rect=(0, 0, 8, 4))
    out.append(("identical", a, a.copy(), {(0, -1): 1.0, (1, -1): 1.0, (2, -1): 1.0, (1, 0): 1.0, (2, 1): 1.0}))
    b = box(1, 0.5, 4, 2, 0, h=2, cy=2, rect=(2, 1, 10, 5))    # ground 3 x 1.5 = 4.5 of 8 + 8; height overlap 1; image 6 x 3 = 18 of 32 + 32
    out.append(("shifted", a, b, {(0, -1): 18 / 46, (0, 0): 18 / 32, (0, 1): 18 / 32, (1, -1): 4.5 / 11.5, (1, 0): 4.5 / 8, (1, 1): 4.5 / 8,
                                  (2, -1): 4.5 / 27.5, (2, 0): 4.5 / 16, (2, 1): 4.5 / 16}))
    b = box(4, 0, 4, 2, 0, h=2, cy=1, rect=(8, 0, 16, 4))
    out.append(("shared edge", a, b, {(0, -1): 0.0, (1, -1): 0.0, (2, -1): 0.0}))
    b = box(4, 2, 4, 2, 0, h=2, cy=1, rect=(8, 4, 16, 8))
    out.append(("shared corner", a, b, {(0, -1): 0.0, (1, -1): 0.0, (2, -1): 0.0}))
    b = box(0.5, 0.25, 2, 1, 0, h=1, cy=0.5, rect=(2, 1, 6, 3))   # inside a: ground 2 of 8, volume 2 of 16, image 8 of 32
    out.append(("inside", a, b, {(0, -1): 8 / 32, (0, 0): 8 / 32, (0, 1): 1.0, (1, -1): 2 / 8, (1, 0): 2 / 8, (1, 1): 1.0, (2, -1): 2 / 16, (2, 0): 2 / 16,
                                 (2, 1): 1.0}))
    b = box(0, 0, 4, 2, 0, h=2, cy=3, rect=(0, 0, 8, 4))
    out.append(("heights touch", a, b, {(1, -1): 1.0, (2, -1): 0.0}))
    b = box(0, 0, 4, 2, 0, h=2, cy=8, rect=(0, 0, 8, 4))
    out.append(("heights disjoint", a, b, {(1, -1): 1.0, (2, -1): 0.0}))
    b = box(0, 0, 4, 0, 0, h=2, cy=1, rect=(0, 0, 8, 4))
    out.append(("zero width", a, b, {(0, -1): 1.0, (1, -1): 0.0, (2, -1): 0.0}))
    b = box(0, 0, -4, 2, 0, h=2, cy=1, rect=(0, 0, 8, 0))
    out.append(("negative length, flat rectangle", a, b, {(0, -1): 0.0, (1, -1): 0.0, (2, -1): 0.0}))
    b = box(0, 0, 4, 2, 0, h=0, cy=1, rect=(0, 0, 8, 4))
    out.append(("zero height", a, b, {(1, -1): 1.0, (2, -1): 0.0}))
    b = box(50, 40, 4, 2, 0, h=2, cy=1, rect=(100, 100, 108, 104))
    out.append(("far apart", a, b, {(0, -1): 0.0, (1, -1): 0.0, (2, -1): 0.0}))
    out.append(("dontcare", a, dontcare_row(0, 0, 16, 4), {(0, 0): 1.0, (0, -1): 0.5, (1, 0): 0.0, (2, 0): 0.0}))
    b = a.copy()
    b[11] = np.nan
    out.append(("a field that is not finite", a, b, {(0, -1): 1.0, (1, -1): 0.0, (2, -1): 0.0}))
    return out
