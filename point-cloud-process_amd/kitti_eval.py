"""The step behind ``to_kitti_eval_format``: what the reference runs on the label files it has written (Final_Project/README.md:225-236,
``evaluate_object_3d_offline`` of its ``kitti_eval`` submodule) -- box overlaps, the greedy detection-to-label matching at up to 41
score thresholds, and the average precision per class, metric (image box, bird's-eye box, 3-D box) and difficulty -- for all frames in
one device call (include/pcr.h, "KITTI evaluation").

The submodule is empty in the reference, so the rules are the ones include/pcr.h writes down; parity with the tool's own binary is
UNPINNED.  Orientation similarity is not evaluated (the reference writes ``alpha = -10``).  There is no CPU fallback: without a HIP
device the compute entry points fail as the others do; ``pcr_kitti_box_overlap`` (one pair, on the host) is the exception.

    python -m point-cloud-process_amd.kitti_eval GT_DIR RESULT_DIR      (through importlib, the directory name has a hyphen:
    python -c "import pcp_amd; pcp_amd.kitti_eval.main()" GT_DIR RESULT_DIR)
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import sys

import numpy as np

from . import _lib as L
from .detection import KITTI_COLUMNS
from .device import default_context

__all__ = ["TYPE_CODE", "CLASSES", "METRICS", "DIFFICULTIES", "read_label_file", "read_label_dir", "frames_from", "box_overlap", "box_overlaps", "match",
           "evaluate", "evaluate_object_3d_offline", "main"]

TYPE_CODE = {"Car": 0, "Pedestrian": 1, "Cyclist": 2, "Van": 3, "Person_sitting": 4, "DontCare": 5}   # anything else: 6
CLASSES = ("car", "pedestrian", "cyclist")
METRICS = ("image", "ground", "3d")
DIFFICULTIES = ("easy", "moderate", "hard")
_SUFFIX = {"image": "", "ground": "_ground", "3d": "_3d"}
SAMPLES = L.PCR_KITTI_EVAL_SAMPLES


# ------------------------------------------------------------------ rows
def _rows_of_table(table):
    """Rows of (type name, 14 or 15 numbers) -> (n,16): the type as its code, a missing score as 0."""
    out = np.zeros((len(table), 16), dtype=np.float64)
    for i, row in enumerate(table):
        if len(row) not in (15, 16):
            raise ValueError(f"a label row has 15 columns (ground truth) or 16 (results), not {len(row)}")
        name = row[0]
        out[i, 0] = TYPE_CODE.get(name, 6) if isinstance(name, str) else float(name)
        out[i, 1:len(row)] = [float(v) for v in row[1:]]
    return out


def read_label_file(filepath):
    """A KITTI label file -> (n,16) rows in ``detection.KITTI_COLUMNS`` order: 15 columns (ground truth, score 0) or 16 (results); the type
    name becomes its code (Car 0, Pedestrian 1, Cyclist 2, Van 3, Person_sitting 4, DontCare 5, anything else 6).  The split on blanks
    is ``extract.read_label``'s ``sep=' '``; nothing is dropped and no frame transform is applied."""
    with open(filepath, "rt") as f:
        return _rows_of_table([line.split() for line in f if line.strip()])


def read_label_dir(dirpath, names=None):
    """-> (names, frames): the ``*.txt`` files of a directory in sorted order, or the given `names` (a missing one raises)."""
    if names is None:
        names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(dirpath, "*.txt")))
    frames = []
    for name in names:
        path = os.path.join(dirpath, name)
        if not os.path.exists(path):
            raise FileNotFoundError(f"no label file {path}")
        frames.append(read_label_file(path))
    return list(names), frames


def frames_from(frames):
    """A list of frames -> list of (n,16) float64 arrays.  A frame may be an (n,16) or (n,15) array of numbers (type codes), a list of
    rows with type names, or the DataFrame ``to_kitti_eval_format`` returns (type names, numbers as ``'.2f'`` strings)."""
    out = []
    for fr in frames:
        if hasattr(fr, "columns") and hasattr(fr, "values"):          # a DataFrame
            cols = [c for c in KITTI_COLUMNS if c in fr.columns]
            out.append(_rows_of_table([list(r) for r in fr[cols].values.tolist()]))
            continue
        if isinstance(fr, np.ndarray) and fr.dtype != object:
            a = np.asarray(fr, dtype=np.float64)
            a = a.reshape(-1, a.shape[-1] if a.ndim == 2 else 16)
            if a.shape[1] == 15:
                a = np.hstack([a, np.zeros((len(a), 1))])
            if a.shape[1] != 16:
                raise ValueError("a frame of numbers has 15 or 16 columns")
            out.append(np.ascontiguousarray(a))
            continue
        out.append(_rows_of_table([list(r) for r in fr]))
    return out


def _ragged(frames):
    first = np.zeros(len(frames) + 1, dtype=np.int64)
    for i, fr in enumerate(frames):
        first[i + 1] = first[i] + len(fr)
    rows = np.concatenate(frames).reshape(-1, 16) if frames else np.zeros((0, 16))
    return np.ascontiguousarray(rows, dtype=np.float64), first


def _ptr(a):
    return L.dptr(a) if a.size else None


def _params(min_overlap):
    p = L.KittiEvalParams()
    L.lib().pcr_kitti_eval_default_params(C.byref(p))
    if min_overlap is not None:
        mo = np.asarray(min_overlap, dtype=np.float64).reshape(3, 3)      # [metric][class]
        for m in range(3):
            for c in range(3):
                p.min_overlap[m][c] = mo[m, c]
    return p


# ------------------------------------------------------------------ overlaps
def box_overlap(a, b, metric, criterion=-1):
    """One pair on the host (``pcr_kitti_box_overlap``: the source the kernel compiles): `metric` 0 / 'image', 1 / 'ground', 2 / '3d'."""
    m = METRICS.index(metric) if isinstance(metric, str) else int(metric)
    a, b = L.as_f64(a).reshape(16), L.as_f64(b).reshape(16)
    out = C.c_double()
    L.check(L.lib().pcr_kitti_box_overlap(L.dptr(a), L.dptr(b), m, int(criterion), C.byref(out)))
    return out.value


def _overlaps(det_frames, gt_frames, criterion, ctx):
    ctx = ctx or default_context()
    det, det_first = _ragged(det_frames)
    gt, gt_first = _ragged(gt_frames)
    F = len(det_frames)
    total = int(sum(len(d) * len(g) for d, g in zip(det_frames, gt_frames)))
    mats = [np.zeros(total) for _ in range(3)]
    pair_first = np.zeros(F + 1, dtype=np.int64)
    L.check(L.lib().pcr_kitti_eval_overlaps(ctx.handle, _ptr(det), L.lptr(det_first), _ptr(gt), L.lptr(gt_first), F, int(criterion), _ptr(mats[0]), _ptr(mats[1]),
                                            _ptr(mats[2]), L.lptr(pair_first)), ctx.handle)
    return mats, pair_first


def box_overlaps(det_rows, gt_rows, criterion=-1, ctx=None):
    """All pairs of one frame on the device -> ``{'image', 'ground', '3d'}``: (len(det_rows), len(gt_rows)) matrices; `criterion` -1
    union, 0 the detection's area or volume, 1 the label's."""
    det, gt = frames_from([det_rows])[0], frames_from([gt_rows])[0]
    mats, _ = _overlaps([det], [gt], criterion, ctx)
    return {name: mats[m].reshape(len(det), len(gt)) for m, name in enumerate(METRICS)}


# ------------------------------------------------------------------ matching and AP
def match(gt_frames, det_frames, cls, difficulty, metric, mode, thresholds=None, min_overlap=None, ctx=None):
    """The staged call (``pcr_kitti_eval_match``): one (class, difficulty, metric) through the kernels of the whole evaluation.
    mode 1 -> (scores descending, tp, fn, n_gt); mode 2 -> (tp, fp, fn), int64 arrays with one entry per threshold."""
    ctx = ctx or default_context()
    gts, dets = frames_from(gt_frames), frames_from(det_frames)
    if len(gts) != len(dets):
        raise ValueError("as many ground-truth frames as result frames")
    det, det_first = _ragged(dets)
    gt, gt_first = _ragged(gts)
    p = _params(min_overlap)
    lib = L.lib()
    if mode == 1:
        scores = np.zeros(max(int((gt[:, 0] == cls).sum()), 1))
        n, tp, fn, n_gt = (np.zeros(1, dtype=np.int64) for _ in range(4))
        L.check(lib.pcr_kitti_eval_match(ctx.handle, _ptr(det), L.lptr(det_first), _ptr(gt), L.lptr(gt_first), len(gts), C.byref(p), int(cls), int(difficulty),
                                         int(metric), None, 0, 1, L.lptr(tp), L.lptr(n_gt), L.lptr(fn), L.dptr(scores), L.lptr(n)), ctx.handle)
        return scores[:int(n[0])].copy(), int(tp[0]), int(fn[0]), int(n_gt[0])
    t = L.as_f64(thresholds).reshape(-1)
    K = len(t)
    tp, fp, fn = (np.zeros(max(K, 1), dtype=np.int64) for _ in range(3))
    L.check(lib.pcr_kitti_eval_match(ctx.handle, _ptr(det), L.lptr(det_first), _ptr(gt), L.lptr(gt_first), len(gts), C.byref(p), int(cls), int(difficulty), int(metric),
                                     _ptr(t), K, 2, L.lptr(tp), L.lptr(fp), L.lptr(fn), None, None), ctx.handle)
    return tp[:K], fp[:K], fn[:K]


def _evaluate_raw(gt_frames, det_frames, min_overlap=None, ctx=None, stage_ms=None):
    ctx = ctx or default_context()
    gts, dets = frames_from(gt_frames), frames_from(det_frames)
    if len(gts) != len(dets):
        raise ValueError("as many ground-truth frames as result frames")
    det, det_first = _ragged(dets)
    gt, gt_first = _ragged(gts)
    p = _params(min_overlap)
    res = L.KittiEvalResult()
    L.check(L.lib().pcr_kitti_eval(ctx.handle, _ptr(det), L.lptr(det_first), _ptr(gt), L.lptr(gt_first), len(gts), C.byref(p), C.byref(res),
                                   L.dptr(stage_ms) if stage_ms is not None else None), ctx.handle)
    return res


def _cell(c):
    return {"n_gt": int(c.n_gt), "n_thresholds": int(c.n_thresholds), "thresholds": np.array(c.thresholds[:]), "tp": np.array(c.tp[:], dtype=np.int64),
            "fp": np.array(c.fp[:], dtype=np.int64), "fn": np.array(c.fn[:], dtype=np.int64), "precision": np.array(c.precision[:]), "recall": np.array(c.recall[:]),
            "ap11": float(c.ap11), "ap40": float(c.ap40)}


def evaluate(gt_frames, det_frames, min_overlap=None, ctx=None):
    """All frames in one device call -> ``result[class][metric][difficulty]`` (``'car' | 'pedestrian' | 'cyclist'``, ``'image' | 'ground' |
    '3d'``, ``'easy' | 'moderate' | 'hard'``), each a dict with the fields of ``pcr_kitti_eval_cell``: ``n_gt, n_thresholds, thresholds,
    tp, fp, fn, precision, recall`` (41 entries) and ``ap11, ap40``.  `min_overlap`: a 3 x 3 table [metric][class] in place of
    0.7 / 0.5 / 0.5.  Frames as ``frames_from`` takes them."""
    res = _evaluate_raw(gt_frames, det_frames, min_overlap, ctx)
    return {cn: {mn: {dn: _cell(res.cell[c][m][d]) for d, dn in enumerate(DIFFICULTIES)} for m, mn in enumerate(METRICS)} for c, cn in enumerate(CLASSES)}


def evaluate_object_3d_offline(gt_dir, result_dir, ctx=None, write=True):
    """The tool's command line: evaluates the frames named by ``result_dir/data/*.txt`` against ``gt_dir/<same name>`` (a frame without
    its ground-truth file raises), prints one ``<class>_detection[_ground|_3d] AP: easy moderate hard`` line (``ap11``) per class and
    metric, writes ``result_dir/stats_<class>_detection[_ground|_3d].txt`` (three lines of 41 precisions) and returns what ``evaluate``
    returns.  A class without a counted label at any difficulty is skipped in print and files."""
    names, dets = read_label_dir(os.path.join(result_dir, "data"))
    _, gts = read_label_dir(gt_dir, names)
    result = evaluate(gts, dets, ctx=ctx)
    for cn in CLASSES:
        if all(result[cn][mn][dn]["n_gt"] == 0 for mn in METRICS for dn in DIFFICULTIES):
            continue
        for mn in METRICS:
            tag = f"{cn}_detection{_SUFFIX[mn]}"
            print(f"{tag} AP: " + " ".join(f"{result[cn][mn][dn]['ap11']:f}" for dn in DIFFICULTIES))
            if write:
                with open(os.path.join(result_dir, f"stats_{tag}.txt"), "wt") as f:
                    for dn in DIFFICULTIES:
                        f.write(" ".join(f"{v:f}" for v in result[cn][mn][dn]["precision"]) + "\n")
    return result


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        print("usage: kitti_eval GT_DIR RESULT_DIR", file=sys.stderr)
        return 2
    evaluate_object_3d_offline(argv[0], argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
