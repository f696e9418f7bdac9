"""KITTI evaluation without a GPU: the restatement (tests/kitti_eval_checks.py) and the host's pcr_kitti_box_overlap -- the source the
overlap kernel compiles -- against answers known by hand; the threshold loop and AP on a worked case; the cleaning flags at their exact
limits; the ABI; the readers."""
import ctypes as C

import numpy as np
import pytest

from tests import kitti_eval_checks as chk


def host_overlap(pcp, a, b, metric, criterion=-1):
    return pcp.kitti_eval.box_overlap(a, b, metric, criterion)


def test_special_pairs_in_closed_form_equal_to_the_bit(pcp):
    """Dyadic extents, ry = 0: every intermediate of either clip is exact, so the closed-form value, the restatement and the host
    function agree in every bit."""
    for name, a, b, want in chk.special_pairs():
        for (metric, criterion), value in want.items():
            r = chk.box_overlap(a, b, metric, criterion)
            h = host_overlap(pcp, a, b, metric, criterion)
            assert r == value and h == value, (name, metric, criterion, value, r, h)


def test_two_unit_squares_at_45_degrees(pcp):
    """About one centre the intersection is a regular octagon of area 2(sqrt 2 - 1); union 2 - that.  Eight vertices of magnitude <= 0.71:
    a few roundings of 1.1e-16 each."""
    a, b = chk.box(3, 7, 1, 1, 0.0), chk.box(3, 7, 1, 1, np.pi / 4)
    area = 2 * (np.sqrt(2) - 1)
    for f in (chk.box_overlap, lambda *x: host_overlap(pcp, *x)):
        assert abs(f(a, b, 1, 0) - area) < 1e-14
        assert abs(f(a, b, 1, 1) - area) < 1e-14
        assert abs(f(a, b, 1, -1) - area / (2 - area)) < 1e-14
        assert abs(f(a, b, 2, -1) - area / (2 - area)) < 1e-14       # h = 1, cy = 0 for both


def test_ry_and_ry_plus_pi_agree_and_rotation_keeps_the_overlap(pcp):
    rng = np.random.default_rng(5)
    for _ in range(50):
        a = chk.box(rng.uniform(-30, 30), rng.uniform(5, 60), rng.uniform(1, 5), rng.uniform(0.5, 2), rng.uniform(-3, 3), h=1.5, cy=1.6)
        b = chk.box(a[11] + rng.normal(0, 0.5), a[13] + rng.normal(0, 0.5), rng.uniform(1, 5), rng.uniform(0.5, 2), rng.uniform(-3, 3), h=1.6, cy=1.7)
        b2 = b.copy()
        b2[14] += np.pi
        for f in (chk.box_overlap, lambda *x: host_overlap(pcp, *x)):
            for metric in (1, 2):
                o, o2 = f(a, b, metric, -1), f(a, b2, metric, -1)
                assert 0.0 <= o <= 1.0
                assert abs(o - o2) < 1e-13
        assert abs(chk.box_overlap(a, b, 1, -1) - host_overlap(pcp, a, b, 1, -1)) < 1e-13
        # symmetric in the union criterion
        assert abs(host_overlap(pcp, a, b, 1, -1) - host_overlap(pcp, b, a, 1, -1)) < 1e-13


def test_axis_aligned_overlaps_in_closed_form(pcp):
    rng = np.random.default_rng(6)
    for _ in range(50):
        la, wa, lb, wb = rng.uniform(0.5, 5, size=4)
        dx, dz = rng.uniform(-3, 3, size=2)
        a, b = chk.box(10, 20, la, wa, 0.0, h=2, cy=1), chk.box(10 + dx, 20 + dz, lb, wb, 0.0, h=3, cy=2)
        ix = max(0.0, min(la / 2, dx + lb / 2) - max(-la / 2, dx - lb / 2))
        iz = max(0.0, min(wa / 2, dz + wb / 2) - max(-wa / 2, dz - wb / 2))
        want = ix * iz / (la * wa + lb * wb - ix * iz)
        want3 = ix * iz * 2 / (2 * la * wa + 3 * lb * wb - ix * iz * 2)      # heights [-1, 1] and [-1, 2]: 2 in common
        for f in (chk.box_overlap, lambda *x: host_overlap(pcp, *x)):
            assert abs(f(a, b, 1, -1) - want) < 1e-13
            assert abs(f(a, b, 2, -1) - want3) < 1e-13
            # a quarter turn swaps length and width
            a90 = chk.box(10, 20, wa, la, np.pi / 2, h=2, cy=1)
            assert abs(f(a90, b, 1, -1) - want) < 1e-13


def test_host_function_refuses_bad_arguments(pcp):
    L = pcp._lib
    a = chk.box()
    out = C.c_double(7.0)
    lib = L.lib()
    assert lib.pcr_kitti_box_overlap(L.dptr(a), L.dptr(a), 3, -1, C.byref(out)) == L.PCR_E_INVALID
    assert lib.pcr_kitti_box_overlap(L.dptr(a), L.dptr(a), 0, 2, C.byref(out)) == L.PCR_E_INVALID
    assert lib.pcr_kitti_box_overlap(None, L.dptr(a), 0, -1, C.byref(out)) == L.PCR_E_INVALID
    assert lib.pcr_kitti_box_overlap(L.dptr(a), L.dptr(a), 0, -1, None) == L.PCR_E_INVALID
    assert out.value == 7.0


def test_threshold_loop_and_ap_worked_by_hand():
    """n_gt = 4, v = [0.9, 0.8, 0.7] (one label is never found).  current starts at 0 and grows by 0.025 per emitted threshold.
      i = 0: l = 0.25, r = 0.50: 0.5 - 0 >= 0 - 0.25: emits 0.9, current = 0.025.
      i = 1: l = 0.50, r = 0.75: 0.75 - 0.025 >= 0.025 - 0.5: emits 0.8, current = 0.05.
      i = 2: the last one, always emitted: 0.7, current = 0.075.
    Three thresholds.  With counts tp = [1, 2, 3], fp = [0, 1, 1], fn = [3, 2, 1]: recall = 1/4, 2/4, 3/4; precision = 1, 2/3, 3/4, then 0;
    the running maximum from the right gives 1, 3/4, 3/4, 0, ...  ap11 samples k = 0, 4, ...: only k = 0 is non-zero: 100 * (1/11);
    ap40 sums k = 1..40: 3/4 + 3/4: 100 * (1.5/40).
    A longer list shows the skipping: n_gt = 200 and 200 scores: l = (i+1)/200; thresholds are emitted where the recall grid of 1/40 is
    crossed, 5 scores apart, 41 in all (recall 0.005, then every 0.025 up to 1)."""
    thr = chk.pick_thresholds([0.9, 0.8, 0.7], 4)
    assert thr.tolist() == [0.9, 0.8, 0.7]
    precision, recall, ap11, ap40 = chk.curves([1, 2, 3], [0, 1, 1], [3, 2, 1])
    assert recall[:4].tolist() == [0.25, 0.5, 0.75, 0.0]
    assert precision[:4].tolist() == [1.0, 0.75, 0.75, 0.0] and not precision[3:].any()
    assert ap11 == 100.0 * (1.0 / 11.0) and ap40 == 100.0 * (1.5 / 40.0)
    v = np.linspace(1.0, 0.005, 200)
    thr = chk.pick_thresholds(v, 200)
    assert len(thr) == 41 and thr[0] == v[0] and thr[-1] == v[-1]
    picked = [int(np.nonzero(v == t)[0][0]) for t in thr]
    assert np.all(np.diff(picked) >= 4) and np.all(np.diff(picked) <= 6)
    assert len(chk.pick_thresholds([], 0)) == 0


def test_cleaning_flags_at_the_exact_limits():
    def label(type, trunc, occ, h2d):
        r = chk.box(type=float(type))
        r[1], r[2], r[5], r[7] = trunc, occ, 100.0, 100.0 + h2d
        return r

    rows = np.array([label(0, 0.15, 0, 40.0),      # easy: every limit met exactly: counted
                     label(0, 0.15, 0, 39.99),     # too low for easy, counted from moderate on
                     label(0, 0.30, 1, 25.0),      # moderate's limits exactly
                     label(0, 0.50, 2, 25.0),      # hard's limits exactly
                     label(0, 0.51, 2, 25.0),      # ignored everywhere
                     label(0, 0.0, 3, 60.0),       # ignored everywhere
                     label(0, 0.0, 0, 24.99),      # ignored everywhere
                     label(3, 0.0, 0, 60.0),       # Van: ignored for Car, absent otherwise
                     label(4, 0.0, 0, 60.0),       # Person_sitting: ignored for Pedestrian
                     label(5, -1, -1, 60.0),       # DontCare
                     label(6, 0.0, 0, 60.0),       # anything else
                     label(1, 0.0, 0, 60.0)])
    assert chk.gt_flags(rows, 0, 0).tolist() == [0, 1, 1, 1, 1, 1, 1, 1, -1, 2, -1, -1]
    assert chk.gt_flags(rows, 0, 1).tolist() == [0, 0, 0, 1, 1, 1, 1, 1, -1, 2, -1, -1]
    assert chk.gt_flags(rows, 0, 2).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, -1, 2, -1, -1]
    assert chk.gt_flags(rows, 1, 0).tolist() == [-1] * 7 + [-1, 1, 2, -1, 0]
    assert chk.gt_flags(rows, 2, 2).tolist() == [-1] * 7 + [-1, -1, 2, -1, -1]
    dets = np.array([label(0, -1, -1, 40.0), label(0, -1, -1, 39.99), label(0, -1, -1, 25.0), label(0, -1, -1, 24.99), label(2, -1, -1, 60.0)])
    assert chk.det_flags(dets, 0, 0).tolist() == [0, 1, 1, 1, -1]
    assert chk.det_flags(dets, 0, 1).tolist() == [0, 0, 0, 1, -1]
    assert chk.det_flags(dets, 2, 2).tolist() == [-1, -1, -1, -1, 0]


def test_matching_rules_on_a_frame_worked_by_hand():
    """One Car label (counted at every difficulty) and three Car detections on top of it: a flat one (2-D height 20: flag 1) in front, a good
    one with score 0.5, a better-placed one with score 0.9; a second label nobody finds; a DontCare region over a fourth detection.
    Mode 1 takes the highest score (0.9).  Mode 2 at t = 0: the flat detection is the candidate until the first flag-0 one replaces it,
    then the larger overlap wins: tp 1, the other good one is a false positive, the flat one is not counted (flag 1), the fourth is taken
    out by the DontCare row in the image metric only (in the ground metric a DontCare row overlaps nothing); fn 1.  At t = 0.6 only the 0.9
    detection and the fourth (0.7) are scanned."""
    a = chk.box(0, 10, 4, 2, 0, h=2, cy=1, rect=(100, 100, 180, 160), type=0)
    far = chk.box(30, 40, 4, 2, 0, h=2, cy=1, rect=(600, 100, 680, 160), type=0)
    gt = np.array([a, far, chk.dontcare_row(300, 100, 428, 164)])
    flat, good, better, fp4 = a.copy(), a.copy(), a.copy(), chk.box(-20, 30, 4, 2, 0, h=2, cy=1, rect=(316, 104, 352, 152), type=0, score=0.7)
    flat[7], flat[15] = 120.0, 0.95
    flat[4:8] = (100, 100, 180, 120)
    good[11], good[15] = 0.5, 0.5           # ground overlap 3.5*2 / (16 - 7) = 7/9
    good[4:8] = (104, 100, 184, 160)        # image overlap 76*60 / (2*4800 - 4560)
    better[11], better[15] = 0.25, 0.9      # 3.75*2 / (16 - 7.5)
    better[4:8] = (102, 100, 182, 160)
    det = np.array([flat, good, better, fp4])
    ov = chk.overlap_matrices(det, gt, -1, dontcare_first=True)
    assert ov[1][1, 0] == 7 / 9 and ov[1][2, 0] == 7.5 / 8.5 and ov[0][3, 2] == 1.0
    gf, df = chk.gt_flags(gt, 0, 1), chk.det_flags(det, 0, 1)
    assert gf.tolist() == [0, 0, 2] and df.tolist() == [1, 0, 0, 0]
    scores, tp, fn = chk.first_mode(ov[1], df, gf, det[:, 15], 0.7)
    # the flat detection has the highest score (0.95) and is taken in mode 1: the label is then neither a tp nor a fn
    assert scores.tolist() == [] and (tp, fn) == (0, 1)
    flat[15] = 0.2
    det = np.array([flat, good, better, fp4])
    scores, tp, fn = chk.first_mode(ov[1], df, gf, det[:, 15], 0.7)
    assert scores.tolist() == [0.9] and (tp, fn) == (1, 1)
    st = chk.new_stats()
    tp, fp, fn = chk.second_mode(ov[1], df, gf, det[:, 15], 0.7, [0.0, 0.6], st)
    # ground metric: the DontCare row overlaps nothing, so the fourth detection (score 0.7) stays a false positive at both thresholds
    assert tp.tolist() == [1, 1] and fp.tolist() == [2, 1] and fn.tolist() == [1, 1]
    assert st["replaced_ignored"] >= 1
    st = chk.new_stats()
    tp, fp, fn = chk.second_mode(ov[0], df, gf, det[:, 15], 0.7, [0.0, 0.6], st)
    # image metric: flat (IoU 1/3) takes no part, `better` (IoU 4680/4920) wins, `good` is a fp, the fourth is removed by the DontCare row
    assert tp.tolist() == [1, 1] and fp.tolist() == [1, 0] and fn.tolist() == [1, 1]
    assert st["dontcare_removed"] == 2       # once per threshold


def test_abi_is_declared_and_bound(pcp):
    L = pcp._lib
    lib = L.lib()
    for n in ("pcr_kitti_eval_default_params", "pcr_kitti_box_overlap", "pcr_kitti_eval_overlaps", "pcr_kitti_eval_match", "pcr_kitti_eval"):
        assert n in L.SIGNATURES and hasattr(lib, n)
    p = L.KittiEvalParams()
    lib.pcr_kitti_eval_default_params(C.byref(p))
    assert [[p.min_overlap[m][c] for c in range(3)] for m in range(3)] == chk.MIN_OVERLAP.tolist()
    assert C.sizeof(L.KittiEvalCell) == 8 * (2 + 6 * 41 + 2) and C.sizeof(L.KittiEvalResult) == 27 * C.sizeof(L.KittiEvalCell)
    assert (L.PCR_KITTI_EVAL_MAX_DET, L.PCR_KITTI_EVAL_MAX_GT, L.PCR_KITTI_EVAL_SAMPLES) == (chk.MAX_DET, chk.MAX_GT, chk.N_SAMPLES)
    z = np.zeros(1, dtype=np.int64)
    res = L.KittiEvalResult()
    assert lib.pcr_kitti_eval(None, None, L.lptr(z), None, L.lptr(z), 0, C.byref(p), C.byref(res), None) == L.PCR_E_INVALID
    assert lib.pcr_kitti_eval_overlaps(None, None, L.lptr(z), None, L.lptr(z), 0, -1, None, None, None, None) == L.PCR_E_INVALID


def test_readers_round_trip_files_and_the_detectors_dataframe(pcp, tmp_path):
    import pandas as pd

    ke = pcp.kitti_eval
    names = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "DontCare", 6: "Tram"}
    gts, dets = chk.make_frames(3, 2, 8, 10)
    gt, det = np.round(gts[0], 2), np.round(dets[0], 2)
    (tmp_path / "gt").mkdir()
    with open(tmp_path / "gt" / "000000.txt", "wt") as f:
        for r in gt:
            f.write(" ".join([names[int(r[0])]] + [f"{v:.2f}" for v in r[1:15]]) + "\n")
    with open(tmp_path / "000000.txt", "wt") as f:
        for r in det:
            f.write(" ".join([names[int(r[0])]] + [f"{v:.2f}" for v in r[1:16]]) + "\n")
    back = ke.read_label_file(str(tmp_path / "gt" / "000000.txt"))
    assert back.shape == gt.shape and np.array_equal(back[:, :15], gt[:, :15]) and not back[:, 15].any()
    assert np.array_equal(ke.read_label_file(str(tmp_path / "000000.txt")), det)
    listed, frames = ke.read_label_dir(str(tmp_path / "gt"))
    assert listed == ["000000.txt"] and np.array_equal(frames[0], back)
    with pytest.raises(FileNotFoundError):
        ke.read_label_dir(str(tmp_path / "gt"), ["000001.txt"])
    # the frame to_kitti_eval_format returns: type names, numbers as '.2f' strings, truncated / occluded / alpha as integers
    label = {k: [f"{v:.2f}" for v in det[:, i]] for i, k in enumerate(chk.COLUMNS) if k not in ("type", "truncated", "occluded", "alpha")}
    label["type"] = [names[int(t)] for t in det[:, 0]]
    df = pd.DataFrame.from_dict(label)
    df["truncated"], df["occluded"], df["alpha"] = -1, -1, -10
    df = df[pcp.detection.KITTI_COLUMNS]
    got = ke.frames_from([df, det, det[:, :15], [["Car"] + [0.0] * 14]])
    assert np.array_equal(got[0], det) and np.array_equal(got[1], det)
    assert np.array_equal(got[2][:, :15], det[:, :15]) and not got[2][:, 15].any()
    assert got[3].shape == (1, 16) and got[3][0, 0] == 0.0
    assert pcp.frames_from is ke.frames_from and pcp.evaluate_object_3d_offline is ke.evaluate_object_3d_offline


def test_compute_entry_points_fail_without_a_device(pcp):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    gts, dets = chk.make_frames(1, 1, 4, 4)
    with pytest.raises(RuntimeError):
        pcp.kitti_eval.evaluate(gts, dets)
    with pytest.raises(RuntimeError):
        pcp.kitti_eval.box_overlaps(dets[0], gts[0])
