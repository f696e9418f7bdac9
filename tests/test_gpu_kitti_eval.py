"""KITTI evaluation on the device (include/pcr.h, "KITTI evaluation") against the restatement of tests/kitti_eval_checks.py: the overlap
matrices within a derived bound (the dyadic special pairs to the bit), the staged matching as equal integers and equal score multisets
on frames the restatement itself certifies as uncontested, the edge cases, the caps, and the whole evaluation to the bit."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import kitti_eval_checks as chk

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def cells_equal(got, want):
    """The nested result of kitti_eval.evaluate against the restatement's, every field to the bit."""
    for c in chk.CLASSES:
        for m in chk.METRICS:
            for d in chk.DIFFICULTIES:
                g, w = got[c][m][d], want[c][m][d]
                for key in ("n_gt", "n_thresholds"):
                    assert g[key] == w[key], (c, m, d, key, g[key], w[key])
                for key in ("thresholds", "tp", "fp", "fn", "precision", "recall"):
                    assert same_bits(np.asarray(g[key]), np.asarray(w[key])), (c, m, d, key, g[key], w[key])
                for key in ("ap11", "ap40"):
                    assert same_bits(np.float64(g[key]), np.float64(w[key])), (c, m, d, key, g[key], w[key])


def raw_eval(pcp, ctx, gts, dets):
    """pcr_kitti_eval itself -> (status, the result struct's bytes); the struct starts out filled, so an untouched one shows."""
    L = pcp._lib
    det, det_first = chk.ragged(dets)
    gt, gt_first = chk.ragged(gts)
    p = L.KittiEvalParams()
    L.lib().pcr_kitti_eval_default_params(C.byref(p))
    res = L.KittiEvalResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    rc = L.lib().pcr_kitti_eval(ctx.handle, L.dptr(det) if det.size else None, L.lptr(det_first), L.dptr(gt) if gt.size else None, L.lptr(gt_first), len(gts),
                                C.byref(p), C.byref(res), None)
    return rc, bytes(res)


# ------------------------------------------------------------------ overlaps
@pytest.fixture(scope="module")
def overlap_frames():
    rng = np.random.default_rng(11)
    gt, det = chk.make_frame(rng, 24, 40)
    assert gt.shape == (24, 16) and det.shape == (40, 16)
    specials = chk.special_pairs()
    gts, dets = [gt] + [b.reshape(1, 16) for _, _, b, _ in specials], [det] + [a.reshape(1, 16) for _, a, _, _ in specials]
    want = {c: [chk.overlap_matrices(d, g, c) for g, d in zip(gts, dets)] for c in (-1, 0, 1)}
    return gts, dets, specials, want


def test_overlap_matrices_within_the_derived_bound_and_special_pairs_to_the_bit(pcp, ctx, overlap_frames):
    """Bound on |delta overlap| for the ground and 3-D metrics, from the frame itself.  Let R be the largest magnitude of a vertex
    coordinate relative to the first centre over the pairs whose rectangles can meet (centre distance + both half diagonals), M the
    largest absolute centre coordinate, P the largest rectangle perimeter, U the smallest rectangle area, eps = 2^-53.
      * a vertex coordinate goes through at most 16 roundings at magnitude <= R (corner: 4; each of at most two cuts that create it:
        6), and the centre difference -- taken once on the device, through a midpoint in the restatement -- adds 3 roundings at
        magnitude M: a vertex is displaced by at most eps*(16 R + 3 M); cos / sin differ by an ulp between the C library and NumPy at
        most, which moves a corner by eps*R, inside the 16;
      * displacing every vertex of a convex polygon by delta changes its area by at most perimeter*delta <= P*delta;
      * the shoelace sum has at most 8 terms of magnitude <= 2 R^2 with 3 roundings each and 8 additions: 100 eps R^2.
    So either side is within dA = eps*(P*(16 R + 3 M) + 100 R^2) of the true area, the two sides within 2 dA of each other.  The overlap
    A/(S - A) has derivative S/(S - A)^2 <= 2/U' with U' = S - A >= the larger rectangle >= U, so |delta| <= 4 dA/U, plus 8 eps for the
    last operations.  In 3-D the common height hh <= h of either box and the union volume >= area*h of the larger: the same bound.
    For this frame that is a few 1e-11; what is observed is printed, and is expected near 1e-15.  The image metric is the same five
    operations on both sides: 8 eps.  The special pairs (dyadic extents, ry = 0) are exact on both sides: equal to the bit."""
    gts, dets, specials, want = overlap_frames
    ke = pcp.kitti_eval
    det, gt = dets[0], gts[0]
    diag = lambda r: 0.5 * np.hypot(r[:, 9], r[:, 10])   # noqa: E731
    real = gt[:, 9] > 0
    dist = np.hypot(det[:, None, 11] - gt[None, real, 11], det[:, None, 13] - gt[None, real, 13])
    reach = diag(det)[:, None] + diag(gt[real])[None, :]
    meet = dist <= reach
    R = float((dist + reach)[meet].max())
    M = float(max(np.abs(det[:, [11, 13]]).max(), np.abs(gt[real][:, [11, 13]]).max()))
    P = float(2 * max((det[:, 9] + det[:, 10]).max(), (gt[real, 9] + gt[real, 10]).max()))
    U = float(min((det[:, 9] * det[:, 10]).min(), (gt[real, 9] * gt[real, 10]).min()))
    bound = 4 * EPS * (P * (16 * R + 3 * M) + 100 * R * R) / U + 8 * EPS
    assert bound < 1e-9
    for criterion in (-1, 0, 1):
        mats, pair_first = ke._overlaps(dets, gts, criterion, ctx)
        assert pair_first.tolist() == [0] + list(np.cumsum([len(d) * len(g) for d, g in zip(dets, gts)]))
        got = [m[:960].reshape(40, 24) for m in mats]
        ref = want[criterion][0]
        err = [float(np.abs(got[m] - ref[m]).max()) for m in range(3)]
        print(f"criterion {criterion}: max |delta| image {err[0]:.3g} ground {err[1]:.3g} 3-D {err[2]:.3g}; bound {bound:.3g}; "
              f"R {R:.3g} M {M:.3g} P {P:.3g} U {U:.3g}; overlapping pairs {int((ref[1] > 0).sum())}")
        assert (ref[1] > 0).sum() >= 20 and (ref[2] > 0).sum() >= 10 and (ref[0] > 0).sum() >= 20
        assert err[0] <= 8 * EPS and err[1] <= bound and err[2] <= bound
        assert np.array_equal(got[1] > 0, ref[1] > 0) and np.array_equal(got[2] > 0, ref[2] > 0)
        for i, (name, a, b, _) in enumerate(specials):
            for m in range(3):
                assert same_bits(mats[m][pair_first[i + 1]], want[criterion][i + 1][m][0, 0]), (name, m, criterion)
                assert same_bits(np.float64(ke.box_overlap(a, b, m, criterion)), mats[m][pair_first[i + 1]]), (name, m, criterion)
    one = ke.box_overlaps(det, gt, -1, ctx)
    mats, _ = ke._overlaps(dets, gts, -1, ctx)
    for m, name in enumerate(chk.METRICS):
        assert same_bits(one[name], mats[m][:960].reshape(40, 24))
        # the host function is the kernel's source: the same bits on every pair
        host = np.array([[ke.box_overlap(a, b, m, -1) for b in gt] for a in det])
        assert same_bits(host, one[name])


# ------------------------------------------------------------------ staged matching
MATCH_SEED = 4


@pytest.fixture(scope="module")
def match_frames():
    gts, dets = chk.make_frames(MATCH_SEED, 24, 12, 12)
    assert max(len(g) for g in gts) <= 24 and max(len(d) for d in dets) <= 24
    overlaps = chk.frame_overlaps(gts, dets)
    stats = chk.new_stats()
    want = chk.evaluate(gts, dets, overlaps=overlaps, stats=stats)
    return gts, dets, overlaps, stats, want


def test_staged_matching_equals_the_restatement_in_every_combination(pcp, ctx, match_frames):
    """Asserted from the restatement alone, before the device is asked: no decision of these frames is contested (every overlap a matching
    reads is further than 1e-9 from MIN_OVERLAP, competing overlaps are further than 1e-9 apart -- the overlaps themselves agree to
    some 1e-15), and the frames take every branch of the matching."""
    gts, dets, overlaps, stats, want = match_frames
    assert stats["closest"] > 1e-9 and stats["gap"] > 1e-9, stats
    for key in ("ignored_assignments", "replaced_ignored", "dontcare_removed", "fn", "score_ties"):
        assert stats[key] >= 1, (key, stats)
    ke = pcp.kitti_eval
    for c, cn in enumerate(chk.CLASSES):
        for d, dn in enumerate(chk.DIFFICULTIES):
            for m, mn in enumerate(chk.METRICS):
                w_scores, w_tp, w_fn, w_n_gt = chk.match_all(gts, dets, c, d, m, 1, overlaps=overlaps)
                scores, tp, fn, n_gt = ke.match(gts, dets, c, d, m, 1, ctx=ctx)
                assert same_bits(scores, w_scores) and (tp, fn, n_gt) == (w_tp, w_fn, w_n_gt), (cn, dn, mn)
                cell = want[cn][mn][dn]
                thr = cell["thresholds"][:cell["n_thresholds"]]
                tp, fp, fn = ke.match(gts, dets, c, d, m, 2, thr, ctx=ctx)
                K = len(thr)
                assert np.array_equal(tp, cell["tp"][:K]) and np.array_equal(fp, cell["fp"][:K]) and np.array_equal(fn, cell["fn"][:K]), (cn, dn, mn)
    assert sum(want[c]["ground"]["hard"]["n_thresholds"] for c in chk.CLASSES) >= 10


# ------------------------------------------------------------------ edge cases
def _car(cx, score=0.0, h2d=60.0, trunc=0.0, occ=0.0, type=0.0, left=0.0):
    r = chk.box(cx, 10, 4, 2, 0, h=2, cy=1, rect=(left, 100, left + 80, 100 + h2d), type=type, score=score)
    r[1], r[2] = trunc, occ
    return r


def test_edge_case_frames_in_one_call(pcp, ctx):
    """Twelve frames: no detections; no labels; only don't-care rows; every label ignored; every detection under the height limit; empty
    altogether; and ordinary ones.  No Cyclist anywhere: n_gt = 0 gives no thresholds and AP 0."""
    e = np.zeros((0, 16))
    car, det = _car(0), _car(0.25, score=0.8)
    gts = [np.array([car]), e, np.array([chk.dontcare_row(0, 100, 128, 164)]), np.array([_car(0, occ=3.0), _car(20, trunc=0.9, left=300)]),
           np.array([car]), e, np.array([car, _car(20, left=300)]), np.array([_car(0, type=1.0)]), np.array([_car(0, type=3.0)]), np.array([car]),
           np.array([chk.dontcare_row(0, 100, 128, 164), car]), np.array([car])]
    dets = [e, np.array([det]), np.array([_car(5, score=0.5, left=16)]), np.array([det, _car(20.25, score=0.6, left=300)]),
            np.array([_car(0.25, score=0.7, h2d=20.0)]), e, np.array([det, _car(20.25, score=0.3, left=300)]), np.array([_car(0.25, score=0.9, type=1.0)]),
            np.array([det]), np.array([_car(0.25, score=0.4), _car(0.5, score=0.4, left=2.0)]), np.array([_car(50, score=0.2, left=16, h2d=60.0)]), np.array([det])]
    assert len(gts) == len(dets) == 12
    stats = chk.new_stats()
    want = chk.evaluate(gts, dets, stats=stats)
    assert stats["closest"] > 1e-9 and stats["gap"] > 1e-9
    got = pcp.kitti_eval.evaluate(gts, dets, ctx=ctx)
    cells_equal(got, want)
    for m in chk.METRICS:
        for d in chk.DIFFICULTIES:
            cyc = got["cyclist"][m][d]
            assert cyc["n_gt"] == 0 and cyc["n_thresholds"] == 0 and cyc["ap11"] == 0.0 and cyc["ap40"] == 0.0 and not cyc["precision"].any()
    assert got["car"]["ground"]["easy"]["n_gt"] == 7 and got["pedestrian"]["3d"]["hard"]["n_gt"] == 1
    # all frames empty, and no frame at all
    for frames in ([e, e], []):
        rc, raw = raw_eval(pcp, ctx, frames, frames)
        assert rc == 0 and not any(raw)


def test_the_overlap_comparison_is_strict(pcp, ctx):
    """Dyadic axis-aligned Pedestrian boxes whose overlap is exactly 0.5 in every metric: a 4 x 2 label (area 8) and a 2 x 2 detection inside
    it (area 4): 4 / (8 + 4 - 4) on the ground, equal heights in 3-D, rectangles 80 x 60 and 40 x 60 in the image.  Exactly 0.5 is NOT
    matched (o > MIN_OVERLAP is strict).  The next representable larger overlap is matched: with min_overlap = the predecessor of 0.5
    the same pair is a true positive (one threshold, precision 1 at k = 0 only: ap11 = 100/11)."""
    gt = chk.box(0, 10, 4, 2, 0, h=2, cy=1, rect=(0, 100, 80, 160), type=1.0)
    det = chk.box(1, 10, 2, 2, 0, h=2, cy=1, rect=(40, 100, 80, 160), type=1.0, score=0.9)
    ke = pcp.kitti_eval
    ov = ke.box_overlaps([det], [gt], -1, ctx)
    assert all(ov[m][0, 0] == 0.5 for m in chk.METRICS)
    below = np.nextafter(0.5, 0.0)
    for mo, matched in ((None, False), (np.full((3, 3), below), True), (np.full((3, 3), np.nextafter(0.5, 1.0)), False)):
        got = ke.evaluate([gt.reshape(1, 16)], [det.reshape(1, 16)], min_overlap=mo, ctx=ctx)
        want = chk.evaluate([gt.reshape(1, 16)], [det.reshape(1, 16)], min_overlap=mo)
        cells_equal(got, want)
        for m in chk.METRICS:
            cell = got["pedestrian"][m]["easy"]
            assert cell["n_gt"] == 1
            assert (cell["n_thresholds"], int(cell["tp"][0]), cell["ap11"]) == ((1, 1, 100.0 * (1.0 / 11.0)) if matched else (0, 0, 0.0)), (m, matched, cell)


@pytest.fixture(scope="module")
def cap_frames():
    rng = np.random.default_rng(21)
    gt, det = chk.make_frame(rng, chk.MAX_GT, chk.MAX_DET, spread=2.0)
    small_gt, small_det = chk.make_frame(rng, 10, 15)
    return [small_gt, gt], [small_det, det]


def test_a_frame_at_the_caps_runs_the_global_memory_path(pcp, ctx, cap_frames):
    """256 x 128 = 32 768 pairs, beyond the 2 048 the mode-2 kernel stages in LDS: that frame's overlaps are read from global memory,
    next to a small frame that is staged; the fourth word of the assigned set is in use (detection rows 192..255)."""
    gts, dets = cap_frames
    assert gts[1].shape == (chk.MAX_GT, 16) and dets[1].shape == (chk.MAX_DET, 16)
    stats = chk.new_stats()
    want = chk.evaluate(gts, dets, stats=stats)
    assert stats["closest"] > 1e-9 and stats["gap"] > 1e-9, stats
    assert want["car"]["ground"]["hard"]["n_thresholds"] >= 5
    cells_equal(pcp.kitti_eval.evaluate(gts, dets, ctx=ctx), want)


def test_a_frame_beyond_a_cap_is_refused_with_the_outputs_untouched(pcp, ctx, cap_frames):
    L = pcp._lib
    gts, dets = cap_frames
    before = ctx.arena_live()
    for big_g, big_d in ((gts[1], np.vstack([dets[1], dets[1][:1]])), (np.vstack([gts[1], gts[1][:1]]), dets[1])):
        rc, raw = raw_eval(pcp, ctx, [gts[0], big_g], [dets[0], big_d])
        assert rc == L.PCR_E_UNSUPPORTED and raw == b"\x5a" * len(raw)
        det, det_first = chk.ragged([dets[0], big_d])
        gt, gt_first = chk.ragged([gts[0], big_g])
        out = np.full(int(det_first[-1] * gt_first[-1]), 7.0)
        pf = np.full(3, -5, dtype=np.int64)
        rc = L.lib().pcr_kitti_eval_overlaps(ctx.handle, L.dptr(det), L.lptr(det_first), L.dptr(gt), L.lptr(gt_first), 2, -1, L.dptr(out), None, None, L.lptr(pf))
        assert rc == L.PCR_E_UNSUPPORTED and (out == 7.0).all() and (pf == -5).all()
    assert ctx.arena_live() == before


# ------------------------------------------------------------------ the whole evaluation
def test_whole_evaluation_to_the_bit_repeatable_and_independent_of_frame_order(pcp, ctx, match_frames):
    gts, dets, overlaps, stats, want = match_frames
    ke = pcp.kitti_eval
    before = ctx.arena_live()
    cells_equal(ke.evaluate(gts, dets, ctx=ctx), want)
    rc1, raw1 = raw_eval(pcp, ctx, gts, dets)
    rc2, raw2 = raw_eval(pcp, ctx, gts, dets)
    assert rc1 == rc2 == 0 and raw1 == raw2
    order = np.random.default_rng(2).permutation(len(gts))
    rc3, raw3 = raw_eval(pcp, ctx, [gts[i] for i in order], [dets[i] for i in order])
    assert rc3 == 0 and raw3 == raw1
    assert ctx.arena_live() == before
    # the looser table is a parameter
    loose = np.array([[0.5, 0.25, 0.25]] * 3)
    cells_equal(ke.evaluate(gts, dets, min_overlap=loose, ctx=ctx), chk.evaluate(gts, dets, min_overlap=loose, overlaps=overlaps))
    stage = np.zeros(3)
    ke._evaluate_raw(gts, dets, ctx=ctx, stage_ms=stage)
    assert (stage >= 0).all() and stage.sum() > 0


def test_python_end_to_end_through_label_files(pcp, ctx, tmp_path, capsys):
    """Label files with two decimals (what the detector writes) -> evaluate_object_3d_offline: the printed lines and the stats files, parsed
    back, equal the restatement on the rows as the files hold them; a DataFrame of to_kitti_eval_format's shape is accepted as a frame."""
    import pandas as pd

    ke = pcp.kitti_eval
    names = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "DontCare", 6: "Tram"}
    gts, dets = chk.make_frames(9, 12, 16, 18)
    gts, dets = [np.round(g, 2) for g in gts], [np.round(d, 2) for d in dets]
    gts = [g[g[:, 0] != 2.0] for g in gts]                    # no Cyclist label: the class is skipped in print and files
    for g in gts:
        g[:, 15] = 0.0
    os.makedirs(tmp_path / "gt")
    os.makedirs(tmp_path / "res" / "data")
    for i, (g, d) in enumerate(zip(gts, dets)):
        with open(tmp_path / "gt" / f"{i:06d}.txt", "wt") as f:
            for r in g:
                f.write(" ".join([names[int(r[0])]] + [f"{v:.2f}" for v in r[1:15]]) + "\n")
        with open(tmp_path / "res" / "data" / f"{i:06d}.txt", "wt") as f:
            for r in d:
                f.write(" ".join([names[int(r[0])]] + [f"{v:.2f}" for v in r[1:16]]) + "\n")
    with open(tmp_path / "gt" / "000099.txt", "wt") as f:      # a ground-truth frame without results is not evaluated
        f.write("Car 0.00 0 -10 0 0 10 10 1 1 1 0 0 10 0\n")
    stats = chk.new_stats()
    want = chk.evaluate(gts, dets, stats=stats)
    assert stats["closest"] > 1e-9 and stats["gap"] > 1e-9, stats
    capsys.readouterr()
    got = ke.evaluate_object_3d_offline(str(tmp_path / "gt"), str(tmp_path / "res"), ctx=ctx)
    printed = capsys.readouterr().out.strip().split("\n")
    cells_equal(got, want)
    lines = []
    present = [cn for cn in chk.CLASSES if any(want[cn][mn][dn]["n_gt"] for mn in chk.METRICS for dn in chk.DIFFICULTIES)]
    assert present == ["car", "pedestrian"]
    for cn in present:
        for mn, suffix in (("image", ""), ("ground", "_ground"), ("3d", "_3d")):
            tag = f"{cn}_detection{suffix}"
            lines.append(f"{tag} AP: " + " ".join(f"{want[cn][mn][dn]['ap11']:f}" for dn in chk.DIFFICULTIES))
            rows = open(tmp_path / "res" / f"stats_{tag}.txt").read().strip().split("\n")
            assert len(rows) == 3
            for row, dn in zip(rows, chk.DIFFICULTIES):
                assert row.split() == [f"{v:f}" for v in want[cn][mn][dn]["precision"]]
    assert printed == lines
    assert not any(n.startswith("stats_cyclist") for n in os.listdir(tmp_path / "res"))
    os.remove(tmp_path / "gt" / "000003.txt")
    with pytest.raises(FileNotFoundError):
        ke.evaluate_object_3d_offline(str(tmp_path / "gt"), str(tmp_path / "res"), ctx=ctx, write=False)
    # to_kitti_eval_format's frame: type names, '.2f' strings, truncated = occluded = -1, alpha = -10
    frames = []
    for d in dets:
        label = {k: [f"{v:.2f}" for v in d[:, i]] for i, k in enumerate(chk.COLUMNS) if k not in ("type", "truncated", "occluded", "alpha")}
        label["type"] = [names[int(t)] for t in d[:, 0]]
        df = pd.DataFrame.from_dict(label)
        df["truncated"], df["occluded"], df["alpha"] = -1, -1, -10
        frames.append(df[pcp.detection.KITTI_COLUMNS])
    cells_equal(ke.evaluate(gts, frames, ctx=ctx), want)
