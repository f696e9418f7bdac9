"""Records tests/golden/kitti_boxes.npz: what the reference's formulation gives for the planted scene of tests/kitti_boxes_checks.py.

The frame transforms are the reference's own functions (Final_Project/scripts/transform_coords_utils.py, imported by path from
--reference); the per-object fields of detect.py:113-163 around them -- pixel box, centre, np.cov + np.linalg.eig yaw, the rotation
into the object frame and its extents -- are restated here in NumPy, because detect.py itself imports Open3D.  Data only: points,
ids, the calibration, 11 numbers and their '.2f' strings per object with rows, and 64 (a, b, c) -> yaw triples straight from
np.linalg.eig, the exact cases b == 0 among them.  --check N also compares the direction rule of include/pcr.h with np.linalg.eig
on N random covariances and prints the branch mismatches and the worst scaled error.

    python scripts/make_kitti_boxes_golden.py --reference <reference checkout> [--check 50000]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import kitti_boxes_checks as chk  # noqa: E402

LDS_ROWS = 512   # PCR_KITTI_LDS_ROWS of include/pcr.h: the scene straddles it


def eig_yaw(H):
    """detect.py:47-54."""
    eigenvalues, eigenvectors = np.linalg.eig(H)
    idx_sort = eigenvalues.argsort()[::-1]
    eigenvectors = eigenvectors[:, idx_sort]
    return np.arctan2(-eigenvectors[0][1], eigenvectors[0][0])


def object_fields(ref, X_velo, param):
    """The 11 numbers of one label row in FIELDS order, computed the reference's way."""
    X_cam = ref.transform_to_cam(X_velo, param)
    X_pixel = ref.transform_to_pixel(X_cam, param)
    top_left, bottom_right = X_pixel.min(axis=0), X_pixel.max(axis=0)
    c_center = X_cam.mean(axis=0)
    X_cam_centered = X_cam - c_center
    orientation = eig_yaw(np.cov(X_cam_centered[:, [0, 2]], rowvar=False, bias=True))
    cos_ry, sin_ry = np.cos(-orientation), np.sin(-orientation)
    R_obj_to_cam = np.asarray([[cos_ry, 0.0, sin_ry], [0.0, 1.0, 0.0], [-sin_ry, 0.0, cos_ry]])
    X_obj = np.dot(R_obj_to_cam.T, X_cam_centered.T).T
    extent = X_obj.max(axis=0) - X_obj.min(axis=0)
    return [top_left[0], top_left[1], bottom_right[0], bottom_right[1], extent[1], extent[0], extent[2], c_center[0], c_center[1], c_center[2], orientation]


def covariance_triples(rng, n):
    """(n, 3) rows a, b, c of symmetric positive semi-definite 2 x 2 matrices: the exact cases first, then random spreads of every
    heading, some with |b| down to 1e-12 of sqrt(ac)."""
    rows = [(2.0, 0.0, 1.0), (1.0, 0.0, 2.0), (1.5, 0.0, 1.5), (0.0, 0.0, 0.0), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), (1.0, 0.5, 1.0), (1.0, -0.5, 1.0)]
    while len(rows) < n:
        l1, l2 = np.sort(rng.uniform(0.01, 4.0, size=2))[::-1]
        t = rng.uniform(-np.pi, np.pi)
        c, s = np.cos(t), np.sin(t)
        a, b, cc = l1 * c * c + l2 * s * s, (l1 - l2) * c * s, l1 * s * s + l2 * c * c
        if len(rows) % 8 == 0:
            b = np.sqrt(a * cc) * 10.0 ** rng.uniform(-12, -6) * rng.choice([-1.0, 1.0])
        rows.append((a, b, cc))
    return np.array(rows[:n], dtype=np.float64)


def check_rule(n, seed):
    rng = np.random.default_rng(seed)
    worst, mismatches = 0.0, 0
    for a, b, c in covariance_triples(rng, n):
        want = eig_yaw(np.array([[a, b], [b, c]]))
        cs, sn = chk.restated_direction(a, b, c)
        got = np.arctan2(sn, cs)
        gap = np.hypot(a - c, 2.0 * b)
        err = abs(got - want) * (gap / (a + c) if a + c > 0 and gap > 0 else 0.0)
        if abs(got - want) > 1e-6 and gap > 0:
            mismatches += 1
        else:
            worst = max(worst, err)
    print(f"direction rule against np.linalg.eig on {n} covariances: {mismatches} branch mismatches, worst scaled error {worst:.2e}")
    return mismatches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--check", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kitti_boxes.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("transform_coords_utils", os.path.join(a.reference, "Final_Project", "scripts", "transform_coords_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    if a.check and check_rule(a.check, seed=1):
        sys.exit("the direction rule does not reproduce np.linalg.eig here")

    points, ids, k = chk.planted_scene(LDS_ROWS)
    present = np.array([o for o in range(k) if (ids == o).any()], dtype=np.int32)
    fields = np.array([object_fields(ref, points[ids == o], chk.CALIB) for o in present])
    strings = np.array([[f"{x:.2f}" for x in row] for row in fields])
    abc = covariance_triples(np.random.default_rng(2), 64)
    yaw = np.array([eig_yaw(np.array([[r[0], r[1]], [r[1], r[2]]])) for r in abc])
    assert np.array_equal(points, points.astype(np.float32).astype(np.float64))
    np.savez_compressed(a.out, points=points.astype(np.float32), ids=ids.astype(np.int32), n_objects=np.int32(k), lds_rows=np.int32(LDS_ROWS),
                        P2=chk.CALIB["P2"], R0_rect=chk.CALIB["R0_rect"], Tr_velo_to_cam=chk.CALIB["Tr_velo_to_cam"], object_ids=present,
                        fields=fields, strings=strings, cov_abc=abc, cov_yaw=yaw)
    print(f"{a.out}: {len(points)} points, {len(present)} objects with rows, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
