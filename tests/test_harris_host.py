"""CPU: the NumPy restatement of the PCL-keypoint rules (tests/harris_checks.py) on constructed cases whose answer is known, and the
module's call surface against the reference wrapper's (PCLKeypoints/src/keypoints.cpp:243-291)."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import harris_checks as hc
from tests.conftest import ROOT


def test_plane_without_noise_has_no_response():
    """All normals equal: C = n n^T, trace 1, det 0 -> 0.04 + 0 - 0.04 = 0 up to rounding."""
    g = np.arange(12) * 0.1
    x, y = [m.ravel() for m in np.meshgrid(g, g, indexing="ij")]
    R = np.linalg.qr(np.random.default_rng(1).normal(size=(3, 3)))[0]
    pts = np.stack([x, y, np.zeros_like(x)], axis=1) @ R.T + np.array([0.3, -1.0, 2.0])
    res = hc.harris3d(pts, 0.25, 0.001, nms=False)
    assert np.isfinite(res["normals"]).all()
    assert np.abs(res["response"]).max() < 1e-12


def test_corner_of_three_faces_has_the_largest_kept_response():
    pts, corner = hc.corner_cloud()
    assert pts.shape == (3 * 15 * 15, 3)
    res = hc.harris3d(pts, 0.25, 0.001, nms=True)
    rows = res["rows"]
    assert len(rows) >= 1
    nearest = rows[np.argmin(np.linalg.norm(pts[rows] - corner, axis=1))]
    assert nearest == rows[np.argmax(res["response"][rows])]
    assert np.linalg.norm(pts[nearest] - corner) < 0.25
    # kept rows are candidates that nothing in their ball beats, in ascending row
    assert (res["response"][rows] >= 0.001).all() and (np.diff(rows) > 0).all()
    nb = hc.neighbours(pts, 0.25)
    for i in rows:
        assert res["response"][nb[i]].max() <= res["response"][i]


def test_rows_at_exactly_the_radius_are_neighbours():
    g = np.arange(5, dtype=np.float64)
    pts = np.stack([m.ravel() for m in np.meshgrid(g, g, g, indexing="ij")], axis=1)
    counts = np.array([len(j) for j in hc.neighbours(pts, 1.0)])
    on_face = ((pts == 0) | (pts == 4)).sum(axis=1)   # 0 interior, 1 face, 2 edge, 3 corner
    assert np.array_equal(counts, 7 - on_face)
    assert sorted(set(counts)) == [4, 5, 6, 7]


def test_refine_lands_on_the_intersection_of_the_planes():
    pts, _ = hc.corner_cloud(jitter=0.0)
    normals = np.repeat(np.eye(3), 15 * 15, axis=0)        # exact: face f is the plane (coordinate f) = 0
    shift = np.array([1.5, -2.0, 0.75])
    start = np.array([[0.1, 0.1, 0.0], [0.0, 0.2, 0.1]]) + shift
    refined, rounds = hc.refine(pts + shift, normals, 0.35, start)
    assert np.abs(refined - shift).max() < 1e-9
    assert (rounds >= 1).all() and (rounds <= 5).all()
    # a corner whose ball holds one face only: A is singular, the corner stays
    far = np.array([[0.0, 1.0, 1.0]]) + shift
    kept, r1 = hc.refine(pts + shift, normals, 0.25, far)
    assert np.array_equal(kept, far) and r1[0] == 1


def test_pcl_rule_iss_on_a_plane_and_in_a_volume():
    """A plane's scatter has e3 = 0 up to rounding: no row passes e3/e2 < gamma with a positive e3 that matters; a jittered volume has keypoints."""
    rng = np.random.default_rng(4)
    vol = rng.uniform(0, 1, (600, 3))
    res = hc.iss_pcl(vol, 0.3, 0.2, 0.8, 0.8, 5)
    assert len(res["rows"]) > 0 and res["candidates"][res["rows"]].all()
    assert (res["score"][res["rows"]] > 0).all()
    for i in res["rows"]:
        assert res["margin"][i] >= 0


WRAPPER = {   # keypoints.cpp:243-291: argument names and defaults
    "keypointIss": [("points", None), ("iss_salient_radius", 3.0), ("iss_non_max_radius", 2.0), ("iss_gamma_21", 0.975), ("iss_gamma_32", 0.975),
                    ("iss_min_neighbors", 5), ("threads", 0)],
    "keypointHarris3D": [("points", None), ("radius", 0.5), ("nms_threshold", 0.001), ("threads", 0), ("is_nms", False), ("is_refine", False)],
    "keypointHarris6D": [("points", None), ("radius", 0.5), ("nms_threshold", 0.001), ("threads", 0), ("is_nms", False), ("is_refine", False)],
    "keypointSift": [("points", None), ("min_scale", 0.1), ("n_octaves", 6), ("n_scales_per_octave", 10), ("min_contrast", 0.05)],
    "featureFPFH33": [("pointcloud", None), ("keypoints", None), ("compute_normal_k", 10), ("feature_radius", 1.0)],
    "featureFPFH33WithNormal": [("pointcloud", None), ("normals", None), ("keypoints", None), ("feature_radius", 1.0)],
    "featureSHOT352": [("pointcloud", None), ("keypoints", None), ("compute_normal_k", 10), ("feature_radius", 1.0)],
    "featureSHOT352WithNormal": [("pointcloud", None), ("normals", None), ("keypoints", None), ("feature_radius", 1.0)],
}


def test_module_signatures_and_defaults_equal_the_wrapper(pcp):
    mod = pcp.PCLKeypoint
    assert pcp.keypointHarris3D is mod.keypointHarris3D and pcp.keypointIss is mod.keypointIss
    for name, want in WRAPPER.items():
        params = [p for p in inspect.signature(getattr(mod, name)).parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD]
        got = [(p.name, None if p.default is p.empty else p.default) for p in params]
        assert got == want, name
        for (_, d), (_, w) in zip(got, want):
            assert type(d) is type(w), name
    for name, extras in (("keypointHarris3D", {"normals", "return_indices", "return_details", "ctx"}), ("keypointIss", {"return_indices", "return_details", "ctx"})):
        kw = {p.name for p in inspect.signature(getattr(mod, name)).parameters.values() if p.kind is p.KEYWORD_ONLY}
        assert kw == extras, name


def test_out_of_scope_entry_points_say_what_they_need(pcp):
    mod = pcp.PCLKeypoint
    pts = np.zeros((4, 3))
    for name, args, word in (("keypointHarris6D", (pts,), "colour"), ("keypointSift", (pts,), "scale space"), ("featureFPFH33", (pts, pts), "descriptor"),
                             ("featureFPFH33WithNormal", (pts, pts, pts), "descriptor"), ("featureSHOT352", (pts, pts), "descriptor"),
                             ("featureSHOT352WithNormal", (pts, pts, pts), "descriptor")):
        with pytest.raises(NotImplementedError) as e:
            getattr(mod, name)(*args)
        assert word in str(e.value), name


def test_abi_is_declared_bound_and_exported(pcp):
    L = pcp._lib
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for name in ("pcr_normals_radius", "pcr_harris3d", "pcr_iss_pcl", "pcr_harris_default_params"):
        assert re.search(r"PCR_API\s+\w+\s+" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    p = L.HarrisParams()
    lib.pcr_harris_default_params(p)
    assert (p.radius, p.threshold, p.nms, p.refine) == (0.5, 0.001, 0, 0)
    assert "parity with PCL's binary32 output is unpinned" in header
    # bad arguments are refused before any device work
    assert lib.pcr_harris3d(None, None, None, None, None, None, None, 0, None, None, None, None) == L.PCR_E_INVALID
    assert lib.pcr_iss_pcl(None, None, 1.0, 1.0, 0.9, 0.9, 5, None, None, None, 0, None) == L.PCR_E_INVALID
    assert lib.pcr_normals_radius(None, None, 1.0, None, None, None) == L.PCR_E_INVALID


def test_ransac_init_knows_the_harris_detector(pcp):
    sig = inspect.signature(pcp.ransac_init)
    assert sig.parameters["detector"].default == "voxel"
    assert "harris_radius" in sig.parameters and sig.parameters["harris_threshold"].default == 0.001
    assert "detector=\"harris\"" in pcp.ransac_init.__doc__
