"""CPU: the NumPy restatement of the PCL-rule FPFH33 rules (tests/pcl_fpfh_checks.py) on cases whose answer is known or can be had by a
literal double loop, and the call surface of the new entry points (pcr_normals_knn, pcr_fpfh_pcl; pcl_features.py) against the reference
wrapper's (PCLKeypoints/src/keypoints.cpp:272-281)."""
import inspect
import math
import os
import re

import numpy as np

from tests import pcl_fpfh_checks as pf
from tests.conftest import ROOT


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


# ------------------------------------------------------------------------------------------------ the call surface
def test_abi_is_declared_bound_and_exported(pcp):
    L = pcp._lib
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for name in ("pcr_normals_knn", "pcr_fpfh_pcl"):
        decl = re.search(r"PCR_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert len(L.SIGNATURES[name][1]) == len(params), name           # one bound argument per declared parameter
    assert len(L.SIGNATURES["pcr_normals_knn"][1]) == 6 and len(L.SIGNATURES["pcr_fpfh_pcl"][1]) == 9
    assert header.count("parity with PCL's binary32 output is unpinned") >= 2
    # bad arguments are refused before any device work (there is no device here)
    assert lib.pcr_normals_knn(None, None, 10, None, None, None) == L.PCR_E_INVALID
    assert lib.pcr_normals_knn(None, None, 17, None, None, None) == L.PCR_E_INVALID
    assert lib.pcr_fpfh_pcl(None, None, None, None, 0, 1.0, None, None, None) == L.PCR_E_INVALID
    assert lib.pcr_fpfh_pcl(None, None, None, None, 4, 1.0, None, None, None) == L.PCR_E_INVALID


WRAPPER = {   # keypoints.cpp:272-281: the shared parameters, their names and defaults
    "fpfh33": [("pointcloud", None), ("keypoints", None), ("compute_normal_k", 10), ("feature_radius", 1.0)],
    "fpfh33_with_normal": [("pointcloud", None), ("normals", None), ("keypoints", None), ("feature_radius", 1.0)],
}
KEYWORD_ONLY = {"fpfh33": {"viewpoint", "ctx", "return_info"}, "fpfh33_with_normal": {"ctx", "return_info"}}


def test_python_signatures_and_defaults_equal_the_wrapper(pcp):
    mod = pcp.pcl_features
    assert pcp.fpfh33 is mod.fpfh33 and pcp.fpfh33_with_normal is mod.fpfh33_with_normal and pcp.estimate_normals_knn is mod.estimate_normals_knn
    for name, want in WRAPPER.items():
        sig = inspect.signature(getattr(mod, name))
        params = [p for p in sig.parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD]
        got = [(p.name, None if p.default is p.empty else p.default) for p in params]
        assert got == want, name
        for (_, d), (_, w) in zip(got, want):
            assert type(d) is type(w), name
        assert {p.name for p in sig.parameters.values() if p.kind is p.KEYWORD_ONLY} == KEYWORD_ONLY[name], name
        # the wrapper's own names take the same shared parameters
        stub = [p.name for p in inspect.signature(getattr(pcp.PCLKeypoint, {"fpfh33": "featureFPFH33", "fpfh33_with_normal": "featureFPFH33WithNormal"}[name])).parameters.values()]
        assert stub == [n for n, _ in want], name
    sig = inspect.signature(mod.estimate_normals_knn)
    assert [(p.name, p.default) for p in sig.parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD][1:] == [("k", 10), ("viewpoint", (0.0, 0.0, 0.0))]
    assert {p.name for p in sig.parameters.values() if p.kind is p.KEYWORD_ONLY} == {"return_curvature", "ctx"}


# ------------------------------------------------------------------------------------------------ the rules
def test_plane_with_equal_normals_fills_one_bin_per_block():
    """Points in z = 0, all normals (0,0,1): a1 = a2 = 0 (no swap), v = d x n is a unit vector in the plane, f1 = v.n = 0,
    f0 = atan2((n x v).n, n.n) = atan2(0, 1) = 0, f2 = 0: bins floor(5.5) = 5 of each block -- 5, 16, 27 -- hold every pair."""
    rng = np.random.default_rng(2)
    pts = np.c_[rng.uniform(-1, 1, (200, 2)), np.zeros(200)]
    nrm = np.tile([[0.0, 0.0, 1.0]], (200, 1))
    s = pf.spfh(pts, nrm, 0.5)
    assert (s["counts"] >= 2).all()
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(s["hist"][:, [5, 16, 27]], np.repeat(s["counts"][:, None] - 1, 3, axis=1))
    assert np.abs(s["values"] - want).max() <= 100 * 2.0 ** -52      # c * (100 / c): one product of a rounded quotient
    kp = np.r_[pts[:20], [[0.01, 0.02, 0.3]]]                         # on the surface and off it
    f = pf.fpfh33(pts, nrm, kp, 0.5)
    assert (f["counts"] > 1).all()
    assert np.abs(f["values"] - want).max() <= 1e-12
    assert (f["values"][:, np.setdiff1d(np.arange(33), [5, 16, 27])] == 0.0).all()


def _literal(pts, nrm, kp, radius):
    """The rules as a per-pair double loop in Python floats."""
    n = len(pts)
    r2 = radius * radius

    def d2(a, b):
        dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return (dx * dx + dy * dy) + dz * dz

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    spfh = np.zeros((n, 33))
    K = np.zeros(n, dtype=np.int64)
    for i in range(n):
        hist = [0] * 33
        for j in range(n):
            if d2(pts[j], pts[i]) > r2:
                continue
            K[i] += 1
            if j == i or not (all(map(math.isfinite, nrm[i])) and all(map(math.isfinite, nrm[j]))):
                continue
            d = [pts[j][c] - pts[i][c] for c in range(3)]
            ln = math.sqrt(dot(d, d))
            if ln == 0.0:
                continue
            a1, a2 = dot(nrm[i], d) / ln, dot(nrm[j], d) / ln
            if abs(a1) < abs(a2):
                u, w2, d, f2 = nrm[j], nrm[i], [-c for c in d], -a2
            else:
                u, w2, f2 = nrm[i], nrm[j], a1
            v = cross(d, u)
            vn = math.sqrt(dot(v, v))
            if vn == 0.0:
                continue
            v = [c / vn for c in v]
            w = cross(u, v)
            f1 = dot(v, w2)
            f0 = math.atan2(dot(w, w2), dot(u, w2))
            for blk, x in enumerate((11.0 * (f0 + math.pi) / (2.0 * math.pi), 11.0 * (f1 + 1.0) * 0.5, 11.0 * (f2 + 1.0) * 0.5)):
                hist[11 * blk + min(max(int(math.floor(x)), 0), 10)] += 1
        if K[i] > 1:
            spfh[i] = [c * (100.0 / (K[i] - 1)) for c in hist]
    out = np.full((len(kp), 33), np.nan)
    counts = np.zeros(len(kp), dtype=np.int64)
    for t, x in enumerate(kp):
        if not all(map(math.isfinite, x)):
            continue
        F = [0.0] * 33
        for j in range(n):
            dd = d2(pts[j], x)
            if dd > r2:
                continue
            counts[t] += 1
            if dd != 0.0:
                for b in range(33):
                    F[b] += spfh[j][b] / dd
        if counts[t] == 0:
            continue
        for blk in range(3):
            s = 0.0
            for b in range(11):
                s += F[11 * blk + b]
            for b in range(11):
                out[t][11 * blk + b] = F[11 * blk + b] * (100.0 / s if s != 0.0 else 0.0)
    return spfh, K, out, counts


def test_restatement_equals_a_literal_double_loop():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1, (60, 3))
    pts[7] = pts[3]                                   # a duplicate
    nrm = _unit(rng, 60)
    nrm[11, 1] = np.nan                               # a row without a normal
    kp = np.r_[pts[[0, 3, 7, 11, 20]], (pts[1:4] + pts[4:7]) / 2, [[9.0, 9.0, 9.0]], [[np.nan, 0.0, 0.0]]]
    radius = 0.45
    spfh, K, out, counts = _literal(pts.tolist(), nrm.tolist(), kp.tolist(), radius)
    s = pf.spfh(pts, nrm, radius)
    assert np.array_equal(s["counts"], K) and K.min() >= 2
    assert np.array_equal(s["values"], spfh)          # integer counts times one rounded quotient: the same bits
    f = pf.fpfh33(pts, nrm, kp, radius)
    assert np.array_equal(f["counts"], counts) and list(counts[-2:]) == [0, 0]
    assert np.isnan(f["values"][-2:]).all() and np.isnan(out[-2:]).all()
    assert np.abs(f["values"][:-2] - out[:-2]).max() <= 2 * (K.max() + 16) * 2.0 ** -53 * 100.0
    assert f["n_spfh"] == len(np.unique(np.concatenate(pf.balls(pts, kp, radius))))


def test_every_block_sums_to_100_or_to_0():
    rng = np.random.default_rng(6)
    pts = np.r_[rng.uniform(0, 1, (300, 3)), [[5.0, 5.0, 5.0]], [[8.0, 8.0, 8.0]], [[8.0, 8.0, 8.0]]]
    nrm = _unit(rng, len(pts))
    kp = np.r_[pts[:50], [[5.0, 5.0, 5.0]], [[5.0, 5.0, 5.2]], [[8.0, 8.0, 8.0]], rng.uniform(0, 1, (10, 3))]
    f = pf.fpfh33(pts, nrm, kp, 0.3)
    blocks = f["values"].reshape(len(kp), 3, 11).sum(axis=2)
    assert np.isfinite(blocks).all()
    assert ((np.abs(blocks - 100.0) <= 1e-10) | (blocks == 0.0)).all()
    assert (np.abs(blocks[:50] - 100.0) <= 1e-10).all()
    assert not f["values"][50].any()                  # a ball of the row alone, at distance 0: 33 zeros
    assert not f["values"][51].any()                  # a ball of one row beside the keypoint, whose SPFH is zero (K = 1)
    assert not f["values"][52].any() and f["counts"][52] == 2     # two rows at distance 0


def test_degenerate_pairs_are_skipped_and_still_counted():
    rng = np.random.default_rng(7)
    pts = rng.uniform(0, 1, (40, 3))
    pts[1] = pts[0]
    pts[2] = pts[0]                                   # rows 0, 1, 2: one position
    nrm = _unit(rng, 40)
    nrm[5] = [np.nan, 0.0, 1.0]
    nrm[6] = [0.0, np.inf, 0.0]
    s = pf.spfh(pts, nrm, 2.0)                        # every row in every ball
    assert (s["counts"] == 40).all()
    binned = s["hist"].reshape(40, 3, 11).sum(axis=2)
    assert (binned[:, 0] == binned[:, 1]).all() and (binned[:, 1] == binned[:, 2]).all()
    want = np.full(40, 39 - 2)                        # every other row but the two without a normal ...
    want[[0, 1, 2]] -= 2                              # ... and but the row's two duplicates
    want[[5, 6]] = 0                                  # a row without a normal has no pair at all
    assert np.array_equal(binned[:, 0], want)
    assert not s["values"][[5, 6]].any()
    # K - 1 = 39 scales the counts whatever was skipped
    assert np.array_equal(s["values"], s["hist"] * (100.0 / 39))
    # a pair whose line is parallel to the frame's normal: the cross product is zero
    pts2 = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.5], [0.3, 0.0, 0.0]])
    nrm2 = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    s2 = pf.spfh(pts2, nrm2, 1.0)
    assert list(s2["counts"]) == [3, 3, 3]
    assert list(s2["hist"].reshape(3, 3, 11).sum(axis=2)[:, 0]) == [1, 1, 2]


def test_knn_normals_of_a_plane_look_at_the_viewpoint():
    rng = np.random.default_rng(8)
    pts = np.c_[rng.uniform(-1, 1, (120, 2)), np.full(120, -2.0)]
    res = pf.knn_normals(pts, 10)
    assert np.abs(res["normals"] - [0.0, 0.0, 1.0]).max() <= 1e-12       # the origin is above the plane
    assert np.abs(res["curvature"]).max() <= 1e-12
    below = pf.knn_normals(pts, 10, viewpoint=(0.0, 0.0, -5.0))
    assert np.abs(below["normals"] - [0.0, 0.0, -1.0]).max() <= 1e-12
    two = pf.knn_normals(pts[:2], 10)
    assert np.isnan(two["normals"]).all() and np.isnan(two["curvature"]).all()
