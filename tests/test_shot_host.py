"""CPU: the NumPy restatement of the SHOT352 rules (tests/shot_checks.py) on cases whose answer is derived by hand or can be had by a
literal per-neighbour loop, and the call surface of the new entry points (pcr_shot_lrf, pcr_shot352; pcl_features.py) against the
reference wrapper's (PCLKeypoints/src/keypoints.cpp:282-291)."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import shot_checks as sc
from tests.conftest import ROOT


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


# ------------------------------------------------------------------------------------------------ the call surface
def test_abi_is_declared_bound_and_exported(pcp):
    L = pcp._lib
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for name, n_params in (("pcr_shot_lrf", 7), ("pcr_shot352", 10)):
        decls = re.findall(r"PCR_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decls) == 1, name                                          # declared once
        params = re.sub(r"/\*.*?\*/", "", decls[0], flags=re.S).split(",")
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert len(L.SIGNATURES[name][1]) == len(params) == n_params, name    # one bound argument per declared parameter
    assert header.count("parity with PCL's binary32 output is unpinned") >= 3
    # bad arguments are refused before any device work (there is no device here)
    one = np.zeros(9)
    d = L.dptr(one)
    assert lib.pcr_shot_lrf(None, None, None, 0, 1.0, None, None) == L.PCR_E_INVALID
    assert lib.pcr_shot_lrf(None, None, d, 1, 1.0, d, None) == L.PCR_E_INVALID
    assert lib.pcr_shot352(None, None, None, None, 0, 1.0, None, None, None, None) == L.PCR_E_INVALID
    assert lib.pcr_shot352(None, None, d, d, 1, 1.0, None, d, None, None) == L.PCR_E_INVALID
    assert not one.any()


WRAPPER = {   # keypoints.cpp:282-291: the shared parameters, their names and defaults
    "shot352": [("pointcloud", None), ("keypoints", None), ("compute_normal_k", 10), ("feature_radius", 1.0)],
    "shot352_with_normal": [("pointcloud", None), ("normals", None), ("keypoints", None), ("feature_radius", 1.0)],
}
KEYWORD_ONLY = {"shot352": {"viewpoint", "ctx", "return_info"}, "shot352_with_normal": {"frames", "ctx", "return_info"}}
STUB = {"shot352": "featureSHOT352", "shot352_with_normal": "featureSHOT352WithNormal"}


def test_python_signatures_and_defaults_equal_the_wrapper(pcp):
    mod = pcp.pcl_features
    assert pcp.shot352 is mod.shot352 and pcp.shot352_with_normal is mod.shot352_with_normal and pcp.shot_lrf is mod.shot_lrf
    assert {"shot352", "shot352_with_normal", "shot_lrf"} <= set(mod.__all__)
    for name, want in WRAPPER.items():
        sig = inspect.signature(getattr(mod, name))
        params = [p for p in sig.parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD]
        got = [(p.name, None if p.default is p.empty else p.default) for p in params]
        assert got == want, name
        for (_, d), (_, w) in zip(got, want):
            assert type(d) is type(w), name
        assert {p.name for p in sig.parameters.values() if p.kind is p.KEYWORD_ONLY} == KEYWORD_ONLY[name], name
        # the wrapper's own names take the same shared parameters, and say where the descriptor is
        stub = getattr(pcp.PCLKeypoint, STUB[name])
        assert [p.name for p in inspect.signature(stub).parameters.values()] == [n for n, _ in want], name
        with pytest.raises(NotImplementedError) as e:
            stub(*([np.zeros((4, 3))] * (len(want) - 1)))
        assert "pcl_features.shot352" in str(e.value) and "descriptor" in str(e.value), name
    sig = inspect.signature(mod.shot_lrf)
    assert [(p.name, p.default) for p in sig.parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD][2:] == [("radius", 1.0)]
    assert {p.name for p in sig.parameters.values() if p.kind is p.KEYWORD_ONLY} == {"ctx", "return_counts"}


# ------------------------------------------------------------------------------------------------ the rules
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _literal_hist(pts, nrm, x, r, F):
    """The histogram rules of include/pcr.h for one keypoint as a per-neighbour loop in Python floats -> (352 ints, K, used)."""
    q4, q2, q34, q78 = math.pi / 4, math.pi / 2, sc.Q34, sc.Q78
    h = [0] * 352
    K = used = 0

    def add(slot, val):
        assert 0 <= slot < 352 and val >= 0
        h[slot] += int(np.rint(val * 4294967296.0))

    def clamp(v, lo, hi):
        return lo if v < lo else (hi if v > hi else v)

    for p, n in zip(pts, nrm):
        v = [p[0] - x[0], p[1] - x[1], p[2] - x[2]]
        d2 = _dot(v, v)
        if not d2 <= r * r:
            continue
        K += 1
        if not all(map(math.isfinite, n)) or d2 == 0.0:
            continue
        used += 1
        c = clamp(_dot(n, F[2]), -1.0, 1.0)
        b = ((1.0 + c) * 10) / 2
        X, Y, Z = (0.0 if abs(t) < 1e-30 else t for t in (_dot(v, F[0]), _dot(v, F[1]), _dot(v, F[2])))
        d = math.sqrt(d2)
        bit4 = 1 if (Y > 0 or (Y == 0 and X < 0)) else 0
        bit3 = (1 - bit4) if (X > 0 or (X == 0 and Y > 0)) else bit4
        desc = ((bit4 << 3) + (bit3 << 2)) << 1
        if X * Y > 0 or X == 0:
            desc += 0 if abs(X) >= abs(Y) else 4
        else:
            desc += 4 if abs(X) > abs(Y) else 0
        desc += 1 if Z > 0 else 0
        desc += 2 if d > 0.5 * r else 0
        sel = desc >> 2
        step = int(math.floor(b + 0.5))
        assert 0 <= step <= 10
        rho = b - step
        vol = desc * 11
        W = 1.0 - abs(rho)
        if rho > 0:
            add(vol + (step + 1) % 10, rho)
        else:
            add(vol + (step - 1 + 10) % 10, -rho)
        if d > 0.5 * r:
            t = (d - 0.75 * r) / (0.5 * r)
            if d > 0.75 * r:
                W += 1 - t
            else:
                W += 1 + t
                add((desc - 2) * 11 + step, -t)
        else:
            t = (d - 0.25 * r) / (0.5 * r)
            if d < 0.25 * r:
                W += 1 + t
            else:
                W += 1 - t
                add((desc + 2) * 11 + step, t)
        theta = math.acos(clamp(Z / d, -1.0, 1.0))
        if Z <= 0:
            u = (theta - q34) / q2
            if theta > q34:
                W += 1 - u
            else:
                W += 1 + u
                add((desc + 1) * 11 + step, -u)
        else:
            u = (theta - q4) / q2
            if theta < q4:
                W += 1 + u
            else:
                W += 1 - u
                add((desc - 1) * 11 + step, u)
        if X != 0 or Y != 0:
            a = clamp((math.atan2(Y, X) - (-q78 + q4 * sel)) / q4, -0.5, 0.5)
            if a > 0:
                W += 1 - a
                add(((desc + 4) % 32) * 11 + step, a)
            else:
                W += 1 + a
                add(((desc - 4 + 32) % 32) * 11 + step, -a)
        add(vol + step, W)
    return h, K, used


def _literal_frame(pts, x, r):
    """The frame rules as loops -> (3x3 rows x, y, z or None, K)."""
    m = [0.0] * 6
    ws = 0.0
    nb = []
    for row, p in enumerate(pts):
        v = [p[0] - x[0], p[1] - x[1], p[2] - x[2]]
        d2 = _dot(v, v)
        if not d2 <= r * r:
            continue
        w = r - math.sqrt(d2)
        nb.append((d2, row, v))
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            m[k] += (w * v[a]) * v[b]
        ws += w
    K = len(nb)
    if K < 5 or not ws > 0:
        return None, K
    M = np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]]) / ws
    e, V = np.linalg.eigh(M)
    axes = []
    for a in (V[:, 2], V[:, 0]):
        a = list(a / math.sqrt(_dot(a, a)))
        lead = max(range(3), key=lambda k: (abs(a[k]), -k))            # the largest magnitude, the first of equal ones
        if a[lead] < 0:
            a = [-c for c in a]
        P = sum(1 for _, _, v in nb if _dot(v, a) >= 0)
        s = 2 * P - K
        if s == 0:
            five = sorted(nb, key=lambda t: (t[0], t[1]))[K // 2 - 2: K // 2 + 3]
            s = 1 if sum(1 for _, _, v in five if _dot(v, a) > 0) >= 3 else -1
        axes.append([-c for c in a] if s < 0 else a)
    xa, za = axes
    ya = [za[1] * xa[2] - za[2] * xa[1], za[2] * xa[0] - za[0] * xa[2], za[0] * xa[1] - za[1] * xa[0]]
    return [xa, ya, za], K


def test_restatement_equals_a_literal_per_neighbour_loop():
    """Frames: the two moment sums run in different orders, so the frames agree to rounding (the eigenvalue gaps of the case are
    asserted).  Histogram, with the restatement's frame on both sides: every hard decision is the same bits, math.acos / atan2 and
    NumPy's may differ in the last place, which moves a contribution by at most one unit of 2^-32: three contributions of a neighbour
    (elevation, azimuth, W) depend on them, so a bin differs by at most 3 * used units."""
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1, (30, 3))
    pts[7] = pts[3]                                   # a duplicate row
    nrm = _unit(rng, 30)
    nrm[11, 1] = np.nan                               # a row without a normal
    r = 0.6
    far = np.argmax(np.linalg.norm(pts - 0.5, axis=1))                        # a keypoint 0.5 beyond the outermost row: a ball of a few rows
    lonely = pts[far] + 0.5 * (pts[far] - 0.5) / np.linalg.norm(pts[far] - 0.5)
    kp = np.r_[pts[[0, 3, 11, 20]], (pts[1:4] + pts[4:7]) / 2, [[9.0, 9.0, 9.0]], [[np.nan, 0.0, 0.0]], [lonely]]
    res = sc.shot352(pts, nrm, kp, r)
    assert list(res["counts"][-3:-1]) == [0, 0] and 1 <= res["counts"][-1] < 5 and res["counts"][:-3].min() >= 5
    assert np.isnan(res["values"][-3:]).all() and np.isnan(res["frames"][-3:]).all()
    assert res["lrf"]["gap"][:-3].min() > 1e-3
    same = 0
    for i, x in enumerate(kp[:-3]):
        F, K = _literal_frame(pts.tolist(), x.tolist(), r)
        assert K == res["counts"][i]
        assert np.abs(np.array(F) - res["frames"][i]).max() < 1e-11, i
        h, K, used = _literal_hist(pts.tolist(), nrm.tolist(), x.tolist(), r, res["frames"][i].tolist())
        assert K == res["counts"][i] and used == res["used"][i]
        assert used < K if i in (0, 1, 2) else used <= K                       # the keypoint's own row (d2 == 0), the row without a normal
        diff = np.abs(np.array(h, dtype=np.int64) - res["hist"][i])
        assert diff.max() <= 3 * used, (i, diff.max())
        same += int(diff.max() == 0)
    print("keypoints whose integer histograms are equal:", same, "of", len(kp) - 3)
    assert _literal_frame(pts.tolist(), lonely.tolist(), r) == (None, res["counts"][-1])


def _mirrored(half, seed, radius=None):
    """p_1 .. p_half and their negatives, |p_1| < |p_2| < ...; with ``radius`` every |p_k| is that radius to rounding (a sphere)."""
    rng = np.random.default_rng(seed)
    p = _unit(rng, half) * (np.sort(rng.uniform(0.2, 0.9, half))[:, None] if radius is None else radius)
    return np.r_[p, -p]


def test_mirrored_surface_is_decided_by_the_five_medians():
    """Keypoint = the origin (no row), surface rows 0..2 = p_1, p_2, p_3 with |p_1| < |p_2| < |p_3|, rows 3..5 = -p_k.  -p is exact,
    so for ANY axis a the products v.a come in exact +- pairs: P = 3 = K / 2 (no product is 0 for generic p), s = 0, a tie on both
    axes.  Ascending (d2, row): +p_1 (row 0), -p_1 (3), +p_2 (1), -p_2 (4), +p_3 (2), -p_3 (5); the ranks K/2-2 .. K/2+2 = 1 .. 5 are
    -p_1, +p_2, -p_2, +p_3, -p_3.  Each of the pairs +-p_2, +-p_3 has exactly one member with v.a > 0, so the count is 2 + [(-p_1).a > 0]
    and the axis is negated exactly when p_1.a > 0: the final x and z both satisfy p_1.axis < 0 -- whichever sign the eigen solver
    returned, since a -> -a maps the count c to 5 - c."""
    pts = _mirrored(3, seed=21)
    res = sc.lrf(pts, np.zeros((1, 3)), 1.0)
    assert res["counts"][0] == 6 and res["tie"][0].all() and res["gap"][0] > 1e-3
    x, y, z = res["frames"][0]
    assert pts[0] @ x < -1e-6 and pts[0] @ z < -1e-6
    assert np.allclose(np.cross(z, x), y, atol=1e-15) and abs(np.linalg.det(res["frames"][0]) - 1.0) < 1e-12
    # the same rows in another order: the tie break is by (d2, row), so moving -p_1 in front of +p_1 flips what rank 0 drops
    swapped = pts[[3, 1, 2, 0, 4, 5]]
    x2, _, z2 = sc.lrf(swapped, np.zeros((1, 3)), 1.0)["frames"][0]
    assert swapped[0] @ x2 < -1e-6 and swapped[0] @ z2 < -1e-6
    assert np.allclose(x2, -x, atol=1e-12) and np.allclose(z2, -z, atol=1e-12)


def test_a_row_at_the_keypoint_leaves_the_canonical_sign():
    """The mirrored surface with the keypoint itself as a seventh row: the zero vector counts as plus for a and for -a, so P = 4 and
    s = 2 * 4 - 7 = 1 > 0 for BOTH signs of any axis -- the sign rule keeps whatever it is given.  The rule text therefore fixes the
    sign it starts from: the component of largest magnitude is positive."""
    pts = np.r_[_mirrored(3, seed=21), np.zeros((1, 3))]
    res = sc.lrf(pts, np.zeros((1, 3)), 1.0)
    assert res["counts"][0] == 7 and not res["tie"][0].any()
    x, y, z = res["frames"][0]
    assert x[np.argmax(np.abs(x))] > 0 and z[np.argmax(np.abs(z))] > 0
    assert np.sort(np.abs(x))[-1] - np.sort(np.abs(x))[-2] > 1e-3 and np.sort(np.abs(z))[-1] - np.sort(np.abs(z))[-2] > 1e-3      # no near tie of magnitudes
    F, K = _literal_frame(pts.tolist(), [0.0, 0.0, 0.0], 1.0)
    assert K == 7 and np.abs(np.array(F) - res["frames"][0]).max() < 1e-11


def test_four_rows_have_no_frame_and_five_have_one():
    rng = np.random.default_rng(22)
    pts = rng.uniform(-0.4, 0.4, (5, 3))
    nrm = _unit(rng, 5)
    four = sc.shot352(pts[:4], nrm[:4], np.zeros((1, 3)), 1.0)
    assert four["counts"][0] == 4 and np.isnan(four["frames"]).all() and np.isnan(four["values"]).all()
    five = sc.shot352(pts, nrm, np.zeros((1, 3)), 1.0)
    assert five["counts"][0] == 5 and np.isfinite(five["frames"]).all() and np.isfinite(five["values"]).all()
    F = five["frames"][0]
    assert np.abs(F @ F.T - np.eye(3)).max() < 1e-14 and np.linalg.det(F) > 0
    # a frame that is given replaces the rule about K
    given = sc.shot352(pts[:4], nrm[:4], np.zeros((1, 3)), 1.0, frames=np.eye(3)[None])
    assert given["counts"][0] == 4 and np.isfinite(given["values"]).all()


def test_one_neighbour_on_the_x_axis_fills_the_slots_derived_by_hand():
    """r = 1, frame = identity, one neighbour at v = (0.6, 0, 0) with normal (0, 0, 1):
    c = 1, b = 10; X = 0.6, Y = Z = 0; bit4 = 0, bit3 = 1, desc = 8; X*Y = 0 and X != 0: |X| > |Y| adds 4 -> 12; Z > 0 no; d = 0.6 > 0.5
    adds 2 -> desc = 14, sel = 3 (centre -7pi/8 + 3pi/4 = -pi/8), vol = 154.  step = floor(10.5) = 10, rho = 0: slot 154 + 9 gets 0, W = 1.
    Radial: t = (0.6 - 0.75) / 0.5 = -0.3, d <= 0.75: W += 0.7, slot 11 * 12 + 10 = 142 gets 0.3.
    Elevation: theta = pi/2, Z <= 0: u = (pi/2 - 3pi/4) / (pi/2) = -0.5, W += 0.5, slot 11 * 15 + 10 = 175 gets 0.5.
    Azimuth: (0 + pi/8) / (pi/4) = 0.5 > 0: W += 0.5, slot 11 * 18 + 10 = 208 gets 0.5.  Last: slot 154 + 10 = 164 gets W = 2.7.
    Each to within one unit of 2^-32 (0.6 - 0.75 and the constants are rounded); the norm is sqrt(0.09 + 0.25 + 0.25 + 7.29)."""
    res = sc.shot352([[0.6, 0.0, 0.0]], [[0.0, 0.0, 1.0]], np.zeros((1, 3)), 1.0, frames=np.eye(3)[None])
    want = {142: 0.3, 175: 0.5, 208: 0.5, 164: 2.7}
    h = res["hist"][0]
    assert set(np.flatnonzero(h)) == set(want)
    for slot, v in want.items():
        assert abs(int(h[slot]) - v * 2.0 ** 32) <= 1.0, slot
    assert res["used"][0] == res["counts"][0] == 1
    out = res["values"][0]
    assert abs(out[164] - 2.7 / math.sqrt(7.88)) < 1e-9 and abs(out[142] - 0.3 / math.sqrt(7.88)) < 1e-9
    h2, K, used = _literal_hist([[0.6, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [0.0, 0.0, 0.0], 1.0, np.eye(3).tolist())
    assert np.abs(np.array(h2) - h).max() <= 1 and (K, used) == (1, 1)
    # the neighbour at the keypoint itself, or without a normal, is skipped: a zero norm, PCL's 0 / 0
    for p, n in (([0.0, 0.0, 0.0], [0.0, 0.0, 1.0]), ([0.6, 0.0, 0.0], [0.0, np.inf, 1.0])):
        skipped = sc.shot352([p], [n], np.zeros((1, 3)), 1.0, frames=np.eye(3)[None])
        assert skipped["counts"][0] == 1 and skipped["used"][0] == 0 and not skipped["hist"].any() and np.isnan(skipped["values"]).all()
    # a frame with an entry that is not finite: NaN
    bad = np.eye(3)[None].copy()
    bad[0, 1, 1] = np.inf
    assert np.isnan(sc.shot352([[0.6, 0.0, 0.0]], [[0.0, 0.0, 1.0]], np.zeros((1, 3)), 1.0, frames=bad)["values"]).all()


def test_finite_rows_have_unit_norm_and_no_negative_entry():
    rng = np.random.default_rng(23)
    pts = rng.uniform(0, 1, (400, 3))
    nrm = _unit(rng, 400)
    kp = np.r_[pts[:30], rng.uniform(0, 1, (10, 3)), [[5.0, 5.0, 5.0]]]
    res = sc.shot352(pts, nrm, kp, 0.3)
    fin = np.isfinite(res["values"]).all(axis=1)
    assert fin[:40].all() and not fin[40] and res["counts"][:40].min() >= 5
    assert np.abs(np.linalg.norm(res["values"][fin], axis=1) - 1.0).max() < 1e-14
    assert (res["values"][fin] >= 0).all() and (res["hist"] >= 0).all()
    # every neighbour that is not skipped adds between 2 and 4 in all: 1 (cosine) + >= 0.5 (radial) + >= 0.5 (elevation) + <= 1 (azimuth)
    total = res["hist"][fin].sum(axis=1) * 2.0 ** -32
    assert (total >= 2 * res["used"][fin] - 1e-6).all() and (total <= 4 * res["used"][fin] + 1e-6).all()
    F = res["frames"][fin]
    assert np.abs(np.einsum("kij,klj->kil", F, F) - np.eye(3)).max() < 1e-14 and (np.linalg.det(F) > 0).all()
