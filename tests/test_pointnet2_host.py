"""CPU-only checks of the PointNet++ ops: the C ABI declares and exports them, the subpackage imports without a device, every argument
check raises before anything could be launched, and the NumPy restatements of tests/pointnet2_checks.py agree with independent
formulations and with cases worked by hand."""
import importlib
import os
import re

import numpy as np
import pytest

from tests import pointnet2_checks as chk
from tests.conftest import ROOT

SYMBOLS = ("pcr_pn2_furthest_point_sampling", "pcr_pn2_ball_query", "pcr_pn2_three_nn", "pcr_pn2_three_interpolate", "pcr_pn2_gather_points",
           "pcr_pn2_group_points")


@pytest.fixture(scope="module")
def pn2():
    return importlib.import_module("point-cloud-process_amd.pointnet2_ops")


def test_symbols_are_declared_in_the_header_and_have_signatures(pcp):
    txt = open(os.path.join(ROOT, "include", "pcr.h")).read()
    declared = set(re.findall(r"PCR_API\s+[\w\s\*]+?\b(pcr_\w+)\s*\(", txt))
    lib = pcp._lib.lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in pcp._lib.SIGNATURES, name
        assert hasattr(lib, name), name
        restype, argtypes = pcp._lib.SIGNATURES[name]
        assert restype is pcp._lib.C.c_int and argtypes[0] is pcp._lib.C.c_void_p     # status; the stream comes first


def test_subpackage_imports_without_a_device_and_is_exported(pcp, pn2):
    u, mods = pn2.pointnet2_utils, pn2.pointnet2_modules
    for name in ("furthest_point_sample", "gather_operation", "three_nn", "three_interpolate", "grouping_operation", "ball_query", "QueryAndGroup",
                 "GroupAll"):
        assert hasattr(u, name), name
    for name in ("build_shared_mlp", "PointnetSAModuleMSG", "PointnetSAModule", "PointnetFPModule"):
        assert hasattr(mods, name), name
    assert pcp.pointnet2_ops is pn2 and pcp.pointnet2_utils is u and pcp.pointnet2_modules is mods
    assert pcp.furthest_point_sample_np is pn2.furthest_point_sample_np
    # the modules build on the host (parameters only): the reference's layout of sub-modules, so that its checkpoints load
    sa = mods.PointnetSAModuleMSG(npoint=16, radii=[0.3, 0.6], nsamples=[4, 8], mlps=[[2, 8], [2, 8, 16]])
    assert sorted(k for k in sa.state_dict() if k.endswith("weight") and ".0.weight" in k) == ["mlps.0.0.weight", "mlps.1.0.weight"]
    assert sa.mlps[0][0].in_channels == 5 and sa.mlps[1][3].out_channels == 16
    fp = mods.PointnetFPModule(mlp=[6, 8])
    assert fp.mlp[0].in_channels == 6 and fp.mlp[0].bias is None and isinstance(fp.mlp[1], pn2.pointnet2_utils.nn.BatchNorm2d)
    assert mods.build_shared_mlp([3, 4], bn=False)[0].bias is not None
    one = mods.PointnetSAModule(mlp=[0, 4], npoint=None)
    assert isinstance(one.groupers[0], u.GroupAll) and one.mlps[0][0].in_channels == 3


def test_every_argument_check_raises_before_a_launch(pn2):
    import torch

    u = pn2.pointnet2_utils
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)     # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)       # noqa: E731
    # CPU tensors that are otherwise right
    for call in (lambda: u.furthest_point_sample(f(2, 8, 3), 4), lambda: u.gather_operation(f(2, 3, 8), i(2, 4)),
                 lambda: u.three_nn(f(2, 8, 3), f(2, 5, 3)), lambda: u.three_interpolate(f(2, 4, 5), i(2, 8, 3), f(2, 8, 3)),
                 lambda: u.grouping_operation(f(2, 4, 8), i(2, 3, 5)), lambda: u.ball_query(0.5, 4, f(2, 8, 3), f(2, 3, 3)),
                 lambda: u.QueryAndGroup(0.5, 4)(f(2, 8, 3), f(2, 3, 3))):
        with pytest.raises(ValueError, match="must be on the GPU"):
            call()
    # dtype
    for call in (lambda: u.furthest_point_sample(f(2, 8, 3).double(), 4), lambda: u.gather_operation(f(2, 3, 8), i(2, 4).long()),
                 lambda: u.gather_operation(f(2, 3, 8).half(), i(2, 4)), lambda: u.three_nn(f(2, 8, 3), f(2, 5, 3).double()),
                 lambda: u.three_interpolate(f(2, 4, 5), i(2, 8, 3).long(), f(2, 8, 3)), lambda: u.three_interpolate(f(2, 4, 5), i(2, 8, 3), i(2, 8, 3)),
                 lambda: u.grouping_operation(f(2, 4, 8), f(2, 3, 5)), lambda: u.ball_query(0.5, 4, f(2, 8, 3).double(), f(2, 3, 3))):
        with pytest.raises(ValueError, match="must have dtype"):
            call()
    # rank and the trailing 3
    for call in (lambda: u.furthest_point_sample(f(8, 3), 4), lambda: u.gather_operation(f(2, 3, 8), i(2, 4, 1)), lambda: u.three_nn(f(8, 3), f(2, 5, 3)),
                 lambda: u.three_interpolate(f(2, 4, 5), i(2, 8), f(2, 8, 3)), lambda: u.grouping_operation(f(2, 4, 8), i(2, 3)),
                 lambda: u.ball_query(0.5, 4, f(2, 8, 3), f(3, 3))):
        with pytest.raises(ValueError, match="must have rank"):
            call()
    for call in (lambda: u.furthest_point_sample(f(2, 8, 4), 4), lambda: u.three_nn(f(2, 8, 3), f(2, 5, 2)),
                 lambda: u.three_interpolate(f(2, 4, 5), i(2, 8, 4), f(2, 8, 4)), lambda: u.ball_query(0.5, 4, f(2, 8, 2), f(2, 3, 3))):
        with pytest.raises(ValueError, match="entries along axis"):
            call()
    # contiguity
    for call in (lambda: u.furthest_point_sample(f(2, 3, 8).transpose(1, 2), 4), lambda: u.gather_operation(f(2, 8, 3).transpose(1, 2), i(2, 4)),
                 lambda: u.three_nn(f(2, 8, 3), f(2, 3, 5).transpose(1, 2)), lambda: u.three_interpolate(f(2, 4, 5), i(2, 8, 3), f(2, 8, 6)[:, :, ::2]),
                 lambda: u.grouping_operation(f(2, 4, 8), i(2, 5, 3).transpose(1, 2)), lambda: u.ball_query(0.5, 4, f(2, 8, 3), f(2, 3, 6)[:, :, :3])):
        with pytest.raises(ValueError, match="must be contiguous"):
            call()
    # batch sizes (and the shared n of idx and weight)
    for call in (lambda: u.gather_operation(f(2, 3, 8), i(3, 4)), lambda: u.three_nn(f(2, 8, 3), f(1, 5, 3)),
                 lambda: u.three_interpolate(f(2, 4, 5), i(3, 8, 3), f(2, 8, 3)), lambda: u.grouping_operation(f(2, 4, 8), i(1, 3, 5)),
                 lambda: u.ball_query(0.5, 4, f(2, 8, 3), f(3, 3, 3))):
        with pytest.raises(ValueError, match="mismatched batch sizes"):
            call()
    with pytest.raises(ValueError, match="mismatched sizes"):
        u.three_interpolate(f(2, 4, 5), i(2, 8, 3), f(2, 9, 3))
    # scalars
    for call in (lambda: u.furthest_point_sample(f(2, 8, 3), -1), lambda: u.furthest_point_sample(f(2, 8, 3), 2.5), lambda: u.ball_query(0.5, -4, f(2, 8, 3), f(2, 3, 3)),
                 lambda: u.ball_query(float("nan"), 4, f(2, 8, 3), f(2, 3, 3)), lambda: u.ball_query(float("inf"), 4, f(2, 8, 3), f(2, 3, 3))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        pn2.furthest_point_sample_np(np.zeros((4, 2)), 2)


def test_sampling_without_a_gpu_fails_loudly(pn2):
    import torch

    pts = np.random.default_rng(0).normal(size=(16, 3))
    if torch.cuda.is_available():
        assert np.array_equal(pn2.furthest_point_sample_np(pts, 4), chk.fps_one(pts, 4))
        return
    with pytest.raises(RuntimeError, match="needs a GPU"):
        pn2.furthest_point_sample_np(pts, 4)


# ------------------------------------------------------------------ the restatements against independent formulations
def test_fps_restatement_equals_the_matrix_formulation():
    rng = np.random.default_rng(11)
    lattice = np.stack(np.meshgrid(*[np.arange(1, 5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)     # ties everywhere
    planted = rng.normal(size=(60, 3)).astype(np.float32)
    planted[[0, 7, 31]] = [[0.0, 0.0, 0.0], [0.01, 0.02, 0.0], [0.0, 0.0, 0.03]]
    dup = rng.normal(size=(20, 3)).astype(np.float32)
    for pts, m in ((rng.normal(size=(1, 3)).astype(np.float32), 3), (rng.normal(size=(2, 3)).astype(np.float32), 5),
                   (rng.normal(size=(90, 3)).astype(np.float32), 90), (lattice, 64), (planted, 60), (np.concatenate([dup, dup]), 30)):
        assert np.array_equal(chk.fps_one(pts, m), chk.fps_by_matrix(pts, m)), (len(pts), m)


def test_ball_query_restatement_equals_the_sort_formulation():
    rng = np.random.default_rng(12)
    xyz = rng.uniform(-1, 1, size=(2, 150, 3)).astype(np.float32)
    xyz[1, 100:] = xyz[1, :50]                                # equal distances
    centres = np.concatenate([xyz[:, :6], rng.uniform(2, 3, size=(2, 3, 3)).astype(np.float32)], axis=1)     # the last three see nothing
    for radius, nsample in ((0.05, 4), (0.4, 8), (0.4, 1), (3.0, 16), (10.0, 200)):
        got = chk.ball_query(radius, nsample, xyz, centres)
        for b in range(2):
            for j in range(centres.shape[1]):
                assert np.array_equal(got[b, j], chk.ball_query_by_sort(radius, nsample, xyz[b], centres[b, j])), (radius, nsample, b, j)
    assert not chk.ball_query(0.4, 8, xyz, centres)[:, 6:].any()
    assert (chk.ball_query(0.05, 4, xyz, centres)[0, :6] == np.arange(6)[:, None]).all()     # alone in its ball: the row repeats the centre


def test_three_nn_restatement_equals_the_sort_formulation():
    rng = np.random.default_rng(13)
    for m in (1, 2, 3, 4, 40):
        known = rng.normal(size=(2, m, 3)).astype(np.float32)
        if m >= 4:
            known[:, m // 2:] = known[:, : m - m // 2]        # duplicated known points: equal distances
        unknown = rng.normal(size=(2, 25, 3)).astype(np.float32)
        d2, idx = chk.three_nn(unknown, known)
        for b in range(2):
            for i in range(25):
                ed, ei = chk.three_nn_by_sort(unknown[b, i], known[b])
                assert np.array_equal(d2[b, i].view(np.uint32), ed.view(np.uint32)) and np.array_equal(idx[b, i], ei), (m, b, i)


# ------------------------------------------------------------------ cases worked by hand
def test_hand_worked_furthest_point_sampling():
    two = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]], dtype=np.float32)
    assert chk.fps_one(two, 5).tolist() == [0, 1, 0, 0, 0]     # pick 2 on: both distances 0, the lower index
    assert chk.fps_one(two[:1], 3).tolist() == [0, 0, 0]
    # index 0 is padding: still the first pick, never again; the picks go on among 1..3
    pad0 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [5.0, 0.0, 0.0], [2.0, 0.0, 0.0]], dtype=np.float32)
    assert chk.fps_one(pad0, 6).tolist() == [0, 2, 3, 1, 1, 1]     # temp after pick 0: 1, 25, 4; after pick 2: 1, 0, 4; then 1 is left, then the lowest eligible index
    # |p|^2 = 1e-3 in float32 widens to a double just above 1e-3 or below?  state it by the rule, not by intuition
    edge = np.array([[3.0, 0.0, 0.0], [np.sqrt(np.float32(1e-3)), 0.0, 0.0], [0.0, 0.04, 0.0]], dtype=np.float32)
    mag1 = np.float64(np.float32(edge[1, 0] * edge[1, 0]))
    assert chk.eligible(edge).tolist() == [True, bool(mag1 > 1e-3), True]     # 0.04^2 = 1.6e-3 > 1e-3
    assert chk.eligible(np.array([[0.0, 0.03, 0.0], [0.02, 0.02, 0.01]], dtype=np.float32)).tolist() == [False, False]
    # nothing eligible: every pick is 0
    assert chk.fps_one(np.full((5, 3), 0.01, dtype=np.float32), 4).tolist() == [0, 0, 0, 0]
    assert chk.fps(np.zeros((2, 3, 3), dtype=np.float32), 2).tolist() == [[0, 0], [0, 0]]
    # a square: from corner 0 the far corner, then the two equally far corners in index order
    square = np.array([[1, 1, 0], [1, 2, 0], [2, 1, 0], [2, 2, 0]], dtype=np.float32)
    assert chk.fps_one(square, 4).tolist() == [0, 3, 1, 2]


def test_hand_worked_ball_query():
    xyz = np.array([[[0.5, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.4, 0.0], [9.0, 9.0, 9.0]]], dtype=np.float32)
    centres = np.array([[[0.0, 0.0, 0.0], [-5.0, 0.0, 0.0], [9.0, 9.0, 9.25]]], dtype=np.float32)
    got = chk.ball_query(0.5, 4, xyz, centres)
    assert got[0, 0].tolist() == [1, 2, 3, 1]     # point 0 at exactly d2 == radius2 is outside; three hits, the fourth slot repeats the first
    assert got[0, 1].tolist() == [0, 0, 0, 0]     # no neighbour
    assert got[0, 2].tolist() == [4, 4, 4, 4]
    assert chk.ball_query(0.5, 2, xyz, centres)[0, 0].tolist() == [1, 2]     # more hits than slots: the first by index
    assert chk.ball_query(np.nextafter(np.float32(0.5), np.float32(1)), 4, xyz, centres)[0, 0].tolist() == [0, 1, 2, 3]


def test_hand_worked_three_nn_and_interpolate():
    known = np.array([[[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]], dtype=np.float32)
    unknown = np.array([[[0.0, 0.0, 0.0], [0.0, 2.0, 0.0]]], dtype=np.float32)
    d2, idx = chk.three_nn(unknown, known)
    assert d2[0].tolist() == [[1.0, 4.0, np.inf], [0.0, 5.0, np.inf]] and idx[0].tolist() == [[0, 1, 0], [1, 0, 0]]     # m = 2
    d2, idx = chk.three_nn(unknown, known[:, :1])
    assert d2[0].tolist() == [[1.0, np.inf, np.inf], [5.0, np.inf, np.inf]] and not idx.any()                            # m = 1
    same = np.zeros((1, 4, 3), dtype=np.float32)
    assert chk.three_nn(unknown[:, :1], same)[1][0, 0].tolist() == [0, 1, 2]     # equal distances: the earlier index stays ahead
    pts = np.array([[[1.0, 2.0, 4.0], [10.0, 20.0, 40.0]]], dtype=np.float32)
    out = chk.three_interpolate(pts, np.array([[[0, 1, 2], [2, 2, 0]]], dtype=np.int32), np.array([[[0.5, 0.25, 0.25], [1.0, 0.0, 2.0]]], dtype=np.float32))
    assert out.tolist() == [[[2.0, 6.0], [20.0, 60.0]]]
    assert chk.gather(pts, np.array([[2, 0, 2]], dtype=np.int32)).tolist() == [[[4.0, 1.0, 4.0], [40.0, 10.0, 40.0]]]
    assert chk.group(pts, np.array([[[2, 0], [1, 1]]], dtype=np.int32)).tolist() == [[[[4.0, 1.0], [2.0, 2.0]], [[40.0, 10.0], [20.0, 20.0]]]]


def test_gradient_restatements_are_the_transposes_of_the_forward_ops():
    rng = np.random.default_rng(14)
    B, c, n, m = 2, 3, 9, 5
    idx = rng.integers(0, m, size=(B, n, 3)).astype(np.int32)
    w = rng.uniform(size=(B, n, 3)).astype(np.float32)
    g = rng.normal(size=(B, c, n)).astype(np.float32)
    p = rng.normal(size=(B, c, m)).astype(np.float32)
    total, mag, count = chk.three_interpolate_grad(g, idx, w, m)
    fwd = sum(p.astype(np.float64)[np.arange(B)[:, None, None], np.arange(c)[None, :, None], idx[:, None, :, s]] * w.astype(np.float64)[:, None, :, s] for s in range(3))
    assert np.isclose((fwd * g).sum(), (total * p).sum(), rtol=1e-12)     # <J p, g> = <p, J^T g>
    assert count.sum() == B * 3 * n and (mag >= np.abs(total) - 1e-15).all()
    gi = rng.integers(0, m, size=(B, 7)).astype(np.int32)
    gg = rng.normal(size=(B, c, 7)).astype(np.float32)
    total, _, count = chk.gather_grad(gg, gi, m)
    assert np.isclose((chk.gather(p, gi).astype(np.float64) * gg).sum(), (total * p).sum(), rtol=1e-12) and count.sum() == B * 7
    qi = rng.integers(0, m, size=(B, 4, 6)).astype(np.int32)
    qg = rng.normal(size=(B, c, 4, 6)).astype(np.float32)
    total, _, count = chk.group_grad(qg, qi, m)
    assert np.isclose((chk.group(p, qi).astype(np.float64) * qg).sum(), (total * p).sum(), rtol=1e-12) and count.sum() == B * 24
    assert chk.summation_bound(np.array([2.0]), np.array([1.0]))[0] == pytest.approx(2.0 * 2.0 ** -24, rel=1e-6)
