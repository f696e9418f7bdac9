"""GPU: the lay-out of a query cloud along a Hilbert curve (csrc/pcr_curve.h, pcr_cloud_morton_sort) changes which 32 records form a
wave tile of the ICP pass and nothing of any result.

Order: DeviceCloud.order() after prepare() equals the stable argsort of the key restated in tests/curve_keys.py, for the default curve
and for PCR_QUERY_CURVE=morton.

Same bits: T_total, iters, n_assoc, status and the transformed source of 12 passes, and nn1, are compared byte for byte between the two
curves (every sum of the one-kernel pass is an order-independent fixed-point sum).  The consumers found whose binary64 sums follow the
record order are the ICP loop's three-launch pass (ungated runs, PCR_ICP_NO_FUSED=1: it therefore keeps the Morton lay-out, see
test_twelve_passes_same_bits), pcr_icp_moments (the 18 moments and the sum of d2), pcr_point2plane_moments (the 29 sums) and, through them, the compat and
point-to-plane loops and PCA; the two moment calls are held here to the bounds their own tests use (rtol 1e-11 / atol 1e-9 and 1e-9 on
the sum of d2: tests/test_gpu_nn_icp.py::test_pass_moments_match_oracle; 4 K 2^-52 sum|term| against the exact sum:
tests/test_gpu_point2plane.py::test_moments_against_numpy), the association counts exactly.  tests/test_gpu_cloud_states.py runs the
other consumers on prepared clouds, which now means clouds on the new curve."""
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import curve_keys as ck
from tests.test_gpu_gate_bounds import CELL, KW, _replace, _lift, _scene_clouds
from tests.test_gpu_gate_bounds import _run as _run_bounds
from tests.test_gpu_point2plane import ref_terms

pytestmark = pytest.mark.gpu


class _env:
    """Environment switches for the calls inside (libpcr reads them per call); None removes one."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


CURVES = {"rule": None, "morton": "morton"}     # restated curve -> PCR_QUERY_CURVE


# ------------------------------------------------------------------------------------------------------------------ order
def _kitti_2048(syn):
    return _scene_clouds(syn)[0], CELL


def _cube_4096(syn):
    return np.random.default_rng(1).uniform(-2.0, 2.0, (4096, 3)), 0.0


def _one_cell(syn):
    return np.array([3.0, -1.0, 0.5]) + np.random.default_rng(2).uniform(0.0, 0.01, (200, 3)), 1.0


def _duplicates(syn):
    p = np.random.default_rng(3).uniform(0.0, 20.0, (500, 3)) * [1.0, 1.0, 0.1]
    rows = np.random.default_rng(4).choice(500, 128, replace=False)
    p[rows[:64]] = p[rows[64:]]                 # 64 rows are copies of 64 others
    return p, 0.5


def _plane(syn):
    p = np.random.default_rng(5).uniform(0.0, 30.0, (1000, 3))
    p[:, 2] = 1.25                               # zero extent along z
    return p, 0.7


def _wide_keys(syn):
    return np.random.default_rng(11).uniform(0.0, 1.0, (4097, 3)), 1.0 / 4096      # 39 key bits, as test_gpu_grid_build.py builds them


def _tiny(n):
    return lambda syn: (np.random.default_rng(20 + n).uniform(0.0, 5.0, (n, 3)), 1.0)


ORDER_CASES = {"n1": (_tiny(1), None), "n2": (_tiny(2), None), "n65": (_tiny(65), None), "kitti_2048": (_kitti_2048, "hilbert2_minor"),
               "cube_4096": (_cube_4096, "hilbert3"), "one_cell": (_one_cell, None), "duplicates_64": (_duplicates, "hilbert2_minor"),
               "plane_const_z": (_plane, "hilbert2_minor"), "key_bits_39": (_wide_keys, "hilbert3")}


@pytest.mark.parametrize("case", list(ORDER_CASES))
def test_order_is_the_restated_curve(pcp, syn, ctx, case):
    make, mode = ORDER_CASES[case]
    pts, cell = make(syn)
    index = pcp.TargetIndex(pts if len(pts) > 1 else np.r_[pts, pts + 1.0], cell=cell, ctx=ctx)
    cell = index.cell
    lo, hi = pts.min(0), pts.max(0)
    inv = 1.0 / ck.layout_cell(pts, cell)
    if mode is not None:
        assert ck.pick(lo, hi, inv)["mode"] == mode
    if case == "key_bits_39":
        assert ck.end_bit(lo, hi, inv) == 39
    if case == "one_cell":
        assert len(set(ck.layout_keys(pts, cell).tolist())) == 1
    try:
        orders = {}
        for curve, switch in CURVES.items():
            dc = pcp.DeviceCloud.upload(pts, ctx)
            assert np.array_equal(dc.order(), np.arange(len(pts)))                # upload order until laid out
            with _env(PCR_QUERY_CURVE=switch):
                dc.prepare(index)
            got = dc.order()
            assert pcp._lib.lib().pcr_cloud_reordered(dc.handle) == 1
            assert np.array_equal(got, ck.layout_order(pts, cell, curve)), (case, curve)
            assert np.array_equal(dc.download(), pts)                              # by caller row, whatever the order
            orders[curve] = got
            dc.free()
        if case in ("kitti_2048", "cube_4096", "key_bits_39", "plane_const_z"):
            assert not np.array_equal(orders["rule"], orders["morton"])            # (the switch does switch)
    finally:
        index.free()


# -------------------------------------------------------------------------------------------------------------- same bits
def _icp(pcp, index, src, switch, **env):
    with _env(PCR_QUERY_CURVE=switch, **env):
        sd = pcp.DeviceCloud.upload(src, index.ctx)
        r = pcp.icp_device(sd, index, np.eye(4), max_iter=12, min_iter=12, **KW)
        order = sd.order()
        out = (r["T_total"].tobytes(), int(r["iters"]), int(r["n_assoc"]), int(r["status"]), sd.download().tobytes())
        sd.free()
    return out, order


def _pair(syn, which):
    if which == "kitti_2048_cell_1":
        src, tgt = _scene_clouds(syn)
        return src, tgt, CELL
    src, tgt, _ = syn.perturbed_pair(8192, seed=3)
    return src.astype(np.float64), tgt.astype(np.float64), 0.0


@pytest.fixture(scope="module", params=["kitti_2048_cell_1", "kitti_8192_auto_cell"])
def pair(request, pcp, syn, ctx):
    src, tgt, cell = _pair(syn, request.param)
    index = pcp.TargetIndex(tgt, cell=cell, ctx=ctx)
    yield src, tgt, index
    index.free()


@pytest.mark.parametrize("env", [dict(PCR_PASS_INLINE="1"), dict(PCR_PASS_INLINE="0"), dict(PCR_ICP_NO_FUSED="1")], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_twelve_passes_same_bits(pcp, pair, env):
    """The one-kernel pass (one and two launches) adds fixed-point integers: the same bits on either curve.  The three-launch pass of
    PCR_ICP_NO_FUSED=1 adds binary64 slabs in record order (measured: T_total differs in its last bits between the curves), so
    pcr_icp lays a source out along the Morton curve for it whatever the switch says, and that is what keeps its bits."""
    src, _, index = pair
    env = {"PCR_PASS_INLINE": None, "PCR_ICP_NO_FUSED": None, **env}
    (hil, o_h), (mor, o_m) = _icp(pcp, index, src, None, **env), _icp(pcp, index, src, "morton", **env)
    assert np.array_equal(o_m, ck.layout_order(src, index.cell, "morton"))
    assert np.array_equal(o_h, ck.layout_order(src, index.cell, "morton" if env["PCR_ICP_NO_FUSED"] else "rule"))
    assert not np.array_equal(ck.layout_order(src, index.cell, "rule"), o_m)
    assert hil[1] == 12 and hil[3] == 0 and hil[2] > len(src) // 2
    assert hil == mor


def test_nn1_same_bits(pcp, pair):
    src, tgt, index = pair
    got = {}
    for curve, switch in CURVES.items():
        with _env(PCR_QUERY_CURVE=switch):
            dc = pcp.DeviceCloud.upload(src, index.ctx)
            got[curve] = (index.nn1(dc), index.nn1(dc, max_d2=5.0), dc.order())
            dc.free()
    assert not np.array_equal(got["rule"][2], got["morton"][2])
    for gate, a, b in zip((False, True), got["rule"][:2], got["morton"][:2]):
        keep = a[0] >= 0                                 # (d2 of a gated-out query is not a result: the existing tests compare the kept ones)
        assert np.array_equal(a[0], b[0]) and a[1][keep].tobytes() == b[1][keep].tobytes(), gate
        assert keep.all() or gate
    d, j = cKDTree(tgt).query(src, k=1)
    clear = got["rule"][0][0] == j                      # (exact ties aside, the rows are the tree's)
    assert clear.mean() > 0.99


def test_order_following_sums_within_their_bounds(pcp, oracle, pair):
    """pcr_icp_moments and pcr_point2plane_moments add binary64 terms in record order: counts exact, sums within their own tests' bounds."""
    src, tgt, index = pair
    rng = np.random.default_rng(9)
    nrm = rng.normal(size=tgt.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    index.set_normals(nrm)
    tree = cKDTree(tgt)
    T, max_dist = np.eye(4), float(np.sqrt(5.0))
    J, r, d2 = ref_terms(src, tgt, nrm, tree, T, max_dist)
    u = 4.0 * len(r) * 2.0**-52
    mom = {}
    for curve, switch in CURVES.items():
        with _env(PCR_QUERY_CURVE=switch):
            dc = pcp.DeviceCloud.upload(src, index.ctx).prepare(index)
            mom[curve] = index.moments(dc, T, max_d2=5.0)
            A, b, Kc, sd2 = index.point2plane_moments(dc, T, max_dist)
            dc.free()
        assert Kc == len(r)
        for i in range(6):
            for k in range(6):
                terms = J[:, i] * J[:, k]
                assert abs(A[i, k] - terms.sum()) <= u * np.abs(terms).sum(), (curve, "A", i, k)
            terms = J[:, i] * r
            assert abs(b[i] - terms.sum()) <= u * np.abs(terms).sum(), (curve, "b", i)
        assert abs(sd2 - d2.sum()) <= u * d2.sum(), curve
    (m_h, o_h, s_h), (m_m, o_m, s_m) = mom["rule"], mom["morton"]
    print("moments: largest difference between the curves", np.abs(m_h - m_m).max(), "sum d2", abs(s_h - s_m))
    assert m_h[0] == m_m[0] and np.array_equal(o_h, o_m)
    assert np.allclose(m_h, m_m, rtol=1e-11, atol=1e-9)
    assert abs(s_h - s_m) < 1e-9 * s_m


# ------------------------------------------------------------------------------------- the gate-bound tests' premise, new lay-out
def _tile_kinds(src, cell, flag):
    """(tiles made of flagged points only, mixed tiles): runs of 32 records in the order of the query curve's key.  No cell may hold
    flagged and unflagged points (equal keys = one cell: the keys are bijections of the cells)."""
    key = ck.layout_keys(src, cell)
    assert not (set(key[flag].tolist()) & set(key[~flag].tolist()))
    fl = flag[ck.layout_order(src, cell)]
    pad = (-len(fl)) % 32
    cnt = np.r_[fl, np.zeros(pad, bool)].reshape(-1, 32).sum(1)
    size = np.r_[np.full(len(cnt) - 1, 32), 32 - pad]
    return int((cnt == size).sum()), int(((cnt > 0) & (cnt < size)).sum())


def test_gate_bounds_premise_on_the_new_curve(pcp, syn, ctx):
    """The far-quarter source of tests/test_gpu_gate_bounds.py (four clumps of 100 moved points, 112 single ones) still has whole
    tiles of moved points and mixed tiles when the tiles are counted with the new key, the device order is that key's, and the
    12-pass result with the carried bounds equals the result without them."""
    src0, tgt = _scene_clouds(syn)
    index = pcp.TargetIndex(tgt, cell=CELL, ctx=ctx)
    try:
        rng = np.random.default_rng(1)
        src, flag = _replace(rng, src0, _lift(rng, src0, cKDTree(tgt), 512, 3.0, 8.0, clumps=(100, 100, 100, 100)))
        full, mixed = _tile_kinds(src, index.cell, flag)
        print("tiles of moved points only:", full, "mixed:", mixed)
        assert full >= 2 and mixed >= 2
        dc = pcp.DeviceCloud.upload(src, ctx).prepare(index)
        assert np.array_equal(dc.order(), ck.layout_order(src, index.cell))
        dc.free()
        with _env(PCR_QUERY_CURVE=None):
            on, off = _run_bounds(pcp, index, src, 12, True), _run_bounds(pcp, index, src, 12, False)
        assert on == off and on[1] == 12 and on[3] == 0
    finally:
        index.free()
