"""GPU: FPFH at chosen rows (compute_fpfh_at_rows / pcr_fpfh_rows) against the full pass.  The rules are the full pass's own, so the
full pass is an exact oracle: "equal" below is np.array_equal on float64 arrays against compute_fpfh_feature(...).data.T[rows] from
the same context and cloud.  ``n_spfh`` is held to its restatement, tests/fpfh_rows_checks.py marked_rows."""
import numpy as np
import pytest

from oracle import oracle_global as og
from tests import fpfh_rows_checks as fr
from tests.test_gpu_global_init_paths import HYBRID_BRUTE_MAX, _check_fpfh, _clean_share, _clusters, _reordered, _unit

pytestmark = pytest.mark.gpu

NB_CAP = 1024                     # pcr_global_dev.h
RADIUS, MAX_NN = 0.12, 20         # the brute-view case
ROWS_SEED = 1


def at_rows(pcp, ctx, cloud, rows, nrm, radius, max_nn):
    f, info = pcp.compute_fpfh_at_rows(cloud, rows, nrm, radius, max_nn, ctx=ctx, return_info=True)
    assert f.data.shape == (33, len(rows)) and f.data.dtype == np.float64
    assert info["m"] == len(rows) and info["n"] == len(nrm)
    return f.data.T, info


@pytest.fixture(scope="module")
def small(pcp, syn, ctx):
    """The 1 500-point object, its normals, 40 random rows (unsorted) with three repeats appended, the full pass and the lists."""
    pts = syn.object_cloud(1500, seed=3).astype(np.float64)
    nrm = pcp.estimate_normals_hybrid(pts, RADIUS, MAX_NN, ctx=ctx)
    rng = np.random.default_rng(ROWS_SEED)
    rows40 = rng.choice(len(pts), 40, replace=False)
    assert (np.diff(rows40) < 0).any()
    rows = np.r_[rows40, rows40[[5, 0, 5]]]
    full = pcp.compute_fpfh_feature(pts, nrm, RADIUS, MAX_NN, ctx=ctx).data.T.copy()
    nbrs = og.hybrid_neighbours(pts, RADIUS, MAX_NN)
    for a in (pts, nrm, rows, full):
        a.setflags(write=False)
    return dict(pts=pts, nrm=nrm, rows40=rows40, rows=rows, full=full, nbrs=nbrs)


def test_brute_view_equals_the_full_pass(pcp, ctx, small):
    pts, nrm, rows = small["pts"], small["nrm"], small["rows"]
    assert len(pts) <= HYBRID_BRUTE_MAX
    got, info = at_rows(pcp, ctx, pts, rows, nrm, RADIUS, MAX_NN)
    assert np.array_equal(got, small["full"][rows])
    assert np.array_equal(got[40:], got[[5, 0, 5]]) and got.any()
    marked = fr.marked_rows(pts, rows, RADIUS, MAX_NN, nbrs=small["nbrs"])
    assert info["n_spfh"] == len(marked)
    assert info["n_spfh"] <= 40 * MAX_NN == 800 < info["n"] == len(pts)       # else the case could silently become the full pass


def test_rows_against_the_oracle(pcp, ctx, small):
    pts, nrm, rows40 = small["pts"], small["nrm"], small["rows40"]
    f_ref, margin = og.fpfh(pts, nrm, RADIUS, MAX_NN, nbrs=small["nbrs"], margins=True)
    clean = _clean_share(margin[rows40])                                      # a condition on the input, from the oracle alone
    assert clean.mean() >= 0.9
    got, _ = at_rows(pcp, ctx, pts, rows40, nrm, RADIUS, MAX_NN)
    _check_fpfh(got, f_ref[rows40], clean)


def test_grid_view_equals_the_full_pass(pcp, syn, ctx):
    pts = syn.kitti_like_scan(6000, seed=1)[:, :3].astype(np.float64)
    assert len(pts) > HYBRID_BRUTE_MAX
    radius, max_nn = 2.5, 30
    nrm = _unit(np.random.default_rng(8), len(pts))
    rows = np.random.default_rng(9).choice(len(pts), 64, replace=False)
    cloud = pcp.DeviceCloud.upload(pts, ctx)
    full = pcp.compute_fpfh_feature(cloud, nrm, radius, max_nn, ctx=ctx).data.T
    got, info = at_rows(pcp, ctx, cloud, rows, nrm, radius, max_nn)
    cloud.free()
    assert np.array_equal(got, full[rows]) and got.any()
    marked = fr.marked_rows(pts, rows, radius, max_nn)
    assert info["n_spfh"] == len(marked) <= 64 * max_nn < len(pts)


def _states(pcp, ctx, pts):
    """(name, cloud) for the stored states of a device cloud (tests/test_gpu_cloud_states.py): fresh upload, re-laid as the query
    cloud of a search, prepared for an index, derived on the device."""
    yield "fresh", pcp.DeviceCloud.upload(pts, ctx)
    yield "re-laid", _reordered(pcp, pts, ctx)
    index = pcp.TargetIndex(pts[::3], kind="grid", ctx=ctx)
    prepared = pcp.DeviceCloud.upload(pts, ctx).prepare(index)
    index.free()
    assert pcp._lib.lib().pcr_cloud_reordered(prepared.handle) == 1
    yield "prepared", prepared
    src = pcp.DeviceCloud.upload(pts.astype(np.float32), ctx)
    derived = pcp.voxel_filter_device(src, 0.02)
    src.free()
    yield "derived", derived


def test_every_cloud_state_gives_the_fresh_upload_s_bytes(pcp, ctx, small):
    pts, nrm, rows = small["pts"], small["nrm"], small["rows"]
    before = ctx.arena_live()
    for name, cloud in _states(pcp, ctx, pts):
        X = cloud.download()
        n = len(X)
        if name == "derived":
            assert 500 < n < len(pts)                      # voxel centroids: rows are positions on a cloud made on the device
        else:
            assert np.array_equal(X, pts), name
        r, nr = rows % n, nrm[:n]
        got, info = at_rows(pcp, ctx, cloud, r, nr, RADIUS, MAX_NN)
        fresh, info_fresh = at_rows(pcp, ctx, X, r, nr, RADIUS, MAX_NN)
        full = pcp.compute_fpfh_feature(cloud, nr, RADIUS, MAX_NN, ctx=ctx).data.T
        cloud.free()
        assert got.tobytes() == fresh.tobytes() and info == info_fresh, name
        assert np.array_equal(got, full[r]), name
        if name != "derived":
            assert got.tobytes() == small["full"][rows].tobytes(), name
    assert ctx.arena_live() == before


COUNTS = (1, 2, 3, 15, 16, 17, NB_CAP + 1)


@pytest.mark.parametrize("max_nn", [2, 16, NB_CAP])
def test_count_boundaries(pcp, ctx, max_nn):
    """Balls of 1 row (the all-zero descriptor), 2, max_nn - 1, max_nn, max_nn + 1 (at max_nn = 2 and 16) and a clump of 1 025 rows
    inside the radius (gather_hybrid's bisection): 3 .. 17 are met with max_nn below them (2, 16) and at or above them (16, 1 024),
    the clump with 2, 16 and 1 024 below it (1 024, the longest list the entry point takes: a full candidate array behind the
    bisection).  One call per ball, its centre the only row; then all centres at once through the gridded search."""
    pts, centre = _clusters(COUNTS, seed=32)
    nrm = _unit(np.random.default_rng(33), len(pts))
    d2 = ((pts[None, :, :] - pts[centre][:, None, :]) ** 2).sum(axis=2)
    assert [(row < 1.0).sum() for row in d2] == list(COUNTS)
    full = pcp.compute_fpfh_feature(pts, nrm, 1.0, max_nn, ctx=ctx).data.T
    assert not full[centre[0]].any() and full[centre[1]].any()
    for c, count in zip(centre, COUNTS):
        got, info = at_rows(pcp, ctx, pts, [c], nrm, 1.0, max_nn)
        assert np.array_equal(got, full[[c]]), (count, max_nn)
        assert 1 <= info["n_spfh"] <= min(count, max_nn), (count, max_nn)
    assert at_rows(pcp, ctx, pts, [centre[0]], nrm, 1.0, max_nn)[1]["n_spfh"] == 1
    moved = _reordered(pcp, pts, ctx)
    got, _ = at_rows(pcp, ctx, moved, centre, nrm, 1.0, max_nn)
    moved.free()
    assert np.array_equal(got, full[centre])


def test_extremes_of_m(pcp, ctx, small):
    pts, nrm, full = small["pts"], small["nrm"], small["full"]
    n = len(pts)
    one, info = at_rows(pcp, ctx, pts, [small["rows40"][0]], nrm, RADIUS, MAX_NN)
    assert np.array_equal(one, full[small["rows40"][:1]]) and 1 <= info["n_spfh"] <= MAX_NN
    every, info = at_rows(pcp, ctx, pts, np.arange(n), nrm, RADIUS, MAX_NN)
    assert np.array_equal(every, full) and info["n_spfh"] == n
    for empty in ([], np.zeros(0, dtype=np.int64)):
        none, info = at_rows(pcp, ctx, pts, empty, nrm, RADIUS, MAX_NN)
        assert none.shape == (0, 33) and info == {"n_spfh": 0, "n": n, "m": 0}


def test_errors_leave_nothing_behind(pcp, ctx, small):
    pts, nrm, rows = small["pts"], small["nrm"], small["rows"]
    L = pcp._lib
    n = len(pts)
    before = ctx.arena_live()
    for bad_rows, bad_nrm in (([n], nrm), ([-1], nrm), ([3, n, 4], nrm), (rows, nrm[:-1]), (rows, None)):
        with pytest.raises(ValueError):
            pcp.compute_fpfh_at_rows(pts, bad_rows, bad_nrm, RADIUS, MAX_NN, ctx=ctx)
    # the entry point itself refuses a bad row before it allocates
    cloud = pcp.DeviceCloud.upload(pts, ctx)
    held = ctx.arena_live()
    out = np.full((2, 33), -7.0)
    bad = np.array([5, n], dtype=np.int64)
    nr = np.ascontiguousarray(nrm)
    for r, m in ((bad, 2), (np.array([-1, 5], dtype=np.int64), 2), (bad, -1)):
        assert L.lib().pcr_fpfh_rows(ctx.handle, cloud.handle, L.dptr(nr), RADIUS, MAX_NN, L.lptr(r), m, L.dptr(out), None) == L.PCR_E_INVALID
    assert (out == -7.0).all() and ctx.arena_live() == held
    assert L.lib().pcr_fpfh_rows(ctx.handle, cloud.handle, L.dptr(nr), RADIUS, MAX_NN, L.lptr(bad), 0, L.dptr(out), None) == L.PCR_OK      # m = 0: nothing read
    assert (out == -7.0).all()
    cloud.free()
    got, _ = at_rows(pcp, ctx, pts, rows, nrm, RADIUS, MAX_NN)
    assert np.array_equal(got, small["full"][rows])
    assert ctx.arena_live() == before


def test_unbounded_neighbourhood_keeps_its_status(pcp, ctx, small):
    """1 100 copies of a point (tests/test_gpu_global_init_paths.py): PCR_E_UNSUPPORTED with the full pass's message, whether the
    chosen row is one of the copies or a row beside them (no radius bounds either's list); the fail word is clear for the call behind."""
    L = pcp._lib
    rng = np.random.default_rng(41)
    pts = np.r_[np.tile([[1.0, 2.0, 3.0]], (1100, 1)), [1.0, 2.0, 3.0] + rng.uniform(-0.5, 0.5, (6, 3))]
    nrm = _unit(rng, len(pts))
    before = ctx.arena_live()
    for rows in ([0], [1103]):
        with pytest.raises(L.PcrError) as e:
            pcp.compute_fpfh_at_rows(pts, rows, nrm, 1.0, 30, ctx=ctx)
        assert e.value.status == L.PCR_E_UNSUPPORTED
        assert b"equidistant" in L.lib().pcr_last_error(ctx.handle)
        got, _ = at_rows(pcp, ctx, small["pts"], small["rows"], small["nrm"], RADIUS, MAX_NN)
        assert np.array_equal(got, small["full"][small["rows"]])
    assert ctx.arena_live() == before


def test_repeatable_and_permutable(pcp, ctx, small):
    pts, nrm, rows = small["pts"], small["nrm"], small["rows"]
    a, ia = at_rows(pcp, ctx, pts, rows, nrm, RADIUS, MAX_NN)
    b, ib = at_rows(pcp, ctx, pts, rows, nrm, RADIUS, MAX_NN)
    assert a.tobytes() == b.tobytes() and ia == ib
    perm = np.random.default_rng(10).permutation(len(rows))
    c, ic = at_rows(pcp, ctx, pts, rows[perm], nrm, RADIUS, MAX_NN)
    assert np.array_equal(c, a[perm]) and ic == ia
    # rows as a list, as int32 and as a strided view are the same rows
    for r in (list(rows), rows.astype(np.int32), np.repeat(rows, 2)[::2]):
        assert np.array_equal(at_rows(pcp, ctx, pts, r, nrm, RADIUS, MAX_NN)[0], a)
