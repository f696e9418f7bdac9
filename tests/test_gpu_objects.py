"""Object batches on the device (include/pcr.h, "object batches") against the restatements of tests/objects_checks.py and the SciPy /
NumPy formulation of Final_Project/scripts/detect.py:269-354: every comparison is bit for bit, on every row.

One planted scene (objects_checks.planted_scene): 6 000 float32-rounded points at lidar scale, rows shuffled, object sizes 3, 4, 5, 63,
64, 65, 255, 256, 257, T-1, T, T+1, 2T+7 (T = the weights kernel's j stage) and 40, noise rows, an id without rows and an object of
five coincident points."""
import ctypes as C

import numpy as np
import pytest

from tests import objects_checks as chk

pytestmark = pytest.mark.gpu

CFG = {"max_radius_distance": 60.0, "num_sample_points": 64, "batch_size": 8}
SEED = 11


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(pcp):
    s = Scene()
    s.tile = pcp.objects.TILE
    s.points, s.normals, s.ids, s.k = chk.planted_scene(s.tile)
    s.offsets, s.rows = chk.restated_groups(s.ids, s.k)
    s.stats = chk.restated_stats(s.points, s.ids, s.k)
    s.w_serial = np.concatenate([chk.serial_weights(s.points[s.ids == o]) for o in range(s.k)])
    with np.errstate(invalid="ignore"):
        s.w_scipy = np.concatenate([chk.scipy_weights(s.points[s.ids == o]) if (s.ids == o).sum() > 1 else np.zeros((s.ids == o).sum()) for o in range(s.k)])
    for a in (s.points, s.normals, s.ids, s.offsets, s.rows, s.w_serial, s.w_scipy):
        a.setflags(write=False)
    return s


def check_batch(batch, s):
    """offsets, rows, stats and weights of an ObjectBatch over the scene: equal to the restatement and to SciPy / NumPy on every row."""
    assert batch.n_objects == s.k and batch.m == len(s.rows)
    assert np.array_equal(batch.offsets, s.offsets)
    assert np.array_equal(batch.rows(), s.rows)
    st = batch.stats()
    assert np.array_equal(st["count"], s.stats["count"])
    assert np.array_equal(st["mean"], s.stats["mean"], equal_nan=True)
    assert np.isnan(st["mean"][chk.UNUSED_ID]).all() and np.isnan(st["mean"]).sum() == 3
    assert np.array_equal(st["min_bound"], s.stats["min_bound"]) and np.array_equal(st["max_bound"], s.stats["max_bound"])
    for o in range(s.k):
        P = s.points[s.ids == o]
        if len(P):
            assert np.array_equal(st["mean"][o], np.mean(P, axis=0)), o
    w = batch.weights()
    assert np.array_equal(w, s.w_serial)
    assert np.array_equal(w, s.w_scipy)
    return st, w


def test_stats_offsets_rows_and_weights_equal_the_reference_bits(pcp, ctx, scene):
    s = scene
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    batch = pcp.ObjectBatch(dc, s.ids)
    try:
        st, w = check_batch(batch, s)
        # keep flags: unselected objects' rows are 0, the others unchanged
        keep = chk.restated_select(st["count"], st["mean"], CFG["max_radius_distance"])
        assert np.array_equal(pcp.objects.select(st["count"], st["mean"], CFG["max_radius_distance"]), keep)
        wk = batch.weights(keep)
        row_kept = np.repeat(keep, np.diff(s.offsets))
        assert np.array_equal(wk[row_kept], w[row_kept]) and not wk[~row_kept].any() and (~row_kept).any()
        assert not batch.weights(np.zeros(s.k, dtype=bool)).any()
    finally:
        batch.free()
        dc.free()
    # the public functions, from host arrays: float32 input gives the same cloud
    got = pcp.object_stats(s.points.astype(np.float32), s.ids)
    for key in ("count", "mean", "min_bound", "max_bound"):
        assert np.array_equal(got[key], s.stats[key], equal_nan=True), key
    by_row = np.zeros(len(s.points))
    by_row[s.rows] = s.w_serial
    assert np.array_equal(pcp.resample_weights(s.points, s.ids), by_row)
    # generating-training-set.py:186-189: the whole cloud as one object
    P = s.points[s.ids == 12]
    assert np.array_equal(pcp.resample_weights(P), chk.scipy_weights(P))


def test_relaid_cloud_gives_the_same_bits(pcp, ctx, scene, syn):
    """A cloud laid out for queries against a grid index (records along the index's curve, id = caller row)."""
    s = scene
    index = pcp.TargetIndex(np.ascontiguousarray(s.points[::2]), kind="grid", ctx=ctx)
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    try:
        dc.prepare(index)
        assert pcp._lib.lib().pcr_cloud_reordered(dc.handle) == 1
        batch = pcp.ObjectBatch(dc, s.ids)
        try:
            check_batch(batch, s)
        finally:
            batch.free()
        np.random.seed(SEED)
        want, N_want = chk.reference_preprocess(s.points, s.normals, s.ids, CFG)
        np.random.seed(SEED)
        got, N = pcp.preprocess(dc, s.ids, CFG, normals=s.normals)
        assert N == N_want and len(got) == len(want)
        for (X, o), (Xw, ow) in zip(got, want):
            assert o == ow and np.array_equal(X, Xw)
    finally:
        dc.free()
        index.free()


def test_preprocess_equals_the_reference(pcp, scene):
    s = scene
    np.random.seed(SEED)
    want, N_want = chk.reference_preprocess(s.points, s.normals, s.ids, CFG)
    state_want = np.random.get_state()
    kept = [o for _, o in want[:N_want]]
    sizes = s.stats["count"][kept]
    assert N_want % 8 != 0 and len(want) % 8 == 0 and (sizes < 64).any() and (sizes >= 64).any()
    assert 5 not in kept and chk.COINCIDENT_ID not in kept and 0 not in kept and 1 not in kept and 2 in kept

    class Pcd:   # Open3D style: .points and .normals
        points, normals = s.points, s.normals

    for arg in (Pcd, (s.points, s.normals)):
        np.random.seed(SEED)
        got, N = pcp.preprocess(arg, s.ids, CFG)
        state = np.random.get_state()
        assert N == N_want and len(got) == len(want)
        assert [o for _, o in got] == [o for _, o in want]
        for (X, _), (Xw, _) in zip(got, want):
            assert X.dtype == np.float64 and X.shape == (64, 6) and np.array_equal(X, Xw)
        assert state[0] == state_want[0] and np.array_equal(state[1], state_want[1]) and state[2:] == state_want[2:]
    # nothing kept, and labels that are all noise
    assert pcp.preprocess((s.points, s.normals), s.ids, dict(CFG, max_radius_distance=0.5)) == ([], 0)
    assert pcp.preprocess((s.points, s.normals), np.full(len(s.ids), -1), CFG) == ([], 0)


def test_preprocess_device_equals_the_reference(pcp, ctx, scene):
    import torch

    s = scene
    np.random.seed(SEED)
    want, N_want = chk.reference_preprocess(s.points, s.normals, s.ids, CFG)
    state_want = np.random.get_state()
    X_want = torch.from_numpy(np.stack([x for x, _ in want])).float()
    np.random.seed(SEED)
    X, ids, N = pcp.preprocess_device((s.points, s.normals), s.ids, CFG)
    assert np.array_equal(np.random.get_state()[1], state_want[1])
    assert X.device.type == "cuda" and X.dtype == torch.float32 and X.is_contiguous() and tuple(X.shape) == (len(want), 64, 6)
    assert N == N_want and ids.tolist() == [o for _, o in want]
    assert torch.equal(X.cpu(), X_want) and same_bits(X.cpu().numpy(), X_want.numpy())
    # without normals: (b, S, 3)
    np.random.seed(SEED)
    X3, ids3, N3 = pcp.preprocess_device((s.points, None), s.ids, CFG)
    assert tuple(X3.shape) == (len(want), 64, 3) and N3 == N and np.array_equal(ids3, ids)
    assert same_bits(X3.cpu().numpy(), np.ascontiguousarray(X_want.numpy()[:, :, :3]))
    # a device cloud with normals= ; nothing kept
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    try:
        np.random.seed(SEED)
        Xd, _, _ = pcp.preprocess_device(dc, s.ids, CFG, normals=s.normals)
        assert same_bits(Xd.cpu().numpy(), X_want.numpy())
        X0, ids0, N0 = pcp.preprocess_device(dc, s.ids, dict(CFG, max_radius_distance=0.5), normals=s.normals)
        assert tuple(X0.shape) == (0, 64, 6) and len(ids0) == 0 and N0 == 0
    finally:
        dc.free()


def test_pack_refuses_bad_indices_before_any_launch(pcp, ctx, scene):
    import torch

    s, L = scene, pcp._lib
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    batch = pcp.ObjectBatch(dc, s.ids)
    try:
        out = torch.full((2, 4, 3), 7.0, dtype=torch.float32, device=f"cuda:{ctx.device}")
        torch.cuda.synchronize()
        ok = np.zeros((2, 4), dtype=np.int64)
        for slots, idx in (([2, s.k], ok), ([2, -1], ok), ([2, 2], np.array([[0, 1, 2, 5], [0, 0, 0, 0]])), ([2, 2], np.array([[0, 1, 2, -1], [0, 0, 0, 0]])),
                           ([chk.UNUSED_ID, 2], ok)):
            with pytest.raises(L.PcrError) as e:
                batch.pack(slots, idx, out.data_ptr())
            assert e.value.status == L.PCR_E_INVALID
        assert (out.cpu() == 7.0).all()
        batch.pack([2, 2], np.array([[0, 1, 2, 4], [4, 4, 0, 0]]), out.data_ptr())
        P = s.points[s.ids == 2]
        want = (P[[0, 1, 2, 4, 4, 4, 0, 0]] - s.stats["mean"][2]).astype(np.float32).reshape(2, 4, 3)
        assert same_bits(out.cpu().numpy(), want)
        with pytest.raises(L.PcrError) as e:
            pcp.ObjectBatch(dc, s.ids, n_objects=s.k - 1)          # a label >= n_objects
        assert e.value.status == L.PCR_E_INVALID
    finally:
        batch.free()
        dc.free()


def test_coincident_points_give_zero_weights_and_numpys_error(pcp, scene):
    s = scene
    P = s.points[s.ids == chk.COINCIDENT_ID]
    w = pcp.resample_weights(P)
    assert w.shape == (5,) and same_bits(w, np.zeros(5))
    assert same_bits(pcp.resample_weights(s.points, s.ids)[s.ids == chk.COINCIDENT_ID], np.zeros(5))
    far = dict(CFG, max_radius_distance=100.0)
    with np.errstate(invalid="ignore"):
        with pytest.raises(ValueError) as e_ref:
            chk.reference_preprocess(s.points, s.normals, s.ids, far)
        with pytest.raises(ValueError) as e:
            pcp.preprocess((s.points, s.normals), s.ids, far)
    assert str(e.value) == str(e_ref.value)


def test_repeat_calls_give_identical_bytes(pcp, ctx, scene):
    s = scene
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    try:
        outs = []
        for _ in range(2):
            batch = pcp.ObjectBatch(dc, s.ids)
            st = batch.stats()
            np.random.seed(SEED)
            X, ids, N = pcp.preprocess_device(dc, s.ids, CFG, normals=s.normals)
            outs.append([batch.offsets, batch.rows(), st["count"], st["mean"], st["min_bound"], st["max_bound"], batch.weights(), X.cpu().numpy(), ids])
            batch.free()
        for a, b in zip(*outs):
            assert same_bits(a, b)
    finally:
        dc.free()


def test_scan_to_set_abstraction_end_to_end(pcp, ctx):
    """Planted ground plus four blobs: segment_and_cluster -> normals -> preprocess_device -> one PointnetSAModuleMSG forward."""
    import torch

    rng = np.random.default_rng(3)
    ground = np.column_stack([rng.uniform(0, 40, 3000), rng.uniform(-20, 20, 3000), -1.7 + rng.normal(0, 0.03, 3000)])
    centres = np.array([[8.0, -6.0, 0.5], [14.0, 5.0, 0.5], [22.0, -3.0, 0.5], [30.0, 9.0, 0.5]])
    blobs = np.concatenate([c + rng.normal(scale=0.3, size=(150, 3)) for c in centres])
    pts = np.concatenate([ground, blobs]).astype(np.float32)
    rng.shuffle(pts)
    np.random.seed(5)
    seg, labels = pcp.segment_and_cluster(pts, radius=0.5, min_pts=10)
    assert labels.max() + 1 == 4
    normals = pcp.estimate_normals_hybrid(seg, 0.5, 30)
    cfg = {"max_radius_distance": 50.0, "num_sample_points": 64, "batch_size": 4}
    X, ids, N = pcp.preprocess_device((seg, normals), labels, cfg)
    assert N == 4 and tuple(X.shape) == (4, 64, 6) and ids.tolist() == [0, 1, 2, 3] and bool(torch.isfinite(X).all())
    torch.manual_seed(0)
    sa = pcp.pointnet2_modules.PointnetSAModuleMSG(npoint=16, radii=[0.3, 0.6], nsamples=[8, 16], mlps=[[3, 8], [3, 16]], bn=False).cuda()
    with torch.no_grad():
        new_xyz, new_feats = sa(X[:, :, :3].contiguous(), X[:, :, 3:].transpose(1, 2).contiguous())
    assert tuple(new_xyz.shape) == (4, 16, 3) and tuple(new_feats.shape) == (4, 24, 16)
    assert bool(torch.isfinite(new_xyz).all()) and bool(torch.isfinite(new_feats).all())


N_MAX = 32   # loop guard: neither call takes that many blocks


@pytest.mark.parametrize("which", ["build", "weights"])
def test_refused_allocation_gives_everything_back(pcp, ctx, scene, which):
    s, L = scene, pcp._lib
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    held = pcp.ObjectBatch(dc, s.ids) if which == "weights" else None

    def call():
        if which == "weights":
            return [held.weights()]
        b = pcp.ObjectBatch(dc, s.ids)
        try:
            st = b.stats()
            return [b.offsets, b.rows(), st["count"], st["mean"], st["min_bound"], st["max_bound"]]
        finally:
            b.free()

    try:
        ctx.fail_alloc(0)
        ctx.sync()
        before = ctx.arena_live()
        want = call()
        assert ctx.arena_live() == before
        got, failures = None, 0
        for n in range(1, N_MAX + 1):
            ctx.fail_alloc(n)
            status = L.PCR_OK
            try:
                got = call()
            except L.PcrError as err:
                status = err.status
            ctx.sync()
            assert status in (L.PCR_OK, L.PCR_E_NOMEM), (n, status)
            assert ctx.arena_live() == before, (n, ctx.arena_live(), before)
            if status == L.PCR_OK:
                break
            failures += 1
        else:
            pytest.fail(f"no success with any of the first {N_MAX} allocations refused")
        assert failures >= 2
        for a, b in zip(got, want):
            assert same_bits(a, b)
    finally:
        ctx.fail_alloc(0)
        if held is not None:
            held.free()
        dc.free()
