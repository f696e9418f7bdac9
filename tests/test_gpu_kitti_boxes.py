"""KITTI boxes on the device (include/pcr.h, "KITTI boxes") against the restatement of tests/kitti_boxes_checks.py, bit for bit on every
object, and against the recorded reference results of tests/golden/kitti_boxes.npz at the tolerance of tests/test_kitti_boxes_host.py.

One planted scene (kitti_boxes_checks.planted_scene): 3 896 float32-rounded points inside the detector's field of view, rows shuffled,
object sizes 1, 2, 5, 63, 64, 65, 127, 128, 129, L-1, L, L+1, 2L+7 (L = PCR_KITTI_LDS_ROWS: both sides of the on-chip branch), five
coincident points, an id without rows, an axis-aligned box and noise rows.  Then one pass scan -> objects -> batch -> classifier ->
label rows over a synthetic street."""
import ctypes as C

import numpy as np
import pytest

from tests import kitti_boxes_checks as chk
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-9


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(pcp):
    s = Scene()
    s.rows = pcp.detection.LDS_ROWS
    s.points, s.ids, s.k = chk.planted_scene(s.rows)
    s.boxes = chk.restated_boxes(s.points, s.ids, s.k, chk.CALIB)
    for a in (s.points, s.ids, s.boxes):
        a.setflags(write=False)
    return s


def boxes_of(pcp, cloud, ids, keep=None):
    batch = pcp.ObjectBatch(cloud, ids)
    try:
        return batch.kitti_boxes(chk.CALIB, keep)
    finally:
        batch.free()


def test_boxes_equal_the_restatement_bit_for_bit(pcp, ctx, scene):
    s = scene
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    try:
        got = boxes_of(pcp, dc, s.ids)
        assert got.shape == (s.k, 16)
        for o in range(s.k):
            assert same_bits(got[o], s.boxes[o]), (o, got[o], s.boxes[o])
        assert np.isnan(got[chk.UNUSED_ID, :15]).all() and got[chk.UNUSED_ID, 15] == 0.0
        assert got[:, 15].max() > s.rows >= got[:, 15][got[:, 15] > 0].min()       # both sides of the on-chip branch ran
        # two calls, identical bits
        assert same_bits(boxes_of(pcp, dc, s.ids), got)
        # keep flags: unkept objects are NaN up to the count, the others unchanged
        keep = np.arange(s.k) % 3 != 1
        gk = boxes_of(pcp, dc, s.ids, keep)
        assert same_bits(gk[keep], got[keep]) and np.isnan(gk[~keep][:, :15]).all() and np.array_equal(gk[:, 15], got[:, 15])
        none = boxes_of(pcp, dc, s.ids, np.zeros(s.k, dtype=bool))
        assert np.isnan(none[:, :15]).all() and np.array_equal(none[:, 15], got[:, 15])
        # the public functions: float32 input is the same cloud
        ob = pcp.object_boxes(s.points.astype(np.float32), s.ids, chk.CALIB, ctx=ctx)
        assert same_bits(ob["center"], got[:, 7:10]) and same_bits(ob["ry"], np.arctan2(got[:, 11], got[:, 10])) and same_bits(ob["height"], got[:, 4])
        assert ob["count"].tolist() == got[:, 15].astype(int).tolist()
        ob2 = pcp.object_boxes(dc, s.ids, chk.CALIB)
        assert all(same_bits(ob[key], ob2[key]) for key in ob)
    finally:
        dc.free()


def test_relaid_and_derived_clouds_give_the_same_bits(pcp, ctx, scene):
    """The grouped order is by caller row: a cloud laid out along a grid index's curve, and a cloud that is the device output of
    ground_segmentation, must give the bits of the plain upload."""
    s = scene
    index = pcp.TargetIndex(np.ascontiguousarray(s.points[::2]), kind="grid", ctx=ctx)
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    try:
        dc.prepare(index)
        assert pcp._lib.lib().pcr_cloud_reordered(dc.handle) == 1
        assert same_bits(boxes_of(pcp, dc, s.ids), s.boxes)
    finally:
        dc.free()
        index.free()
    # a plane of 300 points far below the scene, interleaved with its rows; the plane's own triples remove exactly the plane
    rng = np.random.default_rng(3)
    n, n_plane = len(s.points), 300
    is_plane = np.zeros(n + n_plane, dtype=bool)
    is_plane[rng.choice(n + n_plane, size=n_plane, replace=False)] = True
    ext = np.empty((n + n_plane, 3))
    ext[~is_plane] = s.points
    ext[is_plane] = np.column_stack([rng.uniform(5, 70, n_plane), rng.uniform(-25, 25, n_plane), np.full(n_plane, -9.0)]).astype(np.float32)
    samples = rng.choice(np.flatnonzero(is_plane), size=(8, 3))
    src = pcp.DeviceCloud.upload(ext, ctx)
    out = None
    try:
        out, info = pcp.ground_segmentation(src, 0.05, len(samples), 0.5, samples=samples, return_info=True)
        assert np.array_equal(info["outlier_rows"], np.flatnonzero(~is_plane)) and out.n == n
        assert same_bits(boxes_of(pcp, out, s.ids), s.boxes)
    finally:
        src.free()
        if out is not None:
            out.free()


def test_against_the_recorded_reference(pcp, ctx, scene):
    s = scene
    g = load_golden("kitti_boxes.npz")
    assert np.array_equal(g["points"].astype(np.float64), s.points) and np.array_equal(g["ids"], s.ids)
    got = pcp.object_boxes(s.points, s.ids, {k: g[k] for k in ("P2", "R0_rect", "Tr_velo_to_cam")}, ctx=ctx)
    present = g["object_ids"]
    fields = np.column_stack([got[f] for f in chk.FIELDS[:7]] + [got["center"], got["ry"]])[present]
    well = chk.conditioning(s.boxes)[present] >= 1e-3
    distinct = np.array([len(np.unique(s.points[s.ids == o], axis=0)) for o in present])
    assert well[distinct >= 5].all()
    err = np.abs(fields - g["fields"])
    print("worst error per field", dict(zip(chk.FIELDS, err.max(axis=0))))
    always = [0, 1, 2, 3, 7, 8, 9]
    assert err[:, always].max() < TOL and err[well].max() < TOL
    strings = np.array([[f"{x:.2f}" for x in row] for row in fields])
    assert (strings == g["strings"]).all()


def test_no_objects_and_invalid_arguments_leave_the_arena_balanced(pcp, ctx, scene):
    s = scene
    L = pcp._lib
    f = L.lib().pcr_objects_kitti_boxes
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    batch = pcp.ObjectBatch(dc, s.ids)
    empty = pcp.ObjectBatch(dc, np.full(len(s.ids), -1), n_objects=0)
    try:
        cal = pcp.objects.calib_struct(chk.CALIB)
        out = np.full((s.k, 16), 7.0)
        before = ctx.arena_live()
        # no objects: PCR_OK, nothing written
        assert empty.n_objects == 0 and empty.kitti_boxes(chk.CALIB).shape == (0, 16)
        assert f(ctx.handle, empty.handle, C.byref(cal), None, L.dptr(out)) == L.PCR_OK and (out == 7.0).all()
        assert ctx.arena_live() == before
        for args in ((None, C.byref(cal), L.dptr(out)), (batch.handle, None, L.dptr(out)), (batch.handle, C.byref(cal), None)):
            assert f(ctx.handle, args[0], args[1], None, args[2]) == L.PCR_E_INVALID
            assert ctx.arena_live() == before and (out == 7.0).all()
        for key, bad in (("P2", np.nan), ("R0_rect", np.inf), ("Tr_velo_to_cam", -np.inf)):
            m = chk.CALIB[key].copy()
            m[-1, -1] = bad
            assert f(ctx.handle, batch.handle, C.byref(pcp.objects.calib_struct(dict(chk.CALIB, **{key: m}))), None, L.dptr(out)) == L.PCR_E_INVALID
            assert ctx.arena_live() == before and (out == 7.0).all()
            with pytest.raises(L.PcrError):
                batch.kitti_boxes(dict(chk.CALIB, **{key: m}))
        with pytest.raises(ValueError, match="keep flags"):
            batch.kitti_boxes(chk.CALIB, np.ones(s.k + 1, dtype=bool))
        # and a good call after them
        assert f(ctx.handle, batch.handle, C.byref(cal), None, L.dptr(out)) == L.PCR_OK and same_bits(out, s.boxes)
        assert ctx.arena_live() == before
    finally:
        empty.free()
        batch.free()
        dc.free()


class FixedLogits:
    """A classifier that answers every batch with the same logits: slot i of a batch is class i % 4, with a known confidence."""

    def __init__(self, batch_size, device):
        import torch

        rows = np.full((batch_size, 4), -1.0, dtype=np.float32)
        rows[np.arange(batch_size), np.arange(batch_size) % 4] = 2.0
        self.logits = torch.from_numpy(rows).to(device)
        self.calls = 0

    def __call__(self, X):
        self.calls += 1
        assert X.shape[0] == self.logits.shape[0] and X.shape[2] == 6
        return self.logits


def test_scan_to_label_rows_on_a_synthetic_street(pcp, ctx):
    import torch

    points, planted = chk.synthetic_street()
    samples = np.random.default_rng(4).integers(0, 2**31, size=(1000, 3))
    ground, objects, labels = pcp.segment_ground_and_objects(points.astype(np.float32), samples=samples, ctx=ctx)
    try:
        # the plane is the planted one
        model = objects.ground_model
        normal = model[:3] * np.sign(model[2])
        angle = np.degrees(np.arccos(min(1.0, float(normal @ chk.STREET_NORMAL))))
        print("plane angle to the planted one (deg)", angle, "offset", model[3] * np.sign(model[2]))
        assert angle < 2.0 and abs(np.linalg.norm(normal) - 1.0) < 1e-12
        assert len(ground) > 0.8 * chk.STREET_GROUND
        # the objects are the rows outside the band and inside the field of view, uploaded once
        dist = np.abs(points @ model[:3] + model[3])
        kept = np.flatnonzero((dist > 0.30) & (points[:, 0] >= 1.95) & (points[:, 0] <= 80.0) & (np.abs(points[:, 1]) <= 30.0))
        assert np.array_equal(objects.points, points[kept].astype(np.float32)) and objects.normals.shape == (len(kept), 3)
        assert objects.cloud.n == len(kept) == len(labels) and np.array_equal(objects.cloud.download(), points[kept])
        # every planted box comes back as one object, short of the points it lost to the 0.30 m band
        box_of_object = {}
        for b, size in enumerate(chk.STREET_BOX_SIZES):
            mine = labels[planted[kept] == b]
            lost = size - len(mine)
            assert 0 <= lost == ((planted == b) & (dist <= 0.30)).sum() and lost < 0.15 * size, (b, lost)
            assert len(set(mine.tolist())) == 1 and mine[0] >= 0, (b, set(mine.tolist()))
            assert (labels == mine[0]).sum() == len(mine), b      # and nothing else joined it
            box_of_object[int(mine[0])] = b
        assert len(box_of_object) == 6
        # batch -> classifier -> label rows
        config = {"max_radius_distance": 100.0, "num_sample_points": 32, "batch_size": 4, "num_classes": 4}
        decoder = {0: "cyclist", 1: "misc", 2: "pedestrian", 3: "vehicle"}
        stub = FixedLogits(4, torch.device("cuda", ctx.device))
        np.random.seed(1)
        X, ids, N = pcp.preprocess_device(objects.cloud, labels, config, ctx, normals=objects.normals)
        predictions = pcp.predict(X, ids, N, stub, config)
        assert N >= 6 and stub.calls == -(-N // 4) and sum(len(v) for v in predictions.values()) == N
        label = pcp.to_kitti_eval_format(objects, labels, chk.CALIB, predictions, decoder)
        non_misc = [(c, o) for c in predictions if decoder[c] != "misc" for o in predictions[c]]
        assert len(label) == len(non_misc) >= 3 and len(predictions[1]) >= 1
        assert label["type"].tolist() == [{"cyclist": "Cyclist", "pedestrian": "Pedestrian", "vehicle": "Car"}[decoder[c]] for c, _ in non_misc]
        conf = float(torch.softmax(stub.logits, dim=1).max().cpu())
        assert set(label["score"]) == {f"{100.0 * conf:.2f}"}
        checked = 0
        for r, (c, o) in enumerate(non_misc):
            if int(o) not in box_of_object:
                continue
            mean = pcp.transform_to_cam(points[planted == box_of_object[int(o)]], chk.CALIB).mean(axis=0)
            got = np.array([float(label[key][r]) for key in ("cx", "cy", "cz")])
            print("box", box_of_object[int(o)], "centre error", np.abs(got - mean))
            assert np.abs(got - mean).max() < 0.05
            checked += 1
        assert checked >= 3
        # detect() is the same pass
        np.random.seed(1)
        again = pcp.detect(FixedLogits(4, torch.device("cuda", ctx.device)), points.astype(np.float32), chk.CALIB, config, decoder, samples=samples, ctx=ctx)
        assert again.equals(label)
    finally:
        objects.free()
