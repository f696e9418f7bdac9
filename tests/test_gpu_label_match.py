"""Label match on the device (include/pcr.h, "label match") against the restatement of tests/label_match_checks.py, bit for bit on every
label: the 8 result doubles and every ballot word.

One planted scene (label_match_checks.planted_scene): 1 765 float32-rounded points, rows shuffled, objects of 1, 5, 63, 64, 65, 129
and 1 003 rows, an id without rows, noise rows, and 72 labels in ONE call (more than a wave's width): the label file's, a sphere without
rows, rows in the sphere but none in the box, equal votes (across the kernel's waves and within one), a winner with more in-sphere rows
than votes, spheres at the pruning edge (an empty corner of an object's box, one ulp short of a box, exactly touching one), two
labels on one object, non-zero yaw.  A second scene under the identity calibration has rows exactly ON a sphere and ON box faces.  Then
``process_sample`` over a synthetic street."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from tests import kitti_boxes_checks as kchk
from tests import label_match_checks as chk

pytestmark = pytest.mark.gpu

_u64p = C.POINTER(C.c_uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class Scene:
    pass


@pytest.fixture(scope="module")
def scene():
    s = Scene()
    s.points, s.ids, s.k, s.records, s.names = chk.planted_scene()
    s.words = chk.words_needed(s.ids, s.k)
    s.result, s.bits = chk.restated_match(s.points, s.ids, s.k, chk.CALIB, s.records, s.words)
    for a in (s.points, s.ids, s.records, s.result, s.bits):
        a.setflags(write=False)
    return s


def raw_match(pcp, ctx, batch, calib, records, words, want_bits=True, fill=7.0):
    """The C entry point itself -> (status, result, bits): the outputs start out filled, so unwritten entries show."""
    L = pcp._lib
    records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 16)
    n = len(records)
    result = np.full((n, 8), fill)
    bits = np.full((n, max(words, 0)), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = L.lib().pcr_objects_match_labels(ctx.handle, batch.handle, C.byref(pcp.objects.calib_struct(calib)), L.dptr(records) if n else None, n, L.dptr(result),
                                          bits.ctypes.data_as(_u64p) if want_bits else None, words)
    return rc, result, bits


def check_against(got_result, got_bits, want_result, want_bits, names):
    for l, name in enumerate(names):
        assert same_bits(got_result[l], want_result[l]), (name, got_result[l], want_result[l])
        assert same_bits(got_bits[l], want_bits[l]), (name, got_bits[l], want_bits[l])


def test_result_and_ballot_words_equal_the_restatement_bit_for_bit(pcp, ctx, scene):
    s = scene
    L = pcp._lib
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    batch = pcp.ObjectBatch(dc, s.ids, n_objects=s.k)
    try:
        before = ctx.arena_live()
        rc, result, bits = raw_match(pcp, ctx, batch, chk.CALIB, s.records, s.words)
        assert rc == L.PCR_OK and len(s.records) == 72
        check_against(result, bits, s.result, s.bits, s.names)
        assert ctx.arena_live() == before
        # two calls, identical bits; without the words the result is the same
        rc2, result2, bits2 = raw_match(pcp, ctx, batch, chk.CALIB, s.records, s.words)
        assert rc2 == L.PCR_OK and same_bits(result2, result) and same_bits(bits2, bits)
        rc3, result3, bits3 = raw_match(pcp, ctx, batch, chk.CALIB, s.records, 0, want_bits=False)
        assert rc3 == L.PCR_OK and same_bits(result3, result)
        # more words than needed: the extra ones are written, with zero
        rc4, result4, bits4 = raw_match(pcp, ctx, batch, chk.CALIB, s.records, s.words + 3)
        assert rc4 == L.PCR_OK and same_bits(result4, result) and same_bits(bits4[:, :s.words], bits) and not bits4[:, s.words:].any()
        # one label at a time gives the rows of the batch call (the launch shape does not matter)
        for l in (0, 9, 12, 14, 40):
            rc5, r5, b5 = raw_match(pcp, ctx, batch, chk.CALIB, s.records[l], s.words)
            assert rc5 == L.PCR_OK and same_bits(r5[0], result[l]) and same_bits(b5[0], bits[l])
        # the Python layer
        m = batch.match_labels(chk.CALIB, s.records)
        assert sorted(m) == ["center", "count", "k", "object_id", "positions", "rows", "votes"]
        assert all(m[key].dtype == np.int64 for key in ("k", "object_id", "votes", "count")) and m["center"].shape == (72, 3)
        assert m["k"].tolist() == s.result[:, 0].astype(int).tolist() and m["object_id"].tolist() == s.result[:, 1].astype(int).tolist()
        assert m["votes"].tolist() == s.result[:, 2].astype(int).tolist() and m["count"].tolist() == s.result[:, 3].astype(int).tolist()
        assert same_bits(m["center"], s.result[:, 4:7])
        for l in range(72):
            want = chk.positions_of(s.bits[l])
            assert m["positions"][l].dtype == np.int64 and np.array_equal(m["positions"][l], want)
            o = int(s.result[l, 1])
            assert np.array_equal(m["rows"][l], np.flatnonzero(s.ids == o)[want] if o >= 0 else [])
    finally:
        batch.free()
        dc.free()


def test_exact_boundaries_under_the_identity_calibration(pcp, ctx):
    points, ids, k, records, names = chk.identity_scene()
    want_result, want_bits = chk.restated_match(points, ids, k, chk.IDENTITY, records, 1)
    dc = pcp.DeviceCloud.upload(points, ctx)
    batch = pcp.ObjectBatch(dc, ids, n_objects=k)
    try:
        rc, result, bits = raw_match(pcp, ctx, batch, chk.IDENTITY, records, 1)
        assert rc == pcp._lib.PCR_OK
        check_against(result, bits, want_result, want_bits, names)
        assert int(bits[0, 0]) & 1 and result[0, 2] == 2.0          # the row (3, 4, 0), r = 5: on the sphere and on two faces, included
        assert result[1, 2] == 3.0                                  # the row on three faces votes
    finally:
        batch.free()
        dc.free()


def test_prepared_moved_and_reordered_clouds_give_the_same_bits(pcp, ctx, scene):
    s = scene
    index = pcp.TargetIndex(np.ascontiguousarray(s.points[::2]), kind="grid", ctx=ctx)
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    batch = moved = None
    try:
        dc.prepare(index)
        assert pcp._lib.lib().pcr_cloud_reordered(dc.handle) == 1
        batch = pcp.ObjectBatch(dc, s.ids, n_objects=s.k)
        rc, result, bits = raw_match(pcp, ctx, batch, chk.CALIB, s.records, s.words)
        assert rc == pcp._lib.PCR_OK
        check_against(result, bits, s.result, s.bits, s.names)
        # moved: the restatement over the coordinates the device now holds
        # (a rotation: the moved coordinates use all 53 bits, so -- unlike sums of float32-rounded values, which are exact in any
        # order -- the centre now depends on the order of the object sum)
        c, sn = np.cos(0.01), np.sin(0.01)
        T = np.array([[c, -sn, 0.0, 0.25], [sn, c, 0.0, -0.5], [0.0, 0.0, 1.0, 0.125], [0.0, 0.0, 0.0, 1.0]])
        dc.transform(T)
        P = dc.download()
        assert not np.array_equal(P, P.astype(np.float32).astype(np.float64))
        moved = pcp.ObjectBatch(dc, s.ids, n_objects=s.k)
        want_result, want_bits = chk.restated_match(P, s.ids, s.k, chk.CALIB, s.records, s.words)
        assert not same_bits(want_result, s.result)
        big = int(np.argmax(want_result[:, 3]))
        plain = P[np.flatnonzero(s.ids == int(want_result[big, 1]))[chk.positions_of(want_bits[big])]].mean(axis=0)
        assert want_result[big, 3] > 500 and not same_bits(plain, want_result[big, 4:7])      # the order shows in the bits
        rc, result, bits = raw_match(pcp, ctx, moved, chk.CALIB, s.records, s.words)
        assert rc == pcp._lib.PCR_OK
        check_against(result, bits, want_result, want_bits, s.names)
    finally:
        for b in (batch, moved):
            if b is not None:
                b.free()
        dc.free()
        index.free()


def test_edges_and_invalid_arguments_leave_the_arena_balanced(pcp, ctx, scene):
    s = scene
    L = pcp._lib
    f = L.lib().pcr_objects_match_labels
    dc = pcp.DeviceCloud.upload(s.points, ctx)
    batch = pcp.ObjectBatch(dc, s.ids, n_objects=s.k)
    unlabelled = pcp.ObjectBatch(dc, np.full(len(s.ids), -1), n_objects=3)
    try:
        cal = pcp.objects.calib_struct(chk.CALIB)
        before = ctx.arena_live()
        # L == 0
        rc, result, bits = raw_match(pcp, ctx, batch, chk.CALIB, np.zeros((0, 16)), s.words)
        assert rc == L.PCR_OK and result.shape == (0, 8)
        m = batch.match_labels(chk.CALIB, np.zeros((0, 16)))
        assert m["k"].shape == (0,) and m["center"].shape == (0, 3) and m["positions"] == [] and m["rows"] == []
        # a handle without labelled rows: every label k = 0, winner -1, every word zero
        rc, result, bits = raw_match(pcp, ctx, unlabelled, chk.CALIB, s.records[:5], 2)
        assert rc == L.PCR_OK and not bits.any()
        assert (result[:, 0] == 0).all() and (result[:, 1] == -1).all() and not result[:, 2:4].any() and np.isnan(result[:, 4:7]).all() and not result[:, 7].any()
        assert ctx.arena_live() == before
        # refused before any launch: nothing is written
        good = s.records[:3]

        def refused(records, words=s.words, objs=batch.handle, calib=cal, null_result=False, n=None):
            records = np.ascontiguousarray(records)
            out = np.full((len(records), 8), 7.0)
            bits = np.full((len(records), max(words, 1)), 5, dtype=np.uint64)
            rc = f(ctx.handle, objs, C.byref(calib) if calib is not None else None, L.dptr(records) if records is not None else None,
                   len(records) if n is None else n, None if null_result else L.dptr(out), bits.ctypes.data_as(_u64p), words)
            assert ctx.arena_live() == before and (out == 7.0).all() and (bits == 5).all()
            return rc

        assert refused(good, words=s.words - 1) == L.PCR_E_INVALID          # too few words for the 1 003-row object
        assert refused(good, words=-1) == L.PCR_E_INVALID
        assert refused(good, objs=None) == L.PCR_E_INVALID and refused(good, calib=None) == L.PCR_E_INVALID
        assert refused(good, null_result=True) == L.PCR_E_INVALID and refused(good, n=-1) == L.PCR_E_INVALID
        assert f(ctx.handle, batch.handle, C.byref(cal), None, 2, L.dptr(np.zeros(16)), None, 0) == L.PCR_E_INVALID      # labels NULL with L > 0
        for col, bad in ((0, np.nan), (3, -1.0), (3, np.inf), (5, np.nan), (7, np.inf), (9, -0.5), (10, -1e-300), (11, np.nan), (12, 1.0), (15, np.nan)):
            r = good.copy()
            r[1, col] = bad
            assert refused(r) == L.PCR_E_INVALID, (col, bad)
            with pytest.raises(L.PcrError):
                batch.match_labels(chk.CALIB, r)
        for key, bad in (("R0_rect", np.inf), ("Tr_velo_to_cam", np.nan)):
            mat = chk.CALIB[key].copy()
            mat[-1, -1] = bad
            assert refused(good, calib=pcp.objects.calib_struct(dict(chk.CALIB, **{key: mat}))) == L.PCR_E_INVALID
        with pytest.raises(ValueError, match="label records"):
            batch.match_labels(chk.CALIB, np.zeros((3, 15)))
        # and a good call after them
        rc, result, bits = raw_match(pcp, ctx, batch, chk.CALIB, s.records, s.words)
        assert rc == L.PCR_OK and same_bits(result, s.result) and same_bits(bits, s.bits) and ctx.arena_live() == before
    finally:
        unlabelled.free()
        batch.free()
        dc.free()


def street_labels(points, planted):
    """One KITTI label row per planted box of the synthetic street, drawn generously round it (5 x 3 x 5 m), and one over empty road."""
    rows = []
    for b, kind in enumerate(["Car", "Pedestrian", "Cyclist", "Van", "Misc", "Truck"]):
        c = kchk.restated_cam(points[planted == b], kchk.CALIB).mean(axis=0)
        rows.append([kind, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0, 5.0, 5.0, round(c[0], 2), round(c[1] + 1.5, 2), round(c[2], 2), round(0.3 * b - 0.7, 2)])
    rows.append(["Car", 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5, 1.6, 3.9, 0.0, 1.7, 70.0, 0.1])
    rows.append(["DontCare", -1, -1, -10, 0.0, 0.0, 0.0, 0.0, -1, -1, -1, -1000, -1000, -1000, -10])
    return "".join(" ".join(str(v) for v in row) + "\n" for row in rows)


def test_process_sample_writes_what_match_labels_implies(pcp, ctx, tmp_path):
    points, planted = kchk.synthetic_street()
    samples = np.random.default_rng(4).integers(0, 2**31, size=(1000, 3))
    label_file = tmp_path / "000000.txt"
    label_file.write_text(street_labels(points, planted))
    df = pcp.read_label(str(label_file), kchk.CALIB)
    assert len(df) == 7
    # the pieces, by hand
    _, objects, object_ids = pcp.segment_ground_and_objects(points.astype(np.float32), samples=samples, ctx=ctx)
    try:
        m = pcp.match_labels(objects, object_ids, df, kchk.CALIB, ctx=ctx)
        want_result, want_bits = chk.restated_match(objects.points.astype(np.float64), object_ids, int(object_ids.max()) + 1, kchk.CALIB, pcp.label_records(df),
                                                    chk.words_needed(object_ids, int(object_ids.max()) + 1))
        assert m["object_id"].tolist() == want_result[:, 1].astype(int).tolist() and same_bits(m["center"], want_result[:, 4:7])
        assert (m["object_id"][:6] >= 0).all() and len(set(m["object_id"][:6].tolist())) == 6 and m["object_id"][6] == -1
        for l in range(6):     # every planted box is found whole: the label is larger than the box
            assert m["count"][l] == (object_ids == m["object_id"][l]).sum() == m["votes"][l]
            assert np.array_equal(m["rows"][l], np.flatnonzero(object_ids == m["object_id"][l]))
        obj_points, obj_normals = objects.points.astype(np.float64), np.asarray(objects.normals, dtype=np.float64)
    finally:
        objects.free()
    # the whole pass
    out_dir = tmp_path / "out"
    dataset_label = {c: pcp.init_label() for c in ("vehicle", "pedestrian", "cyclist", "misc")}
    random.seed(11)
    paths = pcp.process_sample(points.astype(np.float32), kchk.CALIB, df, dataset_label, str(out_dir), samples=samples, ctx=ctx)
    category = ["vehicle", "pedestrian", "cyclist", "vehicle", "misc", "vehicle"]
    running = {c: 0 for c in dataset_label}
    for l in range(6):
        running[category[l]] += 1
        path = os.path.join(str(out_dir), category[l], f"{running[category[l]]:06d}.txt")
        assert paths[l] == path
        got = np.loadtxt(path, delimiter=",", ndmin=2)
        rows = m["rows"][l]
        assert got.shape == (len(rows), 6) and np.array_equal(got, np.hstack([obj_points[rows], obj_normals[rows]]))
    assert dataset_label["vehicle"]["type"] == ["Car", "Van", "Truck"] and dataset_label["vehicle"]["num_measurements"] == [int(m["count"][l]) for l in (0, 3, 5)]
    assert dataset_label["pedestrian"]["type"] == ["Pedestrian"] and dataset_label["cyclist"]["ry"] == [df.iloc[2]["ry"]]
    centre = np.column_stack([dataset_label["vehicle"][key] for key in ("vx", "vy", "vz")])
    assert same_bits(centre, m["center"][[0, 3, 5]])
    # the misc draw: random.sample over the ids no label chose, in np.unique's order (the noise id among them), at most three
    candidates = [i for i in np.unique(object_ids) if i not in set(m["object_id"][:6].tolist())]
    random.seed(11)
    drawn = random.sample(candidates, min(3, len(candidates)))
    assert len(paths) == 6 + len(drawn) and dataset_label["misc"]["type"] == ["Misc"] + ["Unknown"] * len(drawn)
    for j, o in enumerate(drawn):
        got = np.loadtxt(paths[6 + j], delimiter=",", ndmin=2)
        assert paths[6 + j] == os.path.join(str(out_dir), "misc", f"{2 + j:06d}.txt") and np.array_equal(got[:, :3], obj_points[object_ids == o])
        assert dataset_label["misc"]["num_measurements"][1 + j] == (object_ids == o).sum()
    # without a directory the frames come back
    dataset_label = {c: pcp.init_label() for c in ("vehicle", "pedestrian", "cyclist", "misc")}
    random.seed(11)
    frames = pcp.process_sample(points.astype(np.float32), kchk.CALIB, df, dataset_label, samples=samples, ctx=ctx)
    assert [f[:2] for f in frames[:6]] == [("vehicle", 1), ("pedestrian", 1), ("cyclist", 1), ("vehicle", 2), ("misc", 1), ("vehicle", 3)]
    assert list(frames[0][2].columns) == ["vx", "vy", "vz", "nx", "ny", "nz"] and np.array_equal(frames[0][2].values[:, :3], obj_points[m["rows"][0]])
