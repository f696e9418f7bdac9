"""Host side of the label match (include/pcr.h, "label match"; Final_Project/scripts/extract.py:86-387 and :506-574): the restatement
of tests/label_match_checks.py against what the reference's own functions recorded in tests/golden/label_match.npz, and ``read_label``,
the frame transforms and ``get_object_category`` of extract.py against the same file.  No GPU needed.

Tolerance against the golden: integers (k, object id, count) are equal; the centre is within 1e-9, the project's TOL for reference
formulations -- the two differ by summation order only, below 1e-10 at these sizes (the test prints the worst).  The recorded labels
keep every row at least 1e-6 m from a sphere and from a box face (``min_margin`` in the file), so no rounding of the reference's BLAS
decides a membership; the exact-boundary labels are checked against the restatement itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import label_match_checks as chk
from tests.conftest import GOLDEN, ROOT, load_golden

TOL = 1e-9


@pytest.fixture(scope="module")
def gold():
    g = load_golden("label_match.npz")
    calib = {k: g[k] for k in ("P2", "R0_rect", "Tr_velo_to_cam")}
    return g, calib, g["points"].astype(np.float64), g["ids"].astype(np.int64), int(g["n_objects"])


@pytest.fixture(scope="module")
def scene():
    points, ids, k, records, names = chk.planted_scene()
    words = chk.words_needed(ids, k)
    result, bits = chk.restated_match(points, ids, k, chk.CALIB, records, words)
    for a in (points, ids, records, result, bits):
        a.setflags(write=False)
    return points, ids, k, records, names, words, result, bits


def test_new_symbol_exported_with_its_signature(pcp):
    L = pcp._lib
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    assert re.search(r"PCR_API\s+int\s+pcr_objects_match_labels\s*\(", header)
    assert "pcr_objects_match_labels" in L.SIGNATURES and hasattr(L.lib(), "pcr_objects_match_labels")
    assert int(re.search(r"#define\s+PCR_LABEL_DOUBLES\s+(\d+)", header).group(1)) == L.PCR_LABEL_DOUBLES == chk.LABEL_DOUBLES
    assert int(re.search(r"#define\s+PCR_LABEL_RESULT_DOUBLES\s+(\d+)", header).group(1)) == L.PCR_LABEL_RESULT_DOUBLES == chk.RESULT_DOUBLES
    assert "UNPINNED" in header[header.index("label match"):header.index("PCR_LABEL_DOUBLES")]      # the boundary rule at exact equality
    for name in ("read_label", "transform_from_cam_to_velo", "transform_from_velo_to_obj", "filter_by_bouding_box", "get_object_category", "init_label",
                 "add_label", "get_object_pcd_df", "match_labels", "process_sample"):
        assert callable(getattr(pcp, name)) and getattr(pcp, name) is getattr(pcp.extract, name), name
    assert callable(pcp.ObjectBatch.match_labels)


def test_entry_point_refuses_null_arguments_without_a_device(pcp):
    L = pcp._lib
    f = L.lib().pcr_objects_match_labels
    cal = L.KittiCalib()
    rec, out = np.zeros(16), np.zeros(8)
    assert f(None, None, C.byref(cal), L.dptr(rec), 1, L.dptr(out), None, 0) == L.PCR_E_INVALID


def test_golden_scene_is_the_planted_scene(gold, scene):
    g, calib, points, ids, k = gold
    P, I, K, records, names, words, result, bits = scene
    assert K == k == chk.N_OBJECTS and np.array_equal(P, points) and np.array_equal(I, ids)
    for key in calib:
        assert np.array_equal(calib[key], chk.CALIB[key]), key
    assert np.array_equal(points, points.astype(np.float32).astype(np.float64))
    count = np.bincount(ids[ids >= 0], minlength=k)
    assert [int(count[o]) for o in range(7)] == [1, 5, 63, 64, 65, 129, 1003] and count[chk.UNUSED_ID] == 0 and (ids == -1).sum() == chk.N_NOISE
    assert words == 16 and np.any(np.diff(np.flatnonzero(ids == 6)) > 1)       # shuffled: objects interleave
    assert len(records) == 72 > 64 and len(names) == 72
    assert os.path.getsize(os.path.join(GOLDEN, "label_match.npz")) < 100_000
    assert open(os.path.join(GOLDEN, "label_match_label.txt")).read() == chk.label_text()
    assert float(g["min_margin"]) > 1e-6


def test_planted_labels_reach_the_cases_they_are_meant_for(scene):
    points, ids, k, records, names, words, result, bits = scene
    row = {name: result[i] for i, name in enumerate(names)}
    assert result[:chk.N_TABLE, 1].astype(int).tolist() == chk.TABLE_WINNER
    assert row["table7"][0] == 0 and row["table7"][1] == -1                                  # (a) a sphere without rows
    assert row["table12"][0] > 0 and row["table12"][1] == -1 and np.isnan(row["table12"][4:7]).all()   # (b) rows in the sphere, none in the box
    votes = lambda name, o: int((np.logical_and(*chk.memberships(points[ids == o], chk.CALIB, records[names.index(name)]))).sum())  # noqa: E731
    assert votes("table10", 8) == votes("table10", 9) == 6 and row["table10"][1] == 8        # (c) equal votes in two waves' objects
    assert votes("table11", 9) == votes("table11", 13) == 4 and row["table11"][1] == 9       #     and within one wave's objects
    assert row["table0"][3] > row["table0"][2] > 0                                           # (d) more rows in the sphere than votes
    assert row["corner_of_box_no_rows"][0] == 0 and row["just_short_of_box"][0] == 0         # (e) the pruning edge
    lo, hi = points[ids == 10].min(axis=0), points[ids == 10].max(axis=0)
    v = records[names.index("corner_of_box_no_rows")][:3]
    assert (lo <= v).all() and (v <= hi).all()                                               #     the centre is inside object 10's box
    assert row["touching_box"][0] == 1 and row["zero_radius_on_a_row"][0] == 1
    assert row["everything"][0] == (ids >= 0).sum() and row["everything"][1] == -1
    assert row["table4"][1] == row["table9"][1] == 5                                         # (g) two labels, one object
    assert 0 < row["small_sphere"][3] < row["table0"][3] and row["small_sphere"][1] == 6
    assert row["zero_dimensions"][1] == -1
    assert sum(1 for r in records if abs(r[8]) > 0.1) > 40                                   # (h) non-zero ry
    # the bit words say what the counts say
    for l in range(len(records)):
        pos = chk.positions_of(bits[l])
        assert len(pos) == result[l, 3] and (result[l, 1] >= 0 or len(pos) == 0)
    assert len({int(r[1]) for r in result}) >= 9


def test_identity_scene_boundaries_are_inclusive():
    points, ids, k, records, names = chk.identity_scene()
    result, bits = chk.restated_match(points, ids, k, chk.IDENTITY, records, 1)
    s, b = chk.memberships(points[ids == 0], chk.IDENTITY, records[0])
    assert s.tolist() == [True, True, True, False, False] and b.tolist() == [True, True, False, False, True]
    # k counts (0, 0, 5) of object 1, ON the sphere, and its (2, 2, 0.5); the row (3, 4, 0), ON the sphere and on two faces, is selected
    assert result[0].tolist()[:4] == [5.0, 0.0, 2.0, 3.0] and int(bits[0, 0]) == 0b00111
    assert np.array_equal(result[0, 4:7], [chk.object_sum(np.array([3.0, 1.0, points[2, 0]])) / 3.0, chk.object_sum(np.array([4.0, 1.0, 0.5])) / 3.0, 0.0])
    s, b = chk.memberships(points[ids == 0], chk.IDENTITY, records[1])
    assert s[4] and b[4]                                                                     # on three faces at once
    assert result[1, 1] == 0 and result[1, 2] == 3


def test_restatement_equals_the_recorded_reference(gold, scene):
    g = gold[0]
    points, ids, k, records, names, words, result, bits = scene
    got = result[:chk.N_TABLE]
    assert got[:, 0].astype(np.int64).tolist() == g["k"].tolist()
    assert got[:, 1].astype(np.int64).tolist() == g["object_id"].tolist()
    assert got[:, 3].astype(np.int64).tolist() == g["count"].tolist()
    found = g["object_id"] >= 0
    assert found.sum() == 10 and np.isnan(got[~found][:, 4:7]).all() and np.isnan(g["center"][~found]).all()
    err = np.abs(got[found][:, 4:7] - g["center"][found])
    print("worst centre error against the recorded reference", err.max())
    assert err.max() < TOL
    # the selected rows are the reference's, as a set (the reference lists them by distance)
    for l in np.flatnonzero(found):
        rows = np.flatnonzero(ids == int(got[l, 1]))[chk.positions_of(bits[l])]
        d = np.linalg.norm(points[rows] - records[l][:3], axis=1)
        assert len(rows) == g["count"][l] and d.max() < records[l][3]


def test_read_label_and_transforms_agree_with_the_recorded_reference(pcp, gold):
    g, calib = gold[0], gold[1]
    df = pcp.read_label(os.path.join(GOLDEN, "label_match_label.txt"), calib)
    assert list(df.columns) == chk.LABEL_COLUMNS + ["vx", "vy", "vz", "radius"]
    assert df.index.values.tolist() == g["label_index"].tolist() and 8 not in df.index      # the row without dimensions is dropped
    assert df["type"].tolist() == g["label_type"].tolist()
    assert np.array_equal(df[chk.LABEL_COLUMNS[1:]].values.astype(np.float64), g["label_numbers"])
    assert np.abs(df[["vx", "vy", "vz"]].values - g["label_velo"]).max() < TOL
    assert np.array_equal(df["radius"].values, g["label_radius"])
    # the records match_labels builds from the frame are the restatement's
    rec = pcp.label_records(df)
    assert rec.shape == (chk.N_TABLE, 16) and np.array_equal(rec, chk.table_records(calib))
    assert np.array_equal(pcp.transform_from_cam_to_velo(g["probe_cam"], calib), chk.restated_cam_to_velo(g["probe_cam"], calib))
    assert np.abs(pcp.transform_from_cam_to_velo(g["probe_cam"], calib) - g["probe_velo"]).max() < TOL
    first = df.iloc[0]
    obj = pcp.transform_from_velo_to_obj(g["probe"], calib, [first["cx"], first["cy"], first["cz"]], first["ry"])
    assert np.abs(obj - g["probe_obj"]).max() < TOL
    # the kernel's xo, yo, zo are this function's columns (yo with the height bias)
    X = chk.restated_cam(g["probe"], calib)
    e = X - np.array([first["cx"], first["cy"], first["cz"]])
    cs, sn = np.cos(first["ry"]), np.sin(first["ry"])
    assert np.array_equal(obj, np.stack([cs * e[:, 0] - sn * e[:, 2], e[:, 1], sn * e[:, 0] + cs * e[:, 2]], axis=1))


def test_filter_by_bouding_box(pcp):
    X = np.array([[0.5, 0.0, 0.0], [-0.5, 0.25, 0.0], [0.0, 0.0, 0.0], [0.6, 0.0, 0.0], [0.0, 0.0, 0.0], [0.1, 0.1, 0.1]])
    dims = np.array([1.0, 0.5, 1.0])
    assert pcp.filter_by_bouding_box(X, np.array([4, 4, 2, 2, 2, 9]), dims) == 2          # rows 0 and 1 are ON faces: 4 and 2 tie, the lowest wins
    assert pcp.filter_by_bouding_box(X, np.array([4, 4, 7, 2, 2, 9]), dims) == 4
    assert pcp.filter_by_bouding_box(X[3:4], np.array([1]), dims) is None


def test_get_object_category_on_every_type(pcp, gold):
    g = gold[0]
    types = g["types"].tolist()
    assert {"Car", "Van", "Truck", "Pedestrian", "Person_sitting", "Cyclist", "Tram", "Misc", "DontCare"} <= set(types)
    assert [pcp.get_object_category(t) for t in types] == g["categories"].tolist()
    assert pcp.get_object_category(None) == str(g["category_of_none"]) == "misc"
    assert [pcp.get_object_category(t) for t in ("Car", "Van", "Truck", "Tram", "Pedestrian", "Person_sitting", "Cyclist", "Misc", "DontCare")] == \
        ["vehicle"] * 4 + ["pedestrian"] * 2 + ["cyclist", "misc", "misc"]


def test_label_containers(pcp):
    import pandas as pd

    d = {c: pcp.init_label() for c in ("vehicle", "misc")}
    assert list(d["misc"]) == ["type", "truncated", "occluded", "vx", "vy", "vz", "num_measurements", "height", "width", "length", "ry"]
    label = pd.Series({"type": "Van", "truncated": 0.1, "occluded": 2, "height": 2.0, "width": 1.9, "length": 5.0, "ry": -0.05})
    pcp.add_label(d, "vehicle", label, 65, np.array([1.0, 2.0, 3.0]))
    pcp.add_label(d, "misc", None, 7, np.array([4.0, 5.0, 6.0]))
    assert d["vehicle"] == {"type": ["Van"], "truncated": [0.1], "occluded": [2], "vx": [1.0], "vy": [2.0], "vz": [3.0], "num_measurements": [65],
                            "height": [2.0], "width": [1.9], "length": [5.0], "ry": [-0.05]}
    assert d["misc"] == {"type": ["Unknown"], "truncated": [-1], "occluded": [-1], "vx": [4.0], "vy": [5.0], "vz": [6.0], "num_measurements": [7],
                         "height": [-1], "width": [-1], "length": [-1], "ry": [-10]}

    class Pcd:
        points = np.arange(12.0).reshape(4, 3)
        normals = -np.arange(12.0).reshape(4, 3)

    frame = pcp.get_object_pcd_df(Pcd, np.array([2, 0]), 2)
    assert list(frame.columns) == ["vx", "vy", "vz", "nx", "ny", "nz"] and frame.values.tolist() == [[6, 7, 8, -6, -7, -8], [0, 1, 2, 0, -1, -2]]
