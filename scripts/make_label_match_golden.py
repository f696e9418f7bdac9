"""Records tests/golden/label_match.npz and tests/golden/label_match_label.txt: what the reference's own functions give for the planted
scene and the label table of tests/label_match_checks.py.

The reference's Final_Project/scripts/extract.py is imported by path from --reference, with empty stub modules in sys.modules for what
it imports and this machine lacks (open3d, progressbar; matplotlib if absent): none of them is touched by the functions called here,
which are its read_label (on the label file this script renders from the table), transform_from_cam_to_velo,
transform_from_velo_to_obj, filter_by_bouding_box and get_object_category.  Around them the loop of extract.py:514-566 is restated
with a brute-force ``<=`` radius query in place of Open3D's, neighbours in ascending distance, over the LABELLED rows (a row DBSCAN
calls noise belongs to no object of the library; the reference's np.unique would let the id -1 win).  Per label: k, the object id
(-1: none), N, and the centre ``.mean(axis=0)`` in that order.  Data only.

Every recorded label is asserted to keep all rows at least 1e-6 m away from its sphere and from its box faces, so that no BLAS rounding
decides a membership; the exact-boundary labels of the tests are checked against the restatement only.

    python scripts/make_label_match_golden.py --reference <reference checkout>
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import label_match_checks as chk  # noqa: E402

MARGIN = 1e-6
TYPES = ["Car", "Van", "Truck", "Pedestrian", "Person_sitting", "Cyclist", "Tram", "Misc", "DontCare", "Unknown", ""]


def load_reference(checkout):
    for name in ("open3d", "progressbar", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    spec = importlib.util.spec_from_file_location("reference_extract", os.path.join(checkout, "Final_Project", "scripts", "extract.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "label_match.npz"))
    ap.add_argument("--label-file", default=os.path.join(ROOT, "tests", "golden", "label_match_label.txt"))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    with open(a.label_file, "w") as f:
        f.write(chk.label_text())
    param = {key: np.asarray(chk.CALIB[key], dtype=np.float64) for key in ("P2", "R0_rect", "Tr_velo_to_cam")}
    df_label = ref.read_label(a.label_file, param)

    points, ids, n_objects, _, _ = chk.planted_scene()
    labelled = np.flatnonzero(ids >= 0)
    P, object_ids = points[labelled], ids[labelled]
    k_all, winner, n_sel, centre, margin = [], [], [], [], []
    for _, label in df_label.iterrows():
        center_velo = np.asarray([label["vx"], label["vy"], label["vz"]])
        center_cam = np.asarray([label["cx"], label["cy"], label["cz"]])
        dims = np.asarray([label["length"], label["height"], label["width"]])
        dist = np.sqrt(((P - center_velo) ** 2).sum(axis=1))
        margin.append(np.abs(dist - label["radius"]).min())
        idx = np.flatnonzero(dist <= label["radius"])
        idx = idx[np.argsort(dist[idx], kind="stable")]
        k_all.append(len(idx))
        object_id_ = None
        if len(idx) > 0:
            point_cloud_obj = ref.transform_from_velo_to_obj(P[idx], param, center_cam, label["ry"])
            point_cloud_obj[:, 1] += label["height"] / 2
            margin.append(min(np.abs(point_cloud_obj - dims / 2).min(), np.abs(point_cloud_obj + dims / 2).min()))
            object_id_ = ref.filter_by_bouding_box(point_cloud_obj, object_ids[idx], dims)
        if object_id_ is None:
            winner.append(-1)
            n_sel.append(0)
            centre.append([np.nan] * 3)
            continue
        idx_object = idx[object_ids[idx] == object_id_]
        winner.append(int(object_id_))
        n_sel.append(len(idx_object))
        centre.append(P[idx_object].mean(axis=0))
    assert min(margin) > MARGIN, f"a row lies within {min(margin):.3e} m of a sphere or a box face: move it"
    assert winner == chk.TABLE_WINNER, (winner, chk.TABLE_WINNER)

    rng = np.random.default_rng(5)
    probe = P[rng.choice(len(P), size=64, replace=False)]
    first = df_label.iloc[0]
    np.savez_compressed(
        a.out, points=points.astype(np.float32), ids=ids.astype(np.int32), n_objects=np.int32(n_objects),
        P2=param["P2"], R0_rect=param["R0_rect"], Tr_velo_to_cam=param["Tr_velo_to_cam"],
        label_index=df_label.index.values.astype(np.int32), label_type=np.array(df_label["type"].tolist()),
        label_numbers=df_label[chk.LABEL_COLUMNS[1:]].values.astype(np.float64), label_velo=df_label[["vx", "vy", "vz"]].values.astype(np.float64),
        label_radius=df_label["radius"].values.astype(np.float64),
        k=np.array(k_all, dtype=np.int64), object_id=np.array(winner, dtype=np.int64), count=np.array(n_sel, dtype=np.int64),
        center=np.array(centre, dtype=np.float64), min_margin=np.float64(min(margin)),
        probe=probe, probe_cam=df_label[["cx", "cy", "cz"]].values.astype(np.float64),
        probe_velo=ref.transform_from_cam_to_velo(df_label[["cx", "cy", "cz"]].values.astype(np.float64), param),
        probe_obj=ref.transform_from_velo_to_obj(probe, param, np.asarray([first["cx"], first["cy"], first["cz"]]), first["ry"]),
        types=np.array(TYPES), categories=np.array([ref.get_object_category(t) for t in TYPES]), category_of_none=np.array(ref.get_object_category(None)))
    print(f"{a.out}: {len(points)} points, {len(df_label)} labels, winners {winner}, counts {n_sel}, k {k_all}, smallest margin {min(margin):.3e} m, "
          f"{os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
