"""NumPy restatement of the label match (include/pcr.h, "label match") in the written operation order -- memberships, votes, winner,
the object sum over the selected rows, the ballot words --, the label table behind tests/golden/label_match_label.txt, and the planted
scenes of its tests.  Nothing here imports the product or the reference."""
import numpy as np

from tests.kitti_boxes_checks import CALIB, object_sum, restated_cam

LABEL_DOUBLES = 16
RESULT_DOUBLES = 8
IDENTITY = {"P2": np.hstack([np.eye(3), np.zeros((3, 1))]), "R0_rect": np.eye(3), "Tr_velo_to_cam": np.hstack([np.eye(3), np.zeros((3, 1))])}
LABEL_COLUMNS = ["type", "truncated", "occluded", "alpha", "left", "top", "right", "bottom", "height", "width", "length", "cx", "cy", "cz", "ry"]

# ------------------------------------------------------------------ the label file (KITTI label_2 format, two decimals)
# type, truncated, occluded, alpha, left, top, right, bottom, height, width, length, cx, cy, cz, ry;  the planted object it is drawn round
LABEL_TABLE = [
    ("Car", 0.00, 0, -1.58, 587.01, 173.33, 614.12, 200.12, 1.50, 1.60, 3.90, 2.50, 1.65, 12.00, 0.30),           # 0: object 6, larger than the box
    ("Pedestrian", 0.00, 1, 0.21, 423.17, 173.67, 433.17, 224.03, 1.75, 0.60, 0.80, -4.00, 1.70, 9.50, -1.20),    # 1: object 2
    ("Cyclist", 0.00, 0, -2.46, 665.45, 160.00, 717.90, 217.99, 1.70, 0.60, 1.80, 6.00, 1.60, 20.00, 1.57),       # 2: object 3
    ("Van", 0.10, 2, 1.85, 387.63, 181.54, 423.81, 203.12, 2.00, 1.90, 5.00, -8.00, 1.75, 25.00, -0.05),          # 3: object 4
    ("Truck", 0.00, 0, -1.67, 657.39, 190.13, 700.07, 223.39, 3.00, 2.50, 8.00, 10.00, 1.80, 40.00, 2.80),        # 4: object 5
    ("Person_sitting", 0.00, 0, 0.02, 600.00, 170.00, 660.00, 260.00, 1.20, 0.60, 0.70, 1.00, 1.60, 7.00, 0.00),  # 5: object 1 (5 rows)
    ("Tram", 0.35, 3, 1.44, 300.00, 150.00, 420.00, 200.00, 3.20, 2.40, 12.00, -12.00, 1.70, 50.00, 0.10),        # 6: object 0 (1 row)
    ("Misc", 0.00, 0, -0.50, 900.00, 170.00, 940.00, 200.00, 1.00, 1.00, 1.00, 15.00, 1.60, 30.00, 0.50),         # 7: nothing there
    ("DontCare", -1, -1, -10, 503.89, 169.71, 590.61, 190.13, -1, -1, -1, -1000, -1000, -1000, -10),              # dropped by read_label
    ("Car", 0.00, 0, -1.60, 650.00, 188.00, 705.00, 225.00, 2.80, 2.40, 7.50, 10.20, 1.80, 40.10, 2.75),          # 8: object 5 again
    ("Car", 0.00, 0, 0.10, 500.00, 170.00, 560.00, 210.00, 1.60, 1.80, 4.00, -2.00, 1.65, 16.00, 0.00),           # 9: objects 8 and 9 tie
    ("Car", 0.00, 0, 0.80, 680.00, 172.00, 720.00, 200.00, 1.50, 1.60, 3.50, 4.00, 1.65, 33.00, 0.70),            # 10: objects 9 and 13 tie
    ("Car", 0.00, 0, 0.30, 300.00, 160.00, 340.00, 175.00, 0.20, 0.20, 4.00, -6.00, 1.00, 14.00, 0.40),           # 11: object 11 in the sphere only
]
N_TABLE = sum(1 for row in LABEL_TABLE if row[8] >= 0)
TABLE_WINNER = [6, 2, 3, 4, 5, 1, 0, -1, 5, 8, 9, -1]   # what the planting intends for the kept rows, in order


def label_text():
    return "".join(" ".join([row[0]] + [f"{v:.2f}" for v in row[1:]]) + "\n" for row in LABEL_TABLE)


def table_geometry():
    """The kept rows -> (n, 8): height, width, length, cx, cy, cz, ry, index in LABEL_TABLE."""
    return np.array([list(row[8:15]) + [i] for i, row in enumerate(LABEL_TABLE) if row[8] >= 0], dtype=np.float64)


# ------------------------------------------------------------------ the written order
def restated_cam_to_velo(X_cam, calib):
    """transform_from_cam_to_velo (extract.py:86-114), elementwise: w_i = (R0[0][i]*X_0 + R0[1][i]*X_1) + R0[2][i]*X_2, d = w - t,
    v_i = (R[0][i]*d_0 + R[1][i]*d_1) + R[2][i]*d_2."""
    X = np.asarray(X_cam, dtype=np.float64).reshape(-1, 3)
    R0, T = np.asarray(calib["R0_rect"], dtype=np.float64), np.asarray(calib["Tr_velo_to_cam"], dtype=np.float64)
    w = [(R0[0, i] * X[:, 0] + R0[1, i] * X[:, 1]) + R0[2, i] * X[:, 2] for i in range(3)]
    d = [w[i] - T[i, 3] for i in range(3)]
    return np.stack([(T[0, i] * d[0] + T[1, i] * d[1]) + T[2, i] * d[2] for i in range(3)], axis=1)


def record(v, radius, c, ry, length, height, width):
    """One label record of include/pcr.h."""
    return np.array([v[0], v[1], v[2], radius, c[0], c[1], c[2], np.cos(ry), np.sin(ry), length, height, width, 0.0, 0.0, 0.0, 0.0], dtype=np.float64)


def table_records(calib):
    """The records read_label + match_labels make of the label file: v = cam_to_velo(c) with + height/2, radius = ||0.5*(h, w, l)||."""
    out = []
    for h, w, l, cx, cy, cz, ry, _ in table_geometry():
        v = restated_cam_to_velo([[cx, cy, cz]], calib)[0]
        v[2] += h / 2
        out.append(record(v, np.linalg.norm(0.5 * np.asarray([h, w, l])), (cx, cy, cz), ry, l, h, w))
    return np.array(out)


def memberships(P, calib, rec):
    """-> (in_sphere, in_box) of the rows P for one record."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    dx, dy, dz = x - rec[0], y - rec[1], z - rec[2]
    in_sphere = (dx * dx + dy * dy) + dz * dz <= rec[3] * rec[3]
    X = restated_cam(P, calib)
    e0, e1, e2 = X[:, 0] - rec[4], X[:, 1] - rec[5], X[:, 2] - rec[6]
    cs, sn = rec[7], rec[8]
    hl, hh, hw = rec[9] / 2, rec[10] / 2, rec[11] / 2
    xo, yo, zo = cs * e0 - sn * e2, e1 + hh, sn * e0 + cs * e2
    in_box = (-hl <= xo) & (xo <= hl) & (-hh <= yo) & (yo <= hh) & (-hw <= zo) & (zo <= hw)
    return in_sphere, in_box


def words_needed(object_ids, n_objects):
    ids = np.asarray(object_ids)
    counts = np.bincount(ids[ids >= 0], minlength=n_objects) if n_objects else np.zeros(0, dtype=np.int64)
    return int(-(-counts.max() // 64)) if len(counts) else 0


def restated_match(points, object_ids, n_objects, calib, records, words):
    """-> (result (L, 8) float64, sel_bits (L, words) uint64) in the layout of include/pcr.h."""
    points = np.asarray(points, dtype=np.float64)
    ids = np.asarray(object_ids)
    records = np.asarray(records, dtype=np.float64).reshape(-1, LABEL_DOUBLES)
    rows_of = [np.flatnonzero(ids == o) for o in range(n_objects)]          # ascending caller row: the grouped order
    result = np.zeros((len(records), RESULT_DOUBLES))
    bits = np.zeros((len(records), words), dtype=np.uint64)
    for l, rec in enumerate(records):
        k, votes, spheres = 0, np.zeros(n_objects, dtype=np.int64), []
        for o in range(n_objects):
            s, b = memberships(points[rows_of[o]], calib, rec)
            k += int(s.sum())
            votes[o] = int((s & b).sum())
            spheres.append(s)
        winner = int(np.argmax(votes)) if n_objects and votes.max() > 0 else -1     # argmax: the first, so the lowest, maximum
        result[l, 0], result[l, 1] = k, winner
        if winner < 0:
            result[l, 4:7] = np.nan
            continue
        sel = spheres[winner]
        P = points[rows_of[winner]]
        n_sel = int(sel.sum())
        result[l, 2], result[l, 3] = votes[winner], n_sel
        # a skipped row adds nothing; adding +0.0 in its place gives the same bits (a partial that began as +0.0 is never -0.0)
        result[l, 4:7] = [object_sum(np.where(sel, P[:, a], 0.0)) / np.float64(n_sel) for a in range(3)]
        for p in np.flatnonzero(sel):
            bits[l, p // 64] |= np.uint64(1) << np.uint64(p % 64)
    return result, bits


def positions_of(bits_row):
    """The set bits of one label's words, ascending."""
    return np.array([64 * w + b for w, word in enumerate(bits_row) for b in range(64) if (int(word) >> b) & 1], dtype=np.int64)


# ------------------------------------------------------------------ the planted scene (CALIB)
SIZES = {0: 1, 1: 5, 2: 63, 3: 64, 4: 65, 5: 129, 6: 1003}
UNUSED_ID = 7
N_OBJECTS = 14
N_NOISE = 300
TABLE_OBJECT = {6: 0, 5: 1, 1: 2, 2: 3, 3: 4, 4: 5, 0: 6}   # index in LABEL_TABLE -> the object planted in it


def _velo_of_object_frame(local, geom, calib):
    """Rows given in a label's object frame (xo, yo, zo) -> the Velodyne frame, by the inverse of the written transform (planting
    only: the float32 rounding that follows is far coarser than this inverse's error)."""
    h, _, _, cx, cy, cz, ry = geom[:7]
    cs, sn = np.cos(ry), np.sin(ry)
    e = np.column_stack([cs * local[:, 0] + sn * local[:, 2], local[:, 1] - h / 2, -sn * local[:, 0] + cs * local[:, 2]])
    X = e + np.array([cx, cy, cz])
    R0, T = np.asarray(calib["R0_rect"]), np.asarray(calib["Tr_velo_to_cam"])
    return (np.linalg.inv(T[:, :3]) @ (np.linalg.inv(R0) @ X.T - T[:, 3:4])).T


def _in_box_rows(rng, n, geom, scale=(0.9, 0.9, 0.9)):
    h, w, l = geom[:3]
    return rng.uniform(-0.5, 0.5, size=(n, 3)) * np.array([l * scale[0], h * scale[1], w * scale[2]])


def planted_scene(seed=17):
    """-> (points (n,3) float64 of float32-rounded coordinates, object_ids (n,) int64, n_objects, records (L,16), names (L,)).
    Objects of 1, 5, 63, 64, 65, 129 and 1003 rows inside the labels of LABEL_TABLE (object 6 is a quarter longer than its box: rows in
    the sphere beyond the faces), id 7 without rows, objects 8 / 9 and 9 / 13 with equal votes under two labels, object 10 along a
    diagonal (its axis-aligned box has empty corners), object 11 beside a thin label, object 12 far from every label, noise rows;
    caller rows shuffled.  The records: the table's, then the edges named in `names`, then jittered copies up to 72 labels."""
    rng = np.random.default_rng(seed)
    geom = {int(g[7]): g for g in table_geometry()}
    pts, ids = [], []

    def add(o, rows):
        pts.append(rows)
        ids.extend([o] * len(rows))

    for t, o in TABLE_OBJECT.items():
        scale = (1.25, 0.9, 0.9) if o == 6 else (0.9, 0.9, 0.9)
        add(o, _velo_of_object_frame(_in_box_rows(rng, SIZES[o], geom[t], scale), geom[t], CALIB))
    # label 10 (table row 10 of LABEL_TABLE -> the tie of objects 8 and 9): six rows of each in the box, 10 and 3 above its top face
    g = geom[10]
    above = lambda n: np.column_stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-g[0] / 2 - 0.6, -g[0] / 2 - 0.3, n), rng.uniform(-0.4, 0.4, n)])  # noqa: E731
    add(8, _velo_of_object_frame(np.vstack([_in_box_rows(rng, 6, g), above(10)]), g, CALIB))
    add(9, _velo_of_object_frame(np.vstack([_in_box_rows(rng, 6, g), above(3)]), g, CALIB))
    # label 11: four rows of object 9 and four of object 13 in the box (both belong to wave 1 of the kernel), 13 has 20 more far off
    g = geom[11]
    add(9, _velo_of_object_frame(_in_box_rows(rng, 4, g), g, CALIB))
    add(13, _velo_of_object_frame(_in_box_rows(rng, 4, g), g, CALIB))
    add(13, np.column_stack([rng.uniform(60, 62, 20), rng.uniform(18, 19, 20), rng.uniform(-1, 0, 20)]))
    # label 12: object 11 beside the thin box, inside its sphere
    g = geom[12]
    add(11, _velo_of_object_frame(np.column_stack([rng.uniform(-1, 1, 12), np.zeros(12), rng.uniform(0.8, 1.2, 12)]), g, CALIB))
    # object 10: a diagonal from (30, -15, 0) to (33, -12, 0), both ends included
    t = np.linspace(0.0, 3.0, 40)
    add(10, np.column_stack([30.0 + t, -15.0 + t, np.zeros(40)]))
    add(12, np.column_stack([rng.uniform(70, 72, 30), rng.uniform(-25, -24, 30), rng.uniform(-1, 0, 30)]))
    add(-1, np.column_stack([rng.uniform(5, 70, N_NOISE), rng.uniform(-25, 25, N_NOISE), rng.uniform(-2, 1, N_NOISE)]))
    points = np.concatenate(pts).astype(np.float32).astype(np.float64)
    ids = np.array(ids, dtype=np.int64)
    order = rng.permutation(len(ids))
    points, ids = np.ascontiguousarray(points[order]), ids[order]

    table = table_records(CALIB)
    names = [f"table{int(g[7])}" for g in table_geometry()]
    records = list(table)
    far = (500.0, 500.0, 500.0)     # a camera-frame centre no row is near: the box is empty whatever the sphere holds

    def edge(name, v, radius):
        names.append(name)
        records.append(record(v, radius, far, 0.0, 1.0, 1.0, 1.0))

    edge("corner_of_box_no_rows", (33.0, -15.0, 0.0), 0.5)              # meets object 10's box at an empty corner
    edge("just_short_of_box", (np.nextafter(34.0, np.inf), -12.0, 0.0), 1.0)   # ends one ulp short of the box: pruned
    edge("touching_box", (34.0, -12.0, 0.0), 1.0)                       # d2 == r*r for the row (33, -12, 0): k = 1
    edge("zero_radius_on_a_row", (33.0, -12.0, 0.0), 0.0)               # radius 0 holds the row it sits on
    edge("everything", (35.0, 0.0, 0.0), 100.0)                         # every labelled row: nothing pruned
    # the same box as table row 0 with a sphere that misses object 6's far end, and with zero dimensions
    r0 = table[0].copy()
    r0[3] = 1.0
    names.append("small_sphere")
    records.append(r0)
    r0 = table[0].copy()
    r0[9:12] = 0.0
    names.append("zero_dimensions")
    records.append(r0)
    j = 0
    while len(records) < 72:
        base = table[j % len(table)].copy()
        shift = rng.normal(scale=0.5, size=3)
        ry = rng.uniform(-np.pi, np.pi)
        dims = base[9:12] * rng.uniform(0.7, 1.5, size=3)
        c = base[4:7] + shift
        v = restated_cam_to_velo([c], CALIB)[0]
        v[2] += dims[1] / 2
        records.append(record(v, np.linalg.norm(0.5 * dims), c, ry, *dims))
        names.append(f"jitter{j}")
        j += 1
    return points, ids, N_OBJECTS, np.array(records), names


# ------------------------------------------------------------------ the exact-boundary scene (identity calibration, ry = 0)
def identity_scene():
    """-> (points, object_ids, n_objects, records, names).  With the identity calibration X = (x, y, z) exactly, and with ry = 0
    xo = x - cx, yo = (y - cy) + height/2, zo = z - cz exactly for these small binary fractions."""
    up = float(np.nextafter(np.float32(3.0), np.float32(4.0)))   # the float32 after 3
    rows = [
        ((3.0, 4.0, 0.0), 0),      # position 0: ON the sphere (25 == 25) and ON the faces xo = +length/2 and yo = +height/2
        ((1.0, 1.0, 0.0), 0),      # inside both
        ((-up, 0.5, 0.0), 0),      # in the sphere, beyond the face xo = -length/2
        ((up, 4.0, 0.0), 0),       # beyond the sphere
        ((-3.0, -4.0, 1.0), 0),    # beyond the first sphere (26 > 25), inside the second; ON the faces xo = -length/2, yo = -height/2, zo = +width/2
        ((0.0, 0.0, 5.0), 1),      # on the sphere, outside the box
        ((0.0, 0.0, -float(np.nextafter(np.float32(5.0), np.float32(6.0)))), 1),   # the float32 beyond the sphere
        ((2.0, 2.0, 0.5), 1),      # inside both: object 1 has one vote
    ]
    points = np.array([r[0] for r in rows], dtype=np.float64)
    assert np.array_equal(points, points.astype(np.float32).astype(np.float64))
    ids = np.array([r[1] for r in rows], dtype=np.int64)
    records = np.array([
        record((0.0, 0.0, 0.0), 5.0, (0.0, 4.0, 0.0), 0.0, 6.0, 8.0, 2.0),
        record((0.0, 0.0, 0.0), 5.125, (0.0, 4.0, 0.0), 0.0, 6.0, 8.0, 2.0),
    ])
    return points, ids, 2, records, ["on_sphere_and_faces", "three_faces"]
