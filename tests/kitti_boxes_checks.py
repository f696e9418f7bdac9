"""NumPy restatement of the KITTI-box stage (include/pcr.h, "KITTI boxes") in the written operation order, the calibration and the
planted scene of its tests, and the synthetic street of the end-to-end test.  Nothing here imports the product or the reference."""
import numpy as np

BOX_DOUBLES = 16
FIELDS = ("left", "top", "right", "bottom", "height", "width", "length", "cx", "cy", "cz", "ry")   # the 11 numbers of a label row


# ------------------------------------------------------------------ a calibration of KITTI's shape
def _tr_velo_to_cam():
    perm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])   # x_cam = -y, y_cam = -z, z_cam = x
    c, s = np.cos(0.01), np.sin(0.01)
    rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(np.hstack([perm @ rz, np.array([[-0.004], [-0.076], [-0.272]])]))


CALIB = {
    "P2": np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]),
    "R0_rect": np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]]),
    "Tr_velo_to_cam": _tr_velo_to_cam(),
}


# ------------------------------------------------------------------ the written order
def restated_cam(points, calib):
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    T, R0 = np.asarray(calib["Tr_velo_to_cam"], dtype=np.float64), np.asarray(calib["R0_rect"], dtype=np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    u = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
    return np.stack([(R0[i, 0] * u[0] + R0[i, 1] * u[1]) + R0[i, 2] * u[2] for i in range(3)], axis=1)


def restated_pixel(X, calib):
    K = np.asarray(calib["P2"], dtype=np.float64)
    q = [((K[i, 0] * X[:, 0] + K[i, 1] * X[:, 1]) + K[i, 2] * X[:, 2]) + K[i, 3] for i in range(3)]
    return np.stack([q[0] / q[2], q[1] / q[2]], axis=1)


def object_sum(v):
    """p_l (l = 0 .. 63) = +0.0 + rows l, l + 64, ... ascending; then p_l += p_{l+s} for l < s, s = 32 .. 1; the sum is p_0."""
    v = np.asarray(v, dtype=np.float64)
    pad = np.zeros(-len(v) % 64)                   # (p + 0.0 == p for every p that began as +0.0)
    p = np.zeros(64)
    for chunk in np.concatenate([v, pad]).reshape(-1, 64):
        p = p + chunk
    s = 32
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def restated_direction(a, b, c):
    a, b, c = np.float64(a), np.float64(b), np.float64(c)
    h = (a - c) * np.float64(0.5)
    if b == 0.0:
        return (np.float64(1.0), np.float64(-0.0)) if h > 0.0 else (np.float64(0.0), np.float64(-1.0))
    r = np.sqrt(h * h + b * b)
    e0, e1 = (h + r, b) if h >= 0.0 else (-b, r - h)
    length = np.sqrt(e0 * e0 + e1 * e1)
    return e0 / length, e1 / length


def direction_branch(a, b, c):
    h = (np.float64(a) - np.float64(c)) * 0.5
    if b == 0.0:
        return "b0_hpos" if h > 0.0 else "b0_hnonpos"
    return "hnonneg" if h >= 0.0 else "hneg"


def restated_boxes(points, object_ids, n_objects, calib, keep=None):
    """-> (n_objects, 16) in the layout of include/pcr.h."""
    points = np.asarray(points, dtype=np.float64)
    ids = np.asarray(object_ids)
    out = np.full((n_objects, BOX_DOUBLES), np.nan)
    for o in range(n_objects):
        P = points[ids == o]                      # ascending caller row
        n = np.float64(len(P))
        out[o, 15] = n
        if len(P) == 0 or (keep is not None and not keep[o]):
            continue
        X = restated_cam(P, calib)
        px = restated_pixel(X, calib)
        ctr = np.array([object_sum(X[:, i]) / n for i in range(3)])
        d = X - ctr
        a, b, c = object_sum(d[:, 0] * d[:, 0]) / n, object_sum(d[:, 0] * d[:, 2]) / n, object_sum(d[:, 2] * d[:, 2]) / n
        cs, sn = restated_direction(a, b, c)
        ms = -sn
        obj = [cs * d[:, 0] - ms * d[:, 2], d[:, 1], ms * d[:, 0] + cs * d[:, 2]]
        ext = [-np.min(-v) - np.min(v) for v in obj]
        out[o, :15] = [np.min(px[:, 0]), np.min(px[:, 1]), -np.min(-px[:, 0]), -np.min(-px[:, 1]), ext[1], ext[0], ext[2], ctr[0], ctr[1], ctr[2],
                       cs, sn, a, b, c]
    return out


def fields_of(boxes):
    """(k, 16) boxes -> (k, 11) numbers of the label rows, FIELDS order; ry = atan2(sn, cs) on the host."""
    boxes = np.asarray(boxes)
    return np.column_stack([boxes[:, 0:10], np.arctan2(boxes[:, 11], boxes[:, 10])])


def conditioning(boxes):
    """hypot(a - c, 2b) / (a + c) per object: the relative gap of the two eigenvalues; NaN where the covariance is zero or absent."""
    a, b, c = boxes[:, 12], boxes[:, 13], boxes[:, 14]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.hypot(a - c, 2.0 * b) / (a + c)


# ------------------------------------------------------------------ the planted scene
def object_sizes(lds_rows):
    return [1, 2, 5, 63, 64, 65, 127, 128, 129, lds_rows - 1, lds_rows, lds_rows + 1, 2 * lds_rows + 7]


COINCIDENT_ID = 13   # five copies of one point
UNUSED_ID = 14       # no rows
ALIGNED_ID = 15      # a box along the sensor's x axis: its x-z spread in the camera frame is axis-aligned up to the calibration's tilt
ALIGNED_SIZE = 40
N_NOISE = 700


def _box_points(rng, n, centre, heading, size):
    local = rng.uniform(-0.5, 0.5, size=(n, 3)) * size
    c, s = np.cos(heading), np.sin(heading)
    return centre + np.column_stack([c * local[:, 0] - s * local[:, 1], s * local[:, 0] + c * local[:, 1], local[:, 2]])


def planted_scene(lds_rows, seed=31):
    """-> (points (n,3) float64 holding float32-rounded coordinates, object_ids (n,) int64, n_objects).  Oriented boxes of random
    heading in (-pi, pi), 1.6-4.5 m long and 0.4-0.9 m wide, centres inside x in [8, 66], y in [-21, 21] (every point inside the
    detector's field of view x in [5, 70], y in [-25, 25]); rows shuffled, so objects interleave."""
    rng = np.random.default_rng(seed)
    pts, ids = [], []
    for o, n in enumerate(object_sizes(lds_rows)):
        centre = np.array([rng.uniform(8.0, 66.0), rng.uniform(-21.0, 21.0), rng.uniform(-1.2, 0.3)])
        size = np.array([rng.uniform(1.6, 4.5), rng.uniform(0.4, 0.9), rng.uniform(0.5, 1.8)])
        pts.append(_box_points(rng, n, centre, rng.uniform(-np.pi, np.pi), size))
        ids += [o] * n
    pts.append(np.repeat(np.array([[41.0, 12.5, -0.75]]), 5, axis=0))
    ids += [COINCIDENT_ID] * 5
    pts.append(_box_points(rng, ALIGNED_SIZE, np.array([20.0, -6.0, -0.5]), 0.0, np.array([4.0, 0.5, 1.5])))
    ids += [ALIGNED_ID] * ALIGNED_SIZE
    pts.append(np.column_stack([rng.uniform(5.0, 70.0, N_NOISE), rng.uniform(-25.0, 25.0, N_NOISE), rng.uniform(-2.0, 1.0, N_NOISE)]))
    ids += [-1] * N_NOISE
    points = np.concatenate(pts).astype(np.float32).astype(np.float64)
    ids = np.array(ids, dtype=np.int64)
    order = rng.permutation(len(ids))
    return np.ascontiguousarray(points[order]), ids[order], ALIGNED_ID + 1


# ------------------------------------------------------------------ the synthetic street of the end-to-end test
STREET_NORMAL = np.array([0.02, -0.015, 1.0]) / np.linalg.norm([0.02, -0.015, 1.0])
STREET_OFFSET = 1.7           # the plane is STREET_NORMAL . p + STREET_OFFSET = 0: the road 1.7 m below the sensor
STREET_BOX_SIZES = [40, 90, 150, 220, 300, 400]
STREET_GROUND = 4800


def synthetic_street(seed=8):
    """-> (points (n,3) float64 of float32-rounded coordinates, planted (n,) int64: -1 ground, b for box b).  A tilted plane with
    0.05 m noise over x in [4, 60], y in [-20, 20], and six boxes of 40-400 points between 0.45 m and 1.9 m above it, more than 8 m
    apart and dense enough (over 30 points per cubic metre) for DBSCAN(0.60, 3) to hold each together.  Rows shuffled.
    The fitted plane is the best sampled triple's, without a refit, so it carries the noise of three ground points: its 0.30 m band
    can reach some 0.1 m higher than the planted plane's.  The boxes start 0.45 m up, so that a box loses rows to the band only if
    the plane is off by more than that, and its centre can be compared with the mean of ALL its planted points."""
    rng = np.random.default_rng(seed)
    n, d = STREET_NORMAL, STREET_OFFSET
    gx, gy = rng.uniform(4.0, 60.0, STREET_GROUND), rng.uniform(-20.0, 20.0, STREET_GROUND)
    gz = -(d + n[0] * gx + n[1] * gy) / n[2] + rng.normal(scale=0.05, size=STREET_GROUND)
    pts, planted = [np.column_stack([gx, gy, gz])], [-1] * STREET_GROUND
    centres = [(10.0, -8.0), (18.0, 6.0), (27.0, -3.0), (36.0, 12.0), (45.0, -12.0), (54.0, 2.0)]
    for b, (m, (cx, cy)) in enumerate(zip(STREET_BOX_SIZES, centres)):
        heading = rng.uniform(-np.pi, np.pi)
        size = np.array([1.2 + 2.3 * m / 400.0, rng.uniform(0.7, 1.0), 0.0])
        z0 = -(d + n[0] * cx + n[1] * cy) / n[2]
        local = _box_points(rng, m, np.array([cx, cy, 0.0]), heading, size)
        local[:, 2] = z0 + rng.uniform(0.45, 1.2 + 0.7 * m / 400.0, size=m)
        pts.append(local)
        planted += [b] * m
    points = np.concatenate(pts).astype(np.float32).astype(np.float64)
    planted = np.array(planted, dtype=np.int64)
    order = rng.permutation(len(planted))
    return np.ascontiguousarray(points[order]), planted[order]
