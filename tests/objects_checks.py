"""NumPy restatements of the object-batch stage (include/pcr.h, "object batches") in the written operation order, the SciPy / NumPy
formulation of Final_Project/scripts/detect.py:269-354 restated as `reference_preprocess`, and the planted scene of the GPU tests.
Nothing here imports the product or the reference."""
import numpy as np
import scipy.spatial.distance


# ------------------------------------------------------------------ the written order
def serial_mean(P):
    """(((p_0 + p_1) + p_2) + ...) / n per axis, rows ascending; 0/0 = NaN for no rows."""
    s = np.zeros(3)
    for row in np.asarray(P, dtype=np.float64).reshape(-1, 3):
        s = s + row
    with np.errstate(invalid="ignore"):
        return s / np.float64(len(P))


def serial_weights(P):
    """w_i = (((d_i0 + d_i1) + ...) + d_i,n-1) / n, d_ij = sqrt(((dx*dx) + dy*dy) + dz*dz) with dx = x_i - x_j; j ascending, all i at once."""
    P = np.asarray(P, dtype=np.float64)
    acc = np.zeros(len(P))
    for j in range(len(P)):
        dx, dy, dz = P[:, 0] - P[j, 0], P[:, 1] - P[j, 1], P[:, 2] - P[j, 2]
        acc = acc + np.sqrt((dx * dx + dy * dy) + dz * dz)
    return acc / np.float64(len(P))


def scipy_weights(P):
    """detect.py:299-301."""
    return scipy.spatial.distance.squareform(scipy.spatial.distance.pdist(np.asarray(P, dtype=np.float64), "euclidean")).mean(axis=0)


def restated_groups(object_ids, n_objects):
    """-> (offsets (n_objects + 1,), rows (m,)): object by object, ascending row within each; ids < 0 belong to no object."""
    ids = np.asarray(object_ids)
    per = [np.flatnonzero(ids == o) for o in range(n_objects)]
    offsets = np.zeros(n_objects + 1, dtype=np.int64)
    if n_objects:
        np.cumsum([len(r) for r in per], out=offsets[1:])
    rows = np.concatenate(per).astype(np.int32) if n_objects else np.zeros(0, dtype=np.int32)
    return offsets, rows


def restated_stats(points, object_ids, n_objects):
    points = np.asarray(points, dtype=np.float64)
    ids = np.asarray(object_ids)
    count = np.zeros(n_objects, dtype=np.int64)
    mean, lo, hi = np.zeros((n_objects, 3)), np.full((n_objects, 3), np.inf), np.full((n_objects, 3), -np.inf)
    for o in range(n_objects):
        P = points[ids == o]
        count[o] = len(P)
        mean[o] = serial_mean(P)
        if len(P):
            lo[o], hi[o] = P.min(axis=0), P.max(axis=0)
    return {"count": count, "mean": mean, "min_bound": lo, "max_bound": hi}


def restated_select(count, mean, max_radius, min_count=4):
    """detect.py:286-292: skipped on count <= 4 or sqrt((c*c).sum()) > radius; a NaN centre is dropped (include/pcr.h)."""
    keep = np.zeros(len(count), dtype=bool)
    for o in range(len(count)):
        c = np.asarray(mean[o], dtype=np.float64)[:2]
        with np.errstate(invalid="ignore"):
            keep[o] = bool(count[o] > min_count and np.sqrt((c * c).sum()) <= max_radius)
    return keep


# ------------------------------------------------------------------ detect.py:269-354
def reference_preprocess(points, normals, object_ids, config):
    points = np.asarray(points)
    normals = np.asarray(normals)
    num_objects = max(object_ids) + 1
    X = []
    y = []
    for object_id in range(num_objects):
        if (object_ids == object_id).sum() <= 4:
            continue
        object_center = np.mean(points[object_ids == object_id], axis=0)[:2]
        if np.sqrt((object_center * object_center).sum()) > config["max_radius_distance"]:
            continue
        points_ = np.copy(points[object_ids == object_id])
        normals_ = np.copy(normals[object_ids == object_id])
        N, _ = points_.shape
        weights = scipy.spatial.distance.squareform(scipy.spatial.distance.pdist(points_, "euclidean")).mean(axis=0)
        weights /= weights.sum()
        idx = np.random.choice(np.arange(N), size=(config["num_sample_points"],), replace=True if config["num_sample_points"] > N else False, p=weights)
        points_processed, normals_processed = points_[idx], normals_[idx]
        points_processed -= points_.mean(axis=0)
        X.append(np.hstack((points_processed, normals_processed)))
        y.append(object_id)
    N = len(y)
    if N % config["batch_size"] != 0:
        num_repeat = config["batch_size"] - N % config["batch_size"]
        for _ in range(num_repeat):
            X.append(X[0])
            y.append(y[0])
    return [(X[i], y[i]) for i in range(len(y))], N


# ------------------------------------------------------------------ the planted scene
def object_sizes(tile):
    return [3, 4, 5, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 7]


COINCIDENT_ID = 13   # five copies of one point
UNUSED_ID = 14       # no rows
FAR_ID = 15          # a last, ordinary object: the unused id lies inside the id range
FAR_SIZE = 40
N_SCENE = 6000


def planted_scene(tile, seed=20):
    """-> (points (6000,3) float64 holding float32-rounded lidar-scale coordinates, normals (6000,3) float64 unit vectors,
    object_ids (6000,) int64, n_objects).  Rows are shuffled, so objects interleave.  Ids 0..12: blobs of `object_sizes(tile)` rows;
    COINCIDENT_ID and object 5 (65 rows) lie more than 70 m out, every other centre within 60 m; UNUSED_ID has no rows; the rest
    of the rows are noise (-1) spread over the scene."""
    rng = np.random.default_rng(seed)
    sizes = object_sizes(tile)
    pts, ids = [], []
    for o, n in enumerate(sizes):
        ang = rng.uniform(-0.5, 0.5)
        r = rng.uniform(4.0, 55.0)
        centre = np.array([max(2.5, r * np.cos(ang)), np.clip(r * np.sin(ang), -28.0, 28.0), rng.uniform(-1.5, 0.5)])
        if o == 5:
            centre = np.array([72.0, 24.0, -0.5])
        pts.append(centre + rng.normal(scale=[0.6, 0.5, 0.4], size=(n, 3)))
        ids += [o] * n
    pts.append(np.repeat(np.array([[78.0, 25.0, -1.0]]), 5, axis=0))
    ids += [COINCIDENT_ID] * 5
    pts.append(np.array([30.0, -20.0, 0.0]) + rng.normal(scale=0.5, size=(FAR_SIZE, 3)))
    ids += [FAR_ID] * FAR_SIZE
    n_noise = N_SCENE - len(ids)
    pts.append(np.column_stack([rng.uniform(2.0, 80.0, n_noise), rng.uniform(-30.0, 30.0, n_noise), rng.uniform(-2.0, 1.0, n_noise)]))
    ids += [-1] * n_noise
    points = np.concatenate(pts).astype(np.float32).astype(np.float64)
    ids = np.array(ids, dtype=np.int64)
    order = rng.permutation(N_SCENE)
    points, ids = np.ascontiguousarray(points[order]), ids[order]
    nrm = rng.normal(size=(N_SCENE, 3))
    normals = np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    return points, normals, ids, FAR_ID + 1
