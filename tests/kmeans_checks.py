"""NumPy float64 restatement of the K-Means rules of include/pcr.h (Lloyd's iteration), shared by the K-Means tests,
scripts/gen_kmeans_golden.py and scripts/kmeans_bench.py.

``step`` is one assign + update, ``fit`` the loop with the final pass, ``predict`` the assignment alone.  Squared distances are taken
in the direct form (x-cx)^2 + (y-cy)^2 (+ (z-cz)^2); ties go to the lowest cluster (np.argmin); an empty cluster keeps its centre;
the loop stops when shift = max_k |c_new[k] - c_old[k]| <= tol.  Every assignment also reports the relative gap
(d2_second - d2_best) / d2_second per point (inf for k = 1, 0 where both are 0): where it is tiny, rounding may pick either cluster.
"""
import numpy as np


def sq_dists(data, centers):
    """(n,k) squared distances, direct form, summed x then y then z."""
    data, centers = np.asarray(data, dtype=np.float64), np.asarray(centers, dtype=np.float64)
    diff = data[:, None, :] - centers[None, :, :]
    d2 = diff[..., 0] * diff[..., 0]
    for c in range(1, data.shape[1]):
        d2 = d2 + diff[..., c] * diff[..., c]
    return d2


def predict(data, centers):
    """-> (labels, best squared distance per point, relative gap to the second-best)."""
    d2 = sq_dists(data, centers)
    labels = np.argmin(d2, axis=1)
    best = d2[np.arange(len(d2)), labels]
    if d2.shape[1] == 1:
        return labels, best, np.full(len(d2), np.inf)
    second = np.partition(d2, 1, axis=1)[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(second > 0, (second - best) / second, 0.0)
    return labels, best, gap


def step(data, centers):
    """One assign + update -> dict: centers (new), labels, counts (int64), sums (k,dim; zeros for an empty cluster), inertia (of the
    INPUT centres), shift, n_empty, gap (per point)."""
    data, centers = np.asarray(data, dtype=np.float64), np.asarray(centers, dtype=np.float64)
    k, dim = centers.shape
    labels, best, gap = predict(data, centers)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums = np.zeros((k, dim))
    for c in range(dim):
        sums[:, c] = np.bincount(labels, weights=data[:, c], minlength=k)
    new = centers.copy()
    live = counts > 0
    new[live] = sums[live] / counts[live, None]
    diff = new - centers
    q = diff[:, 0] * diff[:, 0]
    for c in range(1, dim):
        q = q + diff[:, c] * diff[:, c]
    return {"centers": new, "labels": labels, "counts": counts, "sums": sums, "inertia": float(best.sum()), "shift": float(np.sqrt(q).max()),
            "n_empty": int((~live).sum()), "gap": gap}


def fit(data, centers0, max_iter=300, tol=1e-4):
    """The loop and the final pass -> dict: centers, labels, counts, inertia (all under the final centres), n_iter, converged, n_empty,
    inertia_history, shift_history, min_gap (per iteration, the smallest relative gap over all points; the final pass last)."""
    data = np.asarray(data, dtype=np.float64)
    centers = np.array(centers0, dtype=np.float64)
    inertia_hist, shift_hist, min_gap, converged = [], [], [], False
    for _ in range(max_iter):
        s = step(data, centers)
        centers = s["centers"]
        inertia_hist.append(s["inertia"])
        shift_hist.append(s["shift"])
        min_gap.append(float(s["gap"].min()))
        if s["shift"] <= tol:
            converged = True
            break
    labels, best, gap = predict(data, centers)
    min_gap.append(float(gap.min()))
    counts = np.bincount(labels, minlength=len(centers)).astype(np.int64)
    return {"centers": centers, "labels": labels, "counts": counts, "inertia": float(best.sum()), "n_iter": len(shift_hist), "converged": converged,
            "n_empty": int((counts == 0).sum()), "inertia_history": np.array(inertia_hist), "shift_history": np.array(shift_hist),
            "min_gap": np.array(min_gap)}


def blobs(n, dim, lidar=False):
    """The seeded three-blob data of the mixture tests (tests/test_gpu_gmm.py: blobs); lidar: the blobs +-50 m out."""
    rng = np.random.default_rng(31 * n + dim + (7 if lidar else 0))
    centres = np.array([[0.5, 0.5, 0.2], [5.5, 2.5, -1.0], [1.0, 7.0, 2.0]]) if not lidar else np.array([[50.0, 10.0, -1.0], [-50.0, 5.0, 0.0], [0.0, -50.0, 1.0]])
    pts = centres[rng.integers(0, 3, n), :dim] + rng.normal(size=(n, dim)) * np.array([1.0, 1.7, 0.4])[:dim]
    pts.setflags(write=False)
    return pts


def seeds(data, k):
    """k distinct data rows drawn by default_rng(n + k)."""
    n = len(data)
    return np.array(data[np.random.default_rng(n + k).choice(n, k, replace=False)], dtype=np.float64)
