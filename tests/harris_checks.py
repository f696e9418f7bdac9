"""NumPy float64 restatement of the PCL-keypoint rules of include/pcr.h (radius normals, Harris-3D response, suppression, corner
refinement, PCL-rule ISS), shared by tests/test_harris_host.py, tests/test_gpu_harris.py and scripts/harris_bench.py.

"Within r" is (dx*dx + dy*dy) + dz*dz <= r*r on the float64 coordinates, the point itself included.  Neighbour lists are in
ascending row, so the sums here run in row order; the device sums in another (fixed) order, hence tolerances, never bit equality.
Every function also reports how close a decision was (eigen-gap, margins), so that a test can tell a contested row from a wrong one.
"""
import numpy as np

try:  # the ball queries only: candidates from the tree, the rule itself applied in float64 below
    from scipy.spatial import cKDTree
except Exception:  # pragma: no cover
    cKDTree = None


def neighbours(points, r, centres=None):
    """-> list of int arrays: the rows within r of every centre (default: of every point), ascending."""
    pts = np.asarray(points, dtype=np.float64)
    ctr = pts if centres is None else np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    r2 = float(r) * float(r)
    if cKDTree is not None:
        lists = cKDTree(pts).query_ball_point(ctr, float(r) * (1.0 + 1e-9) + 1e-300)
    else:
        lists = [np.arange(len(pts))] * len(ctr)
    out = []
    for c, cand in zip(ctr, lists):
        cand = np.sort(np.asarray(cand, dtype=np.int64))
        d = pts[cand] - c
        out.append(cand[(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2])
    return out


def normals_radius(points, r, viewpoint=(0.0, 0.0, 0.0), nb=None):
    """-> dict: normals (n,3; NaN rows where m < 3), counts (n,), eigvals (n,3 ascending; NaN where m < 3),
    gap (n,) = (w1 - w0) / w2: where it is tiny the smallest eigenvector is not determined."""
    pts = np.asarray(points, dtype=np.float64)
    vp = np.asarray(viewpoint, dtype=np.float64)
    nb = neighbours(pts, r) if nb is None else nb
    n = len(pts)
    normals = np.full((n, 3), np.nan)
    w_all = np.full((n, 3), np.nan)
    counts = np.array([len(j) for j in nb], dtype=np.int64)
    for i in range(n):
        m = counts[i]
        if m < 3:
            continue
        x = pts[nb[i]] - pts[i]
        mean = x.sum(axis=0) / m
        cov = x.T @ x / m - np.outer(mean, mean)
        w, v = np.linalg.eigh(cov)
        nrm = v[:, 0] / np.linalg.norm(v[:, 0])
        if nrm @ (vp - pts[i]) < 0:
            nrm = -nrm
        normals[i] = nrm
        w_all[i] = w
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (w_all[:, 1] - w_all[:, 0]) / w_all[:, 2]
    return {"normals": normals, "counts": counts, "eigvals": w_all, "gap": gap}


def response(points, r, normals, nb=None):
    """-> dict: response (n,), k (n,) neighbours with a finite normal, counts (n,)."""
    pts = np.asarray(points, dtype=np.float64)
    nrm = np.asarray(normals, dtype=np.float64)
    nb = neighbours(pts, r) if nb is None else nb
    fin = np.isfinite(nrm).all(axis=1)
    n = len(pts)
    resp = np.zeros(n)
    ks = np.zeros(n, dtype=np.int64)
    for i in range(n):
        j = nb[i][fin[nb[i]]]
        ks[i] = len(j)
        if not fin[i] or len(j) == 0:
            continue
        q = nrm[j]
        C = q.T @ q / len(j)
        xx, xy, xz, yy, yz, zz = C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]
        trace = xx + yy + zz
        if trace == 0:
            continue
        det = xx * yy * zz + 2 * xy * xz * yz - xz * xz * yy - xy * xy * zz - yz * yz * xx
        resp[i] = 0.04 + det - 0.04 * trace * trace
    return {"response": resp, "k": ks, "counts": np.array([len(j) for j in nb], dtype=np.int64)}


def suppress(score, cand, nb):
    """-> (kept rows ascending, margin (n,)): a candidate is kept iff no row of its ball has a strictly greater score; margin = s_i minus
    the largest OTHER score of the ball (+inf for a lone row): |margin| tiny = a contested decision."""
    score = np.asarray(score, dtype=np.float64)
    n = len(score)
    margin = np.full(n, np.inf)
    keep = np.zeros(n, dtype=bool)
    for i in range(n):
        others = nb[i][nb[i] != i]
        top = score[others].max() if len(others) else -np.inf
        margin[i] = score[i] - top
        keep[i] = bool(cand[i]) and not (top > score[i])
    return np.flatnonzero(keep), margin


def refine(points, normals, r, corners, max_rounds=5):
    """-> (refined (k,3), rounds (k,)): c <- A^-1 b with A = sum n n^T, b = sum (n n^T) p over the rows within r of c that have a finite
    normal, by the adjugate, while det A != 0; the round whose squared move is <= 1e-6 is the last."""
    pts = np.asarray(points, dtype=np.float64)
    nrm = np.asarray(normals, dtype=np.float64)
    fin = np.isfinite(nrm).all(axis=1)
    out = np.array(corners, dtype=np.float64).reshape(-1, 3)
    rounds = np.zeros(len(out), dtype=np.int64)
    for k in range(len(out)):
        c = out[k].copy()
        for _ in range(max_rounds):
            rounds[k] += 1
            j = neighbours(pts, r, c)[0]
            j = j[fin[j]]
            q = nrm[j]
            A = q.T @ q if len(j) else np.zeros((3, 3))
            b = np.einsum("ja,jb,jb->a", q, q, pts[j]) if len(j) else np.zeros(3)
            xx, xy, xz, yy, yz, zz = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
            det = xx * yy * zz + 2 * xy * xz * yz - xz * xz * yy - xy * xy * zz - yz * yz * xx
            new = c
            if det != 0:
                adj = np.array([[yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy],
                                [xz * yz - xy * zz, xx * zz - xz * xz, xy * xz - xx * yz],
                                [xy * yz - xz * yy, xy * xz - xx * yz, xx * yy - xy * xy]])
                new = adj @ b / det
            move2 = float(((new - c) ** 2).sum())
            c = new
            if not move2 > 1e-6:
                break
        out[k] = c
    return out, rounds


def harris3d(points, radius, threshold, normals=None, nms=True, do_refine=False):
    """-> dict: normals, response, k, counts, rows (keypoints, ascending), margin (suppression), contested (bool per row: the response is
    within 1e-6 of the largest other response of its ball or of the threshold), candidates (bool), refined / rounds (with do_refine)."""
    pts = np.asarray(points, dtype=np.float64)
    nb = neighbours(pts, radius)
    est = None
    if normals is None:
        est = normals_radius(pts, radius, nb=nb)
        normals = est["normals"]
    res = response(pts, radius, normals, nb=nb)
    resp = res["response"]
    out = {"normals": np.asarray(normals, dtype=np.float64), "estimate": est, **res}
    if not nms:
        out["rows"] = np.arange(len(pts))
        return out
    cand = resp >= threshold
    rows, margin = suppress(resp, cand, nb)
    out.update(rows=rows, margin=margin, candidates=cand, contested=(np.abs(margin) < 1e-6) | (np.abs(resp - threshold) < 1e-6))
    if do_refine:
        out["refined"], out["rounds"] = refine(pts, normals, radius, pts[rows])
    return out


def iss_pcl(points, salient_radius, non_max_radius, gamma21, gamma32, min_neighbors):
    """-> dict: score (n,; e3 where the rules hold, else 0), eigvals (n,3 descending), counts (within non_max_radius), candidates,
    rows (keypoints), margin (suppression), rel_margin (|margin| / score: where tiny, rounding decides)."""
    pts = np.asarray(points, dtype=np.float64)
    n = len(pts)
    nb_s = neighbours(pts, salient_radius)
    nb_n = neighbours(pts, non_max_radius)
    score = np.zeros(n)
    eig = np.zeros((n, 3))
    for i in range(n):
        x = pts[nb_s[i]] - pts[i]
        e3, e2, e1 = np.linalg.eigvalsh(x.T @ x)
        eig[i] = (e1, e2, e3)
        if e1 > 0 and e2 > 0 and e3 >= 0 and e2 / e1 < gamma21 and e3 / e2 < gamma32:
            score[i] = e3
    counts = np.array([len(j) for j in nb_n], dtype=np.int64)
    cand = (score > 0) & (counts >= min_neighbors)
    rows, margin = suppress(score, cand, nb_n)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(score > 0, np.abs(margin) / score, np.inf)
    return {"score": score, "eigvals": eig, "counts": counts, "candidates": cand, "rows": rows, "margin": margin, "rel_margin": rel}


def corner_cloud(side=15, step=0.1, jitter=0.002, seed=5):
    """Three mutually orthogonal side x side faces meeting at the origin (the planes x = 0, y = 0, z = 0 over [0, (side-1) step]^2), every
    coordinate jittered by a seeded normal of that sigma.  -> (points (3 side^2, 3), the true corner (3,))."""
    g = np.arange(side) * step
    a, b = [m.ravel() for m in np.meshgrid(g, g, indexing="ij")]
    z = np.zeros_like(a)
    pts = np.concatenate([np.stack([z, a, b], axis=1), np.stack([a, z, b], axis=1), np.stack([a, b, z], axis=1)])
    if jitter:
        pts = pts + np.random.default_rng(seed).normal(size=pts.shape) * jitter
    pts.setflags(write=False)
    return pts, np.zeros(3)
