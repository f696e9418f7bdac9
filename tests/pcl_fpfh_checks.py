"""NumPy / cKDTree restatement of the PCL-rule descriptor rules of include/pcr.h (pcr_normals_knn, pcr_fpfh_pcl): k-nearest normals
flipped toward a viewpoint, the SPFH of a surface row over its radius ball (no cap; degenerate pairs skipped, K still counts them) and
the FPFH33 at keypoint COORDINATES (the 1/d^2-weighted sum over the ball, normalised per block, nothing added).

Everything is binary64.  Sums are taken in whatever order NumPy takes them: the device fixes an order of its own, and the bound of
tests/test_gpu_pcl_fpfh.py covers any order of non-negative terms.  Besides the values, ``spfh`` and ``fpfh33`` return the clean-row
bookkeeping of oracle_global.spfh(margins=True): per row the smallest distance of any of its binned pairs' three bin coordinates (11 x,
before the floor) from an integer -- a pair that close to a bin edge may land on either side of it under another libm."""
import numpy as np
from scipy.spatial import cKDTree


PAIRS_AT_ONCE = 2_000_000


def _d2(p, x):
    d = p - x
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def balls(points, centres, radius):
    """Per centre the rows of its ball, ascending: (dx*dx + dy*dy) + dz*dz <= r*r, evaluated in binary64 as written (the tree only
    proposes candidates, from a slightly larger radius).  A centre that is not finite has an empty ball."""
    p = np.asarray(points, dtype=np.float64)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    tree = cKDTree(p)
    r2 = radius * radius
    out = []
    for x in c:
        if not np.isfinite(x).all():
            out.append(np.zeros(0, dtype=np.int64))
            continue
        cand = np.array(sorted(tree.query_ball_point(x, radius * (1.0 + 1e-9) + 1e-300)), dtype=np.int64)
        out.append(cand[_d2(p[cand], x) <= r2] if len(cand) else cand)
    return out


def knn_normals(points, k, viewpoint=(0.0, 0.0, 0.0)):
    """-> dict(normals (N,3), curvature (N,), gap (N,)): the k nearest rows by (distance, row), the row itself included; the unit
    eigenvector of the covariance's smallest eigenvalue, flipped so that n . (vp - p) >= 0; curvature = e_min / (e0 + e1 + e2), 0 when
    the sum is 0; fewer than 3 rows in the neighbourhood: NaN.  ``gap`` = (e1 - e_min) / e_max, the conditioning of the normal."""
    p = np.asarray(points, dtype=np.float64)
    vp = np.asarray(viewpoint, dtype=np.float64)
    n = len(p)
    rows = np.arange(n)
    normals = np.full((n, 3), np.nan)
    curvature = np.full(n, np.nan)
    gap = np.zeros(n)
    for i in range(n):
        d2 = _d2(p, p[i])
        nb = np.lexsort((rows, d2))[:k]
        if len(nb) < 3:
            continue
        x = p[nb] - p[nb].mean(axis=0)
        w, v = np.linalg.eigh(x.T @ x / (len(nb) - 1))
        nrm = v[:, 0] / np.linalg.norm(v[:, 0])
        if nrm @ (vp - p[i]) < 0:
            nrm = -nrm
        normals[i] = nrm
        s = w[0] + w[1] + w[2]
        curvature[i] = w[0] / s if s != 0 else 0.0
        gap[i] = (w[1] - w[0]) / max(w[2], 1e-300)
    return dict(normals=normals, curvature=curvature, gap=gap)


def pair_features_many(p1, n1, p2, n2):
    """The Darboux frame of pcr_fpfh's SPFH for (P,3) arrays of pairs -> (f (P,3): f0, f1, f2; live (P,)).  A pair is not live -- it
    is skipped -- when its length is 0, when the cross product's norm is 0, or when a component of either normal is not finite."""
    live = np.isfinite(n1).all(axis=1) & np.isfinite(n2).all(axis=1)
    n1 = np.where(live[:, None], n1, 0.0)
    n2 = np.where(live[:, None], n2, 0.0)
    d = p2 - p1
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    live &= ln != 0.0
    lns = np.where(ln != 0.0, ln, 1.0)
    a1 = ((n1[:, 0] * d[:, 0] + n1[:, 1] * d[:, 1]) + n1[:, 2] * d[:, 2]) / lns
    a2 = ((n2[:, 0] * d[:, 0] + n2[:, 1] * d[:, 1]) + n2[:, 2] * d[:, 2]) / lns
    swap = np.abs(a1) < np.abs(a2)
    u = np.where(swap[:, None], n2, n1)
    w2 = np.where(swap[:, None], n1, n2)
    d = np.where(swap[:, None], -d, d)
    f2 = np.where(swap, -a2, a1)
    v = np.stack([d[:, 1] * u[:, 2] - d[:, 2] * u[:, 1], d[:, 2] * u[:, 0] - d[:, 0] * u[:, 2], d[:, 0] * u[:, 1] - d[:, 1] * u[:, 0]], axis=1)
    vn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    live &= vn != 0.0
    v = v / np.where(vn != 0.0, vn, 1.0)[:, None]
    w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    f1 = (v[:, 0] * w2[:, 0] + v[:, 1] * w2[:, 1]) + v[:, 2] * w2[:, 2]
    f0 = np.arctan2((w[:, 0] * w2[:, 0] + w[:, 1] * w2[:, 1]) + w[:, 2] * w2[:, 2], (u[:, 0] * w2[:, 0] + u[:, 1] * w2[:, 1]) + u[:, 2] * w2[:, 2])
    return np.stack([f0, f1, f2], axis=1), live


def bin_coordinates(f):
    """(P,3) features -> (P,3) bin coordinates, before the floor."""
    return np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], axis=1)


def spfh(points, normals, radius, rows=None, nbrs=None):
    """SPFH of the surface rows ``rows`` (None: every row) -> dict(values (R,33), counts (R,) = K, hist (R,33) the integer counts,
    margin (R,), n_spfh = R).  ``nbrs``: the balls of exactly those rows, when the caller has them."""
    p = np.asarray(points, dtype=np.float64)
    nrm = np.asarray(normals, dtype=np.float64)
    rows = np.arange(len(p)) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    nbrs = balls(p, p[rows], radius) if nbrs is None else nbrs
    R = len(rows)
    if sum(len(b) for b in nbrs) > PAIRS_AT_ONCE and R > 1:        # (the pair arrays of a large cloud: half the rows at a time)
        a = spfh(p, nrm, radius, rows[: R // 2], nbrs[: R // 2])
        b = spfh(p, nrm, radius, rows[R // 2:], nbrs[R // 2:])
        out = {k: np.concatenate([a[k], b[k]]) for k in ("values", "counts", "hist", "margin")}
        out["n_spfh"] = R
        return out
    K = np.array([len(b) for b in nbrs], dtype=np.int64)
    others = [b[b != r] for b, r in zip(nbrs, rows)]               # j != i by ROW NUMBER: a duplicate of the row is a pair (and is skipped)
    I = np.repeat(np.arange(R), [len(o) for o in others])
    J = np.concatenate(others + [np.zeros(0, dtype=np.int64)])
    f, live = pair_features_many(p[rows[I]], nrm[rows[I]], p[J], nrm[J])
    x = bin_coordinates(f[live])
    bins = np.minimum(np.maximum(np.floor(x), 0), 10).astype(np.int64) + np.array([0, 11, 22])
    hist = np.zeros((R, 33), dtype=np.int64)
    np.add.at(hist, (np.repeat(I[live], 3), bins.reshape(-1)), 1)
    scale = np.where(K > 1, 100.0 / np.maximum(K - 1, 1), 0.0)     # one product per bin: c_b * (100 / (K - 1))
    margin = np.full(R, np.inf)
    np.minimum.at(margin, I[live], np.abs(x - np.round(x)).min(axis=1))
    return dict(values=hist * scale[:, None], counts=K, hist=hist, margin=margin, n_spfh=R)


def fpfh33(points, normals, keypoints, radius):
    """FPFH33 at the keypoint coordinates -> dict(values (m,33) binary64, counts (m,) = |B(x)|, n_spfh = M the size of the union of
    the balls, margin (m,) = the smallest SPFH margin over the ball's rows, kmax = the largest ball met: of a keypoint or of a row whose
    SPFH it needs)."""
    p = np.asarray(points, dtype=np.float64)
    kp = np.asarray(keypoints, dtype=np.float64).reshape(-1, 3)
    m = len(kp)
    kb = balls(p, kp, radius)
    counts = np.array([len(b) for b in kb], dtype=np.int64)
    union = np.unique(np.concatenate(kb + [np.zeros(0, dtype=np.int64)]))
    s = spfh(p, normals, radius, rows=union)
    slot = np.full(len(p), -1, dtype=np.int64)
    slot[union] = np.arange(len(union))
    values = np.full((m, 33), np.nan)
    margin = np.full(m, np.inf)
    for i, b in enumerate(kb):
        if len(b) == 0:
            continue
        d2 = _d2(p[b], kp[i])
        use = d2 != 0.0
        F = (s["values"][slot[b[use]]] / d2[use][:, None]).sum(axis=0)
        tot = F.reshape(3, 11).sum(axis=1)
        scale = np.where(tot != 0.0, 100.0 / np.where(tot != 0.0, tot, 1.0), 0.0)
        values[i] = F * np.repeat(scale, 11)
        margin[i] = s["margin"][slot[b]].min()
    kmax = int(max(counts.max(initial=0), s["counts"].max(initial=0)))
    return dict(values=values, counts=counts, n_spfh=len(union), margin=margin, kmax=kmax, union=union, spfh=s)
