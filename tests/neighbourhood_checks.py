"""Restatements and input builders for the edge tests of pcr_pca, pcr_normals, pcr_iss and pcr_dbscan (NumPy / SciPy only).

ball_in            scipy's query_ball_point membership, the rule ISS and DBSCAN follow: (dx*dx + dy*dy) + dz*dz <= fl(r*r) in binary64
                   (pinned against cKDTree by tests/test_neighbourhood_host.py).
band_pairs         isolated pairs of points whose squared distance sits exactly at that boundary: "band" pairs just outside it
                   that the kd-tree API's rule `not (sqrt(d2) > r)` would still take, and "edge-in" pairs on it or one ulp inside.
normals_cell / normals_redo_rows
                   the level-0 cell pcr_normals asks for (pcr_normals.hip, with pcr_grid_plan's fallbacks) and the rows its 27-cell
                   scan cannot prove, which pcr_knn and the host PCA must redo.
core_and_outliers, lattice, line_cloud, with_duplicates
                   clouds that put a chosen number of rows on the redo path, or whose distances tie exactly.
normals_reference  neighbours in the kernels' (d2, index) order, covariances accumulated in np.longdouble.
pca_reference      the same for a whole cloud.
iss_nms            ISS.py:55-73 on given eigenvalues: ratio tests, order, suppression, the stop.
No library code is imported here."""
import numpy as np
from scipy.spatial import cKDTree

from oracle import oracle_np as oracle


# ------------------------------------------------------------------ the ball
def ball_in(q, p, r):
    """query_ball_point's decision for p around q (arrays broadcast over leading axes)."""
    return oracle.dist2_direct(q, p) <= np.float64(r) * np.float64(r)


def norm_rule_in(q, p, r):
    """The kd-tree / octree API's decision (result_set.py:80 rejects dist > radius)."""
    return ~(np.sqrt(oracle.dist2_direct(q, p)) > np.float64(r))


def boundary_cases(r, count, seed):
    """`count` (q, p) with |p - q| = r up to a few ulps: q uniform in the unit cube, p = q + r * unit vector, one coordinate of p
    nudged by -3..+3 ulps."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, 1.0, (count, 3))
    u = rng.normal(size=(count, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = q + r * u
    ax = rng.integers(0, 3, count)
    steps = rng.integers(-3, 4, count)
    rows = np.arange(count)
    v = p[rows, ax]
    for s in range(1, 4):
        v = np.where(steps >= s, np.nextafter(v, np.inf), v)
        v = np.where(steps <= -s, np.nextafter(v, -np.inf), v)
    p[rows, ax] = v
    return q, p


def band_pairs(r, count, seed, spacing=10.0):
    """Up to `count` isolated pairs at the boundary of the ball of radius r, as {"band": (Q, P), "edge": (Q, P)}.

    Trial t lives at x = spacing * t + [0, 1) with y, z in [0, r), so no point of another trial is within spacing - 1 - r of
    it.  p = q + r * unit vector in x and z; x carries the offset, so its difference is exact but coarse, and p's y is solved
    from the computed dx and dz so that d2 comes out at r*r.  y and z are of the size of r: one ulp of them moves d2 by a few
    ulps of r*r.  Then p's y or z is stepped by -3..+3 ulps until the pair falls into the class the trial is after (even
    trials: band, odd trials: edge-in).  Trials that find nothing are dropped.
      band     ball_in False, `not (sqrt(d2) > r)` True: one ulp of d2 at r = 0.5 and r = 0.08, none at r = 0.3 and r = 0.6
      edge     d2 == fl(r*r) or one ulp below: inside under both rules"""
    rng = np.random.default_rng(seed)
    r = np.float64(r)
    r2 = r * r
    out = {"band": ([], []), "edge": ([], [])}
    for t in range(count):
        q = np.array([spacing * t + rng.uniform(0.0, 1.0), rng.uniform(0.0, r), rng.uniform(0.0, r)])
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        p0 = q + r * u
        dx, dz = q[0] - p0[0], q[2] - p0[2]
        rest = r2 - dx * dx - dz * dz
        want = "band" if t % 2 == 0 else "edge"
        if not rest > 0:
            continue
        p0[1] = q[1] + np.copysign(np.sqrt(rest), u[1])
        found = None
        for ax in (1, 2):
            for step in (0, 1, -1, 2, -2, 3, -3):
                p = p0.copy()
                for _ in range(abs(step)):
                    p[ax] = np.nextafter(p[ax], np.inf if step > 0 else -np.inf)
                d2 = oracle.dist2_direct(q, p)
                if want == "band":
                    ok = d2 > r2 and not np.sqrt(d2) > r
                else:
                    ok = d2 == r2 or d2 == np.nextafter(r2, 0.0)
                if ok:
                    found = p
                    break
            if found is not None:
                break
        if found is not None:
            out[want][0].append(q)
            out[want][1].append(found)
    return {k: (np.array(a).reshape(-1, 3), np.array(b).reshape(-1, 3)) for k, (a, b) in out.items()}


def pairs_cloud(*pairs):
    """(Q, P), ... -> one cloud Q0, P0, Q1, P1, ... and, per group, the rows of its q's (the p of row i is row i + 1)."""
    pts, rows, base = [], [], 0
    for q, p in pairs:
        both = np.empty((2 * len(q), 3))
        both[0::2], both[1::2] = q, p
        pts.append(both)
        rows.append(base + 2 * np.arange(len(q)))
        base += 2 * len(q)
    return np.concatenate(pts), rows


# ---------------------------------------------------------- clouds for normals
def core_and_outliers(m, seed=0):
    """1500 points on a unit square (sigma_z = 0.01) + m points uniform in [-5,5]^2 x [-1,1], shuffled: the outliers stretch the
    bounding box (and with it the cell) without coming near each other, so about m rows cannot be proven by the 27-cell scan."""
    rng = np.random.default_rng(seed)
    core = np.column_stack([rng.uniform(0, 1, 1500), rng.uniform(0, 1, 1500), rng.normal(0, 0.01, 1500)])
    out = np.column_stack([rng.uniform(-5, 5, m), rng.uniform(-5, 5, m), rng.uniform(-1, 1, m)])
    pts = np.concatenate([core, out])
    return pts[rng.permutation(len(pts))]


# outliers of core_and_outliers -> the number of redo rows it is built to give: the three routes of pcr_knn (pcr_knn.hip)
REDO_CLASSES = {6: (1, 16), 60: (17, 255), 300: (256, 10**9)}


def lattice(nx, ny, nz, spacing):
    """Regular lattice, x fastest: every distance ties with many others, exactly (coordinates are multiples of `spacing`)."""
    g = np.mgrid[0:nz, 0:ny, 0:nx].reshape(3, -1).T[:, ::-1].astype(np.float64)
    return g * spacing


def line_cloud(n=300):
    """n distinct points along x, y = z = 0: two zero extents, so pcr_normals asks for cell 0 and the planner picks emax / 64."""
    rng = np.random.default_rng(7)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    return np.column_stack([x, np.zeros(n), np.zeros(n)])


def with_duplicates(pts, frac, seed):
    """pts with round(frac * n) of its rows overwritten by copies of other rows (exact duplicates), n unchanged."""
    rng = np.random.default_rng(seed)
    n = len(pts)
    m = int(round(frac * n))
    dst = rng.choice(n, m, replace=False)
    src = rng.choice(np.setdiff1d(np.arange(n), dst), m)
    out = pts.copy()
    out[dst] = out[src]
    return out


def normals_cell(pts, k):
    """The level-0 cell of the grid pcr_normals builds: 1.8 * sqrt(k/5 * e0 * e1 / n) over the two largest extents; with a zero
    area pcr_grid_plan chooses 0.55 * sqrt(area / n), else emax / 64, else 1; never below emax / 262144."""
    pts = np.asarray(pts, dtype=np.float64)
    n = len(pts)
    e = np.sort(pts.max(axis=0) - pts.min(axis=0))[::-1]
    emax = e[0]
    cell = 1.8 * np.sqrt(k / 5.0 * e[0] * e[1] / n) if e[0] * e[1] > 0 else 0.0
    if not cell > 0:
        area = e[0] * e[1]
        cell = 0.55 * np.sqrt(area / n) if area > 0 else (emax / 64.0 if emax > 0 else 1.0)
    cell = max(cell, emax / 262144.0)
    if not cell > 0:
        cell = 1.0
    return float(cell)


def knn_d2(pts, k):
    """(idx (n,kk), d2 (n,kk)) of every point's kk = min(k, n) nearest (itself included) in (d2, index) order."""
    pts = np.asarray(pts, dtype=np.float64)
    kk = min(k, len(pts))
    idx, _ = oracle.knn_exact(pts, pts, kk)
    return idx, oracle.dist2_direct(pts[:, None, :], pts[idx])


def normals_redo_rows(pts, k):
    """Rows the one-lane scan of pcr_normals must hand to the redo path (n > k): the k-th neighbour's d2 exceeds
    (cell * (1 - 1e-9))^2, so a point outside the 27 cells could be as close."""
    pts = np.asarray(pts, dtype=np.float64)
    if len(pts) <= k:
        return np.zeros(0, dtype=np.int64)
    _, d2 = knn_d2(pts, k)
    safe = normals_cell(pts, k) * (1.0 - 1e-9)
    return np.flatnonzero(~(d2[:, k - 1] <= safe * safe))


# ------------------------------------------------------- references, longdouble
def cov_longdouble(x):
    """np.cov(x.T) (divisor n - 1) and the mean, accumulated in np.longdouble; one point: zero matrix (what pcr_normals takes)."""
    x = np.asarray(x, dtype=np.longdouble)
    mean = x.sum(axis=0) / len(x)
    c = x - mean
    S = c.T @ c
    S = S / (len(x) - 1) if len(x) > 1 else S * 0
    return S, mean


def eig_desc(S):
    """np.linalg.eigh of the binary64 rounding of S: eigenvalues descending, eigenvectors as columns."""
    w, v = np.linalg.eigh(np.asarray(S, dtype=np.float64))
    return w[::-1].copy(), v[:, ::-1].copy()


def pca_reference(pts):
    S, mean = cov_longdouble(pts)
    w, v = eig_desc(S)
    return w, v, np.asarray(mean, dtype=np.float64), np.asarray(S, dtype=np.float64)


def normals_reference(pts, k):
    """-> (nbr (n,k) int64 in (d2, index) order, -1 past the cloud's size; evs (n,3) descending; normals (n,3); covs (n,3,3))."""
    pts = np.asarray(pts, dtype=np.float64)
    n = len(pts)
    idx, _ = knn_d2(pts, k)
    kk = idx.shape[1]
    nbr = np.full((n, k), -1, dtype=np.int64)
    nbr[:, :kk] = idx
    x = pts[idx].astype(np.longdouble)                       # (n, kk, 3)
    c = x - x.sum(axis=1, keepdims=True) / kk
    S = np.einsum("nki,nkj->nij", c, c)
    S = S / (kk - 1) if kk > 1 else S * 0
    covs = S.astype(np.float64)
    w, v = np.linalg.eigh(covs)
    return nbr, w[:, ::-1].copy(), v[:, :, 0].copy(), covs


def check_normals_exact(pts, k, got, ref=None, eig_tol=1e-9, res_tol=1e-9, dir_tol=1e-7):
    """Every row of estimate_normals(..., return_details=True) against normals_reference: neighbours equal in order; eigenvalues
    within eig_tol * lambda_1; |C n - lambda_3 n| <= res_tol * lambda_1; the direction within dir_tol where (lambda_2 -
    lambda_3) / lambda_1 > 1e-4; unit normals.  Returns the largest figures for the docstrings."""
    nrm, evs, nbr = got
    r_nbr, r_evs, r_nrm, covs = ref if ref is not None else normals_reference(pts, k)
    assert nbr.dtype == np.int32 and nbr.shape == r_nbr.shape
    bad = np.flatnonzero((nbr != r_nbr).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], nbr[bad[:5]], r_nbr[bad[:5]])
    assert np.isfinite(nrm).all() and np.isfinite(evs).all()
    unit = np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max()
    assert unit <= 1e-12, unit
    scale = np.maximum(r_evs[:, 0], 1e-300)
    e_err = (np.abs(evs - r_evs).max(axis=1) / scale)
    assert (evs[:, 0] >= evs[:, 1]).all() and (evs[:, 1] >= evs[:, 2]).all()
    assert e_err.max() <= eig_tol, (e_err.max(), int(e_err.argmax()))
    res = np.linalg.norm(np.einsum("nij,nj->ni", covs, nrm) - evs[:, 2:3] * nrm, axis=1) / scale
    assert res.max() <= res_tol, (res.max(), int(res.argmax()))
    well = (r_evs[:, 1] - r_evs[:, 2]) / scale > 1e-4
    d_err = np.abs(np.abs(np.einsum("ij,ij->i", nrm[well], r_nrm[well])) - 1.0)
    if well.any():
        assert d_err.max() <= dir_tol, (d_err.max(), int(np.flatnonzero(well)[d_err.argmax()]))
    return {"eig": float(e_err.max()), "res": float(res.max()), "dir": float(d_err.max()) if well.any() else 0.0, "well": int(well.sum())}


# ------------------------------------------------------------------------ ISS
def iss_candidates(lam, g21, g32):
    """ISS.py:55 on given eigenvalues (rows descending): NaN ratios (isolated points: 0/0) fail like the reference's comparisons."""
    lam = np.asarray(lam, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.flatnonzero((lam[:, 1] / lam[:, 0] < g21) & (lam[:, 2] / lam[:, 1] < g32))


def iss_nms(pts, lam, g21, g32, nms_radius, count):
    """ISS.py:55-73 on given eigenvalues: candidates by the ratio tests, visited by descending lambda_3 (stable: ties by row),
    one is kept unless an already kept keypoint is ball_in(nms_radius) of it, the walk stops once MORE than `count` are kept."""
    pts = np.asarray(pts, dtype=np.float64)[:, :3]
    cand = iss_candidates(lam, g21, g32)
    order = cand[np.argsort(-np.asarray(lam)[cand, 2], kind="stable")]
    kept = []
    kept_pts = np.zeros((0, 3))
    for i in order:
        if len(kept) and ball_in(pts[i], kept_pts, nms_radius).any():
            continue
        kept.append(int(i))
        kept_pts = np.vstack([kept_pts, pts[i]])
        if len(kept) > count:
            break
    return kept


def nms_boundary_blobs(kind, nms_radius=0.5, seed=0):
    """Two copies of one 80-point blob (inside a ball of radius 0.12; ISS radius 0.1, ratios 0.95), the second translated by T with
    |T| = nms_radius, so that the copies' strongest candidates a and 80 + a -- visited first and second: everything else of a
    copy lies within 0.24 of its strongest and is suppressed by it -- are a band pair (kind "band": both must be kept) or an
    edge-in pair (kind "edge": the second must be dropped).  T is searched until the computed d2 falls into the class.  The
    copies are >= nms_radius - 0.24 apart, beyond the ISS radius: their eigenvalues are those of the blob alone, up to rounding.
    -> (points (160, 3), a)"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(80, 3))
    blob = 0.12 * u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0, 1, (80, 1)) ** (1 / 3) + 0.125
    _, lam, _ = oracle.iss_oracle(blob, radius=0.1, lambda21=0.95, lambda32=0.95, non_max_radius=nms_radius, iss_count=20)
    cand = iss_candidates(lam, 0.95, 0.95)
    top = cand[np.argsort(-lam[cand, 2], kind="stable")]
    a = int(top[0])
    assert lam[top[0], 2] > lam[top[1], 2] * (1 + 1e-6)               # rounding cannot reorder the strongest two of a copy
    r = np.float64(nms_radius)
    r2 = r * r
    for _ in range(20000):
        t = rng.normal(size=3)
        t *= r / np.linalg.norm(t)
        other = blob + t
        d2 = oracle.dist2_direct(blob[a], other[a])
        if kind == "band":
            ok = d2 > r2 and not np.sqrt(d2) > r
        else:
            ok = d2 == r2 or d2 == np.nextafter(r2, 0.0)
        if ok:
            return np.concatenate([blob, other]), a
    raise AssertionError("no translation found")


def ball_counts(pts, r):
    """|N(p_i)| by cKDTree.query_ball_point (self included)."""
    pts = np.asarray(pts, dtype=np.float64)
    return cKDTree(pts).query_ball_point(pts, r, return_length=True, workers=oracle.KD_WORKERS).astype(np.int64)
