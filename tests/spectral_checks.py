"""NumPy float64 restatement of the spectral-clustering rules of include/pcr.h, shared by the spectral tests,
scripts/gen_spectral_golden.py and scripts/spectral_bench.py.

``graph``: the symmetrised k-NN graph as a CSR by row with the weight 1 / sqrt((dx*dx + dy*dy) + dz*dz), neighbours ordered by
(squared distance, row) like a stable sort, and the smallest relative gap between the nnk-th and the (nnk+1)-th other neighbour of
any row (where it is tiny, rounding may pick either).  ``operator`` / ``dense``: the symmetric operator B and its dense ``eigh``.
``embedding``: the columns with the unit norm and the sign rule.  ``maximin``: the default seeds.  ``fit``: all of it with
``kmeans_checks.fit`` on the embedding.
"""
import numpy as np

from tests import kmeans_checks


def lidar(n):
    """Three blobs 50 m apart (the data of the K-Means tests)."""
    return kmeans_checks.blobs(n, 3, lidar=True)


def bridge(n, seed=0):
    """Two elongated blobs 4.5 apart that touch: one component."""
    rng = np.random.default_rng(seed)
    h = n // 2
    a = rng.normal(size=(h, 3)) * [1, 1.7, .4]
    b = rng.normal(size=(n - h, 3)) * [1, 1.7, .4] + [4.5, 0, 0]
    pts = np.vstack([a, b])
    pts.setflags(write=False)
    return pts


def chain(n, seed=0):
    """Eight elongated blobs 4.5 apart in a row, each touching the next: one component.  The first n % 8 blobs hold one point more."""
    rng = np.random.default_rng(seed)
    pts = np.vstack([rng.normal(size=(n // 8 + (1 if i < n % 8 else 0), 3)) * [1, 1.7, .4] + [4.5 * i, 0, 0] for i in range(8)])
    pts.setflags(write=False)
    return pts


def blobs_even(n, seed=0):
    """Three blobs of n // 3 points each at the lidar centres of ``lidar``: three components of equal size."""
    rng = np.random.default_rng(seed)
    centres = np.array([[50.0, 10.0, -1.0], [-50.0, 5.0, 0.0], [0.0, -50.0, 1.0]])
    pts = np.vstack([c + rng.normal(size=(n // 3, 3)) * [1.0, 1.7, 0.4] for c in centres])
    pts.setflags(write=False)
    return pts


def circles(n=600, factor=.4, noise=.03, seed=1):
    """Two concentric rings (sklearn.datasets.make_circles restated: the outer ring first, then the inner one; 2-D)."""
    rng = np.random.RandomState(seed)
    n_out = n // 2
    n_in = n - n_out
    t_out = np.linspace(0, 2 * np.pi, n_out, endpoint=False)
    t_in = np.linspace(0, 2 * np.pi, n_in, endpoint=False)
    X = np.vstack([np.column_stack([np.cos(t_out), np.sin(t_out)]), np.column_stack([np.cos(t_in), np.sin(t_in)]) * factor])
    y = np.hstack([np.zeros(n_out, dtype=np.intp), np.ones(n_in, dtype=np.intp)])
    idx = rng.permutation(n)
    X, y = X[idx], y[idx]
    X = X + rng.normal(scale=noise, size=X.shape)
    return X, y


def _as3(data):
    data = np.asarray(data, dtype=np.float64)
    if data.shape[1] == 2:
        data = np.column_stack([data, np.zeros(len(data))])
    return data


def _d2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbours(data, nnk):
    """-> (idx (n, nnk+1), d2 (n, nnk+1)): the nnk + 1 nearest OTHER rows of every row by (squared distance, row)."""
    data = _as3(data)
    n = len(data)
    want = nnk + 1
    if n <= 2100:
        cand = np.broadcast_to(np.arange(n), (n, n))
    else:
        from scipy.spatial import cKDTree
        cand = cKDTree(data).query(data, k=min(n, want + 9))[1]
    d2 = _d2(data[:, None, :], data[cand])
    d2 = np.where(cand == np.arange(n)[:, None], np.inf, d2)      # the row itself is dropped by id
    order = np.lexsort((cand, d2), axis=1)[:, :want]
    rows = np.arange(n)[:, None]
    return cand[rows, order], d2[rows, order]


def graph(data, nnk):
    """-> dict: indptr (n+1,) int64, indices int32, weights, tie_gap, min_dist."""
    n = len(data)
    idx, d2 = neighbours(data, nnk)
    if idx.shape[1] > nnk:
        a, b = np.sqrt(d2[:, nnk - 1]), np.sqrt(d2[:, nnk])
        tie_gap = float(((b - a) / b).min())
    else:
        tie_gap = np.inf
    idx, dist = idx[:, :nnk], np.sqrt(d2[:, :nnk])
    r = np.repeat(np.arange(n, dtype=np.int64), nnk)
    c = idx.ravel().astype(np.int64)
    w = 1.0 / dist.ravel()
    keys = np.concatenate([r * n + c, c * n + r])
    keys, first = np.unique(keys, return_index=True)
    w = np.concatenate([w, w])[first]
    rows, cols = keys // n, keys % n
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return {"indptr": indptr, "indices": cols.astype(np.int32), "weights": w, "tie_gap": tie_gap, "min_dist": float(dist.min()), "rows": rows}


def degrees(g):
    """Row sums in column order."""
    return np.bincount(g["rows"], weights=g["weights"], minlength=len(g["indptr"]) - 1)


def csr(g):
    from scipy.sparse import csr_matrix
    n = len(g["indptr"]) - 1
    return csr_matrix((g["weights"], g["indices"], g["indptr"]), shape=(n, n))


def operator(g, normalized):
    """-> (B as scipy CSR, deg, scale): spectrum in [-1, 1], lambda = scale (1 - theta)."""
    from scipy.sparse import diags, identity
    W, deg = csr(g), degrees(g)
    if normalized:
        s = 1.0 / np.sqrt(deg)
        return diags(s) @ W @ diags(s), deg, 1.0
    dmax = deg.max()
    return identity(len(deg)) - (diags(deg) - W) / dmax, deg, dmax


def dense(g, normalized):
    """-> dict: lam (all eigenvalues of the Laplacian, ascending), U (eigenvectors of B, column j belongs to lam[j]), deg, scale."""
    B, deg, scale = operator(g, normalized)
    theta, U = np.linalg.eigh(B.toarray())
    return {"lam": scale * (1.0 - theta[::-1]), "U": U[:, ::-1], "deg": deg, "scale": scale}


def embedding(U, deg, m, normalized):
    """Columns j < m: D^-1/2 u_j (normalized) or u_j, unit 2-norm, the entry of largest magnitude positive (lowest row on ties)."""
    V = np.array(U[:, :m] / np.sqrt(deg)[:, None] if normalized else U[:, :m])
    for j in range(m):
        big = int(np.argmax(np.abs(V[:, j])))        # the first of equals
        V[:, j] *= (-1.0 if V[big, j] < 0 else 1.0) / np.sqrt((V[:, j] * V[:, j]).sum())
    return V


def maximin(E, k):
    """Seed 0 = row 0; seed j = the row with the largest minimum squared distance to the seeds before it, the lowest row on ties."""
    seeds = [0]
    mind = None
    for _ in range(1, k):
        d2 = kmeans_checks.sq_dists(E, E[seeds[-1]][None, :])[:, 0]
        mind = d2 if mind is None else np.minimum(mind, d2)
        seeds.append(int(np.argmax(mind)))
    return np.array(seeds, dtype=np.int64)


def fit(data, m, nnk=7, normalized=True, seed_rows=None, kmeans_tol=1e-4, kmeans_max_iter=300):
    g = graph(data, nnk)
    d = dense(g, normalized)
    E = embedding(d["U"], d["deg"], m, normalized)
    seeds = maximin(E, m) if seed_rows is None else np.asarray(seed_rows, dtype=np.int64)
    km = kmeans_checks.fit(E, E[seeds], max_iter=kmeans_max_iter, tol=kmeans_tol)
    return {"graph": g, "lam": d["lam"], "U": d["U"], "deg": d["deg"], "scale": d["scale"], "embedding": E, "seed_rows": seeds, "kmeans": km,
            "labels": km["labels"]}


def same_partition(a, b):
    """Two labelings describe the same partition."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))
