"""GPU: randomised parity sweep of BOTH exact 1-NN paths -- grid (tile directory through the block tables, grouped filter,
hard stage) and brute force (f64 MFMA sweep, group argmin, proven-or-fallback) -- and of the fused ICP moments against the CPU oracle -- shapes, densities, cell sizes and offsets the fixed
tests do not cover.  Every case is seeded; distances must be bit-identical, indices equal outside exact ties."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIE_MARGIN = 1e-12


def _cloud(rng, kind, n):
    if kind == "uniform":
        return rng.uniform(-5, 5, (n, 3))
    if kind == "plane":
        p = rng.uniform(-20, 20, (n, 3))
        p[:, 2] = 0.01 * rng.normal(size=n)
        return p
    if kind == "line":
        t = rng.uniform(-50, 50, n)
        return np.c_[t, 0.3 * t + 1e-3 * rng.normal(size=n), 2.0 + 1e-3 * rng.normal(size=n)]
    if kind == "clusters":
        c = rng.uniform(-30, 30, (12, 3))
        return c[rng.integers(0, 12, n)] + rng.normal(0, 0.05, (n, 3)) * rng.uniform(0.1, 10, (n, 1))
    if kind == "shell":
        v = rng.normal(size=(n, 3))
        return 25.0 * v / np.linalg.norm(v, axis=1, keepdims=True) + rng.normal(0, 0.02, (n, 3))
    if kind == "lattice":  # many exact ties
        g = rng.integers(0, 12, (n, 3)).astype(np.float64) * 0.25
        return g
    raise ValueError(kind)


CASES = [
    # kind, n_tgt, n_q, cell (0 = automatic), offset, query spread
    ("uniform", 1, 50, 0.0, 0.0, 1.0), ("uniform", 2, 50, 0.0, 0.0, 1.0), ("uniform", 3, 64, 0.0, 0.0, 1.0),
    ("uniform", 63, 63, 0.0, 0.0, 1.0), ("uniform", 64, 65, 0.0, 0.0, 1.0), ("uniform", 65, 1, 0.0, 0.0, 1.0),
    ("uniform", 5000, 4097, 0.0, 0.0, 1.2), ("uniform", 5000, 3000, 0.01, 0.0, 1.0), ("uniform", 5000, 3000, 50.0, 0.0, 1.0),
    ("plane", 30000, 9000, 0.0, 0.0, 1.0), ("plane", 30000, 9000, 0.05, 1.0e5, 1.0), ("line", 20000, 5000, 0.0, 0.0, 1.0),
    ("clusters", 40000, 10000, 0.0, 0.0, 1.0), ("clusters", 40000, 10000, 0.02, -3.0e4, 1.5), ("shell", 25000, 8000, 0.0, 0.0, 0.9),
    ("shell", 25000, 8000, 1.0, 0.0, 2.0), ("lattice", 8000, 4000, 0.0, 0.0, 1.0), ("lattice", 8000, 4000, 0.1, 7.0e3, 1.1),
]


@pytest.mark.parametrize("nn", ["grid", "brute"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_nn1_fuzz(pcp, oracle, case, nn):
    kind, n_t, n_q, cell, off, spread = CASES[case]
    rng = np.random.default_rng(1000 + case)
    tgt = _cloud(rng, kind, n_t) + off
    # queries: a mix of perturbed target points, points of the same distribution, and far outliers
    a = tgt[rng.integers(0, n_t, n_q // 2)] + rng.normal(0, 0.03, (n_q // 2, 3))
    b = (_cloud(rng, kind, n_q - n_q // 2) * spread) + off
    q = np.concatenate([a, b])
    if n_q >= 100:
        q[:5] += 500.0          # far outside the grid
        q[5:10] = tgt[:5] if n_t >= 5 else q[5:10]   # exact hits (distance 0)
    index = pcp.TargetIndex(tgt, kind=nn, cell=cell)
    idx, d2 = index.nn1(q)
    oi, od2, margin = oracle.nn1_exact(q, tgt)
    assert np.array_equal(d2, od2), (kind, n_t, cell, nn)
    clear = margin > TIE_MARGIN
    assert np.array_equal(idx[clear], oi[clear])
    # on exact ties the lowest index wins
    tie = ~clear
    if tie.any():
        dd = ((q[tie][:, None, :] - tgt[None, :, :]) ** 2)
        dm = (dd[..., 0] + dd[..., 1]) + dd[..., 2]
        exact_tie = (dm == od2[tie][:, None])
        assert np.array_equal(idx[tie], exact_tie.argmax(axis=1))
    # gated + transformed pass through the fused ICP kernels
    T = np.eye(4)
    T[:3, 3] = rng.normal(0, 0.05, 3)
    gate = float(np.quantile(od2, 0.8)) if n_q > 10 else 0.0
    if gate > 0:
        m, o, s = index.moments(q, T, max_d2=gate)
        qt = q + T[:3, 3]
        _, od2t, _ = oracle.nn1_exact(qt, tgt)
        keep = od2t < gate
        assert int(round(m[0])) == int(keep.sum())
        assert abs(s - od2t[keep].sum()) <= 1e-9 * max(1.0, od2t[keep].sum())


VOX = [("uniform", 1, 0.5), ("uniform", 2, 0.5), ("uniform", 7, 0.01), ("uniform", 5000, 0.37), ("uniform", 5000, 3.0), ("uniform", 5000, 11.0),
       ("plane", 20000, 0.25), ("line", 20000, 0.1), ("clusters", 30000, 0.05), ("lattice", 8000, 0.25), ("lattice", 8000, 0.2499999), ("shell", 25000, 1.7)]


@pytest.mark.parametrize("case", range(len(VOX)))
def test_voxel_filter_fuzz_bit_exact(pcp, oracle, case):
    """voxel_filter.py semantics on shapes the goldens do not cover: keys, D and centroids bit-exact against the restatement
    that is itself pinned to the reference's outputs (lattice points sit exactly ON voxel boundaries)."""
    kind, n, leaf = VOX[case]
    rng = np.random.default_rng(2000 + case)
    pts = _cloud(rng, kind, n) + rng.uniform(-100, 100, 3)
    if case % 2:
        pts = pts.astype(np.float32).astype(np.float64)
    h, D = pcp.voxel_keys(pts, leaf)
    oh, oD = oracle.voxel_keys(pts, leaf)
    assert np.array_equal(D, oD) and np.array_equal(h, oh)
    out = pcp.voxel_filter(pts, leaf, "centroid")
    ref = oracle.voxel_filter(pts, leaf, "centroid")[0]
    if ref.size == 0:
        assert out.size == 0          # one occupied voxel: the reference returns an empty array (its last group is never emitted)
    else:
        assert out.shape == ref.shape and np.array_equal(out, ref)


def _populous(rng, counts, f32=False, shift=0.0):
    """One unit cube per entry of `counts` along x (cube i holds counts[i] points), then a final singleton voxel (the group the
    reference never emits); shuffled, so that the input order inside a voxel is not the storage order.  `shift` = 0.5 aligns the
    cubes with Open3D's voxels (origin = min - voxel / 2)."""
    parts = [rng.uniform(0.0, 1.0, (c, 3)) * 0.998 + 0.001 + np.array([float(i), 0.0, 0.0]) + shift for i, c in enumerate(counts)]
    parts.append(np.array([[len(counts) + 0.5, 0.5, 0.5]]) + shift)
    parts.append(np.array([[0.0, 0.0, 0.0], [len(counts) + 1.0 + shift, 1.0 + shift, 1.0 + shift]]))     # pins min / max: voxel i = cube i at leaf 1
    pts = np.concatenate(parts)
    rng.shuffle(pts)
    return pts.astype(np.float32).astype(np.float64) if f32 else pts


def test_voxel_filter_populous_voxels_bit_exact(pcp, oracle):
    """Voxels far above a lane group's reach (voxel_filter.py:36-51 walks them point by point; np.mean = NumPy's pairwise
    recursion): every size class of the split -- the 1024-point hand-over to a block, the depths at which all nodes split,
    subtrees whose sizes differ by the recursion's rounding to multiples of 8 -- must reproduce np.mean bit for bit."""
    rng = np.random.default_rng(4242)
    counts = [1023, 1024, 1025, 1031, 1032, 1033, 1039, 1040, 2047, 2048, 2049, 2063, 2064, 2065, 3000, 4095, 4096, 4097, 4104, 4111, 4112,
              5000, 8191, 8192, 8193, 8200, 8264, 16390, 33000, 70001]
    pts = _populous(rng, counts)
    out = pcp.voxel_filter(pts, 1.0, "centroid")
    ref = oracle.voxel_filter(pts, 1.0, "centroid")[0]
    assert out.shape == ref.shape and len(ref) >= len(counts)
    assert np.array_equal(out, ref)
    # every listed cube is one voxel of that many points (+ the pinned corner in cube 0)
    h, _ = oracle.voxel_keys(pts, 1.0)
    sizes = np.unique(h, return_counts=True)[1]
    assert sorted(sizes.tolist())[-3:] == [16390, 33000, 70001]


def test_voxel_filter_2m_leaf_on_1m_points(pcp, oracle, syn):
    """The coarse levels of BASELINE configs[4]'s coarse-to-fine ICP: 2 m and 0.5 m leaves on a 1 M-point scan (voxels of tens of
    thousands of points next to the sensor)."""
    pts = syn.kitti_like_scan(1_000_000, seed=11).astype(np.float64)
    for leaf in (2.0, 0.5):
        out = pcp.voxel_filter(pts, leaf, "centroid")
        ref = oracle.voxel_filter(pts, leaf, "centroid")[0]
        assert out.shape == ref.shape and np.array_equal(out, ref), leaf


def test_voxel_down_sample_populous_voxels_running_sum(pcp):
    """Open3D's voxel_down_sample (Registration/main.py:35) adds a voxel's points in input order: binary64 inputs make every
    addition round, so any other order of additions shows in the last bits.  PARITY UNPINNED (Open3D absent): checked against
    oracle/oracle_global.py's restatement."""
    import importlib
    og = importlib.import_module("oracle.oracle_global")
    rng = np.random.default_rng(4343)
    counts = [1, 2, 7, 8, 9, 63, 64, 65, 66, 255, 256, 257, 258, 511, 512, 513, 1000, 10007, 40000]
    pts = _populous(rng, counts, shift=0.5) * 2.0 + 50.0       # cubes of 2 m = voxels at voxel_size 2
    pts = pts[:, [1, 0, 2]].copy()                    # cubes along y: the key order is not the x order
    out = pcp.voxel_down_sample(pts, 2.0)
    ref = og.voxel_down_sample(pts, 2.0)
    assert out.shape == ref.shape and np.array_equal(out, ref)
    assert len(ref) == len(counts) + 3              # one voxel per cube + the singleton + the two corners


def test_voxel_filter_huge_grid_keys_beyond_2_53(pcp, oracle):
    """A tiny leaf on a large extent: h = hx + hy*Dx + hz*Dx*Dy leaves the exactly representable integers (> 2^53, here even
    > 2^64).  The reference sorts the float64 h itself (voxel_filter.py:36); the device then sorts the BIT PATTERN of h
    (monotone for h >= 0) instead of its integer value -- groups, order and centroids stay those of the restatement."""
    rng = np.random.default_rng(77)
    base = rng.uniform(0.0, 200.0, (1500, 3))
    pts = np.concatenate([base, base[:400] + rng.uniform(0, 1e-6, (400, 3))])    # some voxels hold two points
    rng.shuffle(pts)
    leaf = 5e-5
    h, D = pcp.voxel_keys(pts, leaf)
    oh, oD = oracle.voxel_keys(pts, leaf)
    assert np.array_equal(D, oD) and np.array_equal(h, oh)
    assert oh.max() > 2.0 ** 64
    out = pcp.voxel_filter(pts, leaf, "centroid")
    ref = oracle.voxel_filter(pts, leaf, "centroid")[0]
    assert out.shape == ref.shape and np.array_equal(out, ref)
    assert len(ref) < len(pts) - 1          # (really some shared voxels)


KNN = [("uniform", 3000, 1), ("uniform", 3000, 8), ("uniform", 40, 64), ("clusters", 20000, 5), ("plane", 20000, 17), ("lattice", 4000, 9), ("line", 5000, 3)]


@pytest.mark.parametrize("case", range(len(KNN)))
def test_knn_radius_fuzz(pcp, oracle, case):
    kind, n, k = KNN[case]
    rng = np.random.default_rng(3000 + case)
    db = _cloud(rng, kind, n)
    q = np.concatenate([db[rng.integers(0, n, 20)] + rng.normal(0, 0.05, (20, 3)), _cloud(rng, kind, 20) * 1.3])
    root = pcp.kdtree_construction(db, 16)
    idx, dist = pcp.knn_search_batch(root, q, k)
    r = float(np.median(dist[:, min(k, n) - 1])) if n >= 1 else 1.0
    offs, ridx, rdist = pcp.radius_search_batch(root, q, r)
    ei, ed = oracle.knn_exact(db, q, k)        # (d2, index) order: tie slots included
    assert np.array_equal(dist, ed) and np.array_equal(idx, ei)
    eo, eri, erd = oracle.radius_exact(db, q, r)
    assert np.array_equal(offs, eo) and np.array_equal(ridx, eri) and np.array_equal(rdist, erd)   # in order, not as sets
    for j in range(len(q)):
        oi, od = oracle.knn_bruteforce(db, q[j], k)
        assert np.array_equal(dist[j], od)
        ri, rd = oracle.radius_bruteforce(db, q[j], r)
        s, e = offs[j], offs[j + 1]
        assert e - s == len(ri) and np.array_equal(rdist[s:e], rd) and np.array_equal(ridx[s:e], ri)
