"""GPU: every k-NN and radius search path of the grid index against the exact oracle (oracle_np.knn_exact / radius_exact).

pcr_knn picks its pipeline from (q, k) (pcr_knn.hip, pcr_knn): q <= 16 and k <= 16 one launch of the wave-per-query box
kernel (template K = 8 or 16) with the descent behind it; q >= 256 and k <= 16 the batched pipeline (lane-per-query block
scan -> wave-per-query boxes -> block scan at every level -> descent); everything else the descent alone.  The radius
search takes pcr_radius_small for <= 8 queries (8192 neighbours per query at most, the two-pass pcr_radius above that) and
the two-pass search with device sorts otherwise.  For every query and every slot:
  * distances are bit-equal to the oracle's and indices equal, tie slots included (ascending (d2, index) for k-NN,
    ascending (sqrt(d2), index) for radius);
  * the indices of one query are distinct;
  * every reported distance is sqrt(dist2_direct(query, db[idx])).
Every case is seeded."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLAMP = 1.0e8          # a query this far from the cloud lies outside the 2^20 cells of any grid below: clamped coordinates


# ------------------------------------------------------------------------------------------------ checks
def _rows(bad):
    return np.flatnonzero(bad)[:8].tolist()


def check_knn(oracle, db, q, k, idx, dist, ref=None, tag=""):
    oi, od = ref if ref is not None else oracle.knn_exact(db, q, k)
    oi, od = oi[: len(q), :k], od[: len(q), :k]
    assert idx.shape == dist.shape == (len(q), k), tag
    assert np.array_equal(dist, od), (tag, "distances differ in queries", _rows((dist != od).any(axis=1)))
    assert np.array_equal(idx, oi), (tag, "indices differ in queries", _rows((idx != oi).any(axis=1)))
    filled = od < 1e10
    s = np.sort(np.where(filled, idx, -1 - np.arange(k)), axis=1)
    assert (np.diff(s, axis=1) != 0).all(), (tag, "repeated index")
    rec = np.sqrt(oracle.dist2_direct(q[:, None, :], db[np.where(filled, idx, 0)]))
    assert np.array_equal(dist[filled], rec[filled]), tag
    assert (idx[~filled] == 0).all() and (dist[~filled] == 1e10).all(), tag


def check_radius(oracle, db, q, r, offs, idx, dist, tag=""):
    eo, ei, ed = oracle.radius_exact(db, q, r)
    assert np.array_equal(offs, eo), (tag, "counts differ in queries", _rows(np.diff(offs) != np.diff(eo)))
    assert np.array_equal(idx, ei) and np.array_equal(dist, ed), tag    # in order, not as sets
    for j in range(len(q)):
        seg = idx[offs[j]:offs[j + 1]]
        assert len(np.unique(seg)) == len(seg), (tag, j)
    qq = np.repeat(q, np.diff(offs), axis=0)
    assert np.array_equal(dist, np.sqrt(oracle.dist2_direct(qq, db[idx]))), tag
    assert not (dist > r).any(), tag


# ------------------------------------------------------------------------------------------------ clouds
def _lattice_cloud(rng, side=40, n=16000, step=0.25, dups=300):
    """Distinct sites of a side^3 lattice (spacing `step`) plus exact duplicates; shuffled, so duplicates carry lower and
    higher indices.  Used with cell = step: every point lies on cell faces, ties run through the k-th slot."""
    sites = rng.choice(side ** 3, n, replace=False)
    g = np.stack([sites % side, (sites // side) % side, sites // (side * side)], axis=1).astype(np.float64) * step
    g = np.concatenate([g, g[rng.integers(0, n, dups)]])
    return g[rng.permutation(len(g))]


def _dup_clusters(rng):
    """Four dense clusters of 600 points each: 60 distinct points within 2 mm, every one repeated ten times (exact
    duplicates) -- > 384 points (KT_PTS) in one 5-cm cell --, over a sparse uniform background."""
    parts = []
    for c in rng.uniform(-10, 10, (4, 3)):
        base = c + rng.normal(0, 0.002, (60, 3))
        parts.append(np.repeat(base, 10, axis=0))
    parts.append(rng.uniform(-12, 12, (3000, 3)))
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))]


def _queries(rng, db, n, spread):
    """n queries: db points moved by N(0, spread), exact db points (distance 0, duplicates), uniform ones in the grown
    bounding box, and every 97th one far out (clamped).  Positions 0-4 hold one of each kind plus a far but unclamped
    query, so that the prefixes of 5 and 16 queries meet every kind."""
    lo, hi = db.min(0), db.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    a = db[rng.integers(0, len(db), n)] + rng.normal(0, spread, (n, 3))
    b = db[rng.integers(0, len(db), n)]
    c = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (n, 3))
    pick = rng.integers(0, 3, n)[:, None]
    q = np.where(pick == 0, a, np.where(pick == 1, b, c))
    q[::97] = hi + CLAMP + rng.uniform(0, 1, (len(q[::97]), 3))
    if n >= 5:
        q[:5] = [a[0], b[1], hi + CLAMP, c[3], hi + 2.0 * ext.max()]
    return q


def _lattice_queries(rng, db, n, step=0.25):
    """Lattice sites (occupied or not) and sites moved by half a step along some axes: exact ties everywhere."""
    lo, hi = db.min(0), db.max(0)
    q = np.round(rng.uniform(lo, hi, (n, 3)) / step) * step + rng.integers(0, 2, (n, 3)) * (step / 2)
    q[: n // 4] = db[rng.integers(0, len(db), n // 4)]
    q[rng.permutation(n)[: n // 4]] += rng.integers(0, 2, (n // 4, 3)) * (step / 2)
    if n >= 5:
        q[2] = hi + CLAMP
        q[4] = hi + 2.0 * (hi - lo).max()
    return q


def _scan_case(syn, rng=None):
    """The dispatch-grid cloud: a 20 000-point KITTI-like scan (float32 coordinates) and 3000 mixed queries."""
    rng = rng or np.random.default_rng(5100)
    db = syn.kitti_like_scan(20000, seed=31).astype(np.float64)
    return db, _queries(rng, db, 3000, 0.3), 0.0


def _lattice_case():
    rng = np.random.default_rng(5200)
    db = _lattice_cloud(rng)
    return db, _lattice_queries(rng, db, 3000), 0.25


Q_SIZES = (1, 5, 16, 17, 255, 256, 257, 3000)
K_VALUES = (1, 2, 7, 8, 9, 15, 16, 17, 64)


@pytest.fixture(scope="module")
def dispatch_cases(pcp, oracle, syn):
    out = {}
    for name, (db, q, cell) in (("scan", _scan_case(syn)), ("lattice", _lattice_case())):
        index = pcp.TargetIndex(db, cell=cell)
        out[name] = (db, q, index, oracle.knn_exact(db, q, max(K_VALUES)))
    yield out
    for v in out.values():
        v[2].free()


# ------------------------------------------------------------------------------------------------ k-NN dispatch
@pytest.mark.parametrize("k", K_VALUES)
@pytest.mark.parametrize("cloud", ["scan", "lattice"])
def test_knn_dispatch_boundaries(pcp, oracle, dispatch_cases, cloud, k):
    """Every (q, k) row of pcr_knn's dispatch -- single launch K = 8 / 16, batched K = 8 / 16, descent alone for
    17 <= q <= 255 or k > 16 -- on both sides of every boundary.  (The first q queries of one list: the oracle for k = 64
    holds every smaller k and every prefix, (d2, index) being a total order.)"""
    db, q, index, ref = dispatch_cases[cloud]
    for nq in Q_SIZES:
        idx, dist = index.knn(q[:nq], k)
        check_knn(oracle, db, q[:nq], k, idx, dist, ref=ref, tag=(cloud, nq, k))


def test_knn_public_api_single_and_batch(pcp, oracle, syn):
    """The same contract through the reference-shaped API: kdtree / octree searches into KNNResultSet, the batched form."""
    db, q, _ = _scan_case(syn)
    root = pcp.kdtree_construction(db, 16)
    oroot = pcp.octree_construction(db, 4, 0.0001)
    for k in (1, 8, 9, 16, 17):
        ei, ed = oracle.knn_exact(db, q[:6], k)
        for j in range(6):
            for fn, r in ((pcp.kdtree_knn_search, root), (pcp.octree_knn_search, oroot)):
                rs = pcp.KNNResultSet(capacity=k)
                fn(r, db, rs, q[j])
                assert [x.index for x in rs.dist_index_list] == ei[j].tolist(), (k, j)
                assert [x.distance for x in rs.dist_index_list] == ed[j].tolist(), (k, j)
        for nq in (16, 300):
            idx, dist = pcp.knn_search_batch(root, q[:nq], k)
            check_knn(oracle, db, q[:nq], k, idx, dist, tag=(nq, k))


def test_knn_bench_shape_self_query_120k(pcp, oracle, syn):
    """The benchmark's own shape: a 120 000-point scan queried against itself (batched path), k = 8 and 16."""
    db = syn.kitti_like_scan(120_000, seed=0).astype(np.float64)
    root = pcp.kdtree_construction(db, 16)
    ref = oracle.knn_exact(db, db, 16)
    for k in (8, 16):
        idx, dist = pcp.knn_search_batch(root, db, k)
        check_knn(oracle, db, db, k, idx, dist, ref=ref, tag=k)


# ------------------------------------------------------------------------------------------------ clouds and edges
def _edge_case(name, syn):
    rng = np.random.default_rng(5300 + sum(map(ord, name)))
    if name == "uniform":
        db = rng.uniform(-5, 5, (20000, 3))
        return db, _queries(rng, db, 1000, 0.1), 0.0
    if name == "planar":
        db = rng.uniform(-20, 20, (20000, 3))
        db[:, 2] = 0.01 * rng.normal(size=len(db))
        return db, _queries(rng, db, 1000, 0.3), 0.0
    if name == "dup_clusters":
        db = _dup_clusters(rng)
        q = _queries(rng, db, 1000, 0.002)
        # around one cluster: on it, then 1, 3 and 8 cells (of 5 cm) away -- the boxes meet > 384 staged points
        near = db[rng.integers(0, len(db), 40)]
        near = np.concatenate([near, near + [0.05, 0, 0], near + [0, 0.15, 0], near + [0, 0, 0.4]])
        q[5:16] = near[rng.integers(0, len(near), 11)]
        q[300:460] = near
        return db, q, 0.05
    if name == "dup_clusters_auto":
        db = _dup_clusters(rng)
        return db, _queries(rng, db, 1000, 0.002), 0.0
    if name == "lattice_offset":
        db = _lattice_cloud(rng, side=30, n=9000) + np.array([1.0e6, -2.0e6, 3.0e6])
        return db, _lattice_queries(rng, db, 1000), 0.25
    if name == "float32":
        db = rng.uniform(-5, 5, (20000, 3)).astype(np.float32)
        q = _queries(rng, db.astype(np.float64), 1000, 0.1).astype(np.float32).astype(np.float64)
        return db, q, 0.0
    if name == "scan_offset_1e6":
        db = syn.kitti_like_scan(20000, seed=32).astype(np.float64) + np.array([1.0e6, -2.5e6, 40.0])
        return db, _queries(rng, db, 1000, 0.3), 0.05
    if name == "uniform_offset_5e6":
        db = rng.uniform(0, 10, (10000, 3)) + 5.0e6
        return db, _queries(rng, db, 1000, 0.05), 0.01
    if name == "tiny_cell":
        db = rng.uniform(-5, 5, (8000, 3))
        return db, _queries(rng, db, 1000, 0.05), 1e-9        # clamped up to emax / 262144 by the grid plan
    if name == "one_cell":
        db = syn.kitti_like_scan(20000, seed=33).astype(np.float64)
        return db, _queries(rng, db, 1000, 0.3), 1.0e4
    raise ValueError(name)


EDGES = ["uniform", "planar", "dup_clusters", "dup_clusters_auto", "lattice_offset", "float32", "scan_offset_1e6",
         "uniform_offset_5e6", "tiny_cell", "one_cell"]


@pytest.mark.parametrize("name", EDGES)
def test_knn_clouds_and_edges(pcp, oracle, syn, name):
    """Shapes and edges where the proofs of the box kernels are thinnest: exact duplicates in overfull cells, points on cell
    faces, float32 inputs (uploaded as float32), map-sized offsets with small cells, the smallest cell the grid allows,
    one cell for the whole cloud, clamped and far queries, queries equal to db points -- on every pipeline."""
    db, q, cell = _edge_case(name, syn)
    index = pcp.TargetIndex(db, cell=cell)
    db = np.asarray(db, dtype=np.float64)
    ref = oracle.knn_exact(db, q, 17)
    try:
        for nq in (1, 16, 100, 1000):
            for k in (1, 8, 9, 16, 17):
                idx, dist = index.knn(q[:nq], k)
                check_knn(oracle, db, q[:nq], k, idx, dist, ref=ref, tag=(name, nq, k))
    finally:
        index.free()


@pytest.mark.parametrize("n", [1, 5, 8, 9, 16])
def test_knn_fewer_points_than_k(pcp, oracle, n):
    """n < k and n = k on the single-launch, the batched and the descent path: unfilled slots hold (1e10, 0)."""
    rng = np.random.default_rng(5400 + n)
    db = rng.uniform(-1, 1, (n, 3))
    if n >= 5:
        db[n - 1] = db[0]                     # a duplicate
    q = np.concatenate([db[rng.integers(0, n, 150)], rng.uniform(-2, 2, (150, 3))])
    q[7] = CLAMP
    index = pcp.TargetIndex(db)
    try:
        for nq in (3, 16, 40, 300):
            for k in (1, 7, 8, 9, 16, 17):
                idx, dist = index.knn(q[:nq], k)
                check_knn(oracle, db, q[:nq], k, idx, dist, tag=(n, nq, k))
    finally:
        index.free()


# ------------------------------------------------------------------------------------------------ radius
def _radius_case(name, syn):
    rng = np.random.default_rng(5500 + sum(map(ord, name)))
    if name == "scan":
        db = syn.kitti_like_scan(20000, seed=34).astype(np.float64)
        q = _queries(rng, db, 2000, 0.3)
        return db, q, 0.0, (0.0, 0.35, 1.2)
    if name == "lattice":
        db = _lattice_cloud(rng, side=30, n=9000)
        # 0.25 and 0.5: whole steps; 1.25 = |(0.75, 1, 0)|: every radius an exact lattice distance (inclusive boundary)
        return db, _lattice_queries(rng, db, 2000), 0.25, (0.0, 0.25, 0.5, 1.25)
    if name == "dup_clusters":
        db = _dup_clusters(rng)
        return db, _queries(rng, db, 2000, 0.002), 0.05, (0.0, 0.004, 0.3)
    raise ValueError(name)


@pytest.mark.parametrize("name", ["scan", "lattice", "dup_clusters"])
def test_radius_paths(pcp, oracle, syn, name):
    """pcr_radius_small (1 and 8 queries) and the two-pass search (9 and 2000): exact order, r = 0, radii equal to lattice
    distances, empty segments between non-empty ones (far queries interleaved)."""
    db, q, cell, radii = _radius_case(name, syn)
    index = pcp.TargetIndex(db, cell=cell)
    try:
        for r in radii:
            for nq in (1, 8, 9, 2000):
                offs, idx, dist = index.radius(q[:nq], r)
                check_radius(oracle, db, q[:nq], r, offs, idx, dist, tag=(name, r, nq))
                if nq == 2000:
                    c = np.diff(offs)
                    assert (c == 0).any() and (c > 0).any()
        root = pcp.kdtree_construction(db, 16)
        offs, idx, dist = pcp.radius_search_batch(root, q[:300], radii[-1])
        check_radius(oracle, db, q[:300], radii[-1], offs, idx, dist, tag=(name, "batch"))
        for j in range(4):
            rs = pcp.RadiusNNResultSet(radius=radii[-1])
            pcp.kdtree_radius_search(root, db, rs, q[j])
            _, ei, ed = oracle.radius_exact(db, q[j:j + 1], radii[-1])
            assert [x.index for x in rs.dist_index_list] == ei.tolist() and [x.distance for x in rs.dist_index_list] == ed.tolist()
    finally:
        index.free()


def test_radius_small_cap_boundary(pcp, oracle):
    """8192 neighbours fit the single-launch block; 8193 must hand the call over to the two-pass search, complete and
    ordered -- alone and next to a query that fits."""
    rng = np.random.default_rng(5600)
    a = rng.normal(0, 0.1, (8192, 3))
    b = rng.normal(0, 0.1, (8193, 3)) + [10.0, 0, 0]
    a *= 0.45 / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 0.45)     # all within 0.45 of their centre
    b[:, :] = [10.0, 0, 0] + (b - [10.0, 0, 0]) * (0.45 / np.maximum(np.linalg.norm(b - [10.0, 0, 0], axis=1, keepdims=True), 0.45))
    db = np.concatenate([a, b, rng.uniform(-20, 30, (4000, 3)) + [0, 40.0, 0]])
    db = db[rng.permutation(len(db))]
    index = pcp.TargetIndex(db)
    ca, cb, far = [0.0, 0, 0], [10.0, 0, 0], [0.0, 100.0, 0]
    try:
        for qs, want in (([cb, far, ca, cb, far, far, ca, cb], None), ([ca], [8192]), ([ca, cb], [8192, 8193]), ([cb], [8193])):
            q = np.array(qs, dtype=np.float64)
            offs, idx, dist = index.radius(q, 0.5)
            check_radius(oracle, db, q, 0.5, offs, idx, dist, tag=len(qs))
            if want is not None:
                assert np.diff(offs).tolist() == want
    finally:
        index.free()


def test_radius_no_neighbours_and_huge_segment(pcp, oracle):
    """A call where no query has a neighbour (both paths), and one segment of more than 65 536 entries next to empty
    ones in the two-pass search's segmented sorts."""
    rng = np.random.default_rng(5700)
    blob = rng.uniform(-1, 1, (70000, 3))
    blob = blob[np.linalg.norm(blob, axis=1) < 0.99]
    db = np.concatenate([blob, rng.uniform(-1, 1, (75000, 3)) * 0.5, rng.uniform(-30, 30, (2000, 3))])
    db = db[rng.permutation(len(db))]
    index = pcp.TargetIndex(db)
    try:
        far = np.array([[500.0, 0, 0], [0, 500.0, 0], [0, 0, -500.0]])
        for nq in (1, 3):
            offs, idx, dist = index.radius(far[:nq], 1.0)
            assert offs.tolist() == [0] * (nq + 1) and len(idx) == 0
        far12 = np.tile(far, (4, 1)) + rng.uniform(0, 1, (12, 3))
        offs, idx, dist = index.radius(far12, 1.0)
        assert offs.tolist() == [0] * 13 and len(idx) == 0
        q = far12.copy()
        q[4] = [0.0, 0, 0]
        q[9] = [0.01, 0.02, -0.01]
        offs, idx, dist = index.radius(q, 1.0)
        assert np.diff(offs)[4] > 65536
        check_radius(oracle, db, q, 1.0, offs, idx, dist)
    finally:
        index.free()


# ------------------------------------------------------------------------------------------------ coverage proof
def _coverage_cases(pcp, syn):
    """What the child process below runs: the scan case of the dispatch grid on the batched path (q = 3000, k = 8 and 16),
    then the scan queried against itself (q = 20 000)."""
    db, q, cell = _scan_case(syn)
    index = pcp.TargetIndex(db, cell=cell)
    for qq in (q, db):
        for k in (8, 16):
            index.knn(qq, k)
    index.free()


_CHILD = """
import importlib, sys
sys.path.insert(0, {root!r})
t = importlib.import_module("tests.test_gpu_knn_radius_paths")
t._coverage_cases(importlib.import_module("point-cloud-process_amd"), importlib.import_module("point-cloud-process_amd.synthetic"))
"""


def test_batched_cases_reach_every_stage():
    """PCR_KNN_DEBUG=1 (read once per process: a fresh child) makes pcr_knn print how many queries each batched stage
    left.  The dispatch grid's batched scan cases must send queries past the first scan (to the wave-per-query boxes)
    and on to the descent, for both template sizes -- else the exact checks above would only ever see stage 1."""
    env = dict(os.environ, PCR_KNN_DEBUG="1")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    pat = re.compile(r"pcr_knn: (\d+) queries, k = (\d+): (\d+) left by the first scan, (\d+) by the wave-per-query boxes, (\d+) to the descent")
    seen = {}
    for m in pat.finditer(p.stderr):
        nq, k, first, boxes, descent = map(int, m.groups())
        seen[(nq, k)] = (first, boxes, descent)
    assert set(seen) == {(3000, 8), (3000, 16), (20000, 8), (20000, 16)}, p.stderr[-3000:]
    for k in (8, 16):
        first, boxes, descent = seen[(3000, k)]
        # the mixed queries: off-surface ones leave the first scan, the boxes prove some of them, the clamped ones reach the descent
        assert first > 0 and boxes < first and descent > 0, (k, seen)
        # ... while the first scan itself proves most of a scan queried against itself (its 3x3x3 cover at work)
        first, boxes, descent = seen[(20000, k)]
        assert first < 20000 * SELF_LEFT_MAX[k], (k, seen)


SELF_LEFT_MAX = {8: 0.35, 16: 0.15}    # fraction of the self-queries the first scan may leave (k = 8: 26 %, k = 16: 7 % measured)
