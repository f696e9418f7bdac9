"""Host-only sanity of the CPU restatement of the global-initialisation stage (oracle/oracle_global.py).
This stage of the reference is Open3D (absent, randomised): PARITY UNPINNED; the checks are the invariants the
published algorithm guarantees."""
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def og():
    return importlib.import_module("oracle.oracle_global")


def test_fpfh_block_sums_and_rigid_invariance(og, syn):
    pts = og.voxel_down_sample(syn.kitti_like_scan(20000, seed=3).astype(np.float64), 2.0)[:600]
    nb = og.hybrid_neighbours(pts, 10.0, 100)
    nrm, _ = og.normals_hybrid(pts, 4.0, 30)
    f = og.fpfh(pts, nrm, 10.0, 100, nbrs=nb)
    has = np.array([len(i) > 1 for i, _ in nb])
    blocks = f.reshape(len(pts), 3, 11).sum(axis=2)
    assert np.allclose(blocks[has], 200.0, atol=1e-9)      # 100 (own SPFH) + 100 (renormalised neighbours) per block
    assert (f >= 0).all()
    # rigid motion of points, normals and viewpoint leaves the descriptor unchanged (up to rare bin-edge flips)
    T = syn.rigid_transform([0.3, -0.2, 1.0], 0.9, [5.0, -3.0, 1.0])
    q = pts @ T[:3, :3].T + T[:3, 3]
    f2 = og.fpfh(q, nrm @ T[:3, :3].T, 10.0, 100)
    assert (np.abs(f - f2) > 1e-6).mean() < 0.01


def test_ransac_recovers_transform_with_outliers(og, syn):
    rng = np.random.default_rng(5)
    src = rng.uniform(-30, 30, (300, 3))
    T = syn.rigid_transform([0.1, 0.2, 1.0], 0.7, [4.0, -2.0, 0.5])
    tgt = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.02, src.shape)
    corr = np.stack([np.arange(300), np.arange(300)], axis=1)
    bad = rng.choice(300, 180, replace=False)
    corr[bad, 1] = rng.integers(0, 300, 180)                # 60 % wrong matches
    res = og.ransac(src, tgt, corr, max_iteration=4000, max_distance=0.5, seed=11)
    assert res["best_iteration"] >= 0 and res["corr_fitness"] > 0.35
    assert np.abs(res["T"] - T).max() < 0.05
    assert res["iterations"] < 4000                          # the confidence criterion stopped the loop early
    # deterministic in the seed
    assert og.ransac(src, tgt, corr, max_iteration=4000, max_distance=0.5, seed=11)["best_iteration"] == res["best_iteration"]


def test_voxel_down_sample_properties(og):
    rng = np.random.default_rng(2)
    p = rng.uniform(-10, 10, (5000, 3))
    out = og.voxel_down_sample(p, 2.0)
    mn = p.min(axis=0) - 1.0
    cells = np.floor((out - mn) / 2.0)
    assert len(np.unique(cells, axis=0)) == len(out)         # one centroid per occupied voxel, inside its voxel
    assert len(out) == len(np.unique(np.floor((p - mn) / 2.0), axis=0))
    assert np.allclose(out.mean(axis=0), p.mean(axis=0), atol=0.2)


def test_vectorised_pair_features_are_the_scalar_ones(og):
    """The FPFH restatement computes its pair features for all pairs at once (_pair_features_many); pair_features is the same
    definition pair by pair.  They must agree bit for bit, degenerate pairs (coincident points, a normal along the line) included."""
    rng = np.random.default_rng(12)
    p1, p2 = rng.uniform(-5, 5, (400, 3)), rng.uniform(-5, 5, (400, 3))
    n1, n2 = rng.normal(size=(400, 3)), rng.normal(size=(400, 3))
    n1, n2 = n1 / np.linalg.norm(n1, axis=1)[:, None], n2 / np.linalg.norm(n2, axis=1)[:, None]
    p2[:5] = p1[:5]                                            # zero length
    p1[5:10], p2[5:10], n1[5:10], n2[5:10] = 0.0, [0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0]   # d parallel to u: no frame
    p2[10:20] = np.round(p1[10:20]) + [1, 0, 0]                # lattice-like pairs
    p1[10:20] = np.round(p1[10:20])
    many = og._pair_features_many(p1, n1, p2, n2)
    one = np.array([og.pair_features(p1[i], n1[i], p2[i], n2[i]) for i in range(400)])
    assert np.array_equal(many, one)
    assert not many[:10].any()
