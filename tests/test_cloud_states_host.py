"""The scenes of tests/test_gpu_cloud_states.py proven on the CPU (tests/cloud_state_checks.py): each of them CAN tell a consumer that
mishandles a cloud's layout or its remembered box from one that does not.  Conditions on the restatements, no device."""
import numpy as np

from oracle import oracle_global as og
from oracle import oracle_np as oracle
from tests import cloud_state_checks as K


def test_base_cloud_shape():
    P = K.base_cloud()
    assert P.shape == (K.N_BASE, 3) and P.dtype == np.float32 and np.isfinite(P).all()
    assert len(np.unique(P, axis=0)) == K.N_BASE                       # no duplicate rows: a caller row is told by its coordinates
    assert np.array_equal(P, K.base_cloud())                           # seeded
    for n in K.TINY_SIZES:
        assert K.tiny_cloud(n).shape == (n, 3) and K.tiny_cloud(n).dtype == np.float32
    # the blob: one voxel above both hand-over sizes in both grids, and emitted (voxel_filter.py never emits the largest key)
    h, _ = oracle.voxel_keys(P, K.LEAF)
    keys, counts = np.unique(h, return_counts=True)
    assert counts.max() >= K.N_BLOB > K.VOX_BIG_PAIRWISE and keys[counts.argmax()] < keys.max()
    assert max(map(len, K.down_sample_groups(P))) >= K.N_BLOB > K.VOX_BIG_RUNNING
    assert len(K.target_cloud()) <= 20000 and 3000 <= len(K.region_b()) <= 20000


def test_move_is_rigid_and_leaves_the_box():
    R = K.T_MOVE[:3, :3]
    assert np.array_equal(R @ R.T, np.eye(3)) and np.linalg.det(R) == 1.0 and np.array_equal(R @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    fig = K.check_moved_box(K.base_cloud())
    print(fig)
    assert fig["outside"] >= 0.1 and fig["D"] != fig["D_moved"]
    # the restated transform is NumPy's for this matrix (entries 0 and +-1: every product exact)
    P = K.base_cloud().astype(np.float64)
    assert np.array_equal(K.apply(K.T_MOVE, P), P @ R.T + K.T_MOVE[:3, 3])


def test_voxel_sums_are_order_sensitive():
    fig = K.check_order_sensitive(K.base_cloud())
    print(fig)
    assert fig["filter_changed"] >= 1 and fig["down_changed"] >= 1 and fig["several_members"] >= 0.5
    # the restated groups are the oracles' (rows of the emitted voxels, in key order)
    P = K.base_cloud().astype(np.float64)
    assert len(K.filter_groups(P)) == len(oracle.voxel_filter(P, K.LEAF)[0])
    assert len(K.down_sample_groups(P)) == len(og.voxel_down_sample(P, K.VOXEL_SIZE))


def test_morton_rank_is_a_permutation_unlike_the_input_order():
    P = K.base_cloud()
    rank = K.morton_rank(P)
    assert np.array_equal(np.sort(rank), np.arange(len(P)))
    assert (rank != np.arange(len(P))).mean() > 0.99
    # neighbours in rank are neighbours in space: the median step along the curve is far below the median step along the input
    by_rank = P[np.argsort(rank)].astype(np.float64)
    step = lambda a: np.median(np.linalg.norm(np.diff(a, axis=0), axis=1))   # noqa: E731
    assert step(by_rank) < 0.1 * step(P.astype(np.float64))


def test_icp_pair_margins():
    """The compat loop's decisions on the 3 000-point pair, from identity and from an offset start (two passes): a factor 2 from 0.5."""
    src, tgt = K.icp_pair()
    assert src.shape == tgt.shape == (3000, 3)
    full, dec = K.check_icp_margins(src, tgt, np.eye(4))
    print(full["iters"], dec)
    full2, dec2 = K.check_icp_margins(src, tgt, K.T_START)
    print(full2["iters"], dec2)
    assert full2["iters"] >= 2
    assert max(dec[-1]) <= 0.25 and max(dec2[-1]) <= 0.25 and max(dec2[0]) >= 1.0


def test_base_cloud_icp_margins():
    """The loops of the matrix: the base cloud (and the moved one, started from the inverse move) against the 20 000-point target."""
    P = K.base_cloud().astype(np.float64)
    full, dec = K.check_icp_margins(P, K.target_cloud(), K.T_START)
    assert full["iters"] >= 2
    moved = K.apply(K.T_MOVE, P)
    full_m, dec_m = K.check_icp_margins(moved, K.target_cloud(), K.T_START @ np.linalg.inv(K.T_MOVE))
    print(dec, dec_m)
    assert full_m["iters"] == full["iters"]
