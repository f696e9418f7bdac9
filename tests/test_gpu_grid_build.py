"""The grid's table build at the shapes where its shared steps (csrc/pcr_grid_build_dev.h) can go wrong: the single build
(csrc/pcr_grid.hip) against the brute-force index, the fused batch's build (csrc/pcr_batch.hip) against the per-pair path.

Already pinned elsewhere and not repeated: a one-point target searched from far outside, 50 duplicates among 500 targets and a
collinear cloud (test_nn1_edge_cases; the one-point target is kept in the size sweep below for the row compare with 257
queries), coordinates of 1e6 m and sizes that are no multiple of the query tile (test_nn1_far_from_origin_and_odd_sizes), a
cell of more than 65 535 points in the SINGLE build (test_nn1_cell_with_more_than_65535_points)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_QUERIES = 257


def _queries(rng, lo, hi):
    """257 queries over the target's box [lo, hi], a quarter of them outside it (up to three box sizes away)"""
    ext = np.maximum(hi - lo, 1e-3)
    q = rng.uniform(lo, lo + ext, (N_QUERIES, 3))
    out = rng.choice(N_QUERIES, N_QUERIES // 4, replace=False)
    q[out] += rng.choice([-1.0, 1.0], (len(out), 3)) * rng.uniform(1.0, 3.0, (len(out), 3)) * ext
    return q


def _single_build_equals_brute(pcp, tgt, q, cell=0.0):
    bi, bd2 = pcp.TargetIndex(tgt, kind="brute").nn1(q)     # exact, lowest row on ties
    gi, gd2 = pcp.TargetIndex(tgt, kind="grid", cell=cell).nn1(q)
    assert (bi >= 0).all()
    assert np.array_equal(gi, bi)
    assert np.array_equal(gd2, bd2)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_single_build_sizes_around_a_block(pcp, n):
    """Predecessor and successor key in another block of 256 threads, the first and the last record, i + 1 == n."""
    rng = np.random.default_rng(100 + n)
    tgt = rng.uniform(-1.0, 1.0, (n, 3))
    _single_build_equals_brute(pcp, tgt, _queries(rng, tgt.min(0), tgt.max(0)))


def test_single_build_identical_points(pcp):
    """300 copies of one point: one cell on every level, the only run start at 0 and the only end at n."""
    rng = np.random.default_rng(7)
    tgt = np.tile(np.array([[0.3, -1.7, 2.9]]), (300, 1))
    q = _queries(rng, tgt[0] - 0.5, tgt[0] + 0.5)
    _single_build_equals_brute(pcp, tgt, q)
    gi, _ = pcp.TargetIndex(tgt, kind="grid").nn1(q)
    assert (gi == 0).all()


@pytest.mark.parametrize("cells_per_unit,key_bits", [(4096, 39), (256, 27)])
def test_single_build_both_key_widths(pcp, cells_per_unit, key_bits):
    """4 097 uniform points in the unit cube: with cell = 1/4096 the cloud varies 39 Morton bits (the 64-bit key instantiation
    of the build kernels), with 1/256 it varies 27 (the 32-bit one)."""
    rng = np.random.default_rng(11)
    tgt = rng.uniform(0.0, 1.0, (4097, 3))
    ext = (tgt.max(0) - tgt.min(0)).max()
    bits = 3 * int(np.floor(np.log2(np.floor(ext * cells_per_unit) + 2.0)) + 1)     # pcr_morton_end_bit
    assert bits == key_bits and (bits > 32) == (key_bits > 32)
    _single_build_equals_brute(pcp, tgt, _queries(rng, tgt.min(0), tgt.max(0)), cell=1.0 / cells_per_unit)


def test_batch_build_equals_per_pair_path(pcp, monkeypatch, capfd):
    """One fused call over targets of 1, 2, 255, 256 and 257 points (a target's first record follows the previous cloud's slot
    padding: the li == 0 guard keeps the neighbour's key out), 300 identical points, and 70 000 points inside a 1 mm cube plus
    the corners of a 100 m cube (automatic cell ~0.2 m: one level-0 cell of more than 65 535 points, the block-overflow flag as
    the BATCH builds it).  Sources of 40-64 points.  Every result field and both matrices bit for bit the per-pair path's; a
    tiny target may end in the soft PCR_E_TOO_FEW_ASSOC on both paths, which is compared like any other result.
    The fused stages must TAKE all seven pairs (one they hand back is redone per pair, and the comparison would pass without the
    batch's build): the call's own timing line (PCR_BATCH_TIMING) reports the time spent on the per-pair path.  With no pair
    handed back that is the empty loops over three sub-batches, about 1 us; one pair costs two uploads, an index build with its
    synchronisation and an ICP with its read-back, 3 ms each in the reference call below and never under 0.2 ms: bound 50 us."""
    batch = __import__("importlib").import_module("point-cloud-process_amd.batch")
    rng = np.random.default_rng(23)

    def source(around, spread):
        return (around + rng.normal(0.0, spread, (int(rng.integers(40, 65)), 3))).astype(np.float32)

    pairs = []
    for n in (1, 2, 255, 256, 257):
        tgt = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        pairs.append((source(tgt[rng.integers(0, n, 1)], 0.3), tgt, None))
    same = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (300, 1))
    pairs.append((source(same[:1], 0.3), same, None))
    n_dense = 70000
    cell = 0.55 * np.sqrt(100.0 * 100.0 / (n_dense + 8))                   # pcr_grid_plan on a 100 m cube
    base = -50.0 + (np.floor(50.0 / cell) + 0.5) * cell                    # the middle of a level-0 cell, on every axis
    corners = np.array([[x, y, z] for x in (-50.0, 50.0) for y in (-50.0, 50.0) for z in (-50.0, 50.0)])
    dense = np.concatenate([base + rng.uniform(-5e-4, 5e-4, (n_dense, 3)), corners]).astype(np.float32)
    assert cell > 0.2 and (np.floor((dense[:n_dense].astype(np.float64) + 50.0) / cell) == np.floor(50.0 / cell)).all()
    pairs.append((source(np.full((1, 3), base), 0.05), dense, None))

    kw = dict(mode="total", max_iter=3, r_thres=1e-9, t_thres=1e-9)
    keys = ("iters", "status", "n_assoc", "cost", "mean_d2")
    monkeypatch.setenv("PCR_BATCH_SUB", "3")
    monkeypatch.setenv("PCR_BATCH_PER_PAIR", "1")
    ref = batch.native_register_share(pairs, device=0, streams=1, **kw)
    monkeypatch.setenv("PCR_BATCH_PER_PAIR", "0")
    monkeypatch.setenv("PCR_BATCH_TIMING", "1")
    capfd.readouterr()
    got = batch.native_register_share(pairs, device=0, streams=2, **kw)
    line = re.search(r"pcr_icp_batch: 7 pairs, 3 sub-batches of <= 3, .* per-pair path (\d+) us in total", capfd.readouterr().err)
    assert line is not None and int(line.group(1)) < 50, line and line.group(0)
    assert any(r["status"] == 0 and r["n_assoc"] >= 40 for r in ref)       # the pairs do register
    for i, (a, b) in enumerate(zip(ref, got)):
        assert all(a[k] == b[k] for k in keys), (i, {k: (a[k], b[k]) for k in keys})
        assert np.array_equal(a["T"], b["T"]) and np.array_equal(a["T_total"], b["T_total"]), i
