"""The restated lay-out keys of a query cloud (tests/curve_keys.py, the NumPy twin of csrc/pcr_curve.h) and the tile-box model built on
them (scripts/tile_box_model.py).  No GPU needed: tests/test_gpu_query_curve.py pins the device order to this restatement."""
import itertools

import numpy as np
from scipy.spatial import cKDTree

from tests import curve_keys as ck


def _cube(n):
    return np.array(list(itertools.product(range(n), repeat=3)), dtype=np.int64)


def _plane(n, minor):
    return np.array(list(itertools.product(range(n), range(n), range(minor))), dtype=np.int64)


def test_keys_are_bijections():
    """16 x 16 x 16 cells: 3-D Hilbert and Morton keys are permutations of [0, 4096); a 32 x 32 plane with 8 minor cells: the 2-D key
    with a minor axis is a permutation of [0, 8192), for every assignment of the axes."""
    c = _cube(16)
    assert sorted(ck.hilbert3_of_cells(c, 4).tolist()) == list(range(4096))
    assert sorted(ck.morton_of_cells(c, 4).tolist()) == list(range(4096))
    p = _plane(32, 8)
    for ax in itertools.permutations(range(3)):
        q = np.empty_like(p)
        q[:, list(ax)] = p                       # plane axes -> ax[0], ax[1]; minor -> ax[2]
        assert sorted(ck.hilbert2_minor_of_cells(q, 5, ax, 3).tolist()) == list(range(8192)), ax


def test_consecutive_keys_are_face_neighbours():
    """Cells of consecutive 3-D keys differ by one step along one axis; so do the plane cells of consecutive 2-D keys (the minor
    coordinate runs through its cells inside one plane cell).  The Z curve does not have the property: that is the point."""
    c = _cube(16)
    by_key = c[np.argsort(ck.hilbert3_of_cells(c, 4))]
    assert (np.abs(np.diff(by_key, axis=0)).sum(1) == 1).all()
    by_morton = c[np.argsort(ck.morton_of_cells(c, 4))]
    assert np.abs(np.diff(by_morton, axis=0)).sum(1).max() > 1
    p = _plane(32, 8)
    k = ck.hilbert2_minor_of_cells(p, 5, (0, 1, 2), 3)
    by_key = p[np.argsort(k)]
    assert np.array_equal(by_key[:, 2], np.tile(np.arange(8), 1024))         # minor key: the low three bits
    cells = by_key[::8, :2]
    assert (by_key[:, :2].reshape(-1, 8, 2) == cells[:, None, :]).all()
    assert (np.abs(np.diff(cells, axis=0)).sum(1) == 1).all()
    # single-level curves (nb = 1: a cloud inside one or two cells) are still bijections with the property
    c2 = _cube(2)
    assert (np.abs(np.diff(c2[np.argsort(ck.hilbert3_of_cells(c2, 1))], axis=0)).sum(1) == 1).all()


def test_rule():
    """2-D with a minor axis for a 100 x 120 x 3 box (axes by falling extent: y, x; minor z), 3-D for a cube; the boundary (shortest =
    a quarter of the middle) is 2-D; equal extents go to the lower axis index; a degenerate box (one cell) is 2-D with minor z."""
    z = np.zeros(3)
    cv = ck.pick(z, [100.0, 120.0, 3.0], 1.0)
    assert cv["mode"] == "hilbert2_minor" and cv["ax"] == (1, 0, 2) and cv["nb"] == 7 and cv["nb_minor"] == 3
    assert ck.pick(z, [4.0, 4.0, 4.0], 8.0) == dict(mode="hilbert3", nb=6, ax=(0, 1, 2), nb_minor=0)
    assert ck.pick(z, [8.0, 3.0, 2.0], 1.0)["mode"] == "hilbert3"
    assert ck.pick(z, [8.0, 2.0, 8.0], 1.0) == dict(mode="hilbert2_minor", nb=4, ax=(0, 2, 1), nb_minor=3)   # 2 <= 8 / 4; tie x, z -> x
    assert ck.pick(z, [8.0, 2.0 + 1e-9, 8.0], 1.0)["mode"] == "hilbert3"
    assert ck.pick(z, z, 1.0) == dict(mode="hilbert2_minor", nb=2, ax=(0, 1, 2), nb_minor=2)
    assert ck.end_bit(z, [100.0, 120.0, 3.0], 1.0) == 21 and ck.end_bit(z, [1.0, 1.0, 1.0], 4096.0) == 39


def test_layout_order_is_stable_and_complete():
    rng = np.random.default_rng(0)
    p = np.repeat(rng.uniform(0.0, 9.0, (50, 3)), 3, axis=0)          # every point three times
    for curve in ("rule", "morton", "hilbert3", "hilbert2_minor"):
        o = ck.layout_order(p, 1.0, curve)
        assert sorted(o.tolist()) == list(range(150))
        k = ck.layout_keys(p, 1.0, curve)[o]
        assert (np.diff(k.astype(np.int64)) >= 0).all()
        same = np.diff(k.astype(np.int64)) == 0
        assert (np.diff(o)[same] > 0).all()                            # equal keys keep their relative order
    assert np.array_equal(ck.layout_order(p[:1], 1.0), [0])


def test_model_stages_less_under_the_rules_curve(syn):
    """perturbed_pair(20000, seed=0) at the registered pose, the index's automatic cell: the mean number of target points in a
    tile's pass box is lower under the rule's curve than under Morton (a condition on the reference model; the margin is whatever
    scripts/tile_box_model.py prints)."""
    src, tgt, T = syn.perturbed_pair(20000, seed=0)
    src, tgt = src.astype(np.float64), tgt.astype(np.float64)
    tree = cKDTree(tgt)
    cell = ck.auto_cell(tgt)
    q = ck.registered(src, T, tree)
    mean = {c: ck.staged_per_tile(q, ck.layout_order(src, cell, c), tgt, tree).mean() for c in ("morton", "rule")}
    print("mean staged per tile:", mean)
    assert mean["rule"] < mean["morton"]
