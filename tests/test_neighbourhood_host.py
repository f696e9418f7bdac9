"""Pins tests/neighbourhood_checks.py on the CPU: the ball rule against scipy, the restated suppression against the pinned ISS
oracle, and that every designed input lands in the class of inputs it was designed for.  Conditions on the inputs and on the
references only; no library code runs here."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import neighbourhood_checks as nc


@pytest.mark.parametrize("r", [0.5, 0.08, 0.3, 0.6])
def test_ball_in_is_query_ball_point(r):
    """2 100 pairs at distance r up to a few ulps: query_ball_point(q, r) over the one-point tree {p} finds p exactly when
    (dx*dx + dy*dy) + dz*dz <= fl(r*r).  The kd-tree API's rule on sqrt(d2) takes more at r = 0.5 and r = 0.08 (a band of one
    ulp of d2 above fl(r*r)) and the same at r = 0.3 and r = 0.6."""
    q, p = nc.boundary_cases(r, 2100, seed=int(r * 100))
    got = np.array([len(cKDTree(p[i : i + 1]).query_ball_point(q[i], r)) for i in range(len(q))], dtype=bool)
    mine = nc.ball_in(q, p, r)
    assert np.array_equal(got, mine)
    assert 0.1 < mine.mean() < 0.9                                   # the cases straddle the boundary
    norm_only = nc.norm_rule_in(q, p, r) & ~mine          # (about 15 % of the cases at r = 0.5 and 5 % at r = 0.08: 30 is far below both)
    assert not (mine & ~nc.norm_rule_in(q, p, r)).any()
    assert (norm_only.sum() >= 30) == (r in (0.5, 0.08)) and (norm_only.sum() == 0) == (r in (0.3, 0.6)), norm_only.sum()
    # and as one tree over all p (the way ISS and DBSCAN use it): the pairs are found among their neighbours
    lists = cKDTree(p).query_ball_point(q, r)
    assert np.array_equal(np.array([i in l for i, l in enumerate(lists)]), mine)


def test_band_pairs_hit_their_classes():
    for r in (0.5, 0.08):
        bp = nc.band_pairs(r, 400, seed=3)
        (bq, bpp), (eq, ep) = bp["band"], bp["edge"]
        assert len(bq) >= 64 and len(eq) >= 16, (r, len(bq), len(eq))
        assert not nc.ball_in(bq, bpp, r).any() and nc.norm_rule_in(bq, bpp, r).all()
        assert nc.ball_in(eq, ep, r).all() and nc.norm_rule_in(eq, ep, r).all()
        d2 = nc.oracle.dist2_direct(eq, ep)
        assert ((d2 == np.float64(r) * np.float64(r)) | (d2 == np.nextafter(np.float64(r) * np.float64(r), 0.0))).all()
        # isolated: scipy counts 1 around every band point and 2 around every edge-in point
        pts, (brow, erow) = nc.pairs_cloud(bp["band"], bp["edge"])
        counts = nc.ball_counts(pts, r)
        assert (counts[brow] == 1).all() and (counts[brow + 1] == 1).all()
        assert (counts[erow] == 2).all() and (counts[erow + 1] == 2).all()
        assert (pts.max(axis=0) - pts.min(axis=0)).max() / r < 262144 * 0.9      # a grid of cell r is not coarsened
    assert len(nc.band_pairs(0.3, 400, seed=3)["band"][0]) == 0
    assert len(nc.band_pairs(0.3, 400, seed=3)["edge"][0]) >= 16


def test_iss_nms_is_the_oracles_suppression(oracle, syn, golden):
    g = golden("iss.npz")
    cases = []
    for tag in ("object", "sparse", "six"):
        radius, l21, l32, nmr, cap = g[f"{tag}_params"]
        cases.append((g[f"{tag}_points"][:, :3], float(radius), float(l21), float(l32), float(nmr), int(cap)))
    pts = syn.object_cloud(3000, seed=2).astype(np.float64)
    cases += [(pts, 0.08, 0.5, 0.5, 0.08, 20), (pts, 0.08, 0.95, 0.95, 0.005, 1500), (pts, 0.08, 0.95, 0.95, 0.3, 1023), (pts, 0.08, 0.5, 0.5, 0.08, 0)]
    for p, radius, l21, l32, nmr, cap in cases:
        okp, olam, ocounts = oracle.iss_oracle(p, radius=radius, lambda21=l21, lambda32=l32, non_max_radius=nmr, iss_count=cap)
        assert nc.iss_nms(p, olam, l21, l32, nmr, cap) == okp
        assert np.array_equal(nc.ball_counts(p, radius), ocounts)
    assert len(okp) == 1                                            # iss_count 0: exactly one keypoint


def test_designed_clouds_reach_every_redo_route():
    """pcr_normals hands the rows its 27-cell scan cannot prove to pcr_knn, which takes one of three routes by their number (<=
    16, 17..255, >= 256).  core_and_outliers(m): measured redo rows (k = 5 / 9 / 16): m = 6: 6 / 6 / 6, m = 60: 59 / 59 / 58,
    m = 300: 298 / 294 / 288 with the builder's seed.  The lattice (spacing 0.25, cell at most 1.8 * sqrt(16/5 * 1.75^2 / 512) =
    0.249) sends every row there; the line (cell = extent / 64) none at k = 2, a handful at k = 5, nearly all at k = 16."""
    seen = {}
    for m, (lo, hi) in nc.REDO_CLASSES.items():
        pts = nc.core_and_outliers(m)
        assert len(pts) == 1500 + m
        for k in (5, 9, 16):
            r = len(nc.normals_redo_rows(pts, k))
            seen[m, k] = r
            assert lo <= r <= hi, (m, k, r)
    assert seen == {(6, 5): 6, (6, 9): 6, (6, 16): 6, (60, 5): 59, (60, 9): 59, (60, 16): 58, (300, 5): 298, (300, 9): 294, (300, 16): 288}
    lat = nc.lattice(8, 8, 8, 0.25)
    for k in (2, 7, 16):
        assert len(nc.normals_redo_rows(lat, k)) == 512
    line = nc.line_cloud(300)
    assert nc.normals_cell(line, 5) == (line[:, 0].max() - line[:, 0].min()) / 64.0
    assert [len(nc.normals_redo_rows(line, k)) for k in (2, 5, 16)] == [0, 4, 296]
    assert nc.normals_cell(np.zeros((40, 3)), 5) == 1.0
    plane = nc.core_and_outliers(0)
    plane[:, 2] = 0.25
    assert nc.normals_cell(plane, 5) == 1.8 * np.sqrt(np.prod(np.sort(plane.max(axis=0) - plane.min(axis=0))[1:]) / len(plane))


def test_normals_reference_orders_ties_by_row():
    lat = nc.lattice(8, 8, 8, 0.25)
    nbr, evs, nrm, covs = nc.normals_reference(lat, 7)
    # an interior point: itself, then its six face neighbours by ascending row (x fastest)
    i = 3 * 64 + 3 * 8 + 3
    assert nbr[i].tolist() == [i, i - 64, i - 8, i - 1, i + 1, i + 8, i + 64]
    dup = nc.with_duplicates(nc.core_and_outliers(0)[:1000], 0.3, seed=5)
    assert len(np.unique(dup, axis=0)) <= 700 + 1
    nbr, *_ = nc.normals_reference(dup, 5)
    d2 = nc.oracle.dist2_direct(dup[:, None, :], dup[nbr])
    assert (np.diff(d2, axis=1) >= 0).all()
    tie = np.diff(d2, axis=1) == 0
    assert tie.sum() > 300 and (np.diff(nbr, axis=1)[tie] > 0).all()
    # n <= k: the n points, then -1; one point: zero covariance
    nbr, evs, nrm, covs = nc.normals_reference(lat[:3], 5)
    assert nbr.tolist() == [[0, 1, 2, -1, -1], [1, 0, 2, -1, -1], [2, 1, 0, -1, -1]]
    nbr, evs, nrm, covs = nc.normals_reference(lat[:1], 5)
    assert nbr.tolist() == [[0, -1, -1, -1, -1]] and not covs.any() and not evs.any()


def test_dbscan_hand_cases(oracle):
    """Seven points on a line, spacing 1, radius 1, Min_Pts 3.  Neighbour counts (self included): 2 3 3 3 3 3 2.
      seeds come from the END: row 6 is popped first, has 2 < 3 neighbours: noise, and it has left `unvisited` for good;
      row 5 is popped: 3 >= 3 (the seed test is >=) opens cluster 0, stack = [4, 5, 6]: 6 is visited (a noise seed is never
      relabelled), 5 is visited, 4 gets label 0 but 3 > 3 fails (expansion is strict): cluster 0 = {5, 4};
      row 3: 3 >= 3 opens cluster 1, stack [2, 3, 4]: 4 and 3 visited, 2 gets label 1 and does not expand: cluster 1 = {3, 2};
      row 1: opens cluster 2, stack [0, 1, 2]: 0 gets label 2: cluster 2 = {1, 0}.
    Labels [2, 2, 1, 1, 0, 0, -1]: a textbook DBSCAN would give one cluster of seven."""
    line = np.column_stack([np.arange(7.0), np.zeros(7), np.zeros(7)])
    assert oracle.dbscan(line, 1.0, 3).tolist() == [2, 2, 1, 1, 0, 0, -1]
    same = np.tile(np.array([[0.3, -1.2, 4.0]]), (12, 1))
    assert oracle.dbscan(same, 0.0, 12).tolist() == [0] * 12
    assert oracle.dbscan(same, 0.0, 13).tolist() == [-1] * 12
