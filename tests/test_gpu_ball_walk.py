"""GPU: the three walkers of csrc/pcr_ball_visit.h and the radius search agree exactly on who is in a ball -- the lane-group walk
(estimate_normals_radius), the wave walk (fpfh33 at the cloud's own rows), the lane-group walk over the grid of the cloud as stored
(iss_keypoints) and radius_search_batch -- and all equal the restatement (tests/harris_checks.neighbours: (dx^2 + dy^2) + dz^2 <= r^2
in binary64).  Counts are integers: no tolerance.  Inputs (tests/ball_walk_checks.py): balls of 1 .. 257 rows around the walkers' trip
lengths, and rows exactly on the radius."""
import numpy as np
import pytest

from tests import ball_walk_checks as bw
from tests import harris_checks as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["built", "lattice"])
def test_walkers_and_search_agree_on_ball_membership(pcp, ctx, name):
    pts, r = (bw.built_cloud(), bw.BUILT_RADIUS) if name == "built" else (bw.lattice(), 1.0)
    nb = hc.neighbours(pts, r)
    want = np.array([len(b) for b in nb], dtype=np.int32)
    # the conditions on the input, on the restatement
    assert len(pts) <= 3000
    if name == "built":
        assert set(bw.BALL_SIZES) <= set(want.tolist())
    on_radius = sum(int((((pts[b] - pts[i]) ** 2).sum(axis=1) == r * r).sum()) for i, b in enumerate(nb))
    assert on_radius >= 2
    _, normals_counts = pcp.estimate_normals_radius(pts, r, ctx=ctx, return_counts=True)
    _, info = pcp.fpfh33(pts, pts, 10, r, ctx=ctx, return_info=True)
    _, _, iss_counts = pcp.iss_keypoints(pts, radius=r, non_max_radius=r, ctx=ctx, return_details=True)
    root = pcp.kdtree_construction(pts, 1, ctx=ctx)
    offsets, _, _ = pcp.radius_search_batch(root, pts, r)
    root.index.free()
    print(name, "rows", len(pts), "ball sizes", want.min(), "..", want.max(), "pairs exactly on the radius", on_radius)
    assert np.array_equal(normals_counts, want)
    assert np.array_equal(info["counts"], want)
    assert np.array_equal(iss_counts, want)
    assert np.array_equal(np.diff(offsets), want)
