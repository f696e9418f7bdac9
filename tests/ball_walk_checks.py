"""Inputs on which the walkers of csrc/pcr_ball_visit.h can disagree about who is in a ball (tests/test_gpu_ball_walk.py,
scripts/ball_walk_bits.py).  No device code here."""
import numpy as np

BUILT_RADIUS = 1.0
# ball sizes around the walkers' trip lengths: 4 records a trip of the lane-group walk, 64 positions a trip of the wave walk, the 128
# and 256 staged entries of the PCL-rule SPFH / FPFH passes
BALL_SIZES = (1, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257)


def built_cloud(seed=9):
    """One cluster per size in BALL_SIZES, each inside a cube of side 0.5 r (diagonal 0.87 r: every row of a cluster is within r of
    every other) at a seeded offset against the cell grid, 4 r or more from the next cluster -- the ball of a row is its cluster and
    has exactly that many rows -- plus two rows exactly r apart on the x axis (integer coordinates: the distance is exact and is the
    radius).  Rows shuffled.  -> (1477, 3) float64, read-only."""
    rng = np.random.default_rng(seed)
    r = BUILT_RADIUS
    parts = []
    for i, k in enumerate(BALL_SIZES):
        corner = np.array([8.0 * r * (i % 4), 8.0 * r * (i // 4), 0.0]) + rng.uniform(0.0, r, 3)
        parts.append(corner + rng.uniform(0.0, 0.5 * r, (k, 3)))
    parts.append(np.array([[40.0, 40.0, 40.0], [40.0 + r, 40.0, 40.0]]))
    pts = np.concatenate(parts)
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    pts.setflags(write=False)
    return pts


def lattice(side=5):
    """The side^3 unit lattice: at radius 1 the six axis neighbours of a row lie exactly on the radius.  -> (side^3, 3) float64, read-only."""
    g = np.arange(side, dtype=np.float64)
    pts = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    pts.setflags(write=False)
    return pts
