"""TEST INFRASTRUCTURE -- NumPy restatement of the SIFT-3D rules of include/pcr.h (section "PCL keypoints": pcr_sift_scales,
pcr_sift_octave, pcr_sift_extrema, pcr_sift), brute force over all pairs: every ball is a row of the full distance matrix and N(i) comes
from an explicit sort by (d2, row), no tree.  For tests/ and for scripts/sift_bench.py (its scales and tables); the package never imports it.

PARITY UNPINNED: the functions restate the header's rules (pcl::SIFTKeypoint as PCLKeypoints/src/keypoints.cpp:85-109 configures it, with
the stated departure in the down-sampling), not the output of a PCL binary.

Every hard decision also reports its MARGIN -- how far the two sides of the comparison are apart -- so that a test can show, from the
restatement alone, that a device table within its error bound decides every entry the same way."""
from __future__ import annotations

import numpy as np

NN = 25


def scales(base, q):
    """sigma_s = base * pow(2.0, (s - 1.0) / q), s = 0 .. q + 2."""
    return np.array([base * 2.0 ** ((s - 1.0) / q) for s in range(q + 3)], dtype=np.float64)


def tables(sig):
    sig2 = sig * sig
    return sig2, 9.0 * sig2, -0.5 / sig2


def dist2(points):
    p = np.asarray(points, dtype=np.float64)
    dx = p[:, None, 0] - p[None, :, 0]
    dy = p[:, None, 1] - p[None, :, 1]
    dz = p[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def dog(points, field, sig, d2=None):
    """-> D (n, S - 1), counts (n,), info: {"K": counts, "V": max |v| over every ball, "lim_margin": min |d2 - lim_s| over all pairs and
    scales}."""
    p = np.asarray(points, dtype=np.float64)
    d2 = dist2(p) if d2 is None else d2
    v = p[:, field]
    _, lim, h = tables(np.asarray(sig, dtype=np.float64))
    resp = np.empty((len(p), len(lim)))
    lim_margin = np.inf
    for s in range(len(lim)):
        inside = d2 <= lim[s]
        w = np.where(inside, np.exp(d2 * h[s]), 0.0)
        resp[:, s] = (w * v[None, :]).sum(axis=1) / w.sum(axis=1)
        lim_margin = min(lim_margin, np.abs(d2 - lim[s]).min())
    ball = d2 <= lim[-1]
    V = np.where(ball, np.abs(v)[None, :], 0.0).max(axis=1)
    counts = ball.sum(axis=1).astype(np.int32)
    return resp[:, 1:] - resp[:, :-1], counts, {"K": counts, "V": V, "lim_margin": float(lim_margin)}


def bound(info):
    """|D_device - D| per row: 4 V (K + 8) 2^-52 (tests/test_gpu_sift.py derives it)."""
    return 4.0 * info["V"] * (info["K"] + 8.0) * 2.0 ** -52


def neighbours(d2_row, k=NN):
    """The min(k, n) rows smallest in (d2, row) -> (rows, gap between the last one in and the first one out, inf if there is none)."""
    order = np.lexsort((np.arange(len(d2_row)), d2_row))
    k = min(k, len(order))
    gap = np.inf if k == len(order) else float(d2_row[order[k]] - d2_row[order[k - 1]])
    return order[:k], gap


def extrema(points, D, contrast, d2=None):
    """-> entries (K, 2) int64 in ascending (row, c); margins: the smallest distance between the two sides of every decision that was
    reached, by kind -- "contrast", "own" (the row's adjacent columns), "nbr" (the 75 neighbour values, the row's own excluded), "kth"
    (the gap in d2 between the 25th and the 26th neighbour of a candidate; 0 when they tie: then the row decides, exactly); and
    "candidates", the rows that reach the neighbour test."""
    p = np.asarray(points, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    n, C = D.shape
    d2 = dist2(p) if d2 is None else d2
    entries = []
    m = {"contrast": np.inf, "own": np.inf, "nbr": np.inf, "kth": np.inf}
    cand = []
    for i in range(n):
        nb = None
        for c in range(1, C - 1):
            val, lo, hi = D[i, c], D[i, c - 1], D[i, c + 1]
            m["contrast"] = min(m["contrast"], abs(abs(val) - contrast))
            if not abs(val) >= contrast:
                continue
            m["own"] = min(m["own"], abs(val - lo), abs(val - hi))
            is_min, is_max = val < lo and val < hi, val > lo and val > hi
            if not (is_min or is_max):
                continue
            if nb is None:
                nb, gap = neighbours(d2[i])
                m["kth"] = min(m["kth"], gap)
                cand.append(i)
            others = D[nb[nb != i], c - 1:c + 2]
            if others.size:
                m["nbr"] = min(m["nbr"], float(np.abs(val - others).min()))
            block = D[nb, c - 1:c + 2]
            if (is_min and not (val > block).any()) or (is_max and not (val < block).any()):
                entries.append((i, c))
    m["candidates"] = np.array(cand, dtype=np.int64)
    return np.array(entries, dtype=np.int64).reshape(-1, 2), m


def min_margin(dog_info, margins):
    return min(dog_info["lim_margin"], margins["contrast"], margins["own"], margins["nbr"], margins["kth"])


def octave(points, base, q, contrast, field=1, sig=None):
    """One octave on the cloud as given -> dict(cloud, sig, D, counts, info, entries, margins)."""
    p = np.asarray(points, dtype=np.float64)
    sig = scales(base, q) if sig is None else np.asarray(sig, dtype=np.float64)
    d2 = dist2(p)
    D, counts, info = dog(p, field, sig, d2)
    entries, margins = extrema(p, D, contrast, d2)
    return {"cloud": p, "sig": sig, "D": D, "counts": counts, "info": info, "entries": entries, "margins": margins}


def sift(points, min_scale, n_octaves, q, contrast, field=1, *, downsample, scales_of=scales):
    """The octave loop -> dict(octaves: [octave dicts], sizes (n_octaves,), keypoints (K, 4): x, y, z, scale; octave (K,), row (K,),
    column (K,)).  ``downsample(points, leaf)`` is the voxel filter."""
    cloud = np.asarray(points, dtype=np.float64)
    scale = float(min_scale)
    octs, sizes = [], np.zeros(n_octaves, dtype=np.int64)
    kp, oc, row, col = [], [], [], []
    for o in range(n_octaves):
        cloud = np.asarray(downsample(cloud, scale), dtype=np.float64)
        if len(cloud) < NN:
            break
        sizes[o] = len(cloud)
        res = octave(cloud, scale, q, contrast, field, scales_of(scale, q))
        octs.append(res)
        for i, c in res["entries"]:
            kp.append([*cloud[i], res["sig"][c]])
            oc.append(o)
            row.append(i)
            col.append(c)
        scale *= 2.0
    return {"octaves": octs, "sizes": sizes, "keypoints": np.array(kp, dtype=np.float64).reshape(-1, 4), "octave": np.array(oc, dtype=np.int64),
            "row": np.array(row, dtype=np.int64), "column": np.array(col, dtype=np.int64)}


# ------------------------------------------------------------------------------------------------ the shared cases
SEEDED = {"min_scale": 0.1, "n_octaves": 3, "q": 3, "contrast": 0.002}
SEEDED_SEED = 7


def seeded_case(seed=SEEDED_SEED):
    """4 000 rows of a noisy height field (the field is y) over [0,4]^2 in x and z, and a 666-row Gaussian blob above it."""
    rng = np.random.default_rng(seed)
    x, z = rng.uniform(0.0, 4.0, 4000), rng.uniform(0.0, 4.0, 4000)
    y = 0.35 * np.sin(2.3 * x) * np.cos(1.7 * z) + 0.15 * np.sin(5.1 * x + 0.7) * np.sin(4.3 * z) + rng.normal(0.0, 0.02, 4000)
    blob = rng.normal(0.0, 0.18, (666, 3)) + np.array([2.2, 0.9, 1.7])
    return np.r_[np.c_[x, y, z], blob]


SPARSE = {"base": 0.25, "q": 3, "contrast": 1e-3}


def sparse_case(seed=7):
    """About 60 rows: four groups of 3 or 4 rows scattered over a box many balls wide (balls of fewer than 25 rows, with values of their
    own), and two clumps of 26 whose balls hold more than 25 rows."""
    rng = np.random.default_rng(seed)
    far = np.concatenate([rng.normal(0.0, 0.5, (m, 3)) + rng.uniform(0.0, 30.0, 3) for m in (3, 4, 3, 4)])
    a = rng.normal(0.0, 0.35, (26, 3)) + np.array([5.0, 5.0, 5.0])
    b = rng.normal(0.0, 0.35, (26, 3)) + np.array([22.0, 9.0, 14.0])
    return np.r_[far[:7], a, far[7:], b]


ONE_BALL_SEED = {24: 1, 25: 1}   # (the first seed at which the restatement finds an entry)


def one_ball_case(n, seed=None):
    """n rows in a cube of side 3 (base scale 1, q = 3: every ball of radius 3 * 2^(4/3) holds them all, and so does one cell)."""
    rng = np.random.default_rng(1000 * (ONE_BALL_SEED.get(n, 0) if seed is None else seed) + n)
    return rng.uniform(0.0, 3.0, (n, 3))


def lattice():
    """6 x 6 x 4 rows at unit spacing, x fastest."""
    z, y, x = np.meshgrid(np.arange(4.0), np.arange(6.0), np.arange(6.0), indexing="ij")
    return np.c_[x.ravel(), y.ravel(), z.ravel()]


def lattice_row(x, y, z):
    return x + 6 * (y + 6 * z)


LATTICE_ROW = 50                                  # (2, 2, 1): an interior row
LATTICE_CORNERS = [7, 9, 19, 21, 79, 81, 91, 93]  # its 8 neighbours at d2 = 3, ascending: after itself, 6 rows at d2 = 1 and 12 at d2 = 2,
#                                                   the 6 lowest of them are places 20..25 of N -- 81 is in, 91 and 93 are not


def lattice_tables():
    """name -> (table (144, 3) of integers, contrast, the entries): the tie rules on crafted tables."""
    def table(fill, row, **others):
        D = np.full((144, 3), float(fill))
        D[LATTICE_ROW] = row
        for r, v in others.items():
            D[int(r[1:])] = v
        return D
    yes = np.array([[LATTICE_ROW, 1]], dtype=np.int64)
    no = np.empty((0, 2), dtype=np.int64)
    return {
        "a maximum tied with every neighbour is kept": (table(5, [0, 5, 0]), 1.0, yes),
        "a minimum tied with every neighbour is kept": (table(-5, [0, -5, 0]), 1.0, yes),
        "a tie with the row's own adjacent column kills": (table(0, [5, 5, 0]), 1.0, no),
        "a tie with the row's own adjacent column kills a minimum": (table(0, [0, -5, -5]), 1.0, no),
        "tied for the 25th place, the lower row is in and beats": (table(0, [0, 5, 0], r81=[9, 9, 9]), 1.0, no),
        "tied for the 25th place, the higher row is out": (table(0, [0, 5, 0], r91=[9, 9, 9]), 1.0, yes),
        "tied for the 25th place, both: the lower decides": (table(0, [0, 5, 0], r81=[0, 0, 0], r91=[9, 9, 9], r93=[9, 9, 9]), 1.0, yes),
    }
