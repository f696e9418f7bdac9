"""NumPy restatement of the SHOT352 rules of include/pcr.h (pcr_shot_lrf, pcr_shot352): the local reference frame of a keypoint
COORDINATE over its radius ball (weighted moments, eigenvectors, the sign rule with its five-median tie break) and the 32 x 11
histogram with its four interpolations, every contribution quantised to a multiple of 2^-32 and summed as an integer.

Everything is binary64, every dot product in the written order (a0*b0 + a1*b1) + a2*b2.  The moment sums are taken in whatever order
NumPy takes them and the eigenvectors come from LAPACK: frames agree with the device's to rounding (``gap`` and ``sign_margin`` say how
well a frame is conditioned), not to the bit.  Given the SAME frame, every hard decision of the histogram is the same bits on both
sides; only acos, atan2 and the order of the norm's sum differ (tests/test_gpu_shot.py derives the bound)."""
import numpy as np

from tests.pcl_fpfh_checks import balls

Q = 2.0 ** 32
Q4, Q2, Q34, Q78 = 0.785398163397448309615660845819875721, 1.57079632679489661923132169163975144, 2.35619449019234492884698253745962716, 2.74889357189106908365481296036956502
assert (Q4, Q2) == (np.pi / 4, np.pi / 2) and abs(Q34 - 3 * np.pi / 4) < 1e-15 and abs(Q78 - 7 * np.pi / 8) < 1e-15


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _signed(a, v, d2, rows):
    """The sign rule, from the eigenvector with its component of largest magnitude made positive -> (axis, tie: whether the five
    medians decided)."""
    K = len(v)
    if a[np.argmax(np.abs(a))] < 0:                      # (argmax: the first of equal magnitudes)
        a = -a
    t = _dot(v, a)
    s = 2 * int((t >= 0).sum()) - K
    if s < 0:
        return -a, False
    if s > 0:
        return a, False
    order = np.lexsort((rows, d2))                       # ascending (d2, caller row)
    five = order[K // 2 - 2: K // 2 + 3]
    assert len(five) == 5
    return (-a if int((t[five] > 0).sum()) < 3 else a), True


def lrf(pts, kp, r):
    """-> dict(frames (m,3,3) rows x, y, z; counts (m,); gap (m,): the smaller eigenvalue gap over e2; sign_margin (m,): the smallest
    |v.a| / |v| over the nonzero neighbours and both axes; tie (m,2): whether x / z were decided by the five medians)."""
    p = np.asarray(pts, dtype=np.float64)
    kp = np.asarray(kp, dtype=np.float64).reshape(-1, 3)
    m = len(kp)
    frames = np.full((m, 3, 3), np.nan)
    counts = np.zeros(m, dtype=np.int64)
    gap = np.zeros(m)
    margin = np.full(m, np.inf)
    tie = np.zeros((m, 2), dtype=bool)
    for i, b in enumerate(balls(p, kp, r)):
        K = counts[i] = len(b)
        if K < 5:
            continue
        v = p[b] - kp[i]
        d2 = _dot(v, v)
        w = r - np.sqrt(d2)
        if not w.sum() > 0:
            continue
        wv = w[:, None] * v
        M = (wv[:, :, None] * v[:, None, :]).sum(axis=0) / w.sum()
        e, V = np.linalg.eigh(M)                          # ascending
        x = V[:, 2] / np.sqrt(_dot(V[:, 2], V[:, 2]))
        z = V[:, 0] / np.sqrt(_dot(V[:, 0], V[:, 0]))
        nz = d2 != 0
        if nz.any():
            ln = np.sqrt(d2[nz])
            margin[i] = min((np.abs(_dot(v[nz], x)) / ln).min(), (np.abs(_dot(v[nz], z)) / ln).min())
        x, tie[i, 0] = _signed(x, v, d2, b)
        z, tie[i, 1] = _signed(z, v, d2, b)
        frames[i] = [x, np.cross(z, x), z]
        gap[i] = min(e[1] - e[0], e[2] - e[1]) / max(e[2], 1e-300)
    return dict(frames=frames, counts=counts, gap=gap, sign_margin=margin, tie=tie)


def _quant(v):
    return np.rint(v * Q).astype(np.int64)


def _tiny(v):
    return np.where(np.abs(v) < 1e-30, 0.0, v)


def histogram(v, d2, n, F, r):
    """The integer histogram (352,) int64 of one keypoint from its ball: v (K,3) = p_j - x, d2 (K,), normals n (K,3), frame F (3,3)
    finite -> (hist, neighbours that were not skipped)."""
    keep = np.isfinite(n).all(axis=1) & (d2 != 0)
    v, d2, n = v[keep], d2[keep], n[keep]
    h = np.zeros(352, dtype=np.int64)
    if not len(v):
        return h, 0
    r4, rh, r34 = 0.25 * r, 0.5 * r, 0.75 * r
    c = np.clip(_dot(n, F[2]), -1.0, 1.0)
    b = ((1.0 + c) * 10) / 2
    X, Y, Z = _tiny(_dot(v, F[0])), _tiny(_dot(v, F[1])), _tiny(_dot(v, F[2]))
    d = np.sqrt(d2)
    bit4 = (Y > 0) | ((Y == 0) & (X < 0))
    bit3 = np.where((X > 0) | ((X == 0) & (Y > 0)), ~bit4, bit4)
    desc = ((bit4.astype(np.int64) << 3) + (bit3.astype(np.int64) << 2)) << 1
    desc = desc + np.where((X * Y > 0) | (X == 0), np.where(np.abs(X) >= np.abs(Y), 0, 4), np.where(np.abs(X) > np.abs(Y), 4, 0))
    desc = desc + (Z > 0) + 2 * (d > rh)
    sel = desc >> 2
    step = np.floor(b + 0.5).astype(np.int64)
    rho = b - step
    vol = desc * 11
    W = 1.0 - np.abs(rho)
    np.add.at(h, np.where(rho > 0, vol + (step + 1) % 10, vol + (step - 1 + 10) % 10), _quant(np.where(rho > 0, rho, -rho)))
    # radial
    far = d > rh
    t = np.where(far, (d - r34) / rh, (d - r4) / rh)
    alone = np.where(far, d > r34, d < r4)               # the outermost / innermost quarter: nothing goes to the other shell
    W = W + np.where(far == alone, 1 - t, 1 + t)         # far: (alone ? 1 - t : 1 + t); near: (alone ? 1 + t : 1 - t)
    s = ~alone
    np.add.at(h, (np.where(far, desc - 2, desc + 2) * 11 + step)[s], _quant(np.where(far, -t, t))[s])
    # elevation
    theta = np.arccos(np.clip(Z / d, -1.0, 1.0))
    low = Z <= 0
    u = np.where(low, (theta - Q34) / Q2, (theta - Q4) / Q2)
    alone = np.where(low, theta > Q34, theta < Q4)
    W = W + np.where(low == alone, 1 - u, 1 + u)
    s = ~alone
    np.add.at(h, (np.where(low, desc + 1, desc - 1) * 11 + step)[s], _quant(np.where(low, -u, u))[s])
    # azimuth
    az = (X != 0) | (Y != 0)
    a = np.clip((np.arctan2(Y, X) - (-Q78 + Q4 * sel)) / Q4, -0.5, 0.5)
    W = np.where(az, W + np.where(a > 0, 1 - a, 1 + a), W)
    np.add.at(h, (np.where(a > 0, (desc + 4) % 32, (desc - 4 + 32) % 32) * 11 + step)[az], _quant(np.where(a > 0, a, -a))[az])
    np.add.at(h, vol + step, _quant(W))
    return h, len(v)


def normalised(h):
    """h_b = integer 2^-32; out_b = h_b / sqrt(sum h_b^2), the sum in bin order; a zero norm: NaN."""
    hb = h.astype(np.float64) * (1.0 / Q)
    with np.errstate(invalid="ignore", divide="ignore"):
        return hb / np.sqrt(np.add.accumulate(hb * hb)[-1])


def shot352(pts, nrm, kp, r, frames=None):
    """-> dict(values (m,352) binary64, hist (m,352) int64, counts (m,), frames (m,3,3) the frames used, used (m,) the neighbours that
    were not skipped, lrf: the dict of ``lrf`` when the frames were computed here)."""
    p = np.asarray(pts, dtype=np.float64)
    nrm = np.asarray(nrm, dtype=np.float64)
    kp = np.asarray(kp, dtype=np.float64).reshape(-1, 3)
    m = len(kp)
    own = lrf(p, kp, r) if frames is None else None
    frames = own["frames"] if frames is None else np.asarray(frames, dtype=np.float64).reshape(m, 3, 3)
    values = np.full((m, 352), np.nan)
    hist = np.zeros((m, 352), dtype=np.int64)
    counts = np.zeros(m, dtype=np.int64)
    used = np.zeros(m, dtype=np.int64)
    for i, b in enumerate(balls(p, kp, r)):
        counts[i] = len(b)
        if not np.isfinite(frames[i]).all():
            continue
        v = p[b] - kp[i]
        hist[i], used[i] = histogram(v, _dot(v, v), nrm[b], frames[i], r)
        values[i] = normalised(hist[i])
    return dict(values=values, hist=hist, counts=counts, frames=frames, used=used, lrf=own)
