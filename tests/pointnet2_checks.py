"""NumPy restatements of the six PointNet++ ops under the rules of include/pcr.h ("PointNet++ set-abstraction ops"), written from those
rules: every step is a float32 operation in the written order, so the device kernels must reproduce them bit for bit.  Plus float64
restatements of the three gradients with the quantities of the summation bound, and independent formulations of the searches (a full
distance matrix and a sort) that the host tests hold the restatements against."""
import numpy as np

F32 = np.float32
FAR = F32(1e10)


def d2_rows(p, pts):
    """((dx*dx) + (dy*dy)) + (dz*dz) in float32 from the point p (3,) to every row of pts (n, 3)."""
    d = pts.astype(F32, copy=False) - np.asarray(p, dtype=F32)
    sq = d * d
    return (sq[:, 0] + sq[:, 1]) + sq[:, 2]


def eligible(pts):
    """|p|^2 in float32, widened, > 1e-3: the points furthest point sampling may update and choose."""
    sq = pts * pts
    mag = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    return ~(mag.astype(np.float64) <= 1e-3)


def fps_one(pts, m, tied=None):
    """One cloud (n, 3) -> (m,) int32.  tied: a list that receives the picks j whose maximum more than one eligible point attained."""
    pts = np.ascontiguousarray(pts, dtype=F32)
    n = len(pts)
    ok = eligible(pts)
    rows = np.flatnonzero(ok)
    temp = np.full(n, FAR, dtype=F32)
    out = np.zeros(m, dtype=np.int32)
    for j in range(1, m):
        d = d2_rows(pts[out[j - 1]], pts)
        temp[ok] = np.minimum(d[ok], temp[ok])
        if len(rows):
            cand = temp[rows]
            first = np.argmax(cand)                                  # argmax: the first of equal maxima
            out[j] = rows[first]
            if tied is not None and np.count_nonzero(cand == cand[first]) > 1:
                tied.append(j)
    return out


def fps(xyz, m):
    """xyz (B, n, 3) -> (B, m) int32."""
    return np.stack([fps_one(c, m) for c in xyz]) if len(xyz) else np.zeros((0, m), np.int32)


def fps_by_matrix(pts, m):
    """Independent formulation: the full float32 distance matrix once, every pick the arg-max of the column minima over the rows
    picked so far."""
    pts = np.ascontiguousarray(pts, dtype=F32)
    d = pts[:, None, :] - pts[None, :, :]
    sq = d * d
    D = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    ok = eligible(pts)
    picks = [0]
    for _ in range(1, m):
        col = np.minimum(D[picks].min(axis=0), FAR)
        best, arg = -1.0, 0
        for k in range(len(pts)):           # the stated rule, literally: largest, lowest index among equals, eligible only
            if ok[k] and col[k] > best:
                best, arg = col[k], k
        picks.append(arg)
    return np.array(picks[:m], dtype=np.int32)


def ball_query(radius, nsample, xyz, new_xyz):
    """xyz (B, n, 3), new_xyz (B, m, 3) -> (B, m, nsample) int32."""
    r = F32(radius)
    r2 = F32(r * r)
    B, m = new_xyz.shape[:2]
    out = np.zeros((B, m, nsample), dtype=np.int32)
    for b in range(B):
        for j in range(m):
            hits = np.flatnonzero(d2_rows(new_xyz[b, j], xyz[b]) < r2)[:nsample]
            if len(hits):
                out[b, j, :] = hits[0]
                out[b, j, :len(hits)] = hits
    return out


def ball_query_by_sort(radius, nsample, pts, centre):
    """Independent formulation for one centre: sort the distance row, count what lies below r2, order those by index."""
    r = F32(radius)
    r2 = F32(r * r)
    d = d2_rows(centre, pts)
    order = np.argsort(d, kind="stable")
    inside = int(np.searchsorted(d[order], r2, side="left"))
    hits = np.sort(order[:inside])[:nsample]
    row = np.zeros(nsample, dtype=np.int32)
    if len(hits):
        row[:] = hits[0]
        row[:len(hits)] = hits
    return row


def three_nn(unknown, known):
    """unknown (B, n, 3), known (B, m, 3) -> squared distances (B, n, 3) float32 ascending and indices (B, n, 3) int32, by insertion
    with a strict <."""
    B, n = unknown.shape[:2]
    m = known.shape[1]
    dist2 = np.full((B, n, 3), np.inf, dtype=F32)
    idx = np.zeros((B, n, 3), dtype=np.int32)
    for b in range(B):
        # all unknown points at once, the known points in index order: the insertion is the same per row
        best, arg = dist2[b], idx[b]
        for k in range(m):
            d = d2_rows(known[b, k], unknown[b])
            lt0, lt1, lt2 = d < best[:, 0], d < best[:, 1], d < best[:, 2]
            new2 = np.where(lt1, best[:, 1], np.where(lt2, d, best[:, 2]))
            arg2 = np.where(lt1, arg[:, 1], np.where(lt2, k, arg[:, 2]))
            new1 = np.where(lt0, best[:, 0], np.where(lt1, d, best[:, 1]))
            arg1 = np.where(lt0, arg[:, 0], np.where(lt1, k, arg[:, 1]))
            new0 = np.where(lt0, d, best[:, 0])
            arg0 = np.where(lt0, k, arg[:, 0])
            best[:, 0], best[:, 1], best[:, 2] = new0, new1, new2
            arg[:, 0], arg[:, 1], arg[:, 2] = arg0, arg1, arg2
    return dist2, idx


def three_nn_by_sort(u, known):
    """Independent formulation for one unknown point: a stable sort of its distance row (of equal distances the earlier index first)."""
    d = d2_rows(u, known)
    order = np.argsort(d, kind="stable")[:3]
    dist2 = np.full(3, np.inf, dtype=F32)
    idx = np.zeros(3, dtype=np.int32)
    dist2[:len(order)] = d[order]
    idx[:len(order)] = order
    return dist2, idx


def three_interpolate(points, idx, weight):
    """points (B, c, m), idx / weight (B, n, 3) -> (B, c, n): (p1*w1 + p2*w2) + p3*w3 in float32."""
    B = points.shape[0]
    out = np.empty((B, points.shape[1], idx.shape[1]), dtype=F32)
    for b in range(B):
        p, w = points[b].astype(F32, copy=False), weight[b].astype(F32, copy=False)
        t = [p[:, idx[b, :, s]] * w[None, :, s] for s in range(3)]
        out[b] = (t[0] + t[1]) + t[2]
    return out


def gather(points, idx):
    """points (B, c, n), idx (B, npoints) -> (B, c, npoints)."""
    return np.stack([points[b][:, idx[b]] for b in range(len(points))])


def group(points, idx):
    """points (B, c, n), idx (B, npoints, nsample) -> (B, c, npoints, nsample)."""
    return np.stack([points[b][:, idx[b]] for b in range(len(points))])


# ------------------------------------------------------------------ gradients, float64
def scatter_grad(terms, idx, n):
    """terms (B, c, K) float64 summed into (B, c, n) at idx (B, K).  Returns the sums, the sums of |terms| and the number of terms per
    output: what the bound t * u / (1 - t * u) * sum|terms|, u = 2^-24, of a float32 summation in any order needs."""
    B, c, K = terms.shape
    total = np.zeros((B, c, n))
    mag = np.zeros((B, c, n))
    count = np.zeros((B, 1, n))
    for b in range(B):
        for ch in range(c):
            np.add.at(total[b, ch], idx[b], terms[b, ch])
            np.add.at(mag[b, ch], idx[b], np.abs(terms[b, ch]))
        np.add.at(count[b, 0], idx[b], 1.0)
    return total, mag, count


def gather_grad(grad_out, idx, n):
    return scatter_grad(grad_out.astype(np.float64), idx, n)


def group_grad(grad_out, idx, n):
    B, c = grad_out.shape[:2]
    return scatter_grad(grad_out.astype(np.float64).reshape(B, c, -1), idx.reshape(B, -1), n)


def three_interpolate_grad(grad_out, idx, weight, m):
    B, c, n = grad_out.shape
    terms = grad_out.astype(np.float64)[:, :, :, None] * weight.astype(np.float64)[:, None, :, :]
    return scatter_grad(terms.reshape(B, c, 3 * n), idx.reshape(B, 3 * n), m)


def summation_bound(mag, count):
    u = 2.0 ** -24
    return count * u / (1.0 - count * u) * mag
