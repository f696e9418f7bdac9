"""NumPy restatement of the query cloud's lay-out (csrc/pcr_curve.h, pcr_cloud_morton_sort in csrc/pcr_grid.hip) and the CPU model
of what a wave tile of the ICP pass stages under a given source order.  Shared by tests/test_query_curve_host.py,
tests/test_gpu_query_curve.py and scripts/tile_box_model.py.  NumPy and scipy only.

The lay-out: cell coordinates floor((p - lo) * (1 / cell)) over the cloud's own box, the low nb bits of each (nb = a third of the
bits the cloud's Morton key varies), and one of three keys:
  morton           bit b of axis d at key bit 3 b + d
  hilbert3         the 3-D Hilbert index (Skilling's transpose algorithm), x most significant
  hilbert2_minor   the 2-D Hilbert index of the two axes of largest extent, shifted left by the bit count of the third axis, or-ed with
                   the third axis' cell coordinate
The rule (`pick`): hilbert2_minor when the shortest extent is at most a quarter of the middle one, else hilbert3; equal extents go to
the lower axis index.  Records are ordered by a stable sort of the key."""
import numpy as np

COORD_BITS = 21          # PCR_COORD_BITS
GATE = np.sqrt(5.0)      # the ICP gate d^2 < 5 as a radius
TILE = 32                # records per wave tile


def _u(v):
    return np.uint64(v)


def axis_bits(ext, inv):
    """Bits of the cell coordinates along an axis of extent `ext` (pcr_morton_end_bit's count: +1 rounding slack, +1 for "count")."""
    kmax = np.floor(ext * inv) + 2.0
    nb = 1
    while nb < COORD_BITS - 1 and float(1 << nb) <= kmax:
        nb += 1
    return nb


def end_bit(lo, hi, inv):
    """pcr_morton_end_bit: the number of Morton key bits that vary over a cloud with box [lo, hi]."""
    return min(63, 3 * axis_bits(float(np.max(np.asarray(hi) - np.asarray(lo))), inv))


def morton_of_cells(ci, nb):
    ci = np.asarray(ci).astype(np.uint64)
    k = np.zeros(len(ci), dtype=np.uint64)
    for b in range(nb):
        for d in range(3):
            k |= ((ci[:, d] >> _u(b)) & _u(1)) << _u(3 * b + d)
    return k


def hilbert_of_cells(ci, nb):
    """Hilbert index of the low `nb` bits of the (m, N) integer coordinates `ci`, column 0 most significant (Skilling 2004)."""
    X = (np.asarray(ci).astype(np.uint64) & _u((1 << nb) - 1)).copy()
    n = X.shape[1]
    M = 1 << (nb - 1)
    Q = M
    while Q > 1:
        P = _u(Q - 1)
        for i in range(n):
            hit = (X[:, i] & _u(Q)) != 0
            t = np.where(hit, _u(0), (X[:, 0] ^ X[:, i]) & P)
            X[:, 0] ^= np.where(hit, P, _u(0))
            X[:, 0] ^= t
            X[:, i] ^= t
        Q >>= 1
    for i in range(1, n):
        X[:, i] ^= X[:, i - 1]
    t = np.zeros(len(X), dtype=np.uint64)
    Q = M
    while Q > 1:
        t ^= np.where((X[:, n - 1] & _u(Q)) != 0, _u(Q - 1), _u(0))
        Q >>= 1
    k = np.zeros(len(X), dtype=np.uint64)
    for i in range(n):
        x = X[:, i] ^ t
        for b in range(nb):
            k |= ((x >> _u(b)) & _u(1)) << _u(n * b + (n - 1 - i))
    return k


def hilbert3_of_cells(ci, nb):
    return hilbert_of_cells(np.asarray(ci)[:, :3], nb)


def hilbert2_minor_of_cells(ci, nb, ax=(0, 1, 2), nb_minor=1):
    ci = np.asarray(ci).astype(np.uint64)
    return (hilbert_of_cells(ci[:, [ax[0], ax[1]]], nb) << _u(nb_minor)) | (ci[:, ax[2]] & _u((1 << nb_minor) - 1))


def pick(lo, hi, inv, bits=None):
    """pcr_curve_pick: {"mode", "nb", "ax", "nb_minor"} of a cloud with box [lo, hi] at 1 / cell `inv`."""
    e = np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
    nb = (end_bit(lo, hi, inv) if bits is None else bits) // 3
    ax = sorted(range(3), key=lambda a: (-e[a], a))            # falling extent, the lower axis first among equals
    if e[ax[2]] <= 0.25 * e[ax[1]]:
        nbm = 1
        kmax = np.floor(e[ax[2]] * inv) + 2.0
        while nbm < nb and float(1 << nbm) <= kmax:
            nbm += 1
        return dict(mode="hilbert2_minor", nb=nb, ax=tuple(ax), nb_minor=nbm)
    return dict(mode="hilbert3", nb=nb, ax=tuple(ax), nb_minor=0)


def layout_cell(pts, cell):
    """The curve resolution pcr_cloud_morton_sort uses for a cloud laid out at `cell` (an index's level-0 cell)."""
    p = np.asarray(pts, dtype=np.float64)
    emax = float((p.max(0) - p.min(0)).max())
    if not cell > 0:
        cell = emax / 1024.0 if emax > 0 else 1.0
    return max(cell, emax / 262144.0)


def layout_keys(pts, cell, curve="rule"):
    """Keys of the records of `pts` as laid out at `cell`; curve = "rule" (the library's default), "morton", "hilbert3" or
    "hilbert2_minor" (the rule's axes and minor bit count, whatever the rule itself would pick)."""
    p = np.asarray(pts, dtype=np.float64)
    lo, hi = p.min(0), p.max(0)
    cell = layout_cell(p, cell)
    inv = 1.0 / cell
    ci = np.floor((p - lo) * inv).astype(np.int64)
    eb = end_bit(lo, hi, inv)
    nb = eb // 3
    if curve == "morton":
        return morton_of_cells(ci, nb)
    cv = pick(lo, hi, inv, eb)
    mode = cv["mode"] if curve == "rule" else curve
    if mode == "hilbert3":
        return hilbert3_of_cells(ci, nb)
    assert mode == "hilbert2_minor", mode
    nbm = cv["nb_minor"] if cv["mode"] == "hilbert2_minor" else axis_bits(float((hi - lo)[cv["ax"][2]]), inv)
    return hilbert2_minor_of_cells(ci, nb, cv["ax"], min(nbm, nb))


def layout_order(pts, cell, curve="rule"):
    """Caller row of every record in device order: the stable argsort of the key (a cloud of one point is never sorted)."""
    if len(pts) < 2:
        return np.arange(len(pts), dtype=np.int64)
    return np.argsort(layout_keys(pts, cell, curve), kind="stable").astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ the tile model
def auto_cell(tgt):
    """pcr_grid_plan's automatic level-0 cell of a target."""
    e = np.sort(np.asarray(tgt, dtype=np.float64).max(0) - np.asarray(tgt, dtype=np.float64).min(0))[::-1]
    return 0.55 * np.sqrt(e[0] * e[1] / len(tgt))


def staged_per_tile(q, order, tgt, tree):
    """Target points in the pass box of every tile: tiles are runs of 32 of `q[order]`; every query claims the ball to its exact
    nearest target, capped at the gate; the box is the bounding box of the tile's claims."""
    qs = np.asarray(q, dtype=np.float64)[order]
    d, _ = tree.query(qs, k=1)
    r = np.minimum(d, GATE)[:, None]
    xs = np.argsort(tgt[:, 0])
    tx = tgt[xs]
    nt = (len(qs) + TILE - 1) // TILE
    cnt = np.zeros(nt, dtype=np.int64)
    for t in range(nt):
        a, rr = qs[TILE * t:TILE * t + TILE], r[TILE * t:TILE * t + TILE]
        blo, bhi = (a - rr).min(0), (a + rr).max(0)
        c = tx[np.searchsorted(tx[:, 0], blo[0]):np.searchsorted(tx[:, 0], bhi[0], side="right")]
        cnt[t] = int(((c[:, 1] >= blo[1]) & (c[:, 1] <= bhi[1]) & (c[:, 2] >= blo[2]) & (c[:, 2] <= bhi[2])).sum())
    return cnt


def registered(src, T, tree):
    """`src` at the registered pose: T or its inverse, whichever brings it onto the target."""
    R, t = T[:3, :3], T[:3, 3]
    a, b = src @ R.T + t, (src - t) @ R
    return a if tree.query(a[::50])[0].mean() < tree.query(b[::50])[0].mean() else b
