"""Families, references and metrics for the small dense solves of csrc/pcr_linalg.h, reached through pcr_debug_linalg (include/pcr.h):
tests/test_linalg_host.py runs them through the host build, tests/test_gpu_linalg.py through the device build.  No library code.

Reference: mpmath at 60 digits (svd_r, eigsy, lu_solve) on the binary64 inputs as given, computed once per process.
Yardstick: every metric is also taken from plain NumPy in binary64 (LAPACK's svd / eigh / solve and a NumPy restatement of
kabsch_from_moments): that is another algorithm on the same inputs, not the code under test.
Bound, for every family and metric: max(8 x the yardstick's worst value in that family, 1e-14).  The 8 covers what the device build
adds over LAPACK (two reciprocal square roots of <= 2 ulp each where LAPACK divides once, contraction that changes which products
round, about three times as many rotations in cyclic Jacobi); a skipped sweep, a wrong sign or a wrong completion shows at 1e-8 or
above (the sweep test's own thresholds are 1e-8 relative); the floor is the project's number for unit rows (tests/test_gpu_shot.py,
tests/test_gpu_harris.py) and is needed where LAPACK is exact (diagonal and zero inputs).

The metrics themselves are evaluated in np.longdouble, so that their own rounding stays below what they measure.
"""
import functools

import mpmath as mp
import numpy as np

DPS = 60
FACTOR, FLOOR = 8.0, 1e-14
IN = (9, 18, 6, 21, 30, 27)      # doubles per problem, by op (include/pcr.h)
OUT = (21, 21, 18, 13, 22, 23)
LD = np.longdouble
I3 = np.eye(3)


def solve(L, handle, op, inp):
    """n problems through pcr_debug_linalg (handle None: the host build) -> (n, OUT[op]); rows the call did not write stay NaN."""
    inp = np.ascontiguousarray(inp, dtype=np.float64).reshape(-1, IN[op])
    out = np.full((len(inp), OUT[op]), np.nan)
    st = L.lib().pcr_debug_linalg(handle, op, L.dptr(inp), len(inp), L.dptr(out))
    assert st == L.PCR_OK, st
    return out


def _ld(x):
    """mpf -> longdouble, both halves (inside mp.workdps)."""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def _ld_matrix(M):
    return np.array([[_ld(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=LD)


def _fro(a):
    return np.sqrt((a * a).sum(axis=(-2, -1)))


def _unit(v):
    return np.where(v > 0, v, 1)


def orth(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def between(rng, s):
    return orth(rng) @ np.diag(np.asarray(s, dtype=np.float64)) @ orth(rng).T


def givens(p, q, theta):
    G = np.eye(3)
    G[p, p] = G[q, q] = np.cos(theta)
    G[p, q], G[q, p] = -np.sin(theta), np.sin(theta)
    return G


class Problems:
    """Named families laid end to end: inp (n, IN[op]), family[i] the name of row i; base(name) is the family whose yardstick bounds it."""

    def __init__(self):
        self.rows, self.family = [], []

    def add(self, name, row):
        self.rows.append(np.asarray(row, dtype=np.float64).reshape(-1))
        self.family.append(name)

    def done(self):
        self.inp = np.array(self.rows)
        self.inp.setflags(write=False)
        self.family = np.array(self.family)
        self.names = list(dict.fromkeys(self.family.tolist()))
        return self

    def rows_of(self, name):
        return np.flatnonzero(self.family == name)


def base(name):
    return name.split(":")[0]


# ------------------------------------------------------------------------------------------------------------- ops 0 and 1: svd3
SVD_FULL = ("gauss", "close", "orthogonal", "reflect", "scale", "threshold")   # the polar metric leaves none of these out
SVD_DEFICIENT = ("rank1", "rank2", "zero")                                     # ... and all of these
THETAS = (1.0, 1e-3, 1e-7, 1e-9, 1e-12)
ETAS = (1e-2, 1e-6, 1e-9, 1e-12, 0.0)
WARM = ("near", "random", "signed_perm", "identity")


@functools.lru_cache(maxsize=None)
def svd_problems():
    rng = np.random.default_rng(20240)
    P = Problems()
    for _ in range(200):
        P.add("gauss", rng.normal(size=(3, 3)))
    for s in ((1, 1e-4, 1e-8), (1, 1e-8, 1e-16), (1, 1e-3, 1e-3), (1e8, 1, 1e-8)):
        for _ in range(10):
            P.add("graded", between(rng, s))
    for s in ((1, 1, 1), (1, 1, .5), (1, .5, .5), (1, 1 - 1e-15, 1 - 2e-15), (1, 1 - 1e-9, 1 - 2e-9), (1, 1 - 1e-12, .3)):
        for _ in range(8):
            P.add("close", between(rng, s))
    for _ in range(20):
        q = orth(rng)
        P.add("orthogonal", q * np.sign(np.linalg.det(q)))
    for M in (I3, 3 * I3, -I3, np.roll(I3, 1, axis=0), np.diag([1.0, -1.0, 1.0])):
        P.add("orthogonal", M)
    for _ in range(30):   # det U det V = -1
        U, V = orth(rng), orth(rng)
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            V[:, 2] = -V[:, 2]
        P.add("reflect", U @ np.diag(rng.uniform(0.2, 2.0, 3)) @ V.T)
    small = lambda: rng.integers(-4, 5, 3).astype(np.float64)
    while P.family.count("rank2") < 20:
        u1, u2, v1, v2 = small(), small(), small(), small()
        if np.any(np.cross(u1, u2)) and np.any(np.cross(v1, v2)):   # (integers: the cross products are exact)
            P.add("rank2", np.outer(u1, v1) + np.outer(u2, v2))
    while P.family.count("rank1") < 20:
        u, v = small(), small()
        if np.any(u) and np.any(v):
            P.add("rank1", np.outer(u, v))
    P.add("rank1", np.outer(I3[0], I3[2]))
    P.add("rank1", np.outer(I3[1], I3[1]))
    P.add("zero", np.zeros((3, 3)))
    for f in (1e30, 1e-30, 2.0**100, 2.0**-100, 1e60, 1e-60):
        for _ in range(4):
            P.add("scale", between(rng, (1, .5, .25)) * f)
    for M in ([[1, 2, 3], [4, 5, 6], [7, 8, 9]], [[1, 1, 1], [1, 1, 1], [1, 1, 1]], [[1, 0, 3], [4, 0, 6], [7, 0, 9]],
              [[0, 0, 3], [0, 0, 6], [0, 0, 9]], [[1, 2, 0], [4, 5, 0], [7, 8, 0]], [[0, 2, 0], [0, -5, 0], [0, 8, 0]]):
        P.add("sparse", M)
    # both clauses of the `rotated` test in svd3_rotate: the inner product of columns p, q is ~ sin(2 theta) eta, the angle that
    # zeroes it ~ theta whatever eta is
    for p, q in ((0, 1), (0, 2), (1, 2)):
        for theta in THETAS:
            for eta in ETAS:
                for random_u in (False, True):
                    s = np.full(3, 0.37)
                    s[p], s[q] = 1.0, 1.0 + eta
                    U = orth(rng) if random_u else I3
                    P.add("threshold", U @ np.diag(s) @ givens(p, q, theta).T)
    return P.done()


@functools.lru_cache(maxsize=None)
def svd_warm_problems():
    """Op 1: every `threshold` and `close` matrix with four V0 -> (Problems with families "threshold:near" ..., rows of svd_problems())."""
    cold = svd_problems()
    rng = np.random.default_rng(20241)
    P, src = Problems(), []
    perms = [np.roll(I3, k, axis=0)[:, ::d] for k in range(3) for d in (1, -1)]
    for fam in ("threshold", "close"):
        for i in cold.rows_of(fam):
            H = cold.inp[i].reshape(3, 3)
            V = np.linalg.svd(H)[2].T
            q, r = np.linalg.qr(V + 1e-6 * rng.normal(size=(3, 3)))
            starts = {"near": q * np.sign(np.diag(r)), "random": orth(rng),
                      "signed_perm": perms[rng.integers(6)] * rng.choice([-1.0, 1.0], 3), "identity": I3}
            for kind in WARM:
                P.add(f"{fam}:{kind}", np.concatenate([H.reshape(-1), starts[kind].reshape(-1)]))
                src.append(i)
    return P.done(), np.array(src)


@functools.lru_cache(maxsize=None)
def svd_reference():
    """-> s (n, 3) descending, R = U V^T (n, 3, 3), both longdouble, for svd_problems()."""
    inp = svd_problems().inp
    s, R = np.zeros((len(inp), 3), dtype=LD), np.zeros((len(inp), 3, 3), dtype=LD)
    with mp.workdps(DPS):
        for i, row in enumerate(inp):
            U, S, Vt = mp.svd_r(mp.matrix(row.reshape(3, 3).tolist()))
            s[i] = sorted((_ld(S[k]) for k in range(3)), reverse=True)
            R[i] = _ld_matrix(U * Vt)
    return s, R


def svd_metrics(H, U, s, V, ref_s, ref_R):
    """-> metric -> (n,) float64; `polar` is NaN where sigma_3 <= 1e-6 sigma_1 (left out)."""
    H, U, s, V = (np.asarray(a).astype(LD) for a in (H, U, s, V))
    nH = _unit(_fro(H))
    out = {"recon": _fro(np.einsum("nij,nj,nkj->nik", U, s, V) - H) / nH,
           "orthU": np.abs(np.einsum("nji,njk->nik", U, U) - I3).max(axis=(1, 2)),
           "orthV": np.abs(np.einsum("nji,njk->nik", V, V) - I3).max(axis=(1, 2)),
           "sval": np.abs(-np.sort(-s, axis=1) - ref_s).max(axis=1) / nH}
    full = ref_s[:, 2] > 1e-6 * ref_s[:, 0]
    polar = _fro(np.einsum("nij,nkj->nik", U, V) - ref_R) * (ref_s[:, 1] + ref_s[:, 2]) / _unit(ref_s[:, 0])
    out["polar"] = np.where(full, polar, np.nan)
    return {k: v.astype(np.float64) for k, v in out.items()}


def split_svd(out):
    return out[:, :9].reshape(-1, 3, 3), out[:, 9:12], out[:, 12:21].reshape(-1, 3, 3)


def svd_evaluate(out, warm=False):
    """Metrics of an op 0 (warm: op 1) result."""
    ref_s, ref_R = svd_reference()
    if warm:
        P, src = svd_warm_problems()
        ref_s, ref_R = ref_s[src], ref_R[src]
    else:
        P = svd_problems()
    U, s, V = split_svd(out)
    assert np.isfinite(out).all() and (s >= 0).all(), "a singular value or vector is not finite, or a singular value is negative"
    return svd_metrics(P.inp[:, :9].reshape(-1, 3, 3), U, s, V, ref_s, ref_R)


@functools.lru_cache(maxsize=None)
def svd_yardstick():
    H = svd_problems().inp.reshape(-1, 3, 3)
    U, s, Vt = np.linalg.svd(H)
    return svd_metrics(H, U, s, Vt.transpose(0, 2, 1), *svd_reference())


# ------------------------------------------------------------------------------------------------------------- op 2: sym3_jacobi
def _sym(rng, lam):
    A = between_same(rng, lam)
    return (A + A.T) / 2


def between_same(rng, lam):
    Q = orth(rng)
    return Q @ np.diag(np.asarray(lam, dtype=np.float64)) @ Q.T


def upper(A):
    A = np.asarray(A, dtype=np.float64)
    return A[np.triu_indices(3)]


@functools.lru_cache(maxsize=None)
def eig_problems():
    rng = np.random.default_rng(20242)
    P = Problems()
    for _ in range(100):
        P.add("cov", upper(np.cov(rng.normal(size=(20, 3)) * rng.uniform(0.1, 3.0, 3), rowvar=False)))
    for lam in ((1, 1e-4, 1e-8), (1, 1e-8, 1e-16), (1, 1e-12, 0), (1e8, 1, 1e-8)):
        for _ in range(10):
            P.add("graded", upper(_sym(rng, lam)))
    for lam in ((1, 1, 1), (1, 1, .3), (1, .3, .3), (1, 1 - 1e-15, .3), (1, 1 - 1e-9, 1 - 2e-9), (1, 1 - 1e-13, 1 - 1e-13)):
        for _ in range(10):
            P.add("equal", upper(_sym(rng, lam)))
    ints = lambda n, k: rng.integers(-6, 7, (n, k)).astype(np.float64)
    for j in range(12):   # scatter matrices of integer points: every sum is exact, so is the rank
        if j < 3:         # axis-aligned: one coordinate is zero
            pts = ints(12, 3)
            pts[:, j] = 0.0
        else:             # the lattice two integer vectors span
            e = ints(2, 3)
            while not np.any(np.cross(e[0], e[1])):
                e = ints(2, 3)
            pts = ints(12, 2) @ e
        P.add("plane", upper(pts.T @ pts))
    for j in range(12):
        d = I3[j] if j < 3 else ints(1, 3)[0]
        while not np.any(d):
            d = ints(1, 3)[0]
        pts = np.outer(ints(12, 1)[:, 0], d)
        P.add("line", upper(pts.T @ pts))
    P.add("zero", np.zeros(6))
    for d in ((1, 2, 3), (3, 2, 1), (2, 2, 2), (1, 0, 0), (0, 0, 5), (-1, 2, -3), (1e-3, 1e3, 1)):
        P.add("diag", upper(np.diag(d)))
    for lam in ((1, -.5, -2), (1, -1, 0), (1e-3, -1, 1e3), (1, -1, 1), (-1, -2, -3)):
        for _ in range(3):
            P.add("indef", upper(_sym(rng, lam)))
    for f in (1e30, 1e-30, 2.0**100, 2.0**-100, 1e60, 1e-60, 1e150, 1e-150):
        for _ in range(3):
            P.add("scale", upper(_sym(rng, (1, .5, .25)) * f))
    for M in ([[2, 1, 0], [1, 2, 1], [0, 1, 2]], [[1, 1, 1], [1, 1, 1], [1, 1, 1]], [[4, 1, 2], [1, 3, 0], [2, 0, 5]]):
        P.add("hand", upper(M))
    return P.done()


def full_sym(tri):
    A = np.zeros((len(tri), 3, 3))
    iu = np.triu_indices(3)
    A[:, iu[0], iu[1]] = tri
    A[:, iu[1], iu[0]] = tri
    return A


@functools.lru_cache(maxsize=None)
def eig_reference():
    """-> eigenvalues (n, 3) ascending, longdouble, for eig_problems()."""
    A = full_sym(eig_problems().inp)
    lam = np.zeros((len(A), 3), dtype=LD)
    with mp.workdps(DPS):
        for i, M in enumerate(A):
            E = mp.eigsy(mp.matrix(M.tolist()), eigvals_only=True)
            lam[i] = sorted(_ld(E[k]) for k in range(3))
    return lam


def eig_metrics(A, A_after, Q, ref_lam):
    """Each relative to sum |A_ij| of the input."""
    A, A_after, Q = (np.asarray(a).astype(LD) for a in (A, A_after, Q))
    S = _unit(np.abs(A).sum(axis=(1, 2)))
    lam = np.einsum("nii->ni", A_after)
    off = A_after * (1 - I3)
    out = {"eig": np.abs(np.sort(lam, axis=1) - ref_lam).max(axis=1) / S,
           "resid": np.abs(np.einsum("nij,njk->nik", A, Q) - Q * lam[:, None, :]).max(axis=(1, 2)) / S,
           "orth": np.abs(np.einsum("nji,njk->nik", Q, Q) - I3).max(axis=(1, 2)),
           "off": np.abs(off).max(axis=(1, 2)) / S}
    return {k: v.astype(np.float64) for k, v in out.items()}


def eig_evaluate(out):
    assert np.isfinite(out).all()
    return eig_metrics(full_sym(eig_problems().inp), out[:, :9].reshape(-1, 3, 3), out[:, 9:].reshape(-1, 3, 3), eig_reference())


@functools.lru_cache(maxsize=None)
def eig_yardstick():
    A = full_sym(eig_problems().inp)
    w, Q = np.linalg.eigh(A)
    return eig_metrics(A, w[:, :, None] * I3, Q, eig_reference())


# ------------------------------------------------------------------------------------------------ ops 3 and 4: kabsch_from_moments
KINDS = ("general", "coplanar", "collinear", "mirrored", "exact")
KS = (3, 4, 5, 64, 1000)
ORIGINS = ("centroid", "world", "far")
CENTRE, EXTENT = np.array([5.0, -3.0, 2.0]), 10.0


def _rotation(rng, angle):
    w = rng.normal(size=3)
    w *= angle / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return I3 + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _point_set(kind, K, rng):
    """-> A, B (K, 3)."""
    Q = orth(rng)
    c = rng.uniform(-EXTENT / 2, EXTENT / 2, (K, 3))
    if kind == "coplanar":
        c[:, 2] = 0.0
    if kind == "collinear":
        c[:, 1:] = 0.0
    A = CENTRE + c @ Q.T
    R0, t0 = _rotation(rng, rng.uniform(0.05, 0.6)), rng.normal(scale=0.3, size=3)
    if kind == "exact":
        return A, A.copy()
    if kind == "mirrored":
        n = Q[:, 2]
        return A, (A - CENTRE) @ (I3 - 2 * np.outer(n, n)).T + CENTRE + t0 + rng.normal(scale=0.01, size=(K, 3))
    B = (A - CENTRE) @ R0.T + CENTRE + t0
    if kind == "general":
        B = B + rng.normal(scale=0.01, size=(K, 3))
    return A, B


def moments_mp(A, B, origin):
    """Raw moments about `origin`, accumulated in mpmath and rounded once -> m[18] (binary64)."""
    with mp.workdps(DPS):
        o = [mp.mpf(float(v)) for v in origin]
        a = [[mp.mpf(float(p[k])) - o[k] for p in A] for k in range(3)]
        b = [[mp.mpf(float(p[k])) - o[k] for p in B] for k in range(3)]
        m = [mp.mpf(len(A))] + [mp.fsum(a[k]) for k in range(3)] + [mp.fsum(b[k]) for k in range(3)]
        m += [mp.fdot(b[i], a[j]) for i in range(3) for j in range(3)]
        m += [mp.fsum(mp.fdot(a[k], a[k]) for k in range(3)), mp.fsum(mp.fdot(b[k], b[k]) for k in range(3))]
        return np.array([float(v) for v in m])


def kabsch_np(m, origin):
    """kabsch_from_moments restated with LAPACK's svd."""
    K, abar, bbar = m[0], m[1:4] / m[0], m[4:7] / m[0]
    H = m[7:16].reshape(3, 3) - K * np.outer(bbar, abar)
    U, _, Vt = np.linalg.svd(H)
    R = U @ Vt
    aw, bw = abar + origin, bbar + origin
    t = bw - R @ aw
    c2 = (m[17] - K * bbar @ bbar) + (m[16] - K * abar @ abar) - 2.0 * (R * H).sum()
    return R, t, np.sqrt(c2) if c2 > 0 else 0.0


def kabsch_mp(m, origin):
    """The same formulas in mpmath on the rounded moments -> dict of longdouble quantities (R, t, cost^2, sigma and the structural sizes)."""
    with mp.workdps(DPS):
        mm = [mp.mpf(float(v)) for v in m]
        o = mp.matrix([mp.mpf(float(v)) for v in origin])
        K = mm[0]
        abar, bbar = mp.matrix(mm[1:4]) / K, mp.matrix(mm[4:7]) / K
        Sba = mp.matrix(3, 3)
        for i in range(3):
            for j in range(3):
                Sba[i, j] = mm[7 + 3 * i + j]
        H = Sba - K * bbar * abar.T
        U, S, Vt = mp.svd_r(H)
        R = U * Vt
        aw, bw = abar + o, bbar + o
        t = bw - R * aw
        tr = mp.fsum(R[i, j] * H[i, j] for i in range(3) for j in range(3))
        c2 = (mm[17] - K * (bbar.T * bbar)[0]) + (mm[16] - K * (abar.T * abar)[0]) - 2 * tr
        sig = sorted((S[k] for k in range(3)), reverse=True)
        kappa = (mp.mnorm(Sba, "F") + K * mp.norm(bbar) * mp.norm(abar)) / mp.mnorm(H, "F")
        return {"R": _ld_matrix(R), "t": _ld_matrix(t)[:, 0], "c2": _ld(c2) if c2 > 0 else LD(0), "sigma": np.array([_ld(v) for v in sig], dtype=LD),
                "kappa": _ld(kappa), "aw": _ld_matrix(aw)[:, 0], "bw": _ld_matrix(bw)[:, 0],
                "cost_unit": _ld(mm[16] + mm[17] + 2 * mp.fsum(abs(v) for v in mm[7:16]))}


@functools.lru_cache(maxsize=None)
def kabsch_problems():
    """-> (Problems of op 3, family = kind; per row: A, B; the mpmath references)."""
    rng = np.random.default_rng(20243)
    P, sets, refs = Problems(), [], []
    for kind in KINDS:
        for K in KS:
            for _ in range(1 if K == 1000 else 2):
                A, B = _point_set(kind, K, rng)
                for where in ORIGINS:
                    origin = {"centroid": np.round(A.mean(axis=0), 2), "world": np.zeros(3),
                              "far": CENTRE + 1e3 * EXTENT * orth(rng)[0]}[where]
                    m = moments_mp(A, B, origin)
                    P.add(kind, np.concatenate([m, origin]))
                    sets.append((A, B))
                    refs.append(kabsch_mp(m, origin))
    return P.done(), sets, refs


@functools.lru_cache(maxsize=None)
def kabsch_warm_starts():
    """Op 4's V, one random orthogonal matrix per problem of kabsch_problems()."""
    rng = np.random.default_rng(20244)
    return np.array([orth(rng).reshape(-1) for _ in kabsch_problems()[0].inp])


def _on_points(R, t, A):
    return A @ R.T + t


def kabsch_metrics(R, t, cost, other=None):
    """R (n, 3, 3), t (n, 3), cost (n,) against the mpmath reference, each divided by its structural size (kappa = (|Sba| + K |bbar| |abar|)
    / |H| is the cancellation in H).  Where sigma_3 <= 1e-6 sigma_1 the rotation is not determined: `R` and `t` are NaN and `points`
    compares R a_i + t at the associated points instead.  other = (R', t'): compare with that result instead of the reference
    (`R`, `t`, `points` only)."""
    P, sets, refs = kabsch_problems()
    n = len(refs)
    out = {k: np.full(n, np.nan) for k in ("R", "t", "points", "cost", "orth")}
    for i, (ref, (A, _)) in enumerate(zip(refs, sets)):
        Ri, ti = R[i].astype(LD), t[i].astype(LD)
        R_ref, t_ref = (ref["R"], ref["t"]) if other is None else (other[0][i].astype(LD), other[1][i].astype(LD))
        s1, s2, s3 = ref["sigma"]
        naw, nbw = np.sqrt((ref["aw"] ** 2).sum()), np.sqrt((ref["bw"] ** 2).sum())
        if s3 > 1e-6 * s1:
            cond = ref["kappa"] * s1 / (s2 + s3)
            out["R"][i] = _fro(Ri - R_ref) / cond
            out["t"][i] = np.sqrt(((ti - t_ref) ** 2).sum()) / (naw * cond + naw + nbw)
        else:
            Al = A.astype(LD)
            ext = np.sqrt(((Al - ref["aw"]) ** 2).sum(axis=1)).max()
            s_r = s2 if s2 > 1e-6 * s1 else s1
            d = _on_points(Ri, ti, Al) - _on_points(R_ref, t_ref, Al)
            out["points"][i] = np.sqrt((d * d).sum(axis=1)).max() / (ref["kappa"] * ext * s1 / s_r + naw + nbw)
        if other is None:
            out["cost"][i] = abs(LD(cost[i]) ** 2 - ref["c2"]) / ref["cost_unit"]
            out["orth"][i] = np.abs(Ri.T @ Ri - I3).max()
    return out


def split_kabsch(out):
    return out[:, :9].reshape(-1, 3, 3), out[:, 9:12], out[:, 12]


def kabsch_evaluate(out):
    assert np.isfinite(out).all() and (out[:, 12] >= 0).all()
    return kabsch_metrics(*split_kabsch(out))


@functools.lru_cache(maxsize=None)
def kabsch_yardstick():
    P = kabsch_problems()[0]
    res = [kabsch_np(row[:18], row[18:21]) for row in P.inp]
    return kabsch_metrics(np.array([r[0] for r in res]), np.array([r[1] for r in res]), np.array([r[2] for r in res]))


def kabsch_warm_evaluate(run):
    """Op 4: run(inp) -> out.  First call with a random orthogonal V, second call fed with the V the first returned -> the metrics of
    the first call plus `orthV` (the returned V) and `again_R` / `again_points`: the second call's R against the first's."""
    P = kabsch_problems()[0]
    first = run(np.concatenate([P.inp, kabsch_warm_starts()], axis=1))
    assert np.isfinite(first).all()
    metrics = kabsch_evaluate(first[:, :13])
    V = first[:, 13:].reshape(-1, 3, 3).astype(LD)
    metrics["orthV"] = np.abs(np.einsum("nji,njk->nik", V, V) - I3).max(axis=(1, 2)).astype(np.float64)
    second = run(np.concatenate([P.inp, first[:, 13:]], axis=1))
    assert np.isfinite(second).all()
    R1, t1, _ = split_kabsch(first)
    R2, t2, _ = split_kabsch(second)
    again = kabsch_metrics(R2, t2, None, other=(R1, t1))
    metrics["again_R"], metrics["again_points"] = again["R"], again["points"]
    return metrics


KABSCH_BOUND_OF = {"again_R": "R", "again_points": "points", "orthV": "orth"}   # metric of op 4 -> the yardstick metric that bounds it


# -------------------------------------------------------------------------------------------------------- op 5: point2plane_solve
def p2p_system(n_corr, seed, equal_normals=None):
    """The systems of tests/test_point2plane_host.py: A = sum J J^T, b = sum J r over seeded correspondences, J = [s x n, n]."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-10.0, 10.0, (n_corr, 3))
    if equal_normals is None:
        n = rng.normal(size=(n_corr, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
    else:
        n = np.tile(np.asarray(equal_normals, dtype=np.float64), (n_corr, 1))
    r = rng.normal(scale=0.1, size=n_corr)
    J = np.concatenate([np.cross(s, n), n], axis=1)
    return J.T @ J, J.T @ r


@functools.lru_cache(maxsize=None)
def p2p_problems():
    """families: `random` (the host test's seeds and more), `cond1e8` (solvable), `singular` and `nonfinite` (refused)."""
    rng = np.random.default_rng(20245)
    P = Problems()
    pack = lambda A, b: np.concatenate([np.asarray(A)[np.triu_indices(6)], b])
    for seed in range(12):
        P.add("random", pack(*p2p_system(500, seed)))
    for _ in range(12):
        Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
        A = Q @ np.diag(np.logspace(0, -8, 6)) @ Q.T
        P.add("cond1e8", pack((A + A.T) / 2, rng.normal(size=6) * 1e-5))
    for normal in ((0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0)):
        P.add("singular", pack(*p2p_system(500, 7, equal_normals=normal)))
    P.add("singular", np.zeros(27))
    for bad, where in ((np.nan, (2, 2)), (np.inf, (0, 0)), (np.nan, (0, 5)), (-np.inf, (5, 5))):
        A, b = p2p_system(50, 3)
        A[where] = A[where[::-1]] = bad
        P.add("nonfinite", pack(A, b))
    A, b = p2p_system(50, 3)
    b[4] = np.nan
    P.add("nonfinite", pack(A, b))
    return P.done()


def full_sym6(tri):
    A = np.zeros((6, 6))
    iu = np.triu_indices(6)
    A[iu] = tri
    A[(iu[1], iu[0])] = tri
    return A


@functools.lru_cache(maxsize=None)
def p2p_reference():
    """-> list of (x_ref longdouble (6,), cond(A)) for the solvable families, None elsewhere."""
    P = p2p_problems()
    out = []
    with mp.workdps(DPS):
        for row, fam in zip(P.inp, P.family):
            if fam in ("singular", "nonfinite"):
                out.append(None)
                continue
            A = full_sym6(row[:21])
            x = mp.lu_solve(mp.matrix(A.tolist()), -mp.matrix(row[21:].tolist()))
            out.append((np.array([_ld(x[k]) for k in range(6)], dtype=LD), float(np.linalg.cond(A))))
    return out


def euler_mp(x):
    """Rz(x2) Ry(x1) Rx(x0) in mpmath -> longdouble (3, 3)."""
    with mp.workdps(DPS):
        a, b, g = (mp.mpf(float(v)) for v in x[:3])
        Rx = mp.matrix([[1, 0, 0], [0, mp.cos(a), -mp.sin(a)], [0, mp.sin(a), mp.cos(a)]])
        Ry = mp.matrix([[mp.cos(b), 0, mp.sin(b)], [0, 1, 0], [-mp.sin(b), 0, mp.cos(b)]])
        Rz = mp.matrix([[mp.cos(g), -mp.sin(g), 0], [mp.sin(g), mp.cos(g), 0], [0, 0, 1]])
        return _ld_matrix(Rz * Ry * Rx)


def euler_np(x):
    a, be, g = x[:3]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(be), 0, np.sin(be)], [0, 1, 0], [-np.sin(be), 0, np.cos(be)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def p2p_metrics(x, U):
    """x (n, 6), U (n, 4, 4) -> `x`: |x - x_ref| / (cond(A) |x_ref|); `U`: max |U[:3, :3] - Euler product of this x in mpmath| (NaN where
    the input is refused)."""
    out = {"x": np.full(len(x), np.nan), "U": np.full(len(x), np.nan)}
    for i, ref in enumerate(p2p_reference()):
        if ref is None:
            continue
        x_ref, cond = ref
        out["x"][i] = np.sqrt(((x[i].astype(LD) - x_ref) ** 2).sum()) / (cond * np.sqrt((x_ref**2).sum()))
        out["U"][i] = np.abs(U[i][:3, :3].astype(LD) - euler_mp(x[i])).max()
    return out


def p2p_evaluate(out):
    """Metrics of an op 5 result, after the exact parts: ok, the translation column and last row of U, and what a refused input returns."""
    P = p2p_problems()
    x, U, ok = out[:, :6], out[:, 6:22].reshape(-1, 4, 4), out[:, 22]
    refused = np.isin(P.family, ("singular", "nonfinite"))
    assert np.array_equal(ok, np.where(refused, 0.0, 1.0)), ok
    assert np.array_equal(x[refused], np.zeros((refused.sum(), 6))) and np.array_equal(U[refused], np.tile(np.eye(4), (refused.sum(), 1, 1)))
    assert np.isfinite(out[~refused]).all()
    assert np.array_equal(U[:, :3, 3], x[:, 3:]) and np.array_equal(U[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(U), 1)))
    return p2p_metrics(x, U)


@functools.lru_cache(maxsize=None)
def p2p_yardstick():
    P = p2p_problems()
    x, U = np.zeros((len(P.inp), 6)), np.tile(np.eye(4), (len(P.inp), 1, 1))
    for i, (row, ref) in enumerate(zip(P.inp, p2p_reference())):
        if ref is not None:
            x[i] = np.linalg.solve(full_sym6(row[:21]), -row[21:])
            U[i, :3, :3] = euler_np(x[i])
    return p2p_metrics(x, U)


# ------------------------------------------------------------------------------------------------------------------ bound rule
def worst(metrics, problems):
    """-> {(family, metric): worst value in the family, NaN where every problem is left out}."""
    out = {}
    for fam in problems.names:
        rows = problems.rows_of(fam)
        for name, v in metrics.items():
            v = v[rows]
            out[(fam, name)] = float(np.nanmax(v)) if np.isfinite(v).any() or np.isinf(v).any() else float("nan")
    return out


def bounds(yard, problems):
    """max(8 x the yardstick's worst value in the family, 1e-14)."""
    return {k: max(FACTOR * v, FLOOR) if v == v else FLOOR for k, v in worst(yard, problems).items()}


def left_out(metrics, problems, metric):
    """-> family -> share of problems the metric leaves out."""
    return {fam: float(np.isnan(metrics[metric][problems.rows_of(fam)]).mean()) for fam in problems.names}


def failures(metrics, problems, bound, bound_of=None):
    """Every (family, metric) whose worst value exceeds its bound -> list of strings (empty: all within), and the worst-value table."""
    bound_of = bound_of or {}
    w = worst(metrics, problems)
    bad = []
    for (fam, name), v in w.items():
        b = bound[(base(fam), bound_of.get(name, name))]
        if v == v and not v <= b:
            bad.append(f"{fam} {name}: {v:.3e} > {b:.3e}")
    return bad, w


def table(title, w, bound=None, bound_of=None):
    bound_of = bound_of or {}
    lines = [title]
    for (fam, name), v in w.items():
        b = "" if bound is None else f"   bound {bound[(base(fam), bound_of.get(name, name))]:.2e}"
        lines.append(f"  {fam:24s} {name:12s} {'left out' if v != v else f'{v:.2e}'}{b}")
    return "\n".join(lines)


class Op:
    """One op: its problems, its input rows, the evaluation of a result and the yardstick."""

    def __init__(self, op, problems, evaluate, yardstick, yard_problems=None, bound_of=None):
        self.op, self._problems, self.evaluate, self._yard, self._yard_problems, self.bound_of = op, problems, evaluate, yardstick, yard_problems, bound_of

    @property
    def problems(self):
        return self._problems()

    def bounds(self):
        return bounds(self._yard(), (self._yard_problems or self._problems)())


OPS = {
    0: Op(0, svd_problems, svd_evaluate, svd_yardstick),
    1: Op(1, lambda: svd_warm_problems()[0], lambda out: svd_evaluate(out, warm=True), svd_yardstick, svd_problems),
    2: Op(2, eig_problems, eig_evaluate, eig_yardstick),
    3: Op(3, lambda: kabsch_problems()[0], kabsch_evaluate, kabsch_yardstick),
    5: Op(5, p2p_problems, p2p_evaluate, p2p_yardstick),
}


def run_op(L, handle, op):
    """The op's families through the library -> (raw output, failures, worst table).  Op 4 makes two calls (kabsch_warm_evaluate)."""
    if op == 4:
        P = kabsch_problems()[0]
        raw = []

        def run(inp):
            raw.append(solve(L, handle, 4, inp))
            return raw[-1]
        metrics = kabsch_warm_evaluate(run)
        bad, w = failures(metrics, P, OPS[3].bounds(), KABSCH_BOUND_OF)
        return np.concatenate(raw), bad, w
    o = OPS[op]
    out = solve(L, handle, op, o.problems.inp)
    bad, w = failures(o.evaluate(out), o.problems, o.bounds(), o.bound_of)
    return out, bad, w


def raw_op(L, handle, op):
    """The bytes an op's families give, without evaluating them (op 4: both calls)."""
    inp, _ = inputs_of(op)
    out = solve(L, handle, op, inp)
    if op == 4:
        out = np.concatenate([out, solve(L, handle, 4, np.concatenate([inp[:, :21], out[:, 13:]], axis=1))])
    return out


def sample_rows(problems, k):
    """Up to k seeded rows of every family."""
    rng = np.random.default_rng(20247)
    rows = []
    for fam in problems.names:
        r = problems.rows_of(fam)
        rows += sorted(rng.choice(r, size=min(k, len(r)), replace=False).tolist())
    return rows


def inputs_of(op):
    """The rows an op is given (op 4: the first call's)."""
    if op == 4:
        return np.concatenate([kabsch_problems()[0].inp, kabsch_warm_starts()], axis=1), kabsch_problems()[0]
    return OPS[op].problems.inp, OPS[op].problems


# ------------------------------------------------------------------------------------------------- end-to-end sets for pcr_icp
def procrustes_mp(A, B):
    """main.py:131-141 in mpmath on the pairs (a_i, b_i) -> R, t (longdouble)."""
    with mp.workdps(DPS):
        a = [[mp.mpf(float(v)) for v in p] for p in A]
        b = [[mp.mpf(float(v)) for v in p] for p in B]
        K = len(a)
        abar = mp.matrix([mp.fsum(p[k] for p in a) / K for k in range(3)])
        bbar = mp.matrix([mp.fsum(p[k] for p in b) / K for k in range(3)])
        H = mp.matrix(3, 3)
        for i in range(3):
            for j in range(3):
                H[i, j] = mp.fsum((q[i] - bbar[i]) * (p[j] - abar[j]) for p, q in zip(a, b))
        U, S, Vt = mp.svd_r(H)
        R = U * Vt
        return _ld_matrix(R), _ld_matrix(bbar - R * abar)[:, 0], [float(S[k]) for k in range(3)]


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def association_sets():
    """name -> (source, target) float32, row i of the source belongs to row i of the target: targets 1 or more apart, every source point
    within 0.1 of its own.  Coordinates of the first two sets are multiples of 1/128, so that every moment is exact in binary64 and
    in the pass's fixed-point sums and the rank is what the construction says."""
    out = {}
    # collinear, K = 8: rank 1 (svd3_complete_two); the source line leans against the target's
    i = np.arange(8) - 3.5
    base_pt = np.array([2.0, -1.0, 0.5])
    tgt = base_pt + np.outer(i, [1.0, 2.0, 2.0])
    src = base_pt + np.array([1 / 128, 1 / 64, 0.0]) + np.outer(i, [1.0 + 1 / 64, 2.0, 2.0 - 1 / 128])
    out["collinear"] = (_f32(src), _f32(tgt))
    # coplanar, K = 16: a 4 x 4 lattice in the plane of (1, 1, 0) and (0, 1, 1); the source is sheared within the plane
    u, v = np.meshgrid(np.arange(4) - 1.5, np.arange(4) - 1.5, indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    e1, e2 = np.array([1.0, 1.0, 0.0]), np.array([0.0, 1.0, 1.0])
    tgt = base_pt + np.outer(u, e1) + np.outer(v, e2)
    src = base_pt + np.outer(u + v / 64 + 1 / 64, e1) + np.outer(v - u / 64 - 1 / 128, e2)
    out["coplanar"] = (_f32(src), _f32(tgt))
    # mirrored, K = 25: a 5 x 5 lattice of spacing 2 whose points sit 0.01 to 0.04 off its plane; the source is their mirror image in it
    rng = np.random.default_rng(20246)
    Q = orth(rng)
    g = np.stack(np.meshgrid(*[2.0 * (np.arange(k) - (k - 1) / 2) for k in (5, 5)], indexing="ij"), axis=-1).reshape(-1, 2)
    h = rng.uniform(0.01, 0.04, len(g)) * rng.choice([-1.0, 1.0], len(g))
    tgt = base_pt + (np.column_stack([g, h])) @ Q.T
    src = base_pt + (np.column_stack([g, -h])) @ Q.T
    out["mirrored"] = (_f32(src), _f32(tgt))
    # a cube's corners, K = 8: three equal singular values; the source is the cube turned by 0.03 rad
    corners = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    R0 = _rotation(rng, 0.03)
    out["cube"] = (_f32(base_pt + corners @ R0.T + [0.01, -0.02, 0.015]), _f32(base_pt + corners))
    for name, (s, t) in out.items():   # the nearest neighbour of every source point is its own target, by a margin
        d = np.linalg.norm(s[:, None, :].astype(np.float64) - t[None, :, :].astype(np.float64), axis=2)
        own = np.diag(d).copy()
        np.fill_diagonal(d, np.inf)
        assert 5 <= len(t) <= 64 and own.max() < 0.1 and d.min() > 0.9, name
        tt = t.astype(np.float64)
        dt = np.linalg.norm(tt[:, None] - tt[None], axis=2)
        np.fill_diagonal(dt, np.inf)
        assert dt.min() >= 1.0 and np.abs(tt).max() <= 10.0, name
    return out


def check_on_points(R, t, A, R_ref, t_ref, tag):
    """One Procrustes step of a route (R, t) on its pairs -> (max |R a_i + t - the 60-digit Procrustes| at the associated points, to be
    held to POINT_BAR; max |R^T R - I|, to be held to orth_bound)."""
    A = np.asarray(A, dtype=np.float64)
    Rl, tl, Al = np.asarray(R).astype(LD), np.asarray(t).reshape(3).astype(LD), A.astype(LD)
    err = float(np.abs(_on_points(Rl, tl, Al) - _on_points(R_ref, t_ref, Al)).max())
    orth_err = float(np.abs(Rl.T @ Rl - I3).max())
    assert np.isfinite(np.asarray(R)).all() and np.isfinite(np.asarray(t)).all(), tag
    return err, orth_err


POINT_BAR = 1e-9   # the project's tolerance for a transform acting on points of extent 10 or less


def orth_bound(A, B):
    """max(8 x LAPACK's max |R^T R - I| on these pairs, 1e-14)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    U, _, Vt = np.linalg.svd((B - B.mean(axis=0)).T @ (A - A.mean(axis=0)))
    R = (U @ Vt).astype(LD)
    return max(FACTOR * float(np.abs(R.T @ R - I3).max()), FLOOR)
