"""NumPy/SciPy float64 restatement of the point-to-point ICP LOOP with every field of pcr_icp_result, and the seeded scenes the loop
tests run it on (tests/test_icp_loop_host.py pins both on the CPU, tests/test_gpu_icp_loop.py holds every driver of the device loop
to them).

``icp_compat`` follows Registration/main.py:97-156, ``icp_total`` Registration/icp_template.py:128-200 filled in the way the product
fills it (paths relative to the reference).  Both take the parameters of pcr_icp_params (include/pcr.h):

* ``max_d2``: gate on the SQUARED distance, strict < (main.py:119); <= 0 or inf: no gate;
* ``r_metric``: "frobenius" (main.py:149) or "geodesic" (the link at icp_template.py:184): arccos((trace(R_last^T R) - 1) / 2);
* ``min_iter``: never break on the thresholds before this many solves (0: the reference's behaviour);
* ``T0``: main.py's ``transformation`` argument / the pose ransac_init returns (icp_template.py:145-152).

and return the fields of pcr_icp_result: T, T_total, iters, status (0 or TOO_FEW), n_assoc / mean_d2 (of the last association pass),
cost (of the last solve), R_diff[], t_diff[], passes (association passes run) and src_after (the source as the call leaves it).

Associations: cKDTree for the two nearest candidates, oracle.dist2_direct for the squared distance that ranks and gates them (as
oracle.nn1_exact); a row with a non-finite coordinate is never associated.  The solve is oracle.procrustes.  No library code.
"""
import functools
import zlib

import numpy as np
from scipy.spatial import cKDTree

from oracle import oracle_np as oracle

TOO_FEW = 1   # PCR_E_TOO_FEW_ASSOC (include/pcr.h)


def _cloud(a):
    return np.array(a, dtype=np.float64)[:, :3]


def _gated(max_d2):
    return max_d2 > 0 and np.isfinite(max_d2)


def _associate(tree, tgt, src, max_d2):
    """-> (rows of src that are associated, their target rows, their squared distances)."""
    ok = np.flatnonzero(np.isfinite(src).all(axis=1))
    k = 2 if len(tgt) > 1 else 1
    _, cand = tree.query(src[ok], k=k)
    cand = cand.reshape(len(ok), k)
    d2 = oracle.dist2_direct(src[ok][:, None, :], tgt[cand])
    best = np.argmin(d2, axis=1)   # (an exact tie goes to the first = nearer-by-cKDTree candidate: the scenes have none)
    j = cand[np.arange(len(ok)), best]
    d2 = d2[np.arange(len(ok)), best]
    keep = d2 < max_d2 if _gated(max_d2) else np.ones(len(ok), bool)
    return ok[keep], j[keep], d2[keep]


def _apply(T, pts):
    return pts @ T[:3, :3].T + T[:3, 3]


def _homo(R, t):
    T = np.zeros((4, 4))
    T[:3, :3] = R
    T[:3, 3] = np.asarray(t).reshape(3)
    T[3, 3] = 1.0
    return T


def _r_diff(R, R_last, r_metric):
    if r_metric == "geodesic":
        return float(np.arccos(np.clip((np.trace(R_last.T @ R) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(R - R_last))


def _result(T, T_total, iters, status, n_assoc, cost, mean_d2, r_log, t_log, passes, src):
    return {"T": T, "T_total": T_total, "iters": iters, "status": status, "n_assoc": n_assoc, "cost": cost, "mean_d2": mean_d2,
            "R_diff": np.array(r_log), "t_diff": np.array(t_log), "passes": passes, "src_after": src}


def icp_compat(src_pts, tgt_pts, T0=None, *, max_iter=100, r_thres=0.5, t_thres=0.5, max_d2=5.0, r_metric="frobenius", min_iter=0):
    """main.py:97-156.  T is the LAST increment (T0 itself while nothing was solved); T_total composes what was applied to the source."""
    src, tgt = _cloud(src_pts), _cloud(tgt_pts)
    T = np.eye(4) if T0 is None else np.array(T0, dtype=np.float64).reshape(4, 4)
    R_last, t_last = T[:3, :3], T[:3, 3]   # t_last has shape (3,): main.py:100
    tree = cKDTree(tgt)
    T_total = np.eye(4)
    iters = passes = n_assoc = status = 0
    cost = mean_d2 = 0.0
    r_log, t_log = [], []
    for _ in range(max_iter):
        src = _apply(T, src)             # main.py:110, in place
        T_total = T @ T_total
        rows, j, d2 = _associate(tree, tgt, src, max_d2)   # main.py:116-121
        passes += 1
        n_assoc = len(rows)
        mean_d2 = float(d2.mean()) if n_assoc else 0.0
        if n_assoc < 3:                  # main.py:125-127
            status = TOO_FEW
            break
        R, t, cost = oracle.procrustes(src[rows].T, tgt[j].T)   # main.py:131-141
        cost = float(cost)
        T = _homo(R, t)                  # main.py:143-146
        iters += 1
        r_log.append(_r_diff(R, R_last, r_metric))
        t_log.append(float(np.linalg.norm(t - t_last)))   # the first time (3,1) - (3,) -> 3 x 3: main.py:150
        R_last, t_last = R, t
        if r_log[-1] <= r_thres and t_log[-1] <= t_thres and iters >= min_iter:   # main.py:153
            break
    return _result(T, T_total, iters, status, n_assoc, cost, mean_d2, r_log, t_log, passes, src)


def icp_total(src_pts, tgt_pts, T0=None, *, max_iter=50, r_thres=1e-5, t_thres=1e-5, max_d2=5.0, r_metric="geodesic", min_iter=0):
    """icp_template.py:128-200.  T = T_total = homo_mat_total."""
    src, tgt = _cloud(src_pts), _cloud(tgt_pts)
    T_init = np.eye(4) if T0 is None else np.array(T0, dtype=np.float64).reshape(4, 4)
    homo = T_init.copy()                 # icp_template.py:150
    src = _apply(T_init, src)            # icp_template.py:152
    R_last, t_last = T_init[:3, :3], T_init[:3, 3:4]   # icp_template.py:148
    tree = cKDTree(tgt)
    iters = passes = n_assoc = status = 0
    cost = mean_d2 = 0.0
    r_log, t_log = [], []
    for _ in range(max_iter):
        rows, j, d2 = _associate(tree, tgt, src, max_d2)   # icp_template.py:168
        passes += 1
        n_assoc = len(rows)
        mean_d2 = float(d2.mean()) if n_assoc else 0.0
        if n_assoc < 3:                  # icp_template.py:169-171
            status = TOO_FEW
            break
        R, t, cost = oracle.procrustes(src[rows].T, tgt[j].T)   # icp_template.py:178
        cost = float(cost)
        iters += 1
        r_log.append(_r_diff(R, R_last, r_metric))
        t_log.append(float(np.linalg.norm(t - t_last)))
        R_last, t_last = R, t
        if r_log[-1] <= r_thres and t_log[-1] <= t_thres and iters >= min_iter:   # icp_template.py:192-193
            break
        src = _apply(_homo(R, t), src)   # icp_template.py:195-196: also after the last iteration
        homo = _homo(R, t) @ homo        # icp_template.py:197-198
    return _result(homo, homo.copy(), iters, status, n_assoc, cost, mean_d2, r_log, t_log, passes, src)


def restate(mode, src, tgt, T0=None, **kw):
    return (icp_compat if mode == "compat" else icp_total)(src, tgt, T0, **kw)


# ------------------------------------------------------------------------------------------------------------------ scenes
# Every cloud is float32 (what the batch entry point takes; the per-pair entry points widen it exactly), so that all drivers and the
# restatement see the same numbers.  Random coordinates: no two candidate distances tie.
MODES = ("compat", "total")
METRICS = ("frobenius", "geodesic")
SIZES = (3, 4, 63, 64, 65, 257, 1025, 3000)   # 64-query tile, 256-query block, 1024-query accumulate block
GATE = 0.01                                   # squared: 0.1 of a cloud of unit scale whose points are ~0.14 apart; the first passes leave 7 % and 1 % of the main scene outside


def rigid(rotvec, t):
    """4x4 from a rotation vector (Rodrigues) and a translation."""
    w = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.zeros((3, 3))
    if th > 0:
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def target(n=3000, seed=1):
    return _frozen(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)))


@functools.lru_cache(maxsize=None)
def source(n, seed=2, rot=0.05, shift=0.08, noise=0.002, n_tgt=3000):
    """n target points (the first n of a seeded permutation), rigidly perturbed, plus noise."""
    tgt = target(n_tgt).astype(np.float64)
    rng = np.random.default_rng(1000 * seed + n)
    rows = rng.permutation(len(tgt))[:n]
    axis = rng.normal(size=3)
    T = rigid(rot * axis / np.linalg.norm(axis), shift * rng.normal(size=3) / np.sqrt(3.0))
    return _frozen(_apply(T, tgt[rows]) + rng.normal(0.0, noise, (n, 3)))


T0_MOVED = rigid((0.02, -0.03, 0.025), (0.03, -0.02, 0.04))   # edge 6: rotation + translation


OFF = dict(r_thres=-1.0, t_thres=-1.0)   # thresholds off: only max_iter (or too few associations) stops the loop


# edge 2: the scene (seed of source(3000, seed)) whose free run converges at log entry j for every mode and metric -- entry j is at most
# half of entry j - 1 in both logs, no earlier entry is under both thresholds, and both entries are >= 1e-4: two orders above where
# the rounding of acos shows (4e-16 / angle).
# Entries 1 | 2: last pass of the first chunk of passes | first of the second; 6 | 7: first and second pass of the third chunk.
CONVERGE_SEED = {1: 5, 2: 6, 3: 3, 6: 7, 7: 230}
STOP_SHOWS = (1, 2, 3, 7)   # entries whose pending increment still moves the source by > 1e-5: a pass that ran behind the stop shows there
                            # (entry 6's scene stops on its fixed point -- the pending increment is the identity; none better in 260 seeds)


def converges_at(log, j, floor=1e-4):
    """The condition CONVERGE_SEED states, for one free run."""
    R, t = log["R_diff"], log["t_diff"]
    if len(R) <= j or min(R[j], t[j]) < floor or R[j - 1] < 2 * R[j] or t[j - 1] < 2 * t[j]:
        return False
    r_thres, t_thres = np.sqrt(R[j - 1] * R[j]), np.sqrt(t[j - 1] * t[j])
    return not any(R[i] <= r_thres and t[i] <= t_thres for i in range(j))


def thresholds(log, j):
    return float(np.sqrt(log["R_diff"][j - 1] * log["R_diff"][j])), float(np.sqrt(log["t_diff"][j - 1] * log["t_diff"][j]))


# edge 5: eight source points, five of them just inside the gate of target(): the first solve leaves two (found by a seeded search
# with the restatement; every squared distance is at least 0.7 % away from the gate in both passes)
TOO_FEW_GATE = 0.004
TOO_FEW_SRC = _frozen([
    [0.5391313433647156, -0.7416427135467529, 0.6470307111740112], [1.7564046382904053, 1.7757872343063354, 1.9752471446990967],
    [-0.4883674085140228, -0.8328896760940552, -0.3672535717487335], [1.5351951122283936, 1.7441951036453247, 1.5780105590820312],
    [-0.5974694490432739, -0.7188912034034729, -0.04879523068666458], [-0.6596731543540955, 0.6269918084144592, 0.09233662486076355],
    [0.17881980538368225, -0.8055965304374695, 0.4012390077114105], [1.5423654317855835, 1.653470516204834, 1.8405224084854126]])


def nearest_d2(src, tgt):
    """Ungated squared nearest-neighbour distance of every finite row."""
    tgt = _cloud(tgt)
    return _associate(cKDTree(tgt), tgt, _cloud(src), np.inf)[2]


@functools.lru_cache(maxsize=None)
def far_source(n=257, n_far=9):
    """edge 7: source(n) with its last rows thrown 40-60 units outside the target's box."""
    s = np.array(source(n))
    rng = np.random.default_rng(77)
    s[-n_far:] = rng.uniform(40.0, 60.0, (n_far, 3)) * rng.choice([-1.0, 1.0], (n_far, 3))
    return _frozen(s)


@functools.lru_cache(maxsize=None)
def nan_source(n=65, row=17, col=1):
    s = np.array(source(n))
    s[row, col] = np.nan
    return _frozen(s)


# ---------------------------------------------------------------------------------- range of the fixed-point accumulators
def fraction_bits(tgt, nq, max_d2):
    """DESIGN section 3.1.5 restated: every moment is bounded by M = nq * max(R^2, gate, 1), R = half diagonal of the target's box +
    gate radius; totals stay below 2^61 and one correspondence's moments below 2^51: F = min(61 - ex(M), 51 - ex(M / nq)) fraction
    bits, ex(v) the exponent with v < 2^ex.  The pass keeps its fixed-point accumulators iff F >= 20."""
    import math
    t = _cloud(tgt)
    half = 0.5 * (t.max(axis=0) - t.min(axis=0))
    R = math.sqrt(float((half * half).sum())) + math.sqrt(max_d2)
    M = nq * max(R * R, max_d2, 1.0)
    return min(61 - math.frexp(M)[1], 51 - math.frexp(M / nq)[1])


def first_moment_rounding(F, nq):
    """What rounding every coordinate sum to the common grid 2^-F per correspondence does to t = mean(b) - R mean(a): a uniform error
    of 2^-(F+1) / sqrt(3) rms per term, sqrt(nq) of them, divided by nq.  Where this exceeds 1e-11 the pass keeps the first moments on a
    finer grid of their own (pcr_pass_fixed_scale)."""
    return 2.0 ** -(F + 1) / np.sqrt(3.0 * nq)


BIG_NQ = 1000
BIG_SCENES = ((20, 1000), (19, 1000), (25, 1000), (26, 65))   # (F, source points): the limit from both sides; more bits; more bits and few points


@functools.lru_cache(maxsize=None)
def big_scene(F, nq=BIG_NQ):
    """The unit scene blown up so that the rule above gives F: R^2 = 0.9 * 2^(51 - F), and 1.1 * 2^31 for F = 19 (just past F = 20's
    0.9 * 2^31: half diagonals of 44 and 48 km).  The target fills its box.  -> (source (nq), target (3000), gate)."""
    R2 = 1.1 * 2.0 ** 31 if F == 19 else 0.9 * 2.0 ** (51 - F)
    h = np.sqrt(R2) / (np.sqrt(3.0) + np.sqrt(GATE))   # R = h sqrt(3) + h sqrt(GATE)
    return _frozen(source(nq, seed=7).astype(np.float64) * h), _frozen(target().astype(np.float64) * h), float(GATE * h * h)


BIG_CONVERGE = (1, 3)   # log entries at which the free runs of the two 1 000-point scenes at the limit converge (converges_at), every mode and metric


def ulp_perturbed(a, rng):
    """Every coordinate moved by one binary64 ulp, up or down at random."""
    a = np.asarray(a, dtype=np.float64)
    return np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))


# ------------------------------------------------------------------------------------------------------------------ edges
class Case:
    """One edge: clouds, T0 and the loop parameters (a dict, or a function (mode, r_metric) -> dict where the thresholds come from
    the restatement's own logs).  planar: K == 3, the rotation's null direction is free -- only what acts on the associated points
    is compared.  fused_batch: the batch entry point keeps the pair in its fused stages (gated, finite clouds)."""

    def __init__(self, name, src, kw, tgt=None, T0=None, planar=False, fused_batch=True, profiled=False, finite=True):
        self.name, self.src, self.tgt, self.T0, self._kw = name, src, target() if tgt is None else tgt, T0, kw
        self.planar, self.fused_batch, self.profiled, self.finite = planar, fused_batch and finite, profiled, finite
        self._memo = {}

    def kw(self, mode, r_metric):
        return dict(self._kw(mode, r_metric) if callable(self._kw) else self._kw)

    def restated(self, mode, r_metric):
        key = (mode, r_metric)
        if key not in self._memo:
            r = restate(mode, self.src, self.tgt, self.T0, r_metric=r_metric, **self.kw(mode, r_metric))
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._memo[key] = r
        return self._memo[key]

    def __repr__(self):
        return self.name


def _free(src, n_iter, gate=GATE, tgt=None):
    """(mode, r_metric) -> the run with the thresholds off, shared by the cases that take their thresholds from it."""
    memo = {}

    def run(mode, r_metric):
        if (mode, r_metric) not in memo:
            memo[(mode, r_metric)] = restate(mode, src, target() if tgt is None else tgt, None, r_metric=r_metric, max_iter=n_iter, max_d2=gate, **OFF)
        return memo[(mode, r_metric)]
    return run


def _converging(free, j, gate=GATE, **more):
    def kw(mode, r_metric):
        r_thres, t_thres = thresholds(free(mode, r_metric), j)
        return dict(max_iter=15, max_d2=gate, r_thres=r_thres, t_thres=t_thres, **more)
    return kw


FREE = {j: _free(source(3000, seed=s), 10) for j, s in CONVERGE_SEED.items()}
FAR_T0 = rigid((0.0, 0.0, 0.0), (10.0, 0.0, 0.0))


def _k2_source():
    s = np.array(source(3))
    s[2] += 5.0
    return _frozen(s)


def _cases():
    out = []
    for m in (0, 1, 2, 3, 4, 5, 6, 7, 14, 15):   # edge 1: either side of the chunk ends 2, 6 and 14
        out.append(Case(f"max_iter_{m}", source(3000), dict(max_iter=m, max_d2=GATE, **OFF), profiled=m in (0, 1, 3, 7)))
    for j, seed in CONVERGE_SEED.items():        # edge 2
        out.append(Case(f"converges_at_{j}", source(3000, seed=seed), _converging(FREE[j], j), profiled=j in (2, 6)))
    # edge 3: the scene of entry 2 converges with its third solve
    s2, s3 = source(3000, seed=CONVERGE_SEED[2]), source(3000, seed=CONVERGE_SEED[3])
    out.append(Case("min_iter_above_convergence", s2, _converging(FREE[2], 2, min_iter=5), profiled=True))
    out.append(Case("min_iter_at_convergence", s2, _converging(FREE[2], 2, min_iter=3)))
    out.append(Case("min_iter_above_max_iter", s2, lambda mode, r_metric: dict(_converging(FREE[2], 2, min_iter=6)(mode, r_metric), max_iter=4)))
    out.append(Case("min_iter_3_first_chunk", s3, _converging(FREE[3], 3, min_iter=3)))
    # edge 4
    out.append(Case("log_filled_to_256", source(65), dict(max_iter=256, min_iter=256, max_d2=GATE, **OFF)))
    # edge 5
    out.append(Case("too_few_at_pass_0", source(257), dict(max_iter=5, max_d2=GATE, **OFF), T0=FAR_T0))
    out.append(Case("too_few_at_pass_1", TOO_FEW_SRC, dict(max_iter=10, max_d2=TOO_FEW_GATE, **OFF), profiled=True))
    out.append(Case("k_is_3", source(3), dict(max_iter=1, max_d2=GATE, **OFF), planar=True))
    out.append(Case("k_is_2", _k2_source(), dict(max_iter=5, max_d2=GATE, **OFF)))
    out.append(Case("nan_coordinate", nan_source(), dict(max_iter=4, max_d2=GATE, **OFF), finite=False))
    # edge 6
    out.append(Case("T0_rotation_and_translation", source(3000), dict(max_iter=5, max_d2=GATE, **OFF), T0=T0_MOVED, profiled=True))
    # edge 7
    out.append(Case("ungated_zero", far_source(), dict(max_iter=4, max_d2=0.0, **OFF), fused_batch=False))
    out.append(Case("ungated_inf", far_source(), dict(max_iter=4, max_d2=float("inf"), **OFF), fused_batch=False))
    # edge 8
    for n in SIZES[:-1]:
        out.append(Case(f"size_{n}", source(n), dict(max_iter=4, max_d2=GATE, **OFF), planar=n == 3))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}


def _big_cases():
    out = {}
    for F, nq in BIG_SCENES:
        s, t, gate = big_scene(F, nq)
        free = _free(s, 10, gate, t)
        cs = [Case(f"F{F}_n{nq}_max_iter_{m}", s, dict(max_iter=m, max_d2=gate, **OFF), tgt=t) for m in (0, 2, 3, 7)]
        if nq == BIG_NQ and F in (19, 20):   # edge 2 on the two scenes at the limit
            cs += [Case(f"F{F}_n{nq}_converges_at_{j}", s, _converging(free, j, gate), tgt=t) for j in BIG_CONVERGE]
        for c in cs:
            c.free = free
        out[(F, nq)] = cs
    return out


BIG_CASES = _big_cases()


def sensitivity(case, mode, r_metric):
    """s of the issue, per field: the largest |restated(perturbed clouds) - restated| over four runs in which every coordinate of both
    clouds is moved by one binary64 ulp at random -> dict field -> s."""
    base = case.restated(mode, r_metric)
    rng = np.random.default_rng(zlib.crc32(f"{case.name} {mode} {r_metric}".encode()))
    out = {k: 0.0 for k in ("T", "T_total", "src_after", "R_diff", "t_diff")}
    for _ in range(4):
        r = restate(mode, ulp_perturbed(case.src, rng), ulp_perturbed(case.tgt, rng), case.T0, r_metric=r_metric, **case.kw(mode, r_metric))
        assert (r["iters"], r["passes"], r["n_assoc"], r["status"]) == (base["iters"], base["passes"], base["n_assoc"], base["status"])
        for k in out:
            if np.size(base[k]):
                out[k] = max(out[k], float(np.abs(np.asarray(r[k]) - np.asarray(base[k])).max()))
    return out
