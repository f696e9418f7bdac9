"""Pins tests/icp_loop_checks.py on the CPU: the restated loop against the reference's goldens and the oracle, the three rules a loop
gets wrong written out once more by hand, and every scene of tests/test_gpu_icp_loop.py against the condition it was chosen for -- a
scene that loses its condition fails here, not silently on the GPU."""
import numpy as np
import pytest

from tests import icp_loop_checks as K
from tests.conftest import load_golden

ALL = [(m, r) for m in K.MODES for r in K.METRICS]


def test_compat_reproduces_the_reference_goldens():
    """Default parameters = Registration/main.py:98-103; the bars of test_icp_compat_matches_reference_goldens."""
    g = load_golden("icp_compat.npz")
    for tag in map(str, g["cases"]):
        r = K.icp_compat(g[f"{tag}_src"], g[f"{tag}_tgt"], g[f"{tag}_T0"])
        assert r["iters"] == int(g[f"{tag}_iters"][0]), tag
        assert np.linalg.norm(r["T"] - g[f"{tag}_T"]) < 1e-9, tag
        assert np.abs(r["src_after"] - g[f"{tag}_src_after"]).max() < 1e-9, tag
        assert (r["status"] == K.TOO_FEW) == bool(int(g[f"{tag}_failed"][0])), tag


@pytest.mark.parametrize("T0", [None, K.T0_MOVED], ids=["identity", "moved"])
def test_restatement_equals_the_oracle_where_parameters_overlap(oracle, T0):
    src, tgt = K.source(1025), K.target()
    eye = np.eye(4) if T0 is None else T0
    for gate, r_thres, t_thres, n in ((K.GATE, 1e-3, 1e-3, 30), (K.GATE, 0.5, 0.5, 100), (5.0, -1.0, -1.0, 3)):
        o = oracle.icp_point2point(src, tgt, eye, max_iteration=n, R_diff_thres=r_thres, t_diff_thres=t_thres, dist_thres=gate)
        r = K.icp_compat(src, tgt, eye, max_iter=n, r_thres=r_thres, t_thres=t_thres, max_d2=gate)
        assert r["iters"] == o["iters"] and (r["status"] == K.TOO_FEW) == o["failed"]
        for f in ("T", "T_total", "src_after"):
            assert np.abs(r[f] - o[f]).max() < 1e-12, f
        for geodesic in (True, False):
            homo, log = oracle.icp_total(src, tgt, T0, max_iteration=n, R_diff_thres=r_thres, t_diff_thres=t_thres, dist_thres=gate, geodesic=geodesic)
            r = K.icp_total(src, tgt, T0, max_iter=n, r_thres=r_thres, t_thres=t_thres, max_d2=gate, r_metric="geodesic" if geodesic else "frobenius")
            assert r["iters"] == len(log["R_diff"]) and np.abs(r["T"] - homo).max() < 1e-12 and np.array_equal(r["T"], r["T_total"])
            assert np.allclose(r["R_diff"], log["R_diff"], rtol=0, atol=1e-12) and np.allclose(r["t_diff"], log["t_diff"], rtol=0, atol=1e-12)


def test_compat_first_t_diff_is_the_3x3_broadcast():
    """main.py:100,150: t_last is (3,) the first time, so t - t_last is 3 x 3; later it is (3,1) - (3,1)."""
    src, tgt, T0 = K.source(257), K.target(), K.T0_MOVED
    r = K.icp_compat(src, tgt, T0, max_iter=2, max_d2=K.GATE, **K.OFF)
    one = K.icp_compat(src, tgt, T0, max_iter=1, max_d2=K.GATE, **K.OFF)
    t1, t0 = one["T"][:3, 3], T0[:3, 3]
    quirk = np.sqrt(sum((t1[i] - t0[j]) ** 2 for i in range(3) for j in range(3)))
    plain = np.linalg.norm(t1 - t0)
    assert abs(quirk - plain) > 1e-3                      # the scene tells the two apart
    assert abs(r["t_diff"][0] - quirk) < 1e-14
    assert abs(r["t_diff"][1] - np.linalg.norm(r["T"][:3, 3] - t1)) < 1e-14
    assert abs(K.icp_total(src, tgt, T0, max_iter=1, max_d2=K.GATE, **K.OFF)["t_diff"][0] - plain) < 1e-14   # the template has (3,1) from the start


def test_total_updates_source_and_total_after_a_last_iteration_that_did_not_converge():
    """icp_template.py:192-198: the update sits in the else of the convergence test, not behind a test for the last iteration."""
    src, tgt, T0 = K.source(257), K.target(), K.T0_MOVED
    for n in (1, 3):
        c = K.icp_compat(src, tgt, T0, max_iter=n, max_d2=K.GATE, **K.OFF)      # applied T0 and n - 1 increments; T = the n-th
        t = K.icp_total(src, tgt, T0, max_iter=n, max_d2=K.GATE, **K.OFF)
        assert t["iters"] == n and np.abs(t["T_total"] - c["T"] @ c["T_total"]).max() < 1e-14
        assert np.abs(t["src_after"] - K._apply(c["T"], c["src_after"])).max() < 1e-14
        assert np.abs(t["src_after"] - c["src_after"]).max() > 1e-4         # the scene tells the two apart
        # converged at its last iteration: no update (thresholds wide open)
        t = K.icp_total(src, tgt, T0, max_iter=n, max_d2=K.GATE, r_thres=10.0, t_thres=10.0)
        assert t["iters"] == 1 and np.array_equal(t["T_total"], T0) and np.array_equal(t["src_after"], K._apply(T0, src.astype(np.float64)))
    for mode in K.MODES:   # no iteration at all: main.py returns its argument and has not touched the source, the template has applied the initial pose
        r = K.restate(mode, src, tgt, T0, max_iter=0, max_d2=K.GATE)
        assert r["iters"] == r["passes"] == 0 and np.array_equal(r["T"], T0)
        assert np.array_equal(r["T_total"], np.eye(4) if mode == "compat" else T0)
        assert np.array_equal(r["src_after"], src.astype(np.float64) if mode == "compat" else K._apply(T0, src.astype(np.float64)))


@pytest.mark.parametrize("mode", K.MODES)
def test_min_iter_never_breaks_before_that_many_solves(mode):
    src, tgt = K.source(257), K.target()
    wide = dict(max_d2=K.GATE, r_thres=10.0, t_thres=10.0)
    assert K.restate(mode, src, tgt, max_iter=9, **wide)["iters"] == 1
    for min_iter, max_iter, want in ((1, 9, 1), (4, 9, 4), (9, 9, 9), (12, 9, 9)):
        r = K.restate(mode, src, tgt, max_iter=max_iter, min_iter=min_iter, **wide)
        assert r["iters"] == r["passes"] == want == len(r["R_diff"])
    if mode == "total":   # stopped by max_iter below min_iter: not converged, the last update is applied
        a = K.icp_total(src, tgt, max_iter=3, min_iter=5, **wide)
        b = K.icp_total(src, tgt, max_iter=3, max_d2=K.GATE, **K.OFF)
        assert np.array_equal(a["T_total"], b["T_total"]) and np.array_equal(a["src_after"], b["src_after"])


# --------------------------------------------------------------------------------------------------- the scenes' conditions
def test_catalogue_covers_the_sizes_and_edges():
    names = set(K.CASE)
    assert {f"max_iter_{m}" for m in (0, 1, 2, 3, 4, 5, 6, 7, 14, 15)} <= names
    assert {f"converges_at_{j}" for j in (1, 2, 3, 6, 7)} <= names
    assert {f"size_{n}" for n in (3, 4, 63, 64, 65, 257, 1025)} <= names and len(K.CASE["max_iter_4"].src) == 3000
    assert len(names) == len(K.CASES)
    for c in K.CASES + [c for cs in K.BIG_CASES.values() for c in cs]:
        assert c.src.dtype == np.float32 and c.tgt.dtype == np.float32 and 2000 <= len(c.tgt) <= 4000 and len(c.src) <= 3000


@pytest.mark.parametrize("mode,r_metric", ALL)
def test_threshold_free_scenes_run_to_max_iter(mode, r_metric):
    for c in K.CASES:
        kw = c.kw(mode, r_metric)
        if kw["r_thres"] >= 0 or c.name.startswith(("too_few", "k_is_2")):
            continue
        r = c.restated(mode, r_metric)
        assert r["status"] == 0 and r["iters"] == r["passes"] == kw["max_iter"], c
        assert kw["max_iter"] == 0 or r["n_assoc"] >= (3 if c.planar else 4), c
    # the gate bites in the main scene: the first passes leave points outside, later ones none
    n = [K.CASE[f"max_iter_{m}"].restated(mode, r_metric)["n_assoc"] for m in (1, 2, 3)]
    assert n[0] < n[1] < n[2] == 3000 and n[0] > 2000


@pytest.mark.parametrize("mode,r_metric", ALL)
def test_converging_scenes_converge_where_they_say(mode, r_metric):
    for j in K.CONVERGE_SEED:
        c = K.CASE[f"converges_at_{j}"]
        free = K.FREE[j](mode, r_metric)
        assert K.converges_at(free, j), (c, "successive log entries must differ by a factor >= 2 around the threshold, none earlier under both")
        r = c.restated(mode, r_metric)
        assert r["status"] == 0 and r["iters"] == r["passes"] == j + 1 < c.kw(mode, r_metric)["max_iter"], c
        # it stopped on the thresholds: the source is where the free run had it at that point, in TOTAL mode without the last update
        assert np.array_equal(r["R_diff"], free["R_diff"][: j + 1])
        # a pass that ran behind the stop would apply the pending increment once more: that must show in the source
        if j not in K.STOP_SHOWS:
            continue
        if mode == "compat":
            assert np.abs(K._apply(r["T"], r["src_after"]) - r["src_after"]).max() > 1e-5, c
        else:
            last = K.restate("compat", c.src, c.tgt, r_metric=r_metric, **c.kw(mode, r_metric))["T"]
            assert np.abs(K._apply(last, r["src_after"]) - r["src_after"]).max() > 1e-5, c
    for cases in K.BIG_CASES.values():
        for c in cases:
            if "converges_at" in c.name:
                j = int(c.name.rsplit("_", 1)[1])
                assert K.converges_at(c.free(mode, r_metric), j), c
                assert c.restated(mode, r_metric)["iters"] == j + 1, c


@pytest.mark.parametrize("mode,r_metric", ALL)
def test_min_iter_scenes(mode, r_metric):
    r = K.CASE["converges_at_2"].restated(mode, r_metric)
    assert r["iters"] == 3
    above = K.CASE["min_iter_above_convergence"].restated(mode, r_metric)
    assert above["iters"] >= 5 > r["iters"] and above["iters"] < 15 and above["status"] == 0
    assert K.CASE["min_iter_at_convergence"].restated(mode, r_metric)["iters"] == 3
    beyond = K.CASE["min_iter_above_max_iter"]
    assert beyond.kw(mode, r_metric)["min_iter"] > beyond.kw(mode, r_metric)["max_iter"] == beyond.restated(mode, r_metric)["iters"] == 4
    # under the thresholds at its third solve, yet not stopped: in TOTAL mode the fourth increment is applied as well
    assert beyond.restated(mode, r_metric)["R_diff"][2] <= beyond.kw(mode, r_metric)["r_thres"]
    first3 = K.CASE["min_iter_3_first_chunk"]
    assert first3.kw(mode, r_metric)["min_iter"] == 3 and first3.restated(mode, r_metric)["iters"] == 4


@pytest.mark.parametrize("mode,r_metric", ALL)
def test_too_few_scenes(mode, r_metric):
    r = K.CASE["too_few_at_pass_0"].restated(mode, r_metric)
    assert (r["status"], r["iters"], r["passes"], r["n_assoc"]) == (K.TOO_FEW, 0, 1, 0)
    assert np.array_equal(r["T"], K.FAR_T0) and np.array_equal(r["T_total"], K.FAR_T0)
    assert K.nearest_d2(r["src_after"], K.target()).min() > 100 * K.GATE       # everything far beyond the gate
    c = K.CASE["too_few_at_pass_1"]
    assert len(c.src) <= 8
    r = c.restated(mode, r_metric)
    assert (r["status"], r["iters"], r["passes"], r["n_assoc"]) == (K.TOO_FEW, 1, 2, 2)     # stops with too few associations at pass 1
    first = K.restate(mode, c.src, c.tgt, max_iter=1, r_metric=r_metric, max_d2=K.TOO_FEW_GATE, **K.OFF)
    assert first["n_assoc"] == 5 and first["status"] == 0                                # ... after a solve over five: no null direction
    d2 = [K.nearest_d2(c.src, c.tgt), K.nearest_d2(r["src_after"], c.tgt)]
    assert min(np.abs(d / K.TOO_FEW_GATE - 1.0).min() for d in d2) > 5e-3               # nobody sits on the gate
    r = K.CASE["k_is_3"].restated(mode, r_metric)
    assert (r["status"], r["iters"], r["n_assoc"]) == (0, 1, 3)
    r = K.CASE["k_is_2"].restated(mode, r_metric)
    assert (r["status"], r["iters"], r["passes"], r["n_assoc"]) == (K.TOO_FEW, 0, 1, 2)
    c = K.CASE["nan_coordinate"]
    bad = ~np.isfinite(c.src).all(axis=1)
    assert bad.sum() == 1 and np.isnan(c.src).sum() == 1
    r = c.restated(mode, r_metric)
    assert r["n_assoc"] == len(c.src) - 1 and r["status"] == 0 and np.isfinite(r["T"]).all()
    assert np.isnan(r["src_after"][bad]).all() and np.isfinite(r["src_after"][~bad]).all()


@pytest.mark.parametrize("mode,r_metric", ALL)
def test_ungated_scenes_reach_far_outside_the_target_box(mode, r_metric):
    a, b = K.CASE["ungated_zero"].restated(mode, r_metric), K.CASE["ungated_inf"].restated(mode, r_metric)
    src = K.far_source()
    assert (np.abs(src).max(axis=1) > 30).sum() == 9 and np.abs(K.target()).max() <= 1.0
    assert a["n_assoc"] == b["n_assoc"] == len(src) and np.array_equal(a["T_total"], b["T_total"])
    gated = K.restate(mode, src, K.target(), max_iter=4, r_metric=r_metric, max_d2=K.GATE, **K.OFF)
    assert gated["n_assoc"] <= len(src) - 9 and np.abs(gated["T_total"] - a["T_total"]).max() > 1e-3   # the gate matters here


def test_big_scenes_sit_on_either_side_of_the_fraction_bit_limit():
    assert set(K.BIG_CASES) == {(20, 1000), (19, 1000), (25, 1000), (26, 65)}
    for (F, nq), cases in K.BIG_CASES.items():
        c = cases[0]
        gate = c.kw("total", "frobenius")["max_d2"]
        assert K.fraction_bits(c.tgt, len(c.src), gate) == F and len(c.src) == nq
        assert sum("converges_at" in x.name for x in cases) == (2 if F in (19, 20) else 0)
        # the clouds fill their box: every octant of the target's box holds an eighth of it, give or take
        t = c.tgt.astype(np.float64)
        octant = ((t > 0.5 * (t.min(0) + t.max(0))) * np.array([1, 2, 4])).sum(axis=1)
        assert np.bincount(octant, minlength=8).min() > len(t) / 12
        half_diag = 0.5 * np.linalg.norm(t.max(0) - t.min(0))
        assert (40e3 < half_diag < 50e3) if F in (19, 20) else (5e3 < half_diag < 10e3)
        # on the common grid the coordinate sums alone would cost t this much: at or above the bar's order in every scene
        assert K.first_moment_rounding(F, nq) > 1e-10
    # ... and in clouds of ordinary extent nothing: 120 000 points in a scan's box leave 31 bits, the unit scenes over 40
    assert K.first_moment_rounding(31, 120000) < 1e-12 and K.first_moment_rounding(K.fraction_bits(K.target(), 3, K.GATE), 3) < 1e-12
    # the rule itself at its documented switch: 1 000 queries, R^2 ~ 2^31
    box = lambda r: np.array([[-r, -r, -r], [r, r, r]]) / np.sqrt(3.0)
    assert K.fraction_bits(box(2.0 ** 15.5 * 0.999), 1000, 1e-12) == 20 and K.fraction_bits(box(2.0 ** 15.5 * 1.001), 1000, 1e-12) == 19
    assert K.fraction_bits(K.target(), 3000, K.GATE) > 40
