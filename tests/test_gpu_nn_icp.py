"""GPU parity tests (run on the MI355X box): HIP path vs the CPU oracle and the
reference goldens, through the C ABI (ctypes -> libpcr.so)."""
import numpy as np
import pytest

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

TIE_MARGIN = 1e-12  # queries whose two nearest targets are closer than this (relative d2) are ties


def _check_nn(idx, d2, q, t, oracle, gate=None):
    oi, od2, margin = oracle.nn1_exact(q, t)
    if gate is not None:
        gated = od2 < gate
        assert np.array_equal(idx >= 0, gated)
        sel = gated
    else:
        sel = np.ones(len(q), bool)
    clear = sel & (margin > TIE_MARGIN)
    assert np.array_equal(idx[clear], oi[clear])
    # squared distances are bit-identical to the direct form evaluated on the host
    assert np.array_equal(d2[sel], od2[sel])
    return int((~clear & sel).sum())


@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_nn1_small_uniform(pcp, oracle, kind):
    rng = np.random.default_rng(0)
    t = rng.uniform(-1, 1, (3000, 3))
    q = rng.uniform(-1.2, 1.2, (1777, 3))
    index = pcp.TargetIndex(t, kind=kind)
    idx, d2 = index.nn1(q)
    _check_nn(idx, d2, q, t, oracle)
    idx, d2 = index.nn1(q, max_d2=0.002)
    _check_nn(idx, d2, q, t, oracle, gate=0.002)


@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_nn1_kitti_20k_with_transform(pcp, oracle, syn, kind):
    src, tgt, Tt = syn.perturbed_pair(20000, seed=7)
    index = pcp.TargetIndex(tgt, kind=kind)
    T = syn.rigid_transform((0.1, 0.2, 1.0), 0.01, (0.1, 0.0, 0.0))
    idx, d2 = index.nn1(src, T=T, max_d2=5.0)
    moved = src.astype(np.float64)
    moved = np.stack([
        ((T[0, 0] * moved[:, 0] + T[0, 1] * moved[:, 1]) + T[0, 2] * moved[:, 2]) + T[0, 3],
        ((T[1, 0] * moved[:, 0] + T[1, 1] * moved[:, 1]) + T[1, 2] * moved[:, 2]) + T[1, 3],
        ((T[2, 0] * moved[:, 0] + T[2, 1] * moved[:, 1]) + T[2, 2] * moved[:, 2]) + T[2, 3]], axis=1)
    _check_nn(idx, d2, moved, tgt.astype(np.float64), oracle, gate=5.0)


def test_nn1_edge_cases(pcp, oracle):
    rng = np.random.default_rng(3)
    # single target point, queries far outside the grid, duplicate targets, collinear cloud
    t1 = np.array([[1.0, 2.0, 3.0]])
    q = rng.normal(0, 50, (100, 3))
    for kind in ("grid", "brute"):
        idx, d2 = pcp.TargetIndex(t1, kind=kind).nn1(q)
        assert (idx == 0).all() and np.array_equal(d2, oracle.dist2_direct(q, t1[0]))
    t = rng.uniform(0, 1, (500, 3))
    far = rng.uniform(0, 1, (64, 3)) + np.array([1e4, -3e3, 10.0])
    for kind in ("grid", "brute"):
        idx, d2 = pcp.TargetIndex(t, kind=kind).nn1(far)
        bi, bd2 = oracle.nn1_bruteforce(far, t)
        assert np.array_equal(d2, bd2)
    dup = np.concatenate([t, t[:50]])
    for kind in ("grid", "brute"):
        idx, d2 = pcp.TargetIndex(dup, kind=kind).nn1(t[:50] + 1e-9)
        assert np.array_equal(idx, np.arange(50))  # exact ties resolve to the lowest index
    line = np.c_[np.linspace(0, 10, 400), np.zeros(400), np.zeros(400)]
    for kind in ("grid", "brute"):
        idx, d2 = pcp.TargetIndex(line, kind=kind).nn1(line + np.array([0.004, 0.3, -0.2]))
        bi, bd2 = oracle.nn1_bruteforce(line + np.array([0.004, 0.3, -0.2]), line)
        assert np.array_equal(d2, bd2)


def test_empty_cloud_is_an_error(pcp):
    with pytest.raises(RuntimeError):
        pcp.TargetIndex(np.zeros((0, 3)))


@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_pass_moments_match_oracle(pcp, oracle, syn, kind):
    """One association + accumulation pass (pcr_icp_moments) against the oracle's moments.  On the grid index this is the binary64 SLAB
    path (pcr_grid_icp_pass: tile -> hard -> grid_accumulate_kernel), never the fixed-point accumulators of the one-kernel pass: those
    are reachable through pcr_icp only and are held to the restated loop by tests/test_gpu_icp_loop.py."""
    src, tgt, Tt = syn.perturbed_pair(20000, seed=11)
    index = pcp.TargetIndex(tgt, kind=kind)
    m, origin, sum_d2 = index.moments(src, None, 5.0)
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    oi, od2, _ = oracle.nn1_exact(s64, t64)
    keep = od2 < 5.0
    ref = oracle.moments(s64[keep], t64[oi[keep]], origin)
    assert m[0] == ref[0]
    assert np.allclose(m, ref, rtol=1e-11, atol=1e-9)
    assert abs(sum_d2 - od2[keep].sum()) < 1e-9 * od2[keep].sum()
    # bitwise reproducible run to run (fixed reduction order)
    m2, _, s2 = index.moments(src, None, 5.0)
    assert np.array_equal(m, m2) and s2 == sum_d2


@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_icp_compat_matches_reference_goldens(pcp, kind, capsys):
    """icp_point2point vs the outputs of the reference's own Registration/main.py:icp_point2point."""
    g = load_golden("icp_compat.npz")
    big = load_golden("icp_compat_big.npz")     # SURVEY 8c G3 at N = 20 000 (the largest size the literal reference can run)
    for tag in list(g["cases"]) + list(big["cases"]):
        tag = str(tag)
        if tag in big.files or f"{tag}_src" in big.files:
            g = big
        src = pcp.PointCloud(g[f"{tag}_src"])
        T, info = pcp.icp_point2point(src, g[f"{tag}_tgt"], g[f"{tag}_T0"], nn=kind, return_info=True)
        assert info["iters"] == int(g[f"{tag}_iters"][0]), tag
        assert np.linalg.norm(T - g[f"{tag}_T"]) < 1e-4, tag  # BASELINE.json: 1e-4 Frobenius on R|t
        assert np.linalg.norm(T - g[f"{tag}_T"]) < 1e-9, tag  # what the f64 path actually achieves
        assert np.abs(src.points - g[f"{tag}_src_after"]).max() < 1e-9, tag  # in-place side effect (main.py:110)
        failed = int(g[f"{tag}_failed"][0])
        assert (info["status"] == 1) == bool(failed), tag
    assert "ICP failed, cannot find enough associations!" in capsys.readouterr().out


def test_icp_total_matches_oracle(pcp, oracle, syn):
    src, tgt, Tt = syn.perturbed_pair(20000, seed=5)
    T, log = pcp.ICP(src, tgt, max_iteration=30)
    To, logo = oracle.icp_total(src, tgt, max_iteration=30)
    assert len(log["R_diff"]) == len(logo["R_diff"])
    assert np.linalg.norm(T - To) < 1e-8
    assert np.allclose(log["t_diff"], logo["t_diff"], atol=1e-9)
    # and it moves towards the true pose (point-to-point ICP on ring-dominated scans converges slowly)
    assert np.linalg.norm(T[:3, 3] - Tt[:3, 3]) < 0.8 * np.linalg.norm(Tt[:3, 3])


def test_icp_120k_full_size_properties(pcp, oracle, syn):
    """BASELINE config 2 size: grid and brute-force paths agree with each other and with the CPU oracle."""
    src, tgt, Tt = syn.perturbed_pair(120000, seed=0)
    ig = pcp.TargetIndex(tgt, kind="grid")
    ib = pcp.TargetIndex(tgt, kind="brute")
    idx_g, d2_g = ig.nn1(src, max_d2=5.0)
    idx_b, d2_b = ib.nn1(src, max_d2=5.0)
    oi, od2, margin = oracle.nn1_exact(src.astype(np.float64), tgt.astype(np.float64), workers=-1)
    sel = od2 < 5.0
    assert np.array_equal(idx_g >= 0, sel) and np.array_equal(idx_b >= 0, sel)
    assert np.array_equal(d2_g[sel], od2[sel]) and np.array_equal(d2_b[sel], od2[sel])
    clear = sel & (margin > TIE_MARGIN)
    assert np.array_equal(idx_g[clear], oi[clear]) and np.array_equal(idx_b[clear], oi[clear])
    Tg = pcp.icp_point2point(pcp.PointCloud(src), ig, np.eye(4))
    Tb = pcp.icp_point2point(pcp.PointCloud(src), ib, np.eye(4))
    To = oracle.icp_point2point(src, tgt, np.eye(4))["T"]
    assert np.linalg.norm(Tg - To) < 1e-9 and np.linalg.norm(Tb - To) < 1e-9


def test_procrustes_and_pose_utils(pcp):
    g = load_golden("procrustes.npz")
    for key in ("K3", "K10", "K500", "K3000", "refl"):
        A, B = g[f"{key}_A"], g[f"{key}_B"]
        R, t, cost = pcp.procrustes_transformation(A, B)
        assert R.shape == (3, 3) and t.shape == (3, 1)
        if key == "K3":
            # 3 points: H has rank 2, U V^T is only defined up to the sign of the null direction
            # (LAPACK-implementation-defined in the reference); we return the proper rotation and
            # must agree with the reference on the plane the data spans.
            assert np.linalg.det(R) > 0
            assert np.abs((R @ A + t) - (g["K3_R"] @ A + g["K3_t"])).max() < 1e-9
        else:
            assert np.abs(R - g[f"{key}_R"]).max() < 1e-9, key
            assert np.abs(t - g[f"{key}_t"]).max() < 1e-9, key
        assert abs(cost - g[f"{key}_cost"][0]) < 1e-7 * max(1.0, cost), key
    p = load_golden("pose_utils.npz")
    for T, tq in zip(p["T"], p["tq"]):
        assert np.allclose(pcp.homo2tq(T), tq, rtol=0, atol=1e-15)
        assert np.allclose(pcp.rotmat2quaternion(T[:3, :3]), tq[3:], rtol=0, atol=1e-15)


def test_nn1_far_from_origin_and_odd_sizes(pcp, oracle, syn):
    """The tile stage filters in binary32 about the tile centre: absolute coordinates of 1e6 m (UTM-like),
    sizes that are not multiples of the 64-query tile, and query == target (d = 0) must stay exact."""
    rng = np.random.default_rng(8)
    off = np.array([4.0e5, 5.5e6, 300.0])
    tgt = syn.kitti_like_scan(30011, seed=21).astype(np.float64) + off
    src = syn.kitti_like_scan(10007, seed=22).astype(np.float64) + off + rng.normal(0, 0.02, (10007, 3))
    index = pcp.TargetIndex(tgt, kind="grid")
    idx, d2 = index.nn1(src)  # no gate: every query must resolve
    oi, od2, margin = oracle.nn1_exact(src, tgt)
    assert np.array_equal(d2, od2)
    clear = margin > TIE_MARGIN
    assert np.array_equal(idx[clear], oi[clear])
    for n in (1, 63, 65):
        i2, dd = index.nn1(tgt[:n])  # queries that ARE targets
        assert np.array_equal(i2, np.arange(n)) and (dd == 0).all()


@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_nn1_dense_volume_and_clustered_duplicates(pcp, oracle, kind):
    rng = np.random.default_rng(9)
    tgt = rng.uniform(0, 2.0, (40000, 3))
    tgt[5000:5200] = tgt[100]  # 200 exact duplicates of one point: ties must resolve to the lowest index
    q = rng.uniform(-0.1, 2.1, (5000, 3))
    q[:50] = tgt[100] + rng.normal(0, 1e-4, (50, 3))
    index = pcp.TargetIndex(tgt, kind=kind)
    idx, d2 = index.nn1(q)
    bi, bd2 = oracle.nn1_bruteforce(q, tgt)
    assert np.array_equal(d2, bd2)
    assert np.array_equal(idx, bi)  # np.argmin also returns the first (lowest) index on ties
    if kind == "brute":
        # the 50 queries next to the 200 duplicates (12.5 consecutive tiles = at least two argmin groups of 8 tiles inside one
        # target split of this launch) cannot be proven by the packed argmin: they took the exact sweep
        assert index.ctx.search_stats()["brute_fallback"] >= 50


def test_brute_two_distant_dense_clusters(pcp, oracle):
    """The case the round-1 brute-force kernel got wrong: two dense 0.3 m clusters 2 km apart.
    About the box centre |a'|^2 ~ 1e6 m^2 while neighbour d^2 ~ 1e-5 m^2; ranking d^2 - |a'|^2 at 2^-36 relative
    mis-ranked 14 of 20 000 queries.  With |a'|^2 in the MFMA C operand the packed value is d^2 + bias, the rigorous
    band sends what cannot be proven to the exact sweep, and every index must equal scipy's (ties excluded)."""
    rng = np.random.default_rng(77)
    c = np.array([[0.0, 0.0, 0.0], [2000.0, 0.0, 0.0]])
    tgt = c[rng.integers(0, 2, 60000)] + rng.uniform(-0.15, 0.15, (60000, 3))
    q = tgt[rng.integers(0, 60000, 20000)] + rng.normal(0, 0.003, (20000, 3))
    index = pcp.TargetIndex(tgt, kind="brute")
    idx, d2 = index.nn1(q)
    fb = index.ctx.search_stats()["brute_fallback"]
    oi, od2, margin = oracle.nn1_exact(q, tgt)
    assert np.array_equal(d2, od2)
    clear = margin > TIE_MARGIN
    assert np.array_equal(idx[clear], oi[clear])
    assert fb < 2000, fb   # the band is ~1e-8 m^2 here: the fallback is the exception, not the path
    # same through the fused ICP pass (gate = the reference's 5 m^2, main.py:103)
    m, o, s = index.moments(q, np.eye(4), max_d2=5.0)
    assert int(round(m[0])) == int((od2 < 5.0).sum())
    assert abs(s - od2[od2 < 5.0].sum()) <= 1e-9 * max(1.0, od2.sum())


def test_brute_kitti_scan_proves_itself(pcp, syn):
    """On a KITTI-shaped pair the sweep's own bound proves (almost) every query: the exact fallback stays idle, so the
    measured sweep time is the production time."""
    src, tgt, _ = syn.perturbed_pair(120000, seed=0)
    index = pcp.TargetIndex(tgt, kind="brute")
    index.nn1(src)
    assert index.ctx.search_stats()["brute_fallback"] <= 8


def test_icp_is_bitwise_reproducible(pcp, syn):
    """Same inputs -> the same bits, run after run (fixed-order reductions, no order-dependent atomics, no races)."""
    src, tgt, _ = syn.perturbed_pair(120000, seed=0)
    index = pcp.TargetIndex(tgt)
    outs = []
    for rep in range(4):
        sd = pcp.DeviceCloud.upload(src)
        r = pcp.icp_device(sd, index, np.eye(4), mode="total", max_iter=30, r_thres=-1.0, t_thres=-1.0, min_iter=30)
        outs.append((r["T_total"].tobytes(), r["n_assoc"], sd.download().tobytes()))
        sd.free()
    assert all(o == outs[0] for o in outs[1:])
    # the two variants of the pass (one launch with the work queue served in place / publish, then a second launch that
    # serves it: what the library picks while several loops are in flight) round the same partial sums: same bits
    import os
    try:
        for v in ("1", "0"):
            os.environ["PCR_PASS_INLINE"] = v
            sd = pcp.DeviceCloud.upload(src)
            r = pcp.icp_device(sd, index, np.eye(4), mode="total", max_iter=30, r_thres=-1.0, t_thres=-1.0, min_iter=30)
            assert (r["T_total"].tobytes(), r["n_assoc"], sd.download().tobytes()) == outs[0], v
            sd.free()
    finally:
        os.environ.pop("PCR_PASS_INLINE", None)
    idx0 = index.nn1(src)
    idx1 = index.nn1(src)
    assert np.array_equal(idx0[0], idx1[0]) and np.array_equal(idx0[1], idx1[1])


@pytest.mark.parametrize("n", [140000, 400000])
def test_icp_bits_across_wave_generations(pcp, syn, n):
    """Clouds whose ICP pass is more than one generation of waves (> 131 072 points on 256 CUs): the library takes the two-launch
    variant there; forced into the one-launch variant most waves may not wait for work, late items are served by whoever is
    left and, at the latest, by the launch's last wave.  Same bits every time and in both variants."""
    import os
    src, tgt, _ = syn.perturbed_pair(n, seed=0)
    index = pcp.TargetIndex(tgt)
    kw = dict(mode="total", max_iter=8, r_thres=-1.0, t_thres=-1.0, min_iter=8)
    outs = []
    try:
        for v in (None, None, "1", "1", "0"):
            if v is None:
                os.environ.pop("PCR_PASS_INLINE", None)
            else:
                os.environ["PCR_PASS_INLINE"] = v
            sd = pcp.DeviceCloud.upload(src)
            r = pcp.icp_device(sd, index, np.eye(4), **kw)
            outs.append((r["T_total"].tobytes(), int(r["n_assoc"]), sd.download().tobytes()))
            sd.free()
    finally:
        os.environ.pop("PCR_PASS_INLINE", None)
    assert all(o == outs[0] for o in outs[1:])


def test_icp_bits_do_not_depend_on_concurrency(pcp, syn):
    """Three host threads register the same pair on three contexts of one GPU at the same time (the library switches between
    the one-launch and the two-launch pass by what it sees in flight, per pass): every result has the bits of the run alone."""
    import threading
    src, tgt, _ = syn.perturbed_pair(60000, seed=3)
    kw = dict(mode="total", max_iter=25, r_thres=-1.0, t_thres=-1.0, min_iter=25)
    index = pcp.TargetIndex(tgt)
    sd = pcp.DeviceCloud.upload(src)
    alone = pcp.icp_device(sd, index, np.eye(4), **kw)
    want = (alone["T_total"].tobytes(), alone["n_assoc"], sd.download().tobytes())
    sd.free()
    index.free()
    outs, errs = [None] * 3, []

    def run(i):
        try:
            c = pcp.Context(0, shared=(i == 2))
            ix = pcp.TargetIndex(pcp.DeviceCloud.upload(tgt, c), ctx=c)
            for rep in range(3):
                d = pcp.DeviceCloud.upload(src, c)
                r = pcp.icp_device(d, ix, np.eye(4), **kw)
                outs[i] = (r["T_total"].tobytes(), r["n_assoc"], d.download().tobytes())
                d.free()
                if outs[i] != want:
                    break
            ix.free()
            c.close()
        except Exception as e:   # surfaces in the main thread
            errs.append(repr(e))

    th = [threading.Thread(target=run, args=(i,)) for i in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert all(o == want for o in outs)


def test_nn1_cell_with_more_than_65535_points(pcp, oracle):
    """A level-0 cell holding > 65535 points overflows the 16-bit child counts of the 2x2x2-block table: the
    directory must fall back to the per-cell table for that block (and the tile goes to the exact descent)."""
    rng = np.random.default_rng(21)
    blob = np.array([3.0, 3.0, 3.0]) + rng.uniform(0, 1e-3, (70000, 3))
    rest = rng.uniform(0, 6.0, (30000, 3))
    tgt = np.concatenate([rest[:15000], blob, rest[15000:]])
    q = np.concatenate([np.array([3.0, 3.0, 3.0]) + rng.uniform(-0.05, 0.05, (3000, 3)), rng.uniform(-0.2, 6.2, (3000, 3))])
    index = pcp.TargetIndex(tgt, kind="grid", cell=0.1)
    idx, d2 = index.nn1(q)
    ties = _check_nn(idx, d2, q, tgt, oracle)
    assert ties < 50
    # and through the fused ICP pass: same association count as the oracle's gate
    m, o, s = index.moments(q, np.eye(4), max_d2=5.0)
    oi, od2, _ = oracle.nn1_exact(q, tgt)
    assert int(round(m[0])) == int((od2 < 5.0).sum())
    assert abs(s - od2[od2 < 5.0].sum()) <= 1e-9 * max(1.0, od2.sum())
