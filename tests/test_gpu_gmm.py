"""Gaussian mixture on the device (Cluster_KMeans_GMM/GMM.py:13-71; include/pcr.h: pcr_gmm_*) against the NumPy restatements of
tests/gmm_checks.py and the golden recorded from the reference's own class.

Tolerances.  One step: every sum the device forms (sum gamma, sum gamma x, sum gamma d_i d_j, the log-likelihood) within 1e-11 of the
sum of the absolute values of its terms: with |a| <= 745 a 1-ulp exp / log makes a term relatively wrong by <= (745 + small) 2^-52
~ 1.7e-13, summation adds <= log2(n) 2^-53; 1e-11 leaves ~50x, a wrong formula shows at >= 1e-3.  The second moments are compared about
the means the device itself formed (they are inputs of that pass).  The loop: 46 iterations like the reference, parameters within 1e-8
absolute (a 1e-13 relative perturbation of the inputs moves the restatement's final parameters by <= 3.5e-11 over eight seeds)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import gmm_checks
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-11
LOOP_TOL = 1e-8
# the kernels' wave (64), one slot of a block (256), a block's tile (1024: one block / two), three and twenty slabs
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 20000]
KS = [1, 2, 3, 8, 9, 32]   # chunks of 8 (E pass) and 4 (covariance pass) components: both sides of each


@functools.lru_cache(maxsize=None)
def blobs(n, dim, lidar=False):
    """Seeded three-blob data; lidar: the blobs +-50 m out."""
    rng = np.random.default_rng(31 * n + dim + (7 if lidar else 0))
    centres = np.array([[0.5, 0.5, 0.2], [5.5, 2.5, -1.0], [1.0, 7.0, 2.0]]) if not lidar else np.array([[50.0, 10.0, -1.0], [-50.0, 5.0, 0.0], [0.0, -50.0, 1.0]])
    pts = centres[rng.integers(0, 3, n), :dim] + rng.normal(size=(n, dim)) * np.array([1.0, 1.7, 0.4])[:dim]
    pts.setflags(write=False)
    return pts


def start_params(data, k, seed):
    """Means at data rows, random well-conditioned covariances, random weights."""
    rng = np.random.default_rng(seed)
    n, dim = data.shape
    means = data[rng.integers(0, n, k)] + rng.normal(size=(k, dim)) * 0.3
    covs = np.empty((k, dim, dim))
    for c in range(k):
        q, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
        covs[c] = (q * rng.uniform(0.5, 4.0, dim)) @ q.T
        covs[c] = 0.5 * (covs[c] + covs[c].T)
    w = rng.uniform(0.2, 1.0, k)
    return means, covs, w / w.sum()


def upload(pcp, ctx, data):
    data = np.asarray(data)
    if data.shape[1] == 2:
        data = np.column_stack([data, np.zeros(len(data), dtype=data.dtype)])
    return pcp.DeviceCloud.upload(data, ctx)


def device_step(pcp, dc, dim, means, covs, weights):
    L = pcp._lib
    k = len(means)
    m, c, w, nk, ll = np.empty((k, dim)), np.empty((k, dim, dim)), np.empty(k), np.empty(k), C.c_double()
    st = L.lib().pcr_gmm_step(dc.ctx.handle, dc.handle, k, dim, L.dptr(L.as_f64(means)), L.dptr(L.as_f64(covs)), L.dptr(L.as_f64(weights)), L.dptr(m),
                              L.dptr(c), L.dptr(w), L.dptr(nk), C.byref(ll))
    return st, m, c, w, nk, ll.value


def check_step(pcp, ctx, data, k, seed):
    L = pcp._lib
    n, dim = data.shape
    means, covs, weights = start_params(data, k, seed)
    dc = upload(pcp, ctx, data)
    st, m, c, w, nk, ll = device_step(pcp, dc, dim, means, covs, weights)
    dc.free()
    assert st == L.PCR_OK
    ref = gmm_checks.step_log(data, means, covs, weights, about=m if np.isfinite(m).all() else None)
    s, a = ref["sums"], ref["abs_sums"]
    err = {"g": np.abs(nk - s["g"]) / a["g"].clip(1e-300), "gx": np.abs(m * nk[:, None] - s["gx"]) / a["gx"].clip(1e-300),
           "gdd": np.abs(c * nk[:, None, None] - s["gdd"]) / a["gdd"].clip(1e-300), "ll": abs(ll - ref["loglik"]) / ref["abs_loglik"]}
    live = s["g"] > 1e-250     # a component no point supports: 0/0 on both sides, nothing to compare but N_k itself
    print(f"n={n} k={k} dim={dim}: rel. errors g {err['g'].max():.2e} gx {err['gx'][live].max():.2e} gdd {err['gdd'][live].max():.2e} ll {err['ll']:.2e}")
    assert err["g"].max() <= STEP_TOL and err["ll"] <= STEP_TOL
    assert live.any() and err["gx"][live].max() <= STEP_TOL and err["gdd"][live].max() <= STEP_TOL
    assert np.abs(w - nk / n).max() <= 1e-15


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_one_step(pcp, ctx, n, k, dim):
    check_step(pcp, ctx, blobs(n, dim), k, seed=1000 * n + 10 * k + dim)


@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("n", [1025, 20000])
def test_one_step_lidar_scale(pcp, ctx, n, k):
    check_step(pcp, ctx, blobs(n, 3, lidar=True), k, seed=n + k)


def test_step_status_comes_from_the_input_parameters(pcp, ctx):
    L = pcp._lib
    data = blobs(257, 3)
    means, covs, weights = start_params(data, 3, 5)
    dc = upload(pcp, ctx, data)
    bad = covs.copy()
    bad[1] = np.diag([1.0, 0.0, 1.0])
    assert device_step(pcp, dc, 3, means, bad, weights)[0] == L.PCR_E_SINGULAR
    bad[1] = np.diag([1.0, -2.0, 1.0])
    assert device_step(pcp, dc, 3, means, bad, weights)[0] == L.PCR_E_SINGULAR
    assert device_step(pcp, dc, 3, means, covs, weights)[0] == L.PCR_OK      # the context still works
    dc.free()
    one = upload(pcp, ctx, data[:1])     # one point: the OUTPUT covariance is 0, the status is still that of the input
    st, m, c, w, nk, ll = device_step(pcp, one, 3, means[:1], covs[:1], np.ones(1))
    one.free()
    assert st == L.PCR_OK and np.array_equal(m[0], data[0]) and np.array_equal(c, np.zeros((1, 3, 3))) and nk[0] == 1.0


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("gmm.npz")


def check_fit_against(model, want, n_iter):
    assert model.n_iter_ == n_iter
    assert model.means.shape == want["means"].shape and model.covs.shape == want["covs"].shape and model.weights.shape == want["weights"].shape
    for key in ("means", "covs", "weights"):
        d = np.abs(getattr(model, key) - want[key]).max()
        print(f"{key}: max abs difference {d:.3e}")
        assert d <= LOOP_TOL, key
    assert model.nll_history_.shape == (n_iter,)
    rel = np.abs(model.nll_history_ - want["nll_history"]) / np.abs(want["nll_history"])
    print(f"nll history: max rel difference {rel.max():.3e}")
    assert rel.max() <= 1e-8
    assert model.nll_ == model.nll_history_[-1]


@pytest.mark.parametrize("default_draw", [False, True])
def test_loop_against_the_reference_golden(pcp, ctx, default_draw):
    g = golden()
    model = pcp.GMM(n_clusters=3)
    if default_draw:
        np.random.seed(int(g["np_random_seed"]))
        model.fit(g["data"], ctx=ctx)
    else:
        model.fit(g["data"], means_init=g["means_init"], ctx=ctx)
    check_fit_against(model, g, 46)
    assert model.converged_
    labels = model.predict(g["data"], ctx=ctx)
    ref_labels, gap = gmm_checks.predict_log(g["data"], g["means"], g["covs"], g["weights"])
    clear = gap > 1e-9
    assert clear.mean() >= 0.99
    assert labels.shape == (2000,) and np.array_equal(labels[clear], g["labels"][clear]) and np.array_equal(labels[clear], ref_labels[clear])
    proba = model.predict_proba(g["data"], ctx=ctx)
    gamma, _ = gmm_checks.responsibilities(gmm_checks.log_weighted_density(g["data"], model.means, model.covs, model.weights))
    assert proba.shape == (2000, 3) and np.abs(proba - gamma.T).max() <= 1e-11 and np.abs(proba.sum(axis=1) - 1.0).max() <= 1e-14


def test_lidar_scale(pcp, ctx):
    """Where the reference gives 0/0 (its densities underflow ~38 units from every mean) the device follows the log-domain loop."""
    pts = gmm_checks.lidar_blobs()
    means0 = pts[:3].copy()
    with pytest.raises((ValueError, np.linalg.LinAlgError)):
        gmm_checks.fit_literal(pts, means0)
    want = gmm_checks.fit_log(pts, means0)
    model = pcp.GMM(3).fit(pts, means_init=means0, ctx=ctx)
    check_fit_against(model, want, want["n_iter"])
    labels = model.predict(pts, ctx=ctx)
    ref_labels, gap = gmm_checks.predict_log(pts, want["means"], want["covs"], want["weights"])
    assert np.array_equal(labels[gap > 1e-9], ref_labels[gap > 1e-9]) and len(np.unique(labels)) == 3


def test_determinism_and_purity(pcp, ctx):
    pts = gmm_checks.lidar_blobs()
    dc = pcp.DeviceCloud.upload(pts, ctx)
    before = dc.download()
    a = pcp.GMM(3).fit(dc, means_init=pts[:3])
    b = pcp.GMM(3).fit(dc, means_init=pts[:3])
    for key in ("means", "covs", "weights", "nll_history_"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
    assert a.n_iter_ == b.n_iter_ and a.nll_ == b.nll_
    assert a.predict_proba(dc).tobytes() == b.predict_proba(dc).tobytes()
    assert np.array_equal(dc.download(), before) and np.array_equal(before, pts)
    dc.free()


def test_reordered_cloud(pcp, ctx):
    """A cloud laid out for queries against a grid index (records in Morton order, id = caller row): labels come back by caller row
    and the fit stays within the loop tolerance of the fresh upload's (the summation order differs, nothing else)."""
    pts = gmm_checks.lidar_blobs()
    fresh = pcp.GMM(3).fit(pts, means_init=pts[:3], ctx=ctx)
    index = pcp.TargetIndex(blobs(20000, 3, lidar=True), kind="grid", ctx=ctx)
    dc = pcp.DeviceCloud.upload(pts, ctx)
    dc.prepare(index)
    again = pcp.GMM(3).fit(dc, means_init=pts[:3])
    check_fit_against(again, {"means": fresh.means, "covs": fresh.covs, "weights": fresh.weights, "nll_history": fresh.nll_history_}, fresh.n_iter_)
    assert np.array_equal(again.predict(dc), fresh.predict(pts, ctx=ctx))
    assert np.abs(again.predict_proba(dc) - fresh.predict_proba(pts, ctx=ctx)).max() <= 1e-8
    assert np.array_equal(dc.download(), pts)
    dc.free()
    index.free()


def test_device_cloud_pipeline(pcp, ctx):
    """ground_segmentation -> GMM.fit / predict on the segmented DeviceCloud, nothing downloaded in between."""
    rng = np.random.default_rng(3)
    ground = np.column_stack([rng.uniform(-60, 60, 3000), rng.uniform(-60, 60, 3000), -1.7 + rng.normal(0, 0.02, 3000)])
    objects = gmm_checks.lidar_blobs() + np.array([0.0, 0.0, 2.0])
    scene = np.concatenate([ground[:3], objects, ground[3:]])
    dc = pcp.DeviceCloud.upload(scene, ctx)
    seg = pcp.ground_segmentation(dc, samples=np.array([[0, 1, 2]]))
    assert isinstance(seg, pcp.DeviceCloud)
    means0 = np.array([[38.0, 9.0, 1.5], [-28.0, 6.0, 2.5], [1.0, -48.0, 2.0]])
    model = pcp.GMM(3).fit(seg, means_init=means0)
    labels = model.predict(seg)
    kept = seg.download()                      # only now, to check
    seg.free()
    dc.free()
    assert len(kept) == len(labels) and len(kept) >= len(objects)
    want = gmm_checks.fit_log(kept, means0)
    check_fit_against(model, want, want["n_iter"])
    ref_labels, gap = gmm_checks.predict_log(kept, want["means"], want["covs"], want["weights"])
    assert np.array_equal(labels[gap > 1e-9], ref_labels[gap > 1e-9])


def test_random_stream(pcp, ctx):
    """After a default fit the global stream stands where the reference's fit leaves it: one np.random.random((k, dim)) further."""
    data = golden()["data"]
    np.random.seed(123)
    np.random.random((3, 2))
    want = np.random.get_state()
    np.random.seed(123)
    pcp.GMM(3, max_iter=2).fit(data, ctx=ctx)
    got = np.random.get_state()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    np.random.seed(123)
    state = np.random.get_state()
    pcp.GMM(3, max_iter=2).fit(data, means_init=np.ones((3, 2)), ctx=ctx)     # given means: nothing is drawn
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]


def test_edges(pcp, ctx):
    g = golden()
    data = g["data"]
    # max_iter = 1: one iteration, its nll recorded, not converged (inf - nll < tol is false)
    one = pcp.GMM(3, max_iter=1).fit(data, means_init=g["means_init"], ctx=ctx)
    want = gmm_checks.fit_log(data, g["means_init"], max_iter=1)
    check_fit_against(one, want, 1)
    assert not one.converged_
    # a loop that ends at max_iter without the rule firing
    five = pcp.GMM(3, max_iter=5).fit(data, means_init=g["means_init"], ctx=ctx)
    check_fit_against(five, gmm_checks.fit_log(data, g["means_init"], max_iter=5), 5)
    assert not five.converged_
    # k = 1: sample mean and (biased) covariance after the first iteration, converged in the second
    pts = gmm_checks.lidar_blobs()
    m1 = pcp.GMM(1).fit(pts, means_init=np.zeros((1, 3)), ctx=ctx)
    assert m1.n_iter_ == 2 and m1.converged_
    assert np.abs(m1.means[0] - pts.mean(axis=0)).max() <= 1e-12 * np.abs(pts).max()
    assert np.abs(m1.covs[0] - np.cov(pts.T, bias=True)).max() <= 1e-11 * np.cov(pts.T, bias=True).max()
    assert m1.weights.shape == (1, 1) and abs(m1.weights[0, 0] - 1.0) <= 1e-15 and np.array_equal(m1.predict(pts, ctx=ctx), np.zeros(len(pts), dtype=np.intp))
    # (n,2) arrays and float32 input (widened exactly)
    f32 = data.astype(np.float32)
    a = pcp.GMM(3, max_iter=4).fit(f32, means_init=g["means_init"], ctx=ctx)
    check_fit_against(a, gmm_checks.fit_log(f32.astype(np.float64), g["means_init"], max_iter=4), 4)
    assert a.means.shape == (3, 2) and a.covs.shape == (3, 2, 2) and a.predict(f32, ctx=ctx).shape == (2000,)
    b = pcp.GMM(3, max_iter=4).fit(pcp.PointCloud(pts), means_init=pts[:3], ctx=ctx)      # an object with .points
    check_fit_against(b, gmm_checks.fit_log(pts, pts[:3], max_iter=4), 4)


def test_singular_components_raise(pcp, ctx):
    L = pcp._lib
    # fewer points than components: both means land on the point, the covariances are 0
    model = pcp.GMM(2)
    with pytest.raises(np.linalg.LinAlgError) as e:
        model.fit(np.array([[1.0, 2.0, 4.0]]), means_init=np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), ctx=ctx)
    assert e.value.iteration == 1 and e.value.component == 0 and "iteration 1" in str(e.value) and "component 0" in str(e.value)
    assert model.means is None and model.covs is None and model.n_iter_ == 0          # untouched
    # duplicate points (coordinates that scale exactly, so the weighted mean is the point itself)
    with pytest.raises(np.linalg.LinAlgError) as e:
        pcp.GMM(2).fit(np.tile([[1.0, 2.0, 4.0]], (300, 1)), means_init=np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), ctx=ctx)
    assert e.value.iteration == 1 and e.value.component == 0
    with pytest.raises(np.linalg.LinAlgError):
        gmm_checks.fit_log(np.tile([[1.0, 2.0, 4.0]], (300, 1)), np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]))
    # the result record of the C call names both; a component every point has left: N_k underflows to 0
    pts = gmm_checks.lidar_blobs()
    dc = pcp.DeviceCloud.upload(pts, ctx)
    p, res = L.GmmParams(), L.GmmResult()
    L.lib().pcr_gmm_default_params(C.byref(p))
    p.n_clusters = 2
    means0 = np.array([pts[0], [4000.0, 4000.0, 4000.0]])
    out = np.zeros(2 * 9)
    st = L.lib().pcr_gmm_fit(ctx.handle, dc.handle, C.byref(p), L.dptr(means0), L.dptr(out), L.dptr(out), L.dptr(out), None, C.byref(res))
    assert st == L.PCR_E_SINGULAR and (res.bad_iter, res.bad_component) == (1, 1)
    with pytest.raises(np.linalg.LinAlgError) as e:
        gmm_checks.fit_log(pts, means0)
    assert (e.value.iteration, e.value.component) == (1, 1)
    # the context still works
    ok = pcp.GMM(3).fit(dc, means_init=pts[:3])
    assert ok.n_iter_ >= 1
    dc.free()
