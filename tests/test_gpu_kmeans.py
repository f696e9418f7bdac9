"""K-Means on the device (include/pcr.h: pcr_kmeans_*, pcr_cloud_download_rows) against the NumPy restatement of
tests/kmeans_checks.py and the golden recorded from scikit-learn's Lloyd.

Tolerances.  Labels are compared wherever the relative gap between the best and the second-best squared distance exceeds 1e-9 (a
squared distance carries a few 2^-53 of relative error on either side); on the data used here the restatement finds no smaller gap,
which every test asserts first, so in fact all labels are compared.  Counts are exact.  S_k, formed from the device's OWN labels,
within 1e-13 sum |terms|: the fixed-order sum's bound is about (12 + blocks) 2^-53 = 3.5e-15 at n = 20000, a wrong formula shows
at >= 1e-3.  A centre is S_k / N_k, so it is held to 1e-13 sum |terms| / N_k (CENTRE_TOL below); centres are recomputed from the labels in
every iteration, so the loop accumulates nothing and is held to the same bound.  Inertia within 1e-13 relative (histories 1e-12),
shift within 1e-13 (1 + max |c|) (histories 1e-12 absolute)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import gmm_checks, kmeans_checks
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

GAP = 1e-9
SUM_TOL = 1e-13
# the kernels' wave (64), one slot of a block (256), a block's tile (1024: one block / two), three and twenty slabs
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 20000]
KS = [1, 2, 3, 8, 9, 32]   # chunks of 8 clusters: both sides


@functools.lru_cache(maxsize=None)
def blobs(n, dim, lidar=False):
    """Seeded three-blob data; lidar: the blobs +-50 m out."""
    rng = np.random.default_rng(31 * n + dim + (7 if lidar else 0))
    centres = np.array([[0.5, 0.5, 0.2], [5.5, 2.5, -1.0], [1.0, 7.0, 2.0]]) if not lidar else np.array([[50.0, 10.0, -1.0], [-50.0, 5.0, 0.0], [0.0, -50.0, 1.0]])
    pts = centres[rng.integers(0, 3, n), :dim] + rng.normal(size=(n, dim)) * np.array([1.0, 1.7, 0.4])[:dim]
    pts.setflags(write=False)
    return pts


def start_centres(data, k, seed):
    """Centres near data rows (rows may repeat, k may exceed n)."""
    rng = np.random.default_rng(seed)
    n, dim = data.shape
    return data[rng.integers(0, n, k)] + rng.normal(size=(k, dim)) * 0.3


def upload(pcp, ctx, data):
    data = np.asarray(data)
    if data.shape[1] == 2:
        data = np.column_stack([data, np.zeros(len(data), dtype=data.dtype)])
    return pcp.DeviceCloud.upload(data, ctx)


def device_step(pcp, dc, dim, centres):
    L = pcp._lib
    k = len(centres)
    c, cnt, sums, inertia, shift = np.empty((k, dim)), np.empty(k, dtype=np.int64), np.empty((k, dim)), C.c_double(), C.c_double()
    st = L.lib().pcr_kmeans_step(dc.ctx.handle, dc.handle, k, dim, L.dptr(L.as_f64(centres)), L.dptr(c), L.lptr(cnt), L.dptr(sums), C.byref(inertia),
                                 C.byref(shift))
    assert st == L.PCR_OK
    return c, cnt, sums, inertia.value, shift.value


def device_predict(pcp, dc, dim, centres):
    L = pcp._lib
    k = len(centres)
    lab, cnt, inertia = np.empty(dc.n, dtype=np.int32), np.empty(k, dtype=np.int64), C.c_double()
    st = L.lib().pcr_kmeans_predict(dc.ctx.handle, dc.handle, k, dim, L.dptr(L.as_f64(centres)), L.iptr(lab), L.lptr(cnt), C.byref(inertia))
    assert st == L.PCR_OK
    return lab, cnt, inertia.value


def label_sums(data, labels, k):
    """S_k and sum |terms| from given labels."""
    s = np.stack([np.bincount(labels, weights=data[:, c], minlength=k) for c in range(data.shape[1])], axis=1)
    a = np.stack([np.bincount(labels, weights=np.abs(data[:, c]), minlength=k) for c in range(data.shape[1])], axis=1)
    return s, a


def centre_tol(data, labels, k):
    """(k,dim): 1e-13 sum |terms| / N_k; an empty cluster's centre is kept exactly."""
    _, a = label_sums(data, labels, k)
    return SUM_TOL * a / np.bincount(labels, minlength=k).clip(1)[:, None]


def check_step(pcp, ctx, data, k, seed):
    n, dim = data.shape
    centres = start_centres(data, k, seed)
    ref = kmeans_checks.step(data, centres)
    assert (ref["gap"] > GAP).all()            # the precondition: nothing has to be excluded (the cap would be 1 %)
    dc = upload(pcp, ctx, data)
    c, cnt, sums, inertia, shift = device_step(pcp, dc, dim, centres)
    lab, cnt_p, inertia_p = device_predict(pcp, dc, dim, centres)
    dc.free()
    assert np.array_equal(lab, ref["labels"])
    own = np.bincount(lab, minlength=k)
    assert np.array_equal(cnt, own) and np.array_equal(cnt_p, own) and cnt.sum() == n
    s, a = label_sums(data, lab, k)
    err = np.abs(sums - s) / a.clip(1e-300)
    print(f"n={n} k={k} dim={dim}: S_k rel. error {err.max():.2e}, inertia {abs(inertia - ref['inertia']) / max(ref['inertia'], 1e-300):.2e}, "
          f"shift {abs(shift - ref['shift']):.2e}, empty {int((own == 0).sum())}")
    assert err.max() <= SUM_TOL
    live = own > 0
    assert np.array_equal(c[live], sums[live] / own[live, None]) and np.array_equal(c[~live], centres[~live]) and np.array_equal(sums[~live], np.zeros((int((~live).sum()), dim)))
    assert np.isfinite(c).all()
    assert abs(inertia - ref["inertia"]) <= SUM_TOL * ref["inertia"] and inertia_p == inertia
    assert abs(shift - ref["shift"]) <= SUM_TOL * (1.0 + np.abs(centres).max())
    return ref


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_one_step(pcp, ctx, n, k, dim):
    check_step(pcp, ctx, blobs(n, dim), k, seed=1000 * n + 10 * k + dim)


@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("n", [1025, 20000])
def test_one_step_lidar_scale(pcp, ctx, n, k):
    check_step(pcp, ctx, blobs(n, 3, lidar=True), k, seed=n + k)


@pytest.mark.parametrize("n,k", [(1, 3), (63, 32)])
def test_more_clusters_than_points(pcp, ctx, n, k):
    """Empty clusters keep their centre (check_step compares them bit for bit) and are counted."""
    data = blobs(n, 3)
    ref = check_step(pcp, ctx, data, k, seed=77 + n)
    assert ref["n_empty"] >= k - n
    centres = start_centres(data, k, 77 + n)
    model = pcp.K_Means(k, max_iter=1).fit(data, centers_init=centres, ctx=ctx)
    want = kmeans_checks.fit(data, centres, max_iter=1)
    assert model.n_empty_ == want["n_empty"] >= k - n and np.array_equal(model.counts_, want["counts"]) and np.isfinite(model.centers_).all()
    assert np.array_equal(model.centers_[ref["counts"] == 0], centres[ref["counts"] == 0])


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("kmeans.npz")


def golden_case(name):
    g = golden()
    data = g["toy_data"] if name.startswith("toy") else blobs(20000, 3, lidar=True)
    return data, int(g[name + "_k"]), g


def check_fit_against(model, want, data):
    k = len(want["centers"])
    assert model.n_iter_ == want["n_iter"] and model.converged_ == want["converged"]
    assert model.labels_.dtype == np.intp and np.array_equal(model.labels_, want["labels"])
    assert np.array_equal(model.counts_, np.bincount(want["labels"], minlength=k))
    d = np.abs(model.centers_ - want["centers"])
    print(f"centres: max abs difference {d.max():.3e}; inertia rel. {abs(model.inertia_ - want['inertia']) / want['inertia']:.3e}")
    assert model.centers_.shape == want["centers"].shape and (d <= centre_tol(data, want["labels"], k)).all()
    assert abs(model.inertia_ - want["inertia"]) <= 1e-12 * want["inertia"]
    if "inertia_history" in want:
        assert model.inertia_history_.shape == model.shift_history_.shape == (want["n_iter"],)
        assert (np.abs(model.inertia_history_ - want["inertia_history"]) <= 1e-12 * want["inertia_history"]).all()
        assert np.abs(model.shift_history_ - want["shift_history"]).max() <= 1e-12


@pytest.mark.parametrize("default_draw", [False, True])
@pytest.mark.parametrize("name", ["toy_k3", "lidar_k3", "lidar_k8"])
def test_loop_against_the_scikit_learn_golden(pcp, ctx, name, default_draw):
    data, k, g = golden_case(name)
    model = pcp.K_Means(n_clusters=k, tolerance=0.0)
    if default_draw:
        np.random.seed(int(g["np_random_seed"]))
        model.fit(data, ctx=ctx)
    else:
        model.fit(data, centers_init=g[name + "_centers_init"], ctx=ctx)
    want = {"centers": g[name + "_centers"], "labels": g[name + "_labels"].astype(np.intp), "inertia": float(g[name + "_inertia"]),
            "n_iter": int(g[name + "_n_iter"]), "converged": True}
    check_fit_against(model, want, data)
    assert model.shift_history_[-1] == 0.0 and model.n_empty_ == 0
    assert np.array_equal(model.predict(data, ctx=ctx), want["labels"])


def restatement_fit(data, centres0, max_iter, tol):
    """The restatement's run with the preconditions of a comparison: no assignment and no stop that rounding could flip."""
    want = kmeans_checks.fit(data, centres0, max_iter=max_iter, tol=tol)
    assert want["min_gap"].min() > GAP
    if tol > 0:
        assert (np.abs(want["shift_history"] - tol) > 1e-6 * tol).all()
    return want


@pytest.mark.parametrize("tol", [0.0, 1e-4])
@pytest.mark.parametrize("n,k,lidar", [(20000, 8, True), (1025, 9, False)])
def test_loop_against_the_restatement(pcp, ctx, n, k, lidar, tol):
    data = blobs(n, 3, lidar=lidar)
    centres0 = kmeans_checks.seeds(data, k)
    want = restatement_fit(data, centres0, 300, tol)
    assert want["converged"] and want["n_iter"] > 2
    model = pcp.K_Means(k, tolerance=tol).fit(data, centers_init=centres0, ctx=ctx)
    check_fit_against(model, want, data)


def test_edges(pcp, ctx):
    g = golden()
    data, c0 = g["toy_data"], g["toy_k3_centers_init"]
    # max_iter = 1: one iteration, not converged
    one = pcp.K_Means(3, max_iter=1).fit(data, centers_init=c0, ctx=ctx)
    check_fit_against(one, restatement_fit(data, c0, 1, 1e-4), data)
    assert one.n_iter_ == 1 and not one.converged_
    # ... unless the shift is already <= tol
    big = pcp.K_Means(3, max_iter=1, tolerance=1e3).fit(data, centers_init=c0, ctx=ctx)
    assert big.n_iter_ == 1 and big.converged_ and np.array_equal(big.centers_, one.centers_)
    # a loop that ends at max_iter without the rule firing
    five = pcp.K_Means(3, max_iter=5).fit(data, centers_init=c0, ctx=ctx)
    check_fit_against(five, restatement_fit(data, c0, 5, 1e-4), data)
    assert five.n_iter_ == 5 and not five.converged_
    # more iterations than one read-back of the loop state covers, ending between two read-backs
    eleven = pcp.K_Means(3, max_iter=11, tolerance=0.0).fit(data, centers_init=c0, ctx=ctx)
    check_fit_against(eleven, restatement_fit(data, c0, 11, 0.0), data)
    assert eleven.n_iter_ == 11
    # k = 1: the sample mean after the first iteration, converged in the second
    pts = gmm_checks.lidar_blobs()
    m1 = pcp.K_Means(1).fit(pts, centers_init=np.zeros((1, 3)), ctx=ctx)
    assert m1.n_iter_ == 2 and m1.converged_ and m1.shift_history_[1] == 0.0
    assert np.abs(m1.centers_[0] - pts.mean(axis=0)).max() <= 1e-13 * np.abs(pts).max()
    assert np.array_equal(m1.labels_, np.zeros(len(pts), dtype=np.intp)) and list(m1.counts_) == [len(pts)]
    # (n,2) arrays and float32 input (widened exactly)
    f32 = data.astype(np.float32)
    a = pcp.K_Means(3, max_iter=4).fit(f32, centers_init=c0, ctx=ctx)
    check_fit_against(a, restatement_fit(f32.astype(np.float64), c0, 4, 1e-4), f32.astype(np.float64))
    assert a.centers_.shape == (3, 2) and a.predict(f32, ctx=ctx).shape == (2000,)
    # an object with .points; labels=False
    b = pcp.K_Means(3, max_iter=4).fit(pcp.PointCloud(pts), centers_init=pts[:3], labels=False, ctx=ctx)
    want = restatement_fit(pts, pts[:3], 4, 1e-4)
    assert b.labels_ is None and b.n_iter_ == want["n_iter"] and np.array_equal(b.counts_, want["counts"])
    assert (np.abs(b.centers_ - want["centers"]) <= centre_tol(pts, want["labels"], 3)).all()
    assert np.array_equal(pcp.K_Means(3, max_iter=4).fit_predict(pcp.PointCloud(pts), centers_init=pts[:3], ctx=ctx), want["labels"])


def test_duplicate_points(pcp, ctx):
    """All points and all seeds on one point: every tie goes to cluster 0, the others stay empty where they are, nothing is NaN."""
    pts = np.tile([[1.0, 2.0, 4.0]], (300, 1))
    c0 = np.tile([[1.0, 2.0, 4.0]], (3, 1))
    m = pcp.K_Means(3).fit(pts, centers_init=c0, ctx=ctx)
    assert np.array_equal(m.labels_, np.zeros(300, dtype=np.intp)) and list(m.counts_) == [300, 0, 0] and m.n_empty_ == 2
    assert np.array_equal(m.centers_, c0) and m.inertia_ == 0.0 and m.n_iter_ == 1 and m.converged_ and m.shift_history_[0] == 0.0


def test_determinism_and_purity(pcp, ctx):
    pts = blobs(20000, 3, lidar=True)
    c0 = kmeans_checks.seeds(pts, 8)
    dc = pcp.DeviceCloud.upload(pts, ctx)
    before = dc.download()
    a = pcp.K_Means(8, tolerance=0.0).fit(dc, centers_init=c0)
    b = pcp.K_Means(8, tolerance=0.0).fit(dc, centers_init=c0)
    for key in ("centers_", "inertia_history_", "shift_history_", "labels_", "counts_"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
    assert a.n_iter_ == b.n_iter_ > 2 and a.inertia_ == b.inertia_
    assert np.array_equal(dc.download(), before) and np.array_equal(before, pts)
    dc.free()


def test_prepared_cloud_and_row_download(pcp, ctx):
    """A cloud laid out for queries against a grid index (records in Morton order, id = caller row): labels come back by caller row,
    the centres differ by the summation order only; pcr_cloud_download_rows returns the caller's rows in the order asked."""
    L = pcp._lib
    pts = blobs(20000, 3, lidar=True)
    c0 = kmeans_checks.seeds(pts, 8)
    fresh_dc = pcp.DeviceCloud.upload(pts, ctx)
    fresh = pcp.K_Means(8, tolerance=0.0).fit(fresh_dc, centers_init=c0)
    index = pcp.TargetIndex(blobs(1025, 3, lidar=True), kind="grid", ctx=ctx)
    dc = pcp.DeviceCloud.upload(pts, ctx)
    dc.prepare(index)
    again = pcp.K_Means(8, tolerance=0.0).fit(dc, centers_init=c0)
    assert again.n_iter_ == fresh.n_iter_ and np.array_equal(again.labels_, fresh.labels_) and np.array_equal(again.counts_, fresh.counts_)
    assert (np.abs(again.centers_ - fresh.centers_) <= centre_tol(pts, fresh.labels_, 8)).all()
    assert np.array_equal(again.predict(dc), fresh.labels_)
    big = np.random.default_rng(5).integers(0, len(pts), 4096)
    for cloud in (fresh_dc, dc):
        for rows in ([5, 0, 5, len(pts) - 1, 17], [len(pts) - 1], big):
            assert np.array_equal(cloud.download_rows(rows), pts[np.asarray(rows)])
        for bad in ([0, len(pts)], [-1], np.zeros(4097, dtype=np.int64)):
            with pytest.raises(L.PcrError) as e:
                cloud.download_rows(bad)
            assert e.value.status == L.PCR_E_INVALID
    np.random.seed(4)
    drawn = pcp.K_Means(8, max_iter=3).fit(dc)          # the default draw on a prepared cloud: the same rows, by caller row
    np.random.seed(4)
    rows = np.random.choice(len(pts), 8, replace=False)
    given = pcp.K_Means(8, max_iter=3).fit(dc, centers_init=pts[rows])
    assert drawn.centers_.tobytes() == given.centers_.tobytes()
    assert np.array_equal(dc.download(), pts)
    for h in (dc, fresh_dc, index):
        h.free()


def test_device_cloud_pipeline(pcp, ctx):
    """ground_segmentation -> K_Means.fit -> GMM.fit seeded with its centres, on the segmented DeviceCloud; nothing is downloaded in
    between."""
    rng = np.random.default_rng(3)
    ground = np.column_stack([rng.uniform(-60, 60, 3000), rng.uniform(-60, 60, 3000), -1.7 + rng.normal(0, 0.02, 3000)])
    objects = gmm_checks.lidar_blobs() + np.array([0.0, 0.0, 2.0])
    scene = np.concatenate([ground[:3], objects, ground[3:]])
    dc = pcp.DeviceCloud.upload(scene, ctx)
    seg = pcp.ground_segmentation(dc, samples=np.array([[0, 1, 2]]))
    assert isinstance(seg, pcp.DeviceCloud)
    c0 = np.array([[30.0, 0.0, 1.0], [-20.0, 0.0, 2.0], [5.0, -30.0, 2.0]])
    km = pcp.K_Means(3).fit(seg, centers_init=c0)
    mix = pcp.GMM(3).fit(seg, means_init=km.centers_)
    kept = seg.download()                      # only now, to check
    seg.free()
    dc.free()
    assert len(kept) == len(km.labels_) >= len(objects)
    check_fit_against(km, restatement_fit(kept, c0, 300, 1e-4), kept)
    want = gmm_checks.fit_log(kept, km.centers_)
    assert mix.n_iter_ == want["n_iter"]
    for key in ("means", "covs", "weights"):
        assert np.abs(getattr(mix, key) - want[key]).max() <= 1e-8, key


def test_random_stream(pcp, ctx):
    """After a default fit the global stream stands one np.random.choice(n, k, replace=False) further; with centers_init it is untouched."""
    data = golden()["toy_data"]
    np.random.seed(123)
    np.random.choice(len(data), 3, replace=False)
    want = np.random.get_state()
    np.random.seed(123)
    pcp.K_Means(3, max_iter=2).fit(data, ctx=ctx)
    got = np.random.get_state()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    np.random.seed(123)
    state = np.random.get_state()
    pcp.K_Means(3, max_iter=2).fit(data, centers_init=np.ones((3, 2)), ctx=ctx)
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
