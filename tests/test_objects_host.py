"""Host side of the object-batch stage (Final_Project/scripts/detect.py:269-354): exported symbols and signatures, the written
operation order against the SciPy / NumPy formulation it stands for, pcr_objects_select against the restated rule, and the argument
checks that must raise before anything touches a device.  No GPU needed."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from tests import objects_checks as chk
from tests.conftest import ROOT

NEW_SYMBOLS = ["pcr_objects_build", "pcr_objects_free", "pcr_objects_offsets", "pcr_objects_rows", "pcr_objects_stats", "pcr_objects_select",
               "pcr_objects_weights", "pcr_objects_pack_f32"]


def lidar_points(n, seed):
    """float32-rounded coordinates at lidar scale, as float64."""
    rng = np.random.default_rng(seed)
    centre = np.array([rng.uniform(2, 80), rng.uniform(-30, 30), rng.uniform(-2, 1)])
    return (centre + rng.normal(scale=[2.0, 1.0, 0.5], size=(n, 3))).astype(np.float32).astype(np.float64)


def test_new_symbols_exported_with_signatures(pcp):
    L = pcp._lib
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"PCR_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("object_stats", "resample_weights", "preprocess", "preprocess_device", "ObjectBatch"):
        assert callable(getattr(pcp, name)), name
    tile = int(re.search(r"#define\s+PCR_OBJECTS_TILE\s+(\d+)", header).group(1))
    assert tile == L.PCR_OBJECTS_TILE == pcp.objects.TILE and tile % 64 == 0


def test_importing_the_package_does_not_import_torch():
    import subprocess
    import sys

    code = "import importlib, sys; importlib.import_module('point-cloud-process_amd'); sys.exit(1 if 'torch' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


@pytest.mark.parametrize("n", [1, 2, 5, 64, 257, 1300])
def test_written_order_is_the_scipy_numpy_formulation(n):
    """The premise of the device's bit-equality: NumPy's column mean and SciPy's pdist perform the serial sums of include/pcr.h."""
    P = lidar_points(n, seed=n)
    assert np.array_equal(chk.serial_mean(P), np.mean(P, axis=0))
    assert np.array_equal(chk.serial_mean(P), P.mean(axis=0))
    if n > 1:
        assert np.array_equal(chk.serial_weights(P), chk.scipy_weights(P))
    st = chk.restated_stats(P, np.zeros(n, dtype=np.int64), 1)
    assert st["count"][0] == n and np.array_equal(st["min_bound"][0], P.min(axis=0)) and np.array_equal(st["max_bound"][0], P.max(axis=0))


def test_restated_groups_and_an_object_without_rows():
    ids = np.array([2, -1, 0, 2, 0, -5, 2])
    offsets, rows = chk.restated_groups(ids, 4)
    assert offsets.tolist() == [0, 2, 2, 5, 5] and rows.tolist() == [2, 4, 0, 3, 6]
    st = chk.restated_stats(np.arange(21.0).reshape(7, 3), ids, 4)
    assert st["count"].tolist() == [2, 0, 3, 0]
    assert np.isnan(st["mean"][1]).all() and np.isinf(st["min_bound"][3]).all() and (st["max_bound"][3] < 0).all()


def _select(pcp, count, mean, radius, min_count=4):
    L = pcp._lib
    count = np.ascontiguousarray(count, dtype=np.int64)
    mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1, 3)
    keep = np.full(len(count), 7, dtype=np.uint8)
    st = L.lib().pcr_objects_select(L.lptr(count), L.dptr(mean), len(count), min_count, float(radius), keep.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert st == L.PCR_OK
    return keep.astype(bool)


def test_select_count_rule(pcp):
    mean = np.zeros((4, 3))
    assert _select(pcp, [0, 4, 5, 6], mean, 10.0).tolist() == [False, False, True, True]   # detect.py:286: <= 4 is skipped
    assert _select(pcp, [4, 5], mean[:2], 10.0, min_count=5).tolist() == [False, False]


def test_select_radius_rule_is_strict_on_the_far_side(pcp):
    # sqrt(3*3 + 4*4) is exactly 5: on the radius is kept (detect.py:291 skips on >), one ulp beyond is dropped; z plays no part
    on = [3.0, 4.0, 100.0]
    beyond = [3.0, np.nextafter(4.0, 5.0), 0.0]
    r_beyond = np.sqrt(np.float64(3.0) * 3.0 + beyond[1] * beyond[1])
    assert r_beyond == np.nextafter(5.0, 6.0)
    got = _select(pcp, [10, 10, 10, 10], [on, beyond, [-3.0, -4.0, 0.0], beyond], 5.0)
    assert got.tolist() == [True, False, True, False]
    assert _select(pcp, [10], [beyond], r_beyond).tolist() == [True]
    assert _select(pcp, [10], [on], np.nextafter(5.0, 0.0)).tolist() == [False]


def test_select_nan_mean_is_dropped(pcp):
    nan = float("nan")
    got = _select(pcp, [10, 0, 10, 10], [[nan, 0.0, 0.0], [nan, nan, nan], [0.0, nan, 0.0], [1.0, 1.0, nan]], 50.0)
    assert got.tolist() == [False, False, False, True]
    assert _select(pcp, [10], [[nan, nan, nan]], float("inf")).tolist() == [False]


def test_select_random_vectors_equal_the_restated_rule(pcp):
    rng = np.random.default_rng(5)
    for case in range(50):
        k = int(rng.integers(1, 40))
        count = rng.integers(0, 12, size=k)
        mean = rng.uniform(-60, 60, size=(k, 3)).astype(np.float32).astype(np.float64)
        radius = float(rng.uniform(5, 80))
        if case % 5 == 0:   # centres exactly on the radius
            mean[:, :2] = np.array([3.0, 4.0]) * rng.integers(1, 10, size=(k, 1))
            radius = 5.0 * float(rng.integers(1, 10))
        if case % 7 == 0:
            mean[rng.integers(0, k)] = np.nan
        want = chk.restated_select(count, mean, radius)
        assert np.array_equal(_select(pcp, count, mean, radius), want), case
        assert np.array_equal(pcp.objects.select(count, mean, radius), want), case


def test_select_argument_validation(pcp):
    L = pcp._lib
    f = L.lib().pcr_objects_select
    count, mean, keep = np.ones(2, dtype=np.int64), np.zeros((2, 3)), np.zeros(2, dtype=np.uint8)
    kp = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    assert f(None, L.dptr(mean), 2, 4, 1.0, kp) == L.PCR_E_INVALID
    assert f(L.lptr(count), None, 2, 4, 1.0, kp) == L.PCR_E_INVALID
    assert f(L.lptr(count), L.dptr(mean), 2, 4, 1.0, None) == L.PCR_E_INVALID
    assert f(L.lptr(count), L.dptr(mean), -1, 4, 1.0, kp) == L.PCR_E_INVALID
    assert f(None, None, 0, 4, 1.0, None) == L.PCR_OK            # no objects: nothing to read or write
    with pytest.raises(ValueError, match="counts"):
        pcp.objects.select([1, 2], np.zeros((3, 3)), 1.0)


def test_c_entry_points_refuse_null_arguments_without_a_device(pcp):
    L = pcp._lib
    lib = L.lib()
    labels = np.zeros(4, dtype=np.int32)
    out = C.c_void_p(1)
    assert lib.pcr_objects_build(None, None, L.iptr(labels), 1, C.byref(out)) == L.PCR_E_INVALID
    assert not out.value                                           # no handle on an error
    assert lib.pcr_objects_free(None, None) == L.PCR_OK
    off = np.zeros(2, dtype=np.int64)
    assert lib.pcr_objects_offsets(None, L.lptr(off)) == L.PCR_E_INVALID
    assert lib.pcr_objects_rows(None, None, L.iptr(labels)) == L.PCR_E_INVALID
    assert lib.pcr_objects_stats(None, None, L.lptr(off), None, None, None) == L.PCR_E_INVALID
    w = np.zeros(4)
    assert lib.pcr_objects_weights(None, None, None, L.dptr(w)) == L.PCR_E_INVALID
    assert lib.pcr_objects_pack_f32(None, None, None, L.iptr(labels), L.lptr(off), 1, 2, None) == L.PCR_E_INVALID


def test_python_argument_checks_raise_before_any_upload(pcp):
    """Every one of these fails in the argument checks: no context is created, so they pass on a host without a device."""
    P = lidar_points(20, seed=1)
    nrm = np.tile([0.0, 0.0, 1.0], (20, 1))
    ids = np.zeros(20, dtype=np.int64)
    cfg = {"max_radius_distance": 100.0, "num_sample_points": 8, "batch_size": 4}
    empty = np.zeros(0, dtype=np.int64)
    for f in (pcp.preprocess, pcp.preprocess_device):
        with pytest.raises(ValueError, match="empty"):
            f((P, nrm), empty, cfg)                                # detect.py:279: max() of nothing
        with pytest.raises(ValueError, match="normals"):
            f((P, nrm[:19]), ids, cfg)
        with pytest.raises(ValueError, match="object ids"):
            f((P, nrm), ids[:19], cfg)
        with pytest.raises(ValueError, match="integers"):
            f((P, nrm), ids.astype(np.float64), cfg)
        with pytest.raises(ValueError, match="positive"):
            f((P, nrm), ids, dict(cfg, num_sample_points=0))
        with pytest.raises(ValueError, match="positive"):
            f((P, nrm), ids, dict(cfg, batch_size=0))
        with pytest.raises(KeyError):
            f((P, nrm), ids, {"num_sample_points": 8, "batch_size": 4})
        with pytest.raises(ValueError, match=r"\(N,3\)"):
            f((np.zeros(5), None), np.zeros(5, dtype=np.int64), cfg)
    with pytest.raises(ValueError, match="empty"):
        pcp.object_stats(P, empty)
    with pytest.raises(ValueError, match="empty"):
        pcp.resample_weights(P, empty)


def test_planted_scene_is_what_the_gpu_tests_assume():
    tile = 128
    points, normals, ids, n_objects = chk.planted_scene(tile)
    assert points.shape == (6000, 3) and normals.shape == (6000, 3) and ids.shape == (6000,) and n_objects == ids.max() + 1
    assert np.array_equal(points, points.astype(np.float32).astype(np.float64))
    assert points[:, 0].min() > 0.0 and points[:, 0].max() <= 82.0 and np.abs(points[:, 1]).max() <= 32.0
    st = chk.restated_stats(points, ids, n_objects)
    assert st["count"].tolist() == chk.object_sizes(tile) + [5, 0, chk.FAR_SIZE]
    assert (ids == -1).sum() > 1000
    rows0 = np.flatnonzero(ids == 12)
    assert np.any(np.diff(rows0) > 1)                              # objects interleave: the rows of one object are not a run
    P = points[ids == chk.COINCIDENT_ID]
    assert len(P) == 5 and (P == P[0]).all()
    keep60 = chk.restated_select(st["count"], st["mean"], 60.0)
    dropped_by_radius = (st["count"] > 4) & ~keep60
    assert dropped_by_radius.sum() >= 1 and not keep60[chk.COINCIDENT_ID] and keep60.sum() % 8 != 0
    kept_sizes = st["count"][keep60]
    assert (kept_sizes < 64).any() and (kept_sizes >= 64).any()    # S = 64: both `replace` branches of detect.py:306
    assert chk.restated_select(st["count"], st["mean"], 100.0)[chk.COINCIDENT_ID]
    mod = importlib.import_module("point-cloud-process_amd.objects")
    assert mod.TILE == tile
