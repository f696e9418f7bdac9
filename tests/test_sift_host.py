"""CPU: the NumPy restatement of the SIFT-3D rules (tests/sift_checks.py) on tables whose answer is derived by hand, the host-only
pcr_sift_scales, the call surface of the new entry points (pcr_sift*, pcl_keypoints.py), and the CONDITIONS of the GPU cases of
tests/test_gpu_sift.py, asserted from the restatement alone: that the seeded case has keypoints in several octaves, an octave whose
every ball is the whole cloud, a candidate on the list's way in the sparse case, and every decision margin far above the device table's
error bound."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from tests import sift_checks as sk
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def og():
    return importlib.import_module("oracle.oracle_global")


# ------------------------------------------------------------------------------------------------ the call surface
ABI = {"pcr_sift_scales": 3, "pcr_sift_octave": 12, "pcr_sift_extrema": 9, "pcr_sift": 13}


def test_abi_is_declared_bound_and_exported(pcp):
    L = pcp._lib
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for name, n_params in ABI.items():
        decls = re.findall(r"PCR_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decls) == 1, name                                          # declared once
        params = re.sub(r"/\*.*?\*/", "", decls[0], flags=re.S).split(",")
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert len(L.SIGNATURES[name][1]) == len(params) == n_params, name    # one bound argument per declared parameter
    assert header.count("parity with PCL's binary32 output is unpinned") >= 4
    assert "STATED DEPARTURE" in header
    # bad arguments are refused before any device work (there is no device here)
    one = np.zeros(16)
    i4 = np.zeros(4, dtype=np.int32)
    nk = np.zeros(1, dtype=np.int64)
    d, ip, lp = L.dptr(one), L.iptr(i4), L.lptr(nk)
    assert lib.pcr_sift_octave(None, None, 0.1, 3, 0.0, 1, d, None, ip, ip, 4, lp) == L.PCR_E_INVALID
    assert lib.pcr_sift_extrema(None, None, d, 3, 0.0, ip, ip, 4, lp) == L.PCR_E_INVALID
    assert lib.pcr_sift(None, None, 0.1, 3, 3, 0.0, 1, d, ip, ip, 4, lp, None) == L.PCR_E_INVALID
    assert not one.any() and not i4.any() and not nk.any()


def test_python_surface(pcp):
    mod = pcp.pcl_keypoints
    for name in ("sift_keypoints", "sift_octave", "sift_extrema", "sift_scales"):
        assert getattr(pcp, name) is getattr(mod, name) and name in mod.__all__
    sig = inspect.signature(mod.sift_keypoints)
    got = [(p.name, None if p.default is p.empty else p.default) for p in sig.parameters.values() if p.kind is p.POSITIONAL_OR_KEYWORD]
    # keypoints.cpp:85 and the module's defaults: min_scale 0.1, 6 octaves, 10 scales an octave, contrast 0.05
    assert got == [("points", None), ("min_scale", 0.1), ("n_octaves", 6), ("n_scales_per_octave", 10), ("min_contrast", 0.05)]
    kw = {p.name: p.default for p in sig.parameters.values() if p.kind is p.KEYWORD_ONLY}
    assert kw == {"field": "y", "return_scales": False, "return_details": False, "ctx": None}
    # the wrapper's own name is still the stub it was (routed in a later change)
    with pytest.raises(NotImplementedError):
        pcp.PCLKeypoint.keypointSift(np.zeros((4, 3)))
    # refused in Python, before a device is asked for
    bad = np.zeros((30, 3))
    bad[7, 2] = np.inf
    for f in (lambda: mod.sift_keypoints(bad), lambda: mod.sift_octave(bad, 0.1), lambda: mod.sift_extrema(bad, np.zeros((30, 3)))):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):
        mod.sift_keypoints(np.zeros((30, 3)), field="w")


@pytest.mark.parametrize("q", [1, 2, 3, 7, 10, 13])
@pytest.mark.parametrize("b", [0.1, 0.5, 1.0, 3.7e-3, 812.25])
def test_scales_against_the_formula(pcp, b, q):
    got = pcp.sift_scales(b, q)
    want = sk.scales(b, q)
    assert got.shape == (q + 3,)
    assert np.all(np.abs(got - want) <= np.spacing(want))           # pow is within an ulp on either side
    assert got[1] == b and got[q + 1] == 2.0 * b                    # pow(2, 0) and pow(2, 1) are exact: the octave's ends, to the bit
    assert np.all(np.diff(got) > 0)


def test_scales_refuse_what_the_rules_do(pcp):
    L = pcp._lib
    out = np.full(20, -7.0)
    for q in (0, -1, 14, 100):
        assert L.lib().pcr_sift_scales(0.1, q, L.dptr(out)) == L.PCR_E_UNSUPPORTED
    for b in (0.0, -1.0, np.inf, np.nan):
        assert L.lib().pcr_sift_scales(b, 3, L.dptr(out)) == L.PCR_E_INVALID
    assert L.lib().pcr_sift_scales(0.1, 3, None) == L.PCR_E_INVALID
    assert (out == -7.0).all()


# ------------------------------------------------------------------------------------------------ the rules on hand-made tables
def test_lattice_neighbourhood_is_what_the_tables_assume():
    P = sk.lattice()
    assert P.shape == (144, 3) and np.array_equal(P[sk.LATTICE_ROW], [2, 2, 1]) and sk.lattice_row(2, 2, 1) == sk.LATTICE_ROW
    d2 = sk.dist2(P)[sk.LATTICE_ROW]
    assert (np.flatnonzero(d2 == 3) == sk.LATTICE_CORNERS).all()
    assert [(d2 == v).sum() for v in (0, 1, 2)] == [1, 6, 12]
    nb, gap = sk.neighbours(d2)
    assert len(nb) == 25 and gap == 0.0
    assert set(sk.LATTICE_CORNERS[:6]) <= set(nb.tolist()) and not set(sk.LATTICE_CORNERS[6:]) & set(nb.tolist())


@pytest.mark.parametrize("name", list(sk.lattice_tables()))
def test_extrema_tie_rules(name):
    D, contrast, want = sk.lattice_tables()[name]
    got, m = sk.extrema(sk.lattice(), D, contrast)
    assert np.array_equal(got, want), name
    assert np.array_equal(D, np.rint(D))


def test_extrema_contrast_is_inclusive_and_on_the_magnitude():
    P = sk.lattice()
    D = np.zeros((144, 3))
    D[sk.LATTICE_ROW] = [0, -2, 0]
    assert len(sk.extrema(P, D, 2.0)[0]) == 1            # |val| >= contrast
    assert len(sk.extrema(P, D, np.nextafter(2.0, 3.0))[0]) == 0
    # fewer than 25 rows: N(i) is every row
    few = P[:24]
    T = np.zeros((24, 3))
    T[0] = [0, 5, 0]
    T[23] = [6, 6, 6]
    assert len(sk.extrema(few, T, 1.0)[0]) == 0
    T[23] = [5, 5, 5]
    assert sk.extrema(few, T, 1.0)[0].tolist() == [[0, 1]]


def test_dog_of_two_rows_by_hand():
    # two rows a distance d apart, field y: resp_s of row 0 = (y0 + y1 w) / (1 + w), w = exp(-d^2 / (2 sigma_s^2)) while d^2 <= 9 sigma_s^2
    P = np.array([[0.0, 1.0, 0.0], [0.3, 1.5, 0.4]])
    d2 = (0.3 * 0.3 + 0.5 * 0.5) + 0.4 * 0.4
    sig = sk.scales(0.2, 2)
    D, counts, info = sk.dog(P, 1, sig)
    resp = []
    for s in sig:
        w = np.exp(d2 * (-0.5 / (s * s))) if d2 <= 9.0 * (s * s) else 0.0
        resp.append((1.0 + 1.5 * w) / (1.0 + w))
    assert np.allclose(D[0], np.diff(resp), rtol=0, atol=1e-15)
    assert counts.tolist() == [2, 2] and D.shape == (2, 4)
    assert resp[0] == 1.0 and resp[1] == 1.0 and resp[2] > 1.0      # the two smallest scales do not reach the other row
    assert info["V"].tolist() == [1.5, 1.5]


# ------------------------------------------------------------------------------------------------ the conditions of the GPU cases
BOUND_X1000 = 1e-9     # every margin must exceed it; the bound on D at these shapes is < 1e-12


@pytest.fixture(scope="module")
def seeded8(og):
    """The seeded case through 8 octaves with the restated mode-2 filter (bit-equal to the device's: tests/test_gpu_global_init.py)."""
    return sk.sift(sk.seeded_case(), sk.SEEDED["min_scale"], 8, sk.SEEDED["q"], sk.SEEDED["contrast"], downsample=og.voxel_down_sample)


def test_seeded_case_meets_its_conditions(seeded8):
    r = seeded8
    run = r["sizes"] > 0
    assert run.tolist() == [True] * 4 + [False] * 4                  # 8 octaves asked for: the fifth cloud falls under 25 rows
    assert 1500 < r["sizes"][0] < 3000 and r["sizes"][3] >= 25
    first3 = r["octave"] < sk.SEEDED["n_octaves"]
    assert first3.sum() >= 10 and len(np.unique(r["octave"][first3])) >= 2
    whole = [bool((o["counts"] == len(o["cloud"])).all()) for o in r["octaves"]]
    assert any(whole), whole                                         # an octave whose every ball is the whole cloud
    assert not whole[0]
    for k, o in enumerate(r["octaves"]):
        assert sk.bound(o["info"]).max() < 1e-12, k
        assert sk.min_margin(o["info"], o["margins"]) > BOUND_X1000, (k, o["margins"], o["info"]["lim_margin"])
        assert (o["counts"][o["margins"]["candidates"]] >= 25).all()   # (the list's way is the sparse case's)
    balls = r["octaves"][0]["counts"]
    assert 100 < np.median(balls) < 400 and balls.max() < 1000


def test_sparse_case_meets_its_conditions():
    P = sk.sparse_case()
    o = sk.octave(P, **sk.SPARSE)
    assert 55 <= len(P) <= 70
    cand = o["margins"]["candidates"]
    short = o["counts"][cand] < 25
    assert short.any() and (~short).any()                            # both ways are taken
    assert (o["counts"][o["entries"][:, 0]] < 25).any()              # and an entry comes from the list's way
    assert (o["counts"] < 25).sum() >= 10
    assert sk.min_margin(o["info"], o["margins"]) > BOUND_X1000


@pytest.mark.parametrize("n", [24, 25, 26, 63, 64, 65, 129, 257])
def test_one_ball_cases_meet_their_conditions(n):
    o = sk.octave(sk.one_ball_case(n), 1.0, 3, 0.0)
    assert (o["counts"] == n).all()
    assert np.ptp(o["cloud"], axis=0).max() < 3.0 * sk.scales(1.0, 3)[-1]      # inside one cell of the grid
    assert len(o["entries"]) >= 1
    m = dict(o["margins"], contrast=np.inf)                          # (contrast 0: every value passes)
    assert sk.min_margin(o["info"], m) > BOUND_X1000
