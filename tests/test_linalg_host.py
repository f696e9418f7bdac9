"""The HOST build of the 3x3 / 6x6 solves of csrc/pcr_linalg.h through pcr_debug_linalg(NULL, ...): every family of
tests/linalg_checks.py against the 60-digit reference, within max(8 x LAPACK's worst value in the family, 1e-14).  No GPU needed;
tests/test_gpu_linalg.py holds the device build to the same families and bounds."""
import os
import re

import numpy as np
import pytest

from tests import linalg_checks as K
from tests.conftest import ROOT

OPS = (0, 1, 2, 3, 4, 5)


@pytest.mark.parametrize("op", OPS)
def test_every_family_within_the_bounds(pcp, capsys, op):
    out, bad, w = K.run_op(pcp._lib, None, op)
    yard = K.OPS[3 if op == 4 else op]
    with capsys.disabled():   # the yardstick's worst value per family and metric, then the host build's with its bound
        print("\n" + K.table(f"op {op}: LAPACK (NumPy binary64)", K.worst(yard._yard(), (yard._yard_problems or yard._problems)())))
        print(K.table(f"op {op}: host build", w, yard.bounds(), K.KABSCH_BOUND_OF if op == 4 else None))
    assert not bad, bad


def test_what_the_polar_metric_leaves_out():
    """sigma_3 > 1e-6 sigma_1 holds for every problem of the full-rank families and for none of the rank-deficient ones, by
    construction; the same for the device, whose cases are chosen by the reference."""
    share = K.left_out(K.svd_yardstick(), K.svd_problems(), "polar")
    assert all(share[f] == 0.0 for f in K.SVD_FULL), share
    assert all(share[f] == 1.0 for f in K.SVD_DEFICIENT), share
    P, src = K.svd_warm_problems()
    assert len(P.inp) <= 800 and len(K.svd_problems().inp) <= 800
    assert set(K.base(f) for f in P.names) == {"threshold", "close"} and len(P.names) == 8
    assert not np.isnan(K.svd_yardstick()["polar"][src]).any()
    # ops 3 / 4: R and t are compared where the rotation is determined, the points elsewhere; every problem has one of the two
    y = K.kabsch_yardstick()
    P3 = K.kabsch_problems()[0]
    assert (np.isnan(y["R"]) != np.isnan(y["points"])).all() and np.array_equal(np.isnan(y["R"]), np.isnan(y["t"]))
    share = K.left_out(y, P3, "R")
    assert share["mirrored"] < 0.25 and share["exact"] < 0.25 and share["coplanar"] == 1.0 and share["collinear"] == 1.0, share
    assert not np.isnan(y["cost"]).any() and not np.isnan(y["orth"]).any()


def test_threshold_family_walks_both_clauses_of_the_sweep_test():
    """svd3_rotate's `rotated` test restated on the column pairs of every threshold matrix as given: the family holds pairs that are
    orthogonal to working precision, pairs on either side of the first clause (g^2 >= 1e-16 a b) and, below it, on either side of
    the second (g^2 >= 1e-32 a b with a sine of 1e-8 or more)."""
    P = K.svd_problems()
    seen = set()
    for i in P.rows_of("threshold"):
        A = P.inp[i].reshape(3, 3)
        for p, q in ((0, 1), (0, 2), (1, 2)):
            a, b, g = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
            if g == 0.0 or g * g <= 1e-34 * a * b:
                seen.add("orthogonal")
                continue
            d, gg = b - a, 2 * abs(g)
            h = np.hypot(d, gg)
            c2 = 0.5 + 0.5 * abs(d) / h
            s2 = (0.5 * gg / h) ** 2 / c2
            first, second = g * g >= 1e-16 * a * b, g * g >= 1e-32 * a * b and s2 >= 1e-16
            seen.add("first" if first else "second" if second else "neither")
    assert seen == {"orthogonal", "first", "second", "neither"}, seen


def test_argument_errors(pcp):
    L = pcp._lib
    f = L.lib().pcr_debug_linalg
    inp, out = np.zeros(64), np.full(64, 7.0)
    assert f(None, 0, L.dptr(inp), 0, L.dptr(out)) == L.PCR_OK and (out == 7.0).all()   # n == 0: nothing written
    for op in (-1, 6, 100):
        assert f(None, op, L.dptr(inp), 1, L.dptr(out)) == L.PCR_E_INVALID
    for n in (-1, 65537, 2**40):
        assert f(None, 0, L.dptr(inp), n, L.dptr(out)) == L.PCR_E_INVALID
    assert f(None, 0, None, 1, L.dptr(out)) == L.PCR_E_INVALID
    assert f(None, 0, L.dptr(inp), 1, None) == L.PCR_E_INVALID
    assert (out == 7.0).all()
    big = np.zeros((65536, 9))   # the largest legal n
    big[:, ::4] = 1.0
    res = K.solve(L, None, 0, big)
    assert np.array_equal(res[:, 9:12], np.ones((65536, 3)))


def test_header_declares_the_symbol_and_the_binding_has_it(pcp):
    L = pcp._lib
    txt = open(os.path.join(ROOT, "include", "pcr.h")).read()
    assert re.search(r"PCR_API\s+int\s+pcr_debug_linalg\s*\(\s*pcr_ctx\*\s*ctx,\s*int\s+op,\s*const\s+double\*\s*in,\s*int64_t\s+n,\s*double\*\s*out\)", txt)
    assert "pcr_debug_linalg" in L.SIGNATURES and hasattr(L.lib(), "pcr_debug_linalg")
    assert len(L.SIGNATURES["pcr_debug_linalg"][1]) == 5


def test_a_lane_alone_returns_the_bytes_of_the_batch(pcp):
    """(host build: trivially a loop -- this pins the checks module's sampling, which the GPU test uses)"""
    for op in OPS:
        inp, P = K.inputs_of(op)
        whole = K.solve(pcp._lib, None, op, inp)
        rows = K.sample_rows(P, 16)
        assert all(len(set(rows) & set(P.rows_of(f).tolist())) == min(16, len(P.rows_of(f))) for f in P.names)
        for i in rows:
            assert K.solve(pcp._lib, None, op, inp[i]).tobytes() == whole[i].tobytes(), (op, i)


def test_association_sets_are_what_their_names_say(pcp):
    """The end-to-end sets of tests/test_gpu_linalg.py: rank and determinant by the 60-digit Procrustes of the pairs, and the host
    route (pcr_procrustes) on each."""
    sets = K.association_sets()   # (asserts spacing, distances and the unique nearest neighbour)
    assert set(sets) == {"collinear", "coplanar", "mirrored", "cube"}
    for name, (src, tgt) in sets.items():
        A, B = src.astype(np.float64), tgt.astype(np.float64)
        R, t, S = K.procrustes_mp(A, B)
        det = float(np.linalg.det(R.astype(np.float64)))
        if name == "collinear":
            assert S[1] < 1e-30 * S[0]
        if name == "coplanar":
            assert S[1] > 0.1 * S[0] and S[2] < 1e-30 * S[0]
        if name == "mirrored":
            assert S[2] > 1e-6 * S[0] and abs(det + 1.0) < 1e-12
        if name == "cube":
            assert S[0] - S[2] < 1e-5 * S[0] and abs(det - 1.0) < 1e-12
        Rh, th, _ = pcp.procrustes_transformation(A.T, B.T)
        err, orth_err = K.check_on_points(Rh, th.reshape(3), A, R, t, name)
        assert err < K.POINT_BAR and orth_err <= K.orth_bound(A, B), (name, err, orth_err)
