"""The DEVICE build of the 3x3 / 6x6 solves of csrc/pcr_linalg.h (reciprocal square roots, contraction, completions written as
selects) through pcr_debug_linalg, one problem per lane: the families and bounds of tests/linalg_checks.py, which
tests/test_linalg_host.py holds the host build to.  Then the same edges through the code that really finishes an ICP pass: one
Procrustes step of pcr_icp / pcr_icp_batch on association sets that are collinear, coplanar, mirrored or a cube's corners.

Measured on the MI355X: the device build stays within 2.3e-15 on every metric of every family (bounds: 1e-14 to 7.6e-14), the ICP
legs within 5.9e-15 on the points; DESIGN section 4.1 "3x3 solves on the device" has the table per family, and the tests print
each figure next to its bound before they assert.
"""
import numpy as np
import pytest

from tests import icp_loop_checks as LOOP
from tests import linalg_checks as K
from tests.test_gpu_icp_loop import run_driver

pytestmark = pytest.mark.gpu

GATE = 0.25   # squared: every source point is within 0.1 of its own target, every other target 0.9 or more away
# route -> (driver of tests/test_gpu_icp_loop.py, max_d2); pcr_icp_step.h lists the callers of the step
ROUTES = {"grid index, gated, one-launch pass": ("D1", GATE),
          "grid index, ungated (max_d2 = 0)": ("D4", 0.0),
          "grid index, ungated (max_d2 = inf)": ("D4", float("inf")),
          "fused batch": ("D7", GATE),
          "brute-force index (host build of the step)": ("D6", GATE)}


@pytest.mark.parametrize("op", (0, 1, 2, 3, 4, 5))
def test_device_build_within_the_bounds(pcp, ctx, capsys, op):
    L = pcp._lib
    live = ctx.arena_live()
    out, bad, w = K.run_op(L, ctx.handle, op)
    yard = K.OPS[3 if op == 4 else op]
    with capsys.disabled():   # (printed before anything is asserted)
        print("\n" + K.table(f"op {op}: device build", w, yard.bounds(), K.KABSCH_BOUND_OF if op == 4 else None))
    assert not bad, bad
    # two batched calls return the same bytes
    assert K.raw_op(L, ctx.handle, op).tobytes() == out.tobytes()
    # a lane's result does not depend on its neighbours' branches: alone in its wave, a problem returns the bytes it has in the batch
    inp, P = K.inputs_of(op)
    for i in K.sample_rows(P, 16):
        assert K.solve(L, ctx.handle, op, inp[i]).tobytes() == out[i].tobytes(), (op, P.family[i], i)
    assert ctx.arena_live() == live


def test_device_argument_errors_and_the_largest_batch(pcp, ctx):
    L = pcp._lib
    f = L.lib().pcr_debug_linalg
    live = ctx.arena_live()
    inp, out = np.zeros(64), np.full(64, 7.0)
    assert f(ctx.handle, 0, L.dptr(inp), 0, L.dptr(out)) == L.PCR_OK
    for op, n in ((-1, 1), (6, 1), (0, -1), (0, 65537)):
        assert f(ctx.handle, op, L.dptr(inp), n, L.dptr(out)) == L.PCR_E_INVALID
    assert f(ctx.handle, 0, None, 1, L.dptr(out)) == L.PCR_E_INVALID and f(ctx.handle, 0, L.dptr(inp), 1, None) == L.PCR_E_INVALID
    assert (out == 7.0).all()
    # 65536 problems, and 65 (a second block with one lane): every row written, the rows past n untouched
    P = K.svd_problems()
    big = np.tile(P.inp, (65536 // len(P.inp) + 1, 1))[:65536]
    res = K.solve(L, ctx.handle, 0, big)
    first = K.solve(L, ctx.handle, 0, P.inp)
    assert np.isfinite(res).all() and res[:len(P.inp)].tobytes() == first.tobytes() and res[-len(P.inp):].tobytes() == K.solve(L, ctx.handle, 0, big[-len(P.inp):]).tobytes()
    guard = np.full((66, K.OUT[0]), 7.0)
    assert f(ctx.handle, 0, L.dptr(np.ascontiguousarray(P.inp[:65])), 65, L.dptr(guard)) == L.PCR_OK
    assert guard[:65].tobytes() == first[:65].tobytes() and (guard[65] == 7.0).all()
    assert ctx.arena_live() == live


@pytest.mark.parametrize("name", ("collinear", "coplanar", "mirrored", "cube"))
def test_one_icp_step_on_a_degenerate_association_set(pcp, monkeypatch, capsys, name):
    """pcr_icp with max_iter = 1, compat mode, identity T0: T is the Procrustes step of the pairs (source point, its own target).
    collinear: rank 1, svd3_complete_two; coplanar: rank 2, svd3_complete_one; mirrored: the best orthogonal map has determinant -1
    and is returned as it is (main.py:137-139 applies no reflection fix); cube: three equal singular values."""
    src, tgt = K.association_sets()[name]
    A, B = src.astype(np.float64), tgt.astype(np.float64)
    R_ref, t_ref, _ = K.procrustes_mp(A, B)
    bound = K.orth_bound(A, B)
    lines, failures = [], []
    for route, (driver, max_d2) in ROUTES.items():
        case = LOOP.Case(f"{name}: {route}", src, dict(max_iter=1, max_d2=max_d2, **LOOP.OFF), tgt=tgt)
        r = run_driver(pcp, monkeypatch, driver, case, "compat", "frobenius")   # (asserts that this driver is the one that ran)
        assert (r["iters"], r["status"], r["n_assoc"], r["passes"]) == (1, 0, len(src), 1), (name, route, r["iters"], r["status"], r["n_assoc"])
        T = r["T"]
        assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
        err, orth_err = K.check_on_points(T[:3, :3], T[:3, 3], A, R_ref, t_ref, (name, route))
        lines.append(f"  {name:10s} {route:44s} |R a + t - ref| {err:.2e}   |R^T R - I| {orth_err:.2e}   bound {bound:.2e}")
        if not (err < K.POINT_BAR and orth_err <= bound):
            failures.append((route, err, orth_err, bound))
        if name == "mirrored":
            assert np.linalg.det(T[:3, :3]) < -0.5, (route, "the reflection was fixed")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not failures, failures
