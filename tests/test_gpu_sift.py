"""GPU: SIFT-3D keypoints (pcr_sift_octave, pcr_sift_extrema, pcr_sift / pcl_keypoints.py) against the NumPy restatement of the rules,
tests/sift_checks.py.  PARITY UNPINNED: the restatement restates include/pcr.h, not PCL's binary32 output.

The table D.  d2 and the argument d2 * h_s are the same bits on both sides (the same binary64 operations in the same order), so the
membership of every sum is the same.  OpenCL's binary64 exp is within 3 ulp and the host's within 1, so a weight differs by
<= 4 2^-52 relative; the product v_j * w rounds once on each side (2^-52 together); each of num and den is a sum of K non-negative-weight
terms in another order, <= (K - 1) 2^-53 of sum |v_j| w per side.  With V = max |v_j| over the ball:
    |d num| <= (K + 4) 2^-52 V den,   |d den| <= (K + 3) 2^-52 den,
    |d resp_s| <= |d num| / den + |resp| |d den| / den + 2^-52 |resp| <= (2 K + 8) 2^-52 V <= 2 V (K + 8) 2^-52,
and D is the difference of two of them (its own rounding, 2^-52 * 2 V for both sides, is inside the slack of 16 V 2^-52):
    |d D| <= 4 V (K + 8) 2^-52     per entry, K and V of the row from the restatement (K of the largest scale bounds every scale's).
About 1.4e-12 at V = 4 and K = 400.  Measured on an MI355X: DESIGN.md, the SIFT section.

The entries.  From the DEVICE'S OWN table through the restatement's `extrema` every decision is taken on the same bits: equal exactly,
whatever the margins.  From the restatement's own table they are equal exactly because tests/test_sift_host.py shows every decision margin
of these cases above 1e-9, a thousand times the bound."""
import ctypes as C

import numpy as np
import pytest

from tests import sift_checks as sk
from tests.test_gpu_fpfh_rows import _states

pytestmark = pytest.mark.gpu


def octave_abi(pcp, ctx, cloud, base, q, contrast, field=1, *, capacity=None, want_rows=True, want_dog=True, check=True):
    """pcr_sift_octave itself -> (status, D (n, q + 2), counts (n,), entries (K, 2), n_out); outputs not written keep -7."""
    L = pcp._lib
    own = None
    if not isinstance(cloud, pcp.DeviceCloud):
        cloud = own = pcp.DeviceCloud.upload(np.ascontiguousarray(cloud, dtype=np.float64), ctx)
    n = cloud.n
    cap = n * 7 if capacity is None else capacity
    D = np.full((n, max(q, 0) + 2), -7.0)
    counts = np.full(n, -7, dtype=np.int32)
    rows, cols = np.full(max(cap, 1), -7, dtype=np.int32), np.full(max(cap, 1), -7, dtype=np.int32)
    nk = C.c_int64(-7)
    try:
        st = L.lib().pcr_sift_octave(ctx.handle, cloud.handle, float(base), int(q), float(contrast), int(field), L.dptr(D) if want_dog else None,
                                     L.iptr(counts) if want_dog else None, L.iptr(rows) if want_rows else None, L.iptr(cols) if want_rows else None, cap,
                                     C.byref(nk) if want_rows else None)
    finally:
        if own is not None:
            own.free()
    if check:
        L.check(st, ctx.handle, soft=())
    k = nk.value if 0 <= nk.value <= cap else 0
    assert (rows[k:] == -7).all() and (cols[k:] == -7).all()
    return st, D, counts, np.c_[rows[:k], cols[:k]].astype(np.int64), nk.value


def check_octave(pcp, ctx, P, base, q, contrast, field=1, *, margins=True):
    """One octave on the device against the restatement -> (restatement, device D, max |dD| / bound)."""
    sig = pcp.sift_scales(base, q)
    assert np.all(np.abs(sig - sk.scales(base, q)) <= np.spacing(sig))
    ref = sk.octave(P, base, q, contrast, field, sig)
    _, D, counts, entries, k = octave_abi(pcp, ctx, P, base, q, contrast, field)
    assert np.array_equal(counts, ref["counts"])
    assert np.isfinite(D).all()
    err = np.abs(D - ref["D"]).max(axis=1)
    bound = sk.bound(ref["info"])
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"n={len(P)} q={q} field={field}: max |dD| = {err.max():.3g}, bound there = {bound[err.argmax()]:.3g}, max ratio = {ratio:.3g}, entries = {k}")
    assert (err <= bound).all(), (err.max(), ratio)
    own, _ = sk.extrema(P, D, contrast)                              # the device's own table through the restatement: the same bits decide
    assert np.array_equal(entries, own)
    if margins:
        assert np.array_equal(entries, ref["entries"])               # and the restatement's own table: no entry left out, none added
    return ref, D, entries


# ------------------------------------------------------------------------------------------------ A, H: the seeded case
@pytest.fixture(scope="module")
def seeded(pcp):
    P = sk.seeded_case()
    ref = sk.sift(P, sk.SEEDED["min_scale"], 8, sk.SEEDED["q"], sk.SEEDED["contrast"], downsample=pcp.voxel_down_sample, scales_of=pcp.sift_scales)
    return P, ref


@pytest.mark.parametrize("o", [0, 1, 2])
def test_a_seeded_octaves(pcp, ctx, seeded, o):
    _, ref = seeded
    cloud = ref["octaves"][o]["cloud"]
    got, _, entries = check_octave(pcp, ctx, cloud, sk.SEEDED["min_scale"] * 2.0 ** o, sk.SEEDED["q"], sk.SEEDED["contrast"])
    assert np.array_equal(got["D"], ref["octaves"][o]["D"])          # (the restatement is repeatable)
    assert len(entries) >= 5


def sift_abi(pcp, ctx, cloud, min_scale, n_octaves, q, contrast, field=1, capacity=4096):
    L = pcp._lib
    kp = np.full((capacity, 4), -7.0)
    octave, row = np.full(capacity, -7, dtype=np.int32), np.full(capacity, -7, dtype=np.int32)
    sizes = np.full(max(n_octaves, 1), -7, dtype=np.int64)
    nk = C.c_int64(-7)
    st = L.lib().pcr_sift(ctx.handle, cloud.handle, float(min_scale), int(n_octaves), int(q), float(contrast), int(field), L.dptr(kp), L.iptr(octave), L.iptr(row),
                          capacity, C.byref(nk), L.lptr(sizes))
    return st, kp, octave, row, sizes, nk.value


@pytest.mark.parametrize("n_octaves", [1, 3, 8])
def test_h_octave_loop(pcp, ctx, seeded, n_octaves):
    P, ref8 = seeded
    keep = ref8["octave"] < n_octaves
    want_kp, want_oct, want_row, want_col = ref8["keypoints"][keep], ref8["octave"][keep], ref8["row"][keep], ref8["column"][keep]
    want_sizes = np.where(np.arange(8) < n_octaves, ref8["sizes"], 0)[:n_octaves]
    if n_octaves == 8:
        assert (want_sizes[:4] >= 25).all() and (want_sizes[4:] == 0).all()      # stops where the cloud falls under 25 rows
    cloud = pcp.DeviceCloud.upload(P, ctx)
    try:
        st, kp, octave, row, sizes, k = sift_abi(pcp, ctx, cloud, sk.SEEDED["min_scale"], n_octaves, sk.SEEDED["q"], sk.SEEDED["contrast"])
        assert st == 0 and k == len(want_kp) >= (10 if n_octaves > 1 else 5)
        assert np.array_equal(sizes, want_sizes)
        assert np.array_equal(octave[:k], want_oct) and np.array_equal(row[:k], want_row)
        assert np.array_equal(kp[:k], want_kp)                        # positions are the octave's rows and scales the table's, to the bit
        assert (kp[k:] == -7.0).all() and (octave[k:] == -7).all()
        # the Python layer, from the device cloud and from the host array
        for src in (cloud, P, P.tolist()):
            xyz, scales, det = pcp.sift_keypoints(src, sk.SEEDED["min_scale"], n_octaves, sk.SEEDED["q"], sk.SEEDED["contrast"], return_scales=True,
                                                  return_details=True, ctx=ctx)
            assert xyz.dtype == np.float32 and np.array_equal(xyz, want_kp[:, :3].astype(np.float32))
            assert np.array_equal(scales, want_kp[:, 3])
            assert np.array_equal(det["octave"], want_oct) and np.array_equal(det["row"], want_row) and np.array_equal(det["column"], want_col)
            assert np.array_equal(det["octave_sizes"], want_sizes)
        assert np.array_equal(pcp.sift_keypoints(cloud, sk.SEEDED["min_scale"], n_octaves, sk.SEEDED["q"], sk.SEEDED["contrast"], ctx=ctx), xyz)
        # capacity: the needed number, nothing written, and the Python layer's second call
        st, kp, octave, row, sizes, k2 = sift_abi(pcp, ctx, cloud, sk.SEEDED["min_scale"], n_octaves, sk.SEEDED["q"], sk.SEEDED["contrast"], capacity=k - 1)
        assert st == pcp._lib.PCR_E_UNSUPPORTED and k2 == k and (kp == -7.0).all() and (octave == -7).all() and (row == -7).all()
        assert np.array_equal(sizes, want_sizes)
    finally:
        cloud.free()


def test_h_capacity_retry_of_the_python_layer(pcp, ctx):
    # the first buffer holds n entries; a row can be an extremum at several columns, so more can be needed: the second call takes the
    # needed number.  Reached here through a small first buffer.
    calls = []

    def call(capacity):
        calls.append(capacity)
        return (pcp._lib.PCR_E_UNSUPPORTED, 9) if capacity < 9 else (0, 9)
    assert pcp.pcl_keypoints._with_capacity(call, 4) == (0, 9) and calls == [4, 9]


# ------------------------------------------------------------------------------------------------ B: one ball, one cell
@pytest.mark.parametrize("n", [24, 25, 26, 63, 64, 65, 129, 257])
def test_b_one_ball_holds_the_cloud(pcp, ctx, n):
    ref, _, entries = check_octave(pcp, ctx, sk.one_ball_case(n), 1.0, 3, 0.0)
    assert (ref["counts"] == n).all() and len(entries) >= 1


@pytest.mark.parametrize("n", [2048, 2049])
def test_b_ball_at_and_beyond_the_stage(pcp, ctx, n):
    # the extrema kernel stages a ball of up to SIFT_STAGE = 2048 rows in LDS; a larger one takes the list's way
    ref, D, entries = check_octave(pcp, ctx, sk.one_ball_case(n), 1.0, 3, 0.0, margins=False)
    assert (ref["counts"] == n).all() and len(entries) >= 1
    if sk.min_margin(ref["info"], dict(ref["margins"], contrast=np.inf)) > 1e-9:
        assert np.array_equal(entries, ref["entries"])


# ------------------------------------------------------------------------------------------------ C: sparse, the list's way
def test_c_sparse_candidates_take_the_list(pcp, ctx):
    P = sk.sparse_case()
    ref, _, entries = check_octave(pcp, ctx, P, **sk.SPARSE)
    cand = ref["margins"]["candidates"]
    assert (ref["counts"][cand] < 25).any() and (ref["counts"][entries[:, 0]] < 25).any() and (ref["counts"][entries[:, 0]] >= 25).any()
    # fewer than 25 rows in all: N(i) is every row, wherever it lies
    few = P[np.r_[0:7, 33:40, 7:15]]
    assert len(few) == 22
    check_octave(pcp, ctx, few, **sk.SPARSE)


# ------------------------------------------------------------------------------------------------ D: the tie rules on crafted tables
def extrema_abi(pcp, ctx, cloud, D, contrast, capacity=None):
    L = pcp._lib
    D = np.ascontiguousarray(D, dtype=np.float64)
    cap = len(D) * 7 if capacity is None else capacity
    rows, cols = np.full(max(cap, 1), -7, dtype=np.int32), np.full(max(cap, 1), -7, dtype=np.int32)
    nk = C.c_int64(-7)
    st = L.lib().pcr_sift_extrema(ctx.handle, cloud.handle, L.dptr(D), D.shape[1], float(contrast), L.iptr(rows), L.iptr(cols), cap, C.byref(nk))
    k = nk.value if 0 <= nk.value <= cap else 0
    return st, np.c_[rows[:k], cols[:k]].astype(np.int64), nk.value


def test_d_tie_rules_on_the_lattice(pcp, ctx):
    P = sk.lattice()
    cloud = pcp.DeviceCloud.upload(P, ctx)
    try:
        for name, (D, contrast, want) in sk.lattice_tables().items():
            st, got, k = extrema_abi(pcp, ctx, cloud, D, contrast)
            assert st == 0 and np.array_equal(got, want), name
            r, c = pcp.sift_extrema(cloud, D, contrast, ctx=ctx)
            assert np.array_equal(np.c_[r, c], want), name
        # a table of many entries, wide: random integers, ties everywhere
        rng = np.random.default_rng(5)
        for C_ in (3, 6, 15):
            D = rng.integers(-3, 4, (144, C_)).astype(np.float64)
            want, _ = sk.extrema(P, D, 1.0)
            st, got, k = extrema_abi(pcp, ctx, cloud, D, 1.0)
            assert st == 0 and np.array_equal(got, want) and (C_ == 3 or len(want) >= 3), C_
            st, got, k2 = extrema_abi(pcp, ctx, cloud, D, 1.0, capacity=k - 1) if k else (pcp._lib.PCR_E_UNSUPPORTED, got, k)
            assert st == pcp._lib.PCR_E_UNSUPPORTED and k2 == k
    finally:
        cloud.free()


def test_d_extrema_of_a_stretched_cloud_take_both_ways(pcp, ctx):
    # rows along a line with growing gaps: whatever ball the call chooses, some hold 25 rows and some do not
    rng = np.random.default_rng(11)
    x = np.cumsum(np.geomspace(0.001, 4000.0, 300))
    P = np.c_[x, rng.normal(0, 1e-3, 300), rng.normal(0, 1e-3, 300)]
    D = rng.integers(-4, 5, (300, 5)).astype(np.float64)
    want, _ = sk.extrema(P, D, 2.0)
    cloud = pcp.DeviceCloud.upload(P, ctx)
    try:
        st, got, k = extrema_abi(pcp, ctx, cloud, D, 2.0)
    finally:
        cloud.free()
    assert st == 0 and len(want) >= 5 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ E: parameter edges
@pytest.fixture(scope="module")
def patch():
    rng = np.random.default_rng(21)
    return rng.uniform(0.0, 1.0, (300, 3)) * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 0.01, (300, 3))


@pytest.mark.parametrize("q", [1, 13])
def test_e_fewest_and_most_scales(pcp, ctx, patch, q):
    ref, D, entries = check_octave(pcp, ctx, patch, 0.05, q, 1e-4, margins=False)
    assert D.shape == (300, q + 2)
    if sk.min_margin(ref["info"], ref["margins"]) > 1e-9:
        assert np.array_equal(entries, ref["entries"])


@pytest.mark.parametrize("field", [0, 1, 2])
def test_e_every_field(pcp, ctx, patch, field):
    ref, D, entries = check_octave(pcp, ctx, patch, 0.05, 3, 0.0, field, margins=False)
    assert len(entries) >= 1
    rows, cols, info = pcp.sift_octave(patch, 0.05, 3, 0.0, field="xyz"[field], ctx=ctx)
    assert np.array_equal(np.c_[rows, cols], entries) and np.array_equal(info["dog"], D) and np.array_equal(info["counts"], ref["counts"])


def test_e_contrast_edges(pcp, ctx, patch):
    st, D, counts, entries, k = octave_abi(pcp, ctx, patch, 0.05, 3, 1e9)
    assert st == 0 and k == 0 and len(entries) == 0 and np.isfinite(D).all()
    st, D0, _, entries0, k0 = octave_abi(pcp, ctx, patch, 0.05, 3, 0.0)
    assert np.array_equal(D0, D) and k0 >= 1
    assert np.array_equal(entries0, sk.extrema(patch, D0, 0.0)[0])


# ------------------------------------------------------------------------------------------------ F: cloud states, repeated calls
def test_f_every_cloud_state_gives_the_fresh_upload_s_bytes(pcp, ctx):
    rng = np.random.default_rng(4)
    pts = rng.uniform(0.0, 1.0, (1500, 3)) * np.array([1.0, 0.3, 1.0])
    before = ctx.arena_live()
    for name, cloud in _states(pcp, ctx, pts):
        X = cloud.download()
        _, D, counts, entries, k = octave_abi(pcp, ctx, cloud, 0.04, 3, 1e-4)
        _, D2, counts2, entries2, _ = octave_abi(pcp, ctx, cloud, 0.04, 3, 1e-4)
        _, Df, countsf, entriesf, _ = octave_abi(pcp, ctx, X, 0.04, 3, 1e-4)
        cloud.free()
        assert k >= 1, name
        assert D.tobytes() == D2.tobytes() == Df.tobytes(), name
        assert np.array_equal(counts, countsf) and np.array_equal(counts, counts2), name
        assert np.array_equal(entries, entriesf) and np.array_equal(entries, entries2), name
    assert ctx.arena_live() == before


# ------------------------------------------------------------------------------------------------ G: capacity
def test_g_capacity(pcp, ctx, patch):
    L = pcp._lib
    _, D, counts, entries, k = octave_abi(pcp, ctx, patch, 0.05, 3, 0.0)
    assert k >= 2
    st, D1, counts1, e1, k1 = octave_abi(pcp, ctx, patch, 0.05, 3, 0.0, capacity=k - 1, check=False)
    assert st == L.PCR_E_UNSUPPORTED and k1 == k and len(e1) == 0    # (octave_abi asserts that nothing was written to rows / columns)
    assert np.array_equal(D1, D) and np.array_equal(counts1, counts)  # the per-row outputs are complete
    st, _, _, e2, k2 = octave_abi(pcp, ctx, patch, 0.05, 3, 0.0, capacity=k)
    assert st == 0 and np.array_equal(e2, entries)
    st, Dn, cn, e3, k3 = octave_abi(pcp, ctx, patch, 0.05, 3, 0.0, want_dog=False)
    assert st == 0 and np.array_equal(e3, entries) and (Dn == -7.0).all() and (cn == -7).all()
    st, D4, c4, _, _ = octave_abi(pcp, ctx, patch, 0.05, 3, 0.0, want_rows=False)
    assert st == 0 and np.array_equal(D4, D) and np.array_equal(c4, counts)
    st, _, _, e0, k0 = octave_abi(pcp, ctx, patch, 0.05, 3, 0.0, capacity=0, check=False)
    assert st == L.PCR_E_UNSUPPORTED and k0 == k


# ------------------------------------------------------------------------------------------------ I: refused arguments
def test_i_refused_arguments_launch_nothing(pcp, ctx, patch):
    L = pcp._lib
    lib = L.lib()
    cloud = pcp.DeviceCloud.upload(patch, ctx)
    n = cloud.n
    D = np.full((n, 5), -7.0)
    counts = np.full(n, -7, dtype=np.int32)
    rows, cols = np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32)
    kp = np.full((64, 4), -7.0)
    sizes = np.full(3, -7, dtype=np.int64)
    nk = C.c_int64(-7)
    d, ic, ir, il, pk = L.dptr(D), L.iptr(counts), L.iptr(rows), L.iptr(cols), C.byref(nk)
    h, c = ctx.handle, cloud.handle
    before = ctx.arena_live()
    INV, UNS = L.PCR_E_INVALID, L.PCR_E_UNSUPPORTED
    try:
        octave = [((None, c, 0.05, 3, 0.0, 1, d, ic, ir, il, 64, pk), INV), ((h, None, 0.05, 3, 0.0, 1, d, ic, ir, il, 64, pk), INV)]
        for b in (0.0, -0.05, np.inf, np.nan):
            octave.append(((h, c, b, 3, 0.0, 1, d, ic, ir, il, 64, pk), INV))
        for mc in (np.nan, -1e-9, -np.inf):
            octave.append(((h, c, 0.05, 3, mc, 1, d, ic, ir, il, 64, pk), INV))
        for f in (-1, 3, 100):
            octave.append(((h, c, 0.05, 3, 0.0, f, d, ic, ir, il, 64, pk), INV))
        octave += [((h, c, 0.05, 3, 0.0, 1, d, ic, ir, None, 64, pk), INV), ((h, c, 0.05, 3, 0.0, 1, d, ic, ir, il, 64, None), INV),
                   ((h, c, 0.05, 3, 0.0, 1, d, ic, ir, il, -1, pk), INV), ((h, c, 0.05, 3, 0.0, 1, None, None, None, None, 0, None), INV)]
        for q in (0, -2, 14, 1000):
            octave.append(((h, c, 0.05, q, 0.0, 1, d, ic, ir, il, 64, pk), UNS))
        for args, want in octave:
            assert lib.pcr_sift_octave(*args) == want, args[2:6]
        assert b"1 .. 13" in lib.pcr_last_error(h)
        small = np.full((n, 3), -7.0)
        ds = L.dptr(small)
        extrema = [((None, c, ds, 3, 0.0, ir, il, 64, pk), INV), ((h, None, ds, 3, 0.0, ir, il, 64, pk), INV), ((h, c, None, 3, 0.0, ir, il, 64, pk), INV),
                   ((h, c, ds, 3, np.nan, ir, il, 64, pk), INV), ((h, c, ds, 3, -1.0, ir, il, 64, pk), INV), ((h, c, ds, 2, 0.0, ir, il, 64, pk), INV),
                   ((h, c, ds, 3, 0.0, None, il, 64, pk), INV), ((h, c, ds, 3, 0.0, ir, il, -1, pk), INV), ((h, c, ds, 16, 0.0, ir, il, 64, pk), UNS)]
        for args, want in extrema:
            assert lib.pcr_sift_extrema(*args) == want, args[3:5]
        pkp, io, ls = L.dptr(kp), L.iptr(counts), L.lptr(sizes)
        loop = [((None, c, 0.1, 3, 3, 0.0, 1, pkp, io, ir, 64, pk, ls), INV), ((h, None, 0.1, 3, 3, 0.0, 1, pkp, io, ir, 64, pk, ls), INV),
                ((h, c, 0.1, 0, 3, 0.0, 1, pkp, io, ir, 64, pk, ls), INV), ((h, c, 0.1, -1, 3, 0.0, 1, pkp, io, ir, 64, pk, ls), INV),
                ((h, c, 0.0, 3, 3, 0.0, 1, pkp, io, ir, 64, pk, ls), INV), ((h, c, np.nan, 3, 3, 0.0, 1, pkp, io, ir, 64, pk, ls), INV),
                ((h, c, np.inf, 3, 3, 0.0, 1, pkp, io, ir, 64, pk, ls), INV), ((h, c, 0.1, 3, 3, np.nan, 1, pkp, io, ir, 64, pk, ls), INV),
                ((h, c, 0.1, 3, 3, -0.5, 1, pkp, io, ir, 64, pk, ls), INV), ((h, c, 0.1, 3, 3, 0.0, 3, pkp, io, ir, 64, pk, ls), INV),
                ((h, c, 0.1, 3, 3, 0.0, -1, pkp, io, ir, 64, pk, ls), INV), ((h, c, 0.1, 3, 3, 0.0, 1, None, io, ir, 64, pk, ls), INV),
                ((h, c, 0.1, 3, 3, 0.0, 1, pkp, io, ir, 64, None, ls), INV), ((h, c, 0.1, 3, 3, 0.0, 1, pkp, io, ir, -1, pk, ls), INV),
                ((h, c, 0.1, 3, 0, 0.0, 1, pkp, io, ir, 64, pk, ls), UNS), ((h, c, 0.1, 3, 14, 0.0, 1, pkp, io, ir, 64, pk, ls), UNS)]
        for args, want in loop:
            assert lib.pcr_sift(*args) == want, args[2:7]
        # nothing was written, allocated or left behind
        assert (D == -7.0).all() and (counts == -7).all() and (rows == -7).all() and (cols == -7).all() and (kp == -7.0).all() and (sizes == -7).all()
        assert nk.value == -7 and ctx.arena_live() == before
        # a cloud whose extent exceeds 2^18 cells of the ball's radius is refused by the grid, with a message
        wide = pcp.DeviceCloud.upload(np.r_[patch, [[1e7, 0.0, 0.0]]], ctx)
        try:
            assert lib.pcr_sift_octave(h, wide.handle, 0.05, 3, 0.0, 1, None, None, ir, il, 64, pk) == UNS
            assert b"2^18" in lib.pcr_last_error(h)
        finally:
            wide.free()
        assert ctx.arena_live() == before
    finally:
        cloud.free()
    # PCR_E_EMPTY: no cloud of 0 rows can be made on the device (the upload refuses it with this very status, before any pcr_sift* call),
    # so the ABI's own `n <= 0` branch cannot be reached from here; what a caller sees is asserted
    for f in (lambda: pcp.sift_keypoints(np.zeros((0, 3)), ctx=ctx), lambda: pcp.sift_octave(np.zeros((0, 3)), 0.1, ctx=ctx)):
        with pytest.raises(pcp._lib.PcrError) as e:
            f()
        assert e.value.status == pcp._lib.PCR_E_EMPTY
