"""Restatements for the fused set-abstraction kernel (include/pcr.h, pcr_pn2_sa_mlp_max) in NumPy.

``fma32`` is an exact binary32 fused multiply-add; ``sa_mlp_max`` is the kernel's contract written with it (one fmaf chain per output,
k ascending, starting at the bias), so the device result can be compared bit for bit; ``sa_bound`` is the a-priori error of ANY
binary32 evaluation order of the same layers against binary64, which serves the order-free checks and the torch layers of the
classifiers' tail.
"""
import numpy as np

U = 2.0 ** -24     # unit roundoff of binary32


def gamma(n):
    """n u / (1 - n u): the classic bound on the relative error of n binary32 roundings in a row."""
    return n * U / (1.0 - n * U)


def fma32(a, b, c):
    """round_binary32(a * b + c) for binary32 arrays, exactly.  The product of two binary32 numbers is exact in binary64 (48 <= 53
    bits).  The sum p + c is taken with a TwoSum; if its error term is not zero the binary64 sum is inexact and its last bit is forced
    odd (round-to-odd: of the two binary64 neighbours of the true value the odd one), after which the rounding to binary32 is the
    correct single rounding because 53 >= 24 + 2.
    Rounding twice (to binary64, then to binary32) differs from that only where the binary64 sum sits exactly on a binary32 midpoint,
    so the TwoSum runs on those elements alone: a binary64 whose low 29 fraction bits are 1 0...0 (normal binary32 range) or whose
    magnitude is below 2^-126 (where binary32 keeps fewer bits and the midpoints sit elsewhere)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    shape = np.broadcast(a, b, c).shape
    a, b, c = np.atleast_1d(a), np.atleast_1d(b), np.atleast_1d(c)
    p = a * b
    s = p + c
    out = s.astype(np.float32)
    suspect = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | (np.abs(s) < 2.0 ** -126)
    if suspect.any():
        p, c = np.broadcast_to(p, s.shape)[suspect], np.broadcast_to(c, s.shape)[suspect]
        out[suspect] = _fma32_round_to_odd(p, c)
    return out.reshape(shape)


def _fma32_round_to_odd(p, c64):
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    inexact = err != 0.0
    if inexact.any():
        even = (s.view(np.int64) & 1) == 0
        fix = inexact & even
        if fix.any():
            # s is the nearest binary64 and has an even last bit: the odd neighbour lies on the side of the true value
            s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def gather_rows(xyz, new_xyz, feats_t, idx, use_xyz, dtype=np.float32):
    """The rows the kernel builds, (B, m, nsample, K_0): relative coordinates first (use_xyz), then the point's features."""
    B = xyz.shape[0]
    bi = np.arange(B)[:, None, None]
    cols = []
    if use_xyz:
        cols.append(xyz.astype(dtype)[bi, idx] - new_xyz.astype(dtype)[:, :, None, :])
    if feats_t is not None:
        cols.append(feats_t.astype(dtype)[bi, idx])
    return np.concatenate(cols, axis=-1)


def mlp_rows(x, layers):
    """The contract's layers on rows x (..., K_0) float32: acc = bias; acc = fmaf(x[k], W[j, k], acc) for k ascending; y = acc > 0 ? acc : +0."""
    for W, bias in layers:
        W = np.asarray(W, dtype=np.float32)
        acc = np.broadcast_to(np.asarray(bias, dtype=np.float32), x.shape[:-1] + (W.shape[0],)).copy()
        for k in range(W.shape[1]):
            acc = fma32(x[..., k, None], W[:, k], acc)
        x = np.where(acc > 0, acc, np.float32(0.0)).astype(np.float32)
    return x


def sa_mlp_max(xyz, new_xyz, feats_t, idx, layers, use_xyz=True, centres=None):
    """The kernel's contract -> (B, width_last, m) float32.  centres: a list of centre indices to evaluate instead of all m (the
    result then has that many columns): every centre is independent of the others."""
    if centres is not None:
        new_xyz, idx = new_xyz[:, centres], idx[:, centres]
    y = mlp_rows(gather_rows(xyz, new_xyz, feats_t, idx, use_xyz), layers)     # (B, m, nsample, C)
    return np.ascontiguousarray(y.max(axis=2).transpose(0, 2, 1))


def dense_bound(x, e, layers, extra=1, relu_last=True):
    """Layers ``relu(W x + b)`` on binary64 rows x (..., K) beside the bound e (..., K) on what a binary32 evaluation holds in place
    of x -> (y, e_out).  Per layer, for any summation order, e_out = |W| e_in + gamma_(K + extra) (|W| |x^| + bmag) with
    |x^| <= |x| + e_in the computed input; extra = 1 is the addition of the bias.  ReLU is 1-Lipschitz, so it passes the bound on.
    A layer is (W, b) or (W, b, bmag) with bmag >= |b| the magnitude that the roundings of the bias path act on (a batch norm that
    is evaluated on its own rounds |a mean| + |beta|, not their difference)."""
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    for i, layer in enumerate(layers):
        W = np.asarray(layer[0], dtype=np.float64)
        b = np.asarray(layer[1], dtype=np.float64)
        bmag = np.abs(b) if len(layer) < 3 else np.asarray(layer[2], dtype=np.float64)
        aW = np.abs(W).T
        e = e @ aW + gamma(W.shape[1] + extra) * ((np.abs(x) + e) @ aW + bmag)
        x = x @ W.T + b
        if relu_last or i + 1 < len(layers):
            x = np.maximum(x, 0.0)
    return x, e


def sa_bound(xyz, new_xyz, feats_t, idx, layers, use_xyz=True, feats_err=None, extra=1):
    """Binary64 evaluation of the set abstraction on the given (binary32) weights and the a-priori bound on the error of any
    binary32 evaluation of it -> (ref, bound), both (B, width_last, m) float64.  The relative coordinates carry the one rounding of
    their subtraction, u |d|; the features carry feats_err (B, N, C) or nothing; the maximum over the ball is 1-Lipschitz in the
    sup norm, so the bound of a maximum is the largest bound in its ball."""
    x = gather_rows(xyz, new_xyz, feats_t, idx, use_xyz, dtype=np.float64)
    e = np.zeros_like(x)
    if use_xyz:
        e[..., :3] = U * np.abs(x[..., :3])
    if feats_err is not None:
        e[..., (3 if use_xyz else 0):] = np.asarray(feats_err, dtype=np.float64)[np.arange(xyz.shape[0])[:, None, None], idx]
    y, e = dense_bound(x, e, layers, extra=extra)
    return np.ascontiguousarray(y.max(axis=2).transpose(0, 2, 1)), np.ascontiguousarray(e.max(axis=2).transpose(0, 2, 1))
