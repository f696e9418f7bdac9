"""Restatements for the fused feature-propagation kernel (include/pcr.h, pcr_pn2_fp_mlp) in NumPy, built from what the other PointNet++
checks already contain: ``fp_rows`` is ``pointnet2_checks.three_interpolate`` and a concatenation, ``fp_mlp`` is
``sa_fused_checks.mlp_rows`` (one binary32 fmaf chain per output, k ascending, starting at the bias) with a last-layer variant for
``relu_last == 0`` (the stored value is acc + (+0)), and ``fp_bound`` is ``sa_fused_checks.dense_bound`` with the interpolated
entries carrying gamma(3) * sum |p_j w_j|: the a-priori error of ANY binary32 evaluation order against binary64.
"""
import numpy as np

from tests import pointnet2_checks as pchk
from tests import sa_fused_checks as chk


def fp_rows(known_feats_t, idx, weight, skip_feats_t):
    """The rows the kernel builds, (B, n, K_0) float32: ((p0*w0) + (p1*w1)) + (p2*w2) for each of the known points' channels, then the
    point's own features.  known_feats_t (B, m, C2) POINT-major with idx / weight (B, n, 3), or all three None; skip_feats_t
    (B, n, C1) POINT-major or None."""
    cols = []
    if known_feats_t is not None:
        points = np.ascontiguousarray(np.asarray(known_feats_t, dtype=np.float32).transpose(0, 2, 1))
        cols.append(pchk.three_interpolate(points, idx, np.asarray(weight, dtype=np.float32)).transpose(0, 2, 1))
    if skip_feats_t is not None:
        cols.append(np.asarray(skip_feats_t, dtype=np.float32))
    return np.ascontiguousarray(np.concatenate(cols, axis=-1))


def last_layer_rows(x, W, bias):
    """The contract's last layer without ReLU on rows x (..., K): the chain of ``mlp_rows``, then acc + (+0)."""
    W = np.asarray(W, dtype=np.float32)
    acc = np.broadcast_to(np.asarray(bias, dtype=np.float32), x.shape[:-1] + (W.shape[0],)).copy()
    for k in range(W.shape[1]):
        acc = chk.fma32(x[..., k, None], W[:, k], acc)
    return (acc + np.float32(0.0)).astype(np.float32)


def mlp_rows(x, layers, relu_last=True):
    if relu_last:
        return chk.mlp_rows(x, layers)
    x = chk.mlp_rows(x, layers[:-1])
    return last_layer_rows(x, *layers[-1][:2])


def fp_mlp(known_feats_t, idx, weight, skip_feats_t, layers, relu_last=True):
    """The kernel's contract -> (B, width_last, n) float32."""
    y = mlp_rows(fp_rows(known_feats_t, idx, weight, skip_feats_t), layers, relu_last=relu_last)
    return np.ascontiguousarray(y.transpose(0, 2, 1))


def fp_bound(known_feats_t, idx, weight, skip_feats_t, layers, relu_last=True, extra=1, known_err=None, skip_err=None):
    """Binary64 evaluation of the feature propagation on the given data and layers, and the a-priori bound on the error of any binary32
    evaluation of it -> (ref, bound), both (B, width_last, n) float64.  An interpolated entry is three products and two additions in
    binary32: gamma(3) * sum |p_j w_j|, on top of what its inputs carry (known_err (B, m, C2): sum |w_j| e_j, itself passing through
    those roundings); the weights are data (both paths read the same float32 tensor).  The skip features carry skip_err (B, n, C1)
    or nothing.  A layer is (W, b) or (W, b, bmag) as for ``dense_bound``."""
    xs, es = [], []
    if known_feats_t is not None:
        B = idx.shape[0]
        bi = np.arange(B)[:, None, None]
        p = np.asarray(known_feats_t, dtype=np.float64)[bi, idx]                      # (B, n, 3, C2)
        w = np.asarray(weight, dtype=np.float64)[..., None]
        xs.append((p * w).sum(axis=2))
        mag = (np.abs(p) * np.abs(w)).sum(axis=2)
        if known_err is not None:
            mag = mag + (np.asarray(known_err, dtype=np.float64)[bi, idx] * np.abs(w)).sum(axis=2)
            es.append(chk.gamma(3) * mag + (np.asarray(known_err, dtype=np.float64)[bi, idx] * np.abs(w)).sum(axis=2))
        else:
            es.append(chk.gamma(3) * mag)
    if skip_feats_t is not None:
        xs.append(np.asarray(skip_feats_t, dtype=np.float64))
        es.append(np.zeros_like(xs[-1]) if skip_err is None else np.asarray(skip_err, dtype=np.float64))
    y, e = chk.dense_bound(np.concatenate(xs, axis=-1), np.concatenate(es, axis=-1), layers, extra=extra, relu_last=relu_last)
    return np.ascontiguousarray(y.transpose(0, 2, 1)), np.ascontiguousarray(e.transpose(0, 2, 1))
