"""The reference's ``pointnet2_ops.pointnet2_utils`` (Final_Project/pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py) on the MI355X:
the same names and signatures, torch tensors on the device in and out, the six forward ops as HIP kernels behind the C ABI
(include/pcr.h, "PointNet++ set-abstraction ops") launched on torch's current stream with the tensors' own addresses.

Every argument is checked before anything is launched and a bad one raises ValueError: dtype (float32 data, int32 indices), rank,
contiguity, matching batch sizes, and that the tensors live on a GPU.  There is no host path.

The three gradients (gather, group, interpolate) have two paths.  By default they are composed from torch's ``scatter_add_`` on the
device; their summation order is then torch's (floating-point atomics), not a fixed one.  Under ``fixed_order_gradients()`` (or after
``set_fixed_order_gradients(True)``) they are HIP kernels with a written order (include/pcr.h, "PointNet++ gradients"): per output
the terms are added one by one in ascending slot order, so two runs give the same bits, NumPy's ``np.add.at`` on float32 gives the
same bits, and nothing in them depends on ``torch.use_deterministic_algorithms``.  The switch is read in ``forward`` and remembered
for that call's ``backward``.  ``inverse_index`` and ``scatter_rows_ordered`` are the two steps for direct use; the inverse index is
kept on the ``idx`` tensor object (guarded by its ``_version`` and the stream), so tensors grouped with the same ``idx`` share one build.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from .. import _lib

_INT_MAX = 2**31 - 1


def _check(*specs, device=True):
    """specs: (tensor, name, dtype, shape) with shape entries None (free), an int (required) or a letter (equal among the specs)."""
    named = {}
    for t, name, dtype, shape in specs:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"{name} must have dtype {dtype}, not {t.dtype}")
        if t.dim() != len(shape):
            raise ValueError(f"{name} must have rank {len(shape)}, not {t.dim()}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    for t, name, dtype, shape in specs:
        for axis, want in enumerate(shape):
            have = t.shape[axis]
            if have > _INT_MAX:
                raise ValueError(f"{name}: axis {axis} has {have} entries, more than an int32 index reaches")
            if isinstance(want, int) and have != want:
                raise ValueError(f"{name} must have {want} entries along axis {axis}, not {have}")
            if isinstance(want, str):
                other = named.setdefault(want, (have, name, axis))
                if other[0] != have:
                    what = "batch sizes" if want == "B" else "sizes"
                    raise ValueError(f"mismatched {what}: {other[1]} has {other[0]} along axis {other[2]}, {name} has {have} along axis {axis}")
    if device:
        first = specs[0][0]
        for t, name, dtype, shape in specs:
            if t.device.type != "cuda":
                raise ValueError(f"{name} must be on the GPU (it is on {t.device}): these ops have no host path")
            if t.device != first.device:
                raise ValueError(f"{name} is on {t.device}, {specs[0][1]} on {first.device}")


def _count(value, name, least=0):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least or value > _INT_MAX:
        raise ValueError(f"{name} must be an integer in [{least}, 2^31), not {value!r}")
    return int(value)


def _launch(anchor, fn_name, *args):
    """One C-ABI call on the current stream of `anchor`'s device."""
    with torch.cuda.device(anchor.device):
        fn = getattr(_lib.lib(), fn_name)
        _lib.check(fn(torch.cuda.current_stream().cuda_stream, *args))


f32, i32 = torch.float32, torch.int32


class FurthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz (B, N, 3) float32 -> (B, npoint) int32: iterative furthest point sampling from index 0; of equally far points the
        lowest index wins, points with |p|^2 <= 1e-3 are padding and never chosen (include/pcr.h)."""
        _check((xyz, "xyz", f32, ("B", None, 3)))
        npoint = _count(npoint, "npoint")
        B, N, _ = xyz.shape
        if N == 0 and B and npoint:
            raise ValueError("xyz has no points to sample from")
        out = torch.empty((B, npoint), dtype=i32, device=xyz.device)
        temp = torch.empty((B, N), dtype=f32, device=xyz.device)
        _launch(xyz, "pcr_pn2_furthest_point_sampling", B, N, npoint, xyz.data_ptr(), temp.data_ptr(), out.data_ptr())
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return ()


furthest_point_sample = FurthestPointSampling.apply


def _scatter_rows(grad_cols, idx_cols, n):
    """sum of grad_cols (B, C, K) into (B, C, n) at idx_cols (B, K): the transpose of a gather along the last axis."""
    B, C, K = grad_cols.shape
    out = torch.zeros((B, C, n), dtype=grad_cols.dtype, device=grad_cols.device)
    return out.scatter_add_(2, idx_cols.to(torch.int64).view(B, 1, K).expand(B, C, K), grad_cols)


# ---------------------------------------------------------------- the gradients in a fixed order
_fixed_order = False


def set_fixed_order_gradients(enabled):
    """Switch the gradients of gather / group / three_interpolate to the fixed-order kernels (True) or back to torch's
    ``scatter_add_`` (False, the default) for every later ``forward``; returns the previous setting."""
    global _fixed_order
    previous, _fixed_order = _fixed_order, bool(enabled)
    return previous


def fixed_order_gradients_enabled():
    return _fixed_order


@contextlib.contextmanager
def fixed_order_gradients(enabled=True):
    """Context manager around ``set_fixed_order_gradients``: a ``forward`` inside it decides its own ``backward``, wherever that runs."""
    previous = set_fixed_order_gradients(enabled)
    try:
        yield
    finally:
        set_fixed_order_gradients(previous)


def inverse_index(idx, n):
    """idx (B, ...) int32 with entries in [0, n), its trailing axes flattened to K slots per cloud -> (start (B, n + 1), slots (B, K))
    int32: point i of cloud b is named by slots[b, start[b, i]:start[b, i + 1]], ascending (include/pcr.h, pcr_pn2_inverse_index).
    Built on the current stream and kept on the ``idx`` object; reused while ``idx._version``, its address, n and the current
    stream are unchanged (a call on another stream builds its own, so no stream reads an index that another is still writing).
    ``_version`` sees torch's in-place operations only: after writing into ``idx`` through its raw address, drop the attribute
    ``idx._pcr_inverse_index``."""
    rank = idx.dim() if isinstance(idx, torch.Tensor) and idx.dim() == 3 else 2
    _check((idx, "idx", i32, ("B",) + (None,) * (rank - 1)))
    n = _count(n, "n")
    B = idx.shape[0]
    K = _count(int(np.prod(idx.shape[1:])), "the number of slots per cloud")
    if n == 0 and B and K:
        raise ValueError("idx names points of a cloud without points")
    try:
        version = idx._version
    except RuntimeError:     # tensors made in inference mode keep no version: build every time
        version = None
    key = (version, n, idx.data_ptr(), torch.cuda.current_stream(idx.device).cuda_stream)
    kept = getattr(idx, "_pcr_inverse_index", None)
    if kept is not None and version is not None and kept[0] == key:
        return kept[1], kept[2]
    start = torch.empty((B, n + 1), dtype=i32, device=idx.device)
    slots = torch.empty((B, K), dtype=i32, device=idx.device)
    with torch.cuda.device(idx.device):
        need = _lib.lib().pcr_pn2_inverse_index_bytes(B, n, K)
        if need < 0:
            _lib.check(int(need))
        work = torch.empty((int(need),), dtype=torch.uint8, device=idx.device)
    _launch(idx, "pcr_pn2_inverse_index", B, n, K, idx.data_ptr(), work.data_ptr(), int(need), start.data_ptr(), slots.data_ptr())
    if version is not None:
        idx._pcr_inverse_index = (key, start, slots)
    return start, slots


def scatter_rows_ordered(grad, idx, n, weight=None):
    """The transpose of a gather along the last axis in the written order of include/pcr.h ("PointNet++ gradients"):
    out[b, c, i] = the terms of the slots with idx[b, slot] == i, added in ascending slot order in float32 -> (B, C, n).

    grad (B, C, K) with idx (B, K): gather's gradient.  grad (B, C, npoint, nsample) with idx (B, npoint, nsample): group's.
    grad (B, C, m) with idx and weight (B, m, 3): three_interpolate's, term = grad[b, c, j] * weight[b, j, k] rounded once."""
    if weight is not None:
        _check((grad, "grad", f32, ("B", None, "j")), (idx, "idx", i32, ("B", "j", 3)), (weight, "weight", f32, ("B", "j", 3)))
    elif isinstance(idx, torch.Tensor) and idx.dim() == 3:
        _check((grad, "grad", f32, ("B", None, "j", "s")), (idx, "idx", i32, ("B", "j", "s")))
    else:
        _check((grad, "grad", f32, ("B", None, "j")), (idx, "idx", i32, ("B", "j")))
    n = _count(n, "n")
    B, C = grad.shape[:2]
    start, slots = inverse_index(idx, n)
    out = torch.empty((B, C, n), dtype=f32, device=grad.device)
    if weight is not None:
        _launch(grad, "pcr_pn2_three_interpolate_grad", B, C, grad.shape[2], n, grad.data_ptr(), start.data_ptr(), slots.data_ptr(),
                weight.data_ptr(), out.data_ptr())
    elif idx.dim() == 3:
        _launch(grad, "pcr_pn2_group_points_grad", B, C, n, idx.shape[1], idx.shape[2], grad.data_ptr(), start.data_ptr(), slots.data_ptr(), out.data_ptr())
    else:
        _launch(grad, "pcr_pn2_gather_points_grad", B, C, n, idx.shape[1], grad.data_ptr(), start.data_ptr(), slots.data_ptr(), out.data_ptr())
    return out


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B, C, N) float32, idx (B, npoint) int32 -> (B, C, npoint): out[b, c, j] = features[b, c, idx[b, j]]."""
        _check((features, "features", f32, ("B", None, None)), (idx, "idx", i32, ("B", None)))
        B, C, N = features.shape
        npoint = idx.shape[1]
        if N == 0 and B and C and npoint:
            raise ValueError("features has no points to gather from")
        out = torch.empty((B, C, npoint), dtype=f32, device=features.device)
        _launch(features, "pcr_pn2_gather_points", B, C, N, npoint, features.data_ptr(), idx.data_ptr(), out.data_ptr())
        ctx.save_for_backward(idx)
        ctx.n = N
        ctx.fixed_order = _fixed_order
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        if ctx.fixed_order:
            return scatter_rows_ordered(grad_out.contiguous(), idx, ctx.n), None
        return _scatter_rows(grad_out.contiguous(), idx, ctx.n), None


gather_operation = GatherOperation.apply


def _three_nn_dist2(unknown, known):
    """(squared distances, indices) of the three nearest known points of every unknown point, as the kernel leaves them."""
    _check((unknown, "unknown", f32, ("B", None, 3)), (known, "known", f32, ("B", None, 3)))
    B, n, _ = unknown.shape
    m = known.shape[1]
    if m == 0 and B and n:
        raise ValueError("known has no points")
    dist2 = torch.empty((B, n, 3), dtype=f32, device=unknown.device)
    idx = torch.empty((B, n, 3), dtype=i32, device=unknown.device)
    _launch(unknown, "pcr_pn2_three_nn", B, n, m, unknown.data_ptr(), known.data_ptr(), dist2.data_ptr(), idx.data_ptr())
    return dist2, idx


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown (B, n, 3), known (B, m, 3) -> dist (B, n, 3) float32 (Euclidean, ascending) and idx (B, n, 3) int32; fewer than
        three known points: the empty slots are +inf and index 0."""
        dist2, idx = _three_nn_dist2(unknown, known)
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, grad_dist, grad_idx):
        return ()


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features (B, c, m), idx (B, n, 3) int32, weight (B, n, 3) -> (B, c, n): the weighted sum of three columns of features."""
        _check((features, "features", f32, ("B", None, None)), (idx, "idx", i32, ("B", "n", 3)), (weight, "weight", f32, ("B", "n", 3)))
        B, c, m = features.shape
        n = idx.shape[1]
        if m == 0 and B and c and n:
            raise ValueError("features has no points to interpolate from")
        out = torch.empty((B, c, n), dtype=f32, device=features.device)
        _launch(features, "pcr_pn2_three_interpolate", B, c, m, n, features.data_ptr(), idx.data_ptr(), weight.data_ptr(), out.data_ptr())
        ctx.save_for_backward(idx, weight)
        ctx.m = m
        ctx.fixed_order = _fixed_order
        return out

    @staticmethod
    def backward(ctx, grad_out):
        """Gradient of the features only (as in the reference, the weights get none)."""
        idx, weight = ctx.saved_tensors
        if ctx.fixed_order:
            return scatter_rows_ordered(grad_out.contiguous(), idx, ctx.m, weight=weight), None, None
        B, c, n = grad_out.shape
        terms = (grad_out.unsqueeze(-1) * weight.unsqueeze(1)).reshape(B, c, 3 * n)
        return _scatter_rows(terms, idx.reshape(B, 3 * n), ctx.m), None, None


three_interpolate = ThreeInterpolate.apply


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B, C, N), idx (B, npoint, nsample) int32 -> (B, C, npoint, nsample): out[b, c, j, s] = features[b, c, idx[b, j, s]]."""
        _check((features, "features", f32, ("B", None, None)), (idx, "idx", i32, ("B", None, None)))
        B, C, N = features.shape
        _, npoint, nsample = idx.shape
        if N == 0 and B and C and npoint and nsample:
            raise ValueError("features has no points to group")
        out = torch.empty((B, C, npoint, nsample), dtype=f32, device=features.device)
        _launch(features, "pcr_pn2_group_points", B, C, N, npoint, nsample, features.data_ptr(), idx.data_ptr(), out.data_ptr())
        ctx.save_for_backward(idx)
        ctx.n = N
        ctx.fixed_order = _fixed_order
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        if ctx.fixed_order:
            return scatter_rows_ordered(grad_out.contiguous(), idx, ctx.n), None
        B, C = grad_out.shape[:2]
        return _scatter_rows(grad_out.reshape(B, C, -1), idx.reshape(B, -1), ctx.n), None


grouping_operation = GroupingOperation.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        """xyz (B, N, 3), new_xyz (B, npoint, 3) -> (B, npoint, nsample) int32: per centre the first nsample points, by index, strictly
        inside the ball; short rows are filled with their first hit, rows without a hit with 0."""
        _check((xyz, "xyz", f32, ("B", None, 3)), (new_xyz, "new_xyz", f32, ("B", None, 3)))
        nsample = _count(nsample, "nsample")
        radius = float(radius)
        if not np.isfinite(np.float32(radius)):
            raise ValueError(f"radius must be finite as a float32, not {radius!r}")
        B, N, _ = xyz.shape
        npoint = new_xyz.shape[1]
        if N == 0 and B and npoint and nsample:
            raise ValueError("xyz has no points to query")
        out = torch.empty((B, npoint, nsample), dtype=i32, device=xyz.device)
        _launch(xyz, "pcr_pn2_ball_query", B, N, npoint, radius, nsample, new_xyz.data_ptr(), xyz.data_ptr(), out.data_ptr())
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return ()


ball_query = BallQuery.apply


def _layer_specs(weights, biases):
    """The layer lists of grouped_mlp_max / propagated_mlp as lists, checked for their lengths, and one _check spec per tensor."""
    weights, biases = list(weights), list(biases)
    if len(weights) != len(biases) or not weights:
        raise ValueError("weights and biases must be lists of the same length, one entry per layer (at least one)")
    specs = []
    for l, (w, bias) in enumerate(zip(weights, biases)):
        specs += [(w, f"weights[{l}]", f32, (f"w{l}", f"k{l}")), (bias, f"biases[{l}]", f32, (f"w{l}",))]
    return weights, biases, specs


def _layer_chain(weights, biases, k):
    """K_0 = k and K_l = width_(l-1) along the layers (which have passed _check) -> the last width and (n_layers, widths, weights,
    biases) as the C entry points take them."""
    for l, w in enumerate(weights):
        if w.shape[1] != k:
            raise ValueError(f"weights[{l}] must have {k} entries along axis 1, not {w.shape[1]}")
        if w.shape[0] < 1:
            raise ValueError(f"weights[{l}] must have at least one row")
        k = w.shape[0]
    n_layers, C = len(weights), _lib.C
    return k, (n_layers, (C.c_int * n_layers)(*[w.shape[0] for w in weights]), (C.c_void_p * n_layers)(*[w.data_ptr() for w in weights]),
               (C.c_void_p * n_layers)(*[t.data_ptr() for t in biases]))


def _not_differentiable(name, specs, out):
    if torch.is_grad_enabled() and any(t.requires_grad for t, *_ in specs + ([(out,)] if out is not None else [])):
        raise ValueError(f"{name} is not differentiable: call it under torch.no_grad() or on tensors that do not require grad")


def grouped_mlp_max(xyz, new_xyz, features_t, idx, weights, biases, use_xyz=True, out=None):
    """Set abstraction for inference in one kernel (include/pcr.h, pcr_pn2_sa_mlp_max): per centre the rows of its ball -- relative
    coordinates (use_xyz), then the point's features -- through the layers ``relu(W x + b)`` and the maximum over the ball; the grouped
    tensor is never stored.

    xyz (B, N, 3), new_xyz (B, npoint, 3), features_t (B, N, C) POINT-major or None, idx (B, npoint, nsample) int32 (ball_query's),
    weights[l] (width_l, K_l) and biases[l] (width_l,) float32 with K_0 = 3 * use_xyz + C and K_l = width_(l-1) (fold_shared_mlp of
    pointnet2_modules gives them) -> (B, width_last, npoint).  `out`: a (B, width_last, npoint) float32 view to write into instead,
    contiguous in its last two axes (a channel range of a larger (B, C_total, npoint) tensor); it is returned.

    Not differentiable: an input that requires grad while grad is enabled raises ValueError.  A shape the kernel declines raises
    PcrError with status PCR_E_UNSUPPORTED and has launched nothing."""
    weights, biases, layer_specs = _layer_specs(weights, biases)
    specs = [(xyz, "xyz", f32, ("B", "N", 3)), (new_xyz, "new_xyz", f32, ("B", "m", 3)), (idx, "idx", i32, ("B", "m", None))]
    if features_t is not None:
        specs.append((features_t, "features_t", f32, ("B", "N", None)))
    specs += layer_specs
    _check(*specs, device=False)
    c_feat = 0 if features_t is None else features_t.shape[2]
    k = (3 if use_xyz else 0) + c_feat
    if k < 1:
        raise ValueError("grouped_mlp_max without features needs use_xyz")
    k, layer_args = _layer_chain(weights, biases, k)
    B, N, _ = xyz.shape
    _, npoint, nsample = idx.shape
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != f32 or tuple(out.shape) != (B, k, npoint):
            raise ValueError(f"out must be a float32 tensor of shape {(B, k, npoint)}")
        if B and k and npoint and (out.stride(2) != 1 or out.stride(1) != npoint or (B > 1 and out.stride(0) < k * npoint)):
            raise ValueError("out must be contiguous in its last two axes, with a batch stride that keeps the batches apart")
    _not_differentiable("grouped_mlp_max", specs, out)
    if B and npoint and nsample < 1:
        raise ValueError("idx has no samples per centre")
    if B and npoint and N == 0:
        raise ValueError("xyz has no points to group")
    _check(*specs)
    if out is not None and out.device != xyz.device:
        raise ValueError(f"out is on {out.device}, xyz on {xyz.device}")
    if out is None:
        out = torch.empty((B, k, npoint), dtype=f32, device=xyz.device)
    _launch(xyz, "pcr_pn2_sa_mlp_max", B, N, npoint, nsample, c_feat, 1 if use_xyz else 0, xyz.data_ptr(), new_xyz.data_ptr(),
            features_t.data_ptr() if features_t is not None else None, idx.data_ptr(), *layer_args, out.data_ptr(),
            out.stride(0) if B > 1 else k * npoint)
    return out


FP_MLP_MAX_LAYERS, FP_MLP_MAX_WIDTH, FP_MLP_MAX_K0 = 3, 256, 1024     # PCR_PN2_FP_MAX_LAYERS / _WIDTH / _K0 of include/pcr.h


def propagated_mlp(known_feats_t, idx, weight, skip_feats_t, weights, biases, relu_last=True, out=None):
    """Feature propagation for inference in one kernel (include/pcr.h, pcr_pn2_fp_mlp): per point the row of its interpolated features
    -- ((p0*w0) + (p1*w1)) + (p2*w2) over its three known points, three_interpolate's expression -- followed by its own (skip)
    features, through the layers ``relu(W x + b)``; the last layer without the ReLU when relu_last is false.  Neither the interpolated
    tensor nor the concatenation nor a layer's intermediate is stored.

    known_feats_t (B, m, C2) POINT-major, idx (B, n, 3) int32 (three_nn's) and weight (B, n, 3): all three given or all three None
    (then the call is a plain per-point shared MLP on skip_feats_t); skip_feats_t (B, n, C1) POINT-major or None; weights[l]
    (width_l, K_l) and biases[l] (width_l,) float32 with K_0 = C2 + C1 and K_l = width_(l-1) -> (B, width_last, n).  `out`: a
    contiguous (B, width_last, n) float32 tensor to write into instead; it is returned.

    Not differentiable: an input that requires grad while grad is enabled raises ValueError.  A shape the kernel declines raises
    PcrError with status PCR_E_UNSUPPORTED and has launched nothing."""
    weights, biases, layer_specs = _layer_specs(weights, biases)
    interp = (known_feats_t, idx, weight)
    if any(t is None for t in interp) and not all(t is None for t in interp):
        raise ValueError("known_feats_t, idx and weight must be given together or all be None")
    has_known = known_feats_t is not None
    if not has_known and skip_feats_t is None:
        raise ValueError("propagated_mlp needs known_feats_t (with idx and weight) or skip_feats_t")
    specs = []
    if has_known:
        specs += [(known_feats_t, "known_feats_t", f32, ("B", "m", None)), (idx, "idx", i32, ("B", "n", 3)), (weight, "weight", f32, ("B", "n", 3))]
    if skip_feats_t is not None:
        specs.append((skip_feats_t, "skip_feats_t", f32, ("B", "n", None)))
    specs += layer_specs
    _check(*specs, device=False)
    c_known = known_feats_t.shape[2] if has_known else 0
    c_skip = skip_feats_t.shape[2] if skip_feats_t is not None else 0
    k = c_known + c_skip
    if k < 1:
        raise ValueError("propagated_mlp needs at least one feature channel")
    k, layer_args = _layer_chain(weights, biases, k)
    anchor = specs[0][0]
    B = anchor.shape[0]
    n = idx.shape[1] if has_known else skip_feats_t.shape[1]
    m = known_feats_t.shape[1] if has_known else 0
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != f32 or tuple(out.shape) != (B, k, n):
            raise ValueError(f"out must be a float32 tensor of shape {(B, k, n)}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
    _not_differentiable("propagated_mlp", specs, out)
    if has_known and B and n and m == 0:
        raise ValueError("known_feats_t has no points to interpolate from")
    _check(*specs)
    if out is not None and out.device != anchor.device:
        raise ValueError(f"out is on {out.device}, {specs[0][1]} on {anchor.device}")
    if out is None:
        out = torch.empty((B, k, n), dtype=f32, device=anchor.device)
    _launch(anchor, "pcr_pn2_fp_mlp", B, n, m, c_known, c_skip, known_feats_t.data_ptr() if has_known else None,
            idx.data_ptr() if has_known else None, weight.data_ptr() if has_known else None,
            skip_feats_t.data_ptr() if skip_feats_t is not None else None, *layer_args, 1 if relu_last else 0, out.data_ptr())
    return out


class QueryAndGroup(nn.Module):
    """Ball query around every centre, then the neighbours' coordinates relative to the centre (and their features)."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """xyz (B, N, 3), new_xyz (B, npoint, 3), features (B, C, N) or None -> (B, 3 + C, npoint, nsample) (C alone without use_xyz)."""
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        grouped_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is None:
            if not self.use_xyz:
                raise ValueError("QueryAndGroup without features needs use_xyz")
            return grouped_xyz
        grouped = grouping_operation(features, idx)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped


class GroupAll(nn.Module):
    """One group holding the whole cloud."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """xyz (B, N, 3), new_xyz ignored, features (B, C, N) or None -> (B, 3 + C, 1, N) (C alone without use_xyz)."""
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped


def furthest_point_sample_np(points, npoint):
    """points (N, 3) or (B, N, 3), any real dtype (sampled as float32) -> int32 indices (npoint,) or (B, npoint), on device 0."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"points must be (N, 3) or (B, N, 3), not {pts.shape}")
    npoint = _count(npoint, "npoint")
    if not torch.cuda.is_available():
        raise RuntimeError("furthest_point_sample_np needs a GPU: there is no host path")
    dev = torch.from_numpy(pts.reshape((-1,) + pts.shape[-2:])).to("cuda")
    idx = furthest_point_sample(dev, npoint).cpu().numpy()
    return idx[0] if pts.ndim == 2 else idx
