"""The reference's ``pointnet2_ops.pointnet2_modules`` (Final_Project/pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py) over the
device ops of ``pointnet2_utils``: set abstraction (single- and multi-scale grouping) and feature propagation.  Sub-module names and
their order match the reference's, so its checkpoints load (``groupers``, ``mlps.<scale>.<layer>``, ``mlp.<layer>``).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from .. import _lib
from . import pointnet2_utils


def build_shared_mlp(mlp_spec: List[int], bn: bool = True):
    """1x1 convolutions mlp_spec[0] -> mlp_spec[1] -> ..., each followed by batch norm (if bn; the convolution then has no bias) and ReLU."""
    layers = []
    for c_in, c_out in zip(mlp_spec[:-1], mlp_spec[1:]):
        layers.append(nn.Conv2d(c_in, c_out, kernel_size=1, bias=not bn))
        if bn:
            layers.append(nn.BatchNorm2d(c_out))
        layers.append(nn.ReLU(True))
    return nn.Sequential(*layers)


def fold_shared_mlp(mlp):
    """The layers of a ``build_shared_mlp`` sequence in eval mode as ``[(W', b'), ...]``, float32 on the module's device, with each
    batch norm folded into the convolution in front of it so that a layer is ``relu(W' x + b')``.  Computed in binary64 and rounded
    once: ``s = gamma / sqrt(running_var + eps)``, ``W' = W * s`` per output row, ``b' = beta - running_mean * s (+ conv_bias * s)``;
    a convolution without batch norm keeps its own weight and bias.  A module in training mode raises (its batch norm would use
    the batch's statistics)."""
    if mlp.training:
        raise ValueError("fold_shared_mlp needs a module in eval mode: in training mode batch norm uses the batch's statistics")
    folded, relu_last = _fold_layers(list(mlp), nn.Conv2d, nn.BatchNorm2d)
    if not relu_last:
        raise ValueError("every layer of the shared MLP must end in a ReLU")
    return folded


def fold_pointwise_head(head):
    """``fold_shared_mlp`` for a per-point head of ``Conv1d`` (kernel size 1), ``BatchNorm1d``, ``ReLU`` and ``Dropout`` layers in eval
    mode (where dropout is the identity and is skipped) -> ``(layers, relu_last)``: the last layer may come without a ReLU, every
    other one must have it."""
    if head.training:
        raise ValueError("fold_pointwise_head needs a module in eval mode: in training mode batch norm uses the batch's statistics")
    return _fold_layers([layer for layer in head if not isinstance(layer, nn.Dropout)], nn.Conv1d, nn.BatchNorm1d)


def _fold_layers(layers, conv_type, bn_type):
    folded = []
    i = 0
    relu = True
    with torch.no_grad():
        while i < len(layers):
            conv = layers[i]
            if not isinstance(conv, conv_type) or any(k != 1 for k in conv.kernel_size) or conv.groups != 1:
                raise ValueError(f"layer {i} of the shared MLP is not a 1x1 convolution: {conv!r}")
            if not relu:
                raise ValueError("every layer of the shared MLP must end in a ReLU")
            i += 1
            W = conv.weight.detach().to(torch.float64).reshape(conv.out_channels, conv.in_channels)
            bias = conv.bias.detach().to(torch.float64) if conv.bias is not None else torch.zeros(conv.out_channels, dtype=torch.float64, device=W.device)
            if i < len(layers) and isinstance(layers[i], bn_type):
                bn = layers[i]
                i += 1
                if bn.running_var is None or bn.running_mean is None:
                    raise ValueError("a batch norm without running statistics cannot be folded")
                s = 1.0 / torch.sqrt(bn.running_var.detach().to(torch.float64) + bn.eps)
                if bn.weight is not None:
                    s = bn.weight.detach().to(torch.float64) * s
                beta = bn.bias.detach().to(torch.float64) if bn.bias is not None else torch.zeros_like(s)
                W = W * s[:, None]
                bias = beta - bn.running_mean.detach().to(torch.float64) * s + (bias * s if conv.bias is not None else 0.0)
            relu = i < len(layers) and isinstance(layers[i], nn.ReLU)
            if relu:
                i += 1
            folded.append((W.to(torch.float32).contiguous(), bias.to(torch.float32).contiguous()))
    return folded, relu


class _FoldedCache:
    """``fold(module)`` kept per key until one of the module's parameters or buffers is written to, replaced or moved."""

    def __init__(self, fold):
        self._fold = fold
        self._kept = {}

    def get(self, key, module):
        try:
            stamp = tuple((t._version, t.data_ptr()) for t in list(module.parameters()) + list(module.buffers()))
        except RuntimeError:     # tensors made in inference mode keep no version: fold every time
            stamp = None
        kept = self._kept.get(key)
        if kept is None or stamp is None or kept[0] != stamp:
            kept = (stamp, self._fold(module))
            self._kept[key] = kept
        return kept[1]


class _PointnetSAModuleBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None
        self._folded = _FoldedCache(fold_shared_mlp)

    def _folded_mlp(self, scale):
        """fold_shared_mlp of one scale, kept until one of its parameters or buffers is written to, replaced or moved."""
        return self._folded.get(scale, self.mlps[scale])

    def fused_forward(self, xyz: torch.Tensor, features: Optional[torch.Tensor]) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """``forward`` for inference (eval mode, grad disabled; anything else raises): the same sampling and ball query, then per scale
        ONE kernel (pointnet2_utils.grouped_mlp_max) that gathers, runs the shared MLP with its batch norm folded in and takes the
        maximum over the ball, writing its channel range of the (B, sum of widths, npoint) result; the grouped tensor is never
        stored.  A scale that groups everything, or whose shape the kernel declines, goes through ``forward``'s torch path.  Every
        output is one binary32 fmaf chain per layer (include/pcr.h), so the values differ from ``forward``'s by rounding only."""
        if self.training or torch.is_grad_enabled():
            raise RuntimeError("fused_forward is for inference: call it on a module in eval() mode under torch.no_grad()")
        new_xyz = None
        if self.npoint is not None:
            picks = pointnet2_utils.furthest_point_sample(xyz, self.npoint)
            new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), picks).transpose(1, 2).contiguous()
        widths = [[layer for layer in mlp if isinstance(layer, nn.Conv2d)][-1].out_channels for mlp in self.mlps]
        B = xyz.shape[0]
        out = torch.empty((B, sum(widths), self.npoint if self.npoint is not None else 1), dtype=torch.float32, device=xyz.device)
        features_t = None     # point-major copy, made once and shared by the scales
        first = 0
        for scale, (grouper, mlp, width) in enumerate(zip(self.groupers, self.mlps, widths)):
            dst = out[:, first:first + width]
            first += width
            if isinstance(grouper, pointnet2_utils.QueryAndGroup):
                if features is not None and features_t is None:
                    features_t = features.transpose(1, 2).contiguous()
                idx = pointnet2_utils.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz)
                folded = self._folded_mlp(scale)
                try:
                    pointnet2_utils.grouped_mlp_max(xyz, new_xyz, features_t, idx, [w for w, _ in folded], [b for _, b in folded],
                                                    use_xyz=grouper.use_xyz, out=dst)
                    continue
                except _lib.PcrError as err:
                    if err.status != _lib.PCR_E_UNSUPPORTED:
                        raise
            dst.copy_(mlp(grouper(xyz, new_xyz, features)).max(dim=3).values)
        return new_xyz, out

    def forward(self, xyz: torch.Tensor, features: Optional[torch.Tensor]) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """xyz (B, N, 3), features (B, C, N) or None -> new_xyz (B, npoint, 3) (None when the module groups everything) and
        new_features (B, sum of the scales' last widths, npoint)."""
        new_xyz = None
        if self.npoint is not None:
            picks = pointnet2_utils.furthest_point_sample(xyz, self.npoint)
            new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), picks).transpose(1, 2).contiguous()
        pooled = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            grouped = mlp(grouper(xyz, new_xyz, features))    # (B, width, npoint, nsample)
            pooled.append(grouped.max(dim=3).values)          # (B, width, npoint)
        return new_xyz, torch.cat(pooled, dim=1)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Set abstraction with multi-scale grouping: npoint centres by furthest point sampling, per scale a ball query (radii[i],
    nsamples[i]), the shared MLP mlps[i] and a maximum over the ball.  npoint None: one group of all points per scale.  With use_xyz
    the three relative coordinates are prepended to the features, so every mlps[i][0] counts the feature channels only (as in the
    reference, 3 is added to it IN the caller's list)."""

    def __init__(self, npoint, radii, nsamples, mlps, bn=True, use_xyz=True):
        super().__init__()
        if not len(radii) == len(nsamples) == len(mlps):
            raise ValueError("radii, nsamples and mlps must have one entry per scale")
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            if use_xyz:
                spec[0] += 3
            self.mlps.append(build_shared_mlp(spec, bn))


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction with one scale."""

    def __init__(self, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz)


class PointnetFPModule(nn.Module):
    """Feature propagation: the known points' features interpolated to the unknown points (inverse distances to the three nearest,
    normalised), joined with the unknown points' own features, through a shared MLP."""

    def __init__(self, mlp, bn=True):
        super().__init__()
        self.mlp = build_shared_mlp(mlp, bn=bn)
        self._folded = _FoldedCache(fold_shared_mlp)

    def fused_forward(self, unknown, known, unknow_feats, known_feats):
        """``forward`` for inference (eval mode, grad disabled; anything else raises): the same three_nn and the same weights, then ONE
        kernel (pointnet2_utils.propagated_mlp) that interpolates, joins the unknown points' own features and runs the shared MLP with
        its batch norm folded in; neither the interpolated tensor nor the concatenation nor a layer's intermediate is stored.
        ``known is None`` (the expand branch), a shape the kernel declines and a shape measured slower than ``forward``
        (``_kernel_takes``) go through ``forward``.  Every output is one binary32 fmaf chain per layer (include/pcr.h), so the values
        differ from ``forward``'s by rounding only."""
        if self.training or torch.is_grad_enabled():
            raise RuntimeError("fused_forward is for inference: call it on a module in eval() mode under torch.no_grad()")
        if known is None or not self._kernel_takes():
            return self.forward(unknown, known, unknow_feats, known_feats)
        dist, idx = pointnet2_utils.three_nn(unknown, known)
        recip = 1.0 / (dist + 1e-8)
        weight = recip / torch.sum(recip, dim=2, keepdim=True)
        folded = self._folded.get(0, self.mlp)
        try:
            return pointnet2_utils.propagated_mlp(known_feats.transpose(1, 2).contiguous(), idx, weight,
                                                  None if unknow_feats is None else unknow_feats.transpose(1, 2).contiguous(),
                                                  [w for w, _ in folded], [b for _, b in folded])
        except _lib.PcrError as err:
            if err.status != _lib.PCR_E_UNSUPPORTED:
                raise
        return self._joined_mlp(pointnet2_utils.three_interpolate(known_feats, idx, weight), unknow_feats)     # forward's torch ops

    # Above 128 channels the kernel keeps one workgroup of four waves per compute unit, and a workgroup walks its K_0 columns 32 at a
    # time in one serial chain: measured at B = 8 (profiles/fp_fused_bench.json "routed"), [608, 256, 256] on 1024
    # points took 0.256 ms against forward's 0.190 and [768, 256, 256] on 64 points 0.213 against 0.184, while [384, 256, 256] and
    # [320, 256, 128] were faster than forward.
    FUSED_MAX_K0_WIDE = 384

    def _kernel_takes(self):
        """Whether fused_forward hands this module's shape to the kernel: within the kernel's limits (checked here, so that a module
        it declines costs nothing beyond forward), and not one of the shapes measured slower than forward."""
        convs = [layer for layer in self.mlp if isinstance(layer, nn.Conv2d)]
        k0, widest = convs[0].in_channels, max(c.out_channels for c in convs)
        if len(convs) > pointnet2_utils.FP_MLP_MAX_LAYERS or widest > pointnet2_utils.FP_MLP_MAX_WIDTH or k0 > pointnet2_utils.FP_MLP_MAX_K0:
            return False
        return widest <= 128 or k0 <= self.FUSED_MAX_K0_WIDE

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B, n, 3), known (B, m, 3) or None, unknow_feats (B, C1, n) or None, known_feats (B, C2, m) -> (B, mlp[-1], n)."""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            recip = 1.0 / (dist + 1e-8)
            weight = recip / torch.sum(recip, dim=2, keepdim=True)
            interpolated = pointnet2_utils.three_interpolate(known_feats, idx, weight)
        else:
            interpolated = known_feats.expand(*known_feats.shape[:2], unknown.size(1))
        return self._joined_mlp(interpolated, unknow_feats)

    def _joined_mlp(self, interpolated, unknow_feats):
        new_features = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        return self.mlp(new_features.unsqueeze(-1)).squeeze(-1)
