"""The reference's ``pointnet2_ops.pointnet2_modules`` (Final_Project/pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py) over the
device ops of ``pointnet2_utils``: set abstraction (single- and multi-scale grouping) and feature propagation.  Sub-module names and
their order match the reference's, so its checkpoints load (``groupers``, ``mlps.<scale>.<layer>``, ``mlp.<layer>``).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn

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


class _PointnetSAModuleBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None

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

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B, n, 3), known (B, m, 3) or None, unknow_feats (B, C1, n) or None, known_feats (B, C2, m) -> (B, mlp[-1], n)."""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            recip = 1.0 / (dist + 1e-8)
            weight = recip / torch.sum(recip, dim=2, keepdim=True)
            interpolated = pointnet2_utils.three_interpolate(known_feats, idx, weight)
        else:
            interpolated = known_feats.expand(*known_feats.shape[:2], unknown.size(1))
        new_features = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        return self.mlp(new_features.unsqueeze(-1)).squeeze(-1)
