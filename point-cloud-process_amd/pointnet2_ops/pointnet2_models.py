"""The reference's two classifiers (Final_Project/pointnet2/models/pointnet2_ssg_cls.py and pointnet2_msg_cls.py) as plain
``nn.Module``s over ``pointnet2_modules``: the same layer specifications, sub-module names and order (``SA_modules.<i>...``,
``fc_layer.<i>``), so the ``model_state`` of the reference's checkpoint loads with ``load_state_dict``.  The training loop of the
reference's classes (a pytorch_lightning module) is not part of them; the reference's ``train.py`` is ``pointnet2_train``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .pointnet2_modules import PointnetSAModule, PointnetSAModuleMSG


class PointNet2ClassificationSSG(nn.Module):
    """Single-scale grouping: 512 centres (radius 0.2, 64 samples), 128 centres (0.4, 64), one group of everything, three linear layers."""

    def __init__(self, num_classes=4, input_channels=3):
        super().__init__()
        self.num_classes, self.input_channels = num_classes, input_channels
        self._build_model()

    def _build_sa(self):
        c = self.input_channels
        return [PointnetSAModule(npoint=512, radius=0.2, nsample=64, mlp=[c, 64, 64, 128], use_xyz=True),
                PointnetSAModule(npoint=128, radius=0.4, nsample=64, mlp=[128, 128, 128, 256], use_xyz=True),
                PointnetSAModule(mlp=[256, 256, 512, 1024], use_xyz=True)]

    def _build_model(self):
        self.SA_modules = nn.ModuleList(self._build_sa())
        self.fc_layer = nn.Sequential(
            nn.Linear(1024, 512, bias=False),
            nn.BatchNorm1d(512),
            nn.ReLU(True),
            nn.Linear(512, 256, bias=False),
            nn.BatchNorm1d(256),
            nn.ReLU(True),
            nn.Dropout(0.5),
            nn.Linear(256, self.num_classes),
        )

    def _break_up_pc(self, pc):
        xyz = pc[..., 0:3].contiguous()
        features = pc[..., 3:].transpose(1, 2).contiguous() if pc.size(-1) > 3 else None
        return xyz, features

    def forward(self, pointcloud, fused=None):
        """pointcloud (B, N, 3 + input_channels) float32 on the device, every point (x, y, z, features...) -> logits (B, num_classes).
        fused: run the set-abstraction levels through ``fused_forward`` (one kernel per scale, nothing grouped in memory); None
        means exactly when the model is in eval mode and grad is disabled; True anywhere else raises."""
        if fused is None:
            fused = not self.training and not torch.is_grad_enabled()
        elif fused and (self.training or torch.is_grad_enabled()):
            raise RuntimeError("fused=True is for inference: put the model in eval() mode and call it under torch.no_grad()")
        xyz, features = self._break_up_pc(pointcloud)
        for module in self.SA_modules:
            xyz, features = module.fused_forward(xyz, features) if fused else module(xyz, features)
        return self.fc_layer(features.squeeze(-1))


class PointNet2ClassificationMSG(PointNet2ClassificationSSG):
    """Multi-scale grouping: three ball sizes at each of the two levels with centres."""

    def _build_sa(self):
        c = self.input_channels
        mid = 64 + 128 + 128
        return [PointnetSAModuleMSG(npoint=512, radii=[0.1, 0.2, 0.4], nsamples=[16, 32, 128],
                                    mlps=[[c, 32, 32, 64], [c, 64, 64, 128], [c, 64, 96, 128]], use_xyz=True),
                PointnetSAModuleMSG(npoint=128, radii=[0.2, 0.4, 0.8], nsamples=[32, 64, 128],
                                    mlps=[[mid, 64, 64, 128], [mid, 128, 128, 256], [mid, 128, 128, 256]], use_xyz=True),
                PointnetSAModule(mlp=[128 + 256 + 256, 256, 512, 1024], use_xyz=True)]
