"""The reference's two classifiers (Final_Project/pointnet2/models/pointnet2_ssg_cls.py and pointnet2_msg_cls.py) and its two
point-wise segmentation networks (pointnet2_ssg_sem.py and pointnet2_msg_sem.py) as plain ``nn.Module``s over ``pointnet2_modules``:
the same layer specifications, sub-module names and order (``SA_modules.<i>...``, ``FP_modules.<i>...``, ``fc_layer.<i>``, and
``fc_lyaer.<i>`` (sic) in the segmentation networks), so the ``model_state`` of the reference's checkpoint loads with
``load_state_dict``.  The training loop of the
reference's classes (a pytorch_lightning module) is not part of them; the reference's ``train.py`` is ``pointnet2_train``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import pointnet2_utils
from .pointnet2_modules import PointnetFPModule, PointnetSAModule, PointnetSAModuleMSG, _FoldedCache, fold_pointwise_head


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


class PointNet2SemSegSSG(nn.Module):
    """Point-wise segmentation, single-scale grouping: four set-abstraction levels (1024, 256, 64 and 16 centres, 32 samples each),
    four feature-propagation modules back up to every input point, and a per-point head of two 1x1 convolutions."""

    def __init__(self, num_classes=13, input_channels=6):
        super().__init__()
        self.num_classes, self.input_channels = num_classes, input_channels
        self._build_model()
        self._folded_head = _FoldedCache(fold_pointwise_head)

    def _build_sa(self):
        c = self.input_channels
        return [PointnetSAModule(npoint=1024, radius=0.1, nsample=32, mlp=[c, 32, 32, 64], use_xyz=True),
                PointnetSAModule(npoint=256, radius=0.2, nsample=32, mlp=[64, 64, 64, 128], use_xyz=True),
                PointnetSAModule(npoint=64, radius=0.4, nsample=32, mlp=[128, 128, 128, 256], use_xyz=True),
                PointnetSAModule(npoint=16, radius=0.8, nsample=32, mlp=[256, 256, 256, 512], use_xyz=True)]

    def _build_fp(self):
        c = self.input_channels
        return [PointnetFPModule(mlp=[128 + c, 128, 128, 128]), PointnetFPModule(mlp=[256 + 64, 256, 128]),
                PointnetFPModule(mlp=[256 + 128, 256, 256]), PointnetFPModule(mlp=[512 + 256, 256, 256])]

    def _build_model(self):
        self.SA_modules = nn.ModuleList(self._build_sa())
        self.FP_modules = nn.ModuleList(self._build_fp())
        self.fc_lyaer = nn.Sequential(
            nn.Conv1d(128, 128, kernel_size=1, bias=False),
            nn.BatchNorm1d(128),
            nn.ReLU(True),
            nn.Dropout(0.5),
            nn.Conv1d(128, self.num_classes, kernel_size=1),
        )

    _break_up_pc = PointNet2ClassificationSSG._break_up_pc

    def forward(self, pointcloud, fused=None):
        """pointcloud (B, N, 3 + input_channels) float32 on the device, every point (x, y, z, features...) -> logits
        (B, num_classes, N).  fused: the set-abstraction levels and the decoder through their ``fused_forward`` and the head as one
        ``propagated_mlp`` call (nothing grouped, interpolated or concatenated in memory); None means exactly when the model is in
        eval mode and grad is disabled; True anywhere else raises."""
        if fused is None:
            fused = not self.training and not torch.is_grad_enabled()
        elif fused and (self.training or torch.is_grad_enabled()):
            raise RuntimeError("fused=True is for inference: put the model in eval() mode and call it under torch.no_grad()")
        xyz, features = self._break_up_pc(pointcloud)
        l_xyz, l_features = [xyz], [features]
        for module in self.SA_modules:
            xyz, features = module.fused_forward(l_xyz[-1], l_features[-1]) if fused else module(l_xyz[-1], l_features[-1])
            l_xyz.append(xyz)
            l_features.append(features)
        for i in range(-1, -(len(self.FP_modules) + 1), -1):
            module = self.FP_modules[i]
            l_features[i - 1] = (module.fused_forward if fused else module)(l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])
        return self.fused_head(l_features[0]) if fused else self.fc_lyaer(l_features[0])

    def fused_head(self, features):
        """``fc_lyaer`` in eval mode on features (B, 128, N) as one ``propagated_mlp`` call without known points: the batch norm folded
        into the first convolution, dropout the identity, no ReLU behind the last layer."""
        layers, relu_last = self._folded_head.get(0, self.fc_lyaer)
        return pointnet2_utils.propagated_mlp(None, None, None, features.transpose(1, 2).contiguous(), [w for w, _ in layers],
                                              [b for _, b in layers], relu_last=relu_last)

    def predict_labels(self, pointcloud):
        """The class of every point, (B, N) int64: the argmax over the classes of the fused logits.  Puts the model in eval mode."""
        self.eval()
        with torch.no_grad():
            return self.forward(pointcloud, fused=True).argmax(dim=1)


class PointNet2SemSegMSG(PointNet2SemSegSSG):
    """Point-wise segmentation, multi-scale grouping: two ball sizes at each of the four levels.  The two deepest decoder modules are
    512 wide, beyond what the fused kernel takes, and run as torch ops on their 256 and 64 points in either mode."""

    def _build_sa(self):
        c = self.input_channels
        c0, c1, c2 = 32 + 64, 128 + 128, 256 + 256
        return [PointnetSAModuleMSG(npoint=1024, radii=[0.05, 0.1], nsamples=[16, 32], mlps=[[c, 16, 16, 32], [c, 32, 32, 64]], use_xyz=True),
                PointnetSAModuleMSG(npoint=256, radii=[0.1, 0.2], nsamples=[16, 32], mlps=[[c0, 64, 64, 128], [c0, 64, 96, 128]], use_xyz=True),
                PointnetSAModuleMSG(npoint=64, radii=[0.2, 0.4], nsamples=[16, 32], mlps=[[c1, 128, 196, 256], [c1, 128, 196, 256]], use_xyz=True),
                PointnetSAModuleMSG(npoint=16, radii=[0.4, 0.8], nsamples=[16, 32], mlps=[[c2, 256, 256, 512], [c2, 256, 384, 512]], use_xyz=True)]

    def _build_fp(self):
        c = self.input_channels
        c0, c1, c2, c3 = 32 + 64, 128 + 128, 256 + 256, 512 + 512
        return [PointnetFPModule(mlp=[256 + c, 128, 128]), PointnetFPModule(mlp=[512 + c0, 256, 256]),
                PointnetFPModule(mlp=[512 + c1, 512, 512]), PointnetFPModule(mlp=[c3 + c2, 512, 512])]
