"""Writes tests/golden/pointnet2_semseg_keys.json: the state-dict keys and shapes of the reference's two point-wise segmentation
networks (Final_Project/pointnet2/models/pointnet2_ssg_sem.py and pointnet2_msg_sem.py), names and shapes only.

The layout is built here with plain torch containers from the layer numbers written in those two files; nothing of this package and
nothing of the reference is imported (the reference's own classes need its CUDA extension).  What the layout follows from:
``SA_modules.<i>`` is a set-abstraction module holding ``mlps.<scale>``, ``FP_modules.<i>`` a feature-propagation module holding
``mlp``; each of those is a sequence of 1x1 Conv2d (no bias), BatchNorm2d, ReLU per layer; with use_xyz (the reference's default)
every set-abstraction scale sees three more input channels; the head ``fc_lyaer`` (sic) is Conv1d (no bias), BatchNorm1d, ReLU,
Dropout, Conv1d.

    python scripts/make_semseg_keys_golden.py
"""
import json
import os

import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# set-abstraction levels: one list of layer widths per scale (feature channels first, the three coordinates are added below)
SSG_SA = [[[6, 32, 32, 64]], [[64, 64, 64, 128]], [[128, 128, 128, 256]], [[256, 256, 256, 512]]]
SSG_FP = [[128 + 6, 128, 128, 128], [256 + 64, 256, 128], [256 + 128, 256, 256], [512 + 256, 256, 256]]
MSG_SA = [[[6, 16, 16, 32], [6, 32, 32, 64]], [[96, 64, 64, 128], [96, 64, 96, 128]], [[256, 128, 196, 256], [256, 128, 196, 256]],
          [[512, 256, 256, 512], [512, 256, 384, 512]]]
MSG_FP = [[256 + 6, 128, 128], [512 + 96, 256, 256], [512 + 256, 512, 512], [1024 + 512, 512, 512]]


def shared_mlp(spec):
    layers = []
    for c_in, c_out in zip(spec[:-1], spec[1:]):
        layers += [nn.Conv2d(c_in, c_out, kernel_size=1, bias=False), nn.BatchNorm2d(c_out), nn.ReLU(True)]
    return nn.Sequential(*layers)


def network(sa, fp, num_classes=13):
    net = nn.Module()
    net.SA_modules = nn.ModuleList()
    for scales in sa:
        module = nn.Module()
        module.groupers = nn.ModuleList(nn.Module() for _ in scales)
        module.mlps = nn.ModuleList(shared_mlp([spec[0] + 3] + spec[1:]) for spec in scales)
        net.SA_modules.append(module)
    net.FP_modules = nn.ModuleList()
    for spec in fp:
        module = nn.Module()
        module.mlp = shared_mlp(spec)
        net.FP_modules.append(module)
    net.fc_lyaer = nn.Sequential(nn.Conv1d(128, 128, kernel_size=1, bias=False), nn.BatchNorm1d(128), nn.ReLU(True), nn.Dropout(0.5),
                                 nn.Conv1d(128, num_classes, kernel_size=1))
    return net


def main():
    out = {name: [[k, list(v.shape)] for k, v in network(sa, fp).state_dict().items()]
           for name, sa, fp in (("PointNet2SemSegSSG", SSG_SA, SSG_FP), ("PointNet2SemSegMSG", MSG_SA, MSG_FP))}
    path = os.path.join(ROOT, "tests", "golden", "pointnet2_semseg_keys.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{path}: {', '.join(f'{k} {len(v)} entries' for k, v in out.items())}")


if __name__ == "__main__":
    main()
