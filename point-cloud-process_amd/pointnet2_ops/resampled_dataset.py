"""The reference's training-set classes (Final_Project/pointnet2/data/resampled_dataset.py) with its constructor arguments, directory
layout and behaviour:

    <root_dir>/object_names.txt        one category per line; the line number is the class index
    <root_dir>/train.txt, test.txt     one object per line, ``<category>_<id>``
    <root_dir>/<category>/<id>.txt     one point per line, six comma-separated columns x, y, z, nx, ny, nz

Point files are parsed with NumPy as binary64 and rounded to float32 (the reference parses them with pandas).
"""
from __future__ import annotations

import os

import numpy as np
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.sampler import SubsetRandomSampler


class KITTIPCDClsDataset(Dataset):
    def __init__(self, root_dir, filename_labels, split="train"):
        """resampled_dataset.py:9-29: root_dir holds ``filename_labels`` (the categories) and ``<split>.txt`` (the objects)."""
        self.data_root = root_dir
        with open(os.path.join(self.data_root, filename_labels)) as f:
            self.labels = [line.strip() for line in f.readlines()]
        self.label2ind = {label: ind for ind, label in enumerate(self.labels)}
        self.ind2label = {ind: label for ind, label in enumerate(self.labels)}
        with open(os.path.join(self.data_root, split + ".txt")) as f:
            self._data = [line.strip() for line in f.readlines()]

    def __len__(self):
        return len(self._data)

    def __getitem__(self, idx):
        """resampled_dataset.py:34-49 -> ((points, 6) float32, class index)."""
        label, pc_ind = self._data[idx].split("_")
        pts = np.loadtxt(os.path.join(self.data_root, label, pc_ind + ".txt"), delimiter=",", dtype=np.float64, ndmin=2)
        if pts.shape[1] != 6:
            raise ValueError(f"{label}/{pc_ind}.txt must have six comma-separated columns, not {pts.shape[1]}")
        return pts.astype(np.float32), self.label2ind[label]


class KITTIPCDClsDataset_Wrapper(object):
    def __init__(self, root_dir, config):
        """resampled_dataset.py:55-67: config carries ``batch_size`` and ``workers``."""
        self.data_root = root_dir
        self.filename_labels = "object_names.txt"
        self.size_validate = 0.20
        self.bs = config.batch_size
        self.num_workers = config.workers

    def get_dataloader(self):
        """resampled_dataset.py:69-91 -> (train, validation, test) loaders.  A fifth of the training set, drawn with
        ``np.random.shuffle`` (seed NumPy to fix it), is the validation set; both halves are sampled with ``SubsetRandomSampler``;
        every loader drops its last incomplete batch; the test loader shuffles."""
        train_dataset = KITTIPCDClsDataset(self.data_root, self.filename_labels, "train")
        dset_indices = list(range(len(train_dataset)))
        np.random.shuffle(dset_indices)
        val_split_index = int(np.floor(self.size_validate * len(train_dataset)))
        train_idx, val_idx = dset_indices[val_split_index:], dset_indices[:val_split_index]
        train_loader = DataLoader(dataset=train_dataset, shuffle=False, batch_size=self.bs, sampler=SubsetRandomSampler(train_idx),
                                  num_workers=self.num_workers, drop_last=True)
        valid_loader = DataLoader(dataset=train_dataset, shuffle=False, batch_size=self.bs, sampler=SubsetRandomSampler(val_idx),
                                  num_workers=self.num_workers, drop_last=True)
        test_dataset = KITTIPCDClsDataset(self.data_root, self.filename_labels, "test")
        test_loader = DataLoader(dataset=test_dataset, shuffle=True, batch_size=self.bs, num_workers=self.num_workers, drop_last=True)
        return train_loader, valid_loader, test_loader
