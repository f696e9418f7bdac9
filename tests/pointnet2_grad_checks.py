"""NumPy restatements of the fixed-order PointNet++ gradients under the rules of include/pcr.h ("PointNet++ gradients"), written from
those rules: per output the terms of the slots that name it, added one by one in ascending slot order onto +0.0f in float32.
``np.add.at`` on a float32 array performs exactly these additions (unbuffered, in the order of the index array), so it is the
restatement the device is held against; ``scatter_rows_loop`` writes the same thing out as a loop, and the host tests hold the two
against each other.  Plus the test values whose summation order shows in the bits, and the synthetic training set of the training tests."""
import os

import numpy as np

F32 = np.float32


def inverse_index(idx, n):
    """idx (B, K) int -> start (B, n + 1) int32 and slots (B, K) int32: point i's slots are slots[b, start[b, i]:start[b, i + 1]],
    ascending.  A stable sort by point keeps the slots of a point in their order."""
    idx = np.asarray(idx).reshape(len(idx), -1)
    B, K = idx.shape
    start = np.zeros((B, n + 1), dtype=np.int32)
    slots = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        slots[b] = np.argsort(idx[b], kind="stable")
        start[b, 1:] = np.cumsum(np.bincount(idx[b], minlength=n)[:n])
    return start, slots


def scatter_rows_loop(terms, idx, n, descending=False):
    """terms (B, C, K) float32, idx (B, K) -> (B, C, n) float32 by the explicit loop: slot after slot, ascending (descending: the
    same terms in the opposite order, for the test that the inputs tell the orders apart), one rounded float32 addition each."""
    B, C, K = terms.shape
    out = np.zeros((B, C, n), dtype=F32)
    order = range(K - 1, -1, -1) if descending else range(K)
    for b in range(B):
        for slot in order:
            i = idx[b, slot]
            out[b, :, i] = out[b, :, i] + terms[b, :, slot]     # float32 + float32, rounded once per channel
    return out


def scatter_rows_ordered(terms, idx, n):
    """The same sums by np.add.at, one line per (cloud, channel)."""
    terms = np.ascontiguousarray(terms, dtype=F32)
    B, C, K = terms.shape
    out = np.zeros((B, C, n), dtype=F32)
    for b in range(B):
        for c in range(C):
            np.add.at(out[b, c], idx[b], terms[b, c])
    return out


def gather_grad(grad_out, idx, n):
    """grad_out (B, C, npoint), idx (B, npoint) -> (B, C, n)."""
    return scatter_rows_ordered(grad_out, idx, n)


def group_grad(grad_out, idx, n):
    """grad_out (B, C, npoint, nsample), idx (B, npoint, nsample) -> (B, C, n); slot = j * nsample + s."""
    B, C = grad_out.shape[:2]
    return scatter_rows_ordered(grad_out.reshape(B, C, -1), idx.reshape(B, -1), n)


def three_interpolate_terms(grad_out, weight):
    """term[b, c, 3 j + k] = grad_out[b, c, j] * weight[b, j, k], a float32 product rounded once."""
    B, C, n = grad_out.shape
    return (grad_out.astype(F32)[:, :, :, None] * weight.astype(F32)[:, None, :, :]).reshape(B, C, 3 * n)


def three_interpolate_grad(grad_out, idx, weight, m):
    """grad_out (B, C, n), idx / weight (B, n, 3) -> (B, C, m)."""
    return scatter_rows_ordered(three_interpolate_terms(grad_out, weight), idx.reshape(len(idx), -1), m)


def wide_values(rng, shape):
    """Seeded normals, each scaled by a seeded power of two from 2^-20 .. 2^20: sums of them depend on the order in their last bits."""
    return (rng.normal(size=shape) * np.exp2(rng.integers(-20, 21, size=shape))).astype(F32)


def same_bits(got, want):
    """Equal raw bits; where the restatement is NaN (inf - inf) the device must be NaN too, whatever its sign and payload."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def write_shapes_dataset(root_dir, train_per_class=16, test_per_class=4, points=64, seed=0):
    """A tiny synthetic training set in the layout of pointnet2_ops/resampled_dataset.py (object_names.txt, train.txt, test.txt,
    <category>/<id>.txt with six comma-separated columns), for the training tests and scripts/pointnet2_grad_bench.py: category
    ``sphere`` (points on a sphere, outward normals) and ``cube`` (points on a cube's faces, face normals), every object scaled and
    shifted a little.  Returns the category names."""
    rng = np.random.default_rng(seed)
    names = ["sphere", "cube"]
    os.makedirs(root_dir, exist_ok=True)
    with open(os.path.join(root_dir, "object_names.txt"), "w") as f:
        f.writelines(name + "\n" for name in names)
    lists = {"train": [], "test": []}
    for name in names:
        os.makedirs(os.path.join(root_dir, name), exist_ok=True)
        for k in range(train_per_class + test_per_class):
            if name == "sphere":
                normals = rng.normal(size=(points, 3))
                normals /= np.linalg.norm(normals, axis=1, keepdims=True)
                xyz = normals.copy()
            else:
                xyz = rng.uniform(-1.0, 1.0, size=(points, 3))
                face, sign = rng.integers(0, 3, size=points), rng.choice([-1.0, 1.0], size=points)
                normals = np.zeros((points, 3))
                xyz[np.arange(points), face] = sign
                normals[np.arange(points), face] = sign
            xyz = xyz * rng.uniform(0.4, 0.6) + rng.normal(scale=0.02, size=(1, 3))
            np.savetxt(os.path.join(root_dir, name, "%06d.txt" % k), np.hstack([xyz, normals]), delimiter=",", fmt="%.6f")
            lists["train" if k < train_per_class else "test"].append("%s_%06d\n" % (name, k))
    for split, lines in lists.items():
        with open(os.path.join(root_dir, split + ".txt"), "w") as f:
            f.writelines(lines)
    return names
