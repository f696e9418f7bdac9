"""Writes tests/golden/spectral.npz: the reference's own class spetral_clustering (Cluster_KMeans_GMM/spectral_clustering.py:7-46) run
on seeded inputs of tests/spectral_checks.py.

The reference module is imported from the reference tree; its ``LA.eig`` is wrapped to keep what it returned (``fit`` stores only the
labels).  Recorded per case: the data seed, the sorted eigenvalues, V = eigvecs[:, sorted_idx[:k]] and the labels (the partition: the
reference's KMeans is scikit-learn's k-means++ on the global RNG, seeded here right before ``fit``).  Cases:
    bridge      bridge(500, seed 0), k = 2: connected, LA.eig real
    blobs_norm  blobs_even(600, seed 0), k = 3, normalized=True: three components
    blobs_raw   the same, normalized=False
    circles     circles(600, .4, .03, 1) = sklearn.datasets.make_circles: LA.eig returns a complex pair and the class raises inside
                scikit-learn; only that fact is recorded
Asserted before writing: LA.eig came back real on the first three; the blobs split 200/200/200.  Host only; needs the reference tree.

    python scripts/gen_spectral_golden.py [--reference /root/reference] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import spectral_checks  # noqa: E402


def run_reference(ref, data, k, normalized, seed):
    kept = {}
    eig = ref.LA.eig

    def keeping_eig(L):
        kept["vals"], kept["vecs"] = eig(L)
        return kept["vals"], kept["vecs"]

    ref.LA.eig = keeping_eig
    try:
        np.random.seed(seed)
        model = ref.spetral_clustering(n_clusters=k, normalized=normalized)
        error = None
        try:
            model.fit(np.asarray(data))
        except ValueError as e:
            error = str(e).splitlines()[0]
    finally:
        ref.LA.eig = eig
    return model, kept, error


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "spectral.npz"))
    a = ap.parse_args()
    if not os.path.isdir(a.reference):
        sys.exit("reference tree not present: goldens can only be regenerated where it is")
    sys.path.insert(0, os.path.join(a.reference, "Cluster_KMeans_GMM"))
    import spectral_clustering as ref

    out = {"np_random_seed": a.seed, "cases": np.array(["bridge", "blobs_norm", "blobs_raw"])}
    for name, data, k, normalized, args in (("bridge", spectral_checks.bridge(500, 0), 2, True, [500, 0]),
                                            ("blobs_norm", spectral_checks.blobs_even(600, 0), 3, True, [600, 0]),
                                            ("blobs_raw", spectral_checks.blobs_even(600, 0), 3, False, [600, 0])):
        model, kept, error = run_reference(ref, data, k, normalized, a.seed)
        assert error is None, error
        assert np.isrealobj(kept["vals"]) and np.isrealobj(kept["vecs"]), f"{name}: LA.eig returned complex values"
        order = np.argsort(kept["vals"])
        labels = np.asarray(model.predict()).astype(np.int64)
        if name.startswith("blobs"):
            assert sorted(np.bincount(labels).tolist()) == [200, 200, 200], np.bincount(labels)
        out.update({name + "_args": np.array(args), name + "_k": k, name + "_normalized": int(normalized), name + "_eigenvalues": kept["vals"][order],
                    name + "_V": kept["vecs"][:, order[:k]], name + "_labels": labels})
        print(name, "eigenvalues", kept["vals"][order][:k + 1], "sizes", np.bincount(labels))
    X, _ = spectral_checks.circles(600, .4, .03, 1)
    _, kept, error = run_reference(ref, X, 2, True, a.seed)
    assert error is not None and np.iscomplexobj(kept["vals"]), "the reference no longer raises on the circles input"
    out.update({"circles_args": np.array([600, .4, .03, 1]), "circles_reference_raises": "ValueError: " + error})
    print("circles: the reference raises:", error)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
