"""Writes tests/golden/gmm.npz: the reference's own class GMM (Cluster_KMeans_GMM/GMM.py:13-71) run on its 2-D toy set.

The reference module is imported from the reference tree with pylab / matplotlib stubbed in sys.modules (GMM.py:5,8-11 import them for
its plot only); scipy's multivariate_normal.pdf is wrapped to count calls: one EM iteration makes 2 k of them (E-step + likelihood).
The data come from tests/gmm_checks.toy_data (default_rng) and np.random.seed is set right before fit, whose first draw is the
initial means (GMM.py:25).  Asserted before writing: at every iteration |(last_nll - nll) - tol| > 1e-6, so the stopping iteration
cannot flip on rounding.  Runs on the host only; needs the reference tree.

    python scripts/gen_gmm_golden.py [--reference /root/reference] [--data-seed 7] [--seed 0]
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gmm_checks  # noqa: E402


def import_reference(ref_root):
    class _Anything(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return _Anything(name)

        def __call__(self, *a, **k):
            return None

    for name in ("pylab", "matplotlib", "matplotlib.pyplot", "matplotlib.patches"):
        sys.modules[name] = _Anything(name)
    sys.path.insert(0, os.path.join(ref_root, "Cluster_KMeans_GMM"))
    import GMM as ref_gmm

    return ref_gmm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--data-seed", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gmm.npz"))
    a = ap.parse_args()
    if not os.path.isdir(a.reference):
        sys.exit("reference tree not present: goldens can only be regenerated where it is")
    ref = import_reference(a.reference)
    data = gmm_checks.toy_data(a.data_seed)
    k, tol = 3, 0.001

    calls = [0]
    pdf = ref.multivariate_normal.pdf

    def counting_pdf(*args, **kw):
        calls[0] += 1
        return pdf(*args, **kw)

    ref.multivariate_normal.pdf = counting_pdf
    try:
        np.random.seed(a.seed)
        model = ref.GMM(n_clusters=k)
        model.fit(data)
        fit_calls = calls[0]
        labels = model.predict(data)
    finally:
        ref.multivariate_normal.pdf = pdf
    assert fit_calls % (2 * k) == 0
    n_iter = fit_calls // (2 * k)

    np.random.seed(a.seed)
    means0 = np.random.random((k, data.shape[1]))
    lit = gmm_checks.fit_literal(data, means0, model.max_iter, tol)
    assert lit["n_iter"] == n_iter, (lit["n_iter"], n_iter)
    assert np.abs(lit["means"] - model.means).max() <= 1e-12 and np.abs(lit["covs"] - model.covs).max() <= 1e-12
    hist = np.concatenate([[np.inf], lit["nll_history"]])
    steps = hist[:-1] - hist[1:]
    margin = np.abs(steps - tol).min()
    assert margin > 1e-6, f"a step lies within 1e-6 of tol ({margin}): pick another seed"
    assert n_iter < model.max_iter
    print(f"{n_iter} iterations; last steps {steps[-2]:.3e}, {steps[-1]:.3e} against tol {tol}; closest to tol: {margin:.3e}")
    np.savez_compressed(a.out, data=data, data_seed=a.data_seed, np_random_seed=a.seed, means_init=means0, means=model.means, covs=model.covs,
                        weights=model.weights, labels=labels.astype(np.int64), n_iter=n_iter, tol=tol, max_iter=model.max_iter,
                        nll_history=lit["nll_history"])
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
