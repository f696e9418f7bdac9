"""NumPy float64 restatements of Cluster_KMeans_GMM/GMM.py:23-70 shared by the GMM tests and by scripts/gen_gmm_golden.py.

``fit_literal`` follows the reference line by line (scipy ``multivariate_normal.pdf``); ``fit_log`` is the same loop with the E-step
and the likelihood in the log domain (include/pcr.h, deviation 1).  Both take the initial means the reference draws at GMM.py:25 and
return a dict: means (k,dim), covs (k,dim,dim), weights (k,1), n_iter, nll_history.  ``step_log`` is one E + M step with the sums the
device forms and their absolute-value counterparts, for tolerances relative to sum |term|."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


def toy_data(seed=7):
    """The reference's 2-D toy set (GMM.py:74-85,97-98: 400 / 600 / 1000 points about true_Mu with variances true_Var) from default_rng."""
    true_mu = [[0.5, 0.5], [5.5, 2.5], [1, 7]]
    true_var = [[1, 3], [2, 2], [6, 2]]
    rng = np.random.default_rng(seed)
    return np.vstack([rng.normal(m, np.sqrt(v), (c, 2)) for m, v, c in zip(true_mu, true_var, (400, 600, 1000))])


def lidar_blobs(n=1500, seed=11):
    """Three 3-D blobs at lidar range: (40,10,-1), (-30,5,0), (0,-50,1), sigma (1, 2, 0.3), n points in all, shuffled."""
    rng = np.random.default_rng(seed)
    centres = np.array([[40.0, 10.0, -1.0], [-30.0, 5.0, 0.0], [0.0, -50.0, 1.0]])
    pts = np.vstack([c + rng.normal(size=(n // 3, 3)) * np.array([1.0, 2.0, 0.3]) for c in centres])
    rng.shuffle(pts)
    return pts


def _m_step(data, gamma):
    """GMM.py:38-53."""
    n_k = np.sum(gamma, axis=1, keepdims=True)
    means = np.matmul(gamma, data) / n_k
    diff = data[np.newaxis, ...] - means[:, np.newaxis, :]
    covs = np.einsum("kn,kni,knj->kij", gamma, diff, diff) / n_k[..., np.newaxis]
    return means, covs, n_k / data.shape[0], n_k


def fit_literal(data, means0, max_iter=50, tol=0.001):
    """GMM.py:23-63 as written.  Raises what scipy raises (ValueError / LinAlgError) once a density underflows to 0/0."""
    from scipy.stats import multivariate_normal

    data = np.asarray(data, dtype=np.float64)
    k, dim = means0.shape
    means, covs, weights = np.array(means0, dtype=np.float64), np.array(k * [np.identity(dim)]), np.ones((k, 1)) / k
    last_nll, hist = float("inf"), []
    for _ in range(max_iter):
        gamma = np.empty((k, data.shape[0]))
        for i in range(k):
            gamma[i, :] = multivariate_normal.pdf(data, mean=means[i], cov=covs[i])
        gamma = gamma * weights
        with np.errstate(invalid="ignore", divide="ignore"):
            gamma = gamma / np.sum(gamma, axis=0, keepdims=True)
            means, covs, weights, _ = _m_step(data, gamma)
        gamma = np.empty((k, data.shape[0]))
        for i in range(k):
            gamma[i, :] = multivariate_normal.pdf(data, mean=means[i], cov=covs[i])
        gamma = gamma * weights
        nll = -np.sum(np.log(np.sum(gamma, axis=0)))
        hist.append(nll)
        if last_nll - nll < tol:
            break
        last_nll = nll
    return {"means": means, "covs": covs, "weights": weights, "n_iter": len(hist), "nll_history": np.array(hist)}


def log_weighted_density(data, means, covs, weights):
    """a[k,n] = log w_k + log N(x_n; mu_k, Sigma_k) through the Cholesky factor.  LinAlgError for a covariance that is not PD."""
    k, dim = means.shape
    a = np.empty((k, data.shape[0]))
    for i in range(k):
        chol = np.linalg.cholesky(covs[i])
        y = np.linalg.solve(chol, (data - means[i]).T)
        a[i] = (np.log(weights[i, 0]) - 0.5 * dim * LOG_2PI - np.sum(np.log(np.diag(chol)))) - 0.5 * np.sum(y * y, axis=0)
    return a


def responsibilities(a):
    """gamma (k,n) and the per-point log-likelihood from a (k,n)."""
    m = a.max(axis=0, keepdims=True)
    e = np.exp(a - m)
    s = e.sum(axis=0, keepdims=True)
    return e / s, (m + np.log(s))[0]


def step_log(data, means, covs, weights, about=None):
    """One E + M step in the log domain -> dict with the new parameters, nk, loglik (of the INPUT parameters), and `sums` / `abs_sums`:
    per component sum gamma, sum gamma x, sum gamma d_i d_j and the same with |.| on every term; abs_loglik.  d is taken about the
    new means, or about `about` (k,dim): the means the code under test formed, so that its second moments are compared term by term."""
    data = np.asarray(data, dtype=np.float64)
    gamma, ll = responsibilities(log_weighted_density(data, means, np.asarray(covs), np.asarray(weights).reshape(-1, 1)))
    new_means, new_covs, new_weights, n_k = _m_step(data, gamma)
    diff = data[np.newaxis, ...] - (new_means if about is None else np.asarray(about))[:, np.newaxis, :]
    return {
        "means": new_means, "covs": new_covs, "weights": new_weights, "nk": n_k[:, 0], "loglik": ll.sum(), "abs_loglik": np.abs(ll).sum(),
        "sums": {"g": n_k[:, 0], "gx": gamma @ data, "gdd": np.einsum("kn,kni,knj->kij", gamma, diff, diff)},
        "abs_sums": {"g": n_k[:, 0], "gx": gamma @ np.abs(data), "gdd": np.einsum("kn,kni,knj->kij", gamma, np.abs(diff), np.abs(diff))},
    }


def fit_log(data, means0, max_iter=50, tol=0.001):
    """GMM.py:23-63 with deviations 1 and 2 of include/pcr.h: log-domain E-step and likelihood; LinAlgError (attributes iteration,
    component) for a component with N_k = 0 / not finite or a covariance that is not positive definite."""
    data = np.asarray(data, dtype=np.float64)
    k, dim = means0.shape
    means, covs, weights = np.array(means0, dtype=np.float64), np.array(k * [np.identity(dim)]), np.ones((k, 1)) / k
    a = log_weighted_density(data, means, covs, weights)
    last_nll, hist = float("inf"), []
    for it in range(1, max_iter + 1):
        gamma, _ = responsibilities(a)
        with np.errstate(invalid="ignore", divide="ignore"):
            new = _m_step(data, gamma)
        bad = [c for c in range(k) if not (np.isfinite(new[3][c, 0]) and new[3][c, 0] > 0)]
        if not bad:
            for c in range(k):
                try:
                    np.linalg.cholesky(new[1][c])
                    if not np.isfinite(new[1][c]).all():
                        bad.append(c)
                except np.linalg.LinAlgError:
                    bad.append(c)
        if bad:
            err = np.linalg.LinAlgError(f"component {bad[0]} singular in iteration {it}")
            err.iteration, err.component = it, bad[0]
            raise err
        means, covs, weights = new[0], new[1], new[2]
        a = log_weighted_density(data, means, covs, weights)
        nll = -responsibilities(a)[1].sum()
        hist.append(nll)
        if last_nll - nll < tol:
            break
        last_nll = nll
    return {"means": means, "covs": covs, "weights": weights, "n_iter": len(hist), "nll_history": np.array(hist)}


def predict_log(data, means, covs, weights):
    """GMM.py:65-70 in the log domain -> (labels, gap between the two largest a_k per point; inf for k = 1)."""
    a = log_weighted_density(np.asarray(data, dtype=np.float64), means, covs, np.asarray(weights).reshape(-1, 1))
    srt = np.sort(a, axis=0)
    gap = srt[-1] - srt[-2] if a.shape[0] > 1 else np.full(a.shape[1], np.inf)
    return np.argmax(a, axis=0), gap
