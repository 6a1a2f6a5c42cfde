"""The float64 oracle of spx_loo (leave-one-out cross-validation without a refit, Rasmussen & Williams 5.4.2), the N
explicit refits it is an identity for, and the report the choosers write, built from numpy and scipy alone.  Test code only:
nothing in spearmint_amd imports this module."""
import numpy as np
import scipy.linalg as spla
import scipy.special as spsp

from spearmint_amd import hostgp

COVARS = hostgp.COVARS
Z95 = 1.959963984540054


def k_host(comp, hyper_row, covar="Matern52"):
    """amp2 (k + 1e-6 I) + noise I of one hyper row [mean, noise, amp2, ls...], from spearmint_amd/hostgp.py."""
    hyper_row = np.asarray(hyper_row, dtype=float)
    return hostgp.obs_cov(hyper_row[2], hyper_row[1], hyper_row[3:], np.asarray(comp, dtype=float), covar)


def loo_from_k(K, y, mean):
    """(loo_mean, loo_var, kinv_diag) of one draw from its covariance matrix: W = inv(cholesky(K)), c = the squared column
    norms of W, alpha = K^-1 (y - mean)."""
    K = np.asarray(K, dtype=float)
    n = K.shape[0]
    L = spla.cholesky(K, lower=True)
    W = spla.solve_triangular(L, np.eye(n), lower=True)
    c = np.sum(W ** 2, axis=0)
    alpha = spla.cho_solve((L, True), np.asarray(y, dtype=float) - mean)
    return y - alpha / c, 1.0 / c, c


def loo(comp, y, hyper_rows, covar="Matern52"):
    """The three (H, N) arrays of spx_loo for hyper rows (H, 3 + D)."""
    out = [loo_from_k(k_host(comp, h, covar), np.asarray(y, dtype=float), h[0]) for h in np.atleast_2d(hyper_rows)]
    return tuple(np.array([o[k] for o in out]) for k in range(3))


def loo_refits(K, y, mean):
    """(loo_mean, loo_var) by N explicit refits: the GP over all rows but i, predicting row i (noise included)."""
    K = np.asarray(K, dtype=float)
    y = np.asarray(y, dtype=float)
    n = K.shape[0]
    m, v = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        if n == 1:
            m[i], v[i] = mean, K[0, 0]
            continue
        cf = spla.cho_factor(K[np.ix_(keep, keep)], lower=True)
        k = K[keep, i]
        m[i] = mean + np.dot(k, spla.cho_solve(cf, y[keep] - mean))
        v[i] = K[i, i] - np.dot(k, spla.cho_solve(cf, k))
    return m, v


def summary(y, loo_mean, loo_var):
    """The issue's definition of Engine.loo's dict, with scipy's logsumexp."""
    y = np.asarray(y, dtype=float)
    H = loo_mean.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (y - loo_mean) / np.sqrt(loo_var)
        lpd = -0.5 * np.log(2 * np.pi * loo_var) - 0.5 * z ** 2
        mean = np.mean(loo_mean, 0)
        var = np.mean(loo_var, 0) + np.var(loo_mean, 0)
        z_mix = (y - mean) / np.sqrt(var)
        lpd_mix = spsp.logsumexp(lpd, axis=0) - np.log(H)
        return {"y": y, "loo_mean": loo_mean, "loo_var": loo_var, "z": z, "lpd": lpd, "mean": mean, "var": var, "z_mix": z_mix,
                "lpd_mix": lpd_mix, "elpd": float(np.sum(lpd_mix)), "rmse": float(np.sqrt(np.mean((y - mean) ** 2))),
                "coverage95": float(np.mean(np.abs(z_mix) <= Z95)), "outliers": np.nonzero(np.abs(z_mix) > 3)[0]}


def report(complete, comp, y, hyper_rows, covar="Matern52"):
    """What loo.txt holds, as numbers: (header dict, rows (N, 6) = grid_index value loo_mean loo_std z lpd)."""
    lm, lv, _ = loo(comp, y, hyper_rows, covar)
    s = summary(y, lm, lv)
    head = {"completed": len(y), "draws": lm.shape[0], "elpd": s["elpd"], "rmse": s["rmse"], "coverage95": s["coverage95"],
            "outliers": len(s["outliers"])}
    rows = np.column_stack((np.asarray(complete, dtype=float), s["y"], s["mean"], np.sqrt(s["var"]), s["z_mix"], s["lpd_mix"]))
    return head, rows


def parse_report(path):
    """loo.txt back into (header dict of floats, rows (N, 6))."""
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# ")
    head = dict((k, float(v)) for k, v in (kv.split("=") for kv in lines[0][2:].split()))
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[1:]]).reshape(-1, 6)
    return head, rows


def problem(N, D, H, seed, noise=1e-2):
    """Observations in the unit cube, a smooth objective with noise, and H hyper rows around sensible values."""
    rs = np.random.RandomState(seed)
    comp = rs.rand(N, D)
    y = np.sin(3 * comp[:, 0]) + np.sum(comp ** 2, axis=1) + 0.05 * rs.randn(N)
    rows = np.empty((H, 3 + D))
    for h in range(H):
        rows[h, 0] = np.mean(y) + 0.1 * rs.randn()
        rows[h, 1] = noise * (1 + 0.5 * rs.rand())
        rows[h, 2] = np.var(y) * (0.5 + rs.rand()) if N > 1 else 1.0 + rs.rand()
        rows[h, 3:] = 0.4 + 1.2 * rs.rand(D)
    return comp, y, rows
