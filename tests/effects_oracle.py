"""The numpy restatement of spx_main_effects (include/spx.h): the structured rows, the predictive mean of every row from the
oracle (oracle.gp_ei_oracle.compute_ei's `stages`), and the four expressions Engine.main_effects defines its summary by.
Test-only: the product never imports this file."""
import numpy as np

from oracle import gp_ei_oracle as orc


def midpoints(T):
    return (np.arange(int(T)) + 0.5) / int(T)


def structured_rows(base, levels):
    """((D T + 1) Q, D): row (j T + k) Q + q is base[q] with coordinate j set to levels[k]; the last Q rows are base."""
    base = np.ascontiguousarray(np.atleast_2d(base), dtype=np.float64)
    levels = np.asarray(levels, dtype=np.float64).ravel()
    Q, D = base.shape
    T = levels.shape[0]
    rows = np.empty((D * T + 1, Q, D))
    rows[:] = base[None, :, :]
    for j in range(D):
        for k in range(T):
            rows[j * T + k, :, j] = levels[k]
    return rows.reshape(-1, D)


def func_m(comp, vals, hypers, rows, covar="Matern52"):
    """(H, rows): the predictive mean of every row under every hyper draw."""
    out = []
    with orc.covar(covar):
        for h in np.atleast_2d(hypers):
            st = {}
            orc.compute_ei(comp, rows, vals, h, stages=st)
            out.append(st["func_m"])
    return np.array(out)


def reduce_rows(fm, D, T, Q):
    """(curves (H, D, T), base_mean (H, Q)) from the means (H, (D T + 1) Q) of the structured rows."""
    fm = np.ascontiguousarray(fm)
    H = fm.shape[0]
    curves = np.mean(fm[:, :D * T * Q].reshape(H, D, T, Q), axis=-1)
    return curves, np.array(fm[:, D * T * Q:])


def summary(levels, curves, base_mean):
    with np.errstate(divide="ignore", invalid="ignore"):
        f0 = np.mean(base_mean, axis=1)
        total_var = np.var(base_mean, axis=1)
        effect_var = np.var(curves, axis=2)
        first_order = effect_var / total_var[:, None]
    return {"levels": np.asarray(levels, dtype=float), "curves": curves, "base_mean": base_mean, "f0": f0,
            "total_var": total_var, "effect_var": effect_var, "first_order": first_order}


def main_effects(comp, vals, hypers, base, levels=None, T=16, covar="Matern52"):
    base = np.ascontiguousarray(np.atleast_2d(base), dtype=np.float64)
    levels = midpoints(T) if levels is None else np.asarray(levels, dtype=np.float64).ravel()
    Q, D = base.shape
    fm = func_m(comp, vals, hypers, structured_rows(base, levels), covar)
    curves, base_mean = reduce_rows(fm, D, levels.shape[0], Q)
    return summary(levels, curves, base_mean)
