"""numpy oracle of the knowledge gradient (include/spx.h: SPX_ACQ_KG), independent of the kernel's algorithm: the lines are
SORTED by slope and the lower envelope is found by the stack scan (Frazier, Powell & Dayanik 2009, algorithm 1), where the
library looks at every line on its own without a sort (csrc/kg_device.h).

    KG = min_i mu_i - E_Z[min_i (mu_i + b_i Z)] = sum_k (b_k - b_{k+1}) f(-|z_k|),     f(z) = phi(z) + z Phi(z)

value(mu, b): one line set.  lines(...) / values(...): the lines of every (draw, candidate) from a GP's moments and covariances,
as the contract builds them, and their values.  e_min_quadrature: E[min] by Simpson's rule on a dense grid, what the sum is
derived from.  Test code only: nothing in spearmint_amd imports this module."""
import numpy as np
from scipy.special import ndtr

SQRT_2PI = 2.50662827463100050242


def f(u):
    """phi(u) + u Phi(u), clamped at +0.0 from below (u <= 0 here)."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(invalid="ignore", under="ignore"):
        v = u * ndtr(u) + np.exp(-(u * u) / 2.0) / SQRT_2PI
    return np.where(v > 0.0, v, 0.0)


def envelope(mu, b):
    """(indices of the lines on the lower envelope in order of falling slope, their breakpoints).  Equal slopes: the lowest
    intercept stays, then the lowest index."""
    mu = np.asarray(mu, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    order = np.lexsort((np.arange(len(b)), mu, -b))
    keep = []
    for k in order:
        if keep and b[k] == b[keep[-1]]:
            continue
        keep.append(int(k))
    stack, zs = [keep[0]], []
    for k in keep[1:]:
        while True:
            j = stack[-1]
            z = (mu[k] - mu[j]) / (b[j] - b[k])
            if zs and z <= zs[-1]:
                stack.pop()
                zs.pop()
                continue
            break
        stack.append(k)
        zs.append(z)
    return stack, np.array(zs, dtype=np.float64)


def value(mu, b):
    mu = np.asarray(mu, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if not (np.all(np.isfinite(mu)) and np.all(np.isfinite(b))):
        return float("nan")
    stack, zs = envelope(mu, b)
    if len(stack) == 1:
        return 0.0
    db = b[stack[:-1]] - b[stack[1:]]
    return float(np.sum(db * f(-np.abs(zs))))


def lines(func_m, func_v, noise, mu_a, cov):
    """Intercepts (M, A + 1) and slopes (M, A + 1) of one draw: func_m, func_v (M,), mu_a (A,), cov (A, M)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        vs = func_v + noise
        sc = np.sqrt(vs)
        b = np.column_stack((func_v / sc, (cov / sc).T))
    b[~(vs > 0.0)] = np.nan
    mu = np.column_stack((func_m, np.broadcast_to(mu_a, (len(func_m), len(mu_a)))))
    return mu, b


def values(func_m, func_v, noise, mu_a, cov):
    mu, b = lines(func_m, func_v, noise, mu_a, cov)
    return np.array([value(mu[c], b[c]) for c in range(len(func_m))])


def e_min_quadrature(mu, b, lim=12.0, n=1 << 18):
    """E[min_i (mu_i + b_i Z)] by Simpson's rule on n intervals of [-lim, lim]; the integrand has kinks, so the error is of the
    order of h^2 x the slope jumps, h = 2 lim / n (1e-8 at the default)."""
    z = np.linspace(-lim, lim, n + 1)
    m = np.full(z.shape, np.inf)
    for a, s in zip(mu, b):
        m = np.minimum(m, a + s * z)
    w = np.ones(n + 1)
    w[1:-1:2] = 4.0
    w[2:-1:2] = 2.0
    return float(np.sum(w * m * np.exp(-z * z / 2.0)) * (2.0 * lim / n) / 3.0 / SQRT_2PI)


def gp_lines(comp, vals, cand, pts, hyper):
    """func_m, func_v (M,), mu_a (A,), cov (A, M) and the noise of one hyper draw, from the oracle's own GP (the active covar)."""
    import scipy.linalg as spla
    from oracle import gp_ei_oracle as orc
    mean, noise, amp2, ls = orc.unpack_hyper(hyper)
    _, chol, alpha = orc.posterior(comp, vals, hyper)
    kc = orc.cov(amp2, ls, comp, cand)
    ka = orc.cov(amp2, ls, comp, pts)
    beta = spla.solve_triangular(chol, kc, lower=True)
    gam = spla.solve_triangular(chol, ka, lower=True)
    func_m = np.dot(kc.T, alpha) + mean
    func_v = amp2 * (1 + 1e-6) - np.sum(beta ** 2, axis=0)
    mu_a = np.dot(ka.T, alpha) + mean
    cov = orc.cov(amp2, ls, pts, cand) - np.dot(gam.T, beta)
    return func_m, func_v, mu_a, cov, noise


def over_hypers(comp, cand, vals, pts, hypers):
    """KG of every candidate under every draw, (M, H)."""
    out = np.empty((cand.shape[0], np.atleast_2d(hypers).shape[0]))
    for d, h in enumerate(np.atleast_2d(hypers)):
        func_m, func_v, mu_a, cov, noise = gp_lines(comp, vals, cand, pts, h)
        out[:, d] = values(func_m, func_v, noise, mu_a, cov)
    return out


def unit(mu, b):
    """tests/kg_mp.py's unit of error for one line set, evaluated in float64 from this oracle's own envelope (good to a few
    per cent: a scale, not a value)."""
    stack, zs = envelope(np.asarray(mu, dtype=np.float64), np.asarray(b, dtype=np.float64))
    if len(stack) == 1:
        return 0.0
    b = np.asarray(b, dtype=np.float64)
    db = b[stack[:-1]] - b[stack[1:]]
    az = np.abs(zs)
    with np.errstate(under="ignore"):
        p = np.exp(-(az * az) / 2.0) / SQRT_2PI + az * ndtr(-az)
    return float(2.0 ** -53 * np.sum(db * p * (1.0 + az * az / 2.0)) + np.sum((db * p)[az > 37.5]) + 8 * 2.0 ** -1074 * np.sum(db))


def zmax(mu, b):
    """max |z_k| over this oracle's own envelope (0.0 without a breakpoint): what picks a set's band in tests/kg_mp.py."""
    _, zs = envelope(np.asarray(mu, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return float(np.max(np.abs(zs))) if len(zs) else 0.0
