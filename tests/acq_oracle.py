"""Float64 oracle (numpy / scipy) of the acquisitions beside EI -- probability of improvement and the negated lower
confidence bound (include/spx.h: SPX_ACQ_PI, SPX_ACQ_LCB) -- from the moments func_m / func_v of oracle/gp_ei_oracle.py:
plain, averaged over pending fantasies, and the refinement objective (minus the acquisition summed over the draws, with its
gradient in the scaling the reference's grad_optimize_ei has: the factor one half included).

    PI   Phi((best - xi - func_m) / func_s)
    LCB  kappa func_s - func_m

Test code only: nothing in spearmint_amd imports this module."""
import numpy as np
import scipy.linalg as spla
import scipy.stats as sps

from oracle import gp_ei_oracle as orc

EI, PI, LCB = 0, 1, 2
NAMES = {EI: "EI", PI: "PI", LCB: "LCB"}


def value(kind, par, func_m, func_v, best):
    """The acquisition from the moments; func_v < 0 gives NaN (np.sqrt), for LCB with kappa = 0 too (0 * NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        func_s = np.sqrt(func_v)
        if kind == PI:
            return sps.norm.cdf((best - par - func_m) / func_s)
        if kind == LCB:
            return par * func_s - func_m
        u = (best - func_m) / func_s
        return func_s * (u * sps.norm.cdf(u) + sps.norm.pdf(u))


def terms(kind, par, func_m, func_s, best):
    """(a, da/d func_m, da/d func_v): EI's pair is the reference's (g_ei_m, g_ei_s2) = (-Phi, 0.5 phi / func_s)."""
    if kind == PI:
        u = (best - par - func_m) / func_s
        pdf = sps.norm.pdf(u)
        return sps.norm.cdf(u), -pdf / func_s, -pdf * u / (2.0 * func_s * func_s)
    if kind == LCB:
        return par * func_s - func_m, -np.ones(np.shape(func_m)) * np.ones(np.shape(func_s)), \
            par / (2.0 * func_s) * np.ones(np.shape(func_m))
    u = (best - func_m) / func_s
    ncdf, npdf = sps.norm.cdf(u), sps.norm.pdf(u)
    return func_s * (u * ncdf + npdf), -ncdf, 0.5 * npdf / func_s


def moments(comp, cand, vals, hyper):
    """func_m, func_v of every candidate under one draw (orc.compute_ei's own stage arrays)."""
    st = {}
    orc.compute_ei(comp, cand, vals, hyper, stages=st)
    return st["func_m"], st["func_v"]


def over_hypers(kind, par, comp, cand, vals, hypers, want_moments=False):
    """[M, H], as orc.ei_over_hypers lays EI out."""
    hypers = np.atleast_2d(hypers)
    out = np.zeros((cand.shape[0], hypers.shape[0]))
    mom = []
    best = np.min(vals)
    for h in range(hypers.shape[0]):
        func_m, func_v = moments(comp, cand, vals, hypers[h])
        mom.append((func_m, func_v))
        out[:, h] = value(kind, par, func_m, func_v, best)
    return (out, mom) if want_moments else out


def fantasy_values(kind, par, comp_pend, cand, hyper, fant_vals, bests):
    """(M, S): the acquisition of every candidate against every fantasy (orc.compute_ei_fantasies before its mean)."""
    mean, noise, amp2, ls = orc.unpack_hyper(hyper)
    cp_chol = spla.cholesky(orc.cov(amp2, ls, comp_pend) + noise * np.eye(comp_pend.shape[0]), lower=True)
    cand_cross = orc.cov(amp2, ls, comp_pend, cand)
    alpha = spla.cho_solve((cp_chol, True), fant_vals - mean)
    beta = spla.solve_triangular(cp_chol, cand_cross, lower=True)
    func_m = np.dot(cand_cross.T, alpha) + mean
    func_v = amp2 * (1 + 1e-6) - np.sum(beta ** 2, axis=0)
    return value(kind, par, func_m, func_v[:, np.newaxis], bests[np.newaxis, :])


def over_hypers_fantasies(kind, par, comp_pend, cand, hypers, fant, bests):
    """[M, H]: np.mean over the fantasies per draw; fant (H, n, S), bests (H, S)."""
    hypers = np.atleast_2d(hypers)
    return np.stack([np.mean(fantasy_values(kind, par, comp_pend, cand, hypers[h], fant[h], bests[h]), axis=1)
                     for h in range(hypers.shape[0])], axis=1)


def choose(acq):
    return orc.choose(acq)


# ---- the refinement objective: tests/refine_helpers.oracle with the acquisition's terms in EI's place ---------------------
def _draw(p, h, pts, kind, par):
    mean, noise, amp2, ls = orc.unpack_hyper(p.rows[h])
    X = p.X
    chol = spla.cholesky(orc.cov(amp2, ls, X) + noise * np.eye(X.shape[0]), lower=True)
    cross = orc.cov(amp2, ls, X, pts)                      # (n, P)
    cg = orc.grad_corr(ls, X, pts)                         # (n, P, D)
    beta = spla.solve_triangular(chol, cross, lower=True)
    func_s = np.sqrt(amp2 * (1 + 1e-6) - np.sum(beta ** 2, axis=0))
    gv = np.einsum("jp,jpd->pd", -2 * spla.cho_solve((chol, True), cross), cg)
    if p.branch == "fant":
        alpha = spla.cho_solve((chol, True), p.fant[h] - mean)            # (n, S)
        func_m = np.dot(cross.T, alpha) + mean                            # (P, S)
        a, g_m, g_s2 = terms(kind, par, func_m, func_s[:, None], p.bests[h][None, :])
        gm = np.einsum("js,jpd->psd", alpha, cg)
        grad = 0.5 * amp2 * (gm * g_m[:, :, None] + gv[:, None, :] * g_s2[:, :, None])
        return -np.mean(a, axis=1), np.mean(grad, axis=1)
    alpha = spla.cho_solve((chol, True), p.vals - mean)
    func_m = np.dot(cross.T, alpha) + mean
    a, g_m, g_s2 = terms(kind, par, func_m, func_s, np.min(p.vals))
    return -a, 0.5 * amp2 * (np.einsum("j,jpd->pd", alpha, cg) * g_m[:, None] + gv * g_s2[:, None])


def grad_oracle(p, pts, kind, par):
    """(f[P], g[P, D]) of a tests/refine_helpers problem (branch "plain" or "fant"), summed over the draws in draw order."""
    pts = np.atleast_2d(pts)
    f = np.zeros(pts.shape[0])
    g = np.zeros(pts.shape)
    with orc.covar(p.covar):
        for h in range(p.H):
            fh, gh = _draw(p, h, pts, kind, par)
            f += fh
            g = g + gh
    return f, g
