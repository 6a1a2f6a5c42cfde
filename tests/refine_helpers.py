"""Shared by the tests of spx_ei_grad_batch (the unconstrained refinement objective): seeded problems for its three
arithmetic branches -- plain EI, EI per second, EI averaged over pending fantasies --, the handle taken to the state in
which the choosers call it, and a batched float64 oracle: oracle/gp_ei_oracle.py::grad_optimize_ei* factor the covariance
again for every point and draw, this one factors once per draw and evaluates every point against that factor.
tests/test_refine_mp.py holds it to orc.grad_optimize_ei_over_hypers, so the GPU tests do not rest on an unchecked
restatement."""
import numpy as np
import scipy.linalg as spla
import scipy.stats as sps

from oracle import gp_ei_oracle as orc
from tests import constrained_refine_helpers as hp

BRANCHES = ("plain", "persec", "fant")
COVARS = ("Matern52", "Matern32", "ARDSE")


def make_problem(seed, covar="Matern52", branch="plain", N=150, D=4, H=3, S=5, n_pend=3):
    """N rows resident on the handle (with fantasies: N - n_pend observations + n_pend pending points), H draws in the
    ranges of constrained_refine_helpers.make_problem.  The time draws carry length scales, amplitude, noise and mean of
    their own, so that a mix-up of the two tables shows."""
    rs = np.random.RandomState(seed)
    p = hp.Problem()
    p.covar, p.branch, p.D, p.H = covar, branch, D, H
    p.S = S if branch == "fant" else 0
    n_pend = min(n_pend, N - 1) if branch == "fant" else 0
    n = N - n_pend
    p.comp = rs.rand(n, D)
    p.vals = np.sum((p.comp - 0.4) ** 2, axis=1) + 0.02 * rs.randn(n)
    p.rows = np.column_stack((rs.uniform(0.1, 0.3, H), rs.uniform(1e-3, 1e-2, H), rs.uniform(0.5, 1.5, H),
                              rs.uniform(0.3, 1.5, (H, D))))
    p.pend = rs.rand(n_pend, D)
    p.randn = rs.randn(n_pend, max(p.S, 1))
    p.log_durs = 0.7 * np.sum(p.comp, axis=1) / D + 0.1 * rs.randn(n)
    p.trows = np.column_stack((rs.uniform(-0.4, 0.4, H), rs.uniform(1e-3, 1e-2, H), rs.uniform(0.3, 0.9, H),
                               rs.uniform(0.4, 2.0, (H, D))))
    p.compv, p.valsv = p.comp, p.vals             # (what constrained_refine_helpers.points reads)
    p.best = np.min(p.vals)
    finish(p)
    return p


def finish(p):
    """The resident rows X and, in the fantasy branch, the fantasy columns of every draw (the first half of the
    reference's pending branch, orc.fantasize, from the problem's own normals)."""
    p.X = np.concatenate((p.comp, p.pend)) if p.branch == "fant" else p.comp
    if p.branch == "fant":
        with orc.covar(p.covar):
            fb = [orc.fantasize(p.comp, p.pend, p.vals, p.rows[h], p.randn) for h in range(p.H)]
        p.fant = np.array([x[0] for x in fb])
        p.bests = np.array([x[1] for x in fb])
    return p


def points(p, seed, n=21):
    """Half uniform, half comp[argmin] + 1e-3 randn, interleaved (constrained_refine_helpers.points)."""
    return hp.points(p, seed, n)


def setup(eng, p, cand=None):
    """The handle as the choosers leave it before the refinement: factored, with the time model or the fantasies set."""
    eng.set_covar(p.covar)
    if p.branch == "fant":
        eng.set_observations(p.X, np.concatenate((p.vals, np.zeros(p.pend.shape[0]))))
    else:
        eng.set_observations(p.comp, p.vals)
    eng.set_candidates(np.random.RandomState(1).rand(64, p.D) if cand is None else cand)
    eng.set_hypers(p.rows)
    if p.branch == "persec":
        eng.set_time_model(p.log_durs, p.trows)
    eng.factor()
    if p.branch == "fant":
        eng.set_fantasies(p.fant, p.bests)


def one_draw(p, d):
    """The same problem with draw d alone."""
    q = hp.Problem()
    q.__dict__.update(p.__dict__)
    q.H = 1
    q.rows, q.trows = p.rows[d:d + 1], p.trows[d:d + 1]
    if p.branch == "fant":
        q.fant, q.bests = p.fant[d:d + 1], p.bests[d:d + 1]
    return q


# ---- the batched host oracle ----------------------------------------------------------------------------------------------
def _ei_parts(u, func_s):
    ncdf = sps.norm.cdf(u)
    npdf = sps.norm.pdf(u)
    return func_s * (u * ncdf + npdf), -ncdf, 0.5 * npdf / func_s


def _draw(p, h, pts):
    """(-EI, gradient) of draw h at every point: orc.grad_optimize_ei / _fantasies / _per_s with one factorisation."""
    mean, noise, amp2, ls = orc.unpack_hyper(p.rows[h])
    X = p.X
    chol = spla.cholesky(orc.cov(amp2, ls, X) + noise * np.eye(X.shape[0]), lower=True)
    cross = orc.cov(amp2, ls, X, pts)                      # (n, P)
    cg = orc.grad_corr(ls, X, pts)                         # (n, P, D)
    beta = spla.solve_triangular(chol, cross, lower=True)
    func_v = amp2 * (1 + 1e-6) - np.sum(beta ** 2, axis=0)
    func_s = np.sqrt(func_v)
    gv = np.einsum("jp,jpd->pd", -2 * spla.cho_solve((chol, True), cross), cg)
    if p.branch == "fant":
        alpha = spla.cho_solve((chol, True), p.fant[h] - mean)            # (n, S)
        func_m = np.dot(cross.T, alpha) + mean                            # (P, S)
        ei, g_m, g_s2 = _ei_parts((p.bests[h][None, :] - func_m) / func_s[:, None], func_s[:, None])
        gm = np.einsum("js,jpd->psd", alpha, cg)
        grad = 0.5 * amp2 * (gm * g_m[:, :, None] + gv[:, None, :] * g_s2[:, :, None])
        return -np.mean(ei, axis=1), np.mean(grad, axis=1)
    alpha = spla.cho_solve((chol, True), p.vals - mean)
    func_m = np.dot(cross.T, alpha) + mean
    ei, g_m, g_s2 = _ei_parts((np.min(p.vals) - func_m) / func_s, func_s)
    grad = 0.5 * amp2 * (np.einsum("j,jpd->pd", alpha, cg) * g_m[:, None] + gv * g_s2[:, None])
    if p.branch == "plain":
        return -ei, grad
    t_mean, t_noise, t_amp2, t_ls = orc.unpack_hyper(p.trows[h])
    t_chol = spla.cholesky(orc.cov(t_amp2, t_ls, X) + t_noise * np.eye(X.shape[0]), lower=True)
    t_alpha = spla.cho_solve((t_chol, True), p.log_durs - t_mean)
    time_m = np.exp(np.dot(orc.cov(t_amp2, t_ls, X, pts).T, t_alpha) + t_mean)
    g_t = 0.5 * t_amp2 * np.einsum("j,jpd->pd", t_alpha, orc.grad_corr(t_ls, X, pts)) * time_m[:, None]
    return -ei / time_m, (time_m[:, None] * grad - ei[:, None] * g_t) / (time_m[:, None] ** 2)


def oracle(p, pts):
    """(f[P], g[P, D]) summed over the draws in draw order, as grad_optimize_ei_over_hypers does."""
    pts = np.atleast_2d(pts)
    f = np.zeros(pts.shape[0])
    g = np.zeros(pts.shape)
    with orc.covar(p.covar):
        for h in range(p.H):
            fh, gh = _draw(p, h, pts)
            f += fh
            g = g + gh
    return f, g


def orc_reference(p, pts):
    """The same numbers from oracle/gp_ei_oracle.py itself, one point and draw at a time."""
    f = np.zeros(pts.shape[0])
    g = np.zeros(pts.shape)
    with orc.covar(p.covar):
        for k, x in enumerate(pts):
            if p.branch == "fant":
                f[k], g[k] = orc.grad_optimize_ei_over_hypers(x, p.comp, p.vals, p.rows, pend=p.pend, randn_ps=p.randn)
            elif p.branch == "persec":
                f[k], g[k] = orc.grad_optimize_ei_over_hypers(x, p.comp, p.vals, p.rows, log_durs=p.log_durs,
                                                              time_hypers=p.trows)
            else:
                f[k], g[k] = orc.grad_optimize_ei_over_hypers(x, p.comp, p.vals, p.rows)
    return f, g
