"""Shared by the tests of spx_draw_fantasies (the pending posterior, the fantasies and Gamma formed by the library): a
numpy restatement of what the device computes -- in its factored form, with its own summation order and a hand-written
Cholesky, so that it shares no LAPACK call with hostgp.fantasize_from_factor_rows --, the seven host problems of
tests/test_host_logic.py's two fantasy tests, and the handle taken through the new entry point.  No GPU is needed to
import it."""
import numpy as np
import scipy.linalg as spla

from spearmint_amd import hostgp
from tests import pending_helpers as ph


def plain_cholesky(a):
    """Left-looking lower Cholesky, one column at a time; LinAlgError on the first pivot that is not > 0."""
    p = a.shape[0]
    c = np.zeros_like(a)
    for j in range(p):
        piv = a[j, j]
        for k in range(j):
            piv = piv - c[j, k] * c[j, k]
        if not piv > 0:
            raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % (j + 1))
        c[j, j] = np.sqrt(piv)
        for i in range(j + 1, p):
            s = a[i, j]
            for k in range(j):
                s = s - c[i, k] * c[j, k]
            c[i, j] = s / c[j, j]
    return c


def factored_form(vals, mean, noise, l_rows, gamma, z):
    """(pend_fant (P, S), bests (S), Gamma (n + P, S)) as the library forms them from the bottom P rows of the factor of
    cov([comp; pend]) + noise I and gamma = L^-1 ([vals; placeholders] - mean): rows < n of every column of Gamma are
    gamma[:n], rows n.. are T z with T = L_S^-1 C."""
    n, p = vals.shape[0], l_rows.shape[0]
    l21, ls_ = l_rows[:, :n], np.tril(l_rows[:, n:n + p])
    pend_m = np.array([sum(l21[i, j] * gamma[j] for j in range(n)) for i in range(p)]) + mean
    pend_k = np.array([[sum(ls_[i, k] * ls_[j, k] for k in range(min(i, j) + 1)) for j in range(p)] for i in range(p)])
    pend_k = pend_k - noise * np.eye(p)
    c = plain_cholesky(pend_k)
    t = np.zeros((p, p))
    for j in range(p):
        for i in range(j, p):
            s = c[i, j]
            for k in range(j, i):
                s = s - ls_[i, k] * t[k, j]
            t[i, j] = s / ls_[i, i]
    pend_fant = np.dot(c, z) + pend_m[:, None]
    bests = np.minimum(np.min(vals), np.min(pend_fant, axis=0))
    big = np.concatenate((np.tile(gamma[:n, None], (1, z.shape[1])), np.dot(t, z)))
    return pend_fant, bests, big


def host_problems():
    """(name, comp, pend, vals, hyper row, covar, z, atol factor): the four ordinary problems of
    test_fantasies_from_the_bottom_rows_of_the_factor_equal_the_reference_form (1e-9 of the fantasies' scale) and the
    three near-singular ones of test_fantasies_from_factor_rows_with_large_noise_and_nearly_duplicate_pending_points
    (1e-6), drawn as those tests draw them."""
    out = []
    rs = np.random.RandomState(4)
    for n, p, d, kname in ((30, 3, 2, "Matern52"), (120, 5, 6, "Matern52"), (65, 1, 3, "ARDSE"), (40, 4, 2, "Matern32")):
        comp, pend = rs.rand(n, d), rs.rand(p, d)
        pend[0] = comp[3] + 1e-4
        vals = np.sin(3 * comp).sum(axis=1) + 0.01 * rs.randn(n)
        row = np.concatenate(([vals.mean(), 10.0 ** rs.uniform(-4, -2), np.exp(0.5 * rs.randn())], rs.uniform(0.3, 2.0, d)))
        z = rs.randn(p, 50)
        out.append(("ordinary-%d-%d" % (n, p), comp, pend, vals, row, kname, z, 1e-9))
    rs = np.random.RandomState(11)
    for n, p, d, noise in ((60, 4, 3, 1.0), (200, 6, 5, 0.3), (90, 3, 2, 2.0)):
        comp, pend = rs.rand(n, d), rs.rand(p, d)
        pend[1] = pend[0] + 1e-5
        pend[2] = comp[7] + 1e-6
        vals = np.sin(3 * comp).sum(axis=1) + 0.01 * rs.randn(n)
        row = np.concatenate(([vals.mean(), noise, 1.0], rs.uniform(0.5, 1.5, d)))
        z = rs.randn(p, 100)
        out.append(("near-singular-%d-%d" % (n, p), comp, pend, vals, row, "Matern52", z, 1e-6))
    return out


def host_factor(comp, pend, vals, row, covar):
    """(chol of cov([comp; pend]) + noise I, gamma with zero placeholders) on the host."""
    cp = np.concatenate((comp, pend))
    chol = spla.cholesky(hostgp.obs_cov(row[2], row[1], row[3:], cp, covar), lower=True)
    gamma = spla.solve_triangular(chol, np.concatenate((vals, np.zeros(pend.shape[0]))) - row[0], lower=True)
    return chol, gamma


# ---- the handle through spx_draw_fantasies ---------------------------------------------------------------------------
def draw_pass(eng, p, cand, flags=0, entry="factor", time_model=False, z=None):
    """pending_helpers.fant_pass with the fantasies formed by the library from the problem's own normals (p.randn, the
    ones its host fantasies p.fant were formed from -- one (P, S) array shared by every draw)."""
    ph.load(eng, p, cand, time_model)
    if entry == "step":
        eng.ei_step(0)
    else:
        eng.factor()
    eng.draw_fantasies(p.randn if z is None else z, p.pend.shape[0])
    eng.ei_run(flags)
    return ph.collect(eng)


def device_fantasies(eng, H):
    """(pend_fant [H, P, S], bests [H, S]) read back."""
    got = [eng.get_pending_fantasies(h) for h in range(H)]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


def as_fant(p, pend_fant):
    """fant [H, n, S] = [tile(vals); pend_fant] -- what spx_set_fantasies takes."""
    S = pend_fant.shape[2]
    top = np.tile(p.vals[None, :, None], (pend_fant.shape[0], 1, S))
    return np.ascontiguousarray(np.concatenate((top, pend_fant), axis=1))
