"""Host side of the constrained chooser: the probit constraint GP's sampler and the refinement objective
(spearmint/spearmint/chooser/GPConstrainedEIChooser.py).

The sampler draws on numpy's legacy global stream in the reference's order (prior draw of ff, the joint
[amp2_c, ff] slice move, 50 elliptical-slice steps, the length-scale sweep, 20 more elliptical-slice steps, the
gain move), so a seeded run reproduces the reference's chain draw for draw.  The EI grid -- EI times P(feasible)
for every (candidate, draw) -- runs on the GPU (SPX_FLAG_CONSTRAINED); see chooser/GPConstrainedEIChooser.py."""
from __future__ import absolute_import, division

import math

import numpy as np
import numpy.random as npr
import scipy.linalg as spla
import scipy.stats as sps

from . import hostgp
from . import util


def probit_loglik(ff, labels, gain):
    """lpProbit (:1022-1029, :1146-1155): Bernoulli log-likelihood of the labels under Phi(gain ff), clipped to
    [1e-12, 1 - 1e-12]."""
    probs = sps.norm.cdf(ff * gain)
    probs[probs <= 0] = 1e-12
    probs[probs >= 1] = 1 - 1e-12
    return np.sum(labels * np.log(probs) + (1 - labels) * np.log(1 - probs))


def elliptical_slice(xx, chol_upper, log_like_fn):
    """One elliptical-slice step (:1225-1281) with angle_range = 0: the prior draw nu = U^T randn(D, 1), the level,
    the first angle, then shrinking -- three or more uniforms in that order."""
    D = xx.shape[0]
    cur = log_like_fn(xx)
    nu = np.dot(chol_upper.T, npr.randn(D, 1)).flatten()
    hh = np.log(npr.rand()) + cur
    phi = npr.rand() * 2 * math.pi
    phi_min = phi - 2 * math.pi
    phi_max = phi
    while True:
        prop = xx * np.cos(phi) + nu * np.sin(phi)
        cur = log_like_fn(prop)
        if cur > hh:
            return prop, cur
        if phi > 0:
            phi_max = phi
        elif phi < 0:
            phi_min = phi
        else:
            raise Exception("BUG DETECTED: Shrunk to current position and still not acceptable.")
        phi = npr.rand() * (phi_max - phi_min) + phi_min


class ConstraintState(object):
    """The constraint GP's chain: amp2_c, ls_c, gain and the latent vector ff (noise_c fixed at 1e-3, the mean 0.5
    stored but never used, :136-153)."""

    def __init__(self, D):
        self.ls = np.ones(D)
        self.amp2 = 1.0
        self.noise = 1e-3
        self.gain = 1.0
        self.mean = 0.5
        self.ff = None


def sample_constraint_hypers(st, comp, labels, covar, max_ls=2.0, amp2_scale=1.0, data_term=None):
    """One iteration of sample_constraint_hypers (:1014-1026) on `st`.  Returns True when ff was redrawn from the
    prior (N grew, or no ff yet): the caller then resets its ff_samples, as the reference does.

    data_term(amp2_c, ls_c, noise_c, ff) -> -sum log diag L - 0.5 ff' K^-1 ff, optional: the Cholesky of every evaluation of
    the [amp2_c, ff] move through another evaluator (the chooser's: spx_gp_logprob_rhs on the GPU), raising
    numpy.linalg.LinAlgError where spla.cholesky would; by default the host's scipy Cholesky."""
    n = comp.shape[0]
    redrawn = False
    if st.ff is None or st.ff.shape[0] < n:
        redrawn = True
        # cov(amp2_c, ls_c, comp) + 1e-6 I, lower Cholesky, times randn(N) (:1017-1022)
        c = st.amp2 * (hostgp.corr(covar, st.ls, comp) + 1e-6 * np.eye(n)) + 1e-6 * np.eye(n)
        st.ff = np.dot(spla.cholesky(c, lower=True), npr.randn(n))
    Kc = hostgp.corr(covar, st.ls, comp)
    eye = np.eye(n)
    gain = st.gain

    # _sample_constraint_noisy (:1159-1201): joint move over [amp2_c, ff]
    def logprob(h):
        amp2 = h[0]
        ff = h[1:]
        if amp2 < 0:
            return -np.inf
        if data_term is not None:
            lp = data_term(amp2, st.ls, st.noise, ff)
        else:
            chol = spla.cholesky(amp2 * (Kc + 1e-6 * eye) + st.noise * eye, lower=True)
            solve = spla.cho_solve((chol, True), ff)
            lp = -np.sum(np.log(np.diag(chol))) - 0.5 * np.dot(ff, solve)
        lp -= 0.5 * (np.log(amp2) / amp2_scale) ** 2
        return lp + probit_loglik(ff, labels, gain)

    h = util.slice_sample(np.hstack((np.array([st.amp2]), st.ff)), logprob, compwise=False)
    st.amp2 = h[0]
    st.ff = h[1:]
    # the elliptical-slice prior has the noise INSIDE the amplitude here (:1193-1196), one factor for the 50 steps
    chol = spla.cholesky(st.amp2 * ((Kc + 1e-6 * eye) + st.noise * eye), lower=False)
    ff = st.ff
    lik = lambda f: probit_loglik(f, labels, gain)
    for _ in range(50):
        ff, _lp = elliptical_slice(ff, chol, lik)
    st.ff = ff

    # _sample_constraint_ls (:1044-1103).  The length-scale log-probability is lpProbit(ff) alone -- it does not depend
    # on ls; its Cholesky (:1083-1085) of amp2_c (K + 1e-6 I) + 1e-3 I could only matter by raising, which a positive
    # amp2_c and noise_c rule out: the top-hat prior is all that is evaluated here.
    const = probit_loglik(st.ff, labels, gain)

    def ls_logprob(ls):
        if np.any(ls < 0) or np.any(ls > max_ls):
            return -np.inf
        return const

    st.ls = util.slice_sample(st.ls, ls_logprob, compwise=True)
    Kc = hostgp.corr(covar, st.ls, comp)
    # noise OUTSIDE the amplitude for these 20 steps (:1092-1093)
    chol = spla.cholesky(st.amp2 * (Kc + 1e-6 * eye) + st.noise * eye, lower=False)
    ff = st.ff
    for _ in range(20):
        ff, _lp = elliptical_slice(ff, chol, lik)
    st.ff = ff

    def gain_logprob(g):     # updateGain (:1062-1074): again only the probit term (and its Cholesky, see above)
        g = g[0] if np.ndim(g) else g
        if g < 0.01 or g > 10:
            return -np.inf
        return probit_loglik(st.ff, labels, g)

    st.gain = util.slice_sample(np.array([st.gain]), gain_logprob, compwise=True)[0]
    return redrawn


def objective_joint_logprob(comp, vals, ls, covar, noiseless, noise_scale, amp2_scale):
    """_sample_noisy / _sample_noiseless (:1122-1155, :1203-1223): the joint move's covariance is
    amp2 ((K + 1e-6 I) + noise I) -- the noise sits INSIDE the amplitude, unlike every other chooser -- with the
    horseshoe prior on the noise (noisy form only) and the log-normal prior on amp2."""
    n = comp.shape[0]
    Kp = hostgp.corr(covar, ls, comp) + 1e-6 * np.eye(n)
    lo, hi = np.min(vals), np.max(vals)

    def logprob(h):
        mean, amp2 = h[0], h[1]
        noise = 1e-3 if noiseless else h[2]
        if mean > hi or mean < lo:
            return -np.inf
        if amp2 < 0 or (not noiseless and noise < 0):
            return -np.inf
        chol = spla.cholesky(amp2 * (Kp + noise * np.eye(n)), lower=True)
        r = vals - mean
        lp = -np.sum(np.log(np.diag(chol))) - 0.5 * np.dot(r, spla.cho_solve((chol, True), r))
        if not noiseless:
            lp += np.log(np.log(1 + (noise_scale / noise) ** 2))
        lp -= 0.5 * (np.log(amp2) / amp2_scale) ** 2
        return lp

    return logprob


class RefineModel(object):
    """grad_optimize_ei (:549-803) of ONE draw, factored once: -(EI x P) at a point and its gradient.

    Quirk kept (:692-803): without pending jobs the predictive MEAN comes from the GP over the valid points, its
    VARIANCE (and that part of the gradient) from the same hypers over ALL completed points (obsv_chol_full).  With
    pending jobs the fantasies are drawn after npr.set_state(randomstate) -- the state the chooser captured at its
    first _real_init -- on a private RandomState, so the caller's stream is untouched (the reference runs this in a
    multiprocessing child).  With no violation observed the objective is plain EI (use_vanilla_ei)."""

    def __init__(self, compfull, pend, vals_full, labels, hyper, chyper, ff, covar, pending_samples, randomstate):
        mean, noise, amp2, ls = hyper
        self.covar = covar
        self.mean, self.noise, self.amp2, self.ls = mean, noise, amp2, np.asarray(ls, dtype=float)
        good = labels > 0
        comp = compfull[good, :]
        vals = vals_full[good]
        self.compfull, self.comp = compfull, comp
        self.best = np.min(vals)
        self.vanilla = bool(np.all(labels > 0) or np.all(labels <= 0))
        if not self.vanilla:
            _cmean, gain, camp2, cls = chyper
            self.gain, self.camp2, self.cls = gain, camp2, np.asarray(cls, dtype=float)
            nf = compfull.shape[0]
            cc = camp2 * (hostgp.corr(covar, self.cls, compfull) + 1e-6 * np.eye(nf)) + 1e-3 * np.eye(nf)
            self.t_alpha = spla.cho_solve((spla.cholesky(cc, lower=True), True), ff)
        self.pending = pend.shape[0] > 0
        if not self.pending:
            n = comp.shape[0]
            nf = compfull.shape[0]
            self.obsv_chol = spla.cholesky(amp2 * (hostgp.corr(covar, self.ls, comp) + 1e-6 * np.eye(n)) + noise * np.eye(n),
                                           lower=True)
            self.obsv_chol_full = spla.cholesky(amp2 * (hostgp.corr(covar, self.ls, compfull) + 1e-6 * np.eye(nf))
                                                + noise * np.eye(nf), lower=True)
            self.alpha = spla.cho_solve((self.obsv_chol, True), vals - mean)
        else:
            comp_pend = np.concatenate((comp, pend))
            npd = comp_pend.shape[0]
            n = comp.shape[0]
            cp_cov = amp2 * (hostgp.corr(covar, self.ls, comp_pend) + 1e-6 * np.eye(npd)) + noise * np.eye(npd)
            self.comp_pend_chol = spla.cholesky(cp_cov, lower=True)
            pend_cross = amp2 * hostgp.corr(covar, self.ls, comp, pend)
            pend_kappa = amp2 * (hostgp.corr(covar, self.ls, pend) + 1e-6 * np.eye(pend.shape[0]))
            obsv_chol = self.comp_pend_chol[:n, :n]
            alpha = spla.cho_solve((obsv_chol, True), vals - mean)
            beta = spla.cho_solve((obsv_chol, True), pend_cross)
            pend_m = np.dot(pend_cross.T, alpha) + mean
            pend_K = pend_kappa - np.dot(pend_cross.T, beta)
            pend_chol = spla.cholesky(pend_K, lower=True)
            rs = npr.RandomState()
            rs.set_state(randomstate)
            pend_fant = np.dot(pend_chol, rs.randn(pend.shape[0], pending_samples)) + pend_m[:, None]
            fant_vals = np.concatenate((np.tile(vals[:, np.newaxis], (1, pending_samples)), pend_fant))
            self.comp_pend = comp_pend
            self.alpha = spla.cho_solve((self.comp_pend_chol, True), fant_vals - mean)

    def _constraint(self, cand):
        ffc = np.dot((self.camp2 * hostgp.corr(self.covar, self.cls, self.compfull, cand)).T, self.t_alpha)
        return ffc, sps.norm.cdf(self.gain * ffc)

    def neg_ei_and_grad(self, x):
        cand = np.reshape(x, (-1, self.comp.shape[1]))
        amp2 = self.amp2
        func_constraint_m = 1
        if not self.vanilla:
            ffc, func_constraint_m = self._constraint(cand)
        if not self.pending:
            cand_cross = amp2 * hostgp.corr(self.covar, self.ls, self.comp, cand)
            cand_cross_full = amp2 * hostgp.corr(self.covar, self.ls, self.compfull, cand)
            beta = spla.solve_triangular(self.obsv_chol_full, cand_cross_full, lower=True)
            func_m = np.dot(cand_cross.T, self.alpha) + self.mean
            func_v = amp2 * (1 + 1e-6) - np.sum(beta ** 2, axis=0)
            func_s = np.sqrt(func_v)
            u = (self.best - func_m) / func_s
            ncdf = sps.norm.cdf(u)
            npdf = sps.norm.pdf(u)
            ei = func_s * (u * ncdf + npdf)
            constrained_ei = -np.sum(ei * func_constraint_m)
            g_ei_m = -ncdf
            g_ei_s2 = 0.5 * npdf / func_s
            grad_cross = np.squeeze(hostgp.corr_grad_wrt_first(self.covar, self.ls, self.comp, cand))
            grad_cross_full = np.squeeze(hostgp.corr_grad_wrt_first(self.covar, self.ls, self.compfull, cand))
            grad_xp_m = np.dot(self.alpha.transpose(), grad_cross)
            grad_xp_v = np.dot(-2 * spla.cho_solve((self.obsv_chol_full, True), cand_cross_full).transpose(),
                               grad_cross_full)
            grad_xp = 0.5 * amp2 * (grad_xp_m * g_ei_m + grad_xp_v * g_ei_s2)
            if self.vanilla:
                return -np.sum(ei), grad_xp.flatten()
            grad_cross_t = np.squeeze(hostgp.corr_grad_wrt_first(self.covar, self.cls, self.compfull, cand))
            gcm = np.dot(self.t_alpha.transpose(), grad_cross_t)
            gcm = 0.5 * self.camp2 * self.gain * gcm * sps.norm.pdf(self.gain * ffc)
            grad_xp = func_constraint_m * grad_xp + ei * gcm
            return constrained_ei, grad_xp.flatten()
        cand_cross = amp2 * hostgp.corr(self.covar, self.ls, self.comp_pend, cand)
        beta = spla.solve_triangular(self.comp_pend_chol, cand_cross, lower=True)
        func_m = np.dot(cand_cross.T, self.alpha) + self.mean
        func_v = amp2 * (1 + 1e-6) - np.sum(beta ** 2, axis=0)
        func_s = np.sqrt(func_v)
        u = (self.best - func_m) / func_s          # the reference uses `best`, not the fantasies' bests, here (:645)
        ncdf = sps.norm.cdf(u)
        npdf = sps.norm.pdf(u)
        ei = func_s * (u * ncdf + npdf)
        constrained_ei = -np.sum(ei * func_constraint_m)
        g_ei_m = -ncdf
        g_ei_s2 = 0.5 * npdf / func_s
        grad_cross = np.squeeze(hostgp.corr_grad_wrt_first(self.covar, self.ls, self.comp_pend, cand))
        grad_xp_m = np.dot(self.alpha.transpose(), grad_cross)
        grad_xp_v = np.dot(-2 * spla.cho_solve((self.comp_pend_chol, True), cand_cross).transpose(), grad_cross)
        grad_xp = 0.5 * amp2 * (grad_xp_m * np.tile(g_ei_m, (self.comp.shape[1], 1)).T + (grad_xp_v.T * g_ei_s2).T)
        grad_xp = np.sum(grad_xp, axis=0)
        if self.vanilla:
            return -np.sum(ei), grad_xp.flatten()
        grad_cross_t = np.squeeze(hostgp.corr_grad_wrt_first(self.covar, self.cls, self.compfull, cand))
        gcm = np.dot(self.t_alpha.transpose(), grad_cross_t)
        gcm = 0.5 * self.camp2 * self.gain * gcm * sps.norm.pdf(self.gain * ffc)
        grad_xp = func_constraint_m * grad_xp + np.sum(ei) * gcm
        return constrained_ei, grad_xp.flatten()
