"""Constrained expected improvement: EI of the objective GP (valid results only) times the probability of not
violating a constraint from a probit GP over all completed jobs -- the MI355X drop-in for
spearmint/spearmint/chooser/GPConstrainedEIChooser.py.

A job "violates the constraint" when its value is NaN, +-inf or equal to ``constraint_violating_value``.
The EI grid (EI_d x P_d for every candidate and draw, the mean over draws, the argmax) is one libspx pass with
SPX_FLAG_CONSTRAINED; the constraint GP's [amp2_c, ff] move evaluates through spx_gp_logprob_rhs and the objective's
length-scale sweep through spx_gp_logprob; the 20-point refinement evaluates -(EI x P) and its gradient for all waiting
points and draws in one spx_constrained_ei_grad_batch call (gpu_refine=0: constrained.RefineModel on the host, the
oracle of that call); the rest of both samplers runs on the host (constrained.py).

Reference behaviour reproduced on purpose (each changes proposals):
  1. constraint_hyper_samples is never cleared: draw d pairs hyper_samples[d] with the d-th constraint sample
     EVER taken by this object -- burn-in samples on a fresh start (:410-420);
  2. the draws all use ONE latent vector, ff_samples[H-1], which the comp_preds loop leaves in self.ff (:259-267);
     the next call's chain starts from there too, with the constraint hypers of sample H-1;
  3. with no violation yet the factor is Phi(gain_d), not 1 (:816-842);
  4. the spray centre is argmin over ALL completed values -- a NaN wins (:216-217);
  5. the refinement objective's variance comes from the GP over all completed points (:692-803), and with
     pending jobs its fantasies from the RNG state of the first _real_init (:609);
  6. mcmc_iters <= 0 raises; fewer than 2 completed or 2 valid jobs return candidates[0].
Deliberate divergences: constraint_gain is written to the state pickle (the reference reads it back but never
writes it, so its every restart raises KeyError); a pickle without it reads as gain 1.  pending_samples is an int.
visualize2D is accepted and ignored."""
from __future__ import absolute_import, print_function

import os
import time

import numpy as np
import numpy.random as npr

from .. import constrained as con
from .. import hostgp
from .. import refine
from .. import util
from ..helpers import log, pickle_atomically, unpickle
from ._base import GPEIBase, _as_bool


def init(expt_dir, arg_string):
    args = util.unpack_args(arg_string)
    return GPConstrainedEIChooser(expt_dir, **args)


class GPConstrainedEIChooser(GPEIBase):
    acq_allowed = ("EI",)           # PI / LCB are not defined with a constraint model (include/spx.h: spx_set_acquisition)
    recommend_allowed = False
    importance_allowed = False
    loo_allowed = False
    max_ls = 2
    noise_scale = 0.1
    amp2_scale = 1
    constraint_max_ls = 2
    constraint_amp2_scale = 1

    def __init__(self, expt_dir, covar="Matern52", mcmc_iters=20, pending_samples=100, noiseless=False, burnin=100,
                 grid_subset=20, constraint_violating_value=np.inf, verbosity=0, visualize2D=False, **kw):
        GPEIBase.__init__(self, expt_dir, covar=covar, mcmc_iters=mcmc_iters, pending_samples=pending_samples,
                          noiseless=noiseless, **kw)
        self.stats_file = os.path.join(expt_dir, self.__module__ + "_hyperparameters.txt")
        self.burnin = int(burnin)
        self.needs_burnin = True
        self.grid_subset = int(grid_subset)
        self.bad_value = float(constraint_violating_value)
        self.verbosity = int(verbosity)
        if _as_bool(visualize2D):
            log("visualize2D is ignored: no plots on this path")
        self.hyper_samples = []
        self.constraint_hyper_samples = []
        self.ff_samples = []
        self.cst = None

    # -- state (:85-182) --------------------------------------------------------------
    def _state_dict(self):
        d = GPEIBase._state_dict(self)
        d.update({"constraint_ls": self.cst.ls, "constraint_amp2": self.cst.amp2, "constraint_noise": self.cst.noise,
                  "constraint_mean": self.cst.mean, "constraint_gain": self.cst.gain})
        return d

    def _apply_state(self, state):
        GPEIBase._apply_state(self, state)
        self.cst = con.ConstraintState(self.D)
        self.cst.ls = state["constraint_ls"]
        self.cst.amp2 = state["constraint_amp2"]
        self.cst.noise = state["constraint_noise"]
        self.cst.mean = state["constraint_mean"]
        # the reference never writes this key (dump_hypers :87-100) yet reads it back (:149): a pickle without it
        # (the reference's own) is read here as the initial gain
        self.cst.gain = state.get("constraint_gain", 1)
        self.needs_burnin = False

    def _real_init(self, dims, values):
        self.randomstate = npr.get_state()      # (:123) what the pending refinement objective restarts from
        self.locker.lock_wait(self.state_pkl)
        try:
            if os.path.exists(self.state_pkl):
                self._apply_state(unpickle(self.state_pkl))
            else:
                good = np.nonzero(np.logical_and(values != self.bad_value, np.isfinite(values)))[0]
                self.D = dims
                self.ls = np.ones(self.D)
                self.amp2 = np.std(values[good]) + 1e-4
                self.noise = 1e-3
                self.mean = np.mean(values[good])
                self.cst = con.ConstraintState(self.D)
        finally:
            self.locker.unlock(self.state_pkl)

    def dump_hypers(self):
        self.save_state()
        with open(self.stats_file, "w") as fh:        # (:104-120)
            fh.write("Mean Noise Amplitude <length scales>\n")
            fh.write("-----------ALL SAMPLES-------------\n")
            meanhyps = 0 * np.hstack(self.hyper_samples[0])
            for i in self.hyper_samples:
                hyps = np.hstack(i)
                meanhyps += (1 / float(len(self.hyper_samples))) * hyps
                fh.write("".join(str(j) + " " for j in hyps) + "\n")
            fh.write("-----------MEAN OF SAMPLES-------------\n")
            fh.write("".join(str(j) + " " for j in meanhyps) + "\n")

    # -- sampling ---------------------------------------------------------------------
    def _constraint_engine(self, comp):
        """A handle of its own holding the completed points for spx_gp_logprob_rhs (the objective's engine holds the valid
        points; the constraint GP's right-hand side changes with every proposal of the [amp2_c, ff] move)."""
        if getattr(self, "_ceng", None) is None:
            from ..engine import Engine
            self._ceng = Engine(self.device, self.lib_path)
            self._ceng.set_covar(self.covar)
            self._ceng_key = None
        key = (comp.shape, comp.tobytes())
        if self._ceng_key != key:
            self._ceng.set_observations(comp, np.zeros(comp.shape[0]))
            self._ceng_key = key
        return self._ceng

    def _constraint_data_term(self, comp):
        if not self._use_gpu_logprob(comp.shape[0]):
            return None
        eng = self._constraint_engine(comp)

        def data_term(amp2, ls, noise, ff):
            row = np.concatenate(([0.0, noise, amp2], np.asarray(ls, dtype=float)))[None, :]
            lp = eng.gp_logprob_rhs(row, np.asarray(ff, dtype=float)[None, :])[0]
            if np.isneginf(lp):     # spla.cholesky raises here in the reference (:1180)
                raise np.linalg.LinAlgError("constraint covariance not positive definite")
            return lp
        return data_term

    def __getstate__(self):
        d = GPEIBase.__getstate__(self)
        d["_ceng"] = None
        return d

    def sample_constraint_hypers(self, comp, labels):
        if con.sample_constraint_hypers(self.cst, comp, labels, self.covar, self.constraint_max_ls,
                                        self.constraint_amp2_scale, data_term=self._constraint_data_term(comp)):
            self.ff_samples = []
        self.constraint_hyper_samples.append((self.cst.mean, self.cst.gain, self.cst.amp2, self.cst.ls))
        self.ff_samples.append(self.cst.ff)

    def sample_hypers(self, comp, vals):
        """:1105-1114.  The joint move's covariance has the noise inside the amplitude (:1129-1131, :1216-1218): its
        own host log-probability.  The length-scale sweep is the usual amp2 (K + 1e-6 I) + noise I -- the GPU path of
        the other choosers."""
        if self.noiseless:
            self.noise = 1e-3
        lp = con.objective_joint_logprob(comp, vals, self.ls, self.covar, self.noiseless, self.noise_scale,
                                         self.amp2_scale)
        h = util.slice_sample(np.array([self.mean, self.amp2, self.noise]), lp, compwise=False)
        self.mean, self.amp2 = h[0], h[1]
        self.noise = 1e-3 if self.noiseless else h[2]
        self._lp_key = None
        self.ls = self._draw_ls(comp, vals, self.mean, self.amp2, self.noise, self.ls, self.max_ls)
        self.hyper_samples.append((self.mean, self.noise, self.amp2, self.ls))

    # -- the hot path -----------------------------------------------------------------
    def _draw_rows(self):
        H = self.mcmc_iters
        rows = np.array([np.concatenate(([h[0], h[1], h[2]], np.asarray(h[3], dtype=float)))
                         for h in self.hyper_samples[:H]])
        # quirk 1: the first H entries of the never-cleared list; (mean, gain, amp2, ls) -> [gain, noise_c, amp2_c, ls_c]
        crows = np.array([np.concatenate(([c[1], self.cst.noise, c[2]], np.asarray(c[3], dtype=float)))
                          for c in self.constraint_hyper_samples[:H]])
        return rows, crows

    def ei_over_hypers(self, comp, pend, cand, vals, labels):
        """overall_ei[M, H] (:410-426): one GPU pass, EI_d x P_d per (candidate, draw)."""
        rows, crows = self._draw_rows()
        good = labels > 0
        compv, valsv = comp[good, :], vals[good]
        all_valid = bool(np.all(labels > 0) or np.all(labels <= 0))
        eng = self.engine()
        from ..engine import FLAG_CONSTRAINED
        self._lp_key = None
        H = rows.shape[0]
        if pend.shape[0] > 0:
            randn = [npr.randn(pend.shape[0], self.pending_samples) for _ in range(H)]   # (:902, once per draw)
            comp_pend = np.concatenate((compv, pend))
            eng.set_observations(comp_pend, np.concatenate((valsv, np.zeros(pend.shape[0]))))
        else:
            eng.set_observations(compv, valsv)
        eng.set_candidates(cand)
        eng.set_hypers(rows)
        if all_valid:
            eng.set_constraint_model(np.zeros((0, comp.shape[1])), np.zeros(0), crows)
        else:
            eng.set_constraint_model(comp, self.cst.ff, crows)     # quirk 2: self.ff, the same for every draw
        if pend.shape[0] > 0:
            eng.factor()
            self._set_fantasies(eng, valsv, rows, compv.shape[0], pend.shape[0], self.pending_samples, randn, per_draw=True)
            eng.ei_run(FLAG_CONSTRAINED)
        else:
            eng.ei_step(FLAG_CONSTRAINED)
        warning = eng.last_warning()
        if warning:
            log("libspx " + warning)
        draws = eng.ei_draws()
        overall = np.zeros((cand.shape[0], self.mcmc_iters))
        overall[:, :H] = draws
        self.last_overall_ei = overall
        return overall

    def _refine_gpu(self, points, comp, pend, vals, labels):
        """The 20 L-BFGS-B problems against what the grid pass left resident: every waiting point of every instance goes
        through one spx_constrained_ei_grad_batch call (valid points or [valid; pend] factored, the constraint model
        factored).  With pending jobs the objective's fantasies are not the grid pass's: they restart from the RNG state
        of the first _real_init (quirk 5), the same normals for every draw, on a private generator."""
        eng = self.engine()
        good = labels > 0
        valsv = vals[good]
        if pend.shape[0] > 0:
            rows, _crows = self._draw_rows()
            rs = npr.RandomState()
            rs.set_state(self.randomstate)
            randn = rs.randn(pend.shape[0], self.pending_samples)
            self._set_fantasies(eng, valsv, rows, valsv.shape[0], pend.shape[0], self.pending_samples, randn, per_draw=False)
        best = np.min(valsv)
        return refine.lbfgs_many(lambda X: eng.constrained_ei_grad_batch(X, best), points, [(0, 1)] * comp.shape[1],
                                 log=log)

    def _refine(self, points, comp, pend, vals, labels):
        # (covar=SE: the reference's refinement raises AttributeError -- gp has no grad_SE -- and the host path does)
        if self.covar != "SE" and self._use_gpu_refine(int(np.sum(labels > 0))):
            return self._refine_gpu(points, comp, pend, vals, labels)
        rows = self.hyper_samples[:self.mcmc_iters]
        crows = self.constraint_hyper_samples[:self.mcmc_iters]
        models = [con.RefineModel(comp, pend, vals, labels, h, c, self.cst.ff, self.covar, self.pending_samples,
                                  self.randomstate) for h, c in zip(rows, crows)]

        def batch(X):
            f = np.zeros(X.shape[0])
            g = np.zeros(X.shape)
            for k in range(X.shape[0]):
                for m in models:
                    e, gk = m.neg_ei_and_grad(X[k])
                    f[k] += e
                    g[k] = g[k] + gk
            return f, g

        return refine.lbfgs_many(batch, points, [(0, 1)] * comp.shape[1], log=log, serial=True)

    # -- plugin entry (:190-408) -------------------------------------------------------
    def next(self, grid, values, durations, candidates, pending, complete):
        if complete.shape[0] < 2:
            return int(candidates[0])
        comp, cand, pend, vals = self._split(grid, values, candidates, pending, complete)
        idx = np.logical_and(vals != self.bad_value, np.isfinite(vals))
        goodvals = np.nonzero(idx)[0]
        log("Found %d constraint violating jobs" % (vals.shape[0] - goodvals.shape[0]))
        log("Received %d valid results" % goodvals.shape[0])
        if goodvals.shape[0] < 2:
            return int(candidates[0])
        labels = np.zeros(vals.shape[0])
        labels[goodvals] = 1
        if self.D == -1:
            self._real_init(np.asarray(grid).shape[1], np.asarray(values, dtype=float)[complete])
        numcand = cand.shape[0]
        best_comp = np.argmin(vals)       # quirk 4: over ALL completed values
        cand2 = np.vstack((npr.randn(10, comp.shape[1]) * 0.001 + comp[best_comp, :], cand))
        if self.mcmc_iters <= 0:
            raise Exception("mcmc_iters <= 0")
        compv, valsv = comp[goodvals, :], vals[goodvals]
        t0 = time.perf_counter()      # (phase times of this call: last_phase_s, scripts/bench_constrained.py)
        if self.needs_burnin:
            for it in range(self.burnin):
                self.sample_constraint_hypers(comp, labels)
                self.sample_hypers(compv, valsv)
                self._log_hypers("BURN %d/%d] " % (it + 1, self.burnin))
            self.needs_burnin = False
        self.hyper_samples = []
        for it in range(self.mcmc_iters):
            self.sample_constraint_hypers(comp, labels)
            self.sample_hypers(compv, valsv)
            if self.verbosity > 0:
                self._log_hypers("%d/%d] " % (it + 1, self.mcmc_iters))
        self.dump_hypers()
        # the comp_preds loop (:259-267) leaves ff_samples[H-1] and constraint sample H-1 in place (quirk 2)
        H = self.mcmc_iters
        self.cst.ff = self.ff_samples[H - 1]
        c = self.constraint_hyper_samples[H - 1]
        self.cst.mean, self.cst.gain, self.cst.amp2, self.cst.ls = c
        self.mean, self.noise, self.amp2, self.ls = self.hyper_samples[H - 1]

        t1 = time.perf_counter()
        overall = self.ei_over_hypers(comp, pend, cand2, vals, labels)
        t2 = time.perf_counter()
        inds = np.argsort(np.mean(overall, axis=1))[-self.grid_subset:]
        cand2 = cand2[inds, :]
        refined = self._refine(cand2, comp, pend, vals, labels)
        t3 = time.perf_counter()
        cand = np.vstack((cand, refined, cand2))          # (:384-398: the refined points, then their starting points)
        overall = self.ei_over_hypers(comp, pend, cand, vals, labels)
        best_cand = int(np.argmax(np.mean(overall, axis=1)))
        self.last_phase_s = {"samplers": t1 - t0, "grid_pass": t2 - t1, "refine": t3 - t2,
                             "second_pass": time.perf_counter() - t3}
        self.dump_hypers()
        if best_cand >= numcand:
            return (int(numcand), cand[best_cand, :])
        return int(candidates[best_cand])
