"""GP expected-improvement chooser on the candidate grid, MCMC over hypers --
the MI355X drop-in for spearmint/spearmint/chooser/GPEIChooser.py.

Same plugin API (init / next), same state pickle, same sampler; the EI grid is
evaluated by libspx.so on the GPU (see _base.py)."""
from __future__ import absolute_import, print_function

import numpy as np
import numpy.random as npr

from .. import hostgp
from .. import util
from ._base import GPEIBase


def init(expt_dir, arg_string):
    args = util.unpack_args(arg_string)
    return GPEIChooser(expt_dir, **args)


class GPEIChooser(GPEIBase):
    # GPEIChooser.py:312 puts the log-normal prior on amp2 itself and its
    # noiseless sampler has no bounds check on the mean (:323-340).
    amp2_prior_on_sqrt = False
    noiseless_checks_mean = False
    max_ls = 2
    ts_allowed = True               # acq=TS: the grid argmin of one posterior sample path (_base.py: _thompson_gpu)
    kg_allowed = True               # acq=KG: the knowledge gradient over the grid (_base.py: _kg_gpu)

    def __del__(self):
        # the reference persists its hypers when the object dies (:66-83)
        try:
            self.save_state()
        except Exception:
            pass

    def next(self, grid, values, durations, candidates, pending, complete):
        # Too little data for a GP: take the first candidate (:127-128). No GPU touched.
        if complete.shape[0] < 2:
            return int(candidates[0])
        if self.D == -1:
            self._real_init(np.asarray(grid).shape[1], np.asarray(values)[complete])
        comp, cand, pend, vals = self._split(grid, values, candidates, pending, complete)

        if self.mcmc_iters <= 0:
            # ML-II point estimate instead of MCMC (:157-175): optimise the hypers on the host, fall
            # back to the defaults if that fails, then score the grid once -- the same GPU call with
            # a single hyper row (argmax of a one-column mean == argmax(ei))
            try:
                self.mean, self.amp2, self.noise, self.ls = hostgp.optimize_hypers(comp, vals, self.covar)
            except Exception:
                self.ls = np.ones(self.D)
                self.amp2 = np.std(vals)
                self.noise = 1e-3
            self._log_hypers()
            if self.acq == "TS":   # (pending jobs are ignored: no fantasies, no normals for them)
                best = self._thompson_gpu(comp, cand, vals, self.current_hyper_row()[None, :])
            elif self.acq == "KG" and pend.shape[0] == 0:
                best = self._kg_gpu(grid, comp, cand, vals, self.current_hyper_row()[None, :])
            else:
                randn = [npr.randn(pend.shape[0], self.pending_samples)] if pend.shape[0] > 0 else []
                best, _, _ = self.ei_over_hypers_gpu(comp, pend, cand, vals, self.current_hyper_row()[None, :],
                                                     randn=randn)
            if self.recommend:     # (the proposal is fixed; no random numbers from here on)
                self._recommend(grid, comp, vals, self.current_hyper_row()[None, :])
            if self.importance:    # (after the recommendation, whose factorisation it reuses)
                self._importance(grid, comp, vals, self.current_hyper_row()[None, :])
            if self.loo:           # (last: it reuses what either of the two has factored)
                self._loo(complete, comp, vals, self.current_hyper_row()[None, :])
            return int(candidates[best])
        # The reference alternates "sample hypers" and "compute_ei" (:145-151).
        # Without pending experiments compute_ei consumes no random numbers, so
        # drawing all H samples first and scoring them in one GPU call is the
        # same computation; with pending ones its fantasy normals are drawn here,
        # right after the sample they belong to.
        rows, randn = [], []
        if pend.shape[0] > 0 and self.acq != "TS":
            for _ in range(self.mcmc_iters):
                self.sample_hypers(comp, vals)
                self._log_hypers()
                rows.append(self.current_hyper_row())
                # compute_ei's only use of the RNG (:238), at the same point of the stream
                randn.append(npr.randn(pend.shape[0], self.pending_samples))
        else:       # nothing else draws random numbers between two samples: all of them in one sampler call
            def after(i):
                self._log_hypers()
                rows.append(self.current_hyper_row())
            self._lp_key = None
            self.sample_hypers_many(comp, vals, self.mcmc_iters, after)
        if self.acq == "TS":       # the chain above is that of a call without pending jobs; then one draw, one sample path
            best = self._thompson_gpu(comp, cand, vals, np.array(rows))
        elif self.acq == "KG" and pend.shape[0] == 0:   # (with pending jobs: EI over the fantasies, below -- the MES rule)
            best = self._kg_gpu(grid, comp, cand, vals, np.array(rows))
        else:
            best, _, _ = self.ei_over_hypers_gpu(comp, pend, cand, vals, np.array(rows), randn=randn)
        if self.recommend:         # (the proposal is fixed; no random numbers from here on)
            self._recommend(grid, comp, vals, np.array(rows))
        if self.importance:        # (after the recommendation, whose factorisation it reuses)
            self._importance(grid, comp, vals, np.array(rows))
        if self.loo:               # (last: it reuses what either of the two has factored)
            self._loo(complete, comp, vals, np.array(rows))
        return int(candidates[best])
