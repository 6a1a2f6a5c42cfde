"""Default Spearmint chooser: GP-EI over the grid, MCMC over hypers, the best
few candidates refined by L-BFGS-B on the summed EI -- the MI355X drop-in for
spearmint/spearmint/chooser/GPEIOptChooser.py.

Both full passes over the candidate grid (GPEIOptChooser.py:269 and :293) run
on the GPU, and so does the objective of the `grid_subset` (=20) L-BFGS-B
refinements: all points that wait for an
evaluation share one spx_ei_grad_batch call (spearmint_amd/refine.py)."""
from __future__ import absolute_import, print_function

import os

import numpy as np
import numpy.random as npr
import scipy.optimize as spo

from .. import hostgp
from .. import refine
from .. import util
from ..helpers import log, unpickle
from ._base import GPEIBase, _as_bool


def init(expt_dir, arg_string):
    args = util.unpack_args(arg_string)
    return GPEIOptChooser(expt_dir, **args)


class GPEIOptChooser(GPEIBase):
    amp2_prior_on_sqrt = True       # :668
    noiseless_checks_mean = True    # :685-686
    max_ls = 2
    ts_allowed = True               # acq=TS: the grid argmin of one posterior sample path (_base.py: _thompson_gpu)
    kg_allowed = True               # acq=KG: the knowledge gradient over the grid, not refined (_base.py: _kg_gpu)
    ts_refine_allowed = True        # ts_refine=1: ... minimised off the grid from its grid_subset lowest rows (_thompson_refine)

    def __init__(self, expt_dir, covar="Matern52", mcmc_iters=10, pending_samples=100,
                 noiseless=False, burnin=100, grid_subset=20, use_multiprocessing=True, rescore_grid=0, **kw):
        GPEIBase.__init__(self, expt_dir, covar=covar, mcmc_iters=mcmc_iters,
                          pending_samples=pending_samples, noiseless=noiseless, **kw)
        self.stats_file = os.path.join(expt_dir, self.__module__ + "_hyperparameters.txt")
        self.burnin = int(burnin)
        self.needs_burnin = True
        self.grid_subset = int(grid_subset)
        # accepted for command-line compatibility; the refinement below is serial
        # (a fork-based Pool cannot share a HIP context)
        self.use_multiprocessing = _as_bool(use_multiprocessing)
        self.rescore_grid = _as_bool(rescore_grid)   # 1: score [grid; refined] again in the second pass, as the reference does
        # the host refinement (gpu_refine=0, or SPX_REFINE_MIN_N keeping the first proposals on the host) knows EI alone
        if self.acq not in ("EI", "TS") and not self._use_gpu_refine(0):      # (acq=TS: the path's own objective, on the GPU always)
            raise ValueError("acq=%s needs the refinement on the GPU at every size (allowed with gpu_refine=0 or "
                             "SPX_REFINE_MIN_N > 0: acq=EI)" % self.acq)
        self.hyper_samples = []

    # -- state -----------------------------------------------------------------
    def _state_dict(self):
        d = GPEIBase._state_dict(self)
        d["hyper_samples"] = self.hyper_samples
        return d

    def _apply_state(self, state):
        GPEIBase._apply_state(self, state)
        self.hyper_samples = state["hyper_samples"]
        self.needs_burnin = False

    def _fresh_state(self, dims, values):
        GPEIBase._fresh_state(self, dims, values)
        self.hyper_samples.append((self.mean, self.noise, self.amp2, self.ls))

    def _real_init(self, dims, values):
        self.randomstate = npr.get_state()   # replayed by the pending branch (:171, :588)
        GPEIBase._real_init(self, dims, values)

    def dump_hypers(self):
        """State pickle + human-readable table (:84-120)."""
        self.save_state()
        with open(self.stats_file, "w") as fh:
            fh.write("Mean Noise Amplitude <length scales>\n")
            fh.write("-----------ALL SAMPLES-------------\n")
            rows = [np.hstack(h) for h in self.hyper_samples]
            avg = 0 * rows[0]
            for r in rows:
                avg = avg + (1 / float(len(rows))) * r
                fh.write(" ".join(str(v) for v in r) + " \n")
            fh.write("-----------MEAN OF SAMPLES-------------\n")
            fh.write(" ".join(str(v) for v in avg) + " \n")

    def generate_stats_html(self):
        """HTML/JS snippet for the status page (web/app.py:75-80; :125-148)."""
        if not os.path.exists(self.state_pkl):
            return "Chooser not yet ready to display output"
        self._apply_state(unpickle(self.state_pkl))
        try:
            mean_mean = np.mean(np.vstack([h[0] for h in self.hyper_samples]))
            mean_noise = np.mean(np.vstack([h[1] for h in self.hyper_samples]))
            mean_ls = np.mean(np.vstack([h[3][np.newaxis, :] for h in self.hyper_samples]), 0)
            out = ('<br /><span class="label label-info">Estimated mean:</span> ' + str(mean_mean) +
                   '<br /><span class="label label-info">Estimated noise:</span> ' + str(mean_noise) +
                   '<br /><br /><span class="label label-info">Inverse parameter sensitivity'
                   ' - Gaussian Process length scales</span><br /><br />'
                   '<div id="lschart"></div><script type="text/javascript">'
                   'var lsdata = [' + ",".join(["%.2f" % v for v in mean_ls]) + '];')
        except Exception:
            return "Chooser not yet ready to display output."
        out += 'bar_chart("#lschart", lsdata, ' + str(self.max_ls) + ');</script>'
        if self.importance and os.path.exists(self.importance_file):
            # the real thing beside its stand-in: first-order sensitivity indices of the posterior mean (importance.txt)
            try:
                with open(self.importance_file) as fh:
                    rows = [ln.split() for ln in fh.read().splitlines()[1:]]
                sdata = [float(r[1]) for r in rows]
            except Exception:
                return out
            out += ('<br /><br /><span class="label label-info">Parameter sensitivity'
                    ' - first-order indices of the posterior mean</span><br /><br />'
                    '<div id="sensitivity"></div><script type="text/javascript">'
                    'var sdata = [' + ",".join(["%.2f" % v for v in sdata]) + '];'
                    'bar_chart("#sensitivity", sdata, 1);</script>')
        if self.loo and os.path.exists(self.loo_file):
            out += self._loo_chart_html()
        return out

    def _loo_chart_html(self, size=360, pad=36):
        """Predicted against observed, from loo.txt: one dot per completed job at (value, loo_mean) with a bar of
        +- 2 loo_std, and the diagonal a model that believed every run would put them on.  Inline SVG: the page's bar_chart
        draws bars only.  Rows without a finite value, mean or std are left out; nothing to draw: nothing added."""
        try:
            with open(self.loo_file) as fh:
                rows = np.array([[float(v) for v in ln.split()[1:4]] for ln in fh.read().splitlines()[1:]], dtype=float)
            rows = rows.reshape(-1, 3)
            rows = rows[np.all(np.isfinite(rows), axis=1)]
            if rows.shape[0] == 0:
                return ""
            lo = float(min(np.min(rows[:, 0]), np.min(rows[:, 1] - 2 * rows[:, 2])))
            hi = float(max(np.max(rows[:, 0]), np.max(rows[:, 1] + 2 * rows[:, 2])))
        except Exception:
            return ""
        span = (hi - lo) or 1.0

        def px(v):
            return pad + (size - 2 * pad) * (v - lo) / span

        def py(v):
            return size - px(v)
        marks = []
        for y, m, s in rows:
            marks.append('<line x1="%.1f" y1="%.1f" x2="%.1f" y2="%.1f" stroke="#999" />' % (px(y), py(m - 2 * s), px(y), py(m + 2 * s)))
            marks.append('<circle cx="%.1f" cy="%.1f" r="3" fill="#3a87ad" />' % (px(y), py(m)))
        return ('<br /><br /><span class="label label-info">Leave-one-out check'
                ' - predicted against observed, +- 2 std</span><br /><br />'
                '<svg id="loochart" width="%d" height="%d">' % (size, size) +
                '<line x1="%.1f" y1="%.1f" x2="%.1f" y2="%.1f" stroke="#ccc" />' % (px(lo), py(lo), px(hi), py(hi)) +
                "".join(marks) +
                '<text x="%d" y="%d" font-size="10">observed %.3g .. %.3g</text>' % (pad, size - 8, lo, hi) + '</svg>')

    # -- sampling ----------------------------------------------------------------
    def sample_hypers(self, comp, vals):
        GPEIBase.sample_hypers(self, comp, vals)
        self.hyper_samples.append((self.mean, self.noise, self.amp2, self.ls))

    def _sample_and_collect(self, comp, vals, n_iter, prefix):
        """n_iter x sample_hypers (one library call on the native path), each sample logged and appended like :621-628."""
        def after(i):
            self.hyper_samples.append((self.mean, self.noise, self.amp2, self.ls))
            self._log_hypers(prefix % (i + 1, n_iter))
        self._lp_key = None
        self.sample_hypers_many(comp, vals, n_iter, after)

    def hyper_rows(self):
        return np.array([np.concatenate(([h[0], h[1], h[2]], np.asarray(h[3], dtype=float)))
                         for h in self.hyper_samples])

    # -- local refinement on the host (:360-388 summed over draws) ---------------
    def _fantasy_normals(self, pend):
        """The reference restores the RNG state captured in _real_init before every
        fantasy draw (:588), so all draws share one (P, S) matrix -- and the global
        stream is left right after it."""
        out = []
        for _ in self.hyper_samples:
            npr.set_state(self.randomstate)
            out.append(npr.randn(pend.shape[0], self.pending_samples))
        return out

    def _refine(self, points, comp, vals, pend):
        """L-BFGS-B on the summed EI of each kept point (:285-289).  On the GPU all kept points are
        optimised together: every instance's next objective evaluation goes into one
        spx_ei_grad_batch call against the factorisation (and, with pending jobs, the fantasies)
        the first EI pass left resident.  Tiny problems use host models, one point at a time."""
        bounds = [(0, 1)] * comp.shape[1]
        if self.covar == "SE":   # getattr(gp, 'grad_SE') at :404 / :486
            raise AttributeError("gp has no attribute 'grad_SE': the reference's refinement cannot run with covar=SE")
        if self._use_gpu_refine(comp.shape[0]):
            return refine.lbfgs_many(self.engine().ei_grad_batch, points, bounds, log=log)
        if pend.shape[0] > 0:
            models = []
            for h in self.hyper_samples:
                npr.set_state(self.randomstate)
                models.append(hostgp.PendingPointModel(comp, pend, vals, h,
                                                       npr.randn(pend.shape[0], self.pending_samples), self.covar))
        else:
            models = [hostgp.PointModel(comp, vals, h, self.covar) for h in self.hyper_samples]

        def objective(x):
            total, grad = 0.0, np.zeros(x.shape[0])
            for m in models:
                e, g = m.neg_ei_and_grad(x)
                total += e
                grad = grad + g
            return total, grad

        out = np.array(points, dtype=float, copy=True)
        for i in range(out.shape[0]):
            log("Optimizing candidate %d/%d" % (i + 1, out.shape[0]))
            out[i, :] = spo.fmin_l_bfgs_b(objective, out[i, :].flatten(), bounds=bounds, disp=0)[0]
        return out

    # -- acq=TS, ts_refine=1 ----------------------------------------------------------
    def _thompson_refine(self, cand, idx):
        """The sample path _thompson_gpu left resident, minimised off the grid: L-BFGS-B from its grid_subset lowest rows
        (stable order) with Engine.thompson_grad_batch as the objective, all instances in one call per step
        (refine.lbfgs_many).  The refined points and the grid's winner are then valued together by that one function, and a
        refined point displaces the winner only if it is STRICTLY lower -- the MES rule, for the same reason: a point the
        optimiser did not move is a copy of a grid row with the row's value, and keeps its index.  A path with a NaN proposes
        the grid index (numpy's rule: the first NaN).  Draws no random numbers.  Returns None (the grid index stands) or x."""
        eng = self.engine()
        path = np.asarray(eng.thompson_path(0, 0), dtype=float)
        t = self.last_thompson
        t.update({"refined": False, "x": np.array(cand[idx], dtype=float, copy=True), "value": float(path[idx])})
        if np.isnan(path).any():
            return None
        keep = np.argsort(path, kind="stable")[:self.grid_subset]
        refined = refine.lbfgs_many(eng.thompson_grad_batch, cand[keep, :], [(0, 1)] * cand.shape[1], log=log)
        f_all, _ = eng.thompson_grad_batch(np.vstack((refined, cand[idx:idx + 1])))
        f_all = np.asarray(f_all, dtype=float)
        t["value"] = float(f_all[-1])
        if refined.shape[0] == 0:
            return None
        k = int(np.argmin(f_all[:-1]))
        if not f_all[k] < f_all[-1]:
            return None
        t.update({"refined": True, "x": np.array(refined[k], dtype=float, copy=True), "value": float(f_all[k])})
        return t["x"]

    # -- plugin entry ---------------------------------------------------------------
    def next(self, grid, values, durations, candidates, pending, complete):
        if complete.shape[0] < 2:
            return int(candidates[0])
        if self.D == -1:
            self._real_init(np.asarray(grid).shape[1], np.asarray(values)[complete])
        comp, cand, pend, vals = self._split(grid, values, candidates, pending, complete)
        numcand = cand.shape[0]

        # ten jittered copies of the incumbent in front of the grid (:234-238)
        best_comp = np.argmin(vals)
        cand2 = np.vstack((np.random.randn(10, comp.shape[1]) * 0.001 + comp[best_comp, :], cand))

        if self.mcmc_iters <= 0:
            raise NotImplementedError("mcmc_iters=0: the reference's own branch (GPEIOptChooser.py:300-321) cannot run -- it passes "
                                      "(comp, vals, True) where grad_optimize_ei expects (comp, pend, vals) and dies with a "
                                      "ValueError; use GPEIChooser for ML-II hypers or mcmc_iters >= 1")

        if self.needs_burnin:
            self._sample_and_collect(comp, vals, self.burnin, "BURN %d/%d] ")
            self.needs_burnin = False

        self.hyper_samples = []
        self._sample_and_collect(comp, vals, self.mcmc_iters, "%d/%d] ")
        self.dump_hypers()
        rows = self.hyper_rows()

        if self.acq == "TS":
            # Thompson sampling: the argmin of ONE sample path over the grid.  No sprayed points (their normals above are drawn
            # all the same: the generator is where an acq=EI call leaves it at this point) and no pending fantasies.
            # ts_refine=1: the path is then minimised off the grid (include/spx.h: spx_thompson_grad_batch).
            idx = self._thompson_gpu(comp, cand, vals, rows)
            x = self._thompson_refine(cand, idx) if self.ts_refine else None
            job = int(candidates[idx]) if x is None else (int(numcand), x)
            if self.recommend:
                self._recommend(grid, comp, vals, rows, refine_count=self.grid_subset)
            if self.importance:
                self._importance(grid, comp, vals, rows)
            if self.loo:
                self._loo(complete, comp, vals, rows)
            return job

        if self.acq == "KG" and pend.shape[0] == 0:
            # The knowledge gradient: the grid point of the highest value.  No sprayed points (their normals above are drawn all
            # the same: the generator is where an acq=EI call leaves it) and no refinement -- it needs the gradient of the
            # envelope, which the library does not have.  With pending jobs the call is scored with EI below: the MES rule.
            job = int(candidates[self._kg_gpu(grid, comp, cand, vals, rows)])
            if self.recommend:
                self._recommend(grid, comp, vals, rows, refine_count=self.grid_subset)
            if self.importance:
                self._importance(grid, comp, vals, rows)
            if self.loo:
                self._loo(complete, comp, vals, rows)
            return job

        # pass 1 over grid + sprayed points, keep the grid_subset best (:269-271)
        randn = self._fantasy_normals(pend) if pend.shape[0] > 0 else None
        _, mean1, _ = self.ei_over_hypers_gpu(comp, pend, cand2, vals, rows, want_draws=False, randn=randn)
        keep = np.argsort(mean1)[-self.grid_subset:]
        refined = self._refine(cand2[keep, :], comp, vals, pend)

        # pass 2 over grid + refined points (:292-299).  The reference scores the whole grid again; a
        # candidate's EI does not depend on which other candidates share the call (bit for bit: the
        # sharding tests rely on it), so the grid rows keep their pass-1 values and only the refined
        # points are scored.  rescore_grid=1 runs the literal second pass instead.
        randn = self._fantasy_normals(pend) if pend.shape[0] > 0 else None
        if self.acq == "MES" and pend.shape[0] == 0:
            # MES values a point against the y* table of the pass it was fitted in, and a second pass over other candidates
            # would fit another table (rescore_grid does not apply).  Pass 1's table is still resident: the refined points
            # and the grid's winner (by pass 1's means) are valued together by the refinement's own objective
            # (spx_ei_grad_batch: minus the sum over the draws), one function for both sides.  A refined point displaces the
            # grid's winner only if it is strictly better by that function: a point the optimiser did not move is a copy of a
            # grid row with bit for bit the row's value (a point's result does not depend on its batch), so the row keeps its
            # index instead of coming back as a new point on a rounding of two different sums.
            g_best = int(np.argmax(mean1[10:]))
            f_all, _ = self.engine().ei_grad_batch(np.vstack((refined, cand[g_best:g_best + 1])))
            v_all = -np.asarray(f_all, dtype=float)
            k_best = int(np.argmax(v_all[:-1]))
            best = numcand + k_best if v_all[k_best] > v_all[-1] else g_best
        elif self.rescore_grid:
            cand_all = np.vstack((cand, refined))
            best, _, _ = self.ei_over_hypers_gpu(comp, pend, cand_all, vals, rows, randn=randn)
        else:
            _, mean_ref, _ = self.ei_over_hypers_gpu(comp, pend, refined, vals, rows, want_draws=False, randn=randn)
            best = int(np.argmax(np.concatenate((mean1[10:], mean_ref))))
        job = (int(numcand), refined[best - numcand, :]) if best >= numcand else int(candidates[best])
        if self.recommend:         # (the proposal is fixed; no random numbers from here on)
            self._recommend(grid, comp, vals, rows, refine_count=self.grid_subset)
        if self.importance:        # (after the recommendation, whose factorisation it reuses)
            self._importance(grid, comp, vals, rows)
        if self.loo:               # (last: it reuses what either of the two has factored)
            self._loo(complete, comp, vals, rows)
        return job
