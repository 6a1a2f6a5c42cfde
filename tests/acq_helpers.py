"""Shared by the CPU and GPU tests of the acquisitions beside EI: the test-only engines (the oracle behind the Engine
interface, with spx_set_acquisition's semantics), and the host run of a chooser's next() built from tests/acq_oracle.py and
scipy.optimize.  The product never imports this file."""
import numpy as np
import scipy.optimize as spo

from oracle import gp_ei_oracle as orc
from tests import acq_oracle as ao
from tests import standin_engine
from tests.helpers import OracleEngine


class AcqStandinEngine(standin_engine.Engine):
    """tests/standin_engine.Engine + the acquisition setting (recorded, and honoured by ei_step)."""

    def __init__(self, *a, **k):
        standin_engine.Engine.__init__(self, *a, **k)
        self.acq = (ao.EI, 0.0)
        self.acq_calls = []

    def set_covar(self, name):
        pass

    def set_acquisition(self, kind, par=0.0):
        self.acq = (int(kind), float(par))
        self.acq_calls.append(self.acq)

    def get_acquisition(self):
        return self.acq

    def ei_step(self, flags=0):
        if self.acq[0] == ao.EI:
            return standin_engine.Engine.ei_step(self, flags)
        a = ao.over_hypers(self.acq[0], self.acq[1], self.comp, self.cand, self.vals, self.hypers)
        self._draws = a
        mean = np.mean(a, axis=1)
        i = int(np.argmax(mean))
        self._best = (i + self.index_base, float(mean[i]))


class _P(object):
    pass


class AcqOracleEngine(OracleEngine):
    """tests/helpers.OracleEngine + set_acquisition / get_acquisition / get_moments: what Engine does with the setting, from
    the oracle.  EI goes through the parent's code untouched."""

    def __init__(self, covar="Matern52"):
        OracleEngine.__init__(self, covar)
        self.acq = (ao.EI, 0.0)
        self.acq_calls = []
        self._mom = None

    def set_acquisition(self, kind, par=0.0):
        self.acq = (int(kind), float(par))
        self.acq_calls.append(self.acq)

    def get_acquisition(self):
        return self.acq

    def get_moments(self, draw):
        return self._mom[draw]

    def ei_run(self, flags=0):
        kind, par = self.acq
        if kind == ao.EI:
            return OracleEngine.ei_run(self, flags)
        with orc.covar(self.covar):
            if self.fant is None:
                a, self._mom = ao.over_hypers(kind, par, self.comp, self.cand, self.vals, self.hypers, want_moments=True)
            else:
                a = ao.over_hypers_fantasies(kind, par, self.comp, self.cand, self.hypers, self.fant, self.bests)
        self._ei = a
        self.calls.append(("ei_run", self.cand.shape[0], self.hypers.shape[0], None if self.fant is None else self.fant.shape[2]))

    def ei_grid(self, comp, vals, cand, hypers, want_mean=True, want_draws=False, flags=0):
        kind, par = self.acq
        if kind == ao.EI:
            return OracleEngine.ei_grid(self, comp, vals, cand, hypers, want_mean, want_draws, flags)
        with orc.covar(self.covar):
            a = ao.over_hypers(kind, par, comp, cand, vals, hypers)
        self.set_observations(comp, vals); self.set_candidates(cand); self.set_hypers(hypers)
        self._last_comp, self._last_vals, self._last_rows = comp, vals, np.atleast_2d(hypers)
        self._last_time, self.fant = None, None
        mean = np.mean(a, axis=1)
        idx = int(np.argmax(mean))
        self.calls.append(("ei_grid", cand.shape[0], np.atleast_2d(hypers).shape[0]))
        return idx, float(mean[idx]), mean, (a if want_draws else None)

    def ei_grad_batch(self, points):
        kind, par = self.acq
        if kind == ao.EI:
            return OracleEngine.ei_grad_batch(self, points)
        p = _P()
        p.covar, p.H = self.covar, self.hypers.shape[0]
        if self.fant is not None:
            p.branch, p.X, p.rows, p.fant, p.bests = "fant", self.comp, self.hypers, self.fant, self.bests
        else:
            p.branch, p.X, p.vals, p.rows = "plain", self._last_comp, self._last_vals, self._last_rows
            p.H = p.rows.shape[0]
        return ao.grad_oracle(p, np.atleast_2d(points), kind, par)


def host_opt_next(grid, values, candidates, complete, rows, kind, par, grid_subset, sprayed, covar="Matern52"):
    """What GPEIOptChooser.next proposes without pending jobs, given its hyper rows and its ten sprayed points, from the
    oracle alone: pass 1 over [sprayed; grid candidates], the grid_subset best refined one at a time by
    scipy.optimize.fmin_l_bfgs_b on the oracle's objective, then the argmax over [grid candidates; refined]."""
    grid = np.asarray(grid, dtype=float)
    comp, cand, vals = grid[complete], grid[candidates], np.asarray(values, dtype=float)[complete]
    cand2 = np.vstack((sprayed, cand))
    with orc.covar(covar):
        mean1 = np.mean(ao.over_hypers(kind, par, comp, cand2, vals, rows), axis=1)
    keep = np.argsort(mean1)[-grid_subset:]
    p = _P()
    p.covar, p.branch, p.X, p.vals, p.rows, p.H = covar, "plain", comp, vals, rows, rows.shape[0]

    def objective(x):
        f, g = ao.grad_oracle(p, x[None, :], kind, par)
        return float(f[0]), g[0]
    refined = np.array([spo.fmin_l_bfgs_b(objective, cand2[k].copy(), bounds=[(0, 1)] * grid.shape[1], disp=0)[0] for k in keep])
    with orc.covar(covar):
        mean_ref = np.mean(ao.over_hypers(kind, par, comp, refined, vals, rows), axis=1)
    allm = np.concatenate((mean1[10:], mean_ref))
    best = int(np.argmax(allm))
    numcand = cand.shape[0]
    return ((numcand, refined[best - numcand]) if best >= numcand else int(candidates[best])), allm, refined
