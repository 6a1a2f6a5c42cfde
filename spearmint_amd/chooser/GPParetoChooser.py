"""Two objectives, value against run time: every job reports a value and a duration, and this chooser spends the next job
on extending the trade-off between them -- the grid candidate with the largest expected hypervolume improvement (EHVI)
over the front of the completed jobs, on the GPU (include/spx.h: SPX_ACQ_EHVI).  The reference has no such chooser.

Objectives, both minimised: the job's value, and log(duration).  The two GPs, their hyper-parameter state, its pickle and
the slice sampling of both per call are GPEIperSecChooser's, which this class extends: from one seed both choosers sample
the same hyper chains.  Arguments beyond that chooser's: ref1=auto|<float>, ref2=auto|<float> -- the reference point the
hypervolume is measured from (ref2 in log-seconds); auto: pareto.reference_point of the completed jobs.  Completed jobs
that do not lie strictly inside a given reference point are left out of the front.

Grid-based, like GPEIChooser: next() returns the grid's argmax; there is no refinement off the grid.  Pending jobs follow
the deterministic "believer" rule: a small EHVI pass scores the pending rows as candidates, the believed values of both
objectives are np.mean over the draws of the two func_m, and these are appended to the observations and to the second
values of the main pass.  The front still comes from completed jobs only, and no random number is drawn.

Out of scope: more than two objectives, correlated objectives, several GPUs, and a second objective other than the
duration (the engine itself takes any second value vector)."""
from __future__ import absolute_import, print_function

import os
import tempfile

import numpy as np

from .. import pareto
from .. import util
from ..helpers import log
from .GPEIperSecChooser import GPEIperSecChooser


def init(expt_dir, arg_string):
    args = util.unpack_args(arg_string)
    return GPParetoChooser(expt_dir, **args)


def _parse_ref(name, v):
    if str(v).strip().lower() == "auto":
        return None
    try:
        out = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s=%r is not a reference value (allowed: auto, or a finite number)" % (name, v))
    if not np.isfinite(out):
        raise ValueError("%s=%r is not a reference value (allowed: auto, or a finite number)" % (name, v))
    return out


class GPParetoChooser(GPEIperSecChooser):

    def __init__(self, expt_dir, ref1="auto", ref2="auto", **kw):
        for name in ("acq", "acq_par"):
            if name in kw:
                raise ValueError("%s= is not available on GPParetoChooser: it scores with the expected hypervolume "
                                 "improvement (allowed: leave it out)" % name)
        if int(kw.get("ndev", 1)) > 1:
            raise ValueError("ndev=%d is not available on GPParetoChooser: the two GPs' moments of every candidate live on one "
                             "device (allowed: ndev=1)" % int(kw["ndev"]))
        if "ref_compat" in kw and int(kw["ref_compat"]):
            raise ValueError("ref_compat=1 is not available on GPParetoChooser (allowed: ref_compat=0)")
        self.ref1, self.ref2 = _parse_ref("ref1", ref1), _parse_ref("ref2", ref2)
        GPEIperSecChooser.__init__(self, expt_dir, **kw)     # (recommend / importance / loo = 1: ValueError there)
        self.pareto_file = os.path.join(expt_dir, "pareto.txt")
        self.last_pareto = None

    # -- the front of the completed jobs ---------------------------------------------
    def _front(self, vals, ldurs):
        """(indices into the completed jobs, front (n, 2), (r1, r2)): automatic reference coordinates come from all completed
        jobs; with a given one, jobs that do not lie strictly inside it take no part."""
        auto = pareto.reference_point(vals, ldurs)
        ref = (auto[0] if self.ref1 is None else self.ref1, auto[1] if self.ref2 is None else self.ref2)
        inside = np.nonzero((vals < ref[0]) & (ldurs < ref[1]))[0]
        idx = inside[pareto.pareto_front(vals[inside], ldurs[inside])]
        return idx, np.stack((vals[idx], ldurs[idx]), axis=1).reshape(-1, 2), ref

    def _write_pareto(self, complete, vals, durations, idx, front, ref, hv):
        lines = ["# completed=%d front=%d ref=%.17g %.17g hypervolume=%.17g" % (vals.shape[0], idx.shape[0], ref[0], ref[1], hv)]
        for i in idx:
            lines.append("%d %.17g %.17g" % (int(complete[i]), vals[i], durations[i]))
        self.locker.lock_wait(self.pareto_file)
        try:
            fh = tempfile.NamedTemporaryFile(mode="w", delete=False, dir=os.path.dirname(os.path.abspath(self.pareto_file)))
            try:
                try:
                    fh.write("\n".join(lines) + "\n")
                finally:
                    fh.close()
                os.rename(fh.name, self.pareto_file)
            except Exception:
                if os.path.exists(fh.name):
                    os.unlink(fh.name)
                raise
        finally:
            self.locker.unlock(self.pareto_file)

    # -- the hot path ------------------------------------------------------------------
    def _believed(self, eng, comp, pend, vals, ldurs, rows, trows, front, ref):
        """The believer rule: np.mean over the draws of both GPs' func_m at the pending rows, from a small EHVI pass that scores
        those rows as candidates."""
        from ..engine import ACQ_EHVI
        H = rows.shape[0]
        eng.set_observations(comp, vals)
        eng.set_candidates(pend)
        eng.set_hypers(rows)
        eng.set_time_model(ldurs, trows)
        eng.set_acquisition(ACQ_EHVI, 0.0)
        eng.set_pareto_front(front, ref)
        eng.ei_step()
        m1 = np.array([eng.get_moments(d)[0] for d in range(H)])
        m2 = np.array([eng.get_moments(H + d)[0] for d in range(H)])
        return np.mean(m1, axis=0), np.mean(m2, axis=0)

    def ehvi_over_hypers_gpu(self, comp, pend, cand, vals, ldurs, front, ref):
        """(index of the grid's argmax, mean EHVI over the draws (M,))."""
        from ..engine import ACQ_EHVI
        rows, trows = self._paired_samples()
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        trows = np.ascontiguousarray(trows, dtype=np.float64)
        eng = self.engine()
        self._lp_key = None
        self._resident_plain = False
        if pend.shape[0] > 0:
            b1, b2 = self._believed(eng, comp, pend, vals, ldurs, rows, trows, front, ref)
            comp = np.concatenate((comp, pend))
            vals = np.concatenate((vals, b1))
            ldurs = np.concatenate((ldurs, b2))
        eng.set_acquisition(ACQ_EHVI, 0.0)
        eng.set_pareto_front(front, ref)
        idx, _, mean, _ = eng.ei_per_sec_grid(comp, vals, ldurs, cand, rows, trows, want_mean=True, want_draws=False)
        warning = eng.last_warning()
        if warning:
            log("libspx " + warning)
        return idx, mean

    # -- plugin entry ------------------------------------------------------------------
    def next(self, grid, values, durations, candidates, pending, complete):
        if complete.shape[0] < 2:
            return int(candidates[0])
        durations = np.asarray(durations, dtype=np.float64)
        done = durations[complete]
        if not np.all(np.isfinite(done)) or np.any(done <= 0):
            raise ValueError("GPParetoChooser: the duration of every completed job must be positive and finite (the second "
                             "objective is its logarithm)")
        if self.D == -1:
            self._real_init(np.asarray(grid).shape[1], np.asarray(values)[complete], done)
        comp, cand, pend, vals = self._split(grid, values, candidates, pending, complete)
        ldurs = np.log(done).reshape(-1)
        # GPEIperSecChooser's own first steps, through its own code: the ten points it sprays around the incumbent for its
        # refinement (unused here: this chooser stays on the grid) and the sampling of both GPs
        self._spray(comp, vals)
        self._sample_call(comp, vals, ldurs)

        idx, front, ref = self._front(vals, ldurs)
        hv = pareto.dominated_hypervolume(front, ref)
        best, _ = self.ehvi_over_hypers_gpu(comp, pend, cand, vals, ldurs, front, ref)
        self.last_pareto = {"front_index": np.asarray(complete)[idx].astype(np.int64), "front": front, "ref": ref,
                            "hypervolume": hv}
        self._write_pareto(np.asarray(complete), vals, done, idx, front, ref, hv)
        log("front: %d of %d completed jobs, hypervolume %.6g" % (idx.shape[0], vals.shape[0], hv))
        return int(candidates[best])
