"""Shared by the CPU and GPU tests of the two-objective chooser (tests/test_pareto_host.py, tests/test_gpu_z_ehvi.py): the
oracle behind the Engine interface with SPX_ACQ_EHVI's semantics, a seeded two-objective toy problem driven call by call, and
csrc/ehvi_device.h compiled for the host.  The product never imports this file."""
import os
import subprocess
import tempfile

import numpy as np
import numpy.random as npr

from oracle import gp_ei_oracle as orc
from tests import ehvi_oracle as eo
from tests.helpers import OracleEngine, branin


class EhviOracleEngine(OracleEngine):
    """tests/helpers.OracleEngine + set_acquisition / set_pareto_front / get_moments: what Engine does under ACQ_EHVI, from
    tests/ehvi_oracle.py.  Every other acquisition goes through the parent's code untouched."""

    def __init__(self, covar="Matern52"):
        OracleEngine.__init__(self, covar)
        self.acq = (0, 0.0)
        self.front = None
        self._mom = None

    def set_acquisition(self, kind, par=0.0):
        self.acq = (int(kind), float(par))

    def get_acquisition(self):
        return self.acq

    def set_pareto_front(self, front, ref):
        self.front = None if front is None else (np.array(front, dtype=float).reshape(-1, 2), (float(ref[0]), float(ref[1])))

    def get_pareto_front(self):
        return self.front

    def _ehvi(self, comp, vals, second, cand, rows, trows):
        if self.front is None:
            raise ValueError("spx_ei_run: SPX_ACQ_EHVI needs a front")
        front, ref = self.front
        with orc.covar(self.covar):
            self._ei, self._mom = eo.over_hypers(comp, cand, vals, second, rows, trows, front[:, 0], front[:, 1], ref[0], ref[1],
                                                 want_moments=True)
        self._H = np.atleast_2d(rows).shape[0]

    def ei_step(self, flags=0):
        if self.acq[0] != eo.EHVI:
            return OracleEngine.ei_step(self, flags)
        if not getattr(self, "_time_set", False):
            raise ValueError("spx_ei_step: SPX_ACQ_EHVI needs the second objective's GP")
        self._ehvi(self.comp, self.vals, self.log_durs, self.cand, self.hypers, self.time_hypers)
        self.calls.append(("ehvi_step", self.cand.shape[0], self._H))

    def get_moments(self, draw):
        m = self._mom[draw % self._H]
        return (m[0], m[1]) if draw < self._H else (m[2], m[3])

    def ei_per_sec_grid(self, comp, vals, log_durs, cand, hypers, time_hypers, want_mean=True, want_draws=False, flags=0):
        if self.acq[0] != eo.EHVI:
            return OracleEngine.ei_per_sec_grid(self, comp, vals, log_durs, cand, hypers, time_hypers, want_mean, want_draws, flags)
        self.set_observations(comp, vals); self.set_candidates(cand); self.set_hypers(hypers)
        self.set_time_model(log_durs, time_hypers)
        self._ehvi(self.comp, self.vals, self.log_durs, self.cand, self.hypers, self.time_hypers)
        mean = np.mean(self._ei, axis=1)
        idx = int(np.argmax(mean))
        self.calls.append(("ehvi_grid", self.cand.shape[0], self._H, self.comp.shape[0]))
        return idx, float(mean[idx]), mean, (self._ei if want_draws else None)


def toy_duration(x):
    return 1.0 + 3.0 * x[..., 0] + np.sin(5.0 * x[..., 1]) ** 2


def pareto_sequence(make_chooser, make_engine, iters=6, seed=11, pending_at=(3,), n_pending=2, grid_points=40):
    """`iters` proposals of a fresh GPParetoChooser per call (restarted from its state pickle) on a seeded toy problem --
    value Branin, duration 1 + 3 x0 + sin^2(5 x1) --, each after npr.seed(seed + call); at the calls `pending_at` the
    n_pending lowest free grid rows are pending.  Returns [dict(job, state, last_pareto, text, pending, complete, cand)]."""
    grid = np.random.RandomState(3).rand(grid_points, 2)
    values = np.zeros(grid_points) + np.nan
    durations = np.zeros(grid_points) + np.nan
    done = np.zeros(grid_points, dtype=bool)
    for k in (0, 1, 2):
        values[k], durations[k], done[k] = branin(grid[k, 0], grid[k, 1]), toy_duration(grid[k]), True
    out = []
    for it in range(iters):
        ch = make_chooser()
        ch._eng = make_engine()
        npr.seed(seed + it)
        free = np.nonzero(~done)[0]
        pend = free[:n_pending] if it in pending_at else np.zeros(0, dtype=int)
        cand = np.array([i for i in free if i not in pend], dtype=int)
        complete = np.nonzero(done)[0]
        job = ch.next(grid, values, durations, cand, pend, complete)
        rec = {"job": int(job), "state": npr.get_state(), "last_pareto": ch.last_pareto, "text": open(ch.pareto_file).read(),
               "pending": pend, "complete": complete, "cand": cand, "rows": ch._paired_samples(), "engine": ch._eng,
               "grid": grid, "values": values.copy(), "durations": durations.copy()}
        out.append(rec)
        values[job], durations[job], done[job] = branin(grid[job, 0], grid[job, 1]), toy_duration(grid[job]), True
        if hasattr(ch._eng, "close"):
            ch._eng.close()
        ch._eng = None
    return out


def same_rng_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


_client = []


def device_header_on_host(edges, levels, m1, v1, m2, v2):
    """EHVI of every candidate from spearmint_amd/csrc/ehvi_device.h compiled for the host (tests/c/ehvi_client.cpp, no
    contraction, with the address and undefined-behaviour sanitizers), or None without a host C++ compiler."""
    from tests import plan_helpers as ph
    if not _client:
        cxx = ph.compiler()
        exe = None
        if cxx:
            exe = os.path.join(tempfile.mkdtemp(prefix="spx_ehvi_client_"), "ehvi_client")
            subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                                   os.path.join(ph.ROOT, "tests", "c", "ehvi_client.cpp")])
        _client.append(exe)
    if _client[0] is None:
        return None
    nums = [float(len(edges)), float(len(m1))] + list(edges) + list(levels)
    for row in zip(m1, v1, m2, v2):
        nums += list(row)
    text = "".join(float(x).hex() + "\n" for x in nums)
    out = subprocess.run([_client[0]], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split()
    return np.array([float.fromhex(v) for v in out])
