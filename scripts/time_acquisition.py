"""What the acquisitions beside EI cost (include/spx.h: spx_set_acquisition), one JSON line per measurement:

    python scripts/time_acquisition.py                 an EI, a PI and an LCB pass (spx_ei_step) at bench.py's C2 and C3 shapes
    python scripts/time_acquisition.py --next          GPEIOptChooser.next() at N = 256 / 20 000 candidates, recommend=0 and 1

Every step is timed with the host clock around a call that ends synchronised; the figure is the median over --steps after
--warmup.  The three acquisitions of a shape are interleaved round by round, so that a drift of the box hits them alike.  The
script ends itself after --timeout seconds (exit status 124) and stops at the first error: nothing is tried twice."""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spearmint_amd import engine as spx  # noqa: E402
from spearmint_amd.synthetic import synthetic_problem  # noqa: E402

SHAPES = {"c2": dict(N=256, M=20000, D=8, H=10), "c3": dict(N=2048, M=200000, D=32, H=20)}     # bench.py WORKLOADS
ACQS = (("EI", spx.ACQ_EI, 0.0), ("PI", spx.ACQ_PI, 0.01), ("LCB", spx.ACQ_LCB, 2.0))


def time_passes(name, steps, warmup, rounds):
    s = SHAPES[name]
    comp, cand, vals, hypers = synthetic_problem(s["N"], s["M"], s["D"], s["H"], 1234)
    eng = spx.Engine(0)
    eng.set_observations(comp, vals)
    eng.set_candidates(cand)
    eng.set_hypers(hypers)
    ms = dict((a[0], []) for a in ACQS)
    for rnd in range(rounds):
        for label, kind, par in ACQS:
            eng.set_acquisition(kind, par)
            for i in range(warmup + steps):
                t0 = time.perf_counter()
                eng.ei_step(0)
                dt = time.perf_counter() - t0
                if i >= warmup:
                    ms[label].append(1e3 * dt)
    for label, kind, par in ACQS:
        eng.set_acquisition(kind, par)
        eng.ei_step(0)
        print(json.dumps({"what": "pass", "shape": name, "acq": label, "par": par, "steps": len(ms[label]),
                          "median_ms": float(np.median(ms[label])), "min_ms": float(np.min(ms[label])),
                          "max_ms": float(np.max(ms[label])), "fused": eng.stat("last_step_fused"), "best": eng.best()[0]}))
        sys.stdout.flush()
    eng.close()


def time_next(calls):
    import numpy.random as npr
    from spearmint_amd import helpers
    import spearmint_amd.chooser._base as b
    import spearmint_amd.chooser.GPEIOptChooser as o
    from spearmint_amd import refine
    helpers.log = b.log = o.log = refine.log = lambda *a: None
    N, M, D = 256, 20000, 8
    comp, cand, vals, _ = synthetic_problem(N, M, D, 1, 9)
    grid = np.vstack((comp, cand))
    values = np.concatenate((vals, np.full(M, np.nan)))
    args = (grid, values, np.ones(N + M), np.arange(N, N + M), np.array([], dtype=int), np.arange(N))
    out = {}
    for rnd in range(2):                    # (0, 1, 0, 1: interleaved)
        for rec in (0, 1):
            ch = o.init(tempfile.mkdtemp(), "mcmc_iters=10,burnin=10,use_multiprocessing=0,recommend=%d" % rec)
            for k in range(calls):
                npr.seed(3 + k)
                t0 = time.perf_counter()
                job = ch.next(*args)
                out.setdefault((rec, "first" if k == 0 else "warm"), []).append(1e3 * (time.perf_counter() - t0))
            if rec:
                last = dict(ch.last_recommendation, x=None)
            ch.engine().close()
    for (rec, which), v in sorted(out.items()):
        print(json.dumps({"what": "next", "N": N, "M": M, "D": D, "recommend": rec, "call": which, "calls": len(v),
                          "median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}))
    print(json.dumps({"what": "next", "last_recommendation": last, "last_job": job if isinstance(job, int) else int(job[0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--next", action="store_true")
    ap.add_argument("--calls", type=int, default=4, help="with --next: next() calls per chooser (the first one burns in)")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()

    def too_long(*_):
        sys.stderr.write("time_acquisition.py: --timeout %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(a.timeout)
    if a.next:
        time_next(a.calls)
    else:
        for name in a.shapes.split(","):
            time_passes(name, a.steps, a.warmup, a.rounds)


if __name__ == "__main__":
    main()
