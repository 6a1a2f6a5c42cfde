"""Time one constrained spx_ei_step (SPX_FLAG_CONSTRAINED) against the plain step at C2 and C3 sizes, and one whole
GPConstrainedEIChooser.next() at N = 256 / 20 000 candidates.  Reads nothing of the reference.

    python scripts/bench_constrained.py [--out profiles/constrained_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import numpy.random as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spearmint_amd.engine import FLAG_CONSTRAINED, Engine  # noqa: E402

SIZES = {"C2": dict(N=256, D=8, M=20000, H=10), "C3": dict(N=2048, D=32, M=200000, H=20)}


def step_times(eng, name, N, D, M, H, reps):
    rs = np.random.RandomState(1)
    comp = rs.rand(N, D)
    vals = np.sum((comp - 0.5) ** 2, axis=1)
    good = np.ones(N, dtype=bool)
    good[rs.choice(N, N // 6, replace=False)] = False
    cand = rs.rand(M, D)
    rows = np.column_stack((np.full(H, 0.5), np.full(H, 1e-2), np.ones(H), rs.uniform(0.8, 1.6, (H, D))))
    crows = np.column_stack((np.full(H, 1.5), np.full(H, 1e-3), np.ones(H), rs.uniform(0.8, 1.6, (H, D))))
    eng.set_observations(comp[good], vals[good])
    eng.set_candidates(cand)
    eng.set_hypers(rows)
    eng.set_constraint_model(comp, rs.randn(N), crows)
    out = {}
    for label, flags in (("plain", 0), ("constrained", FLAG_CONSTRAINED)):
        ts = []
        for r in range(reps + 2):
            eng.set_hypers(rows)      # a step re-factors, as in next()
            if flags:
                eng.set_constraint_model(comp, rs.randn(N), crows)
            t0 = time.perf_counter()
            eng.ei_step(flags)
            ts.append(time.perf_counter() - t0)
        out[label + "_ms"] = 1e3 * float(np.median(ts[2:]))
    out["ratio"] = out["constrained_ms"] / out["plain_ms"]
    out.update(dict(N=N, N_valid=int(good.sum()), D=D, M=M, H=H))
    return out


def next_time(burnin=10, mcmc_iters=10):
    from spearmint_amd.chooser.GPConstrainedEIChooser import GPConstrainedEIChooser
    rs = np.random.RandomState(3)
    N, D, M = 256, 8, 20000
    grid = rs.rand(N + M, D)
    values = np.concatenate((np.sum((grid[:N] - 0.4) ** 2, axis=1), np.zeros(M)))
    values[rs.choice(N, 30, replace=False)] = np.nan
    out = {}
    for label in ("cold", "warm"):
        d = tempfile.mkdtemp(prefix="spx_cbench_")
        c = GPConstrainedEIChooser(d, mcmc_iters=mcmc_iters, burnin=burnin, grid_subset=20)
        if label == "warm":
            npr.seed(2)
            c.next(grid, values, np.ones(N + M), np.arange(N, N + M), np.array([], dtype=int), np.arange(N))
        npr.seed(3)
        t0 = time.perf_counter()
        ret = c.next(grid, values, np.ones(N + M), np.arange(N, N + M), np.array([], dtype=int), np.arange(N))
        out[label + "_s"] = time.perf_counter() - t0
        out[label + "_phases_s"] = dict(c.last_phase_s)
        out["proposal_" + label] = ret[0] if isinstance(ret, tuple) else ret
    out["config"] = "N=256 (30 NaN), D=8, 20000 candidates, mcmc_iters=%d, burnin=%d, grid_subset=20" % (mcmc_iters, burnin)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrained_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps-only", action="store_true", help="the two step timings only (for a rocprofv3 run)")
    a = ap.parse_args()
    eng = Engine(0)
    res = {name: step_times(eng, name, reps=a.reps, **cfg) for name, cfg in SIZES.items()}
    eng.close()
    if a.steps_only:
        print(json.dumps(res))
        return
    res["next"] = next_time()
    res["next_defaults"] = next_time(burnin=100, mcmc_iters=20)     # the chooser's own defaults
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
