"""What a Thompson-sampling call costs (include/spx.h: spx_thompson), one JSON line per measurement:

    python scripts/time_thompson.py --parent-lib PATH [--shapes c2,c3] [--features 256,1024,4096] [--paths 1,8] > profiles/ts_time.jsonl

Per shape (bench.py's C2 and C3), F and S, over one resident, factored problem:
    thompson      this tree, spx_thompson(F, S) from fixed base randoms (the host's share -- the frequencies, the upload, the
                  H x S results coming home -- is inside the figure);
    fant_parent   the library named by --parent-lib (a build of the parent commit): spx_ei_run over S resident fantasies with the
                  same H -- the floor of the route: the same K(X*,X), the same predict GEMM with S right-hand sides.
Every call ends synchronised and is timed with the host clock; the figure is the median over --steps x --rounds (5 x 3 = 15)
after --warmup, the two forms interleaved round by round.  Then, with option "timing" = 1, the HIP-event time of the stages
"ts_prior" and "ts_finish".  The line says what the call adds to the floor, how that compares with the ts_prior stage, and how
the stage compares with k_ts_prior's FMA-unit bound (csrc/ts_kernels.hip):  M H F ceil(S / 16) (Dp + 32) / 16 cycles of a SIMD
over 1024 SIMDs at the device's clock.
--chooser: a warm GPEIChooser.next() with acq=TS against acq=EI at N = 256 completed jobs and 20 000 candidates (mcmc_iters=10).
Without a usable HIP device the script ends with status 2."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spearmint_amd import engine as spx  # noqa: E402
from spearmint_amd.synthetic import synthetic_problem  # noqa: E402

SHAPES = {"c2": dict(N=256, M=20000, D=8, H=10), "c3": dict(N=2048, M=200000, D=32, H=20),     # bench.py WORKLOADS
          "small": dict(N=30, M=1000, D=3, H=3)}
NEW_SYMBOLS = ("spx_thompson", "spx_get_thompson_path", "spx_get_thompson_prior")


def parent_engine(path):
    """An engine on a library from before spx_thompson: bound without the entry points it does not have."""
    full = spx.ABI
    spx.ABI = dict((k, v) for k, v in full.items() if k not in NEW_SYMBOLS)
    try:
        return spx.Engine(0, lib=path)
    finally:
        spx.ABI = full


def padded_dim(D):
    return 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else (D + 31) // 32 * 32


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def time_shape(name, features, paths, steps, warmup, rounds, parent_lib):
    s = SHAPES[name]
    N, M, D, H = s["N"], s["M"], s["D"], s["H"]
    comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 1234)
    ours = spx.Engine(0)
    parent = parent_engine(parent_lib) if parent_lib else None
    for e in (ours, parent):
        if e is not None:
            e.set_observations(comp, vals)
            e.set_candidates(cand)
            e.set_hypers(hypers)
            e.factor()
    clock_khz = ours.stat("clock_khz")
    for S in paths:
        if parent is not None:
            parent.set_fantasies(np.tile(vals[None, :, None], (H, 1, S)), np.full((H, S), vals.min()))
        for F in features:
            R = spx.thompson_randoms(np.random.RandomState(F + S), "Matern52", D, H, N, F, S)
            forms = {"thompson": lambda: ours.thompson(S=S, F=F, randoms=R)}
            if parent is not None:
                forms["fant_parent"] = parent.ei_run
            for fn in forms.values():
                for _ in range(warmup):
                    fn()
            ms = dict((k, []) for k in forms)
            for _ in range(rounds):
                for k, fn in forms.items():
                    for _ in range(steps):
                        ms[k].append(timed(fn))
            med = dict((k, float(np.median(v))) for k, v in ms.items())
            ours.set_option("timing", 1)
            ours.thompson(S=S, F=F, randoms=R)
            t = ours.timings()
            ours.set_option("timing", 0)
            prior_ms, finish_ms = t["ts_prior"][0], t["ts_finish"][0]
            bound_ms = 1e3 * M * H * F * ((S + 15) // 16) * (padded_dim(D) + 32) / 16.0 / (1024.0 * clock_khz * 1e3)
            line = dict(what="thompson", shape=name, N=N, M=M, D=D, H=H, F=F, S=S, steps=steps * rounds,
                        thompson_ms=med["thompson"], ts_prior_stage_ms=prior_ms, ts_finish_stage_ms=finish_ms,
                        ts_prior_launches=t["ts_prior"][1], ts_prior_bound_ms=bound_ms, stage_over_bound=prior_ms / bound_ms,
                        clock_khz=clock_khz)
            if parent is not None:
                added = med["thompson"] - med["fant_parent"]
                line.update(fant_parent_ms=med["fant_parent"], added_ms=added, added_over_prior_stage=added / prior_ms,
                            thompson_over_floor=med["thompson"] / med["fant_parent"])
            print(json.dumps(line), flush=True)
    ours.close()
    if parent is not None:
        parent.close()


def time_chooser(steps):
    from spearmint_amd.chooser import GPEIChooser
    N, M, D = 256, 20000, 8
    rs = np.random.RandomState(5)
    grid = rs.rand(N + M, D)
    values = np.full(N + M, np.nan)
    values[:N] = np.sum((grid[:N] - 0.4) ** 2, axis=1) + 0.05 * rs.randn(N)
    done, free, pend = np.arange(N), np.arange(N, N + M), np.arange(0)
    out = {}
    for acq in ("EI", "TS"):
        d = tempfile.mkdtemp(prefix="spx_time_ts_")
        ch = GPEIChooser.init(d, "mcmc_iters=10,acq=%s" % acq)
        np.random.seed(3)
        ch.next(grid, values, np.zeros(N + M), free, pend, done)          # warm: engine, buffers, sampler depth
        out[acq] = float(np.median([timed(lambda: ch.next(grid, values, np.zeros(N + M), free, pend, done)) for _ in range(steps)]))
        ch._eng.close()
    print(json.dumps(dict(what="chooser_next", N=N, M=M, D=D, mcmc_iters=10, steps=steps, next_ei_ms=out["EI"], next_ts_ms=out["TS"],
                          ts_over_ei=out["TS"] / out["EI"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--features", default="256,1024,4096")
    ap.add_argument("--paths", default="1,8")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chooser", action="store_true")
    a = ap.parse_args()
    if spx.device_count() < 1:
        sys.stderr.write("time_thompson: no HIP device\n")
        return 2
    for name in [v for v in a.shapes.split(",") if v]:
        time_shape(name, [int(v) for v in a.features.split(",")], [int(v) for v in a.paths.split(",")], a.steps, a.warmup,
                   a.rounds, a.parent_lib)
    if a.chooser:
        time_chooser(a.steps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
