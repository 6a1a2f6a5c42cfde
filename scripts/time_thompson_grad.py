"""What an evaluation of a sample path off the grid costs (include/spx.h: spx_thompson_grad_batch), one JSON line per measurement:

    python scripts/time_thompson_grad.py --parent-lib PATH [--shapes c2,c3] [--chooser] > profiles/ts_grad_time.jsonl

Per shape (bench.py's C2 and C3) with F = 1024, S = 1, H = 1 -- what GPEIOptChooser runs -- and P = 20 points, over one resident,
factored problem that holds one sample path:
    grad_warm     this tree, spx_thompson_grad_batch with alpha resident;
    grad_first    the first call after a spx_thompson, which builds alpha = W^T Gamma (the spx_thompson in front of it is
                  outside the bracket);
    lcb_parent    the library named by --parent-lib (a build of the parent commit): spx_ei_grad_batch under LCB at the same N,
                  P and H = 1 -- the closest objective that library has; it streams W twice per call.
Every call ends synchronised and is timed with the host clock; the figure is the median over --steps x --rounds (5 x 3 = 15)
after --warmup, the forms interleaved round by round.  The line also carries the derived parts of a bound: the prior kernel's
FMA-unit time (csrc/ts_grad_kernels.hip: per tile of 16 points x 16 features 64 (Dp / 4 + 4 + 4 ceil(Dp / 16)) + 496 cycles of ONE
SIMD, a wave per 16 points, so ceil(P / 16) waves run side by side and the bound is one wave's walk over F features) and the
update kernel's read time (N Dp 8 bytes per 8 dimensions and point, against 5.3 TB/s when every point reads from memory).
--chooser: a warm GPEIOptChooser.next() with acq=TS, ts_refine=0 against ts_refine=1 at N = 256 completed jobs and 20 000
candidates (mcmc_iters=10).  Without a usable HIP device the script ends with status 2."""
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

SHAPES = {"c2": dict(N=256, M=20000, D=8), "c3": dict(N=2048, M=200000, D=32),     # bench.py WORKLOADS, one draw
          "small": dict(N=30, M=1000, D=3)}
NEW_SYMBOLS = ("spx_thompson_grad_batch",)
F, S, H, P = 1024, 1, 1, 20


def parent_engine(path):
    """An engine on a library from before spx_thompson_grad_batch: bound without the entry point it does not have."""
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


def time_shape(name, steps, warmup, rounds, parent_lib):
    s = SHAPES[name]
    N, M, D = s["N"], s["M"], s["D"]
    comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 1234)
    ours = spx.Engine(0)
    parent = parent_engine(parent_lib) if parent_lib else None
    for e in (ours, parent):
        if e is not None:
            e.set_observations(comp, vals)
            e.set_candidates(cand)
            e.set_hypers(hypers)
            e.factor()
    if parent is not None:
        parent.set_acquisition(spx.ACQ_LCB, 0.0)
    clock_khz = ours.stat("clock_khz")
    R = spx.thompson_randoms(np.random.RandomState(F + S), "Matern52", D, H, N, F, S)
    x = np.random.RandomState(2).rand(P, D)
    ours.thompson(S=S, F=F, randoms=R)

    def first():
        ours.thompson(S=S, F=F, randoms=R)           # (outside the bracket)
        return timed(lambda: ours.thompson_grad_batch(x))
    forms = {"grad_warm": lambda: timed(lambda: ours.thompson_grad_batch(x)), "grad_first": first}
    if parent is not None:
        forms["lcb_parent"] = lambda: timed(lambda: parent.ei_grad_batch(x))
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    ms = dict((k, []) for k in forms)
    for _ in range(rounds):
        for k, fn in forms.items():
            for _ in range(steps):
                ms[k].append(fn())
    med = dict((k, float(np.median(v))) for k, v in ms.items())
    Dp = padded_dim(D)
    tile_cycles = 64 * (Dp // 4 + 4 + 4 * ((Dp + 15) // 16)) + 4 * 4 * 31
    prior_bound_ms = 1e3 * (F // 16) * tile_cycles * ((Dp + 31) // 32) / (clock_khz * 1e3)
    update_read_ms = 1e3 * P * ((D + 7) // 8) * N * Dp * 8 / 5.3e12
    line = dict(what="thompson_grad", shape=name, N=N, M=M, D=D, H=H, F=F, S=S, P=P, steps=steps * rounds,
                grad_warm_ms=med["grad_warm"], grad_first_ms=med["grad_first"], prior_wave_fma_bound_ms=prior_bound_ms,
                update_read_bound_ms=update_read_ms, clock_khz=clock_khz)
    if parent is not None:
        line.update(lcb_parent_ms=med["lcb_parent"], lcb_over_grad_warm=med["lcb_parent"] / med["grad_warm"])
    print(json.dumps(line), flush=True)
    ours.close()
    if parent is not None:
        parent.close()


def time_chooser(steps):
    from spearmint_amd.chooser import GPEIOptChooser
    N, M, D = 256, 20000, 8
    rs = np.random.RandomState(5)
    grid = rs.rand(N + M, D)
    values = np.full(N + M, np.nan)
    values[:N] = np.sum((grid[:N] - 0.4) ** 2, axis=1) + 0.05 * rs.randn(N)
    done, free, pend = np.arange(N), np.arange(N, N + M), np.arange(0)
    out, refined = {}, 0
    for r in (0, 1):
        d = tempfile.mkdtemp(prefix="spx_time_tsg_")
        ch = GPEIOptChooser.init(d, "mcmc_iters=10,burnin=10,acq=TS,ts_refine=%d" % r)
        np.random.seed(3)
        ch.next(grid, values, np.zeros(N + M), free, pend, done)          # warm: engine, buffers, sampler depth, burn-in
        ts = []
        for _ in range(steps):
            ts.append(timed(lambda: ch.next(grid, values, np.zeros(N + M), free, pend, done)))
            refined += int(bool(r and ch.last_thompson["refined"]))
        out[r] = float(np.median(ts))
        ch._eng.close()
    print(json.dumps(dict(what="chooser_next", N=N, M=M, D=D, mcmc_iters=10, steps=steps, next_ts_ms=out[0], next_ts_refine_ms=out[1],
                          refine_adds_ms=out[1] - out[0], refined_calls=refined)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chooser", action="store_true")
    a = ap.parse_args()
    if spx.device_count() < 1:
        sys.stderr.write("time_thompson_grad: no HIP device\n")
        return 2
    for name in [v for v in a.shapes.split(",") if v]:
        time_shape(name, a.steps, a.warmup, a.rounds, a.parent_lib)
    if a.chooser:
        time_chooser(a.steps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
