"""What a knowledge-gradient step costs (include/spx.h: SPX_ACQ_KG), one JSON line per shape:

    python scripts/time_kg.py --parent-lib PATH [--shapes c2,c3] [--points 64] > profiles/kg_time.jsonl

Per shape (bench.py's C2 and C3) and A representer points, over one resident problem:
    kg_step       this tree, spx_ei_step under SPX_ACQ_KG (factorisation, k(X, A), Gamma_a, the S = A + 1 pass, the KG kernels);
    fant_parent   the library named by --parent-lib (a build of the parent commit): spx_ei_run over S = A + 1 resident
                  fantasies with the same H -- the floor of the route: the same K(X*,X), the same predict GEMM with S right-hand
                  sides (its factorisation is not in the figure; kg_run, this tree's spx_ei_run under KG, is the like-for-like).
Every call ends synchronised and is timed with the host clock; the figure is the median over --steps x --rounds (5 x 3 = 15)
after --warmup, the forms interleaved round by round.  Then, with option "timing" = 1, the HIP-event time of the stage "kg"
(k_kg_mu once, k_kg_lines + k_kg_value per work item) and the bound derived in csrc/kg_kernels.hip from the operations as
built: sweep 1 makes n^2 fp64 divisions per (draw, candidate), n = A + 1, about 16 fp64 instructions of 4 cycles per wave each:
M H n^2 cycles of a SIMD over 1024 SIMDs at the device's clock.
Without a usable HIP device the script ends with status 2."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spearmint_amd import engine as spx  # noqa: E402
from spearmint_amd.synthetic import synthetic_problem  # noqa: E402

SHAPES = {"c2": dict(N=256, M=20000, D=8, H=10), "c3": dict(N=2048, M=200000, D=32, H=20),     # bench.py WORKLOADS
          "small": dict(N=30, M=1000, D=3, H=3)}
NEW_SYMBOLS = ("spx_set_kg_points", "spx_get_kg_points", "spx_get_kg_lines")


def parent_engine(path):
    """An engine on a library from before SPX_ACQ_KG: bound without the entry points it does not have."""
    full = spx.ABI
    spx.ABI = dict((k, v) for k, v in full.items() if k not in NEW_SYMBOLS)
    try:
        return spx.Engine(0, lib=path)
    finally:
        spx.ABI = full


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def time_shape(name, A, steps, warmup, rounds, parent_lib):
    s = SHAPES[name]
    N, M, D, H = s["N"], s["M"], s["D"], s["H"]
    comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 1234)
    pts = cand[np.random.RandomState(7).permutation(M)[:A]]
    ours = spx.Engine(0)
    parent = parent_engine(parent_lib) if parent_lib else None
    for e in (ours, parent):
        if e is not None:
            e.set_observations(comp, vals)
            e.set_candidates(cand)
            e.set_hypers(hypers)
            e.factor()
    ours.set_kg_points(pts)
    ours.set_acquisition("KG")
    clock_khz = ours.stat("clock_khz")
    forms = {"kg_step": ours.ei_step, "kg_run": ours.ei_run}
    if parent is not None:
        parent.set_fantasies(np.tile(vals[None, :, None], (H, 1, A + 1)), np.full((H, A + 1), vals.min()))
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
    ours.ei_step()
    t = ours.timings()
    ours.set_option("timing", 0)
    n = A + 1
    bound_ms = 1e3 * M * H * float(n) * n / (1024.0 * clock_khz * 1e3)
    line = dict(what="kg", shape=name, N=N, M=M, D=D, H=H, A=A, steps=steps * rounds, kg_step_ms=med["kg_step"], kg_run_ms=med["kg_run"],
                kg_stage_ms=t["kg"][0], kg_stage_launches=t["kg"][1], kg_kernel_bound_ms=bound_ms, stage_over_bound=t["kg"][0] / bound_ms,
                clock_khz=clock_khz)
    if parent is not None:
        line.update(fant_parent_ms=med["fant_parent"], run_over_floor=med["kg_run"] / med["fant_parent"],
                    step_over_floor=med["kg_step"] / med["fant_parent"])
    print(json.dumps(line), flush=True)
    ours.close()
    if parent is not None:
        parent.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    bad = [v for v in a.shapes.split(",") if v and v not in SHAPES]
    if bad:
        sys.stderr.write("time_kg: no shape %s (known: %s)\n" % (", ".join(bad), ", ".join(sorted(SHAPES))))
        return 2
    if spx.device_count() < 1:
        sys.stderr.write("time_kg: no HIP device\n")
        return 2
    for name in [v for v in a.shapes.split(",") if v]:
        time_shape(name, a.points, a.steps, a.warmup, a.rounds, a.parent_lib)
    return 0


if __name__ == "__main__":
    sys.exit(main())
