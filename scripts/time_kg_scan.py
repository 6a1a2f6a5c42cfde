"""What option "kg_scan" costs (include/spx.h; csrc/kg_scan_kernels.hip), one JSON line per (shape, A):

    python scripts/time_kg_scan.py --parent-lib PATH [--cases c2:64,c3:64,c2:255,c2:1023] > profiles/kg_scan_time.jsonl

Per case (bench.py's C2 and C3 shapes, A representer points) over one resident problem, spx_ei_run under SPX_ACQ_KG with per-launch
timing: the HIP-event time of the stage "kg" (k_kg_mu once; per work item k_kg_lines and then k_kgs_order + k_kgs_value, or
k_kg_value) in three forms, interleaved call by call, the median over --calls (15) after --warmup:
    scan         this tree, option "kg_scan" = 1;
    pairs        this tree, option 0 (A <= 255);
    parent       the library named by --parent-lib (a build of the parent commit), its plain pass (A <= 255).
For A > 255 no parent figure exists; the line then carries fant_parent_ms, the parent's spx_ei_run over S = A + 1 resident
fantasies (host clock, synchronised): the floor of the route -- the same K(X*,X), the same predict GEMM over S right-hand sides --
beside scan_run_ms, this tree's whole spx_ei_run.
The bound is the one csrc/kg_scan_kernels.hip derives for E = 8 envelope lines: (3 n + E) divisions of 16 fp64 issue slots, E - 1
evaluations of f of 120, P / 2 log2 P (log2 P + 1) / 2 compare-exchanges of 2, 4 cycles per wave instruction of 64 lanes, over
1024 SIMDs at the device's clock.  Without a usable HIP device the script ends with status 2."""
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


def bound_ms(M, H, n, clock_khz, E=8):
    P = 2
    while P < n:
        P <<= 1
    lg = P.bit_length() - 1
    slots = (n + 2 * (n - E) + E) * 16 + (E - 1) * 120 + (P // 2) * (lg * (lg + 1) // 2) * 2
    return 1e3 * M * H * slots * 4.0 / 64.0 / (1024.0 * clock_khz * 1e3)


def kg_stage(e):
    """One spx_ei_run with per-launch timing: (ms of the stage "kg", ms of the call by the host clock)."""
    e.set_option("timing", 1)
    t0 = time.perf_counter()
    e.ei_run()
    ms = 1e3 * (time.perf_counter() - t0)
    t = e.timings()
    e.set_option("timing", 0)
    return t["kg"][0], ms


def time_case(name, A, calls, warmup, parent_lib):
    s = SHAPES[name]
    N, M, D, H = s["N"], s["M"], s["D"], s["H"]
    comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 1234)
    pts = cand[np.random.RandomState(7).permutation(M)[:A]]
    engines = {"scan": spx.Engine(0)}
    if A <= spx.KG_MAX_POINTS:
        engines["pairs"] = spx.Engine(0)
    parent = spx.Engine(0, lib=parent_lib) if parent_lib else None
    if parent is not None and A <= spx.KG_MAX_POINTS:
        engines["parent"] = parent
    for k, e in list(engines.items()) + ([("floor", parent)] if parent is not None and "parent" not in engines else []):
        e.set_observations(comp, vals)
        e.set_candidates(cand)
        e.set_hypers(hypers)
        e.factor()
        if k == "floor":
            e.set_fantasies(np.tile(vals[None, :, None], (H, 1, A + 1)), np.full((H, A + 1), vals.min()))
            continue
        if k == "scan":
            e.set_option("kg_scan", 1)
        e.set_kg_points(pts)
        e.set_acquisition("KG")
    clock_khz = engines["scan"].stat("clock_khz")
    for e in engines.values():
        for _ in range(warmup):
            e.ei_run()
    stage, run = dict((k, []) for k in engines), dict((k, []) for k in engines)
    floor = []
    for _ in range(calls):
        for k, e in engines.items():
            st, ms = kg_stage(e)
            stage[k].append(st)
            run[k].append(ms)
        if parent is not None and "parent" not in engines:
            t0 = time.perf_counter()
            parent.ei_run()
            floor.append(1e3 * (time.perf_counter() - t0))
    n = A + 1
    b = bound_ms(M, H, n, clock_khz)
    line = dict(what="kg_scan", shape=name, N=N, M=M, D=D, H=H, A=A, calls=calls, clock_khz=clock_khz, scan_bound_ms=b,
                pairs_bound_ms=1e3 * M * H * float(n) * n / (1024.0 * clock_khz * 1e3))
    for k in engines:
        line[k + "_stage_ms"] = float(np.median(stage[k]))
        line[k + "_run_ms"] = float(np.median(run[k]))
    line["scan_stage_over_bound"] = line["scan_stage_ms"] / b
    for k in ("pairs", "parent"):
        if k in engines:
            line["scan_over_" + k] = line["scan_stage_ms"] / line[k + "_stage_ms"]
    if floor:
        line["fant_parent_ms"] = float(np.median(floor))
        line["scan_run_over_floor"] = line["scan_run_ms"] / line["fant_parent_ms"]
    print(json.dumps(line), flush=True)
    for e in set(list(engines.values()) + ([parent] if parent is not None else [])):
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--cases", default="c2:64,c3:64,c2:255,c2:1023")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    cases = []
    for v in [v for v in a.cases.split(",") if v]:
        name, _, pts = v.partition(":")
        if name not in SHAPES or not pts.isdigit() or not 1 <= int(pts) <= spx.KG_SCAN_MAX_POINTS:
            sys.stderr.write("time_kg_scan: no case %s (shapes: %s; points 1 .. %d)\n" % (v, ", ".join(sorted(SHAPES)), spx.KG_SCAN_MAX_POINTS))
            return 2
        cases.append((name, int(pts)))
    if spx.device_count() < 1:
        sys.stderr.write("time_kg_scan: no HIP device\n")
        return 2
    for name, pts in cases:
        time_case(name, pts, a.calls, a.warmup, a.parent_lib)
    return 0


if __name__ == "__main__":
    sys.exit(main())
