"""What the knowledge gradient over the fantasies of pending jobs costs (include/spx.h: option "kg_fantasies"), one JSON line per
measurement:

    python scripts/time_kg_pending.py --parent-lib PATH [--shapes c2,c3] [--fantasies 8,100] > profiles/kg_pending_time.jsonl

Per shape (bench.py's C2 and C3), A = --points (64) representer points and number of fantasies S, over the same resident
problem, factor and fantasies, the pass alone (spx_ei_run, which ends synchronised) in two forms:
    kg_fant     this tree, SPX_ACQ_KG with option kg_fantasies: the S + A column GEMM branch and the KG stages;
    ei_parent   the floor of the route: the EI pass over S + A fantasies -- the same GEMM width -- on the library named by
                --parent-lib (a build of the parent commit; without it, this tree's EI pass, labelled so).
The figure is the median of --calls (15) host-clock timings per form, the two forms interleaved call by call.  Then, on the KG
handle, option "timing" and three more passes: the HIP-event time of the stage "kg" (k_kgf_mu, k_kgf_lines and k_kgf_order of
every work item, k_kgf_value and k_kgf_mean behind the last chunk) beside the fp64-VALU bound derived in
csrc/kg_fant_kernels.hip, M H S / 9.9e9 s at n = 65.  A combination whose intercepts (H S Mp 8 bytes) exceed the library's 4 GiB
budget is reported as refused and the largest S that fits is timed in its place.  Each combination runs in a child process
under --timeout seconds; the script stops at the first child that fails: nothing is tried twice."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spearmint_amd import engine as spx  # noqa: E402
from spearmint_amd.synthetic import synthetic_problem  # noqa: E402

SHAPES = {"c2": dict(N=256, M=20000, D=8, H=10), "c3": dict(N=2048, M=200000, D=32, H=20)}     # bench.py WORKLOADS
NEW_SYMBOLS = ("spx_get_kg_fantasy_lines", "spx_get_kg_fantasy_var")
BUDGET = 4 << 30
BOUND_SCANS_PER_S = 9.9e9       # csrc/kg_fant_kernels.hip: 247 cycles of one SIMD per scan at n = 65 over 1024 SIMDs at 2.4 GHz


def parent_engine(path):
    """An engine on a library from before this feature: bound without the entry points it does not have."""
    full = spx.ABI
    spx.ABI = dict((k, v) for k, v in full.items() if k not in NEW_SYMBOLS)
    try:
        return spx.Engine(0, lib=path)
    finally:
        spx.ABI = full


def time_one(name, S, calls, parent_lib, A):
    s = SHAPES[name]
    N, M, D, H = s["N"], s["M"], s["D"], s["H"]
    common = {"what": "kg_pending", "shape": name, "N": N, "M": M, "D": D, "H": H, "S": S, "A": A}
    Mp = (M + 127) // 128 * 128
    if H * S * Mp * 8 > BUDGET:
        fit = BUDGET // (H * Mp * 8)
        print(json.dumps(dict(common, form="refused", measured=False, mean_bytes=H * S * Mp * 8, budget=BUDGET, largest_S=fit)))
        S = common["S"] = fit
    comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 1234)
    rs = np.random.RandomState(5)
    fant = vals[None, :, None] + 0.1 * rs.randn(H, N, S + A)     # (the parent's EI pass takes all S + A columns, KG the first S)
    bests = np.min(fant, axis=1)
    engines = {"kg_fant": spx.Engine(0), "ei_parent": parent_engine(parent_lib) if parent_lib else spx.Engine(0)}
    for e in engines.values():
        e.set_observations(comp, vals); e.set_candidates(cand); e.set_hypers(hypers)
    engines["kg_fant"].set_option("kg_fantasies", 1)
    engines["kg_fant"].set_kg_points(cand[rs.choice(M, A, replace=False)])
    engines["kg_fant"].set_acquisition(spx.ACQ_KG, 0.0)
    for form, e in engines.items():
        e.factor()
        ncol = S if form == "kg_fant" else S + A
        e.set_fantasies(np.ascontiguousarray(fant[:, :, :ncol]), np.ascontiguousarray(bests[:, :ncol]))
        e.ei_run(0)                       # warm-up: every buffer reserved
    ms = dict((form, []) for form in engines)
    for _ in range(calls):
        for form, e in engines.items():
            t0 = time.perf_counter()
            e.ei_run(0)
            ms[form].append(1e3 * (time.perf_counter() - t0))
    med = dict((form, float(np.median(v))) for form, v in ms.items())
    for form in engines:
        print(json.dumps(dict(common, form=form, measured=True, calls=calls, median_ms=med[form], min_ms=float(np.min(ms[form])),
                              max_ms=float(np.max(ms[form])),
                              library="parent build" if form == "ei_parent" and parent_lib else "this tree")))
    e = engines["kg_fant"]
    e.set_option("timing", 1)
    for _ in range(3):
        e.ei_run(0)
    stage_ms = e.timings()["kg"][0] / 3.0
    e.set_option("timing", 0)
    scans = float(M) * H * S
    bound_ms = 1e3 * scans / BOUND_SCANS_PER_S * (A + 1) / 65.0      # (the bound is linear in n)
    print(json.dumps(dict(common, form="kg_stage", measured=True, stage_ms_per_pass=stage_ms, scans=scans,
                          derived_bound_ms=bound_ms, stage_over_bound=stage_ms / bound_ms,
                          kg_fant_over_ei_parent=med["kg_fant"] / med["ei_parent"])))
    sys.stdout.flush()
    for e in engines.values():
        e.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--fantasies", default="8,100")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--points", type=int, default=64, help="A, the representer points")
    ap.add_argument("--parent-lib", default=None, help="libspx.so of the parent commit's build, for the form ei_parent")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each combination's child process may take")
    ap.add_argument("--child", action="store_true", help="time the one named combination in this process")
    a = ap.parse_args(argv)
    names, counts = a.shapes.split(","), [int(v) for v in a.fantasies.split(",")]
    for name in names:
        if name not in SHAPES:
            ap.error("no shape %r (allowed: %s)" % (name, ", ".join(sorted(SHAPES))))
    if a.child:
        try:
            time_one(names[0], counts[0], a.calls, a.parent_lib, a.points)
        except spx.SpxError as ex:
            sys.stderr.write("time_kg_pending.py: no usable HIP device or library call failed: %s\n" % ex)
            sys.exit(2)
        return
    for name in names:
        for S in counts:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", name, "--fantasies", str(S), "--calls",
                   str(a.calls), "--points", str(a.points)]
            cmd += ["--parent-lib", a.parent_lib] if a.parent_lib else []
            try:
                rc = subprocess.run(cmd, timeout=a.timeout).returncode
            except subprocess.TimeoutExpired:
                sys.stderr.write("time_kg_pending.py: %s S=%d did not finish in %d s\n" % (name, S, a.timeout))
                sys.exit(124)
            if rc:
                sys.stderr.write("time_kg_pending.py: %s S=%d ended with status %d\n" % (name, S, rc))
                sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
