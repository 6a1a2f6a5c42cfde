"""What KG over pending fantasies costs in the wide form (include/spx.h: option "kg_fantasies" = 2), one JSON line per measurement:

    python scripts/time_kg_pending_scan.py --parent-lib PATH [--shapes c2,c3] [--fantasies 8,100] [--points 64,255,1023]
        > profiles/kg_pending_scan_time.jsonl

Per shape (bench.py's C2 and C3), S and A, over the same resident problem, factor and fantasies, the pass alone (spx_ei_run) as
    wide            this tree, option kg_fantasies = 2;
    narrow          this tree, option kg_fantasies = 1 (A <= 255);
    narrow_parent   the library named by --parent-lib, option kg_fantasies = 1 (A <= 255);
    ei_parent       that library's EI pass over S + A fantasies, the GEMM floor of the route (A > 255, where no narrow form exists).
Medians of --calls (15) host-clock timings, the forms interleaved call by call; then per KG form option "timing" and three more
passes: the HIP-event time of the stage "kg", for the wide form beside the fp64-VALU bound derived in
csrc/kg_fant_scan_kernels.hip, (n + 2 P + E) + 7.5 E cycles per scan at E = 8, P = n - 8.  Each combination runs in a child process
under --timeout seconds; the script stops at the first child that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_kg_pending import SHAPES, parent_engine, spx, synthetic_problem  # noqa: E402


def time_one(name, S, A, calls, parent_lib):
    s = SHAPES[name]
    N, M, D, H = s["N"], s["M"], s["D"], s["H"]
    common = {"what": "kg_pending_scan", "shape": name, "N": N, "M": M, "D": D, "H": H, "S": S, "A": A}
    comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 1234)
    rs = np.random.RandomState(5)
    fant = vals[None, :, None] + 0.1 * rs.randn(H, N, S + A)
    bests = np.min(fant, axis=1)
    pts = cand[rs.choice(M, A, replace=False)]
    engines = {"wide": (spx.Engine(0), 2)}
    if A <= 255:
        engines["narrow"] = (spx.Engine(0), 1)
        if parent_lib:
            engines["narrow_parent"] = (parent_engine(parent_lib), 1)
    elif parent_lib:
        engines["ei_parent"] = (parent_engine(parent_lib), 0)
    for form, (e, on) in engines.items():
        e.set_observations(comp, vals); e.set_candidates(cand); e.set_hypers(hypers)
        ncol = S
        if on:
            e.set_option("kg_scan", 1 if A > 255 else 0)
            e.set_option("kg_fantasies", on)
            e.set_kg_points(pts)
            e.set_acquisition(spx.ACQ_KG, 0.0)
        else:
            ncol = S + A
        e.factor()
        e.set_fantasies(np.ascontiguousarray(fant[:, :, :ncol]), np.ascontiguousarray(bests[:, :ncol]))
        e.ei_run(0)                       # warm-up: every buffer reserved
    ms = dict((form, []) for form in engines)
    for _ in range(calls):
        for form, (e, _) in engines.items():
            t0 = time.perf_counter()
            e.ei_run(0)
            ms[form].append(1e3 * (time.perf_counter() - t0))
    n, E = A + 1, 8
    bound_ms = 1e3 * float(M) * H * S * ((n + 2 * max(n - E, 0) + E) + 7.5 * E) / (1024 * 2.4e9)
    for form, (e, on) in engines.items():
        rec = dict(common, form=form, measured=True, calls=calls, median_ms=float(np.median(ms[form])), min_ms=float(np.min(ms[form])),
                   max_ms=float(np.max(ms[form])), library="this tree" if form in ("wide", "narrow") else "parent build")
        if on:
            e.set_option("timing", 1)
            for _ in range(3):
                e.ei_run(0)
            rec["kg_stage_ms_per_pass"] = e.timings()["kg"][0] / 3.0
            if form == "wide":
                rec.update(derived_bound_ms=bound_ms, stage_over_bound=rec["kg_stage_ms_per_pass"] / bound_ms)
        print(json.dumps(rec))
        e.close()
    sys.stdout.flush()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--fantasies", default="8,100")
    ap.add_argument("--points", default="64,255,1023", help="A, the representer points (c3: 64 only)")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--parent-lib", default=None, help="libspx.so of the parent commit's build")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each combination's child process may take")
    ap.add_argument("--child", action="store_true", help="time the one named combination in this process")
    a = ap.parse_args(argv)
    names, counts, points = a.shapes.split(","), [int(v) for v in a.fantasies.split(",")], [int(v) for v in a.points.split(",")]
    if a.child:
        time_one(names[0], counts[0], points[0], a.calls, a.parent_lib)
        return
    for name in names:
        for S in counts:
            for A in (points if name != "c3" else [64]):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", name, "--fantasies", str(S), "--points", str(A),
                       "--calls", str(a.calls)] + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
                try:
                    rc = subprocess.run(cmd, timeout=a.timeout).returncode
                except subprocess.TimeoutExpired:
                    sys.stderr.write("time_kg_pending_scan.py: %s S=%d A=%d did not finish in %d s\n" % (name, S, A, a.timeout))
                    sys.exit(124)
                if rc:
                    sys.stderr.write("time_kg_pending_scan.py: %s S=%d A=%d ended with status %d\n" % (name, S, A, rc))
                    sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
