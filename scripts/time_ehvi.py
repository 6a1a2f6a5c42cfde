"""What an expected-hypervolume-improvement step costs (include/spx.h: SPX_ACQ_EHVI), one JSON line per measurement:

    python scripts/time_ehvi.py --parent-lib PATH [--shapes c2,c3] [--fronts 8,64] > profiles/ehvi_time.jsonl

Per shape (bench.py's C2 and C3) and per front size, forms of the same spx_ei_step over the same resident problem:
    ehvi            this tree, SPX_ACQ_EHVI against a front of n points (second objective: the per-second problem's durations);
    ei_keep         this tree, plain EI with SPX_FLAG_KEEP_MOMENTS;
    ei_keep_parent  the same on the library named by --parent-lib (a build of the parent commit);
    per_sec_parent  the parent's per-second step (SPX_FLAG_PER_SEC) with the same time model.
Every step is timed with the host clock around a call that ends synchronised; the figure is the median over --steps x --rounds
(5 x 3 = 15) after --warmup, the forms interleaved round by round so that a drift of the box hits them alike.  An EHVI step is
timed in two states: `ehvi`, with the internal handle holding the rows and candidates (only the hypers are set again before
each step, as a chooser's next draws are, so both GPs are factored again), and `ehvi_new_candidates`, where the candidates are
set again too and the internal handle takes its device-to-device copy.  Then, with option "timing" = 1, the HIP-event time of
the stage "ehvi" (k_ehvi alone).  The line "expected" puts the figures together: two kept-moments steps of the parent plus
the stage, beside the measured step.  Each shape runs in a child process under --timeout seconds; the script stops at the first
child that fails or runs out of time: nothing is tried twice.  Without a usable HIP device the child ends with status 2."""
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

SHAPES = {"c2": dict(N=256, M=20000, D=8, H=10), "c3": dict(N=2048, M=200000, D=32, H=20),     # bench.py WORKLOADS
          "small": dict(N=30, M=1000, D=3, H=3)}
NEW_SYMBOLS = ("spx_set_pareto_front", "spx_get_pareto_front")


def parent_engine(path):
    """An engine on a library from before SPX_ACQ_EHVI: bound without the entry points it does not have."""
    full = spx.ABI
    spx.ABI = dict((k, v) for k, v in full.items() if k not in NEW_SYMBOLS)
    try:
        return spx.Engine(0, lib=path)
    finally:
        spx.ABI = full


def a_front(n, vals, second):
    """n points through the observed range of both objectives, in the engine's order, and a reference point beyond them."""
    lo1, hi1, lo2, hi2 = float(np.min(vals)), float(np.max(vals)), float(np.min(second)), float(np.max(second))
    t = (np.arange(n) + 0.5) / max(n, 1)
    front = np.stack((lo1 + (hi1 - lo1) * t, hi2 - (hi2 - lo2) * np.sqrt(t)), axis=1)
    return front, (hi1 + 0.1 * (hi1 - lo1), hi2 + 0.1 * (hi2 - lo2))


def time_shape(name, fronts, steps, warmup, rounds, parent_lib):
    s = SHAPES[name]
    N, M, D, H = s["N"], s["M"], s["D"], s["H"]
    comp, cand, vals, hypers, second, th = synthetic_problem(N, M, D, H, 1234, per_sec=True)
    for n in fronts:
        front, ref = a_front(n, vals, second)
        engines = {"ehvi": spx.Engine(0), "ehvi_new_candidates": spx.Engine(0), "ei_keep": spx.Engine(0)}
        if parent_lib:
            engines["ei_keep_parent"] = parent_engine(parent_lib)
            engines["per_sec_parent"] = parent_engine(parent_lib)
        flags = {"ehvi": 0, "ehvi_new_candidates": 0, "ei_keep": spx.FLAG_KEEP_MOMENTS, "ei_keep_parent": spx.FLAG_KEEP_MOMENTS,
                 "per_sec_parent": spx.FLAG_PER_SEC}
        with_time = ("ehvi", "ehvi_new_candidates", "per_sec_parent")
        for form, e in engines.items():
            e.set_observations(comp, vals)
            e.set_candidates(cand)
            e.set_hypers(hypers)
            if form in with_time:
                e.set_time_model(second, th)
            if form.startswith("ehvi"):
                e.set_acquisition(spx.ACQ_EHVI, 0.0)
                e.set_pareto_front(front, ref)
        ms = dict((form, []) for form in engines)
        for rnd in range(rounds):
            for form, e in engines.items():
                for i in range(warmup + steps):
                    # outside the clock: new draws of both GPs, as every call of a chooser brings them (for the EHVI forms
                    # this is what makes the internal handle factor again); the second form also takes new candidates
                    e.set_hypers(hypers)
                    if form in with_time:
                        e.set_time_model(second, th)
                    if form == "ehvi_new_candidates":
                        e.set_candidates(cand)
                    t0 = time.perf_counter()
                    e.ei_step(flags[form])
                    if i >= warmup:
                        ms[form].append(1e3 * (time.perf_counter() - t0))
        H_ = hypers.shape[0]
        same_obj = all(np.array_equal(a, b) for a, b in zip(engines["ehvi"].get_moments(0), engines["ei_keep"].get_moments(0)))
        common = {"what": "ehvi", "shape": name, "N": N, "M": M, "D": D, "H": H_, "front": n}
        med = {}
        for form in engines:
            med[form] = float(np.median(ms[form]))
            print(json.dumps(dict(common, form=form, measured=True, steps=len(ms[form]), median_ms=med[form],
                                  min_ms=float(np.min(ms[form])), max_ms=float(np.max(ms[form])),
                                  library="parent build" if form.endswith("_parent") else "this tree")))
        e = engines["ehvi"]
        e.set_option("timing", 1)
        for _ in range(steps):
            e.set_hypers(hypers)
            e.set_time_model(second, th)
            e.ei_step(0)
        stage_ms, launches = e.timings()["ehvi"]
        e.set_option("timing", 0)
        per_pass = stage_ms / max(launches, 1)
        print(json.dumps(dict(common, form="ehvi_stage", measured=True, passes=launches, stage_ms_per_pass=per_pass,
                              g_evaluations=2.0 * M * H_ * (n + 1))))
        base = med.get("ei_keep_parent", med["ei_keep"])
        print(json.dumps(dict(common, form="expected", measured=False, two_kept_steps_plus_stage_ms=2.0 * base + per_pass,
                              ehvi_ms=med["ehvi"], ehvi_new_candidates_ms=med["ehvi_new_candidates"],
                              ehvi_over_expected=med["ehvi"] / (2.0 * base + per_pass),
                              ei_keep_over_parent=(med["ei_keep"] / med["ei_keep_parent"] if parent_lib else None),
                              ehvi_over_per_sec_parent=(med["ehvi"] / med["per_sec_parent"] if parent_lib else None),
                              objective_moments_equal_ei_keep=bool(same_obj))))
        sys.stdout.flush()
        for e in engines.values():
            e.close()
        if not same_obj:
            sys.stderr.write("time_ehvi.py: the EHVI pass's objective moments differ from the EI pass's at %s\n" % name)
            sys.exit(1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--fronts", default="8,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libspx.so of the parent commit's build, for the *_parent forms")
    ap.add_argument("--timeout", type=int, default=600, help="seconds each shape's child process may take")
    ap.add_argument("--child", action="store_true", help="time the one named shape in this process")
    a = ap.parse_args(argv)
    names = a.shapes.split(",")
    for name in names:
        if name not in SHAPES:
            ap.error("no shape %r (allowed: %s)" % (name, ", ".join(sorted(SHAPES))))
    try:
        fronts = [int(x) for x in a.fronts.split(",")]
    except ValueError:
        ap.error("--fronts takes integers separated by commas")
    if any(n < 0 or n > spx.MAX_FRONT for n in fronts):
        ap.error("--fronts: 0 .. %d points" % spx.MAX_FRONT)
    if a.child:
        try:
            time_shape(names[0], fronts, a.steps, a.warmup, a.rounds, a.parent_lib)
        except spx.SpxError as ex:
            sys.stderr.write("time_ehvi.py: no usable HIP device or library call failed: %s\n" % ex)
            sys.exit(2)
        return
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", name, "--fronts", a.fronts, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
        cmd += ["--parent-lib", a.parent_lib] if a.parent_lib else []
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.stderr.write("time_ehvi.py: %s did not finish in %d s\n" % (name, a.timeout))
            sys.exit(124)
        if rc:
            sys.stderr.write("time_ehvi.py: %s ended with status %d\n" % (name, rc))
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
