"""What the main-effects report costs (include/spx.h: spx_main_effects), one JSON line per measurement:

    python scripts/time_main_effects.py [--parent-lib PATH] [--shapes c2,c3]

Two forms of the same computation at bench.py's C2 and C3 shapes with T = 16 levels and Q = 256 base points:
    (a) device   spx_main_effects: base + levels uploaded, the rows formed and the means reduced on the device;
    (b) host     the host-orchestrated form through the entry points that existed before it: the host-built rows uploaded
                 (spx_set_candidates), the pass with the moments kept, spx_get_moments per draw, np.mean over each block --
                 on the library named by --parent-lib (a build of the parent commit) when given, else on this tree's own;
and, to place the two new kernels inside (a):
    (c) pass     spx_ei_run(SPX_FLAG_KEEP_MOMENTS) alone over the same rows already resident (no upload, no download).
(a) - (c) is everything (a) adds to the pass: k_effects_rows, k_effects_mean, the upload of (Q D + T) doubles, the download
of H (D T + Q) doubles and two host synchronisations -- an UPPER bound on the two kernels, reported beside the time their
byte counts take at the HBM bandwidth a copy reaches on this device (6.29 TB/s).  The library's streams are its own, so
events recorded by this script cannot bracket kernels inside a library call; the bound is what can be had without a timing
stage inside the library.

Every step is timed with the host clock around calls that end synchronised; the figure is the median over --steps after
--warmup.  The forms of a shape are interleaved round by round, so that a drift of the box hits them alike.  The results of
(a) and (b) are compared bit for bit once per shape.  The script ends itself after --timeout seconds (exit status 124) and
stops at the first error: nothing is tried twice."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spearmint_amd import engine as spx  # noqa: E402
from spearmint_amd.synthetic import synthetic_problem  # noqa: E402

SHAPES = {"c2": dict(N=256, D=8, H=10), "c3": dict(N=2048, D=32, H=20)}     # bench.py WORKLOADS
HBM_COPY_BYTES_PER_S = 6.29e12


def structured_rows(base, levels):
    Q, D = base.shape
    T = levels.shape[0]
    rows = np.empty((D * T + 1, Q, D))
    rows[:] = base[None, :, :]
    for j in range(D):
        rows[j * T:(j + 1) * T, :, j] = levels[:, None]
    return rows.reshape(-1, D)


def host_form(eng, rows, H, D, T, Q):
    eng.set_candidates(rows)
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    fm = np.array([eng.get_moments(d)[0] for d in range(H)])
    return np.mean(fm[:, :D * T * Q].reshape(H, D, T, Q), axis=-1), fm[:, D * T * Q:]


def time_shape(name, T, Q, steps, warmup, rounds, parent_lib):
    s = SHAPES[name]
    N, D, H = s["N"], s["D"], s["H"]
    comp, base, vals, hypers = synthetic_problem(N, Q, D, H, 1234, near=0)
    levels = (np.arange(T) + 0.5) / T
    t0 = time.perf_counter()
    rows = structured_rows(base, levels)
    build_ms = 1e3 * (time.perf_counter() - t0)
    dev = spx.Engine(0)
    if parent_lib:       # (a library from before this entry point: bound without it)
        full = spx.ABI
        spx.ABI = dict((k, v) for k, v in full.items() if k != "spx_main_effects")
        try:
            host = spx.Engine(0, lib=parent_lib)
        finally:
            spx.ABI = full
    else:
        host = spx.Engine(0)
    for e in (dev, host):
        e.set_observations(comp, vals)
        e.set_hypers(hypers)
        e.factor()
    ms = {"device": [], "host": [], "pass": []}
    got = want = None
    for rnd in range(rounds):
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            got = dev.main_effects(base, levels)
            if i >= warmup:
                ms["device"].append(1e3 * (time.perf_counter() - t0))
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            want = host_form(host, rows, H, D, T, Q)
            if i >= warmup:
                ms["host"].append(1e3 * (time.perf_counter() - t0))
        dev.set_candidates(rows)
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            dev.ei_run(spx.FLAG_KEEP_MOMENTS)
            if i >= warmup:
                ms["pass"].append(1e3 * (time.perf_counter() - t0))
    same = bool(np.array_equal(got["curves"], want[0]) and np.array_equal(got["base_mean"], want[1]))
    n_rows = rows.shape[0]
    common = {"what": "main_effects", "shape": name, "N": N, "D": D, "H": H, "T": T, "Q": Q, "rows": n_rows}
    for form in ("device", "host", "pass"):
        rec = dict(common, form=form, steps=len(ms[form]), median_ms=float(np.median(ms[form])), min_ms=float(np.min(ms[form])),
                   max_ms=float(np.max(ms[form])))
        if form == "host":
            rec.update(library=("parent build" if parent_lib else "this tree"), rows_built_on_host_ms=build_ms, rows_upload_bytes=rows.nbytes,
                       means_download_bytes=H * n_rows * 8)
        if form == "device":
            rec.update(passes=dev.stat("last_effects_passes"), same_bits_as_host_form=same)
        print(json.dumps(rec))
    a, c = float(np.median(ms["device"])), float(np.median(ms["pass"]))
    rows_bytes = n_rows * D * 8                                   # k_effects_rows: a pure write stream
    mean_bytes = H * n_rows * 8 + H * (D * T + Q) * 8             # k_effects_mean: the kept means in, curves + base_mean out
    print(json.dumps(dict(common, form="kernels", device_minus_pass_ms=a - c, share_of_device_upper_bound=(a - c) / a,
                          k_effects_rows_bytes=rows_bytes, k_effects_mean_bytes=mean_bytes,
                          rows_at_hbm_copy_rate_ms=1e3 * rows_bytes / HBM_COPY_BYTES_PER_S,
                          mean_at_hbm_copy_rate_ms=1e3 * mean_bytes / HBM_COPY_BYTES_PER_S)))
    sys.stdout.flush()
    dev.close()
    host.close()
    if not same:
        sys.stderr.write("time_main_effects.py: the two forms differ at %s\n" % name)
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libspx.so of the parent commit's build, for form (b)")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()

    def too_long(*_):
        sys.stderr.write("time_main_effects.py: --timeout %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(a.timeout)
    for name in a.shapes.split(","):
        time_shape(name, a.levels, a.points, a.steps, a.warmup, a.rounds, a.parent_lib)


if __name__ == "__main__":
    main()
