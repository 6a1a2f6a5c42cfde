"""What leave-one-out cross-validation costs (include/spx.h: spx_loo), one JSON line per measurement:

    python scripts/time_loo.py [--parent-lib PATH] [--shapes c2,c3]

Two routes to the same three arrays at bench.py's C2 and C3 shapes, over a resident factorisation:
    (a) device   spx_loo: the squared row norms of the resident L^-T reduced on the device, 3 H N doubles downloaded;
    (b) host     the only route there was before it: spx_get_factor(L, alpha) per draw -- one N x N download each --, the
                 host's triangular inversion, sum(inv(L)**2, 0) -- on the library named by --parent-lib (a build of the
                 parent commit) when given, else on this tree's own;
and, derived, not measured: the bytes of the live triangle of L^-T, H N (N + 1) / 2 x 8, at the bandwidth a copy reaches on
this device (6.29 TB/s) -- what k_loo_diag has to read.  The library's stream is its own, so events recorded by this script
cannot bracket the kernel inside the call; (a) is the whole call: launch, kernel, three small downloads, their host
synchronisations.

Every step is timed with the host clock around calls that end synchronised; the figure is the median over --steps x --rounds
after --warmup.  The two routes of a shape are interleaved round by round, so that a drift of the box hits them alike, and
their results are compared once per shape (rtol 1e-8: the host route's inverse is LAPACK's).  Each shape runs in a child
process of its own under --timeout seconds; the script stops at the first child that fails or runs out of time: nothing is
tried twice."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spearmint_amd import engine as spx  # noqa: E402
from spearmint_amd.synthetic import synthetic_problem  # noqa: E402

SHAPES = {"c2": dict(N=256, D=8, H=10), "c3": dict(N=2048, D=32, H=20)}     # bench.py WORKLOADS
HBM_COPY_BYTES_PER_S = 6.29e12


def host_route(eng, y, H, N):
    lm, lv, c = np.empty((H, N)), np.empty((H, N)), np.empty((H, N))
    eye = np.eye(N)
    for d in range(H):
        L, alpha = eng.get_factor(d, want_K=False)[1:]
        c[d] = np.sum(spla.solve_triangular(L, eye, lower=True, check_finite=False) ** 2, axis=0)
        lv[d] = 1.0 / c[d]
        lm[d] = y - alpha / c[d]
    return lm, lv, c


def time_shape(name, steps, warmup, rounds, parent_lib):
    s = SHAPES[name]
    N, D, H = s["N"], s["D"], s["H"]
    comp, _, vals, hypers = synthetic_problem(N, 1, D, H, 1234, near=0)
    dev = spx.Engine(0)
    if parent_lib:       # (a library from before this entry point: bound without it)
        full = spx.ABI
        spx.ABI = dict((k, v) for k, v in full.items() if k != "spx_loo")
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
    ms = {"device": [], "host": []}
    got = want = None
    for rnd in range(rounds):
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            got = dev.loo()
            if i >= warmup:
                ms["device"].append(1e3 * (time.perf_counter() - t0))
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            want = host_route(host, vals, H, N)
            if i >= warmup:
                ms["host"].append(1e3 * (time.perf_counter() - t0))
    same = bool(np.allclose(got["loo_mean"], want[0], rtol=1e-8, atol=1e-10 * np.abs(want[0]).max())
                and np.allclose(got["loo_var"], want[1], rtol=1e-8) and np.allclose(got["kinv_diag"], want[2], rtol=1e-8))
    tri_bytes = H * N * (N + 1) // 2 * 8
    common = {"what": "loo", "shape": name, "N": N, "D": D, "H": H}
    for form in ("device", "host"):
        rec = dict(common, form=form, measured=True, steps=len(ms[form]), median_ms=float(np.median(ms[form])),
                   min_ms=float(np.min(ms[form])), max_ms=float(np.max(ms[form])))
        if form == "host":
            rec.update(library=("parent build" if parent_lib else "this tree"), factor_download_bytes=H * N * N * 8)
        else:
            rec.update(download_bytes=3 * H * N * 8, agrees_with_host_route=same)
        print(json.dumps(rec))
    a = float(np.median(ms["device"]))
    bound_ms = 1e3 * tri_bytes / HBM_COPY_BYTES_PER_S
    print(json.dumps(dict(common, form="bound", measured=False, live_triangle_bytes=tri_bytes, copy_bytes_per_s=HBM_COPY_BYTES_PER_S,
                          triangle_at_copy_rate_ms=bound_ms, device_call_over_bound=a / bound_ms)))
    sys.stdout.flush()
    dev.close()
    host.close()
    if not same:
        sys.stderr.write("time_loo.py: the two routes differ at %s\n" % name)
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libspx.so of the parent commit's build, for route (b)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds each shape's child process may take")
    ap.add_argument("--child", action="store_true",
                    help="time the one named shape in this process (what the script starts per shape; the form to put under a profiler)")
    a = ap.parse_args()
    names = a.shapes.split(",")
    if a.child:
        time_shape(names[0], a.steps, a.warmup, a.rounds, a.parent_lib)
        return
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", name, "--steps", str(a.steps), "--warmup",
               str(a.warmup), "--rounds", str(a.rounds)] + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.stderr.write("time_loo.py: %s did not finish in %d s\n" % (name, a.timeout))
            sys.exit(124)
        if rc:
            sys.stderr.write("time_loo.py: %s ended with status %d\n" % (name, rc))
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
