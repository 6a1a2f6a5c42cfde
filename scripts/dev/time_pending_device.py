"""Dev: one pending pass (factor -> fantasies -> ei_run) and a whole pending GPEIOptChooser.next() with the fantasies
formed by the library (gpu_fantasies=1), by the host (gpu_fantasies=0) and, given --parent-lib, by the host on a libspx
built from the parent commit (the parent's LIBRARY under this tree's Python: the host path's Python code is the parent's,
unchanged, so what differs is the library alone; the two symbols the parent lacks are left out of the binding while it
loads) -- five alternating runs each, medians and spreads as JSON.
    python scripts/dev/time_pending_device.py [--parent-lib PATH] [--out profiles/pending_device_fantasies.json] [--runs 5]"""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import numpy.random as npr
from spearmint_amd import hostgp
from spearmint_amd.chooser import GPEIOptChooser
from spearmint_amd.engine import Engine
from spearmint_amd.synthetic import synthetic_problem

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--sizes", default="small,c3")
args = ap.parse_args()
SIZES = {"small": (256, 20000, 6, 10, 4, 100), "c3": (2048, 200000, 32, 20, 4, 100)}     # N, M, D, H, P, S
if args.parent_lib:       # the parent's library has no spx_draw_fantasies: bind it without the two new symbols
    from spearmint_amd import engine as _engine
    _load, _abi = _engine.load_library, dict(_engine.ABI)

    def _load_either(path=None):
        if path != args.parent_lib:
            return _load(path)
        try:
            for k in ("spx_draw_fantasies", "spx_get_pending_fantasies"):
                _engine.ABI.pop(k, None)
            return _load(path)
        finally:
            _engine.ABI.update(_abi)
    _engine.load_library = _load_either
modes = [("device", None, 1), ("host", None, 0)] + ([("parent", args.parent_lib, 0)] if args.parent_lib else [])


def one_pass(eng, device, comp, cand, vals, hyp, pend, randn):
    N, P = comp.shape[0], pend.shape[0]
    t0 = time.perf_counter()
    eng.set_observations(np.concatenate((comp, pend)), np.concatenate((vals, np.zeros(P))))
    eng.set_candidates(cand)
    eng.set_hypers(hyp)
    eng.factor()
    t1 = time.perf_counter()
    if device:
        eng.draw_fantasies(np.stack(randn), P)
    else:
        fant, bests = hostgp.fantasies_from_engine(eng, vals, hyp, N, P, randn[0].shape[1], randn, per_draw=True)
        eng.set_fantasies(fant, bests)
    t2 = time.perf_counter()
    eng.ei_run()
    eng.best()
    eng.ei_mean()
    t3 = time.perf_counter()
    return {"total": t3 - t0, "fantasies": t2 - t1}


def summary(xs):
    xs = sorted(xs)
    return {"median_ms": 1e3 * xs[len(xs) // 2], "min_ms": 1e3 * xs[0], "max_ms": 1e3 * xs[-1], "runs_ms": [1e3 * x for x in xs]}


out = {"runs": args.runs, "sizes": {}}
for name in args.sizes.split(","):
    N, M, D, H, P, S = SIZES[name]
    comp, cand, vals, hyp = synthetic_problem(N, M, D, H, 31)
    rs = np.random.RandomState(2)
    pend = rs.rand(P, D)
    randn = [rs.randn(P, S) for _ in range(H)]
    engines = {m: Engine(0, lib) for m, lib, _ in modes}
    t = {m: {"total": [], "fantasies": []} for m, _, _ in modes}
    for rep in range(args.runs + 1):                       # (the first round warms every handle up)
        for m, _, dev in modes:
            r = one_pass(engines[m], dev, comp, cand, vals, hyp, pend, randn)
            if rep:
                for k in r:
                    t[m][k].append(r[k])
    for e in engines.values():
        e.close()
    rec = {"N": N, "M": M, "D": D, "H": H, "P": P, "S": S,
           "pass": {m: {k: summary(v) for k, v in t[m].items()} for m in t}}
    # a whole next(): N complete, P pending, M candidates of one grid
    grid = np.concatenate((comp, pend, cand))
    values = np.concatenate((vals, np.zeros(P + M)))
    complete, pending, candidates = np.arange(N), np.arange(N, N + P), np.arange(N + P, N + P + M)
    tn = {m: [] for m, _, _ in modes}
    jobs = {}
    for rep in range(args.runs + 1):
        for m, lib, dev in modes:
            d = tempfile.mkdtemp()
            ch = GPEIOptChooser.init(d, "mcmc_iters=%d,burnin=2,grid_subset=20,pending_samples=%d,use_multiprocessing=0,gpu_fantasies=%d%s"
                                     % (H, S, dev, (",lib=" + lib) if lib else ""))
            npr.seed(7)
            t0 = time.perf_counter()
            job = ch.next(grid, values, np.ones(grid.shape[0]), candidates, pending, complete)
            dt = time.perf_counter() - t0
            ch.engine().close()
            if rep:
                tn[m].append(dt)
            jobs[m] = job[0] if isinstance(job, tuple) else job
    rec["next"] = {m: summary(v) for m, v in tn.items()}
    rec["next_job"] = {m: int(v) for m, v in jobs.items()}
    out["sizes"][name] = rec
    print(name, json.dumps(rec["pass"]), json.dumps(rec["next"]), rec["next_job"], flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
