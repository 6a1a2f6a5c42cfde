"""Dev: the refinement objective (spx_ei_grad_batch) per call -- plain, per second, with fantasies -- and a whole lbfgs_many;
the minimum over ROUNDS rounds of this process.  Another build of the library: SPX_LIB=/path/libspx.so.
   (lbfgs_many is timed warm, minimum of ROUNDS runs after one warm-up run; profiles/r04_refine_paths.log and the 118 -> 87 ms
   of DESIGN.md section 8 f3 were ONE cold run of it, so those figures are not comparable with this script's.)
   python scripts/dev/time_refine_paths.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from spearmint_amd import refine
from spearmint_amd.engine import Engine, FLAG_PER_SEC
from spearmint_amd.synthetic import synthetic_problem
ROUNDS = 3
def per_call(fn, reps=10):
    fn(); best = 1e30
    for _ in range(ROUNDS):
        t = time.time()
        for _ in range(reps): fn()
        best = min(best, (time.time() - t) / reps * 1e3)
    return best
eng = Engine(0)
for (N, D, H) in ((2048, 32, 20), (300, 6, 10), (40, 4, 10)):
    prob = synthetic_problem(N, 2000, D, H, 9, per_sec=True)
    comp, cand, vals, hyp, ld, th = prob
    rs = np.random.RandomState(0)
    out = []
    # plain
    eng.ei_grid(comp, vals, cand, hyp)
    for P in (1, 20):
        out.append("plain P=%d %.3f ms" % (P, per_call(lambda: eng.ei_grad_batch(cand[:P]))))
    out.append("lbfgs_many(20 points) %.1f ms" % per_call(lambda: refine.lbfgs_many(eng.ei_grad_batch, cand[:20], [(0, 1)] * D), reps=1))
    # per second
    eng.ei_per_sec_grid(comp, vals, ld, cand, hyp, th)
    out.append("per-sec P=20 %.3f ms" % per_call(lambda: eng.ei_grad_batch(cand[:20])))
    # fantasies
    S = 100
    eng.set_observations(comp, vals); eng.set_candidates(cand); eng.set_hypers(hyp); eng.factor()
    fant = rs.randn(H, N, S) * 0.1 + vals[None, :, None]
    eng.set_fantasies(fant, fant.min(axis=1)); eng.ei_run()
    t = time.time(); eng.ei_grad_batch(cand[:20]); first = (time.time() - t) * 1e3
    out.append("fantasies S=100 P=20 %.3f ms (first call %.1f ms)" % (per_call(lambda: eng.ei_grad_batch(cand[:20])), first))
    print("N=%d D=%d H=%d | " % (N, D, H) + "  ".join(out), flush=True)
