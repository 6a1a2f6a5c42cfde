"""Dev tool: wall time per call of the calls where host work shows, with a variant build against the in-tree library
(as scripts/dev/lib_ab.py: alternating, each run in its own process).  The variant also runs against ITSELF under a second
label, which gives the spread of the machine on the day: a difference between builds means something only beyond it.
Call sets: `host` -- spx_gp_logprob at N = 64 x 1 draw and N = 256 x 10 draws, spx_ei_step at N = 128, 20 000 candidates,
10 draws; `staging` -- spx_ei_step at N = 256, 20 000 candidates, 10 draws through a 1 MiB K(X*,X) staging buffer (40 chunks
x 10 draws = 400 work items a pass: the event traffic of the hand-off dominates) under streams = 1, 2 and 3.
   python scripts/dev/plan_time.py _variants/libspx_parent.so [rounds] [host|staging|all]
(profiles/plan_refactor_time.log: the host set; profiles/staging_ring_time.log: all)"""
import json
import os
import subprocess
import sys
import time

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
# name: N, M, H, timed calls per loop, options (every call starts from DEFAULTS: none inherits the options of the call before)
DEFAULTS = {"kstar_budget_bytes": 512 << 20, "streams": 1}
SETS = {"host": {"logprob N=64 H=1": (64, 16, 1, 400, {}), "logprob N=256 H=10": (256, 16, 10, 300, {}),
                 "ei_step N=128 M=20000 H=10": (128, 20000, 10, 150, {})},
        "staging": {"ei_step N=256 M=20000 H=10 1MiB streams=%d" % ns: (256, 20000, 10, 12, {"kstar_budget_bytes": 1 << 20, "streams": ns})
                    for ns in (1, 2, 3)}}
SETS["all"] = dict(SETS["host"], **SETS["staging"])

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, root)
    import numpy as np
    from spearmint_amd.engine import Engine
    from spearmint_amd.synthetic import synthetic_problem
    eng = Engine(0, lib=None if sys.argv[2] == "-" else sys.argv[2])
    out = {}
    for name, (N, Mc, H, reps, opts) in SETS[sys.argv[3]].items():
        comp, cand, vals, hypers = synthetic_problem(N, Mc, 6, H, 5)
        for k, v in dict(DEFAULTS, **opts).items():
            eng.set_option(k, v)
        eng.set_observations(comp, vals)
        eng.set_candidates(cand)
        eng.set_hypers(hypers)
        if name.startswith("logprob"):
            def call():
                eng.set_hypers(hypers)
                return eng.gp_logprob()
        else:
            def call():
                eng.ei_step()
                return np.array(eng.best())
        for _ in range(30):
            chk = call()
        ts = []
        for rep in range(7):
            t = time.perf_counter()
            for _ in range(reps):
                call()
            ts.append((time.perf_counter() - t) / reps * 1e6)
        out[name] = (sorted(ts)[len(ts) // 2], min(ts), float(np.sum(chk)))
    print(json.dumps(out))
    sys.exit(0)

variant = sys.argv[1]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
which = sys.argv[3] if len(sys.argv) > 3 else "host"
CALLS = tuple(SETS[which])
runs = (("parent_a", variant), ("parent_b", variant), ("child", "-"))
res = {label: [] for label, _ in runs}
for rnd in range(rounds):
    for label, lib in runs:
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, which], stdout=subprocess.PIPE, timeout=240, check=True)
        res[label].append(json.loads(o.stdout.decode().strip().splitlines()[-1]))
        print("round %d %-8s %s" % (rnd, label, "  ".join("%s: %.2f us" % (c, res[label][-1][c][0]) for c in CALLS)), flush=True)


def med(v):
    return sorted(v)[len(v) // 2]


print("\nper call: median over %d rounds of each round's median of 7 timed loops [min .. max of the rounds' medians], microseconds" % rounds)
for c in CALLS:
    same = len(set(r[c][2] for v in res.values() for r in v)) == 1
    line = "%-28s" % c
    for label, _ in runs:
        v = [r[c][0] for r in res[label]]
        line += "  %s %.2f [%.2f .. %.2f]" % (label, med(v), min(v), max(v))
    pa, pb, ch = (med([r[c][0] for r in res[k]]) for k in ("parent_a", "parent_b", "child"))
    both = [r[c][0] for k in ("parent_a", "parent_b") for r in res[k]]
    line += "  | parent-parent %+.2f %%, child-parent %+.2f %%, child median %s the parents' range" % (
        100 * (pb / pa - 1), 100 * (ch / ((pa + pb) / 2) - 1), "inside" if min(both) <= ch <= max(both) else "OUTSIDE")
    print(line + ("" if same else "   <-- RESULTS DIFFER"))
