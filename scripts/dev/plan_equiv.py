"""Dev tool: a record of what a library computes and reports over a lattice of shapes, forms and flags -- one line per case
with the SHA-256 of every output, every statistic and (option timing) the per-stage launch counts.  Two builds of the library
that queue the same launches give the same record line for line (profiles/plan_refactor_equiv.log: the build before the
planner of csrc/spx_plan.h against the build after it).
   python scripts/dev/plan_equiv.py LIB|- OUTFILE        (- : the in-tree library; each build in its own process)
   python scripts/dev/plan_equiv.py --digest OUTFILE     (the record condensed for a commit: per kind of call, N and H the number
                                                          of its lines and the SHA-256 over them)"""
import hashlib
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
from spearmint_amd.engine import FLAG_CONSTRAINED, FLAG_KEEP_MOMENTS, FLAG_PER_SEC, Engine   # noqa: E402
from spearmint_amd.synthetic import synthetic_problem                                         # noqa: E402
from tests.factor_helpers import FORMS, OPTION_DEFAULTS                                       # noqa: E402

NS, HS, D, M, S_FANT = (17, 64, 65, 130, 300), (1, 3, 32, 33), 3, 1000, 3
STATS = ("flow_fallbacks", "flow_rearms", "flow_enabled", "last_step_fused", "last_factor_flow", "last_factor_cov_in_flow",
         "last_logprob_one_launch", "last_step_skipped_padding", "last_corun_launches", "last_kstar_ring")
FLAGS = {"plain": FLAG_KEEP_MOMENTS, "per_sec": FLAG_PER_SEC | FLAG_KEEP_MOMENTS, "constrained": FLAG_CONSTRAINED | FLAG_KEEP_MOMENTS}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:10]


def tail(e, timing):
    """The statistics in the order of STATS and, with option timing, the launches per stage in the order of spx_timing_name."""
    s = "stats=" + ",".join("%d" % e.stat(k) for k in STATS)
    if timing:
        s += " launches=" + ",".join("%d" % v[1] for v in e.timings().values())
    return s


def main(lib, out_path):
    e = Engine(0, lib=None if lib == "-" else lib)
    e.set_option("kstar_budget_bytes", 1 << 20)           # several chunks and one draw per item at M = 1000
    out = open(out_path, "w")
    out.write("# stats: %s\n# launches: %s\n" % (",".join(STATS), ",".join(e.timings())))
    for N in NS:
        for H in HS:
            comp, cand, vals, hypers, log_durs, th = synthetic_problem(N, M, D, H, 100 * N + H, per_sec=True)
            rs = np.random.RandomState(N + H)
            crows = np.column_stack((rs.uniform(0.5, 3.0, H), np.full(H, 1e-3), rs.uniform(0.5, 2.0, H), rs.uniform(0.3, 1.5, (H, D))))
            ff = rs.randn(N) * 1.5
            fant = rs.randn(H, N, S_FANT)
            bests = np.min(fant, axis=1) - 0.1
            e.set_observations(comp, vals)
            e.set_candidates(cand)
            for timing in (0, 1):
                for form, opts in FORMS.items():
                    e.set_hypers(hypers)
                    for k, v in opts.items():
                        e.set_option(k, v)
                    e.set_option("timing", timing)
                    lp = e.gp_logprob()
                    out.write("lp N=%d H=%d %s timing=%d lp=%s %s\n" % (N, H, form, timing, sha(lp), tail(e, timing)))
                    for k in opts:
                        e.set_option(k, OPTION_DEFAULTS[k])
                for ei_flow in (0, 1):
                    for streams in (1, 2, 3):
                        for S in (0, S_FANT):
                            for kind, flags in FLAGS.items():
                                for step in ((0, 1) if S == 0 else (0,)):
                                    e.set_hypers(hypers)
                                    e.set_time_model(log_durs, th) if kind == "per_sec" else e.set_time_model(None, None)
                                    e.set_constraint_model(comp, ff, crows) if kind == "constrained" else e.set_constraint_model(None, None, None)
                                    e.set_option("ei_flow", ei_flow)
                                    e.set_option("streams", streams)
                                    e.set_option("timing", timing)
                                    if step:
                                        e.ei_step(flags)
                                    else:
                                        e.factor()
                                        if S:
                                            e.set_fantasies(fant, bests)
                                        e.ei_run(flags)
                                    stats = tail(e, timing)       # (before the read-backs: spx_get_factor's K launches nothing timed)
                                    idx, val = e.best()
                                    res = ["best=%d/%s" % (idx, sha(np.array(val))), "mean=" + sha(e.ei_mean()), "draws=" + sha(e.ei_draws())]
                                    for d in sorted(set((0, H - 1))):
                                        K, L, a = e.get_factor(d)
                                        res.append("K%d=%s L%d=%s alpha%d=%s" % (d, sha(K), d, sha(L), d, sha(a)))
                                        if S == 0:
                                            res.append("mom%d=%s" % (d, sha(*e.get_moments(d))))
                                        if kind == "per_sec":
                                            res.append("tmean%d=%s" % (d, sha(e.get_time_mean(d))))
                                        if kind == "constrained":
                                            res.append("cprob%d=%s" % (d, sha(e.get_constraint_prob(d))))
                                    rows, gam = e.get_factor_rows(0, max(N - 3, 0), min(3, N))
                                    res.append("rows=" + sha(rows, gam))
                                    out.write("ei N=%d H=%d ei_flow=%d streams=%d S=%d %s step=%d timing=%d %s %s\n"
                                              % (N, H, ei_flow, streams, S, kind, step, timing, " ".join(res), stats))
                                    e.set_fantasies(None, None)
                e.set_option("timing", 0)
                e.set_option("ei_flow", -1)
                e.set_option("streams", 1)
            out.flush()
            print("N=%d H=%d done" % (N, H), flush=True)
    out.close()
    e.close()


def digest(path):
    groups = {}
    for line in open(path):
        if line.startswith("#"):
            sys.stdout.write(line)
            continue
        kind, n, h = line.split()[:3]
        groups.setdefault((kind, n, h), []).append(line)
    for (kind, n, h), lines in groups.items():
        print("%s %s %s cases=%d sha256=%s" % (kind, n, h, len(lines), hashlib.sha256("".join(lines).encode()).hexdigest()[:32]))


if __name__ == "__main__":
    digest(sys.argv[2]) if sys.argv[1] == "--digest" else main(sys.argv[1], sys.argv[2])
