"""Dev tool, the sibling of scripts/dev/plan_equiv.py for the EI pass's acquisitions: a record of what a library computes, reports
and refuses over every acquisition row (EI / PI / LCB, fantasies, MES, MES over fantasies, EHVI, Thompson sampling, the five KG
forms), spx_main_effects, and per-second / constrained / time-only EI -- one line per case with the SHA-256 of every output the
getters serve, every statistic and (option timing) the launches per stage; then the text of each refused combination.  Two
builds that queue the same launches give the same record line for line (profiles/pass_refactor_equiv.log: the build before
plan_ei decided the acquisition's branches and buffers against the build after).
   python scripts/dev/pass_equiv.py LIB|- OUTFILE        (- : the in-tree library; each build in its own process)
   python scripts/dev/pass_equiv.py --digest OUTFILE     (the record condensed for a commit)"""
import hashlib
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
from spearmint_amd.engine import FLAG_CONSTRAINED, FLAG_KEEP_MOMENTS, FLAG_PER_SEC, FLAG_TIME_ONLY, Engine   # noqa: E402
from spearmint_amd.synthetic import synthetic_problem                                                         # noqa: E402

NS, HS, D, M, S, A, K = (17, 128, 130, 300), (1, 3), 2, 1000, 3, 5, 4
STATS = ("last_kg_points", "last_kg_fantasies", "last_kg_scan", "last_kg_lines", "last_mes_samples", "last_mes_fantasies",
         "last_mes_grid", "last_ts_paths", "last_step_fused", "last_kstar_ring", "last_step_skipped_padding", "last_corun_launches",
         "last_factor_flow")
# row: (acquisition, its parameter, fantasies, options, flags)
ROWS = {"EI": ("EI", 0.0, 0, {}, 0), "PI": ("PI", 0.01, 0, {}, 0), "LCB": ("LCB", 2.0, 0, {}, 0), "EI-keep": ("EI", 0.0, 0, {}, FLAG_KEEP_MOMENTS),
        "EI-fant": ("EI", 0.0, S, {}, 0), "PI-fant": ("PI", 0.01, S, {}, 0),
        "MES": ("MES", K, 0, {}, 0), "MES-fant": ("MES", K, S, {"mes_fantasies": 1}, FLAG_KEEP_MOMENTS), "EHVI": ("EHVI", 0.0, 0, {}, 0),
        "KG-pairs": ("KG", 0.0, 0, {}, FLAG_KEEP_MOMENTS), "KG-scan": ("KG", 0.0, 0, {"kg_scan": 1}, 0),
        "KG-fant": ("KG", 0.0, S, {"kg_fantasies": 1}, FLAG_KEEP_MOMENTS), "KG-fant-wide": ("KG", 0.0, S, {"kg_fantasies": 2, "kg_scan": 1}, 0),
        "KG-fant-wide-noscan": ("KG", 0.0, S, {"kg_fantasies": 2}, FLAG_KEEP_MOMENTS),
        "per_sec": ("EI", 0.0, 0, {}, FLAG_PER_SEC | FLAG_KEEP_MOMENTS), "constrained": ("EI", 0.0, 0, {}, FLAG_CONSTRAINED | FLAG_KEEP_MOMENTS),
        "time_only": ("EI", 0.0, 0, {}, FLAG_PER_SEC | FLAG_KEEP_MOMENTS | FLAG_TIME_ONLY)}
ACQ_OPTS = ("mes_fantasies", "kg_fantasies", "kg_scan")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:10]


def tail(e, timing):
    s = "stats=" + ",".join("%d" % e.stat(k) for k in STATS)
    if timing:
        s += " launches=" + ",".join("%d" % v[1] for v in e.timings().values())
    return s


def attempt(f):
    """'ok', or the text of the refusal."""
    try:
        f()
        return "ok"
    except Exception as ex:     # noqa: BLE001  (the text is the record)
        return "%s: %s" % (type(ex).__name__, ex)


def outputs(e, row, H, flags):
    """The SHA-256 of everything the getters serve after the pass of `row`."""
    acq, _, nf, _, _ = ROWS[row]
    res = []
    if row != "time_only":
        idx, val = e.best()
        res += ["best=%d/%s" % (idx, sha(np.array(val))), "mean=" + sha(e.ei_mean()), "draws=" + sha(e.ei_draws())]
    for d in sorted(set((0, H - 1))):
        if (flags & FLAG_KEEP_MOMENTS or acq in ("MES", "EHVI")) and (nf == 0) and row != "time_only":
            res.append("mom%d=%s" % (d, sha(*e.get_moments(d))))
        if flags & FLAG_PER_SEC:
            res.append("tmean%d=%s" % (d, sha(e.get_time_mean(d))))
        if flags & FLAG_CONSTRAINED:
            res.append("cprob%d=%s" % (d, sha(e.get_constraint_prob(d))))
        if acq == "MES" and nf == 0:
            res.append("mes%d=%s" % (d, sha(*[e.mes_info(d)[k] for k in ("ystar", "fit", "G")])))
        if acq == "MES" and nf:
            for s in (0, nf - 1):
                i = e.mes_fantasy_info(d, s)
                res.append("mesf%d.%d=%s" % (d, s, sha(i["ystar"], i["fit"], i["G"], *e.mes_fantasy_moments(d, s))))
        if acq == "KG":
            keep = bool(flags & FLAG_KEEP_MOMENTS)
            res.append("kgl%d=%s" % (d, sha(*e.kg_lines(d, want_cov=keep))))
            if nf:
                res.append("kgfv%d=%s" % (d, sha(e.kg_fantasy_var(d))))
                for s in (0, nf - 1):
                    res.append("kgf%d.%d=%s" % (d, s, sha(*e.kg_fantasy_lines(d, s, want_mu_c=keep))))
    return res


def main(lib, out_path):
    e = Engine(0, lib=None if lib == "-" else lib)
    e.set_option("kstar_budget_bytes", 1 << 20)           # two chunks of one draw per item at N = 130, M = 1000
    out = open(out_path, "w")
    out.write("# stats: %s\n# launches: %s\n" % (",".join(STATS), ",".join(e.timings())))
    for N in NS:
        for H in HS:
            comp, cand, vals, hypers, log_durs, th = synthetic_problem(N, M, D, H, 100 * N + H, per_sec=True)
            rs = np.random.RandomState(N + H)
            crows = np.column_stack((rs.uniform(0.5, 3.0, H), np.full(H, 1e-3), rs.uniform(0.5, 2.0, H), rs.uniform(0.3, 1.5, (H, D))))
            ff = rs.randn(N) * 1.5
            fant = rs.randn(H, N, S)
            bests = np.min(fant, axis=1) - 0.1
            pts = rs.uniform(0.0, 1.0, (A, D))
            base, levels = rs.uniform(0.0, 1.0, (4, D)), np.linspace(0.0, 1.0, 3)
            e.set_observations(comp, vals)
            e.set_candidates(cand)
            for timing in (0, 1):
                for streams in (1, 2, 3):
                    e.set_option("streams", streams)
                    for row, (acq, par, nf, opts, flags) in ROWS.items():
                        for step in ((0, 1) if nf == 0 else (0,)):
                            e.set_hypers(hypers)
                            need_time = acq == "EHVI" or flags & FLAG_PER_SEC
                            e.set_time_model(log_durs, th) if need_time else e.set_time_model(None, None)
                            e.set_constraint_model(comp, ff, crows) if flags & FLAG_CONSTRAINED else e.set_constraint_model(None, None, None)
                            e.set_pareto_front([[-1.0, 0.5], [0.0, -0.5]], (5.0, 5.0)) if acq == "EHVI" else e.set_pareto_front(None, None)
                            e.set_kg_points(pts if acq == "KG" else None)
                            for k in ACQ_OPTS:
                                e.set_option(k, opts.get(k, 0))
                            e.set_acquisition(acq, par)
                            e.set_option("timing", timing)
                            if step:
                                e.ei_step(flags)
                            else:
                                e.factor()
                                if nf:
                                    e.set_fantasies(fant, bests)
                                e.ei_run(flags)
                            stats = tail(e, timing)
                            out.write("pass N=%d H=%d streams=%d %s step=%d timing=%d %s %s\n"
                                      % (N, H, streams, row, step, timing, " ".join(outputs(e, row, H, flags)), stats))
                            e.set_fantasies(None, None)
                            e.set_acquisition("EI")
                    # Thompson sampling (F = 32, S = 3) and the main effects (Q = 4, T = 3) under an acquisition that is not EI:
                    # what spx_get_acquisition reports afterwards is what was set
                    e.set_hypers(hypers)
                    e.set_time_model(None, None)
                    e.set_option("timing", timing)
                    e.factor()
                    idx, mn, _ = e.thompson(S=S, F=32, rng=np.random.RandomState(N))
                    stats = tail(e, timing)
                    res = ["idx=" + sha(idx), "min=" + sha(mn)]
                    for d in sorted(set((0, H - 1))):
                        res.append("ts%d=%s" % (d, sha(e.thompson_path(d, S - 1), *e.thompson_prior(d, 0))))
                    out.write("ts N=%d H=%d streams=%d timing=%d %s %s\n" % (N, H, streams, timing, " ".join(res), stats))
                    for acq, par in (("EI", 0.0), ("LCB", 2.0), ("MES", K)):
                        e.set_acquisition(acq, par)
                        curves = e.main_effects(base, levels)
                        out.write("effects N=%d H=%d streams=%d timing=%d acq=%s curves=%s acq_after=%r %s\n"
                                  % (N, H, streams, timing, acq, sha(curves["curves"], curves["base_mean"]), e.get_acquisition(), tail(e, timing)))
                        e.set_candidates(cand)
                    e.set_acquisition("EI")
                e.set_option("timing", 0)
                e.set_option("streams", 1)
            # the refusals, by their text (two-call form and step)
            e.set_hypers(hypers)
            e.factor()
            big = rs.uniform(0.0, 1.0, (300, D))
            refusals = []
            for name, acq, par, opts, nf, flags, points in (
                    ("kg_fant_off", "KG", 0.0, {}, S, 0, pts), ("mes_fant_off", "MES", K, {}, S, 0, None),
                    ("ehvi_fant", "EHVI", 0.0, {}, S, 0, None), ("ehvi_no_front", "EHVI", 0.0, {}, 0, 0, None),
                    ("kg_per_sec", "KG", 0.0, {}, 0, FLAG_PER_SEC, pts), ("pi_per_sec", "PI", 0.01, {}, 0, FLAG_PER_SEC, None),
                    ("kg_no_points", "KG", 0.0, {}, 0, 0, None), ("kg_300_no_scan", "KG", 0.0, {"kg_scan": 1}, 0, 0, big),
                    ("kg_300_fant_narrow", "KG", 0.0, {"kg_scan": 1, "kg_fantasies": 1}, S, 0, big),
                    ("time_only_alone", "EI", 0.0, {}, 0, FLAG_TIME_ONLY, None), ("per_sec_no_model", "EI", 0.0, {}, 0, FLAG_PER_SEC, None),
                    ("constrained_no_model", "EI", 0.0, {}, 0, FLAG_CONSTRAINED, None)):
                for form in ("run", "step"):
                    e.set_hypers(hypers)
                    e.set_time_model(log_durs, th) if name == "ehvi_fant" else e.set_time_model(None, None)
                    e.set_pareto_front([[-1.0, 0.5], [0.0, -0.5]], (5.0, 5.0)) if name == "ehvi_fant" else e.set_pareto_front(None, None)
                    e.factor()
                    for k in ACQ_OPTS:
                        e.set_option(k, opts.get(k, 0))
                    e.set_kg_points(points)
                    if name == "kg_300_no_scan":
                        e.set_option("kg_scan", 0)        # (the points were set while the option was on)
                    if nf:
                        e.set_fantasies(fant, bests)
                    e.set_acquisition(acq, par)
                    text = attempt((lambda: e.ei_run(flags)) if form == "run" else (lambda: e.ei_step(flags)))
                    refusals.append("refusal N=%d H=%d %s %s fantasies_after=%d: %s\n" % (N, H, name, form, e.stat("fantasies_count"), text))
                    e.set_fantasies(None, None)
                    e.set_acquisition("EI")
            out.writelines(refusals)
            e.set_kg_points(None)
            for k in ACQ_OPTS:
                e.set_option(k, 0)
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
        if kind == "refusal" and n == "N=130" and h == "H=3":
            sys.stdout.write(line)
    for (kind, n, h), lines in groups.items():
        print("%s %s %s cases=%d sha256=%s" % (kind, n, h, len(lines), hashlib.sha256("".join(lines).encode()).hexdigest()[:32]))


if __name__ == "__main__":
    digest(sys.argv[2]) if sys.argv[1] == "--digest" else main(sys.argv[1], sys.argv[2])
