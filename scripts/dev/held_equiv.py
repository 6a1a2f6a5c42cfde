"""Dev tool: seeded random walks over the whole API of one handle, at the shapes of tests/held_helpers.py -- after every call one
line with the call's outcome and error text, accept / refuse of every getter with the SHA-256 of what it served, the
statistics, spx_not_pd_info and (the walks with option timing) the launches per stage.  Two builds of the library that keep
the same state give the same record line for line (profiles/held_refactor_equiv.log: the build before csrc/spx_held.h
against the build after it, each in its own process).
   python scripts/dev/held_equiv.py LIB|- OUTFILE [walks]          (- : the in-tree library)
        [--devices 0,0[,0,0] [--hyper-shards P]]                   (the same walks on the front of a multi-device handle over
                                                                      these device ids, without the constraint calls that it
                                                                      refuses outright: profiles/multi_held_equiv.log)
   python scripts/dev/held_equiv.py --compare PARENT_OUT CHILD_OUT   (the digest of the child's record and every differing
                                                                      line, sorted by cause)"""
import hashlib
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)

WALKS, STEPS = 400, 12
STATS = ("obs_dims", "last_fantasies_device", "fantasies_pending_rows", "fantasies_count", "flow_fallbacks", "flow_enabled",
         "last_step_fused", "last_factor_flow", "last_factor_cov_in_flow", "last_logprob_one_launch", "last_step_skipped_padding")
FRONT_STATS = ("obs_dims", "last_fantasies_device", "fantasies_pending_rows", "fantasies_count", "flow_fallbacks", "flow_rearms",
               "ranks_seen")            # what a multi-device handle answers itself


def record(lib, out_path, walks, devices=None, hyper_shards=1):
    from tests import held_helpers as hh
    p = hh.Problem()
    calls = hh.front_calls() if devices else hh.CALLS
    stats = FRONT_STATS if devices else STATS
    getters = dict(hh.GETTERS)
    getters["get_cross_cov"] = lambda e, p: e.get_cross_cov(hh.H - 1, 0, 5)       # (needs the factor AND candidates)
    names = sorted(calls)
    out = open(out_path, "w")
    out.write("# getters: %s\n# stats: %s\n" % (",".join(getters), ",".join(stats)))
    if devices:
        out.write("# front: devices=%s hyper_shards=%d\n" % (",".join("%d" % d for d in devices), hyper_shards))
    for w in range(walks):
        rs = np.random.RandomState(1000 + w)
        e = hh.engine(None if lib == "-" else lib, devices, hyper_shards)    # a walk starts on a new handle: no difference outlives its walk
        timing = w & 1
        e.set_option("timing", timing)
        for k in range(STEPS):
            # the first calls of a walk lean towards the setters, so that most walks get as far as a factor and a pass
            name = names[rs.randint(len(names))]
            if k < 3 and rs.rand() < 0.8:
                name = ("set_observations", "set_candidates", "set_hypers")[k]
            kind, res = hh.outcome(calls[name], e, p)
            served = []
            for g, fn in getters.items():
                gk, gres = hh.outcome(fn, e, p)
                served.append("%s=%s" % (g, hh.sha(gres) if gk == "ok" else "-"))
            line = "w=%d t=%d k=%d call=%s rc=%s res=%s %s stats=%s npd=%d/%d" % (
                w, timing, k, name.replace(" ", ""), kind, hh.sha(res) if kind == "ok" and res is not None else "-",
                " ".join(served), ",".join("%d" % e.stat(s) for s in stats), *hh.not_pd_info(e))
            if timing:
                line += " launches=" + ",".join("%d" % v[1] for v in e.timings().values())
            out.write(line + " | err=" + (res if kind != "ok" else "-") + "\n")
        e.close()
        if w % 50 == 49:
            out.flush()
            print("%d walks" % (w + 1), flush=True)
    out.close()


def fields(line):
    head, err = line.rstrip("\n").split(" | err=")
    d = dict(tok.split("=", 1) for tok in head.split())
    d["err"] = err
    return d


def cause(parent, child, diff):
    """Which of the expected differences a run of differing lines belongs to: by the call that opened it and what differs there."""
    call = child["call"]
    if parent["rc"] not in ("ok", "arg"):
        return "1 a call failed part-way: what it was overwriting is refused afterwards"
    if call == "set_time_model(NULL)":
        return "2 spx_set_time_model(NULL, NULL) drops results (and, with the factor, the fantasies: their statistics)"
    if call == "set_constraint_model(NULL)":
        return "3 spx_set_constraint_model(NULL, ..) drops results"
    if call.startswith("set_option(covar"):
        return "4 option covar marks the constraint and full factorisations not held at once"
    if call == "set_time_model" and set(diff) == {"stats"}:
        return "5 spx_set_time_model drops the fantasies with the factor, as include/spx.h says: their statistics read 0 at once"
    if call in ("set_constraint_model", "set_partition") and set(diff) == {"get_time_mean"}:
        return "6 the durations of a SPX_FLAG_TIME_ONLY pass are results: %s drops them with the rest" % call
    return "UNEXPLAINED"


def front_cause(parent, child, diff):
    """The same for two records of a multi-device handle (profiles/multi_held_equiv.log: the build whose front kept six loose
    flags against the build whose front keeps a Held)."""
    call = child["call"]
    if parent["rc"] not in ("ok", "arg"):
        return "1 a call failed part-way: what it was overwriting is refused by every reader of the front afterwards"
    if call in ("set_fantasies", "draw_fantasies") and parent["rc"] == "arg" and "2-D partition" in parent["err"]:
        return "3 %s refused in the 2-D partition no longer drops the results" % call
    if call in ("set_fantasies(NULL)", "draw_fantasies(NULL)"):
        return "4 the clear forms keep the last results readable, as on a single handle"
    if set(diff) == {"err"} and parent["err"].startswith(child["err"] + " (device slot "):
        return ("5 (further) a refusal the front now makes from its own record, before a kid is asked: the same text without the "
                "kid's '(device slot i)'")
    if call.startswith("set_option(covar") and parent["rc"] == "ok" and all(v[0] == "-" for k, v in diff.items() if k != "npd"):
        return ("6 (further) option covar set to the value it has (whichever of the two calls sets it) drops nothing, as on a "
                "single handle (row FACTOR: made from option covar -- which did not change); the front used to refuse its own "
                "results after it")
    if set(diff) == {"npd"}:
        return ("7 (further) 'the kids hold the shards of the last spx_gp_logprob' is one fact now, and spx_not_pd_info reports "
                "that batch, in the handle's numbering, exactly while it holds: spx_set_observations does not end it (the kids "
                "keep those hypers), the re-broadcast that spx_set_time_model begins with does (rows HYP and FACTOR of the front's "
                "table in DESIGN.md)")
    return "UNEXPLAINED"


def compare(parent_path, child_path):
    global cause
    if any(ln.startswith("# front:") for ln in open(child_path)):
        cause = front_cause
    pl = [ln for ln in open(parent_path) if not ln.startswith("#")]
    cl = [ln for ln in open(child_path) if not ln.startswith("#")]
    assert len(pl) == len(cl), (len(pl), len(cl))
    print("lines: %d each; child's record sha256 %s; parent's %s" % (
        len(cl), hashlib.sha256("".join(cl).encode()).hexdigest()[:32], hashlib.sha256("".join(pl).encode()).hexdigest()[:32]))
    per_call = {}
    for ln in cl:
        per_call.setdefault(fields(ln)["call"], []).append(ln)
    for call in sorted(per_call):
        print("  %-34s lines=%4d sha256=%s" % (call, len(per_call[call]), hashlib.sha256("".join(per_call[call]).encode()).hexdigest()[:16]))
    runs, cur = {}, None
    for a, b in zip(pl, cl):
        fa, fb = fields(a), fields(b)
        assert (fa["w"], fa["k"], fa["call"]) == (fb["w"], fb["k"], fb["call"])
        if fa["k"] == "0":
            cur = None
        if a == b:
            cur = None
            continue
        diff = {k: (fa[k], fb[k]) for k in fa if fa[k] != fb.get(k)}
        if cur is None:
            cur = cause(fa, fb, diff)
        runs.setdefault(cur, []).append("w=%s k=%s %s: %s" % (fa["w"], fa["k"], fa["call"], "  ".join(
            "%s %s -> %s" % (k, v[0], v[1]) for k, v in sorted(diff.items()))))
    print("differing lines: %d of %d" % (sum(len(v) for v in runs.values()), len(cl)))
    for c in sorted(runs):
        print("\n== %s: %d lines (parent -> child)" % (c, len(runs[c])))
        for ln in runs[c]:
            print("  " + ln)
    return 1 if "UNEXPLAINED" in runs else 0


if __name__ == "__main__":
    args, devices, shards = sys.argv[1:], None, 1
    for flag in ("--devices", "--hyper-shards"):
        if flag in args:
            i = args.index(flag)
            if flag == "--devices":
                devices = [int(d) for d in args[i + 1].split(",")]
            else:
                shards = int(args[i + 1])
            del args[i:i + 2]
    if args[0] == "--compare":
        sys.exit(compare(args[1], args[2]))
    record(args[0], args[1], int(args[2]) if len(args) > 2 else WALKS, devices, shards)
