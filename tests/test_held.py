"""csrc/spx_held.h on a CPU: what a handle holds, what dropping a thing takes with it, and that no sequence of entry points --
failed ones included -- reaches a state in which a product is held without what it was made from.  The header is run by
tests/c/held_client.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers
(tests/plan_helpers.py).  Every expected set here is a literal written from the table in DESIGN.md ("What a handle holds"),
none is asked of the code under test."""
import pytest

from tests import plan_helpers as ph

pytestmark = pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")

THINGS = ["OBS", "CAND", "HYP", "TIME", "CON", "FACTOR", "CON_FACTOR", "FULL_FACTOR", "FANT", "ALPHA_S", "RESULTS",
          "COVAR", "PARTITION"]                      # the order of Held::Thing; the last two are never held
REAL = THINGS[:11]
NUM = {t: i for i, t in enumerate(THINGS)}
TIME_ONLY, MOMENTS, TMEAN, CONP, GLOBAL2D = 1, 2, 4, 8, 16        # the result attributes, as held_client.cpp numbers them

# drop(X) from "everything held" leaves ...
LEFT_AFTER_DROP = {
    "OBS": {"CAND", "HYP", "CON", "CON_FACTOR"},
    "CAND": {"OBS", "HYP", "TIME", "CON", "FACTOR", "CON_FACTOR", "FULL_FACTOR", "FANT", "ALPHA_S"},
    "HYP": {"OBS", "CAND", "CON", "CON_FACTOR"},
    "TIME": {"OBS", "CAND", "HYP", "CON", "CON_FACTOR", "FULL_FACTOR"},
    "CON": {"OBS", "CAND", "HYP", "TIME", "FACTOR", "FANT", "ALPHA_S"},
    "FACTOR": {"OBS", "CAND", "HYP", "TIME", "CON", "CON_FACTOR", "FULL_FACTOR"},
    "CON_FACTOR": set(REAL) - {"CON_FACTOR"},
    "FULL_FACTOR": set(REAL) - {"FULL_FACTOR"},
    "FANT": {"OBS", "CAND", "HYP", "TIME", "CON", "FACTOR", "CON_FACTOR", "FULL_FACTOR"},
    "ALPHA_S": set(REAL) - {"ALPHA_S"},
    "RESULTS": set(REAL) - {"RESULTS"},
    "COVAR": {"OBS", "CAND", "HYP", "TIME", "CON"},
    "PARTITION": set(REAL) - {"RESULTS"},
}
# what set(X) needs held (the rest of "made from" may be absent when X is made: a factor without a time model, a pass
# without fantasies or a constraint model)
NEEDS = {
    "OBS": set(), "CAND": set(), "HYP": set(), "CON": set(),
    "TIME": {"OBS", "HYP"},
    "FACTOR": {"OBS", "HYP"},
    "CON_FACTOR": {"CON"},
    "FULL_FACTOR": {"OBS", "HYP", "CON"},
    "FANT": {"FACTOR"},
    "ALPHA_S": {"FANT"},
    "RESULTS": {"FACTOR", "CAND"},
}


def bits(names):
    return sum(1 << NUM[n] for n in names)


def names(b):
    return {t for t in THINGS if b >> NUM[t] & 1}


def run(ops):
    """ops: (bits, attrs, "drop" | "set", thing, new_attrs) -> [(bits, attrs, ok)], one run of the client."""
    text = "".join("%d %d %s %d %d\n" % (b, a, op, NUM[t], na) for b, a, op, t, na in ops)
    out = [tuple(int(v) for v in line.split()) for line in ph.ask("held_client", text)]
    assert len(out) == len(ops)
    return out


def test_drop_table():
    full = bits(REAL)
    got = run([(full, MOMENTS | TMEAN, "drop", t, 0) for t in THINGS])
    for t, (b, a, ok) in zip(THINGS, got):
        assert names(b) == LEFT_AFTER_DROP[t], (t, sorted(names(b)))
        assert a == (MOMENTS | TMEAN if "RESULTS" in LEFT_AFTER_DROP[t] else 0), (t, a)


def test_drop_of_what_is_not_held_still_takes_what_was_made_from_it():
    # (an entry point drops what it is ABOUT to write: the first spx_set_candidates of a handle, say)
    (b, a, ok), = run([(bits(REAL) & ~bits(["CAND"]), MOMENTS, "drop", "CAND", 0)])
    assert names(b) == LEFT_AFTER_DROP["CAND"] and a == 0


def test_set_guard():
    ops, want = [], []
    for t in REAL:
        for missing in sorted(NEEDS[t]):
            ops.append((bits(REAL) & ~bits([t, missing]), 0, "set", t, 0))
            want.append((bits(REAL) & ~bits([t, missing]), 0, 0))          # refused, nothing changed
        ops.append((bits(NEEDS[t]), 0, "set", t, MOMENTS if t == "RESULTS" else 0))
        want.append((bits(NEEDS[t] | {t}), MOMENTS if t == "RESULTS" else 0, 1))
    for t in ("COVAR", "PARTITION"):                                       # never held
        ops.append((bits(REAL), 0, "set", t, 0))
        want.append((bits(REAL), 0, 0))
    assert run(ops) == want


# ---- every state any sequence of entry points can reach ---------------------------------------------------------------------
# An entry point: what it refuses without (before it touches anything), then its steps in order -- the drops at its
# beginning, the sets at its end.  A call can fail after any step, so every prefix of the steps ends in a reachable state.
# A pass may leave any combination of the result attributes (more than the flags of spx_ei_run can produce: a superset of the
# reachable states is checked).
PASSES = range(32)


def entry_points(held, attrs):
    """[(name, steps)] of the calls that state (held names, attrs) does not refuse outright."""
    D, S = "drop", "set"
    eps = [("set_observations", [(D, "OBS"), (S, "OBS")]),
           ("set_observations, another D", [(D, "OBS"), (D, "CAND"), (D, "HYP"), (S, "OBS")]),
           ("set_candidates / sobol_grid(as_candidates)", [(D, "CAND"), (S, "CAND")]),
           ("set_time_model(NULL)", [(D, "TIME")]),
           ("set_constraint_model(NULL)", [(D, "CON")]),
           ("set_option(covar)", [(D, "COVAR")]),
           ("comm_attach / set_partition", [(D, "PARTITION")]),
           ("clear fantasies", [(D, "FANT")] + ([(S, "RESULTS", attrs)] if "RESULTS" in held else []))]
    if "OBS" in held:
        eps.append(("set_hypers", [(D, "HYP"), (S, "HYP")]))
    if {"OBS", "HYP"} <= held:
        eps.append(("set_time_model", [(D, "TIME"), (S, "TIME")]))
        eps.append(("set_constraint_model", [(D, "CON"), (S, "CON")]))
        eps.append(("gp_logprob", [(D, "FACTOR")]))
        con = [(S, "CON_FACTOR")] if "CON" in held else []
        eps.append(("factor", con + [(D, "FACTOR"), (S, "FACTOR")]))
        if "CAND" in held:
            for a in PASSES:
                eps.append(("ei_step", con + [(D, "FACTOR"), (D, "RESULTS"), (S, "FACTOR"), (S, "RESULTS", a)]))
    if "FACTOR" in held:
        eps.append(("set_fantasies / draw_fantasies", [(D, "FANT"), (S, "FANT")]))
        if "CAND" in held:
            for a in PASSES:
                eps.append(("ei_run", [(D, "RESULTS"), (S, "RESULTS", a)]))
        if "FANT" in held:
            eps.append(("ei_grad_batch", [(S, "ALPHA_S")]))
        if {"CON", "CON_FACTOR"} <= held:
            eps.append(("constrained_ei_grad_batch", [(S, "ALPHA_S")] if "FANT" in held else [(S, "FULL_FACTOR")]))
    return eps


FRONT = ["OBS", "CAND", "HYP", "TIME", "FACTOR", "FANT", "RESULTS"]     # what a multi-device handle's own record ever holds


def front_entry_points(held, attrs):
    """The same for the front of a multi-device handle (csrc/spx_multi.hip): no constraint model; spx_ei_step is spx_factor, then
    spx_ei_run; another hyper-shard count takes the draws and the candidates with it; no ALPHA_S of its own."""
    D, S = "drop", "set"
    eps = [("set_observations", [(D, "OBS"), (S, "OBS")]),
           ("set_observations, another D", [(D, "OBS"), (D, "CAND"), (D, "HYP"), (S, "OBS")]),
           ("set_candidates / sobol_grid(as_candidates)", [(D, "CAND"), (S, "CAND")]),
           ("set_time_model(NULL)", [(D, "TIME")]),
           ("set_option(covar)", [(D, "COVAR")]),
           ("set_acquisition", [(D, "RESULTS")]),
           ("set_partition(other ph)", [(D, "HYP"), (D, "CAND"), (D, "PARTITION")]),
           ("clear fantasies", [(D, "FANT")] + ([(S, "RESULTS", attrs)] if "RESULTS" in held else []))]
    if "OBS" in held:
        eps.append(("set_hypers", [(D, "HYP"), (S, "HYP")]))
    if "HYP" in held:
        eps.append(("gp_logprob", [(D, "FACTOR")]))
    if {"OBS", "HYP"} <= held:
        eps.append(("set_time_model", [(D, "TIME"), (S, "TIME")]))
        eps.append(("factor", [(D, "FACTOR"), (S, "FACTOR")]))
        if "CAND" in held:
            for a in PASSES:
                eps.append(("ei_step", [(D, "FACTOR"), (S, "FACTOR"), (D, "RESULTS"), (S, "RESULTS", a)]))
    if "FACTOR" in held:
        eps.append(("set_fantasies / draw_fantasies", [(D, "FANT"), (S, "FANT")]))
        eps.append(("ei_grad_batch", []))
        if "CAND" in held:
            for a in PASSES:
                eps.append(("ei_run", [(D, "RESULTS"), (S, "RESULTS", a)]))
    return [(name, steps) for name, steps in eps if steps]


def test_reachable_states():
    seen = reachable(entry_points, REAL)
    # (how many there are is not asserted tightly: the model above grows with the API -- 850 today, 106 sets of things, the 24
    # of them with RESULTS under 32 attribute combinations -- but an enumeration that stopped early would mean the walk is broken)
    assert len(seen) > 500, len(seen)
    assert (bits(REAL) & ~bits(["FULL_FACTOR"]), MOMENTS | TMEAN) in seen


def test_reachable_states_of_the_front():
    seen = reachable(front_entry_points, FRONT)
    # 22 sets of things: CAND or not, times { OBS and HYP not both: 3; both: TIME or not, times { no FACTOR; FACTOR: FANT or not,
    # times RESULTS or not where CAND is held } }; the 4 of them with RESULTS under 32 attribute combinations
    assert len(seen) == 18 + 4 * 32, len(seen)
    assert (bits(FRONT), MOMENTS | TMEAN | GLOBAL2D) in seen


def reachable(entry_points, allowed):
    """Every (bits, attrs) that sequences of `entry_points` reach from a new handle, a failure allowed after any step; the
    invariants are held to each of them."""
    seen = {(0, 0)}
    frontier = [(0, 0)]
    while frontier:
        # walk every entry point of every new state one step at a time; each step of all of them is one run of the client
        walks = [[state, steps, name] for state in frontier for name, steps in entry_points(names(state[0]), state[1])]
        frontier = []
        depth = 0
        while walks:
            ops = [(st[0], st[1], steps[depth][0], steps[depth][1], steps[depth][2] if len(steps[depth]) > 2 else 0)
                   for st, steps, _ in walks]
            nxt = []
            for (st, steps, name), (b, a, ok) in zip(walks, run(ops)):
                op = steps[depth][0]
                assert ok, ("refused inside an entry point that its own checks let through", name, sorted(names(st[0])), steps[depth])
                if op == "drop":
                    assert b & ~st[0] == 0, ("drop added a bit", name, sorted(names(st[0])), sorted(names(b)))
                held = names(b)
                for t in held:
                    assert t in allowed and NEEDS[t] <= held, ("held without what it was made from", name, t, sorted(held))
                if "RESULTS" not in held:
                    assert a == 0, ("result attributes without results", name, sorted(held), a)
                if (b, a) not in seen:
                    seen.add((b, a))
                    frontier.append((b, a))
                if depth + 1 < len(steps):
                    nxt.append([(b, a), steps, name])
            walks = nxt
            depth += 1
    return seen
