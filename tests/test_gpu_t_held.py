"""What a handle holds after each entry point (csrc/spx_held.h), seen from outside: every reader after every writer against a
literal table of accept / refuse, calls that fail without a fault, and the two clear forms that used to leave results
readable.  The tables are written from the "made from" table of DESIGN.md ("What a handle holds"), not taken from a run."""
import numpy as np
import pytest

from tests import held_helpers as hh

pytestmark = pytest.mark.gpu

# the readers, in the order of a table row: the getters first (they change nothing), then the entry points that need
# something held -- each of those leaves what the ones after it need as it was
READERS = ["get_best", "get_ei_mean", "get_ei_draws", "get_moments", "get_time_mean", "get_constraint_prob", "get_factor",
           "get_factor_rows", "get_pending_fantasies", "ei_run(bare)", "ei_grad_batch", "constrained_ei_grad_batch",
           "set_fantasies", "draw_fantasies"]
NONE = "RRRRRRRRRRRRRR"      # neither a factor nor results
#                                           bmdMTC FRP rgc sd      (A accepted, R refused, one letter per reader)
TABLE = {
    "plain": {                              # OBS CAND HYP FACTOR FANT (device) RESULTS; with fantasies a pass keeps no moments
        None:                               "AAARRR" "AAA" "AAR" "AA",
        "set_observations":                 NONE,
        "set_candidates":                   "RRRRRR" "AAA" "AAR" "AA",
        "set_hypers":                       NONE,
        "set_time_model":                   NONE,
        "set_time_model(NULL)":             NONE,
        "set_constraint_model":             "RRRRRR" "AAA" "AAR" "AA",      # (a constraint model that is not factored yet)
        "set_constraint_model(NULL)":       "RRRRRR" "AAA" "AAR" "AA",
        "set_option(covar, other)":         NONE,
        "set_option(covar, same)":          "AAARRR" "AAA" "AAR" "AA",
        "gp_logprob":                       NONE,
        "sobol_grid(as_candidates)":        "RRRRRR" "AAA" "AAR" "AA",
        "set_partition":                    "RRRRRR" "AAA" "AAR" "AA",
        "factor":                           "RRRRRR" "AAR" "AAR" "AA",
        "set_fantasies(NULL)":              "AAARRR" "AAR" "AAR" "AA",      # the last pass stays readable
        "draw_fantasies(NULL)":             "AAARRR" "AAR" "AAR" "AA",
        "set_fantasies":                    "RRRRRR" "AAR" "AAR" "AA",      # (fantasies from the host: no pending rows to serve)
        "draw_fantasies":                   "RRRRRR" "AAA" "AAR" "AA",
        "ei_run(plain)":                    "AAARRR" "AAA" "AAR" "AA",
        "ei_step(plain)":                   "AAAARR" "AAR" "AAR" "AA",      # a new factor: no fantasies, so moments are kept
        "ei_grad_batch":                    "AAARRR" "AAA" "AAR" "AA",
    },
    "per_sec": {                            # OBS CAND HYP TIME FACTOR RESULTS (moments, durations)
        None:                               "AAAAAR" "AAR" "AAR" "AA",
        "set_observations":                 NONE,
        "set_candidates":                   "RRRRRR" "AAR" "AAR" "AA",
        "set_hypers":                       NONE,
        "set_time_model":                   NONE,
        "set_time_model(NULL)":             NONE,
        "set_constraint_model":             "RRRRRR" "AAR" "AAR" "AA",      # (the refinement objective is not defined with a time model)
        "set_constraint_model(NULL)":       "RRRRRR" "AAR" "AAR" "AA",
        "set_option(covar, other)":         NONE,
        "set_option(covar, same)":          "AAAAAR" "AAR" "AAR" "AA",
        "gp_logprob":                       NONE,
        "sobol_grid(as_candidates)":        "RRRRRR" "AAR" "AAR" "AA",
        "set_partition":                    "RRRRRR" "AAR" "AAR" "AA",
        "factor":                           "RRRRRR" "AAR" "AAR" "AA",
        "set_fantasies(NULL)":              "AAAAAR" "AAR" "AAR" "AA",
        "draw_fantasies(NULL)":             "AAAAAR" "AAR" "AAR" "AA",
        "set_fantasies":                    "RRRRRR" "AAR" "ARR" "AA",      # (fantasies with a time model: no refinement objective)
        "draw_fantasies":                   "RRRRRR" "AAA" "ARR" "AA",
        "ei_run(per_sec)":                  "AAAAAR" "AAR" "AAR" "AA",
        "ei_step(per_sec)":                 "AAAAAR" "AAR" "AAR" "AA",
        "ei_grad_batch":                    "AAAAAR" "AAR" "AAR" "AA",
    },
    "constrained": {                        # OBS CAND HYP CON FACTOR CON_FACTOR FULL_FACTOR RESULTS (moments, probabilities)
        None:                               "AAAARA" "AAR" "AAA" "AA",
        "set_observations":                 NONE,
        "set_candidates":                   "RRRRRR" "AAR" "AAA" "AA",
        "set_hypers":                       NONE,
        "set_time_model":                   NONE,
        "set_time_model(NULL)":             NONE,
        "set_constraint_model":             "RRRRRR" "AAR" "AAR" "AA",      # the new model is not factored yet
        "set_constraint_model(NULL)":       "RRRRRR" "AAR" "AAR" "AA",
        "set_option(covar, other)":         NONE,
        "set_option(covar, same)":          "AAAARA" "AAR" "AAA" "AA",
        "gp_logprob":                       NONE,
        "sobol_grid(as_candidates)":        "RRRRRR" "AAR" "AAA" "AA",
        "set_partition":                    "RRRRRR" "AAR" "AAA" "AA",
        "factor":                           "RRRRRR" "AAR" "AAA" "AA",
        "set_fantasies(NULL)":              "AAAARA" "AAR" "AAA" "AA",
        "draw_fantasies(NULL)":             "AAAARA" "AAR" "AAA" "AA",
        "set_fantasies":                    "RRRRRR" "AAR" "AAA" "AA",
        "draw_fantasies":                   "RRRRRR" "AAA" "AAA" "AA",
        "ei_run(constrained)":              "AAAARA" "AAR" "AAA" "AA",
        "ei_step(constrained)":             "AAAARA" "AAR" "AAA" "AA",
        "ei_grad_batch":                    "AAAARA" "AAR" "AAA" "AA",
    },
}
CASES = [(kind, writer) for kind, rows in TABLE.items() for writer in rows]


@pytest.fixture(scope="module")
def prob():
    return hh.Problem()


@pytest.fixture(scope="module")
def eng():
    e = hh.engine()
    yield e
    e.close()


def readers_row(e, p):
    row = ""
    for name in READERS:
        kind, res = hh.outcome(hh.GETTERS.get(name) or hh.CALLS[name], e, p)
        assert kind in ("ok", "arg"), (name, kind, res)        # accepted, or refused as an argument error: never a fault
        row += "A" if kind == "ok" else "R"
    return row


@pytest.mark.parametrize("kind,writer", CASES, ids=["%s-%s" % (k, w or "base") for k, w in CASES])
def test_accept_refuse_table(eng, prob, kind, writer):
    assert len(TABLE[kind][writer]) == len(READERS)
    hh.base(eng, prob, kind)
    if writer is not None:
        hh.CALLS[writer](eng, prob)
    got = readers_row(eng, prob)
    print(kind, writer, got)
    assert got == TABLE[kind][writer]


@pytest.fixture(scope="module")
def fresh_bits(prob):
    """What a handle that has done nothing else serves after spx_ei_step with kept moments."""
    e = hh.engine()
    hh.reset(e, prob)
    e.ei_step(hh.FLAGS["plain"])
    bits = hh.read_all(e, prob)
    e.close()
    assert bits["get_best"] and bits["get_moments"] and bits["get_factor"]
    return bits


@pytest.mark.parametrize("call", ["factor", "ei_step(plain)"])
def test_a_call_that_fails_without_a_fault_leaves_nothing_of_what_it_was_overwriting(eng, prob, fresh_bits, call):
    hh.reset(eng, prob)
    eng.ei_step(hh.FLAGS["plain"])                       # a factor and results are held
    assert hh.read_all(eng, prob) == fresh_bits
    eng.set_hypers(prob.bad_hypers)
    kind, text = hh.outcome(hh.CALLS[call], eng, prob)
    assert kind == "not_pd" and "1-th leading minor" in text and "(draw 1)" in text, (kind, text)
    assert hh.not_pd_info(eng) == (1, 0)                 # draw 1, pivot 0: what the library has always reported here
    assert readers_row(eng, prob) == NONE
    hh.CALLS["set_hypers"](eng, prob)                    # the next good call: the bits of a fresh handle
    eng.ei_step(hh.FLAGS["plain"])
    assert hh.read_all(eng, prob) == fresh_bits
    assert hh.not_pd_info(eng) == (-1, -1)


# ---- the front of a multi-device handle: the same record and table (csrc/spx_multi.hip) -----------------------------------------
# On one GPU: two slots that share the candidates, and four slots in two draw shards x two candidate shards (the 2-D partition,
# which takes no fantasies: its "plain" base has none, so its pass keeps the moments).  What differs from the single handle, by
# spx_set_partition with the shard count the handle has changes nothing; the front holds no constraint model.
FRONT_READERS = ["get_best", "get_ei_mean", "get_ei_draws", "get_moments", "get_time_mean", "get_factor", "get_factor_rows",
                 "get_cross_cov", "get_pending_fantasies", "ei_run(bare)", "ei_grad_batch"]
F_NONE = "RRRRRRRRRRR"
#                                           bmdMT FRXP rg
FRONT_TABLE = {
    ("2", "plain"): {                       # OBS CAND HYP FACTOR FANT (device) RESULTS; with fantasies a pass keeps no moments
        None:                               "AAARR" "AAAA" "AA",
        "set_observations":                 F_NONE,
        "set_candidates":                   "RRRRR" "AAAA" "AA",
        "set_hypers":                       F_NONE,
        "set_time_model":                   F_NONE,
        "set_time_model(NULL)":             F_NONE,
        "set_option(covar, other)":         F_NONE,
        "set_option(covar, same)":          "AAARR" "AAAA" "AA",
        "gp_logprob":                       F_NONE,
        "sobol_grid(as_candidates)":        "RRRRR" "AAAA" "AA",
        "set_partition":                    "AAARR" "AAAA" "AA",      # (the count it has)
        "factor":                           "RRRRR" "AAAR" "AA",
        "set_fantasies(NULL)":              "AAARR" "AAAR" "AA",      # the last pass stays readable
        "draw_fantasies(NULL)":             "AAARR" "AAAR" "AA",
        "set_fantasies":                    "RRRRR" "AAAR" "AA",      # (fantasies from the host: no pending rows to serve)
        "draw_fantasies":                   "RRRRR" "AAAA" "AA",
        "ei_run(plain)":                    "AAARR" "AAAA" "AA",
        "ei_step(plain)":                   "AAAAR" "AAAR" "AA",      # a new factor: no fantasies, so moments are kept
        "ei_grad_batch":                    "AAARR" "AAAA" "AA",
    },
    ("2", "per_sec"): {                     # OBS CAND HYP TIME FACTOR RESULTS (moments, durations)
        None:                               "AAAAA" "AAAR" "AA",
        "set_observations":                 F_NONE,
        "set_candidates":                   "RRRRR" "AAAR" "AA",
        "set_hypers":                       F_NONE,
        "set_time_model":                   F_NONE,
        "set_time_model(NULL)":             F_NONE,
        "set_option(covar, other)":         F_NONE,
        "set_option(covar, same)":          "AAAAA" "AAAR" "AA",
        "gp_logprob":                       F_NONE,
        "sobol_grid(as_candidates)":        "RRRRR" "AAAR" "AA",
        "set_partition":                    "AAAAA" "AAAR" "AA",
        "factor":                           "RRRRR" "AAAR" "AA",
        "set_fantasies(NULL)":              "AAAAA" "AAAR" "AA",
        "draw_fantasies(NULL)":             "AAAAA" "AAAR" "AA",
        "set_fantasies":                    "RRRRR" "AAAR" "AR",      # (fantasies with a time model: no refinement objective)
        "draw_fantasies":                   "RRRRR" "AAAA" "AR",
        "ei_run(per_sec)":                  "AAAAA" "AAAR" "AA",
        "ei_step(per_sec)":                 "AAAAA" "AAAR" "AA",
        "ei_grad_batch":                    "AAAAA" "AAAR" "AA",
    },
    ("4x2", "plain"): {                     # OBS CAND HYP FACTOR RESULTS (moments); no refinement objective in the 2-D partition
        None:                               "AAAAR" "AAAR" "AR",
        "set_observations":                 F_NONE,
        "set_candidates":                   "RRRRR" "AAAR" "AR",
        "set_hypers":                       F_NONE,
        "set_time_model":                   F_NONE,
        "set_time_model(NULL)":             F_NONE,
        "set_option(covar, other)":         F_NONE,
        "set_option(covar, same)":          "AAAAR" "AAAR" "AR",
        "gp_logprob":                       F_NONE,
        "sobol_grid(as_candidates)":        "RRRRR" "AAAR" "AR",
        "set_partition":                    "AAAAR" "AAAR" "AR",
        "factor":                           "RRRRR" "AAAR" "AR",
        "set_fantasies(NULL)":              "AAAAR" "AAAR" "AR",
        "draw_fantasies(NULL)":             "AAAAR" "AAAR" "AR",
        "set_fantasies":                    "AAAAR" "AAAR" "AR",      # refused: nothing changes
        "draw_fantasies":                   "AAAAR" "AAAR" "AR",
        "ei_run(plain)":                    "AAAAR" "AAAR" "AR",
        "ei_step(plain)":                   "AAAAR" "AAAR" "AR",
        "ei_grad_batch":                    "AAAAR" "AAAR" "AR",
    },
    ("4x2", "per_sec"): {                   # OBS CAND HYP TIME FACTOR RESULTS (moments, durations)
        None:                               "AAAAA" "AAAR" "AR",
        "set_observations":                 F_NONE,
        "set_candidates":                   "RRRRR" "AAAR" "AR",
        "set_hypers":                       F_NONE,
        "set_time_model":                   F_NONE,
        "set_time_model(NULL)":             F_NONE,
        "set_option(covar, other)":         F_NONE,
        "set_option(covar, same)":          "AAAAA" "AAAR" "AR",
        "gp_logprob":                       F_NONE,
        "sobol_grid(as_candidates)":        "RRRRR" "AAAR" "AR",
        "set_partition":                    "AAAAA" "AAAR" "AR",
        "factor":                           "RRRRR" "AAAR" "AR",
        "set_fantasies(NULL)":              "AAAAA" "AAAR" "AR",
        "draw_fantasies(NULL)":             "AAAAA" "AAAR" "AR",
        "set_fantasies":                    "AAAAA" "AAAR" "AR",
        "draw_fantasies":                   "AAAAA" "AAAR" "AR",
        "ei_run(per_sec)":                  "AAAAA" "AAAR" "AR",
        "ei_step(per_sec)":                 "AAAAA" "AAAR" "AR",
        "ei_grad_batch":                    "AAAAA" "AAAR" "AR",
    },
}
FRONT_CASES = [(front, kind, writer) for (front, kind), rows in FRONT_TABLE.items() for writer in rows]
REFUSED_ON = {"4x2": ("set_fantasies", "draw_fantasies", "ei_grad_batch")}     # writers that the 2-D partition refuses
NP_PAIRWISE_MAX_N = 524288              # csrc/np_sum.h: the most draws spx_set_hypers takes


@pytest.fixture(scope="module")
def fronts():
    es = {"2": hh.engine(devices=[0, 0]), "4x2": hh.engine(devices=[0, 0, 0, 0], hyper_shards=2)}
    yield es
    for e in es.values():
        e.close()


def front_row(e, p):
    row = ""
    for name in FRONT_READERS:
        kind, res = hh.outcome(hh.FRONT_GETTERS.get(name) or hh.CALLS[name], e, p)
        assert kind in ("ok", "arg"), (name, kind, res)
        row += "A" if kind == "ok" else "R"
    return row


@pytest.mark.parametrize("front,kind,writer", FRONT_CASES, ids=["%s-%s-%s" % (f, k, w or "base") for f, k, w in FRONT_CASES])
def test_accept_refuse_table_of_the_front(fronts, prob, front, kind, writer):
    e = fronts[front]
    assert len(FRONT_TABLE[front, kind][writer]) == len(FRONT_READERS)
    hh.base(e, prob, kind)
    if writer is not None:
        wk, res = hh.outcome(hh.CALLS[writer], e, prob)
        assert wk == ("arg" if writer in REFUSED_ON.get(front, ()) else "ok"), (writer, wk, res)
    got = front_row(e, prob)
    print(front, kind, writer, got)
    assert got == FRONT_TABLE[front, kind][writer]


def raw(e, rc):
    """The outcome of a raw library call (one that the Engine's own wrapper would not pass on, or not without changing its
    Python-side shapes)."""
    return hh.outcome(e._check, rc)[0]


# calls that the front refuses from its own record, before any slot is asked: (name, fronts it is refused on, the call)
REFUSALS = [
    ("candidates of another D", ("2", "4x2"),
     lambda e, p: raw(e, e._lib.spx_set_candidates(e._h, hh._dp(np.zeros((5, hh.D + 1))), 5, hh.D + 1, 0))),
    ("fewer draws than draw shards", ("4x2",),
     lambda e, p: raw(e, e._lib.spx_set_hypers(e._h, hh._dp(np.ascontiguousarray(p.hypers[:1])), 1))),
    ("more draws than the mean over draws takes", ("2", "4x2"),
     lambda e, p: raw(e, e._lib.spx_set_hypers(e._h, hh._dp(np.zeros((NP_PAIRWISE_MAX_N + 1, 3 + hh.D))), NP_PAIRWISE_MAX_N + 1))),
    ("set_fantasies in the 2-D partition", ("4x2",), lambda e, p: hh.outcome(hh.CALLS["set_fantasies"], e, p)[0]),
    ("draw_fantasies in the 2-D partition", ("4x2",), lambda e, p: hh.outcome(hh.CALLS["draw_fantasies"], e, p)[0]),
]
REFUSAL_CASES = [(f, k, i) for i, r in enumerate(REFUSALS) for f in r[1] for k in ("plain", "per_sec")]


@pytest.mark.parametrize("front,kind,which", REFUSAL_CASES, ids=["%s-%s-%s" % (f, k, REFUSALS[i][0]) for f, k, i in REFUSAL_CASES])
def test_a_call_the_front_refuses_changes_nothing(fronts, prob, front, kind, which):
    e = fronts[front]
    hh.base(e, prob, kind)
    before = hh.read_all(e, prob, hh.FRONT_GETTERS)
    assert before["get_best"] and before["get_ei_draws"] and before["get_factor"] and before["get_cross_cov"]
    assert REFUSALS[which][2](e, prob) == "arg"
    assert hh.read_all(e, prob, hh.FRONT_GETTERS) == before             # the same bytes from every reader, results included
    assert front_row(e, prob) == FRONT_TABLE[front, kind][None]         # and the draws, the shards and the factor still run


def test_fewer_candidates_than_slots_leave_a_slot_idle(eng, prob):
    m = hh.engine(devices=[0, 0, 0])
    try:
        got = {}
        for e in (m, eng):
            hh.base(e, prob, "plain")
            e.set_candidates(prob.cand[:2])
            e.ei_run(hh.FLAGS["plain"])
            got[e is m] = hh.read_all(e, prob, hh.FRONT_GETTERS)
        assert front_row(m, prob) == FRONT_TABLE["2", "plain"][None]
        assert got[True] == got[False] and got[True]["get_best"] and got[True]["get_cross_cov"]    # the single handle's bits
    finally:
        m.close()
        eng.set_candidates(prob.cand)


# ---- the two clear forms that left results readable: each of these read them back before ---------------------------------------
RESULT_GETTERS = ["get_best", "get_ei_mean", "get_ei_draws", "get_moments"]


def test_results_are_dropped_by_clearing_the_time_model(eng, prob):
    hh.base(eng, prob, "per_sec")
    eng.set_time_model(None, None)
    for name in RESULT_GETTERS + ["get_time_mean"]:
        kind, res = hh.outcome(hh.GETTERS[name], eng, prob)
        assert kind == "arg", (name, kind)
    eng.ei_step(hh.FLAGS["plain"])                       # ... and the plain pass that follows is a fresh handle's
    got = hh.read_all(eng, prob)
    e2 = hh.engine()
    hh.reset(e2, prob)
    e2.ei_step(hh.FLAGS["plain"])
    want = hh.read_all(e2, prob)
    e2.close()
    assert got == want and got["get_time_mean"] is None


def test_results_are_dropped_by_clearing_the_constraint_model(eng, prob, fresh_bits):
    hh.base(eng, prob, "constrained")
    eng.set_constraint_model(None, None, None)
    for name in RESULT_GETTERS + ["get_constraint_prob"]:
        kind, res = hh.outcome(hh.GETTERS[name], eng, prob)
        assert kind == "arg", (name, kind)
    assert hh.outcome(hh.GETTERS["get_factor"], eng, prob)[0] == "ok"       # the objective's factor is untouched
    eng.ei_run(hh.FLAGS["plain"])                        # ... and the plain pass over that factor is a fresh handle's
    got = hh.read_all(eng, prob)
    assert got == fresh_bits and got["get_constraint_prob"] is None
