"""What a handle holds after each entry point (csrc/spx_held.h), seen from outside: every reader after every writer against a
literal table of accept / refuse, calls that fail without a fault, and the two clear forms that used to leave results
readable.  The tables are written from the "made from" table of DESIGN.md ("What a handle holds"), not taken from a run."""
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
