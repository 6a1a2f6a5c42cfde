"""Shared by the tests of the per-second branch of the grid pass (spx_set_time_model, SPX_FLAG_PER_SEC, SPX_FLAG_TIME_ONLY,
spx_get_time_mean): seeded problems (spearmint_amd.synthetic.synthetic_problem with per_sec=True), the handle taken through
that branch, everything a pass leaves behind collected for a bit-for-bit comparison, and the float64 oracle
(oracle/gp_ei_oracle.ei_per_s_over_hypers, tests/helpers.OracleEngine.get_time_mean).  No GPU is needed to import it."""
import functools

import numpy as np

from oracle import gp_ei_oracle as orc
from spearmint_amd.synthetic import synthetic_problem
from tests import helpers

PER_SEC, KEEP_MOMENTS, TIME_ONLY = 1, 2, 8
KEEP = PER_SEC | KEEP_MOMENTS


@functools.lru_cache(maxsize=None)
def problem(N, M, D, H, seed):
    """(comp, cand, vals, hypers, log_durs, time_hypers); the two models differ in every entry of every draw."""
    p = synthetic_problem(N, M, D, H, seed, near=min(10, M), per_sec=True)
    assert np.all(p[3] != p[5])
    return p


def load(eng, prob, covar="Matern52"):
    comp, cand, vals, hypers, log_durs, th = prob
    eng.set_covar(covar)
    eng.set_observations(comp, vals)
    eng.set_candidates(cand)
    eng.set_hypers(hypers)
    eng.set_time_model(log_durs, th)


def collect(eng, flags=KEEP):
    """What the pass left: per-draw values, their mean, the winner and its value; with the moments kept func_m / func_v and
    the predicted durations of every draw.  A time-only pass leaves the durations alone."""
    out = {}
    if not flags & TIME_ONLY:
        out.update(draws=eng.ei_draws(), mean=eng.ei_mean(), best=eng.best())
    if flags & KEEP_MOMENTS:
        if not flags & TIME_ONLY:
            mv = [eng.get_moments(h) for h in range(eng.H)]
            out["func_m"] = np.stack([m for m, _ in mv], axis=1)
            out["func_v"] = np.stack([v for _, v in mv], axis=1)
        if flags & PER_SEC:
            out["tmean"] = np.stack([eng.get_time_mean(h) for h in range(eng.H)], axis=1)
    return out


def step(eng, flags=KEEP):
    eng.ei_step(flags)
    return collect(eng, flags)


def factor_run(eng, flags=KEEP):
    eng.factor()
    eng.ei_run(flags)
    return collect(eng, flags)


def assert_same(a, b, what=""):
    """Bit for bit (a NaN equal to a NaN) in everything both hold; the winner and its value."""
    for k in ("draws", "mean", "func_m", "func_v", "tmean"):
        if k in a and k in b:
            assert a[k].shape == b[k].shape, (what, k)
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, int(np.sum(a[k] != b[k])))
    if "best" in a and "best" in b:
        assert a["best"][0] == b["best"][0], (what, a["best"], b["best"])
        assert a["best"][1] == b["best"][1] or (np.isnan(a["best"][1]) and np.isnan(b["best"][1])), what


def scramble(eng, prob):
    """ANOTHER problem of ANOTHER padded size through the default path, so that every buffer the next pass should write holds
    wrong values (and the two streams a finished pass of other launch counts): a variant that skips a store or a wait cannot
    pass on what the run before it left behind.  The caller loads its own problem again."""
    comp, cand, vals, hypers, log_durs, th = prob
    N, D = comp.shape
    other = problem(N + 130, cand.shape[0] // 2 + 77, D, hypers.shape[0], 9000 + N)
    load(eng, other)
    eng.ei_step(KEEP)


@functools.lru_cache(maxsize=None)
def oracle(N, M, D, H, seed, covar="Matern52"):
    """(overall_ei[M, H], func_time_m[M, H]) of problem(...) from the float64 oracle."""
    comp, cand, vals, hypers, log_durs, th = problem(N, M, D, H, seed)
    return oracle_of((comp, cand, vals, hypers, log_durs, th), covar)


def oracle_of(prob, covar="Matern52"):
    comp, cand, vals, hypers, log_durs, th = prob
    with orc.covar(covar), np.errstate(all="ignore"):
        ei = orc.ei_per_s_over_hypers(comp, cand, vals, log_durs, hypers, th)
    return ei, oracle_time_mean(prob, covar)


def oracle_time_mean(prob, covar="Matern52"):
    comp, cand, vals, hypers, log_durs, th = prob
    o = helpers.OracleEngine(covar)
    o.set_observations(comp, vals)
    o.set_candidates(cand)
    o.set_hypers(hypers)
    o.set_time_model(log_durs, th)
    with np.errstate(all="ignore"):
        return np.stack([o.get_time_mean(h) for h in range(th.shape[0])], axis=1)


def oracle_plain(prob, covar="Matern52"):
    comp, cand, vals, hypers, log_durs, th = prob
    with orc.covar(covar), np.errstate(all="ignore"):
        return orc.ei_over_hypers(comp, cand, vals, hypers)


def fresh(fn, *args, **kw):
    """fn(engine, ...) on a new engine."""
    from spearmint_amd.engine import Engine
    e = Engine(0)
    try:
        return fn(e, *args, **kw)
    finally:
        e.close()


def fresh_step(prob, flags=KEEP, covar="Matern52"):
    def run(e):
        load(e, prob, covar)
        return step(e, flags)
    return fresh(run)
