"""Shared by the tests of the pending branch of the grid pass (spx_set_fantasies followed by spx_ei_run): seeded problems
(tests/refine_helpers.make_problem with branch="fant"), the handle taken through that branch, its float64 oracle
(oracle/gp_ei_oracle.compute_ei_fantasies, one draw at a time) and host restatements of the two plans the pass makes
(predict_gemm_padding_plan of csrc/predict_kernels.hip; plan_chunks lives in tests/test_gpu_k_constrained_paths.py).
No GPU is needed to import it: tests/test_pending_mp.py uses the oracle side on the CPU."""
import contextlib
import functools

import numpy as np
import scipy.linalg as spla

from oracle import gp_ei_oracle as orc
from tests import constrained_refine_helpers as hp
from tests import refine_helpers as rh
from tests import refine_mp as rm

FLAG_PER_SEC, FLAG_KEEP_MOMENTS, FLAG_TIME_ONLY = 1, 2, 8
OPTION_DEFAULTS = {"kstar_budget_bytes": 0, "streams": 1, "step_overlap": -1, "ei_fused": -1, "gemm_partial": -1,
                   "timing": 0, "cov_flat": -1, "ei_flow": -1, "stage_copies": -1, "gemm_waves": 0,
                   "kstar_corun": -1, "lean_flow_cov": -1, "lean_one": -1}


@contextlib.contextmanager
def options(eng, **kw):
    try:
        for k, v in kw.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in kw:
            eng.set_option(k, OPTION_DEFAULTS[k])


def padding_plan(n_rows):
    """predict_gemm_padding_plan of csrc/predict_kernels.hip for the production GEMM: (live 16-row tiles of the last row
    block, whether the pass skips the padding).  It skips with 1 .. 6 live tiles where that saves at least 12 %."""
    Np = (n_rows + 127) // 128 * 128
    nlive, nrb = (n_rows + 15) // 16, Np // 128
    lt = nlive - 8 * (nrb - 1)
    return lt, bool(1 <= lt <= 6 and 25 * (8 - lt) >= 12 * (nrb + 1))


@functools.lru_cache(maxsize=64)
def problem(seed, covar="Matern52", N=150, D=3, H=3, S=5, n_pend=3):
    """N rows resident = N - n_pend observations + n_pend pending points, S fantasy columns per draw."""
    return rh.make_problem(seed, covar, "fant", N=N, D=D, H=H, S=S, n_pend=n_pend)


def candidates(p, seed, M):
    return np.random.RandomState(seed).rand(M, p.D)


def padded_vals(p):
    return np.concatenate((p.vals, np.zeros(p.pend.shape[0])))


def log_durs(p, seed=5):
    """Log durations of ALL resident rows (pending points included): what a time model over the same rows needs."""
    rs = np.random.RandomState(seed)
    return 0.7 * np.sum(p.X, axis=1) / p.D + 0.1 * rs.randn(p.X.shape[0])


def load(eng, p, cand, time_model=False):
    eng.set_covar(p.covar)
    eng.set_observations(p.X, padded_vals(p))
    eng.set_candidates(cand)
    eng.set_hypers(p.rows)
    if time_model:
        eng.set_time_model(log_durs(p), p.trows)


def collect(eng):
    return {"draws": eng.ei_draws(), "mean": eng.ei_mean(), "best": eng.best()}


def fant_pass(eng, p, cand, flags=0, entry="factor", time_model=False):
    """Everything from the observations on: resident data, factorisation (spx_factor, or a whole spx_ei_step as the
    choosers' first pass is), fantasies, spx_ei_run."""
    load(eng, p, cand, time_model)
    if entry == "step":
        eng.ei_step(0)
    else:
        eng.factor()
    eng.set_fantasies(p.fant, p.bests)
    eng.ei_run(flags)
    return collect(eng)


def plain_pass(eng, p, cand, flags=0, time_model=False):
    """The pass over the same resident rows without fantasies (what clearing or dropping them must give back)."""
    load(eng, p, cand, time_model)
    eng.factor()
    eng.ei_run(flags)
    return collect(eng)


def fresh(fn, *args, **kw):
    """fn(engine, ...) on a new engine."""
    from spearmint_amd.engine import Engine
    e = Engine(0)
    try:
        return fn(e, *args, **kw)
    finally:
        e.close()


def scramble(eng, p, cand):
    """ANOTHER problem of the same sizes through the default path, so that every buffer the next pass should write holds
    wrong values of the right shape: a variant that skips a store cannot pass on what the run before it left behind."""
    q = hp.Problem()
    q.__dict__.update(p.__dict__)
    q.rows = p.rows[::-1].copy()
    q.rows[:, 2] *= 1.3
    q.fant = 0.9 * p.fant[::-1, :, ::-1] + 0.05
    q.bests = np.min(q.fant, axis=1)
    fant_pass(eng, q, cand[::-1].copy())


def oracle(p, cand):
    """overall_ei[M, H] of the pending branch for the problem's own fantasy columns."""
    out = np.empty((cand.shape[0], p.H))
    with orc.covar(p.covar):
        for h in range(p.H):
            out[:, h] = orc.compute_ei_fantasies(p.X, cand, p.rows[h], p.fant[h], p.bests[h])
    return out


def oracle_plain(p, cand):
    with orc.covar(p.covar):
        return orc.ei_over_hypers(p.X, cand, padded_vals(p), p.rows)


def oracle_time_mean(p, cand, h):
    """exp(predicted log duration) under time draw h over the resident rows, as orc.compute_ei_per_s forms it."""
    with orc.covar(p.covar):
        t_mean, t_noise, t_amp2, t_ls = orc.unpack_hyper(p.trows[h])
        chol = spla.cholesky(orc.cov(t_amp2, t_ls, p.X) + t_noise * np.eye(p.X.shape[0]), lower=True)
        t_alpha = spla.cho_solve((chol, True), log_durs(p) - t_mean)
        return np.exp(np.dot(orc.cov(t_amp2, t_ls, p.X, cand).T, t_alpha) + t_mean)


def with_columns(p, s0, s1):
    """The same problem with the fantasy columns [s0, s1) alone."""
    q = hp.Problem()
    q.__dict__.update(p.__dict__)
    q.fant, q.bests, q.S = np.ascontiguousarray(p.fant[:, :, s0:s1]), np.ascontiguousarray(p.bests[:, s0:s1]), s1 - s0
    return q


# ---- the 50-digit fixture as a reference of the GRID pass ------------------------------------------------------------------
def tail_oracle(q, pts):
    """The float64 oracle of the grid pass for one draw of the tail problem (tests/refine_mp.tail_problem): EI[P]."""
    with orc.covar(q.covar), np.errstate(all="ignore"):
        if q.branch == "fant":
            return orc.compute_ei_fantasies(q.X, pts, q.rows[0], q.fant[0], q.bests[0])
        if q.branch == "persec":
            return orc.compute_ei_per_s(q.comp, pts, q.vals, q.log_durs, q.rows[0], q.trows[0])
        return orc.compute_ei(q.comp, pts, q.vals, q.rows[0])


def value_band_errors(ei, ei_ref, log10f):
    """Max relative error per band of log10 |f_ref| (tests/refine_mp.TAIL_BANDS; None: empty band)."""
    idx = rm.band_of(log10f)
    out = []
    for i in range(len(rm.TAIL_BANDS)):
        sel = idx == i
        out.append(float(np.max(np.abs(ei[sel] - ei_ref[sel]) / np.abs(ei_ref[sel]))) if sel.any() else None)
    return out
