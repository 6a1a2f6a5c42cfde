"""Shared by tests/test_gpu_t_held.py and scripts/dev/held_equiv.py: one small problem that still reaches every buffer of a
handle, every entry point as a named call on it, and every reader as (accepted, what it served).

Shapes: N = 70 observations (two 64-blocks on the log-likelihood path, one 128-row tile on the EI path), M = 130 candidates
(two tiles), H = 2 draws, D = 2, S = 2 fantasies of P = 1 pending row (the last observation), 9 constraint points."""
import ctypes
import hashlib

import numpy as np

from spearmint_amd import sobol
from spearmint_amd.engine import (FLAG_CONSTRAINED, FLAG_KEEP_MOMENTS, FLAG_PER_SEC, FLAG_TIME_ONLY, Engine, LinAlgError, MultiEngine,
                                  SpxError, _dp)
from spearmint_amd.synthetic import synthetic_problem

N, M, H, D, S, P, NC = 70, 130, 2, 2, 2, 1, 9
KEEP = FLAG_KEEP_MOMENTS
FLAGS = {"plain": KEEP, "per_sec": FLAG_PER_SEC | KEEP, "constrained": FLAG_CONSTRAINED | KEEP,
         "time_only": FLAG_PER_SEC | KEEP | FLAG_TIME_ONLY, "bare": 0}


class Problem(object):
    def __init__(self, seed=11):
        self.comp, self.cand, self.vals, self.hypers, self.log_durs, self.th = synthetic_problem(N, M, D, H, seed, per_sec=True)
        rs = np.random.RandomState(seed + 1)
        self.comp_c = rs.rand(NC, D)
        self.ff = rs.randn(NC) * 1.5
        self.crows = np.column_stack((rs.uniform(0.5, 3.0, H), np.full(H, 1e-3), rs.uniform(0.5, 2.0, H), rs.uniform(0.3, 1.5, (H, D))))
        self.z = rs.randn(P, S)
        self.fant = rs.randn(H, N, S)
        self.bests = np.min(self.fant, axis=1) - 0.1
        self.pts = rs.rand(3, D)
        self.bad_hypers = self.hypers.copy()
        self.bad_hypers[1, 2] = -1.0                   # a negative amplitude in draw 1: its K(X,X) fails at the first pivot
        self.dirs = sobol.load_dirs("jk1111")


def engine(lib=None, devices=None, hyper_shards=1):
    """An Engine whose Python-side shapes are this problem's from the start (its wrappers check them before they call).
    devices: the front of a multi-device handle over these device ids instead, its slots in `hyper_shards` draw shards
    (spx_set_partition; "set_partition" of CALLS and reset() ask for the same count again: nothing changes)."""
    e = Engine(0, lib=lib) if devices is None else MultiEngine(devices, lib=lib)
    e.N, e.D, e.M, e.H = N, D, M, H
    e.hyper_shards = hyper_shards
    if hyper_shards != 1:
        e.set_partition(hyper_shards)
    return e


def front_calls():
    """CALLS without what a multi-device handle refuses outright: the constraint model and its passes."""
    return {k: f for k, f in CALLS.items() if "constrain" not in k}


def outcome(fn, *args):
    """("ok", result) or (class of the refusal, the library's text)."""
    try:
        return "ok", fn(*args)
    except LinAlgError as ex:
        return "not_pd", str(ex)
    except ValueError as ex:
        return "arg", str(ex)
    except SpxError as ex:
        return "hip", str(ex)


def _pending(e):
    # (not Engine.get_pending_fantasies: that asks the handle's statistics for the sizes first and refuses by itself)
    pf, b = np.empty((P, S)), np.empty(S)
    e._check(e._lib.spx_get_pending_fantasies(e._h, 0, _dp(pf), _dp(b)))
    return pf, b


# the getters: they change nothing
GETTERS = {
    "get_best": lambda e, p: np.array(e.best(), dtype=np.float64),
    "get_ei_mean": lambda e, p: e.ei_mean(),
    "get_ei_draws": lambda e, p: e.ei_draws(),
    "get_moments": lambda e, p: np.concatenate(e.get_moments(H - 1)),
    "get_time_mean": lambda e, p: e.get_time_mean(H - 1),
    "get_constraint_prob": lambda e, p: e.get_constraint_prob(H - 1),
    "get_factor": lambda e, p: np.concatenate([a.ravel() for a in e.get_factor(H - 1)]),
    "get_factor_rows": lambda e, p: np.concatenate([a.ravel() for a in e.get_factor_rows(0, N - 3, 3)]),
    "get_pending_fantasies": lambda e, p: np.concatenate([a.ravel() for a in _pending(e)]),
}

# ... of a multi-device handle: no constraint model; K(X*,X) of the first candidates (needs the factor AND candidates)
FRONT_GETTERS = {k: f for k, f in GETTERS.items() if k != "get_constraint_prob"}
FRONT_GETTERS["get_cross_cov"] = lambda e, p: e.get_cross_cov(H - 1, 0, min(5, e.M))

# every entry point that writes, under the name the tables and the walks use
CALLS = {
    "set_observations": lambda e, p: e.set_observations(p.comp, p.vals),
    "set_candidates": lambda e, p: e.set_candidates(p.cand),
    "set_hypers": lambda e, p: e.set_hypers(p.hypers),
    "set_hypers(not PD)": lambda e, p: e.set_hypers(p.bad_hypers),
    "set_time_model": lambda e, p: e.set_time_model(p.log_durs, p.th),
    "set_time_model(NULL)": lambda e, p: e.set_time_model(None, None),
    "set_constraint_model": lambda e, p: e.set_constraint_model(p.comp_c, p.ff, p.crows),
    "set_constraint_model(NULL)": lambda e, p: e.set_constraint_model(None, None, None),
    "set_option(covar, other)": lambda e, p: e.set_covar("Matern32"),
    "set_option(covar, same)": lambda e, p: e.set_covar("Matern52"),
    "gp_logprob": lambda e, p: e.gp_logprob(),
    "sobol_grid(as_candidates)": lambda e, p: e.sobol_grid(p.dirs, D, M, 1, fetch=False, as_candidates=True)[0],
    "set_partition": lambda e, p: e.set_partition(e.hyper_shards, 0, 0),
    "factor": lambda e, p: e.factor(),
    "set_fantasies": lambda e, p: e.set_fantasies(p.fant, p.bests),
    "set_fantasies(NULL)": lambda e, p: e.set_fantasies(None, None),
    "draw_fantasies": lambda e, p: e.draw_fantasies(p.z, P),
    "draw_fantasies(NULL)": lambda e, p: e.draw_fantasies(None, 0),
    "ei_grad_batch": lambda e, p: np.concatenate([a.ravel() for a in e.ei_grad_batch(p.pts)]),
    "constrained_ei_grad_batch": lambda e, p: np.concatenate([a.ravel() for a in e.constrained_ei_grad_batch(p.pts, float(np.min(p.vals)))]),
}
for _k, _f in FLAGS.items():
    CALLS["ei_run(%s)" % _k] = lambda e, p, _f=_f: e.ei_run(_f)
    CALLS["ei_step(%s)" % _k] = lambda e, p, _f=_f: e.ei_step(_f)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()[:12]


def read_all(e, p, getters=GETTERS):
    """{getter: None where it refused, else the SHA-256 of what it served}."""
    out = {}
    for name, fn in getters.items():
        kind, res = outcome(fn, e, p)
        out[name] = sha(res) if kind == "ok" else None
    return out


def reset(e, p):
    """Back to a handle that holds this problem's observations, candidates and hypers and nothing made from them."""
    e.set_covar("Matern52")
    e.set_partition(e.hyper_shards, 0, 0)
    e.set_observations(p.comp, p.vals)
    e.set_candidates(p.cand)
    e.set_hypers(p.hypers)
    e.set_time_model(None, None)
    if not isinstance(e, MultiEngine):
        e.set_constraint_model(None, None, None)


def base(e, p, kind):
    """One of the three base handles: "plain" (device fantasies, a pass with kept moments), "per_sec" (kept moments),
    "constrained" (kept moments, then one spx_constrained_ei_grad_batch: the full handle is factored)."""
    reset(e, p)
    if kind == "plain":
        e.factor()
        if e.hyper_shards == 1:                        # (the 2-D partition of a multi-device handle takes no fantasies)
            e.draw_fantasies(p.z, P)
        e.ei_run(FLAGS["plain"])
    elif kind == "per_sec":
        e.set_time_model(p.log_durs, p.th)
        e.ei_step(FLAGS["per_sec"])
    else:
        e.set_constraint_model(p.comp_c, p.ff, p.crows)
        e.ei_step(FLAGS["constrained"])
        CALLS["constrained_ei_grad_batch"](e, p)


def not_pd_info(e):
    d, pv = ctypes.c_int32(-9), ctypes.c_int32(-9)
    e._check(e._lib.spx_not_pd_info(e._h, ctypes.byref(d), ctypes.byref(pv)))
    return int(d.value), int(pv.value)
