"""What plan_factor / plan_ei (csrc/spx_plan.h) say will run is what runs: for the shapes of tests/test_plan.py that sit on
either side of a decision below N = 300 (and M <= 2000), the call is made and the library's statistics -- and, with option
timing, the per-stage launch counts of the factorisation -- are compared with the plan that tests/c/plan_client.cpp prints for
the same shape and options.  The plans of all cases come from one run of the client."""
import numpy as np
import pytest

from spearmint_amd.engine import FLAG_KEEP_MOMENTS, FLAG_PER_SEC, FLAG_TIME_ONLY, Engine
from spearmint_amd.synthetic import synthetic_problem
from tests import plan_helpers as ph

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")]

OPTION_DEFAULTS = {"streams": 1, "timing": 0, "kstar_ring": 0, "kstar_budget_bytes": 0}      # every other one: -1

# spx_gp_logprob: (N, H, D, options)
LOGPROB = [(17, 1, 2, {}), (65, 1, 2, {}), (130, 32, 2, {}), (130, 33, 2, {}),
           (17, 1, 64, {}), (17, 1, 65, {}),                                       # Dp = 64 / 96: fused / not
           (300, 21, 2, {}), (300, 22, 2, {}), (300, 22, 2, {"lean_zc": 1}),      # zero-copy on / off / asked for
           (130, 3, 2, {"lean_one": 0}), (130, 3, 2, {"lean_one": 0, "lean_merge": 0}), (130, 3, 2, {"lean_flow_cov": 0}),
           (130, 3, 2, {"lean_flow": 0}), (130, 3, 2, {"lean_flow": 0, "lean_ps": 0}), (130, 3, 2, {"lean_flow": 0, "lean_lazy": 1})]
# an EI pass: (N, M, H, kind, options); the 1 MiB staging buffer gives two chunks of one draw per item at N = 130
SMALL = {"kstar_budget_bytes": 1 << 20}
RING = dict(SMALL, streams=3)
EI = [(130, 1000, 3, "plain", SMALL), (130, 1000, 3, "plain", RING), (130, 1000, 3, "plain", dict(RING, kstar_ring=2)),
      (130, 1000, 3, "plain", dict(RING, timing=1)), (130, 1000, 3, "time_only", RING), (130, 1000, 3, "fantasies", SMALL),
      (130, 1000, 3, "plain", dict(SMALL, ei_flow=0)),
      (129, 1000, 3, "plain", {}), (129, 1000, 3, "plain", {"gemm_partial": 0}),
      (128, 1000, 3, "plain", {}), (128, 1000, 3, "plain", {"ei_fused": 0})]
EI_FLAGS = {"plain": 0, "fantasies": 0, "time_only": FLAG_PER_SEC | FLAG_KEEP_MOMENTS | FLAG_TIME_ONLY}
S_FANT = 3


def _ident(case):
    return "-".join(str(c) if not isinstance(c, dict) else "_".join("%s%d" % kv for kv in sorted(c.items())) or "defaults" for c in case)


@pytest.fixture(scope="module")
def plans():
    """{(case, timing, step): plan(s)}: every plan of the module from ONE run of the client."""
    keys, cases = [], []
    for c in LOGPROB:
        N, H, D, opts = c
        for timing in (0, 1):
            keys.append(("lp", _ident(c), timing))
            cases.append(("factor", dict(opts, N=N, H=H, D=D, lean=1, defer=1, dest=1, timing=timing)))
    for c in EI:
        N, M, H, kind, opts = c
        time = int(kind == "time_only")
        for step in (0, 1):
            # a step keeps the two-call form with option timing (its stage timers bracket each call) and with fantasies
            # (they are set between the calls)
            pending = int(step and not opts.get("timing") and kind != "fantasies")
            keys.append(("fac", _ident(c), step))
            cases.append(("factor", dict(opts, N=N, H=H, D=2, time=time, defer=pending)))
            keys.append(("ei", _ident(c), step))
            # the budgets the library reads off the device's free memory: at least the 64 MiB floor for the fantasies' partial
            # means, and far more than the six 1 MiB slots a whole pass of these shapes has items for the ring
            cases.append(("ei", dict(opts, N=N, M=M, H=H, D=2, S=S_FANT if kind == "fantasies" else 0, nmodels=1 + time,
                                     flags=EI_FLAGS[kind], pending=pending, fant_budget=64 << 20, ring_budget=6 << 20)))
    return dict(zip(keys, ph.plans(cases)))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _set(e, opts):
    for k, v in opts.items():
        e.set_option(k, v)


def _reset(e, opts):
    for k in opts:
        e.set_option(k, OPTION_DEFAULTS.get(k, -1))


def _factor_counts(p, lean):
    """Launches per stage of one factorisation, read off its plan (do_factor's TIMED launches)."""
    nblk = p["nblk"]
    if lean:
        scale = (0 if p["merged_prologue"] else 1) + (1 if p["rl"] and p["merged_prologue"] and not p["fused"] else 0)
        panel = 0 if p["flow"] or p["ps"] else nblk            # k_lean_trsm, or k_chol_panel with right-hand-side rows: every column
    else:
        scale = 1
        panel = 0 if p["flow"] else nblk - 1                  # k_chol_panel: nothing below the last diagonal block
    return {"scale_rows": scale, "cov_self": 0 if p["cov_in_flow"] else 1, "chol_diag": 1 if p["flow"] else nblk,
            "chol_panel": panel}


def _factor_stats(e):
    return {k: e.stat("last_" + k) for k in ("factor_flow", "factor_cov_in_flow", "logprob_one_launch")}


def _plan_stats(p):
    return {"factor_flow": p["flow"], "factor_cov_in_flow": p["cov_in_flow"], "logprob_one_launch": p["fused"]}


@pytest.mark.parametrize("timing", (0, 1))
@pytest.mark.parametrize("case", LOGPROB, ids=_ident)
def test_logprob_runs_its_plan(eng, plans, case, timing):
    N, H, D, opts = case
    p = plans[("lp", _ident(case), timing)]
    comp, _, vals, hypers = synthetic_problem(N, 16, D, H, 11)
    eng.set_observations(comp, vals)
    eng.set_hypers(hypers)
    _set(eng, dict(opts, timing=timing))          # ("timing" restarts the accumulators)
    try:
        lp = eng.gp_logprob()
        got, counts = _factor_stats(eng), eng.timings()
    finally:
        _reset(eng, dict(opts, timing=0))
    assert np.all(np.isfinite(lp))
    print(case, timing, got, {k: counts[k][1] for k in ("scale_rows", "cov_self", "chol_diag", "chol_panel")})
    assert got == _plan_stats(p)
    if timing:
        assert {k: counts[k][1] for k in ("scale_rows", "cov_self", "chol_diag", "chol_panel")} == _factor_counts(p, True)


@pytest.mark.parametrize("step", (0, 1))
@pytest.mark.parametrize("case", EI, ids=_ident)
def test_ei_pass_runs_its_plan(eng, plans, case, step):
    N, M, H, kind, opts = case
    pf, pe = plans[("fac", _ident(case), step)], plans[("ei", _ident(case), step)]
    comp, cand, vals, hypers, log_durs, th = synthetic_problem(N, M, 2, H, 12, per_sec=True)
    eng.set_observations(comp, vals)
    eng.set_candidates(cand)
    eng.set_hypers(hypers)
    eng.set_time_model(log_durs, th) if kind == "time_only" else eng.set_time_model(None, None)
    _set(eng, opts)
    counts = None
    try:
        if step and kind != "fantasies":
            eng.ei_step(EI_FLAGS[kind])
        else:
            eng.factor()
            if opts.get("timing"):
                counts = {k: v[1] for k, v in eng.timings().items()}
            if kind == "fantasies":
                rs = np.random.RandomState(5)
                fant = rs.randn(H, N, S_FANT)
                eng.set_fantasies(fant, np.min(fant, axis=1) - 0.1)
            eng.ei_run(EI_FLAGS[kind])
        got = dict(_factor_stats(eng), step_fused=eng.stat("last_step_fused"),
                   step_skipped_padding=eng.stat("last_step_skipped_padding"), kstar_ring=eng.stat("last_kstar_ring"))
    finally:
        eng.set_fantasies(None, None)
        _reset(eng, opts)
    print(case, step, got, counts)
    assert got == dict(_plan_stats(pf), step_fused=pe["fused"], step_skipped_padding=int(pe["gemm_nlive"] > 0), kstar_ring=pe["R"])
    if counts is not None:
        assert {k: counts[k] for k in ("scale_rows", "cov_self", "chol_diag", "chol_panel")} == _factor_counts(pf, False)
