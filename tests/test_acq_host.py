"""The acquisitions beside EI and the model-mean recommendation on a CPU-only box: the oracle's gradients against central
differences, the C ABI's argument checks (spx_create touches no GPU), the choosers' acq= / acq_par= / recommend=
arguments, and recommend=1 against recommend=0 on the seeded Branin sequences the goldens cover."""
import os

import numpy as np
import numpy.random as npr
import pytest

from oracle import gp_ei_oracle as orc
from spearmint_amd import engine
from spearmint_amd.chooser import GPConstrainedEIChooser, GPEIChooser, GPEIOptChooser, GPEIperSecChooser
from tests import acq_oracle as ao
from tests import refine_helpers as rh
from tests.acq_helpers import AcqOracleEngine, AcqStandinEngine
from tests.constrained_refine_helpers import central_differences
from tests.helpers import branin


# ---- the oracle itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,par", [(ao.PI, 0.0), (ao.PI, 0.01), (ao.LCB, 0.0), (ao.LCB, 2.0)])
@pytest.mark.parametrize("branch", ["plain", "fant"])
@pytest.mark.parametrize("covar", rh.COVARS)
def test_oracle_gradient_is_half_the_central_difference_of_its_value(kind, par, branch, covar):
    """The objective is minus the acquisition summed over the draws; its gradient carries the reference's factor one half
    (tests/constrained_refine_helpers.central_differences has it too).  The EI oracle agrees with its own central
    differences to 1.5e-7 of max |g| (tests/test_gpu_m_refine_paths.py); the same bar here, with room: 1e-6."""
    p = rh.make_problem(7, covar=covar, branch=branch, N=30, D=3, H=2, S=4, n_pend=2)
    pts = rh.points(p, 3, n=4)
    f, g = ao.grad_oracle(p, pts, kind, par)
    for k, x in enumerate(pts):
        fd = central_differences(lambda y: ao.grad_oracle(p, y[None], kind, par)[0][0], x, range(p.D))
        assert np.allclose(fd, g[k], rtol=1e-6, atol=1e-6 * np.abs(g[k]).max()), (k, fd, g[k])
    assert np.all(np.isfinite(f))


def test_oracle_ei_terms_are_the_reference_ones():
    p = rh.make_problem(5, branch="plain", N=20, D=2, H=2)
    pts = rh.points(p, 1, n=3)
    f, g = ao.grad_oracle(p, pts, ao.EI, 0.0)
    f0, g0 = rh.oracle(p, pts)
    assert np.array_equal(f, f0) and np.array_equal(g, g0)


def test_oracle_values_and_nan_rule():
    m, v = np.array([0.3, -0.2, 0.1]), np.array([0.04, 0.09, -1e-9])
    pi = ao.value(ao.PI, 0.01, m, v, -0.1)
    lcb = ao.value(ao.LCB, 0.0, m, v, -0.1)
    assert np.isnan(pi[2]) and np.isnan(lcb[2])            # func_v < 0: NaN, kappa = 0 included
    assert np.allclose(lcb[:2], -m[:2]) and np.all((pi[:2] > 0) & (pi[:2] < 1))
    assert ao.choose(np.column_stack((lcb, lcb))) == 2      # first NaN wins


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------
def test_set_acquisition_argument_checks_touch_no_gpu():
    eng = engine.Engine(0)
    assert eng.get_acquisition() == (engine.ACQ_EI, 0.0)
    eng.set_acquisition(engine.ACQ_PI, 0.01)
    assert eng.get_acquisition() == (engine.ACQ_PI, 0.01)
    eng.set_acquisition("LCB", 2)
    assert eng.get_acquisition() == (engine.ACQ_LCB, 2.0)
    for kind, par in ((3, 0.0), (-1, 0.0), (engine.ACQ_PI, -1e-3), (engine.ACQ_LCB, float("inf")),
                      (engine.ACQ_LCB, float("nan")), (engine.ACQ_EI, 0.5)):
        with pytest.raises(ValueError) as ei:
            eng.set_acquisition(kind, par)
        assert "spx_set_acquisition" in str(ei.value)
        assert eng.get_acquisition() == (engine.ACQ_LCB, 2.0)      # a refused call changes nothing
    with pytest.raises(ValueError):
        eng.set_acquisition("UCB")
    eng.set_acquisition(engine.ACQ_EI)
    assert eng.get_acquisition() == (engine.ACQ_EI, 0.0)
    assert eng._lib.spx_get_acquisition(eng._h, None, None) == 0   # either output may be NULL
    eng.close()


def test_multi_handle_replicates_the_setting():
    eng = engine.MultiEngine([0, 0])       # (repeated ids: the host transport; creation touches no GPU)
    eng.set_acquisition(engine.ACQ_PI, 0.25)
    assert eng.get_acquisition() == (engine.ACQ_PI, 0.25)
    with pytest.raises(ValueError):
        eng.set_acquisition(engine.ACQ_EI, 1.0)
    assert eng.get_acquisition() == (engine.ACQ_PI, 0.25)
    eng.close()


# ---- chooser arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_accepts_acq_arguments(mod, tmp_path):
    ch = mod.init(str(tmp_path), "acq=PI,acq_par=0.01")
    assert (ch.acq, ch.acq_par) == ("PI", 0.01) and not ch.recommend
    eng = AcqStandinEngine()
    ch._apply_acquisition(eng)
    assert eng.acq_calls == [(engine.ACQ_PI, 0.01)]
    d = mod.init(str(tmp_path), "")
    assert (d.acq, d.acq_par) == ("EI", 0.0)
    eng = AcqStandinEngine()
    d._apply_acquisition(eng)
    assert eng.acq_calls == []                                     # EI: the handle's default is left alone
    assert mod.init(str(tmp_path), "acq=lcb,acq_par=2,recommend=1").acq == "LCB"


@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
@pytest.mark.parametrize("args", ["acq=UCB", "acq=PI,acq_par=-1", "acq=LCB,acq_par=inf", "acq=LCB,acq_par=nan",
                                  "acq=EI,acq_par=0.5", "acq=PI,acq_par=x"])
def test_chooser_refuses_bad_acq_arguments(mod, args, tmp_path):
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), args)
    assert "allowed" in str(ei.value)
    if args == "acq=UCB":
        assert "EI, PI, LCB" in str(ei.value)


@pytest.mark.parametrize("mod", [GPEIperSecChooser, GPConstrainedEIChooser])
def test_per_second_and_constrained_choosers_are_ei_only(mod, tmp_path):
    for args in ("acq=LCB", "acq=PI,acq_par=0.01", "recommend=1"):
        with pytest.raises(ValueError) as ei:
            mod.init(str(tmp_path), args)
        assert "allowed" in str(ei.value)
    assert mod.init(str(tmp_path), "acq=EI,recommend=0").acq == "EI"


# ---- recommend=1 ---------------------------------------------------------------------------------------------------------
def _sequence(mod, arg, d, grid, iters, seed):
    """tests/helpers.run_trajectory (a fresh chooser per proposal, restarted from its state pickle), keeping what each call
    left behind: the proposal, numpy's generator state, the chooser's last recommendation."""
    grid = np.array(grid, copy=True)
    values = np.zeros(grid.shape[0]) + np.nan
    durations = np.zeros(grid.shape[0]) + np.nan
    done = np.zeros(grid.shape[0], dtype=bool)
    out = []
    for it in range(iters):
        ch = mod.init(str(d), arg)
        eng = AcqOracleEngine()
        ch._eng = eng
        npr.seed(seed + it)
        complete = np.nonzero(done)[0]
        job = ch.next(grid, values, durations, np.nonzero(~done)[0], np.zeros(0, dtype=int), complete)
        state = npr.get_state()
        rec = None
        if ch.last_recommendation is not None:
            rec = dict(ch.last_recommendation)
            with orc.covar("Matern52"):      # the oracle's mean of means over the whole grid, with this call's hyper rows
                rows = ch.hyper_rows() if hasattr(ch, "hyper_rows") else eng._last_rows
                mom = ao.over_hypers(ao.LCB, 0.0, grid[complete], grid, values[complete], rows)
            rec["grid_mean"] = -np.mean(mom, axis=1)
            rec["engine_acq"] = eng.get_acquisition()
        if isinstance(job, tuple):
            pt = np.asarray(job[1], dtype=float).ravel()
            grid = np.vstack((grid, pt[None, :]))
            values, durations, done = np.append(values, np.nan), np.append(durations, np.nan), np.append(done, False)
            idx = grid.shape[0] - 1
        else:
            idx = int(job)
        out.append((idx, grid[idx].copy(), state, rec))
        values[idx] = branin(grid[idx, 0], grid[idx, 1])
        durations[idx] = 1.0
        done[idx] = True
        if mod is GPEIChooser and ch.D != -1:
            ch.__del__()
    return out


@pytest.mark.parametrize("tag,mod,arg,iters", [("g", GPEIChooser, "mcmc_iters=4", 8),
                                               ("o", GPEIOptChooser, "mcmc_iters=3,burnin=5,grid_subset=4,use_multiprocessing=0", 6)])
def test_recommend_changes_no_proposal_and_draws_no_random_numbers(golden_dir, tmp_path, tag, mod, arg, iters):
    g = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))
    seed = int(g[tag + "_seed"])
    runs = {}
    for r in (0, 1):
        d = tmp_path / ("r%d" % r)
        d.mkdir()
        runs[r] = _sequence(mod, arg + ",recommend=%d" % r, d, g["grid"], iters, seed)
    # the reference's own proposals (the golden), with and without the recommendation
    for r in (0, 1):
        assert [p[0] for p in runs[r]] == list(g[tag + "_idx"][:iters])
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a[1], b[1])
        assert a[2][0] == b[2][0] and np.array_equal(a[2][1], b[2][1]) and a[2][2:] == b[2][2:]     # numpy's generator state
        assert a[3] is None
    assert not os.path.exists(str(tmp_path / "r0" / "recommendation.txt"))         # recommend=0: nothing computed or written
    lines = open(str(tmp_path / "r1" / "recommendation.txt")).read().splitlines()
    recs = [p[3] for p in runs[1] if p[3] is not None]
    assert len(lines) == len(recs) == iters - 2                  # (the first two calls return before there is a GP)
    for line, rec in zip(lines, recs):
        f = [float(v) for v in line.split()]
        assert f[0] == rec["mean"] and f[1] == rec["std"] and int(f[2]) == rec["grid_index"] and np.array_equal(f[3:], rec["x"])
        assert rec["engine_acq"] == (engine.ACQ_EI, 0.0)         # the previous acquisition is back
        gm = rec["grid_mean"]
        assert rec["std"] > 0 and np.all((rec["x"] >= 0) & (rec["x"] <= 1))
        if mod is GPEIChooser:                                     # grid only: the grid minimiser of the mean of means
            assert rec["grid_index"] == int(np.argmin(gm)) and np.isclose(rec["mean"], gm.min(), rtol=1e-9, atol=1e-12)
        else:                                                      # refined: never worse than the grid's best
            assert rec["mean"] <= gm.min() + 1e-9 * abs(gm.min()) + 1e-12
            assert rec["grid_index"] == -1 or rec["grid_index"] == int(np.argmin(gm))


def test_recommend_keeps_a_non_ei_acquisition(tmp_path):
    """acq=PI with recommend=1: the recommendation pass runs LCB(0) and hands the handle back with PI set."""
    rs = np.random.RandomState(4)
    grid = rs.rand(60, 2)
    values = branin(grid[:, 0], grid[:, 1])
    ch = GPEIChooser.init(str(tmp_path), "mcmc_iters=2,acq=PI,acq_par=0.01,recommend=1")
    eng = AcqOracleEngine()
    ch._eng = eng
    npr.seed(1)
    job = ch.next(grid, values, values * 0, np.arange(8, 60), np.zeros(0, dtype=int), np.arange(8))
    assert isinstance(job, int)
    assert eng.get_acquisition() == (engine.ACQ_PI, 0.01)
    assert eng.acq_calls == [(engine.ACQ_PI, 0.01), (engine.ACQ_LCB, 0.0), (engine.ACQ_PI, 0.01)]
    assert 0 <= ch.last_recommendation["grid_index"] < 60


def test_non_ei_acquisition_with_host_refinement_is_refused_at_construction(tmp_path, monkeypatch):
    """gpu_refine=0, or SPX_REFINE_MIN_N keeping the first proposals on the host: the host refinement knows EI alone, and
    the combination is known when the chooser is made -- not after a sampler run and a grid pass."""
    for args in ("acq=PI,gpu_refine=0", "acq=LCB,acq_par=2,gpu_refine=0"):
        with pytest.raises(ValueError) as ei:
            GPEIOptChooser.init(str(tmp_path), args)
        assert "allowed" in str(ei.value) and "gpu_refine" in str(ei.value)
    assert GPEIOptChooser.init(str(tmp_path), "acq=EI,gpu_refine=0").acq == "EI"
    assert GPEIOptChooser.init(str(tmp_path), "acq=PI,gpu_refine=1").acq == "PI"
    assert GPEIChooser.init(str(tmp_path), "acq=PI,gpu_refine=0").acq == "PI"          # (grid only: nothing to refine)
    monkeypatch.setenv("SPX_REFINE_MIN_N", "8")
    with pytest.raises(ValueError):
        GPEIOptChooser.init(str(tmp_path), "acq=PI")
    assert GPEIOptChooser.init(str(tmp_path), "acq=EI").acq == "EI"


class NanRowsEngine(AcqOracleEngine):
    """scipy's solves refuse NaN inputs; the device returns NaN for a NaN candidate.  This engine does what the device
    does: the oracle on the finite rows, NaN values and moments on the others."""

    def ei_run(self, flags=0):
        cand = self.cand
        ok = np.all(np.isfinite(cand), axis=1)
        H = self.hypers.shape[0]
        full = np.full((cand.shape[0], H), np.nan)
        mom = [(np.full(cand.shape[0], np.nan), np.full(cand.shape[0], np.nan)) for _ in range(H)]
        if ok.any():
            self.cand = cand[ok]
            AcqOracleEngine.ei_run(self, flags)
            full[ok] = self._ei
            for h in range(H):
                mom[h][0][ok], mom[h][1][ok] = self._mom[h]
        self.cand, self._ei, self._mom = cand, full, mom


@pytest.mark.parametrize("mod,args", [(GPEIChooser, "mcmc_iters=2"), (GPEIOptChooser, "mcmc_iters=2,burnin=2,grid_subset=3")])
def test_recommendation_never_names_a_point_without_a_mean(mod, args, tmp_path):
    """A proposal follows numpy's argmax (first NaN wins); a recommendation is a point to use: NaN rows of the grid are
    neither refined nor recommended, and a grid without any mean gives no recommendation and no line."""
    rs = np.random.RandomState(6)
    grid = rs.rand(50, 2)
    values = branin(grid[:, 0], grid[:, 1])
    comp, vals = grid[:8], values[:8]
    bad = grid.copy()
    bad[[3, 20, 41], 0] = np.nan
    ch = mod.init(str(tmp_path), args + ",recommend=1")
    ch._eng = NanRowsEngine()
    rows = np.array([[0.1, 1e-3, 1.0, 0.7, 0.9], [0.0, 1e-2, 1.3, 1.1, 0.5]])
    rec = ch._recommend(bad, comp, vals, rows, refine_count=3 if mod is GPEIOptChooser else 0)
    assert rec is ch.last_recommendation and np.isfinite(rec["mean"]) and np.isfinite(rec["std"])
    assert rec["grid_index"] not in (3, 20, 41) and np.all(np.isfinite(rec["x"]))
    clean = ch._recommend(np.delete(bad, [3, 20, 41], axis=0), comp, vals, rows, refine_count=3 if mod is GPEIOptChooser else 0)
    assert clean["mean"] == rec["mean"] and np.array_equal(clean["x"], rec["x"])      # the NaN rows changed nothing
    assert len(open(ch.recommendation_file).read().splitlines()) == 2
    assert ch._recommend(np.full((5, 2), np.nan), comp, vals, rows) is None and ch.last_recommendation is None
    assert len(open(ch.recommendation_file).read().splitlines()) == 2
    assert not os.path.exists(ch.recommendation_file + ".lock")
