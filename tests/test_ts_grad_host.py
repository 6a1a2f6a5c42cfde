"""The gradient of a sample path without a GPU (include/spx.h: spx_thompson_grad_batch): sin2pi of csrc/ts_device.h on the host
against 50 digits, the oracle of the path's value and gradient (tests/ts_grad_oracle.py) against tests/ts_oracle.py and central
differences, the binding's refusals, and GPEIOptChooser's ts_refine=1 on a stand-in engine."""
import os

import numpy as np
import pytest

from spearmint_amd import engine, refine
from spearmint_amd.chooser import GPConstrainedEIChooser, GPEIChooser, GPEIOptChooser, GPEIperSecChooser, GPParetoChooser
from tests import plan_helpers as ph
from tests import ts_grad_mp, ts_grad_oracle as tgo, ts_oracle as tso
from tests.helpers import branin
from tests.mes_helpers import same_state
from tests.ts_grad_helpers import TsGradOracleEngine, sin2pi_on_host

COVARS = ("Matern52", "Matern32", "ARDSE", "SE")


# ---- sin2pi of csrc/ts_device.h on the host -----------------------------------------------------------------------------------
@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_device_header_against_50_digits():
    """The header's own text compiled for the host against the 50-digit table -- a dense sweep of [-1/2, 1/2], both sides of
    +-1/4 where the minimum switches, +-1/2, +-0, every power of two down to the smallest sub-normal -- at the budget the header
    derives: SPX_TS_SIN_ULPS = 4 ulp of the result, and ONE quantum where the result is sub-normal.
    Measured here: 2.635 ulp (at r = 0.25004837410042796); every sub-normal result is the correctly rounded one (the table's
    low word cannot hold a fraction of a quantum, so an error there is counted in whole quanta)."""
    fx = np.load(ts_grad_mp.FIXTURE)
    r, hi, lo = fx["r"], fx["hi"], fx["lo"]
    got = sin2pi_on_host(r)
    e = ts_grad_mp.ulp_errors(got, hi, lo)
    i = int(np.argmax(e))
    sub = np.abs(hi) < ts_grad_mp.TINY
    print("sin2pi on the host: worst %.3f ulp at r = %r over %d points; sub-normal results: worst %.3f quantum over %d"
          % (e[i], float(r[i]), len(e), float(np.max(e[sub])), int(np.sum(sub))))
    assert len(r) > 9000 and np.sum(sub) > 50 and np.sum(np.abs(np.abs(r) - 0.25) < 1e-15) >= 18
    assert tgo.SIN_ULPS == 4 and e[i] <= tgo.SIN_ULPS
    assert np.max(e[sub]) <= 1.0
    # the sign is r's everywhere, the zeros included: sin2pi(+-0) = +-0, sin2pi(+-1/2) = +-0
    assert np.array_equal(np.signbit(got), np.signbit(r))
    for z in (0.0, -0.0, 0.5, -0.5):
        v = sin2pi_on_host([z])[0]
        assert v == 0.0 and np.signbit(v) == np.signbit(z)
    assert abs(sin2pi_on_host([0.25])[0] - 1.0) <= 2.0 ** -52 and sin2pi_on_host([-0.25])[0] == -sin2pi_on_host([0.25])[0]
    assert np.isnan(sin2pi_on_host([np.nan])[0])


def test_fixture_is_what_mpmath_gives():
    pytest.importorskip("mpmath")
    fx = np.load(ts_grad_mp.FIXTURE)
    r = ts_grad_mp.points()
    assert np.array_equal(r, fx["r"]) and np.array_equal(np.signbit(r), np.signbit(fx["r"]))
    pick = np.arange(0, len(r), 7)
    hi, lo = ts_grad_mp.reference(r[pick])
    assert np.array_equal(hi, fx["hi"][pick]) and np.array_equal(lo, fx["lo"][pick])


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def _problem(covar, D, seed, N=14, M=9, S=3, F=32):
    rs = np.random.RandomState(seed)
    comp, cand = rs.rand(N, D), rs.rand(M, D)
    vals = np.sin(3 * comp[:, 0]) + 0.1 * rs.randn(N)
    row = np.concatenate(([0.2, 0.05, 1.3], rs.uniform(0.4, 1.2, D)))
    R = engine.thompson_randoms(np.random.RandomState(seed + 1), covar, D, 1, N, F, S)
    return comp, cand, vals, row, R


@pytest.mark.parametrize("D", [1, 3, 9])
@pytest.mark.parametrize("covar", COVARS)
def test_oracle_value_and_central_differences(covar, D):
    """value == ts_oracle.paths at the same rows (two float64 routes of one formula), and the gradient against central
    differences of ts_oracle.paths: step 1e-5, error O(h^2 f''') ~ 1e-10 (2 pi nu)^3 plus the value's rounding / h."""
    comp, cand, vals, row, R = _problem(covar, D, 40 + D)
    want = tso.paths(covar, comp, cand, vals, row, R)
    h = 1e-5
    for s in (0, 2):
        f, g, p, gp, m, gu = tgo.value_grad(covar, comp, vals, row, R, s, cand, parts=True)
        scale = np.max(np.abs(want[s])) + 1.0
        assert np.max(np.abs(f - want[s])) <= 1e-11 * scale
        assert np.allclose(f, (m + row[0]) + p, rtol=0, atol=1e-15 * scale) and np.allclose(g, gu + gp, rtol=0, atol=1e-12)
        for j in range(D):
            e = np.zeros(D)
            e[j] = h
            fd = (tso.paths(covar, comp, cand + e, vals, row, R)[s] - tso.paths(covar, comp, cand - e, vals, row, R)[s]) / (2 * h)
            assert np.max(np.abs(fd - g[:, j])) <= 2e-5 * (1.0 + np.max(np.abs(g))), (s, j)
    # a NaN or infinite coordinate: NaN for that point alone
    bad = cand.copy()
    bad[1, 0], bad[3, D - 1] = np.nan, np.inf
    fb, gb = tgo.value_grad(covar, comp, vals, row, R, 0, bad)
    ok = np.ones(len(cand), dtype=bool)
    ok[[1, 3]] = False
    f0, g0 = tgo.value_grad(covar, comp, vals, row, R, 0, cand)
    assert np.all(np.isnan(fb[~ok])) and np.all(np.isnan(gb[~ok])) and np.array_equal(fb[ok], f0[ok]) and np.array_equal(gb[ok], g0[ok])


def test_grad_bound_holds_between_two_routes_of_the_oracle():
    """The bound is positive, scales with the weights, and covers the distance between the long-double prior gradient and a plain
    float64 evaluation of the same formula (which stays inside the float64 part of the budget)."""
    covar, D = "Matern52", 3
    comp, cand, vals, row, R = _problem(covar, D, 77, F=48)
    pth = tgo.Path(covar, comp, vals, row, R, 1)
    _, gp, sn = pth.prior(cand)
    b = tgo.grad_bound(row, pth.w, pth.nu, pth.phase, cand, 4, sn)
    assert b.shape == (len(cand), D) and np.all(b > 0)
    r = tso.phases(pth.nu, pth.phase, cand)
    g64 = -(pth.scale * tso.TWO_PI) * np.dot(np.sin(2 * np.pi * r) * pth.w[None, :], pth.nu)
    assert np.max(np.abs(g64 - gp.astype(np.float64)) / b) <= 1.0
    b2 = tgo.grad_bound(row, 2 * pth.w, pth.nu, pth.phase, cand, 4, sn)
    assert np.allclose(b2, 2 * b)


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_engine_refuses_before_any_device_is_touched():
    eng = engine.Engine(0)                                              # (lazy: no GPU is touched by any call below)
    eng.D, eng.H, eng.N, eng.M = 2, 1, 3, 4
    with pytest.raises(ValueError) as ei:
        eng.thompson_grad_batch(np.zeros((3, 2)))
    assert "spx_thompson_grad_batch" in str(ei.value) and "call spx_thompson first" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        eng.thompson_grad_batch(np.zeros((3, 5)))
    assert "(P, D)" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        eng.thompson_grad_batch(np.zeros((3, 2)), path_of=[0, 0])
    assert "path_of" in str(ei.value)
    assert eng._lib.spx_thompson_grad_batch(eng._h, None, None, 1, None, None, None) == engine.SPX_ERR_ARG
    eng.close()
    multi = engine.MultiEngine([0, 0])
    with pytest.raises(ValueError) as ei:
        multi.thompson_grad_batch(np.zeros((1, 2)))
    assert "multi-device" in str(ei.value)
    x = np.zeros((1, 2))
    rc = multi._lib.spx_thompson_grad_batch(multi._h, engine._dp(x), None, 1, engine._dp(np.zeros(1)), engine._dp(x.copy()), None)
    assert rc == engine.SPX_ERR_ARG and "call spx_thompson first" in multi._lib.spx_last_error().decode()
    multi.close()


# ---- the chooser ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod,args", [(GPEIChooser, "acq=TS,ts_refine=1"), (GPEIChooser, "ts_refine=1"),
                                      (GPEIperSecChooser, "ts_refine=1"), (GPConstrainedEIChooser, "ts_refine=1"),
                                      (GPParetoChooser, "ts_refine=1"), (GPEIperSecChooser, "acq=TS,ts_refine=1"),
                                      (GPEIOptChooser, "ts_refine=1"), (GPEIOptChooser, "acq=EI,ts_refine=1"),
                                      (GPEIOptChooser, "acq=LCB,acq_par=1,ts_refine=1"), (GPEIOptChooser, "acq=MES,ts_refine=1")])
def test_chooser_refuses_ts_refine(mod, args, tmp_path):
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), args)
    assert "allowed" in str(ei.value)


def test_chooser_accepts_ts_refine(tmp_path):
    assert GPEIOptChooser.init(str(tmp_path), "acq=TS").ts_refine is False
    assert GPEIOptChooser.init(str(tmp_path), "acq=TS,ts_refine=0").ts_refine is False
    assert GPEIOptChooser.init(str(tmp_path), "acq=TS,ts_refine=1").ts_refine is True
    assert GPEIOptChooser.init(str(tmp_path), "acq=TS,ts_refine=1,covar=SE").covar == "SE"
    assert GPEIChooser.init(str(tmp_path), "acq=TS,ts_refine=0").ts_refine is False


def _branin_inputs(golden_dir, n_done=12, n_pend=0, n_rows=120):
    grid = np.array(np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:n_rows], copy=True)
    values = np.zeros(grid.shape[0]) + np.nan
    done = np.arange(n_done)
    values[done] = branin(grid[done, 0], grid[done, 1])
    pend = np.arange(n_done, n_done + n_pend)
    free = np.arange(n_done + n_pend, grid.shape[0])
    return grid, values, np.zeros(grid.shape[0]), free, pend, done


ARG = "mcmc_iters=3,burnin=4,grid_subset=3,acq=TS,acq_par=32"


def _run(tmp_path, name, arg, inputs, seed=5):
    d = tmp_path / name
    d.mkdir()
    ch = GPEIOptChooser.init(str(d), arg)
    ch._eng = TsGradOracleEngine()
    np.random.seed(seed)
    job = ch.next(*inputs)
    return ch, job, np.random.get_state()


@pytest.mark.parametrize("covar", ["Matern52", "SE"])
@pytest.mark.parametrize("n_pend", [0, 2])
def test_ts_refine_minimises_the_path_off_the_grid(n_pend, covar, golden_dir, tmp_path):
    inputs = _branin_inputs(golden_dir, n_pend=n_pend)
    grid, free = inputs[0], inputs[3]
    arg = ARG + ",covar=" + covar
    c0, job0, st0 = _run(tmp_path, "plain", arg, inputs)
    ca, joba, sta = _run(tmp_path, "zero", arg + ",ts_refine=0", inputs)
    c1, job1, st1 = _run(tmp_path, "refine", arg + ",ts_refine=1", inputs)
    # ts_refine=0 is the chooser as it was: the proposal, the record and the generator
    assert job0 == joba and isinstance(job0, int) and c0.last_thompson == ca.last_thompson and same_state(st0, sta)
    assert set(c0.last_thompson) == {"draw", "grid_index", "path_min", "features"}
    # ts_refine=1 draws no random numbers and starts from the same path
    assert same_state(st0, st1)
    t = c1.last_thompson
    assert set(t) == {"draw", "grid_index", "path_min", "features", "refined", "x", "value"}
    assert all(t[k] == c0.last_thompson[k] for k in ("draw", "grid_index", "path_min", "features"))
    eng = c1._eng
    kinds = [c[0] for c in eng.calls]
    assert kinds.count("thompson") == 1 and "thompson_grad_batch" in kinds and "ei_grad_batch" not in kinds
    assert eng.calls[-1] == ("thompson_grad_batch", 3 + 1)               # the refined points and the grid's winner, one call
    path = eng.paths[0, 0]
    assert t["path_min"] == np.min(path)
    if t["refined"]:
        numcand, x = job1
        assert numcand == len(free) and np.array_equal(x, t["x"])
        assert np.all(x >= 0.0) and np.all(x <= 1.0)
        f = eng.thompson_grad_batch(x[None, :])[0][0]
        assert f == t["value"] and f < np.min(path)                       # strictly lower than the grid's winner
    else:
        assert job1 == job0 and np.array_equal(t["x"], grid[job0])
    # on this problem the minimum of a smooth path lies between the grid's points
    assert t["refined"]
    assert t["value"] <= np.min(path)


def test_an_unmoved_point_keeps_its_grid_index(golden_dir, tmp_path, monkeypatch):
    """A point the optimiser did not move is a copy of a grid row with the row's value: not strictly lower, so the proposal is
    the grid index, not a new point."""
    inputs = _branin_inputs(golden_dir)
    monkeypatch.setattr(refine, "lbfgs_many", lambda fn, pts, bounds, log=None, serial=None: np.array(pts, dtype=float, copy=True))
    c0, job0, _ = _run(tmp_path, "plain", ARG, inputs)
    monkeypatch.setattr(refine, "lbfgs_many", lambda fn, pts, bounds, log=None, serial=None: np.array(pts, dtype=float, copy=True))
    c1, job1, _ = _run(tmp_path, "refine", ARG + ",ts_refine=1", inputs)
    assert isinstance(job1, int) and job1 == job0
    t = c1.last_thompson
    assert t["refined"] is False and np.array_equal(t["x"], inputs[0][job0])
    assert abs(t["value"] - t["path_min"]) <= 1e-9 * (1.0 + abs(t["path_min"]))


def test_a_nan_path_proposes_the_first_nan(golden_dir, tmp_path):
    inputs = _branin_inputs(golden_dir)
    grid, free = inputs[0], inputs[3]
    grid[free[40], 1] = np.nan
    grid[free[17], 0] = np.nan
    c1, job1, st1 = _run(tmp_path, "refine", ARG + ",ts_refine=1", inputs)
    assert job1 == free[17]
    t = c1.last_thompson
    assert t["refined"] is False and t["grid_index"] == 17 and np.isnan(t["value"]) and np.isnan(t["path_min"])
    assert "thompson_grad_batch" not in [c[0] for c in c1._eng.calls]
    c0, job0, st0 = _run(tmp_path, "plain", ARG, inputs)
    assert job0 == job1 and same_state(st0, st1)


def test_reports_run_after_a_refined_call(golden_dir, tmp_path):
    inputs = _branin_inputs(golden_dir)
    d = tmp_path / "r"
    d.mkdir()
    ch = GPEIOptChooser.init(str(d), ARG + ",ts_refine=1,recommend=1")
    ch._eng = TsGradOracleEngine()
    np.random.seed(6)
    ch.next(*inputs)
    assert ch.last_recommendation is not None and ch.last_acq_used == "TS" and "refined" in ch.last_thompson
