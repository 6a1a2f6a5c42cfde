"""spx_loo on the MI355X: the values against a 50-digit yardstick on the library's own K and against the float64 oracle at
every boundary of the row walk (the 64-column groups, the 256-column unrolled step, the 128-row padding), the identities with
the downloaded factor, bit-for-bit independence of everything that is not the draw's own factorisation, the time model, the
handle's state before and after, every refusal, NaN, and the choosers' loo=1 end to end.  Every case is a few milliseconds
of device work."""
import os

import numpy as np
import numpy.random as npr
import pytest
import scipy.linalg as spla

from spearmint_amd import engine as spx
from spearmint_amd.synthetic import synthetic_problem
from tests import loo_mp
from tests import loo_oracle as lo
from tests.effects_helpers import same_bits

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
COVARS = ["Matern52", "Matern32", "ARDSE", "SE"]


@pytest.fixture(scope="module")
def eng():
    e = spx.Engine(0)   # raises if libspx.so or the GPU is missing -- no fallback
    yield e
    e.close()


def _factored(eng, comp, y, rows, covar="Matern52"):
    eng.set_covar(covar)
    eng.set_observations(comp, y)
    eng.set_hypers(rows)
    eng.factor()


def _same(a, b):
    return all(same_bits(a[k], b[k]) for k in ("loo_mean", "loo_var", "kinv_diag"))


def _assert_close(got, want, y, where=""):
    """The project's tolerance for alpha (tests/test_gpu_a_parity.py): rtol 1e-8, atol 1e-10 x the largest magnitude."""
    for g, w, name in zip((got["loo_mean"], got["loo_var"], got["kinv_diag"]), want, ("loo_mean", "loo_var", "kinv_diag")):
        assert g.shape == w.shape
        assert np.allclose(g, w, rtol=1e-8, atol=1e-10 * np.abs(w).max()), (where, name, np.max(np.abs(g - w)))


# ---- 1. against the 50-digit yardstick on the library's own K ----------------------------------------------------------------
@pytest.mark.parametrize("covar", COVARS)
@pytest.mark.parametrize("N,D", [(24, 3), (24, 9), (40, 3), (40, 9)])
def test_values_against_the_yardstick(eng, N, D, covar):
    """K is fetched from the handle, so the covariance's rounding is not judged here.  Bound: max(32 x the float64 oracle's
    error on the same K, 64 eps), relative to max|y - mean| for loo_mean and to the value for loo_var and kinv_diag.  Both
    routes are backward-stable solves whose error scales with cond(K); they differ in blocking and summation order only.
    Measured on one MI355X over the 16 cases (device / oracle, largest): see DESIGN.md section 14."""
    H = 3
    comp, y, rows = lo.problem(N, D, H, 3000 + N + D, noise=1e-3)
    try:
        _factored(eng, comp, y, rows, covar)
        got = eng.loo()
        for d in range(H):
            K = eng.get_factor(d, want_L=False, want_alpha=False)[0]
            want = loo_mp.loo_mp(K, y, rows[d, 0])
            e_dev = loo_mp.errors((got["loo_mean"][d], got["loo_var"][d], got["kinv_diag"][d]), want, y, rows[d, 0])
            e_orc = loo_mp.errors(lo.loo_from_k(K, y, rows[d, 0]), want, y, rows[d, 0])
            print("N=%d D=%d %s draw %d cond %.2e  device %.2e %.2e %.2e  oracle %.2e %.2e %.2e"
                  % ((N, D, covar, d, np.linalg.cond(K)) + e_dev + e_orc))
            for a, b in zip(e_dev, e_orc):
                assert a <= max(32 * b, 64 * EPS)
    finally:
        eng.set_covar("Matern52")


# ---- 2. against the float64 oracle, across every boundary of the walk -----------------------------------------------------------
# N: one and two rows; the ends of a 64-column group (63, 64, 65); the padding to 128 (127, 128, 129: Np = 128 / 256); the
# unrolled 256-column step with 0, 1, 2, 3 groups left over (255, 256, 257 -> Np = 256, 384; 300 -> 384; 641 -> 768).
@pytest.mark.parametrize("N,D,H", [(1, 1, 1), (1, 3, 3), (2, 3, 1), (2, 9, 3), (63, 1, 3), (64, 3, 1), (65, 9, 3), (127, 3, 3),
                                   (128, 1, 1), (129, 9, 1), (255, 3, 1), (256, 9, 3), (257, 1, 3), (300, 3, 3), (641, 9, 1),
                                   (641, 1, 3)])
def test_values_against_the_oracle(eng, N, D, H):
    comp, y, rows = lo.problem(N, D, H, 3100 + N + D, noise=1e-2)
    _factored(eng, comp, y, rows)
    got = eng.loo()
    assert got["loo_mean"].shape == (H, N) and np.array_equal(got["y"], y)
    _assert_close(got, lo.loo(comp, y, rows), y, (N, D, H))
    if N == 1:
        # the closed form, exactly where it is exact: loo_var = 1 / c and loo_mean = y - alpha / c are single IEEE operations
        # on the library's own c and alpha.  Against K_00 = amp2 (1 + 1e-6) + noise and the prior mean, to rounding: W =
        # K_00^-1/2 comes from the hardware's reciprocal square root and one Newton step (within 2 ulp), c = W^2 doubles that
        # and rounds, 1 / c rounds once more: 5 ulp, bound 8 eps.  alpha / c = (y - mean)(1 + the same few eps), and the
        # subtraction rounds at the size of its operands: 16 eps of max(|y|, |mean|).
        for d in range(H):
            K, L, alpha = eng.get_factor(d)
            c = got["kinv_diag"][d, 0]
            assert got["loo_var"][d, 0] == 1.0 / c and got["loo_mean"][d, 0] == y[0] - alpha[0] / c
            assert abs(got["loo_var"][d, 0] / K[0, 0] - 1) <= 8 * EPS
            assert abs(got["loo_mean"][d, 0] - rows[d, 0]) <= 16 * EPS * max(abs(y[0]), abs(rows[d, 0]))
    # the summary is loo_summary of the two arrays
    ref = spx.loo_summary(y, got["loo_mean"], got["loo_var"])
    for k in ("z", "lpd", "mean", "var", "z_mix", "lpd_mix"):
        assert same_bits(got[k], ref[k]), k


# ---- 3. identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,H", [(40, 3, 3), (129, 9, 1), (300, 3, 3)])
def test_identities_with_the_downloaded_factor(eng, N, D, H):
    comp, y, rows = lo.problem(N, D, H, 3200 + N, noise=1e-2)
    _factored(eng, comp, y, rows)
    got = eng.loo()
    assert np.all(np.abs(got["loo_var"] * got["kinv_diag"] - 1.0) <= EPS)            # 1 / c: one correctly rounded division
    for d in range(H):
        L, alpha = eng.get_factor(d, want_K=False)[1:]
        c = np.sum(spla.solve_triangular(L, np.eye(N), lower=True) ** 2, axis=0)       # sum(inv(L)**2, 0)
        assert np.allclose(got["kinv_diag"][d], c, rtol=1e-8, atol=0)
        assert np.array_equal(got["loo_mean"][d], y - alpha / got["kinv_diag"][d])     # one division, one subtraction


# ---- 4. bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 300])
def test_bits_do_not_depend_on_how_the_factor_was_reached(eng, N):
    D, H = 3, 3
    comp, cand, y, rows = synthetic_problem(N, 200, D, H, 3300 + N)
    _factored(eng, comp, y, rows)
    one = eng.loo()
    assert _same(eng.loo(), one)                                       # called twice
    eng.set_candidates(cand)                                           # with candidates
    assert _same(eng.loo(), one)
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)                                  # ... and a finished pass
    assert _same(eng.loo(), one)
    eng.ei_step()                                                      # the factor of spx_ei_step
    assert _same(eng.loo(), one)
    eng.ei_grid(comp, y, cand, rows)                                   # ... and of spx_ei_grid
    assert _same(eng.loo(), one)
    try:
        for ei_flow in (0, 1):
            for lean_flow_cov in (0, 1):
                eng.set_option("ei_flow", ei_flow)
                eng.set_option("lean_flow_cov", lean_flow_cov)
                eng.factor()
                assert _same(eng.loo(), one), (ei_flow, lean_flow_cov)
    finally:
        eng.set_option("ei_flow", -1)
        eng.set_option("lean_flow_cov", -1)
    # a draw alone and as draw 0, 1, 2 of three
    for d in range(H):
        eng.set_hypers(rows[d:d + 1])
        eng.factor()
        alone = eng.loo()
        for k in ("loo_mean", "loo_var", "kinv_diag"):
            assert same_bits(alone[k][0], one[k][d]), (d, k)
    # a second handle
    other = spx.Engine(0)
    try:
        _factored(other, comp, y, rows)
        assert _same(other.loo(), one)
    finally:
        other.close()


# ---- 5. the time model -----------------------------------------------------------------------------------------------------------
def test_time_model(eng):
    N, D, H = 150, 4, 3
    comp, cand, y, rows, log_durs, trows = synthetic_problem(N, 50, D, H, 3400, per_sec=True)
    _factored(eng, comp, y, rows)
    plain = eng.loo()
    with pytest.raises(ValueError) as ei:
        eng.loo("time")                                                # no time model in this factorisation
    assert "time model" in str(ei.value)
    assert _same(eng.loo(), plain)
    eng.set_time_model(log_durs, trows)
    with pytest.raises(ValueError):
        eng.loo("time")                                                # held now, but the factorisation is gone with the change
    eng.factor()
    got = eng.loo("time")
    assert np.array_equal(got["y"], log_durs)
    _assert_close(got, lo.loo(comp, log_durs, trows), log_durs, "time")
    assert _same(eng.loo("objective"), plain)                          # the objective's output: the same bits beside a time model
    eng.set_time_model(None, None)
    with pytest.raises(ValueError):
        eng.loo()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------
def _refused(eng, *a):
    with pytest.raises(ValueError) as ei:
        eng.loo(*a)
    assert eng._lib.spx_last_error()
    return str(ei.value)


def test_a_reader_changes_nothing(eng):
    comp, cand, y, rows = synthetic_problem(150, 400, 3, 3, 3500)
    eng.set_observations(comp, y); eng.set_candidates(cand); eng.set_hypers(rows)
    eng.set_acquisition(spx.ACQ_PI, 0.01)
    try:
        eng.ei_step(spx.FLAG_KEEP_MOMENTS)
        before = (eng.best(), eng.ei_mean(), [eng.get_moments(d) for d in range(3)], eng.ei_grad_batch(cand[:5]))
        eng.loo()
        after = (eng.best(), eng.ei_mean(), [eng.get_moments(d) for d in range(3)], eng.ei_grad_batch(cand[:5]))
        assert before[0] == after[0] and np.array_equal(before[1], after[1])
        for a, b in zip(before[2], after[2]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(before[3][0], after[3][0]) and np.array_equal(before[3][1], after[3][1])
        assert eng.get_acquisition() == (spx.ACQ_PI, 0.01)
        eng.ei_run(spx.FLAG_KEEP_MOMENTS)                              # candidates and factor still there: the same pass again
        assert eng.best() == before[0] and np.array_equal(eng.ei_mean(), before[1])
    finally:
        eng.set_acquisition(spx.ACQ_EI)


def test_accepts_or_refuses_after_every_writer(eng):
    N, H = 60, 2
    comp, cand, y, rows, log_durs, trows = synthetic_problem(N, 300, 2, H, 3600, per_sec=True)
    eng.set_observations(comp, y); eng.set_candidates(cand); eng.set_hypers(rows)
    assert "spx_factor" in _refused(eng)                               # before any factorisation
    eng.factor()
    one = eng.loo()
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    held = (eng.best(), eng.ei_mean(), eng.get_moments(0)[0])

    def results_readable():
        assert eng.best() == held[0] and np.array_equal(eng.ei_mean(), held[1]) and np.array_equal(eng.get_moments(0)[0], held[2])
    # bad arguments with everything held: refused, the handle as it was
    assert eng._lib.spx_loo(eng._h, 0, None, None, None) == spx.SPX_ERR_ARG
    assert eng._lib.spx_loo(eng._h, 7, spx._dp(np.zeros((H, N))), spx._dp(np.zeros((H, N))), None) == spx.SPX_ERR_ARG
    assert "time model" in _refused(eng, "time")
    results_readable()
    assert _same(eng.loo(), one)
    # kinv_diag may be NULL
    a, b = np.empty((H, N)), np.empty((H, N))
    assert eng._lib.spx_loo(eng._h, 0, spx._dp(a), spx._dp(b), None) == 0
    assert np.array_equal(a, one["loo_mean"]) and np.array_equal(b, one["loo_var"])
    # fantasies, both ways in and both ways out
    fant = np.repeat(np.repeat(y[None, :, None], H, axis=0), 2, axis=2)
    eng.set_fantasies(fant, np.full((H, 2), np.min(y)))
    eng.ei_run()
    with_fant = (eng.best(), eng.ei_mean())
    assert "fantasies" in _refused(eng)
    assert eng.best() == with_fant[0] and np.array_equal(eng.ei_mean(), with_fant[1])
    eng.ei_run()                                                       # the fantasies and the candidates are still there
    assert eng.best() == with_fant[0]
    eng.set_fantasies(None, None)
    assert _same(eng.loo(), one)
    eng.draw_fantasies(np.random.RandomState(1).randn(3, 4), 3)        # the last three rows as pending points
    assert "fantasies" in _refused(eng)
    eng.draw_fantasies(None, 0)
    assert _same(eng.loo(), one)
    # every writer of an input takes the factorisation away: refused until the next one
    for write in (lambda: eng.set_observations(comp, y), lambda: eng.set_hypers(rows), lambda: eng.set_covar("Matern32"),
                  lambda: eng.set_time_model(log_durs, trows), lambda: eng.set_time_model(None, None), lambda: eng.gp_logprob()):
        eng.set_covar("Matern52")
        eng.set_hypers(rows)
        eng.factor()
        assert _same(eng.loo(), one)
        write()
        assert "spx_factor" in _refused(eng)
        eng.set_covar("Matern52")
    eng.set_time_model(None, None)
    eng.set_hypers(rows)
    eng.factor()
    assert _same(eng.loo(), one)
    # a factorisation that fails: a status code, and nothing to read
    bad = rows.copy()
    bad[1, 2] = -1.0
    eng.set_hypers(bad)
    with pytest.raises(np.linalg.LinAlgError):
        eng.factor()
    assert eng.not_pd_info()[0] == 1
    assert "spx_factor" in _refused(eng)
    eng.set_hypers(rows)                                               # the handle is usable
    eng.factor()
    assert _same(eng.loo(), one)
    eng.set_candidates(cand)
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    results_readable()


def test_multi_device_handle_is_refused(eng):
    comp, cand, y, rows = synthetic_problem(60, 300, 2, 2, 3700)
    me = spx.MultiEngine([0, 0])                                       # two slots on one GPU (host transport)
    try:
        me.set_observations(comp, y); me.set_candidates(cand); me.set_hypers(rows)
        me.factor(); me.ei_run()
        held = (me.best(), me.ei_mean())
        with pytest.raises(ValueError):
            me.loo()
        a, b = np.empty((2, 60)), np.empty((2, 60))
        assert me._lib.spx_loo(me._h, 0, spx._dp(a), spx._dp(b), None) == spx.SPX_ERR_ARG
        assert b"single-GPU" in me._lib.spx_last_error()
        assert me.best() == held[0] and np.array_equal(me.ei_mean(), held[1])
        me.ei_run()
        assert me.best() == held[0]
    finally:
        me.close()


# ---- 7. NaN ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 300])
def test_nan_observation(eng, N):
    """alpha = K^-1 (y - mean) is NaN in every row once one y is, so loo_mean is NaN throughout; loo_var and kinv_diag do not
    read y and keep their bits.  No error is returned."""
    comp, y, rows = lo.problem(N, 3, 2, 3800 + N)
    _factored(eng, comp, y, rows)
    clean = eng.loo()
    bad = y.copy()
    bad[7] = np.nan
    _factored(eng, comp, bad, rows)
    got = eng.loo()
    assert np.all(np.isnan(got["loo_mean"]))
    assert np.array_equal(got["loo_var"], clean["loo_var"]) and np.array_equal(got["kinv_diag"], clean["kinv_diag"])
    assert np.isnan(got["elpd"]) and list(got["outliers"]) == []


# ---- 8. the choosers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pending", [0, 1])
@pytest.mark.parametrize("name,args", [("GPEIChooser", "mcmc_iters=3"),
                                       ("GPEIOptChooser", "mcmc_iters=3,burnin=5,grid_subset=4,use_multiprocessing=0")])
def test_choosers_write_the_oracles_report(tmp_path, name, args, n_pending):
    import importlib
    from tests.helpers import branin
    mod = importlib.import_module("spearmint_amd.chooser." + name)
    grid = np.random.RandomState(41).rand(20 + n_pending + 400, 2)
    values = branin(grid[:, 0], grid[:, 1])
    complete = np.arange(20)[::-1].copy()
    pending = np.arange(20, 20 + n_pending)
    cand = np.arange(20 + n_pending, grid.shape[0])
    jobs, seen = {}, []
    for loo in (0, 1):
        d = tmp_path / ("c%d" % loo)
        d.mkdir()
        ch = mod.init(str(d), args + ",loo=%d" % loo)
        orig = ch._loo

        def record(complete, comp, vals, rows, orig=orig):
            seen.append(np.array(rows, copy=True))
            return orig(complete, comp, vals, rows)
        ch._loo = record
        npr.seed(17)
        try:
            jobs[loo] = ch.next(grid, values, values * 0, cand, pending, complete)
            if loo:
                assert ch.engine().stat("fantasies_count") == 0 and ch.last_loo["loo_mean"].shape == (3, 20)
        finally:
            ch.engine().close()
    a, b = jobs[0], jobs[1]
    assert type(a) is type(b)
    if isinstance(a, tuple):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    else:
        assert a == b
    assert not os.path.exists(str(tmp_path / "c0" / "loo.txt")) and len(seen) == 1
    head, rows = lo.parse_report(str(tmp_path / "c1" / "loo.txt"))
    want_head, want_rows = lo.report(complete, grid[complete], values[complete], seen[0])
    assert rows.shape == (20, 6) and np.array_equal(rows[:, 0], complete) and np.array_equal(rows[:, 1], values[complete])
    for col in range(2, 6):
        assert np.allclose(rows[:, col], want_rows[:, col], rtol=1e-8, atol=1e-10 * np.abs(want_rows[:, col]).max()), col
    assert head["completed"] == 20 and head["draws"] == 3 and head["outliers"] == want_head["outliers"]
    assert head["coverage95"] == want_head["coverage95"]
    for k in ("elpd", "rmse"):
        assert np.isclose(head[k], want_head[k], rtol=1e-8, atol=0), k
