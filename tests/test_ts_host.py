"""Thompson sampling without a GPU (include/spx.h: spx_thompson; tests/ts_oracle.py restates its contract): the spectral law of
every covariance, the conditioning algebra, cos2pi of csrc/ts_device.h on the host against 50 digits, the chooser arguments,
the order in which the base randoms are drawn, and that acq=EI is where it was."""
import json
import os

import numpy as np
import pytest
import scipy.linalg as spla

from oracle import gp_ei_oracle as orc
from spearmint_amd import engine
from spearmint_amd.chooser import GPConstrainedEIChooser, GPEIChooser, GPEIOptChooser, GPEIperSecChooser, GPParetoChooser
from tests import plan_helpers as ph
from tests import ts_mp, ts_oracle as tso
from tests.helpers import branin
from tests.mes_helpers import same_state
from tests.ts_helpers import TsOracleEngine, cos2pi_on_host, ei_state_runs

COVARS = ("Matern52", "Matern32", "ARDSE", "SE")


# ---- the spectral law -----------------------------------------------------------------------------------------------------
F_LAW = 65536
LAW_BAR = 5.0 * np.sqrt(1.5 / F_LAW)          # 0.0239 per unit amp2: the per-term variance of 2 cos cos is at most 1.5


def _law_statistic(covar, D, law=None):
    """max over all pairs of 40 points of |feature kernel - exact kernel| per unit amp2; `law`: (name of the law the
    frequencies are formed with, degrees of freedom of chi) when it is not the covariance's own."""
    rs = np.random.RandomState(7)
    X = rs.rand(40, D)
    ls = rs.uniform(0.3, 1.5, D)
    row = np.concatenate(([0.0, 1e-3, 1.0], ls))
    R = engine.thompson_randoms(np.random.RandomState(11), covar, D, 1, 1, F_LAW, 1)
    law_name, chi = covar, R["chi"]
    if law is not None:
        law_name = law[0]
        chi = np.random.RandomState(12).chisquare(law[1], F_LAW)
        if covar == "SE":                    # (a Student law for SE: Matern frequencies, SE's unit length scales)
            row = np.concatenate(([0.0, 1e-3, 1.0], np.ones(D)))
    got = tso.feature_kernel(law_name, row, R["omega_z"], chi, R["phase"], X, X)
    with orc.covar(covar):
        want = orc.corr(ls, X, X)
    return float(np.max(np.abs(got - want)))


@pytest.mark.parametrize("D", [3, 8])
@pytest.mark.parametrize("covar", COVARS)
def test_spectral_law(covar, D):
    stat = _law_statistic(covar, D)
    print("spectral law %s D=%d: %.4f (bar %.4f)" % (covar, D, stat, LAW_BAR))
    assert stat <= LAW_BAR


@pytest.mark.parametrize("D", [3, 8])
@pytest.mark.parametrize("covar,law", [("Matern52", ("Matern52", 3)), ("Matern32", ("Matern32", 5)), ("SE", ("Matern52", 5))])
def test_spectral_law_test_has_power(covar, law, D):
    """The same statistic under a wrong law -- 3 degrees of freedom for Matern52, 5 for Matern32, a Student law for SE --
    exceeds the bar."""
    stat = _law_statistic(covar, D, law)
    print("wrong law %s <- %s D=%d: %.4f (bar %.4f)" % (covar, law, D, stat, LAW_BAR))
    assert stat > LAW_BAR


# ---- the conditioning algebra ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("covar,N,D,seed", [("Matern52", 24, 3, 1), ("ARDSE", 40, 2, 2), ("Matern32", 40, 5, 3)])
def test_conditioning_algebra(covar, N, D, seed):
    """S = 4096 oracle paths from ONE set of F = 2048 features.  Given the features the paths are Gaussian in (w, eps) with
    mean exactly func_m (E w = E eps = 0: unbiased for any F) and the variance of the posterior-variance formula with its
    prior-prior blocks replaced by the feature kernel Phi Phi^T.  A wrong sig, a wrong sign of eps or a wrong scale moves the
    variance; a wrong mean term moves the mean."""
    S, F, M = 4096, 2048, 30
    rs = np.random.RandomState(100 + seed)
    comp, cand = rs.rand(N, D), rs.rand(M, D)
    vals = np.sin(3 * comp[:, 0]) + 0.1 * rs.randn(N)
    row = np.concatenate(([0.2, 0.05, 1.3], rs.uniform(0.4, 1.2, D)))
    R = engine.thompson_randoms(np.random.RandomState(seed), covar, D, 1, N, F, S)
    P = tso.paths(covar, comp, cand, vals, row, R)
    mean, noise, amp2, ls = orc.unpack_hyper(row)
    with orc.covar(covar):
        K = orc.cov(amp2, ls, comp) + noise * np.eye(N)
        Ks = orc.cov(amp2, ls, comp, cand)
    L = spla.cholesky(K, lower=True)
    A = spla.cho_solve((L, True), Ks)                                   # K^-1 k*, (N, M)
    func_m = np.dot(A.T, vals - mean) + mean
    m_hat, v_hat = np.mean(P, axis=0), np.var(P, axis=0, ddof=1)
    z = np.abs(m_hat - func_m) / np.sqrt(v_hat / S)
    kf = lambda a, b: tso.feature_kernel(covar, row, R["omega_z"], R["chi"], R["phase"], a, b)
    sig2 = tso.sig_of(row) ** 2
    v_exact = (np.diag(kf(cand, cand)) - 2.0 * np.sum(A * kf(comp, cand), axis=0)
               + np.sum(A * np.dot(kf(comp, comp) + sig2 * np.eye(N), A), axis=0))
    rel = np.abs(v_hat / v_exact - 1.0)
    print("conditioning %s N=%d: largest z %.2f, largest relative variance error %.3f (bar %.3f)"
          % (covar, N, np.max(z), np.max(rel), 5 * np.sqrt(2.0 / (S - 1))))
    assert np.max(z) <= 5.0
    assert np.max(rel) <= 5.0 * np.sqrt(2.0 / (S - 1))
    assert abs(sig2 - (noise + 1e-6 * amp2)) <= 1e-15 * sig2              # sig^2 is the diagonal term of the chooser covariance


# ---- cos2pi of csrc/ts_device.h on the host --------------------------------------------------------------------------------
@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_device_header_against_50_digits():
    """The header's own text (coefficients, order of operations) compiled for the host against the 50-digit table, +-1/2,
    +-1/4, 0 and the denormals included, at the budget the header derives: SPX_TS_COS_ULPS = 4 ulp of the result.
    Measured here: 2.77 ulp (at r = 2.65e-8; 2.42 ulp for |r| >= 1/8)."""
    fx = np.load(ts_mp.FIXTURE)
    got = cos2pi_on_host(fx["r"])
    e = ts_mp.ulp_errors(got, fx["hi"], fx["lo"])
    i = int(np.argmax(e))
    print("ts_device.h on the host: worst %.3f ulp at r = %r over %d points" % (e[i], float(fx["r"][i]), len(e)))
    assert tso.COS_ULPS == 4 and e[i] <= tso.COS_ULPS
    pick = lambda x: got[list(fx["r"]).index(x)]
    assert pick(0.25) == 0.0 and pick(-0.25) == 0.0                     # the zeros are exact
    assert pick(5e-324) == pick(0.0) and abs(pick(0.0) - 1.0) <= 2.0 ** -52
    assert np.isnan(cos2pi_on_host([np.nan])[0])


# ---- the base randoms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_draw", [False, True])
@pytest.mark.parametrize("covar", COVARS)
def test_random_number_consumption_order(covar, per_draw):
    D, H, N, F, S = 3, 2, 7, 32, 5
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    R = engine.thompson_randoms(a, covar, D, H, N, F, S, per_draw)
    lead = (H,) if per_draw else ()
    oz = b.randn(F, D)
    chi = b.chisquare({"Matern52": 5, "Matern32": 3}[covar], F) if covar.startswith("Matern") else None
    ph_, w, eps = b.rand(F), b.randn(*(lead + (S, F))), b.randn(*(lead + (S, N)))
    assert np.array_equal(R["omega_z"], oz) and np.array_equal(R["phase"], ph_)
    assert (R["chi"] is None) if chi is None else np.array_equal(R["chi"], chi)
    assert np.array_equal(R["w"], w) and np.array_equal(R["eps"], eps)
    assert same_state(a.get_state(), b.get_state())
    np.random.seed(9)                                                   # rng=None: numpy's global generator
    G = engine.thompson_randoms(None, covar, D, H, N, F, S, per_draw)
    assert np.array_equal(G["omega_z"], np.random.RandomState(9).randn(F, D))
    with pytest.raises(AttributeError):
        engine.thompson_randoms(a, "Matern12", D, H, N, F, S)


# ---- what the call holds, and the size it refuses (csrc/spx_plan.h: plan_ts) ------------------------------------------------------
TS_PLAN_CASES = [(2, 1, 1, 1, 1, 16, 0), (130, 1000, 9, 3, 17, 1024, 1), (257, 257, 33, 1, 3, 48, 0), (2048, 200000, 32, 20, 8, 4096, 0),
                 (2, 2097152, 1, 1, 256, 16, 0),       # H S Mp 8 == 4 GiB exactly: the largest that fits
                 (2, 2097153, 1, 1, 256, 16, 0),       # one candidate more is another 128-candidate tile: refused
                 (2, 1048576, 1, 2, 256, 16, 1), (2, 1048577, 1, 2, 256, 16, 1),
                 (2, 5, 1, 257, 255, 16, 0),           # H S == 65535: the per-path launches' grid still holds it
                 (2, 5, 1, 256, 256, 16, 0),           # 65536: refused
                 (65, 3 * 10 ** 9, 3, 1, 1, 16, 0)]    # beyond 2^31 candidates: refused, and nothing overflows on the way


@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_plan_ts():
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in TS_PLAN_CASES)
    got = [json.loads(ln) for ln in ph.ask("ts_plan_client", text)]
    assert len(got) == len(TS_PLAN_CASES)
    up = lambda a, b: (a + b - 1) // b * b             # noqa: E731
    for (N, M, D, H, S, F, per_draw), g in zip(TS_PLAN_CASES, got):
        Mp, Np = up(M, 128), up(N, 128)
        Dp = 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else up(D, 32)
        nd = H if per_draw else 1
        want = {"Mp": Mp, "Dp": Dp, "sblocks": (S + 15) // 16, "par_doubles": H * F * Dp + F + 2 * H, "w_bytes": nd * S * F * 8,
                "eps_bytes": nd * S * N * 8, "obs_bytes": H * S * N * 8, "gamma_bytes": H * S * Np * 8, "path_bytes": H * S * Mp * 8,
                "fits": int(H * S <= 65535 and H * S * Mp * 8 <= 4 << 30)}
        assert g == want, ((N, M, D, H, S, F, per_draw), g, want)
    assert [g["fits"] for g in got] == [1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 0]


# ---- the binding ------------------------------------------------------------------------------------------------------------
def test_engine_refuses_before_any_device_is_touched():
    eng = engine.Engine(0)                                              # (lazy: no GPU is touched by any call below)
    assert eng.stat("last_ts_paths") == 0 and eng.stat("last_ts_features") == 0
    eng.D, eng.H, eng.N, eng.M = 2, 1, 3, 4
    with pytest.raises(ValueError) as ei:
        eng.thompson(S=1, F=16, rng=np.random.RandomState(0))
    assert "spx_thompson" in str(ei.value) and "spx_factor" in str(ei.value)
    with pytest.raises(ValueError):
        eng.thompson_path(0, 0)
    with pytest.raises(ValueError):
        eng.thompson_prior(0, 0)
    assert engine.TS_MAX_FEATURES == 8192 and engine.TS_MAX_PATHS == 256
    eng.close()
    multi = engine.MultiEngine([0, 0])
    with pytest.raises(ValueError) as ei:
        multi.thompson()
    assert "multi-device" in str(ei.value)
    rc = multi._lib.spx_thompson(multi._h, 16, 1, None, None, None, None, None, 0, None, None)
    assert rc == engine.SPX_ERR_ARG
    multi.close()


# ---- chooser arguments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_accepts_ts(mod, tmp_path):
    ch = mod.init(str(tmp_path), "acq=TS")
    assert (ch.acq, ch.acq_par) == ("TS", 1024.0)                       # acq_par = 0, the default, means F = 1024
    assert mod.init(str(tmp_path), "acq=ts,acq_par=48").acq_par == 48.0
    assert mod.init(str(tmp_path), "acq=TS,acq_par=8192").acq_par == 8192.0
    assert ch.last_thompson is None
    assert mod.init(str(tmp_path), "acq=TS,gpu_refine=0").acq == "TS"   # nothing is refined under TS


@pytest.mark.parametrize("args", ["acq=TS,acq_par=8", "acq=TS,acq_par=24", "acq=TS,acq_par=8208", "acq=TS,acq_par=-16",
                                  "acq=TS,acq_par=nan", "acq=TS,acq_par=16.5", "acq=TS,ndev=2"])
@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_refuses_bad_ts_arguments(mod, args, tmp_path):
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), args)
    assert "allowed" in str(ei.value)


@pytest.mark.parametrize("mod", [GPEIperSecChooser, GPConstrainedEIChooser, GPParetoChooser])
def test_the_other_choosers_refuse_ts(mod, tmp_path):
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), "acq=TS")
    assert "allowed" in str(ei.value)


# ---- a call ---------------------------------------------------------------------------------------------------------------
def _branin_inputs(golden_dir, n_done=12, n_pend=0):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:300]
    values = np.zeros(grid.shape[0]) + np.nan
    done = np.arange(n_done)
    values[done] = branin(grid[done, 0], grid[done, 1])
    pend = np.arange(n_done, n_done + n_pend)
    free = np.arange(n_done + n_pend, grid.shape[0])
    return grid, values, np.zeros(grid.shape[0]), free, pend, done


@pytest.mark.parametrize("n_pend", [0, 2])
@pytest.mark.parametrize("mod,arg", [(GPEIChooser, "mcmc_iters=3"), (GPEIOptChooser, "mcmc_iters=3,burnin=4,grid_subset=3")])
def test_a_ts_call_draws_one_path_under_one_draw(mod, arg, n_pend, golden_dir, tmp_path):
    """The chain runs as without pending jobs, then d = randint(H), the engine gets the completed points and hyper row d alone,
    one path with F features is drawn from numpy's generator in the documented order, and its grid argmin is proposed.
    Pending jobs change nothing but the candidate set: no fantasies, no normals for them."""
    grid, values, durs, free, pend, done = _branin_inputs(golden_dir, n_pend=n_pend)
    ch = mod.init(str(tmp_path), arg + ",acq=TS,acq_par=64")
    eng = ch._eng = TsOracleEngine()
    np.random.seed(5)
    job = ch.next(grid, values, durs, free, pend, done)
    after = np.random.get_state()
    assert isinstance(job, int) and job in set(free)
    kinds = [c[0] for c in eng.calls]
    assert kinds.count("thompson") == 1 and "ei_grid" not in kinds and "ei_run" not in kinds and eng.fant is None
    assert eng.calls[-1] == ("thompson", len(free), 1, 1, 64)
    assert eng.comp.shape[0] == len(done) and eng.hypers.shape[0] == 1
    t = ch.last_thompson
    assert ch.last_acq_used == "TS" and set(t) == {"draw", "grid_index", "path_min", "features"}
    assert 0 <= t["draw"] < 3 and t["features"] == 64 and free[t["grid_index"]] == job
    assert t["path_min"] == np.min(eng.paths[0, 0]) and t["grid_index"] == int(np.argmin(eng.paths[0, 0]))
    # the same call of an acq=EI chooser (no pending jobs): the chain consumes the same numbers, so the generator of the TS call
    # is the EI call's advanced by randint(H) and thompson_randoms
    (tmp_path / "ei").mkdir()
    ei = mod.init(str(tmp_path / "ei"), arg)
    ei._eng = TsOracleEngine()
    np.random.seed(5)
    g2, v2, d2, free2, _, done2 = _branin_inputs(golden_dir, n_pend=0)
    ei.next(g2, v2, d2, free2, np.arange(0), done2)
    rs = np.random.RandomState()
    rs.set_state(np.random.get_state())
    assert int(rs.randint(3)) == t["draw"]
    engine.thompson_randoms(rs, "Matern52", 2, 1, len(done), 64, 1)
    assert same_state(rs.get_state(), after)


def test_reports_run_after_a_ts_call(golden_dir, tmp_path):
    grid, values, durs, free, pend, done = _branin_inputs(golden_dir)
    ch = GPEIChooser.init(str(tmp_path), "mcmc_iters=2,acq=TS,acq_par=32,recommend=1")
    ch._eng = TsOracleEngine()
    np.random.seed(6)
    ch.next(grid, values, durs, free, pend, done)
    assert ch.last_recommendation is not None and ch.last_acq_used == "TS"


def test_acq_ei_is_where_it_was(golden_dir, tmp_path):
    """With acq=EI the proposals on the golden seeds are the golden ones, and numpy's generator after EVERY call -- without
    pending jobs on both choosers, and with a pending job -- is in the state tests/golden/ts_ei_states.npz recorded on the
    commit before acq=TS existed (tests/ts_helpers.ei_state_runs), through an engine that knows thompson and choosers that
    know TS."""
    g = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))
    fx = np.load(os.path.join(golden_dir, "ts_ei_states.npz"))
    got = ei_state_runs(golden_dir, tmp_path, TsOracleEngine)
    assert set(got) == set(fx.files)
    for k in fx.files:
        assert got[k].dtype == fx[k].dtype and np.array_equal(got[k], fx[k]), k
    assert list(got["g_idx"]) == list(g["g_idx"][:5])
