"""Leave-one-out cross-validation on a CPU-only box: the float64 oracle against a 50-digit yardstick and against N explicit
refits, the arithmetic Engine.loo defines its summary by, the C ABI's argument checks (spx_create touches no GPU), and the
choosers' loo= argument on oracle-backed engines."""
import ctypes
import os

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine
from spearmint_amd.chooser import GPConstrainedEIChooser, GPEIChooser, GPEIOptChooser, GPEIperSecChooser
from tests import loo_mp
from tests import loo_oracle as lo
from tests.acq_helpers import AcqStandinEngine
from tests.effects_helpers import EffectsOracleEngine
from tests.helpers import branin

EPS = 2.0 ** -52


def oracle_bound(cond, y, mean):
    """What the float64 oracle may be off by.  Both of its steps (a Cholesky factorisation and triangular solves) are backward
    stable, so its error is a modest multiple of cond(K) eps: 8, five times the largest multiple seen over the cases (1.6).
    Beside it stands the rounding of the results themselves: a few eps of the value for loo_var and kinv_diag, and for
    loo_mean, which is stated relative to max|y - mean|, a few eps of |y| over that scale."""
    scale = np.max(np.abs(y - mean))
    return 8 * cond * EPS + 8 * EPS * (1 + np.max(np.abs(y)) / scale)


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, "loo_mp.npz"))


CASES = loo_mp.cases()


# ---- the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_against_the_yardstick_and_the_refits(case, recorded):
    name, comp, y, row, covar = case
    assert np.array_equal(recorded[name + "_comp"], comp) and np.array_equal(recorded[name + "_y"], y)
    assert np.array_equal(recorded[name + "_row"], row)
    K = lo.k_host(comp, row, covar)
    cond = np.linalg.cond(K)
    bound = oracle_bound(cond, y, row[0])
    got = lo.loo_from_k(K, y, row[0])
    # 50 digits on the same K
    err = loo_mp.errors(got, loo_mp.loo_mp(K, y, row[0]), y, row[0])
    print(name, "cond %.2e" % cond, "oracle error (mean, var, kinv_diag) %.2e %.2e %.2e" % err, "bound %.2e" % bound,
          "recorded", recorded[name + "_err"])
    assert max(err) <= bound
    # the fixture: the yardstick's values as recorded (K rebuilt here may differ from the recorded run's in the last place
    # of an exponential, which moves the exact answer by cond eps at the most: inside the same bound)
    scale = np.max(np.abs(y - row[0]))
    assert np.max(np.abs(got[0] - recorded[name + "_mean"])) / scale <= 2 * bound
    assert np.max(np.abs(got[1] / recorded[name + "_var"] - 1)) <= 2 * bound
    assert np.max(np.abs(got[2] / recorded[name + "_c"] - 1)) <= 2 * bound
    assert np.all(recorded[name + "_err"][:3] <= bound)
    # N explicit refits: the same quantities by the definition (no more accurate than the identity: twice the bound)
    m, v = lo.loo_refits(K, y, row[0])
    assert np.max(np.abs(got[0] - m)) / scale <= 2 * bound
    assert np.max(np.abs(got[1] / v - 1)) <= 2 * bound


def test_one_observation_is_the_prior():
    comp, y, rows = lo.problem(1, 3, 2, 5)
    lm, lv, c = lo.loo(comp, y, rows)
    for h in range(2):
        k00 = rows[h, 2] * (1 + 1e-6) + rows[h, 1]
        assert abs(lv[h, 0] / k00 - 1) <= 2 * EPS and abs(lm[h, 0] - rows[h, 0]) <= 4 * EPS * abs(y[0])


# ---- engine arithmetic ---------------------------------------------------------------------------------------------------
def test_summary_by_hand():
    y = np.array([1.0, 2.0, 4.0])
    lm = np.array([[1.0, 1.0, 0.0], [1.0, 3.0, 2.0]])
    lv = np.array([[1.0, 4.0, 1.0], [1.0, 4.0, 0.25]])
    s = engine.loo_summary(y, lm, lv)
    assert np.array_equal(s["z"], [[0.0, 0.5, 4.0], [0.0, -0.5, 4.0]])
    l2pi = np.log(2 * np.pi)
    assert np.allclose(s["lpd"], [[-0.5 * l2pi, -0.5 * (l2pi + np.log(4)) - 0.125, -0.5 * l2pi - 8],
                                  [-0.5 * l2pi, -0.5 * (l2pi + np.log(4)) - 0.125, -0.5 * (l2pi + np.log(0.25)) - 8]], rtol=1e-15, atol=0)
    assert np.array_equal(s["mean"], [1.0, 2.0, 1.0])
    assert np.array_equal(s["var"], [1.0, 5.0, 0.625 + 1.0])               # mean of the variances + variance of the means
    assert np.array_equal(s["z_mix"], [0.0, 0.0, 3.0 / np.sqrt(1.625)])
    assert np.allclose(s["lpd_mix"][:2], s["lpd"][0, :2], rtol=1e-15)       # equal densities: their mean is either
    want2 = np.log(0.5 * (np.exp(s["lpd"][0, 2]) + np.exp(s["lpd"][1, 2])))
    assert abs(s["lpd_mix"][2] - want2) <= 1e-14 * abs(want2)
    assert s["elpd"] == np.sum(s["lpd_mix"]) and s["rmse"] == np.sqrt(9.0 / 3)
    assert s["coverage95"] == 2.0 / 3 and list(s["outliers"]) == []
    s2 = engine.loo_summary(y + np.array([0.0, 0.0, 3.0]), lm, lv)             # z_mix = 6 / sqrt(1.625)
    assert list(s2["outliers"]) == [2] and s2["coverage95"] == 2.0 / 3
    assert sorted(s) == sorted(lo.summary(y, lm, lv))
    for k, v in lo.summary(y, lm, lv).items():
        assert np.allclose(s[k], v, rtol=1e-14, atol=0), k


def test_summary_of_one_draw_is_that_draw():
    rs = np.random.RandomState(2)
    y, lm, lv = rs.randn(7), rs.randn(1, 7), 0.1 + rs.rand(1, 7)
    s = engine.loo_summary(y, lm, lv)
    assert np.array_equal(s["var"], lv[0]) and np.array_equal(s["mean"], lm[0])
    assert np.array_equal(s["lpd_mix"], s["lpd"][0]) and np.array_equal(s["z_mix"], s["z"][0])


def test_summary_with_a_nan_observation():
    y = np.array([0.5, np.nan, 1.5])
    lm = np.array([[0.4, 1.0, 1.4], [0.6, 1.0, 1.6]])
    lv = np.ones((2, 3))
    s = engine.loo_summary(y, lm, lv)
    assert np.isnan(s["z"][:, 1]).all() and np.isnan(s["lpd_mix"][1]) and np.isnan(s["z_mix"][1])
    assert np.isfinite(s["lpd_mix"][[0, 2]]).all() and np.isfinite(s["z"][:, [0, 2]]).all()
    assert np.isnan(s["elpd"]) and np.isnan(s["rmse"])
    assert s["coverage95"] == 2.0 / 3 and list(s["outliers"]) == []          # a NaN z is neither covered nor an outlier


def test_mixture_density_does_not_underflow():
    """lpd down to -1e4: exp underflows to 0 at -745, the mixture's log must not become -inf."""
    y = np.zeros(3)
    z = np.array([[np.sqrt(2e4), 1.0, np.sqrt(2e4)], [np.sqrt(2.2e4), np.sqrt(2e4), 0.0]])
    s = engine.loo_summary(y, -z, np.ones((2, 3)))
    assert np.min(s["lpd"]) < -1e4
    assert np.all(np.isfinite(s["lpd_mix"]))
    base = -0.5 * np.log(2 * np.pi)
    assert abs(s["lpd_mix"][0] - (base - 1e4 - np.log(2))) <= 1e-10       # the second term is e^-1000 of the first
    assert abs(s["lpd_mix"][1] - (base - 0.5 - np.log(2))) <= 1e-14
    assert np.allclose(s["lpd_mix"], lo.summary(y, -z, np.ones((2, 3)))["lpd_mix"], rtol=1e-15)


# ---- argument checks with no GPU -------------------------------------------------------------------------------------------
def _err(lib):
    return lib.spx_last_error().decode()


def test_argument_and_call_order_checks_touch_no_device():
    lib = engine.load_library()
    h = ctypes.c_void_p()
    assert lib.spx_create(0, ctypes.byref(h)) == 0
    a, b, c = np.zeros((1, 4)), np.zeros((1, 4)), np.zeros((1, 4))
    dp = engine._dp
    assert lib.spx_loo(None, 0, dp(a), dp(b), dp(c)) == engine.SPX_ERR_ARG
    assert lib.spx_loo(h, 0, None, dp(b), dp(c)) == engine.SPX_ERR_ARG and "NULL" in _err(lib)
    assert lib.spx_loo(h, 0, dp(a), None, dp(c)) == engine.SPX_ERR_ARG and "NULL" in _err(lib)
    for model in (-1, 2):
        assert lib.spx_loo(h, model, dp(a), dp(b), dp(c)) == engine.SPX_ERR_ARG and "model=" in _err(lib)
    # everything in order but no factorisation: a call-order error, not a device error -- the handle is still lazy (on a box
    # without a GPU an initialisation would have answered SPX_ERR_HIP)
    for model in (0, 1):
        assert lib.spx_loo(h, model, dp(a), dp(b), None) == engine.SPX_ERR_ARG and "spx_factor" in _err(lib)
    lib.spx_destroy(h)


def test_engine_method_and_multi_handle():
    assert "spx_loo" in engine.ABI and engine.LOO_MODEL == {"objective": 0, "time": 1}
    eng = engine.Engine(0)
    with pytest.raises(ValueError):
        eng.loo("constraint")
    with pytest.raises(ValueError) as ei:
        eng.loo()
    assert "spx_factor" in str(ei.value)
    eng.close()
    multi = engine.MultiEngine([0, 0])                   # (repeated ids: creation touches no GPU)
    with pytest.raises(ValueError) as ei:
        multi.loo()
    assert "multi-device" in str(ei.value)
    multi.close()
    plain = engine.Engine(devices=[0, 0])                # the same handle without the class: the library refuses
    plain.H, plain.N = 1, 4
    with pytest.raises(ValueError) as ei:
        plain.loo()
    assert "single-GPU" in str(ei.value)
    plain.close()


# ---- choosers ----------------------------------------------------------------------------------------------------------------
class LooOracleEngine(EffectsOracleEngine):
    """tests/effects_helpers.EffectsOracleEngine (the oracle behind everything next() calls, pending jobs, recommend= and
    importance= included) + loo from tests/loo_oracle.py, against what factor() / ei_step() / ei_grid() last factored."""

    def __init__(self, covar="Matern52"):
        EffectsOracleEngine.__init__(self, covar)
        self.loo_calls = []

    def loo(self, model="objective"):
        if self.fant is not None:
            raise ValueError("spx_loo: fantasies are held")
        comp, vals, rows = self._last_comp, self._last_vals, np.atleast_2d(self._last_rows)
        self.loo_calls.append((model, comp.shape[0], rows.shape[0], self.factor_calls))
        lm, lv, c = lo.loo(comp, vals, rows, self.covar)
        out = engine.loo_summary(vals, lm, lv)
        out["kinv_diag"] = c
        return out


class LooStandinEngine(AcqStandinEngine):
    """tests/standin_engine.Engine (through tests/acq_helpers.AcqStandinEngine, which adds the setters a chooser calls)
    + last_warning, factor and loo: the least an engine needs for a loo=1 proposal without pending jobs and a host sampler."""

    def __init__(self, *a, **k):
        AcqStandinEngine.__init__(self, *a, **k)
        self.log = []

    def set_observations(self, comp, vals):
        self.log.append("set_observations")
        AcqStandinEngine.set_observations(self, comp, vals)

    def ei_grid(self, *a, **k):
        self.log.append("ei_grid")
        return AcqStandinEngine.ei_grid(self, *a, **k)

    def last_warning(self):
        return None

    def factor(self):
        self.log.append("factor")
        self._factored = (self.comp, self.vals, self.hypers)

    def loo(self, model="objective"):
        self.log.append("loo")
        comp, vals, rows = self._factored
        lm, lv, c = lo.loo(comp, vals, rows)
        out = engine.loo_summary(vals, lm, lv)
        out["kinv_diag"] = c
        return out


def test_standin_engine_sees_one_factorisation_and_one_reduction(tmp_path):
    rs = np.random.RandomState(4)
    grid = rs.rand(40, 2)
    values = branin(grid[:, 0], grid[:, 1])
    jobs = {}
    for loo in (0, 1):
        d = tmp_path / ("s%d" % loo)
        d.mkdir()
        ch = GPEIChooser.init(str(d), "mcmc_iters=2,sampler=python,gpu_logprob=0,loo=%d" % loo)
        eng = LooStandinEngine()
        ch._eng = eng
        npr.seed(3)
        jobs[loo] = ch.next(grid, values, values * 0, np.arange(8, 40), np.zeros(0, dtype=int), np.arange(8))
        tail = [c for c in eng.log if c != "set_observations"]
        assert tail == (["ei_grid", "factor", "loo"] if loo else ["ei_grid"])        # loo=0 calls nothing new
        assert eng.log[-3:] == ["set_observations", "factor", "loo"] if loo else True
    assert jobs[0] == jobs[1]
    assert not os.path.exists(str(tmp_path / "s0" / "loo.txt")) and os.path.exists(str(tmp_path / "s1" / "loo.txt"))


def _sequence(mod, arg, d, grid, iters, seed, n_pending=0):
    grid = np.array(grid, copy=True)
    values = np.zeros(grid.shape[0]) + np.nan
    done = np.zeros(grid.shape[0], dtype=bool)
    out = []
    for it in range(iters):
        ch = mod.init(str(d), arg)
        eng = LooOracleEngine()
        ch._eng = eng
        npr.seed(seed + it)
        complete = np.nonzero(done)[0][::-1]                # (not sorted: the file follows `complete`, not the grid)
        free = np.nonzero(~done)[0]
        pending = free[-n_pending:] if (n_pending and complete.shape[0] >= 2) else np.zeros(0, dtype=int)
        cand = free[:free.shape[0] - pending.shape[0]]
        job = ch.next(grid, values, values * 0, cand, pending, complete)
        state = npr.get_state()
        text = open(ch.loo_file).read() if os.path.exists(ch.loo_file) else None
        if isinstance(job, tuple):
            grid = np.vstack((grid, np.asarray(job[1], dtype=float).ravel()[None, :]))
            values, done = np.append(values, np.nan), np.append(done, False)
            idx = grid.shape[0] - 1
        else:
            idx = int(job)
        out.append({"idx": idx, "pt": grid[idx].copy(), "state": state, "rep": ch.last_loo, "eng": eng, "complete": complete,
                    "comp": grid[complete].copy(), "values": values[complete].copy(), "ch": ch, "text": text})
        values[idx] = branin(grid[idx, 0], grid[idx, 1])
        done[idx] = True
        if mod is GPEIChooser and ch.D != -1:
            ch.__del__()
    return out


@pytest.mark.parametrize("mod,arg,iters", [(GPEIChooser, "mcmc_iters=3", 5),
                                           (GPEIOptChooser, "mcmc_iters=2,burnin=3,grid_subset=3,use_multiprocessing=0", 4)])
@pytest.mark.parametrize("extra,n_pending,reuses", [("", 0, False), (",recommend=1", 0, True),
                                                    (",importance=1,importance_levels=3,importance_points=16", 0, True),
                                                    (",recommend=1,importance=1,importance_levels=3,importance_points=16", 0, True),
                                                    ("", 2, False), (",recommend=1", 2, True)])
def test_loo_changes_no_proposal_and_writes_the_report(golden_dir, tmp_path, mod, arg, iters, extra, n_pending, reuses):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:80]
    runs = {}
    for loo in (0, 1):
        d = tmp_path / ("l%d" % loo)
        d.mkdir()
        runs[loo] = _sequence(mod, arg + extra + ",loo=%d" % loo, d, grid, iters, 11, n_pending)
    for a, b in zip(runs[0], runs[1]):
        assert a["idx"] == b["idx"] and np.array_equal(a["pt"], b["pt"])
        sa, sb = a["state"], b["state"]
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]       # numpy's generator state
        assert a["rep"] is None and not a["eng"].loo_calls and a["text"] is None
        # loo=0 calls nothing new: the same factorisations as with the report
        assert a["eng"].factor_calls == b["eng"].factor_calls - (0 if reuses or not b["eng"].loo_calls else 1)
    assert not os.path.exists(str(tmp_path / "l0" / "loo.txt"))
    seen = 0
    for r in runs[1]:
        n = r["complete"].shape[0]
        if n < 2:
            assert r["rep"] is None and r["text"] is None
            continue
        seen += 1
        eng, rep, ch = r["eng"], r["rep"], r["ch"]
        (model, n_obs, n_draws, factors), = eng.loo_calls
        assert model == "objective" and n_obs == n                 # completed points only, pending jobs or not
        assert factors == eng.factor_calls                         # nothing factored after the report
        assert ch._lp_key is None and ch._factor_covers is None
        assert rep is ch.last_loo and np.array_equal(rep["grid_index"], r["complete"]) and np.array_equal(rep["y"], r["values"])
        assert rep["loo_mean"].shape == (n_draws, n)
        # the file: a header and one line per completed job in the order of `complete`; every float reads back exactly
        lines = r["text"].splitlines()
        assert r["text"].endswith("\n") and len(lines) == 1 + n
        assert lines[0].startswith("# completed=%d draws=%d elpd=" % (n, n_draws))
        head, rows = lo.parse_report(ch.loo_file) if r is runs[1][-1] else (None, None)
        for i, line in enumerate(lines[1:]):
            f = line.split()
            assert len(f) == 6 and int(f[0]) == r["complete"][i]
            want = (rep["y"][i], rep["mean"][i], np.sqrt(rep["var"][i]), rep["z_mix"][i], rep["lpd_mix"][i])
            assert [float(v) for v in f[1:]] == list(want)
            assert f[1:] == ["%.17g" % v for v in want]
        hd = dict(kv.split("=") for kv in lines[0][2:].split())
        assert list(hd) == ["completed", "draws", "elpd", "rmse", "coverage95", "outliers"]
        assert float(hd["elpd"]) == rep["elpd"] and float(hd["rmse"]) == rep["rmse"]
        assert float(hd["coverage95"]) == rep["coverage95"] and int(hd["outliers"]) == len(rep["outliers"])
        # ... and it is the oracle's report of these observations under the draws the engine was given
        want_head, want_rows = lo.report(r["complete"], eng._last_comp, r["values"], eng._last_rows)
        got_rows = np.array([[float(v) for v in ln.split()] for ln in lines[1:]])
        assert np.allclose(got_rows, want_rows, rtol=1e-12, atol=0)
        assert np.array_equal(eng._last_comp, r["comp"])
    assert seen == iters - 2
    # rewritten, not appended: the file is the LAST call's; no lock and no temporary file stay behind
    assert open(str(tmp_path / "l1" / "loo.txt")).read() == runs[1][-1]["text"]
    assert not os.path.exists(str(tmp_path / "l1" / "loo.txt.lock"))
    assert sorted(os.listdir(str(tmp_path / "l1"))) == sorted(set(os.listdir(str(tmp_path / "l0"))) | {"loo.txt"})


def test_factorisation_is_reused_or_redone(tmp_path):
    """No factorisation of its own where _recommend / _importance has just factored exactly these rows; one where nothing has
    (the one-shot grid call leaves no record) and always while a job is pending (the proposal's covers the pending rows)."""
    rs = np.random.RandomState(4)
    grid = rs.rand(60, 2)
    values = branin(grid[:, 0], grid[:, 1])
    counts = {}
    for key, extra, pending in (("plain", "", 0), ("rec", ",recommend=1", 0), ("imp", ",importance=1,importance_points=8,importance_levels=2", 0),
                                ("pend", "", 2), ("pend_rec", ",recommend=1", 2)):
        for loo in (0, 1):
            d = tmp_path / ("%s%d" % (key, loo))
            d.mkdir()
            ch = GPEIChooser.init(str(d), "mcmc_iters=2,loo=%d%s" % (loo, extra))
            eng = LooOracleEngine()
            ch._eng = eng
            npr.seed(1)
            ch.next(grid, values, values * 0, np.arange(8, 60 - pending), np.arange(60 - pending, 60), np.arange(8))
            counts[key, loo] = eng.factor_calls
            assert len(eng.loo_calls) == loo
            if loo:
                assert eng.loo_calls[0][1] == 8 and eng.fant is None
    assert counts["plain", 1] == counts["plain", 0] + 1
    assert counts["rec", 1] == counts["rec", 0] and counts["imp", 1] == counts["imp", 0]
    assert counts["pend", 1] == counts["pend", 0] + 1
    assert counts["pend_rec", 1] == counts["pend_rec", 0]


def test_report_is_rewritten_atomically(tmp_path, monkeypatch):
    """The new text is complete in a temporary file of the same directory before one rename puts it in place, under the
    chooser's lock: a reader sees the old report or the new one."""
    rs = np.random.RandomState(4)
    grid = rs.rand(30, 2)
    values = branin(grid[:, 0], grid[:, 1])
    ch = GPEIChooser.init(str(tmp_path), "mcmc_iters=2,loo=1")
    ch._eng = LooOracleEngine()
    target = str(tmp_path / "loo.txt")
    open(target, "w").write("old report\n")
    seen = []
    real = os.rename

    def rename(src, dst):
        if dst == target:
            seen.append((os.path.dirname(src), open(src).read(), open(dst).read(), os.path.exists(target + ".lock")))
        return real(src, dst)
    monkeypatch.setattr(os, "rename", rename)
    npr.seed(1)
    ch.next(grid, values, values * 0, np.arange(6, 30), np.zeros(0, dtype=int), np.arange(6))
    monkeypatch.undo()
    (src_dir, new_text, old_text, locked), = seen
    assert src_dir == str(tmp_path) and old_text == "old report\n" and locked
    assert new_text == open(target).read() and len(new_text.splitlines()) == 7
    assert not os.path.exists(target + ".lock")


@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_arguments(mod, tmp_path):
    ch = mod.init(str(tmp_path), "")
    assert (ch.loo, ch.last_loo, ch.loo_file) == (False, None, os.path.join(str(tmp_path), "loo.txt"))
    assert mod.init(str(tmp_path), "loo=1").loo is True
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), "loo=1,ndev=2")
    assert "allowed" in str(ei.value) and "ndev=1" in str(ei.value)
    with pytest.raises(ValueError):
        mod.init(str(tmp_path), "loo=yes")
    assert mod.init(str(tmp_path), "loo=0,ndev=2").loo is False


@pytest.mark.parametrize("mod", [GPEIperSecChooser, GPConstrainedEIChooser])
def test_per_second_and_constrained_choosers_refuse(mod, tmp_path):
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), "loo=1")
    assert "allowed" in str(ei.value) and "loo=0" in str(ei.value)
    assert mod.init(str(tmp_path), "loo=0").loo is False


def test_stats_html_gains_the_chart(tmp_path):
    grid = np.random.RandomState(5).rand(40, 2)
    values = branin(grid[:, 0], grid[:, 1])
    html = {}
    for loo in (0, 1):
        d = tmp_path / ("h%d" % loo)
        d.mkdir()
        ch = GPEIOptChooser.init(str(d), "mcmc_iters=2,burnin=2,grid_subset=2,loo=%d" % loo)
        ch._eng = LooOracleEngine()
        npr.seed(2)
        ch.next(grid, values, values * 0, np.arange(6, 40), np.zeros(0, dtype=int), np.arange(6))
        html[loo] = GPEIOptChooser.init(str(d), "loo=%d" % loo).generate_stats_html()
    assert html[0].endswith('bar_chart("#lschart", lsdata, 2);</script>') and "loochart" not in html[0]
    assert html[1].startswith(html[0])
    tail = html[1][len(html[0]):]
    assert '<svg id="loochart"' in tail and tail.endswith("</svg>")
    assert tail.count("<circle") == 6 and tail.count("<line") == 6 + 1        # a dot and a +- 2 std bar per job, and the diagonal
    # loo=1 but no file yet: today's snippet, byte for byte
    os.remove(str(tmp_path / "h1" / "loo.txt"))
    assert GPEIOptChooser.init(str(tmp_path / "h1"), "loo=1").generate_stats_html() == html[0]
