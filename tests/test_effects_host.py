"""The main-effects report on a CPU-only box: the estimator against an analytic case, the arithmetic Engine.main_effects
defines its summary by, the summation order the device must reproduce, the C ABI's argument checks (spx_create touches no
GPU), and the choosers' importance= arguments on an oracle-backed engine."""
import ctypes
import os

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine
from spearmint_amd.chooser import GPConstrainedEIChooser, GPEIChooser, GPEIOptChooser, GPEIperSecChooser
from tests import effects_oracle as eo
from tests.effects_helpers import EffectsOracleEngine
from tests.helpers import branin, np_mean_device_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the estimator means something ---------------------------------------------------------------------------------------
def _analytic_case():
    rng = np.random.RandomState(7)
    comp = rng.rand(60, 3)
    vals = 3 * comp[:, 0] + np.sin(2 * np.pi * comp[:, 1]) + 0.01 * rng.randn(60)
    hyper = np.array([[np.mean(vals), 1e-4, np.var(vals), 1.0, 0.4, 1.8]])
    return comp, vals, hyper


def test_first_order_indices_of_an_additive_function(golden_dir):
    """f = 3 x0 + sin(2 pi x1): Var = 9/12 + 1/2, first-order indices 0.6 / 0.4 / 0.  With the 256-point Sobol prefix the
    oracle gave 0.594 / 0.398 / 3.7e-5 (error 0.006); the bound is three times that -- room for BLAS differences, not for a
    wrong formula.  The same estimate from 256 pseudo-random base points was off by up to 0.14: total_var over Q points is
    the noisy term, which is why the choosers pass the Sobol prefix of the grid."""
    comp, vals, hyper = _analytic_case()
    base = np.ascontiguousarray(np.load(os.path.join(golden_dir, "sobol.npz"))["jk_8x300_s1"][:3, :256].T)
    rep = eo.main_effects(comp, vals, hyper, base, T=8)
    assert rep["curves"].shape == (1, 3, 8) and rep["base_mean"].shape == (1, 256)
    print("first_order", rep["first_order"][0])
    assert np.all(np.abs(rep["first_order"][0] - np.array([0.6, 0.4, 0.0])) <= 0.02)
    # the curves themselves: a line of slope 3 and a sine, each about its own mean
    lv = rep["levels"]
    c = rep["curves"][0] - np.mean(rep["curves"][0], axis=1)[:, None]
    assert np.max(np.abs(c[0] - 3 * (lv - 0.5))) < 0.1 and np.max(np.abs(c[1] - (np.sin(2 * np.pi * lv) - np.mean(np.sin(2 * np.pi * lv))))) < 0.1
    assert np.max(np.abs(c[2])) < 0.05


# ---- engine arithmetic ---------------------------------------------------------------------------------------------------
def test_summary_is_the_four_numpy_expressions():
    rs = np.random.RandomState(3)
    curves, base_mean, levels = rs.randn(4, 3, 5), rs.randn(4, 9), eo.midpoints(5)
    base_mean[2, :] = 1.25                   # total_var == 0: numpy's own x/0
    curves[2, 1, :] = -0.5                   # ... and 0/0
    rep = engine.effects_summary(levels, curves, base_mean)
    assert rep["levels"] is levels and rep["curves"] is curves and rep["base_mean"] is base_mean
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(rep["f0"], np.mean(base_mean, axis=1))
        assert np.array_equal(rep["total_var"], np.var(base_mean, axis=1))
        assert np.array_equal(rep["effect_var"], np.var(curves, axis=2))
        want = np.var(curves, axis=2) / np.var(base_mean, axis=1)[:, None]
    assert np.array_equal(np.isnan(rep["first_order"]), np.isnan(want))
    assert np.array_equal(rep["first_order"][~np.isnan(want)], want[~np.isnan(want)])
    assert np.isnan(rep["first_order"][2, 1]) and np.all(np.isinf(rep["first_order"][2, [0, 2]]))
    assert sorted(rep) == sorted(eo.summary(levels, curves, base_mean))


@pytest.mark.parametrize("Q", [1, 7, 8, 9, 128, 129, 300])
def test_block_mean_is_numpys_pairwise_sum_and_one_division(Q):
    """np.mean over the last axis of (H, D, T, Q) == np.add.reduce over each block / Q, and both are the walk csrc/np_sum.h
    restates (tests/helpers.np_mean_device_order mirrors the kernel): the order k_effects_mean must reproduce."""
    H, D, T = 2, 3, 2
    x = np.random.RandomState(100 + Q).randn(H * D * T * Q) * np.exp(np.random.RandomState(Q).randn(H * D * T * Q) * 3)
    got = np.mean(x.reshape(H, D, T, Q), axis=-1)
    blocks = x.reshape(-1, Q)
    by_block = np.array([np.add.reduce(b) / Q for b in blocks]).reshape(H, D, T)
    assert np.array_equal(got, by_block)
    mirror = np.array([np_mean_device_order(b) for b in blocks]).reshape(H, D, T)
    assert np.array_equal(got, mirror)


def test_rows_are_in_the_documented_order():
    base = np.arange(6, dtype=float).reshape(3, 2) / 10
    rows = eo.structured_rows(base, [0.25, 0.75])
    assert rows.shape == ((2 * 2 + 1) * 3, 2)
    for j in range(2):
        for k in range(2):
            for q in range(3):
                want = base[q].copy()
                want[j] = (0.25, 0.75)[k]
                assert np.array_equal(rows[(j * 2 + k) * 3 + q], want)
    assert np.array_equal(rows[12:], base)


# ---- argument checks with no GPU -------------------------------------------------------------------------------------------
def _err(lib):
    return lib.spx_last_error().decode()


def test_argument_and_call_order_checks_touch_no_device():
    lib = engine.load_library()
    h = ctypes.c_void_p()
    assert lib.spx_create(0, ctypes.byref(h)) == 0
    base, levels, curves, bm = np.zeros((4, 2)), np.zeros(3), np.zeros((1, 2, 3)), np.zeros((1, 4))
    dp = engine._dp
    call = lib.spx_main_effects
    assert call(None, dp(base), 4, dp(levels), 3, dp(curves), dp(bm)) == engine.SPX_ERR_ARG
    for args in ((None, 4, dp(levels), 3, dp(curves), dp(bm)), (dp(base), 4, None, 3, dp(curves), dp(bm)),
                 (dp(base), 4, dp(levels), 3, None, dp(bm))):
        assert call(h, *args) == engine.SPX_ERR_ARG and "NULL" in _err(lib)
    for q in (0, -3, (128 << 12) + 1):
        assert call(h, dp(base), q, dp(levels), 3, dp(curves), dp(bm)) == engine.SPX_ERR_ARG and "Q=" in _err(lib)
    for t in (0, -1):
        assert call(h, dp(base), 4, dp(levels), t, dp(curves), dp(bm)) == engine.SPX_ERR_ARG and "T=" in _err(lib)
    # everything in order but no factorisation: a call-order error, not a device error -- the handle is still lazy (on a box
    # without a GPU an initialisation would have answered SPX_ERR_HIP)
    assert call(h, dp(base), 4, dp(levels), 3, dp(curves), None) == engine.SPX_ERR_ARG and "spx_factor" in _err(lib)
    lib.spx_destroy(h)


def test_engine_method_and_multi_handle():
    assert "spx_main_effects" in engine.ABI
    eng = engine.Engine(0)
    with pytest.raises(ValueError):
        eng.main_effects(np.zeros((4, 2)))               # no observations: D unknown
    eng.close()
    multi = engine.MultiEngine([0, 0])                   # (repeated ids: creation touches no GPU)
    multi.D, multi.H = 2, 1
    with pytest.raises(ValueError) as ei:
        multi.main_effects(np.zeros((4, 2)), T=3)
    assert "single-GPU" in str(ei.value)
    multi.close()


def test_effects_plan_splits_and_stages(tmp_path):
    """spx_plan.h: plan_effects is a pure function -- compiled here for the host."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "p.cpp"
    src.write_text('#include <stdio.h>\n#include "spx_plan.h"\n'
                   "int main() { EffectsShape s; s.D = 3; s.H = 2; s.Q = 9; s.T = 5; s.pass_rows_opt = 50;\n"
                   "  EffectsPlan p = plan_effects(s);\n"
                   '  printf("%lld %lld %lld %d %d %d %d\\n", (long long)p.rows, (long long)p.nblocks, (long long)p.pass_rows, p.npass,\n'
                   "         (int)p.gather, (int)p.mean_lds, p.wg_blocks);\n"
                   "  s.pass_rows_opt = 0; s.Q = 7000; p = plan_effects(s);\n"
                   '  printf("%d %d %d %d\\n", p.npass, (int)p.gather, (int)p.mean_lds, p.wg_blocks);\n'
                   "  s.Q = 256; p = plan_effects(s);\n"
                   '  printf("%d %d %zu\\n", (int)p.mean_lds, p.wg_blocks, p.lds_bytes); return 0; }\n')
    exe = str(tmp_path / "p")
    subprocess.check_call([gxx, "-std=c++17", "-I", os.path.join(ROOT, "spearmint_amd", "csrc"), str(src), "-o", exe])
    out = subprocess.check_output([exe]).decode().split("\n")
    assert out[0].split() == ["144", "15", "50", "3", "1", "1", "256"]
    assert out[1].split() == ["1", "0", "0", "256"]          # a block longer than the LDS tile is walked from memory
    assert out[2].split() == ["1", "23", str(23 * 257 * 8)]


# ---- choosers ----------------------------------------------------------------------------------------------------------------
def _sequence(mod, arg, d, grid, iters, seed, n_pending=0):
    grid = np.array(grid, copy=True)
    values = np.zeros(grid.shape[0]) + np.nan
    done = np.zeros(grid.shape[0], dtype=bool)
    out = []
    for it in range(iters):
        ch = mod.init(str(d), arg)
        eng = EffectsOracleEngine()
        ch._eng = eng
        npr.seed(seed + it)
        complete = np.nonzero(done)[0]
        free = np.nonzero(~done)[0]
        pending = free[-n_pending:] if (n_pending and complete.shape[0] >= 2) else np.zeros(0, dtype=int)
        cand = free[:free.shape[0] - pending.shape[0]]
        job = ch.next(grid, values, values * 0, cand, pending, complete)
        state = npr.get_state()
        if isinstance(job, tuple):
            grid = np.vstack((grid, np.asarray(job[1], dtype=float).ravel()[None, :]))
            values, done = np.append(values, np.nan), np.append(done, False)
            idx = grid.shape[0] - 1
        else:
            idx = int(job)
        out.append((idx, grid[idx].copy(), state, ch.last_importance, eng, int(complete.shape[0]), ch))
        values[idx] = branin(grid[idx, 0], grid[idx, 1])
        done[idx] = True
        if mod is GPEIChooser and ch.D != -1:
            ch.__del__()
    return out


@pytest.mark.parametrize("mod,arg,iters", [(GPEIChooser, "mcmc_iters=3", 5),
                                           (GPEIOptChooser, "mcmc_iters=2,burnin=3,grid_subset=3,use_multiprocessing=0", 4)])
@pytest.mark.parametrize("extra,n_pending", [("", 0), (",recommend=1", 0), ("", 2)])
def test_importance_changes_no_proposal_and_draws_no_random_numbers(golden_dir, tmp_path, mod, arg, iters, extra, n_pending):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:80]
    runs = {}
    for imp in (0, 1):
        d = tmp_path / ("i%d" % imp)
        d.mkdir()
        runs[imp] = _sequence(mod, arg + extra + ",importance=%d,importance_levels=4,importance_points=32" % imp, d, grid, iters,
                              11, n_pending)
    for a, b in zip(runs[0], runs[1]):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        assert a[2][0] == b[2][0] and np.array_equal(a[2][1], b[2][1]) and a[2][2:] == b[2][2:]     # numpy's generator state
        assert a[3] is None and not a[4].effects_calls
    assert not os.path.exists(str(tmp_path / "i0" / "importance.txt"))
    seen = 0
    for idx, pt, state, rep, eng, n_complete, ch in runs[1]:
        if n_complete < 2:
            assert rep is None
            continue
        seen += 1
        (base, n_obs, n_draws, factors), = eng.effects_calls
        assert np.array_equal(base, grid[:32]) and n_obs == n_complete      # the Sobol prefix; completed points only
        H = n_draws
        assert rep["curves"].shape == (H, 2, 4) and rep["base_mean"].shape == (H, 32) and np.all(np.isfinite(rep["curves"]))
        assert np.array_equal(rep["levels"], eo.midpoints(4))
        assert np.array_equal(rep["first_order_mean"], np.mean(rep["first_order"], axis=0))
        assert np.array_equal(rep["first_order_std"], np.std(rep["first_order"], axis=0))
        assert np.array_equal(rep["curves_mean"], np.mean(rep["curves"], axis=0))
        # one factorisation for the report -- none where the recommendation has just factored the same inputs
        assert ch._lp_key is None
        # (the proposal factors through the resident calls only with pending jobs: once per grid pass)
        proposal = 0 if not n_pending else (2 if mod is GPEIOptChooser else 1)
        assert factors == eng.factor_calls == proposal + 1
        if extra:
            assert ch.last_recommendation is not None
    assert seen == iters - 2
    # the file holds the LAST call's report, 1 + D lines that parse back
    rep, n_complete = runs[1][-1][3], runs[1][-1][5]
    lines = open(str(tmp_path / "i1" / "importance.txt")).read().splitlines()
    assert len(lines) == 1 + 2 and lines[0].startswith("# ")
    head = dict(kv.split("=") for kv in lines[0][2:].split())
    assert (int(head["completed"]), int(head["draws"]), int(head["levels"]), int(head["points"])) == (n_complete, rep["curves"].shape[0], 4, 32)
    assert float(head["f0"]) == np.mean(rep["f0"]) and float(head["total_var"]) == np.mean(rep["total_var"])
    for j, line in enumerate(lines[1:]):
        f = line.split()
        assert int(f[0]) == j and len(f) == 4 + 4
        assert float(f[1]) == rep["first_order_mean"][j] and float(f[2]) == rep["first_order_std"][j]
        assert float(f[3]) == np.mean(rep["effect_var"], axis=0)[j]
        assert np.array_equal([float(v) for v in f[4:]], rep["curves_mean"][j])
    assert not os.path.exists(str(tmp_path / "i1" / "importance.txt.lock"))
    assert sorted(os.listdir(str(tmp_path / "i1"))) == sorted(set(os.listdir(str(tmp_path / "i0"))) | {"importance.txt"})   # no temporary file left


def test_report_factors_once_without_a_recommendation(tmp_path):
    rs = np.random.RandomState(4)
    grid = rs.rand(60, 2)
    values = branin(grid[:, 0], grid[:, 1])
    ch = GPEIChooser.init(str(tmp_path), "mcmc_iters=2,importance=1,importance_points=1000,importance_levels=3,acq=PI,acq_par=0.01")
    eng = EffectsOracleEngine()
    ch._eng = eng
    npr.seed(1)
    ch.next(grid, values, values * 0, np.arange(8, 60), np.zeros(0, dtype=int), np.arange(8))
    assert eng.factor_calls == 1 and len(eng.effects_calls) == 1
    assert eng.effects_calls[0][0].shape == (60, 2)                    # min(Q, len(grid)) rows
    assert eng.get_acquisition() == (engine.ACQ_PI, 0.01)              # the report does not touch the setting
    assert ch.last_importance["curves"].shape == (2, 2, 3)


@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_arguments(mod, tmp_path):
    ch = mod.init(str(tmp_path), "")
    assert (ch.importance, ch.importance_levels, ch.importance_points, ch.last_importance) == (False, 16, 256, None)
    ch = mod.init(str(tmp_path), "importance=1,importance_levels=8,importance_points=64")
    assert (ch.importance, ch.importance_levels, ch.importance_points) == (True, 8, 64)
    for args in ("importance=1,importance_levels=0", "importance_levels=x", "importance_points=0", "importance=1,importance_points=%d" % ((128 << 12) + 1),
                 "importance=1,ndev=2"):
        with pytest.raises(ValueError) as ei:
            mod.init(str(tmp_path), args)
        assert "allowed" in str(ei.value), args
    assert mod.init(str(tmp_path), "importance=0,ndev=2").importance is False


@pytest.mark.parametrize("mod", [GPEIperSecChooser, GPConstrainedEIChooser])
def test_per_second_and_constrained_choosers_refuse(mod, tmp_path):
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), "importance=1")
    assert "allowed" in str(ei.value) and "importance=0" in str(ei.value)
    assert mod.init(str(tmp_path), "importance=0").importance is False


def test_stats_html_gains_the_second_chart(tmp_path):
    grid = np.random.RandomState(5).rand(40, 2)
    values = branin(grid[:, 0], grid[:, 1])
    html = {}
    for imp in (0, 1):
        d = tmp_path / ("h%d" % imp)
        d.mkdir()
        ch = GPEIOptChooser.init(str(d), "mcmc_iters=2,burnin=2,grid_subset=2,importance=%d,importance_levels=3,importance_points=16" % imp)
        ch._eng = EffectsOracleEngine()
        npr.seed(2)
        ch.next(grid, values, values * 0, np.arange(6, 40), np.zeros(0, dtype=int), np.arange(6))
        html[imp] = GPEIOptChooser.init(str(d), "importance=%d" % imp).generate_stats_html()
        if imp:
            first = ch.last_importance["first_order_mean"]
    assert html[0].endswith('bar_chart("#lschart", lsdata, 2);</script>') and "#sensitivity" not in html[0]
    assert html[1].startswith(html[0])
    tail = html[1][len(html[0]):]
    assert '<div id="sensitivity"></div>' in tail and tail.endswith('bar_chart("#sensitivity", sdata, 1);</script>')
    assert "var sdata = [" + ",".join("%.2f" % v for v in first) + "];" in tail
    # importance=1 but no file yet: today's snippet, byte for byte
    os.remove(str(tmp_path / "h1" / "importance.txt"))
    assert GPEIOptChooser.init(str(tmp_path / "h1"), "importance=1").generate_stats_html() == html[0]
