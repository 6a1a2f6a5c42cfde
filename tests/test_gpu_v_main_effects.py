"""spx_main_effects on the MI355X: bit for bit the host-orchestrated form through the entry points that existed before it
(the rows built on the host, spx_set_candidates, spx_ei_run(KEEP_MOMENTS), spx_get_moments, np.mean over each block) at every
shape where the row kernel, the pass or the reduction takes another path; every split of the rows into passes; the oracle;
the handle's state before and after; and the choosers' importance=1 end to end.  Every case is a few milliseconds of
device work."""
import os

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine as spx
from spearmint_amd.synthetic import synthetic_problem
from tests import effects_oracle as eo
from tests.effects_helpers import host_form, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = spx.Engine(0)   # raises if libspx.so or the GPU is missing -- no fallback
    yield e
    e.close()


def _problem(eng, N, D, H, Q, T, seed, covar="Matern52"):
    comp, _, vals, hypers = synthetic_problem(N, 1, D, H, seed, near=0)
    rs = np.random.RandomState(seed + 1)
    base, levels = rs.rand(Q, D), rs.rand(T)
    eng.set_covar(covar)
    eng.set_observations(comp, vals)
    eng.set_hypers(hypers)
    eng.factor()
    return comp, vals, hypers, base, levels


def _both(eng, base, levels):
    want = host_form(eng, base, levels)
    got = eng.main_effects(base, levels)
    return got, want


def _assert_contract(got, want):
    assert got["curves"].shape == want[0].shape and got["base_mean"].shape == want[1].shape
    assert same_bits(got["curves"], want[0]), np.max(np.abs(got["curves"] - want[0]))
    assert same_bits(got["base_mean"], want[1])


# ---- 1. the contract, bit for bit ---------------------------------------------------------------------------------------------
# N: the fused pass (20), its boundary (128), the GEMM path with a partial last block (129, 300).  D: across the 8-dimension
# padding.  Q: the leaves (< 8, 8, 9 ... 128) and the first split (129, 300) of numpy's pairwise sum; 6200: a block longer
# than k_effects_mean's LDS tile, walked from memory.  Totals that are no multiple of 128.
@pytest.mark.parametrize("N,D,H,T,Q", [(20, 1, 1, 1, 1), (20, 3, 3, 5, 7), (128, 9, 1, 5, 8), (129, 3, 3, 1, 9),
                                       (129, 33, 1, 5, 129), (300, 9, 3, 5, 300), (300, 1, 3, 5, 129), (128, 33, 3, 1, 7),
                                       (20, 3, 1, 5, 6200), (300, 3, 1, 1, 6200)])
def test_contract_bit_for_bit(eng, N, D, H, T, Q):
    comp, vals, hypers, base, levels = _problem(eng, N, D, H, Q, T, 2000 + N + D)
    got, want = _both(eng, base, levels)
    assert got["curves"].shape == (H, D, T) and got["base_mean"].shape == (H, Q)
    _assert_contract(got, want)
    assert np.all(np.isfinite(got["curves"])) and np.all(np.isfinite(got["base_mean"]))
    assert eng.stat("last_effects_rows") == (D * T + 1) * Q and eng.stat("last_effects_passes") == 1
    assert eng.stat("last_step_fused") == (1 if N <= 128 else 0)
    # the summary is the four numpy expressions
    ref = eo.summary(levels, got["curves"], got["base_mean"])
    for k in ("f0", "total_var", "effect_var", "first_order"):
        assert same_bits(got[k], ref[k]), k


def test_default_levels_are_the_midpoints(eng):
    comp, vals, hypers, base, _ = _problem(eng, 40, 2, 2, 16, 4, 2100)
    got = eng.main_effects(base, T=4)
    assert np.array_equal(got["levels"], (np.arange(4) + 0.5) / 4)
    _assert_contract(got, host_form(eng, base, got["levels"]))


# ---- 2. every covar -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE", "SE"])
def test_every_covar(eng, covar):
    try:
        comp, vals, hypers, base, levels = _problem(eng, 150, 5, 2, 40, 3, 2200, covar)
        got, want = _both(eng, base, levels)
        _assert_contract(got, want)
    finally:
        eng.set_covar("Matern52")


# ---- 3. the split -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 300])
def test_split_into_passes_and_chunks_gives_the_same_bits(eng, N):
    """2064 rows in blocks of 129.  effects_pass_rows = 700: three passes whose boundaries (700, 1400) cut blocks;
    kstar_budget_bytes for 256 candidates per chunk: every pass itself has three chunks (256, 512 cut blocks too)."""
    D, H, T, Q = 3, 3, 5, 129
    comp, vals, hypers, base, levels = _problem(eng, N, D, H, Q, T, 2300 + N)
    one = eng.main_effects(base, levels)
    assert eng.stat("last_effects_passes") == 1
    Np = -(-N // 128) * 128
    try:
        for pass_rows, budget, passes in ((700, 0, 3), (700, 8 * Np * 256, 3), (0, 8 * Np * 256, 1), (129, 0, 16)):
            eng.set_option("effects_pass_rows", pass_rows)
            eng.set_option("kstar_budget_bytes", budget)
            got = eng.main_effects(base, levels)
            assert eng.stat("last_effects_passes") == passes
            assert same_bits(got["curves"], one["curves"]) and same_bits(got["base_mean"], one["base_mean"]), (pass_rows, budget)
    finally:
        eng.set_option("effects_pass_rows", 0)
        eng.set_option("kstar_budget_bytes", 0)
    _assert_contract(one, host_form(eng, base, levels))


# ---- 4. invariants, bit for bit -----------------------------------------------------------------------------------------------
def test_invariants(eng):
    D, H, T, Q = 4, 3, 5, 33
    comp, vals, hypers, base, levels = _problem(eng, 300, D, H, Q, T, 2400)
    one = eng.main_effects(base, levels)

    def same(got):
        return same_bits(got["curves"], one["curves"]) and same_bits(got["base_mean"], one["base_mean"])
    assert same(eng.main_effects(base, levels))                      # a second call
    for kind, par in ((spx.ACQ_PI, 0.01), (spx.ACQ_LCB, 2.0)):       # the acquisition setting: not read, not changed
        eng.set_acquisition(kind, par)
        assert same(eng.main_effects(base, levels))
        assert eng.get_acquisition() == (kind, par)
    eng.set_acquisition(spx.ACQ_EI)
    try:
        for streams in (2, 3, 1):
            for partial in (0, 1):
                eng.set_option("streams", streams)
                eng.set_option("gemm_partial", partial)
                assert same(eng.main_effects(base, levels)), (streams, partial)
    finally:
        eng.set_option("streams", 1)
        eng.set_option("gemm_partial", -1)
    # the factor of spx_ei_step in place of spx_factor's
    eng.set_candidates(base)
    eng.ei_step()
    assert same(eng.main_effects(base, levels))


def test_nan_in_one_base_row(eng):
    """base[q0][c0] = NaN: every row made from base[q0] is NaN except where coordinate c0 is the substituted one.  NaN are
    exactly the blocks (j != c0, k) and base_mean[:, q0]; every other value keeps its bits."""
    D, H, T, Q = 3, 2, 4, 20
    comp, vals, hypers, base, levels = _problem(eng, 200, D, H, Q, T, 2500)
    clean = eng.main_effects(base, levels)
    bad = base.copy()
    q0, c0 = 11, 1
    bad[q0, c0] = np.nan
    got, want = _both(eng, bad, levels)
    _assert_contract(got, want)
    nan_c = np.zeros((H, D, T), dtype=bool)
    nan_c[:, [j for j in range(D) if j != c0], :] = True
    nan_b = np.zeros((H, Q), dtype=bool)
    nan_b[:, q0] = True
    assert np.array_equal(np.isnan(got["curves"]), nan_c) and np.array_equal(np.isnan(got["base_mean"]), nan_b)
    assert np.array_equal(got["curves"][~nan_c], clean["curves"][~nan_c])
    assert np.array_equal(got["base_mean"][~nan_b], clean["base_mean"][~nan_b])


# ---- 5. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,Q,T", [("a", 64, 5), ("c", 300, 2)])
def test_against_the_oracle(eng, golden_dir, case, Q, T):
    """Where tests/test_gpu_a_parity.py holds func_m to rtol 1e-9 / atol 1e-10 (the ei_small_* goldens), curves and
    base_mean are within the same tolerance of tests/effects_oracle.py."""
    g = np.load(os.path.join(golden_dir, "ei_small_%s.npz" % case))
    eng.set_observations(g["comp"], g["vals"])
    eng.set_hypers(g["hypers"])
    eng.factor()
    base = np.ascontiguousarray(g["cand"][:Q])
    got = eng.main_effects(base, T=T)
    ref = eo.main_effects(g["comp"], g["vals"], g["hypers"], base, T=T)
    err_c, err_b = np.max(np.abs(got["curves"] - ref["curves"])), np.max(np.abs(got["base_mean"] - ref["base_mean"]))
    print("max abs error: curves %.3e base_mean %.3e" % (err_c, err_b))
    assert np.allclose(got["curves"], ref["curves"], rtol=1e-9, atol=1e-10)
    assert np.allclose(got["base_mean"], ref["base_mean"], rtol=1e-9, atol=1e-10)


# ---- 6. state -----------------------------------------------------------------------------------------------------------------
def _refused(eng, fn, *a, **k):
    with pytest.raises(ValueError) as ei:
        fn(*a, **k)
    assert eng._lib.spx_last_error()
    return str(ei.value)


def test_state_after_the_call(eng):
    comp, cand, vals, hypers = synthetic_problem(150, 400, 3, 3, 2600)
    base, levels = cand[:32], eo.midpoints(4)
    eng.set_observations(comp, vals); eng.set_candidates(cand); eng.set_hypers(hypers)
    eng.ei_step(spx.FLAG_KEEP_MOMENTS)
    best, mean, mom = eng.best(), eng.ei_mean(), eng.get_moments(1)
    f0, g0 = eng.ei_grad_batch(cand[:5])
    eng.main_effects(base, levels)
    for fn, args in ((eng.best, ()), (eng.ei_mean, ()), (eng.ei_draws, ()), (eng.get_moments, (0,)), (eng.ei_run, ()),
                     (eng.ei_run, (spx.FLAG_KEEP_MOMENTS,))):
        _refused(eng, fn, *args)
    f1, g1 = eng.ei_grad_batch(cand[:5])                             # the factor stays: the bits it returned before
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)
    eng.set_candidates(cand)                                         # and a pass works again
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    assert eng.best() == best and np.array_equal(eng.ei_mean(), mean)
    assert np.array_equal(eng.get_moments(1)[0], mom[0]) and np.array_equal(eng.get_moments(1)[1], mom[1])


def test_refusals_leave_everything_held(eng):
    comp, cand, vals, hypers = synthetic_problem(60, 300, 2, 2, 2700)
    base = cand[:16]
    N, H = comp.shape[0], hypers.shape[0]
    # before any factorisation
    eng.set_observations(comp, vals); eng.set_candidates(cand); eng.set_hypers(hypers)
    assert "spx_factor" in _refused(eng, eng.main_effects, base, T=3)
    eng.factor()
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    held = (eng.best(), eng.ei_mean(), eng.get_moments(0)[0])
    # bad arguments with everything held
    for kw in ({"levels": np.zeros(0)},):
        _refused(eng, eng.main_effects, base, **kw)
    assert eng._lib.spx_main_effects(eng._h, spx._dp(base), 0, spx._dp(np.zeros(3)), 3, spx._dp(np.zeros(99)), None) == spx.SPX_ERR_ARG
    assert eng.best() == held[0] and np.array_equal(eng.ei_mean(), held[1]) and np.array_equal(eng.get_moments(0)[0], held[2])
    # fantasies held
    fant = np.repeat(np.repeat(vals[None, :, None], H, axis=0), 2, axis=2)
    eng.set_fantasies(fant, np.full((H, 2), np.min(vals)))
    eng.ei_run()
    held = (eng.best(), eng.ei_mean())
    assert "fantasies" in _refused(eng, eng.main_effects, base, T=3)
    assert eng.best() == held[0] and np.array_equal(eng.ei_mean(), held[1])
    eng.ei_run()                                                     # the fantasies and the candidates are still there
    assert eng.best() == held[0]
    eng.set_fantasies(None, None)
    eng.main_effects(base, T=3)                                      # ... and without them the call goes through
    # a two-slot multi-device handle (repeated device id)
    me = spx.MultiEngine([0, 0])
    try:
        me.set_observations(comp, vals); me.set_candidates(cand); me.set_hypers(hypers)
        me.factor(); me.ei_run()
        held = (me.best(), me.ei_mean())
        assert "single-GPU" in _refused(me, me.main_effects, base, T=3)
        assert me.best() == held[0] and np.array_equal(me.ei_mean(), held[1])
        me.ei_run()
        assert me.best() == held[0]
    finally:
        me.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_opt_chooser_on_branin(golden_dir, tmp_path):
    from spearmint_amd.chooser import GPEIOptChooser
    from tests.helpers import run_trajectory
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"]
    args = "mcmc_iters=3,burnin=5,grid_subset=4,use_multiprocessing=0"
    runs, last = {}, {}
    for tag, extra in (("plain", ""), ("report", ",importance=1,recommend=1,importance_levels=8,importance_points=128")):
        d = tmp_path / tag
        d.mkdir()

        def make(d=d, extra=extra, tag=tag):
            ch = GPEIOptChooser.init(str(d), args + extra)
            if last.get(tag) is not None:
                last[tag].engine().close()
            last[tag] = ch
            return ch
        runs[tag] = run_trajectory(make, grid, 5, 31)
    for a, b in zip(runs["plain"], runs["report"]):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    ch = last["report"]
    rep = ch.last_importance
    assert rep["curves"].shape == (3, 2, 8) and rep["base_mean"].shape == (3, 128)
    assert np.all(np.isfinite(rep["curves"])) and np.all(np.isfinite(rep["first_order_mean"]))
    assert ch.last_recommendation is not None
    lines = open(os.path.join(str(tmp_path / "report"), "importance.txt")).read().splitlines()
    assert len(lines) == 3 and lines[0].startswith("# completed=4 draws=3 levels=8 points=128 ")
    assert [float(v) for v in lines[2].split()[4:]] == list(rep["curves_mean"][1])
    assert not os.path.exists(os.path.join(str(tmp_path / "plain"), "importance.txt"))
    for c in last.values():
        c.engine().close()
