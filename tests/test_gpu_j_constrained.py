"""GPConstrainedEIChooser on the GPU: P(feasible) and EI x P of the SPX_FLAG_CONSTRAINED pass against the oracle
(tests/constrained_oracle.py, itself held to the reference's own vectors), the reference's next() sequences through
the drop-in module, and the argument checks of the new entry points."""
import importlib
import os
import sys

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import hostgp
from tests import constrained_oracle as co
from tests.test_gpu_a_parity import assert_ei_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVARS = ["Matern52", "Matern32", "ARDSE", "SE"]


@pytest.fixture()
def eng():
    from spearmint_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _problem(seed, n_full, n_bad, M, D, H):
    rs = np.random.RandomState(seed)
    comp = rs.rand(n_full, D)
    vals = np.sum((comp - 0.4) ** 2, axis=1) + 0.02 * rs.randn(n_full)
    labels = np.ones(n_full)
    if n_bad:
        labels[rs.choice(n_full, n_bad, replace=False)] = 0
    cand = rs.rand(M, D)
    rows = np.column_stack((rs.uniform(0.1, 0.3, H), rs.uniform(1e-3, 1e-2, H), rs.uniform(0.5, 1.5, H),
                            rs.uniform(0.3, 1.5, (H, D))))
    crows = np.column_stack((rs.uniform(0.5, 3.0, H), np.full(H, 1e-3), rs.uniform(0.5, 2.0, H),
                             rs.uniform(0.3, 1.5, (H, D))))
    ff = rs.randn(n_full) * 1.5
    return comp, vals, labels, cand, rows, crows, ff


def _run(eng, covar, comp, vals, labels, cand, rows, crows, ff, pend=None, randn=None):
    from spearmint_amd.engine import FLAG_CONSTRAINED, FLAG_KEEP_MOMENTS
    good = labels > 0
    all_valid = bool(np.all(good))
    compv, valsv = comp[good], vals[good]
    eng.set_covar(covar)
    H = rows.shape[0]
    if pend is None or pend.shape[0] == 0:
        eng.set_observations(compv, valsv)
    else:
        eng.set_observations(np.concatenate((compv, pend)), np.concatenate((valsv, np.zeros(pend.shape[0]))))
    eng.set_candidates(cand)
    eng.set_hypers(rows)
    if all_valid:
        eng.set_constraint_model(np.zeros((0, comp.shape[1])), np.zeros(0), crows)
    else:
        eng.set_constraint_model(comp, ff, crows)
    if pend is None or pend.shape[0] == 0:
        eng.ei_step(FLAG_CONSTRAINED | FLAG_KEEP_MOMENTS)
        P = np.stack([eng.get_constraint_prob(h) for h in range(H)], axis=1)
    else:
        eng.factor()
        n = compv.shape[0]
        fant = np.empty((H, n + pend.shape[0], randn[0].shape[1]))
        bests = np.empty((H, randn[0].shape[1]))
        for h in range(H):
            l_rows, gam = eng.get_factor_rows(h, n, pend.shape[0])
            fant[h], bests[h] = hostgp.fantasize_from_factor_rows(valsv, rows[h], l_rows, gam, randn[h])
        eng.set_fantasies(fant, bests)
        eng.ei_run(FLAG_CONSTRAINED)
        P = None
    idx, _ = eng.best()
    return eng.ei_draws(), P, idx


def assert_product_close(got, ref):
    """EI x P: rtol 1e-9 where EI is not in its far tail; below 1e-20 the cancellation in u Phi(u) + phi(u) costs the
    oracle and the GPU alike a few digits (1.4e-9 relative seen at 1e-40), so the project's EI tolerance holds there."""
    assert_ei_close(got, ref)
    big = np.isfinite(ref) & (ref >= 1e-20)
    np.testing.assert_allclose(got[big], ref[big], rtol=1e-9, atol=0)


def _oracle(covar, comp, vals, labels, cand, rows, crows, ff, pend=None, randn=None):
    pend = np.zeros((0, comp.shape[1])) if pend is None else pend
    all_valid = bool(np.all(labels > 0))
    ei = np.stack([co.compute_constrained_ei(covar, comp, vals, labels, pend, cand, ff, rows[h], crows[h],
                                             None if randn is None else randn[h]) for h in range(rows.shape[0])], axis=1)
    P = np.stack([np.broadcast_to(co.constraint_prob(covar, comp, ff, crows[h], cand, all_valid), (cand.shape[0],))
                  for h in range(rows.shape[0])], axis=1)
    return ei, P


@pytest.mark.parametrize("covar", COVARS)
@pytest.mark.parametrize("n_full,n_bad", [(44, 7), (129, 40), (300, 57)])
def test_probability_and_product_match_oracle(eng, covar, n_full, n_bad):
    comp, vals, labels, cand, rows, crows, ff = _problem(n_full + len(covar), n_full, n_bad, 3000, 3, 4)
    draws, P, idx = _run(eng, covar, comp, vals, labels, cand, rows, crows, ff)
    ei_o, P_o = _oracle(covar, comp, vals, labels, cand, rows, crows, ff)
    np.testing.assert_allclose(P, P_o, rtol=1e-9, atol=0)
    assert_product_close(draws, ei_o)
    assert idx == int(np.argmax(np.mean(ei_o, axis=1)))


def test_all_valid_factor_is_phi_of_gain(eng):
    comp, vals, labels, cand, rows, crows, ff = _problem(5, 37, 0, 700, 2, 3)
    draws, P, idx = _run(eng, "Matern52", comp, vals, labels, cand, rows, crows, ff)
    ei_o, P_o = _oracle("Matern52", comp, vals, labels, cand, rows, crows, ff)
    np.testing.assert_allclose(P, P_o, rtol=1e-12)
    assert not np.allclose(P[:, 0], P[:, 1])             # each draw weighted by its own gain (quirk 3)
    assert_product_close(draws, ei_o)


def test_fantasies_match_oracle(eng):
    comp, vals, labels, cand, rows, crows, ff = _problem(8, 61, 11, 1500, 2, 3)
    pend = np.random.RandomState(3).rand(3, 2)
    npr.seed(4)
    randn = [npr.randn(3, 9) for _ in range(3)]
    draws, _, _ = _run(eng, "Matern52", comp, vals, labels, cand, rows, crows, ff, pend, randn)
    ei_o, _ = _oracle("Matern52", comp, vals, labels, cand, rows, crows, ff, pend, randn)
    assert_product_close(draws, ei_o)


def test_ties_pick_the_first(eng):
    comp, vals, labels, cand, rows, crows, ff = _problem(9, 40, 6, 512, 2, 2)
    cand = np.vstack([cand[:256], cand[:256]])            # every value twice: np.argmax takes the first
    draws, _, idx = _run(eng, "Matern52", comp, vals, labels, cand, rows, crows, ff)
    assert idx == int(np.argmax(np.mean(draws, axis=1))) and idx < 256


def _dropin():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "chooser" or k.startswith("chooser.")}
    try:
        return importlib.import_module("chooser.GPConstrainedEIChooser")
    finally:
        # the reference's own `chooser` package is imported by other tests: leave sys.modules as it was
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k in [k for k in sys.modules if k == "chooser" or k.startswith("chooser.")]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize("name", ["nan", "mixed_noiseless", "allvalid"])
def test_next_sequences_match_reference(golden_dir, tmp_path, name):
    g = np.load(os.path.join(golden_dir, "constrained_next_%s.npz" % name))
    m = _dropin()
    c = m.init(str(tmp_path), str(g["args"]))
    st = npr.get_state()
    for k in range(int(g["ncalls"])):
        npr.set_state((st[0], g["before%d_key" % k], int(g["before%d_pos" % k]), int(g["before%d_has_gauss" % k]),
                       float(g["before%d_cached" % k])))
        ret = c.next(g["grid"], g["values"], np.ones(g["grid"].shape[0]), g["candidates%d" % k], g["pending%d" % k],
                     g["complete%d" % k])
        np.testing.assert_allclose(c.last_overall_ei, g["overall_ei%d" % k], rtol=1e-6, atol=1e-12)
        if isinstance(ret, tuple):
            assert ret[0] == int(g["ret_idx%d" % k])
            np.testing.assert_allclose(ret[1], g["ret_pt%d" % k], rtol=1e-6, atol=1e-9)
        else:
            assert "ret_pt%d" % k not in g and ret == int(g["ret_idx%d" % k])
        after = npr.get_state()
        np.testing.assert_array_equal(after[1], g["after%d_key" % k])
        assert after[2] == int(g["after%d_pos" % k])
        st = after


def test_c3_sized_constrained_step(eng):
    """2 048 observations, 1 700 valid, 200 000 candidates, 20 draws: P on 20 000 candidates against the oracle and the
    winner consistent with the draws."""
    from spearmint_amd.engine import FLAG_CONSTRAINED, FLAG_KEEP_MOMENTS
    rs = np.random.RandomState(12)
    D, H, N, M = 8, 20, 2048, 200000
    comp = rs.rand(N, D)
    vals = np.sum((comp - 0.5) ** 2, axis=1) + 0.01 * rs.randn(N)
    labels = np.ones(N)
    labels[rs.choice(N, N - 1700, replace=False)] = 0
    good = labels > 0
    cand = rs.rand(M, D)
    rows = np.column_stack((np.full(H, 0.6), np.full(H, 1e-2), rs.uniform(0.5, 1.0, H), rs.uniform(0.8, 1.6, (H, D))))
    crows = np.column_stack((rs.uniform(0.5, 2, H), np.full(H, 1e-3), rs.uniform(0.5, 1.5, H), rs.uniform(0.8, 1.6, (H, D))))
    ff = rs.randn(N)
    eng.set_observations(comp[good], vals[good])
    eng.set_candidates(cand)
    eng.set_hypers(rows)
    eng.set_constraint_model(comp, ff, crows)
    eng.ei_step(FLAG_CONSTRAINED | FLAG_KEEP_MOMENTS)
    idx, _ = eng.best()
    sub = rs.choice(M, 20000, replace=False)
    for h in (0, 7, 19):
        P = eng.get_constraint_prob(h)
        np.testing.assert_allclose(P[sub], co.constraint_prob("Matern52", comp, ff, crows[h], cand[sub], False), rtol=1e-9)
    draws = eng.ei_draws()
    assert idx == int(np.argmax(np.mean(draws, axis=1)))
    # EI x P itself against the oracle: three draws on 2 000 of the subsample, and all 20 draws at the winner and at
    # 200 others -- the oracle's mean over draws is largest at the GPU's winner
    few = sub[:2000]
    for h in (0, 7, 19):
        ref = co.compute_constrained_ei("Matern52", comp, vals, labels, np.zeros((0, D)), cand[few], ff, rows[h], crows[h])
        assert_product_close(draws[few, h], ref)
    pts = np.concatenate(([idx], sub[:200]))
    ref = np.stack([co.compute_constrained_ei("Matern52", comp, vals, labels, np.zeros((0, D)), cand[pts], ff, rows[h],
                                              crows[h]) for h in range(H)], axis=1)
    assert_product_close(draws[pts], ref)
    assert int(np.argmax(np.mean(ref, axis=1))) == 0


def test_argument_errors(eng):
    from spearmint_amd.engine import FLAG_CONSTRAINED, FLAG_PER_SEC, FLAG_KEEP_MOMENTS
    comp, vals, labels, cand, rows, crows, ff = _problem(1, 20, 4, 256, 2, 2)
    eng.set_observations(comp, vals)
    eng.set_candidates(cand)
    eng.set_hypers(rows)
    with pytest.raises(ValueError):
        eng.ei_step(FLAG_CONSTRAINED)                      # no constraint model
    eng.set_time_model(vals, rows)
    eng.set_constraint_model(comp, ff, crows)
    with pytest.raises(ValueError):
        eng.ei_step(FLAG_CONSTRAINED | FLAG_PER_SEC)
    eng.set_time_model(None, None)
    eng.ei_step(0)
    with pytest.raises(ValueError):
        eng.get_constraint_prob(0)                         # the last pass was not constrained
    eng.ei_step(FLAG_CONSTRAINED | FLAG_KEEP_MOMENTS)
    with pytest.raises(ValueError):
        eng.get_constraint_prob(5)
    eng.set_constraint_model(None, None, None)
    with pytest.raises(ValueError):
        eng.ei_step(FLAG_CONSTRAINED)


def test_multi_device_handle_refuses(golden_dir):
    from spearmint_amd.engine import FLAG_CONSTRAINED, MultiEngine
    comp, vals, labels, cand, rows, crows, ff = _problem(2, 20, 4, 256, 2, 2)
    m = MultiEngine([0], None)
    try:
        m.set_observations(comp, vals)
        m.set_candidates(cand)
        m.set_hypers(rows)
        with pytest.raises(ValueError):
            m.set_constraint_model(comp, ff, crows)
        with pytest.raises(ValueError):
            m.ei_step(FLAG_CONSTRAINED)
    finally:
        m.close()


def _np_logprob(comp, row, r, covar="Matern52"):
    n = comp.shape[0]
    K = row[2] * (hostgp.corr(covar, row[3:], comp) + 1e-6 * np.eye(n)) + row[1] * np.eye(n)
    import scipy.linalg as spla
    L = spla.cholesky(K, lower=True)
    return -np.sum(np.log(np.diag(L))) - 0.5 * np.dot(r - row[0], spla.cho_solve((L, True), r - row[0]))


@pytest.mark.parametrize("N,k", [(2, 1), (37, 5), (64, 32), (129, 3), (300, 17), (1000, 8), (2048, 32)])
def test_logprob_rhs_matches_numpy(eng, N, k):
    rs = np.random.RandomState(N + k)
    D = 4
    comp = rs.rand(N, D)
    eng.set_observations(comp, np.zeros(N))
    rows = np.column_stack((np.zeros(k), np.full(k, 1e-3), rs.uniform(0.3, 2.0, k), rs.uniform(0.3, 1.5, (k, D))))
    rhs = rs.randn(k, N) * 1.3
    lp = eng.gp_logprob_rhs(rows, rhs)
    ref = np.array([_np_logprob(comp, rows[j], rhs[j]) for j in range(k)])
    np.testing.assert_allclose(lp, ref, rtol=1e-10, atol=0)


@pytest.mark.parametrize("N", [23, 200])
def test_logprob_rhs_equals_logprob_on_vals_minus_mean(eng, N):
    rs = np.random.RandomState(N)
    D = 3
    comp = rs.rand(N, D)
    vals = rs.randn(N)
    rows = np.column_stack((rs.uniform(-0.5, 0.5, 6), rs.uniform(1e-3, 1e-2, 6), rs.uniform(0.5, 1.5, 6),
                            rs.uniform(0.3, 1.5, (6, D))))
    eng.set_observations(comp, vals)
    eng.set_hypers(rows)
    plain = eng.gp_logprob()
    rows0 = rows.copy()
    rows0[:, 0] = 0.0
    got = eng.gp_logprob_rhs(rows0, vals[None, :] - rows[:, :1])
    np.testing.assert_array_equal(got, plain)
    # the handle's ordinary call afterwards reads the resident values again
    eng.set_hypers(rows)
    np.testing.assert_array_equal(eng.gp_logprob(), plain)


def test_logprob_rhs_argument_errors(eng):
    comp = np.random.RandomState(0).rand(10, 2)
    with pytest.raises(ValueError):
        eng._check(eng._lib.spx_gp_logprob_rhs(eng._h, None, None, 1, None))
    eng.set_observations(comp, np.zeros(10))
    with pytest.raises(ValueError):
        eng.gp_logprob_rhs(np.tile([0, 1e-3, 1, 1, 1], (33, 1)), np.zeros((33, 10)))


def test_covar_change_refactors_the_constraint_model(eng):
    comp, vals, labels, cand, rows, crows, ff = _problem(31, 60, 9, 800, 2, 2)
    _run(eng, "Matern52", comp, vals, labels, cand, rows, crows, ff)
    from spearmint_amd.engine import FLAG_CONSTRAINED, FLAG_KEEP_MOMENTS
    eng.set_covar("ARDSE")        # no new spx_set_constraint_model: the next step must refactor it under ARDSE
    eng.ei_step(FLAG_CONSTRAINED | FLAG_KEEP_MOMENTS)
    P = np.stack([eng.get_constraint_prob(h) for h in range(2)], axis=1)
    _, P_o = _oracle("ARDSE", comp, vals, labels, cand, rows, crows, ff)
    np.testing.assert_allclose(P, P_o, rtol=1e-9, atol=0)


def test_covar_se_raises_like_the_reference(tmp_path):
    """The reference's next() raises AttributeError for covar=SE (gp has no grad_SE); so does the drop-in, in its
    refinement, after the state pickle is written -- as the reference does."""
    m = _dropin()
    c = m.init(str(tmp_path), "covar=SE,mcmc_iters=2,burnin=2,grid_subset=3")
    rs = np.random.RandomState(4)
    grid = rs.rand(40, 2)
    values = np.concatenate((np.sum((grid[:12] - 0.4) ** 2, axis=1), np.zeros(28)))
    values[[2, 7]] = np.nan
    with pytest.raises(AttributeError, match="grad_SE"):
        c.next(grid, values, np.ones(40), np.arange(12, 40), np.array([], dtype=int), np.arange(12))
    assert os.path.exists(c.state_pkl)
