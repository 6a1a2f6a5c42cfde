"""The reference side of tests/test_gpu_o_factor_pivots.py, on the CPU: every problem of its tables stops LAPACK's dpotrf at
the pivot the GPU test expects and keeps the agreed distance from failing earlier; the barely positive definite mirrors
factor; the extended-precision factorisation that the accuracy test measures against agrees with 50 digits; and the host
stand-in engine reports -inf for exactly the failing draws.  No device result is looked at here."""
import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import factor_helpers as fh
from tests.helpers import OracleEngine


@pytest.mark.parametrize("N", fh.FULL_NS)
def test_full_table_fails_lapack_at_the_expected_pivot(N):
    """Matern52, every (partner, pivot) of the full list: info == j + 1, the number in scipy's message is j + 1, the leading
    block's smallest eigenvalue is >= 2e-5 amp2, the other draws factor -- and the mirror (noise = 0) factors."""
    cases = fh.full_cases(N)
    assert {j for _, j in cases} == set(fh.full_pivots(N)) and N - 1 in fh.full_pivots(N)
    for i, j in cases:
        p = fh.case_problem(N, "Matern52", i, j)
        assert p.expected == (1, j) and np.array_equal(p.X[i], p.X[j])
        fh.check_inputs(p)
        assert fh.scipy_minor(fh.oracle_K(p, 1)) == j + 1
        q = fh.case_problem(N, "Matern52", i, j, pd=True)
        assert q.expected == (-1, -1) and np.array_equal(q.X, p.X)
        for h in range(3):
            assert fh.lapack_info(fh.oracle_K(q, h)) == 0
        assert fh.leading_min_eig(fh.oracle_K(q, 1), j) >= fh.MIN_LEADING_EIG * q.rows[1, 2]


@pytest.mark.parametrize("N,covar", fh.REDUCED_TABLE)
def test_reduced_table_fails_lapack_at_the_expected_pivot(N, covar):
    for i, j in fh.reduced_cases(N):
        for H, bad in ((3, (1,)), (40, (7, 33))):
            p = fh.case_problem(N, covar, i, j, H=H, bad_draws=bad)
            fh.check_inputs(p)
            assert p.expected == (bad[0], j)
        assert fh.lapack_info(fh.oracle_K(fh.case_problem(N, covar, i, j, pd=True), 1)) == 0


def test_lowest_pivot_tables():
    for pairs, want in fh.TWO_PAIRS:
        p = fh.dup_problem(fh.TWO_PAIRS_N, 4, 3, "Matern52", pairs, 4000 + want, (1,))
        assert p.expected == (1, want) and want == min(j for _, j in pairs)
        fh.check_inputs(p)
    p = fh.dup_problem(300, 4, 5, "Matern52", fh.THREE_PAIRS, 4050, (1, 2, 4), own_pair=True)
    assert p.pivots == {1: 200, 2: 70, 4: 17} and p.expected == (1, 200)
    fh.check_inputs(p)
    for H in fh.BATCH_HS:
        p = fh.batch_problem(H)
        assert p.bad_draws == tuple(fh.spread_bad_draws(H)) and p.expected == (0, 129)
        assert len(set(p.pivots.values())) == len(p.bad_draws)
        fh.check_inputs(p)


def test_forms_are_the_documented_option_sets():
    assert len(fh.FORMS) == 12 and fh.FORMS["a_one_launch"] == {}
    for name, opts in fh.FORMS.items():
        assert set(opts) <= set(fh.OPTION_DEFAULTS), name
    assert set(fh.IN_LAUNCH_FORMS) | set(fh.PER_LAUNCH_FORMS) == set(fh.FORMS)
    assert not set(fh.IN_LAUNCH_FORMS) & set(fh.PER_LAUNCH_FORMS)


def _mpf(mp, x):
    """A np.longdouble as an mpf, exactly (two float64 pieces)."""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


@pytest.mark.parametrize("covar", orc.COVARS)
def test_chol_longdouble_against_50_digits(covar):
    """One N = 9 problem per covariance function (an ordinary draw): L, gamma, alpha and lp agree with mpmath's at 50 digits
    to 1e-17 relative (by the largest entry for the arrays) -- ~90 units of the 64-bit significand."""
    mp = pytest.importorskip("mpmath")
    p = fh.dup_problem(9, fh.BASE[covar][0], 2, covar, [], 77, ())
    K = fh.oracle_K(p, 0)
    y = p.vals - p.rows[0, 0]
    L, gamma, alpha, lp = fh.chol_longdouble(K, y)
    with mp.workdps(50):
        Km = mp.matrix(K.tolist())
        Lm = mp.cholesky(Km)
        gm = mp.lu_solve(Lm, mp.matrix(y.tolist()))
        am = mp.lu_solve(Lm.T, gm)
        lpm = -sum(mp.log(Lm[i, i]) for i in range(9)) - mp.mpf("0.5") * sum(g * g for g in gm)
        errL = max(abs(_mpf(mp, L[i, j]) - Lm[i, j]) for i in range(9) for j in range(9)) / max(abs(Lm[i, j]) for i in range(9) for j in range(9))
        errg = max(abs(_mpf(mp, gamma[i]) - gm[i]) for i in range(9)) / max(abs(g) for g in gm)
        erra = max(abs(_mpf(mp, alpha[i]) - am[i]) for i in range(9)) / max(abs(a) for a in am)
        errlp = abs(_mpf(mp, lp) - lpm) / abs(lpm)
        print("chol_longdouble vs 50 digits (%s): L %.2e gamma %.2e alpha %.2e lp %.2e"
              % (covar, float(errL), float(errg), float(erra), float(errlp)))
        assert max(errL, errg, erra, errlp) <= mp.mpf("1e-17")
    # and float64 LAPACK is where it should be against it
    assert np.allclose(np.asarray(L, dtype=np.float64), np.linalg.cholesky(K), rtol=1e-13, atol=1e-15)


def test_chol_longdouble_refuses_a_failing_matrix():
    p = fh.case_problem(17, "Matern52", 0, 15)
    with pytest.raises(AssertionError, match="pivot 15"):
        fh.chol_longdouble(fh.oracle_K(p, 1))


@pytest.mark.parametrize("covar", orc.COVARS)
def test_oracle_engine_logprob_is_minus_inf_for_exactly_the_bad_draws(covar):
    for H, bad in ((3, (1,)), (12, (0, 6, 11)), (5, ())):
        p = fh.case_problem(130, covar, 63, 64, H=H, bad_draws=bad)
        e = OracleEngine(covar)
        e.set_observations(p.X, p.vals)
        e.set_hypers(p.rows)
        lp = e.gp_logprob()
        assert np.array_equal(np.isneginf(lp), np.isin(np.arange(H), bad))
        ok = ~np.isneginf(lp)
        assert np.isfinite(lp[ok]).all()
        for h in np.nonzero(ok)[0][:2]:       # the stand-in's finite values are the long-double ones
            want = fh.chol_longdouble(fh.oracle_K(p, h), p.vals - p.rows[h, 0])[3]
            assert abs(lp[h] - float(want)) <= 1e-9 * abs(float(want)) + 1e-9 * 130
        e.set_hypers(fh.good_rows(p))
        assert np.isfinite(e.gp_logprob()).all()
