"""The blocked Cholesky's failure report (csrc/chol_kernels.hip: factor16_mfma / diag_block and its five callers) held to
LAPACK's in every form of the factorisation: the pivot that fails is the one dpotrf stops at -- both parities of a pivot
pair, every 16-row sub-block and 64-row block-column base, the last live row next to the padding --, the lowest pivot and
the lowest draw win, a failure is not a hand-off time-out and leaves nothing behind, and the barely positive definite mirror
of every problem factors as accurately as LAPACK does.  The problems are tests/factor_helpers.py's; tests/test_factor_reference.py
holds each of them to the reference on the CPU.  A non-positive pivot is an ordinary status code of an ordinary call."""
import contextlib

import numpy as np
import pytest
from numpy.linalg import LinAlgError
from scipy.linalg import lapack

from oracle import gp_ei_oracle as orc
from tests import factor_helpers as fh
from tests.factor_helpers import options

pytestmark = pytest.mark.gpu
FLOOR = 16 * np.finfo(float).eps      # 3.6e-15: a case where LAPACK happens to be exact is not an impossible bar


@pytest.fixture()
def eng():
    from spearmint_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def fresh(fn, *a, **kw):
    from spearmint_amd.engine import Engine
    e = Engine(0)
    try:
        return fn(e, *a, **kw)
    finally:
        e.close()


def cands(p, M=16):
    return np.random.RandomState(5).rand(M, p.X.shape[1]) * fh.BASE[p.covar][2]


def load(e, p, rows=None):
    e.set_covar(p.covar)
    e.set_observations(p.X, p.vals)
    e.set_hypers(p.rows if rows is None else rows)


def logprob(e, p, rows=None):
    load(e, p, rows)
    lp = e.gp_logprob()
    return lp, e.not_pd_info()


def minor_raised(fn, *a, **kw):
    """The number in the LinAlgError's "%d-th leading minor ..." (and the exception)."""
    with pytest.raises(LinAlgError) as info:
        fn(*a, **kw)
    return fh.minor_in(info.value), info.value


def bad_mask(p):
    return np.isin(np.arange(p.rows.shape[0]), p.bad_draws)


def check_logprob(e, p, what=""):
    """One failing batch through spx_gp_logprob under the engine's current options: the report is (expected draw, pivot),
    -inf at exactly the failing rows, and the finite rows are, bit for bit, those of the same batch with good rows in the
    failing rows' places.  Returns the values."""
    lp, info = logprob(e, p)
    assert info == p.expected, (what, p.pairs, info, p.expected)
    bad = bad_mask(p)
    assert np.array_equal(np.isneginf(lp), bad), (what, p.pairs, lp)
    assert np.isfinite(lp[~bad]).all(), (what, p.pairs)
    lp_good, info_good = logprob(e, p, fh.good_rows(p))
    assert info_good[0] < 0 and np.isfinite(lp_good).all(), (what, p.pairs)
    assert np.array_equal(lp[~bad], lp_good[~bad]), (what, p.pairs)
    return lp


def check_raise(e, p, j):
    load(e, p)
    n, _ = minor_raised(e.gp_logprob, raise_not_pd=True)
    assert n == j + 1, (p.pairs, n)


# ---- 1. the pivot, everywhere ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", fh.FULL_NS)
def test_pivot_default_loglikelihood_and_factor(eng, N):
    """The one-launch log-likelihood and spx_factor through k_lean_flow (the defaults), every pivot of the full list with
    every partner: spx_not_pd_info() == (1, j); gp_logprob(raise_not_pd=True), factor() and ei_grid() raise LinAlgError
    with the number scipy.linalg.cholesky gives for the oracle's K: j + 1."""
    for i, j in fh.full_cases(N):
        p = fh.case_problem(N, "Matern52", i, j)
        K = fh.oracle_K(p, 1)
        assert fh.lapack_info(K) == j + 1                      # (the reference, before any device result)
        minor = fh.scipy_minor(K)
        assert minor == j + 1
        check_logprob(eng, p, "default")
        check_raise(eng, p, j)
        eng.set_candidates(cands(p))
        n, _ = minor_raised(eng.factor)
        assert n == minor and eng.not_pd_info() == (1, j), (i, j, n, eng.not_pd_info())
        n, _ = minor_raised(eng.ei_grid, p.X, p.vals, cands(p), p.rows)
        assert n == minor and eng.not_pd_info() == (1, j), (i, j, n, eng.not_pd_info())


@pytest.mark.parametrize("N,covar", fh.REDUCED_TABLE)
@pytest.mark.parametrize("form", fh.OTHER_FORMS)
def test_pivot_every_other_loglikelihood_form(eng, form, N, covar):
    """The reduced list through every other form of spx_gp_logprob (at most 32 rows): the same report, and the finite rows
    are the default form's bit for bit (which thereby runs for the other three covariance functions too; their spx_factor
    is the factor_flow1 entry of test_pivot_other_entry_points)."""
    for i, j in fh.reduced_cases(N):
        p = fh.case_problem(N, covar, i, j)
        assert fh.lapack_info(fh.oracle_K(p, 1)) == j + 1
        base = check_logprob(eng, p, "default")
        with options(eng, **fh.FORMS[form]):
            lp = check_logprob(eng, p, form)
            check_raise(eng, p, j)
        assert np.array_equal(lp, base), (form, i, j)


def _entry_rows(eng, p, j, H, bad):
    """More than 32 rows: the row-major k_chol_diag / k_chol_panel, padded to 128."""
    q = fh.case_problem(p.X.shape[0], p.covar, p.pairs[0][0], j, H=H, bad_draws=bad)
    assert fh.lapack_info(fh.oracle_K(q, bad[0])) == j + 1
    check_logprob(eng, q, "rows%d" % H)
    check_raise(eng, q, j)


def _entry_rhs(eng, p, j):
    load(eng, p)
    rhs = np.random.RandomState(j).randn(p.rows.shape[0], p.X.shape[0])
    lp = eng.gp_logprob_rhs(p.rows, rhs)
    assert eng.not_pd_info() == (1, j)
    assert np.array_equal(np.isneginf(lp), bad_mask(p)) and np.isfinite(lp[~bad_mask(p)]).all()
    good = eng.gp_logprob_rhs(fh.good_rows(p), rhs)
    assert eng.not_pd_info()[0] < 0 and np.array_equal(lp[~bad_mask(p)], good[~bad_mask(p)])


def _entry_factor(eng, p, j, **opts):
    with options(eng, **opts):
        load(eng, p)
        eng.set_candidates(cands(p))
        n, _ = minor_raised(eng.factor)
    assert n == j + 1 and eng.not_pd_info() == (1, j), (opts, n, eng.not_pd_info())


def _entry_step(eng, p, j, **opts):
    """spx_ei_step: the error is reported after the single synchronisation."""
    with options(eng, **opts):
        load(eng, p)
        eng.set_candidates(cands(p, 300))
        n, _ = minor_raised(eng.ei_step, 0)
    assert n == j + 1 and eng.not_pd_info() == (1, j), (opts, n, eng.not_pd_info())
    with pytest.raises(ValueError):
        eng.ei_draws()


def _entry_time(eng, p, j):
    """The objective's draws are fine and time-model draw 1 fails: draw H + 1."""
    H = p.rows.shape[0]
    log_durs = 0.3 * np.random.RandomState(3).randn(p.X.shape[0])
    n, ex = minor_raised(eng.ei_per_sec_grid, p.X, p.vals, log_durs, cands(p), fh.good_rows(p), p.rows)
    assert n == j + 1 and eng.not_pd_info() == (H + 1, j), (n, eng.not_pd_info())
    assert str(ex).rstrip(")").endswith(", time model"), str(ex)


def _entry_constraint(eng, p, j):
    """Duplicated comp_c rows and noise_c = -1.5e-6 amp2_c in draw 1 of the constraint model: draw 2H + 1."""
    H = p.rows.shape[0]
    load(eng, p, fh.good_rows(p))
    eng.set_candidates(cands(p))
    eng.set_constraint_model(p.X, np.random.RandomState(9).randn(p.X.shape[0]), p.rows)
    n, ex = minor_raised(eng.factor)
    assert n == j + 1 and eng.not_pd_info() == (2 * H + 1, j), (n, eng.not_pd_info())
    assert "constraint" in str(ex)
    eng.set_constraint_model(None, None, None)


ENTRIES = {
    "rows33": lambda e, p, j: _entry_rows(e, p, j, 33, (7, 32)),
    "rows40": lambda e, p, j: _entry_rows(e, p, j, 40, (7, 33)),
    "logprob_rhs": _entry_rhs,
    "factor_flow0": lambda e, p, j: _entry_factor(e, p, j, ei_flow=0),
    "factor_flow1": lambda e, p, j: _entry_factor(e, p, j, ei_flow=1),
    "step_streams1_overlap0": lambda e, p, j: _entry_step(e, p, j, streams=1, step_overlap=0),
    "step_streams1_overlap1": lambda e, p, j: _entry_step(e, p, j, streams=1, step_overlap=1),
    "step_streams2_overlap0": lambda e, p, j: _entry_step(e, p, j, streams=2, step_overlap=0),
    "step_streams2_overlap1": lambda e, p, j: _entry_step(e, p, j, streams=2, step_overlap=1),
    "per_sec_time_model": _entry_time,
    "constraint_model": _entry_constraint,
}


@pytest.mark.parametrize("N,covar", fh.REDUCED_TABLE)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_pivot_other_entry_points(eng, entry, N, covar):
    """The reduced list through every other call that factors: more than 32 log-likelihood rows, spx_gp_logprob_rhs,
    spx_factor both ways, spx_ei_step, a failing time-model draw (H + d) and a failing constraint model (2H + d)."""
    for i, j in fh.reduced_cases(N):
        p = fh.case_problem(N, covar, i, j)
        assert fh.lapack_info(fh.oracle_K(p, 1)) == j + 1
        ENTRIES[entry](eng, p, j)


@pytest.mark.parametrize("N", fh.REDUCED_NS)
def test_pivot_three_engines(N):
    """MultiEngine([0, 0, 0]), 7 draws as 3 + 2 + 2 with the failing draw 4 on the second engine's shard: gp_logprob and
    factor (draws partitioned) report the GLOBAL draw and the pivot."""
    from spearmint_amd.engine import MultiEngine
    me = MultiEngine([0, 0, 0])
    try:
        for i, j in fh.reduced_cases(N):
            p = fh.case_problem(N, "Matern52", i, j, H=7, bad_draws=(4,))
            assert fh.lapack_info(fh.oracle_K(p, 4)) == j + 1
            me.set_partition(1)
            load(me, p)
            lp = me.gp_logprob()
            assert me.not_pd_info() == (4, j), (i, j, me.not_pd_info())
            assert np.array_equal(np.isneginf(lp), bad_mask(p))
            n, _ = minor_raised(me.gp_logprob, raise_not_pd=True)
            assert n == j + 1
            me.set_partition(3)
            load(me, p)
            me.set_candidates(cands(p, 64))
            n, _ = minor_raised(me.factor)
            assert n == j + 1 and me.not_pd_info() == (4, j), (i, j, n, me.not_pd_info())
    finally:
        me.close()


# ---- 2. the lowest pivot wins ---------------------------------------------------------------------------------------------
LOWEST_FORMS = list(fh.FORMS) + ["rows40", "factor_flow1", "factor_flow0"]


@contextlib.contextmanager
def _form(eng, name):
    with options(eng, **fh.FORMS.get(name, {"ei_flow": 0} if name == "factor_flow0" else {})):
        yield


def _report(eng, name, p):
    """(values or None, spx_not_pd_info()) of one failing batch through the named form."""
    with _form(eng, name):
        if name.startswith("factor"):
            load(eng, p)
            eng.set_candidates(cands(p))
            minor_raised(eng.factor)
            return None, eng.not_pd_info()
        return logprob(eng, p)


@pytest.mark.parametrize("form", LOWEST_FORMS)
def test_two_failing_pairs_in_one_draw_report_the_lower(eng, form):
    """Two duplicate pairs in one draw, j1 < j2 in the same 16-row sub-block, in different sub-blocks of one 64-block, and in
    different block columns ((70, 200) and (10, 257) at N = 300): j1, in the in-launch forms (atomicCAS / atomicMin at device
    scope) and in the per-launch forms (the first writer)."""
    H, bad = (40, (33,)) if form == "rows40" else (3, (1,))
    for pairs, want in fh.TWO_PAIRS:
        p = fh.dup_problem(fh.TWO_PAIRS_N, 4, H, "Matern52", pairs, 4000 + want, bad)
        assert fh.lapack_info(fh.oracle_K(p, bad[0])) == want + 1
        lp, info = _report(eng, form, p)
        assert info == (bad[0], want), (form, pairs, info)
        if lp is not None:
            assert np.array_equal(np.isneginf(lp), bad_mask(p))


@pytest.mark.parametrize("form", LOWEST_FORMS)
def test_three_draws_fail_at_different_pivots(eng, form):
    """Draws 1, 2 and 4 of 5 (rows40: of 40) fail at pivots 200, 70 and 17: the report is the lowest DRAW with that draw's own
    pivot, not the lowest pivot of the batch; each failing draw alone in front reports its own."""
    H = 40 if form == "rows40" else 5
    p = fh.dup_problem(300, 4, H, "Matern52", fh.THREE_PAIRS, 4050, (1, 2, 4), own_pair=True)
    for b, j in p.pivots.items():
        assert fh.lapack_info(fh.oracle_K(p, b)) == j + 1
    lp, info = _report(eng, form, p)
    assert info == (1, 200), (form, info)
    if lp is not None:
        assert np.array_equal(np.isneginf(lp), bad_mask(p))
    for b, j in p.pivots.items():
        sub = p._replace(rows=p.rows[b:] if H == 5 else np.roll(p.rows, -b, axis=0))
        _, info = _report(eng, form, sub)
        assert info == (0, j), (form, b, info)


@pytest.mark.parametrize("H", fh.BATCH_HS)
def test_failing_draws_first_middle_and_last(eng, H):
    """Failing draws at row 0, in the middle and at the last row of 1, 3, 12, 32 and 33 rows, each at its own pivot (129, 70,
    17 at N = 130), through every log-likelihood form: (0, 129), -inf at exactly those rows, the other rows untouched."""
    p = fh.batch_problem(H)
    for b, j in p.pivots.items():
        assert fh.lapack_info(fh.oracle_K(p, b)) == j + 1
    base = check_logprob(eng, p, "default")
    for form in fh.OTHER_FORMS:
        with options(eng, **fh.FORMS[form]):
            lp = check_logprob(eng, p, form)
        assert np.array_equal(lp, base), form
    for b, j in p.pivots.items():                        # the last failing draw alone: its own pivot at the last row
        rows = fh.good_rows(p)
        rows[b] = p.rows[b]
        _, info = logprob(eng, p, rows)
        assert info == (b, j), (H, b, info)


# ---- 3. a failure is not a time-out, and leaves nothing behind -------------------------------------------------------------
def _plain(e, p, rows=None):
    return logprob(e, p, rows)[0]


@pytest.mark.parametrize("form", list(fh.FORMS))
def test_a_failure_is_not_a_timeout_and_leaves_nothing_behind(eng, form):
    """After a not-PD call (a late block column: pivot 129 of 300, so the draw's remaining hand-offs run on the substituted
    pivots): no fallback, no warning, the data-flow launch still enabled; the next calls on the handle -- good rows of the
    same sizes, four times, then other sizes -- are a fresh engine's bit for bit, and report no draw."""
    p = fh.case_problem(300, "Matern52", 63, 129, H=5, bad_draws=(0, 3))
    other = fh.case_problem(130, "Matern52", 0, 1, H=7, bad_draws=())
    want = fresh(_plain, p, fh.good_rows(p))
    want_other = fresh(_plain, other)
    with options(eng, **fh.FORMS[form]):
        for _ in range(2):
            lp, info = logprob(eng, p)
            assert info == (0, 129) and np.array_equal(np.isneginf(lp), bad_mask(p))
            assert eng.stat("flow_fallbacks") == 0 and eng.last_warning() is None
            if form in fh.FLOW_FORMS:
                assert eng.stat("flow_enabled") == 1
            for _ in range(4):
                got, info = logprob(eng, p, fh.good_rows(p))
                assert np.array_equal(got, want) and info[0] < 0, (form, info)
            got, info = logprob(eng, other)
            assert np.array_equal(got, want_other) and info[0] < 0, (form, info)
        assert eng.stat("flow_fallbacks") == 0 and eng.last_warning() is None


@pytest.mark.parametrize("ei_flow", [1, 0])
def test_after_a_failed_factor_nothing_runs_until_a_good_one(eng, ei_flow):
    """spx_factor fails at pivot 129: ei_run, set_fantasies and ei_grad_batch are refused (no results of an earlier
    factorisation), no fallback is counted -- and a following good ei_step matches the oracle."""
    from tests.test_gpu_a_parity import assert_ei_close
    p = fh.case_problem(300, "Matern52", 63, 129, H=3)
    cand = cands(p, 500)
    good = fh.good_rows(p)
    with options(eng, ei_flow=ei_flow):
        load(eng, p, good)
        eng.set_candidates(cand)
        eng.ei_step(0)                                   # an earlier, good factorisation with results
        eng.set_hypers(p.rows)
        n, _ = minor_raised(eng.factor)
        assert n == 130 and eng.not_pd_info() == (1, 129)
        assert eng.stat("flow_fallbacks") == 0 and eng.last_warning() is None and eng.stat("flow_enabled") == 1
        for fn, a in ((eng.ei_run, (0,)), (eng.set_fantasies, (np.zeros((3, 300, 2)), np.zeros((3, 2)))),
                      (eng.ei_grad_batch, (cand[:3],)), (eng.ei_draws, ())):
            with pytest.raises(ValueError):
                fn(*a)
        eng.set_hypers(good)
        eng.ei_step(0)
        assert eng.not_pd_info()[0] < 0
        draws = eng.ei_draws()
    with orc.covar(p.covar):
        assert_ei_close(draws, orc.ei_over_hypers(p.X, cand, p.vals, good))
    assert np.array_equal(draws, fresh(lambda e: e.ei_grid(p.X, p.vals, cand, good, want_draws=True)[3]))


# ---- 4. just positive definite: the device succeeds and is as accurate as LAPACK -------------------------------------------
def _lapack_solves(K, y):
    L, info = lapack.dpotrf(K, lower=1, clean=1)
    assert info == 0
    gamma, info = lapack.dtrtrs(L, y, lower=1)
    assert info == 0
    alpha, info = lapack.dtrtrs(L, gamma, lower=1, trans=1)
    assert info == 0
    return L, gamma, alpha


def _errors(L, gamma, alpha, ref, j):
    """Relative errors against the long-double factorisation: L[j, j], row j of L, gamma, alpha (the last three by norm)."""
    Lr, gr, ar, _ = ref
    nrm = lambda a: float(np.sqrt(np.sum(np.square(a))))     # noqa: E731  (long double throughout)
    return (float(abs(L[j, j] - Lr[j, j]) / Lr[j, j]), nrm(L[j] - Lr[j]) / nrm(Lr[j]), nrm(gamma - gr) / nrm(gr),
            nrm(alpha - ar) / nrm(ar))


def _accuracy_cases(N):
    return sorted(set(fh.reduced_cases(N)) | (set(fh.full_cases(N)) if N == 300 else set()))


@pytest.mark.parametrize("N,covar", fh.REDUCED_TABLE)
def test_barely_positive_definite_factor_is_as_accurate_as_lapack(eng, N, covar):
    """The mirror (noise = 0: pivot j is about +2e-6 amp2) through spx_factor, as objective draw 1 and as time-model draw 0:
    it factors; K, L, alpha and gamma are the same bits with ei_flow 1 and 0; the device's K is the oracle's to 1e-13; and
    against the long-double factorisation of the DEVICE's K, the largest relative error over the N's cases of L[j, j], of
    row j of L, of gamma and of alpha is at most 4 x the same maximum of dpotrf / dtrtrs in float64 (floor 16 ulp).

    Measured on an MI355X, device maximum / LAPACK maximum (bar: 4) for L[j, j], row j of L, gamma, alpha:
        N = 130 Matern52  0.36, 0.36, 0.36, 0.36        N = 300 Matern52  0.55, 0.55, 0.60, 0.55
        N = 130 Matern32  0.67, 0.67, 0.67, 0.67        N = 130 ARDSE     0.16, 0.16, 0.16, 0.16
        N = 130 SE        0.16, 0.16, 0.16, 0.16   (X scaled by 4: ARDSE's problem at length scale 0.25)
    LAPACK's own maxima: 1.0e-10 ... 3.6e-10 for L[j, j] and gamma, 2.0e-10 ... 7.3e-10 for alpha, 1.4e-13 ... 5.1e-13
    for row j -- the barely positive pivot loses six digits in either arithmetic, and its error is what all four see."""
    H = 2
    log_durs = 0.3 * np.random.RandomState(3).randn(N)
    dev_max, lap_max = np.zeros(4), np.zeros(4)
    for i, j in _accuracy_cases(N):
        p = fh.case_problem(N, covar, i, j, H=H, pd=True)
        trows = p.rows[::-1].copy()                          # time-model draw 0 is the barely positive definite one
        got = []
        for ei_flow in (1, 0):
            with options(eng, ei_flow=ei_flow):
                load(eng, p)
                eng.set_candidates(cands(p))
                eng.set_time_model(log_durs, trows)
                eng.factor()
                assert eng.not_pd_info()[0] < 0
                got.append([eng.get_factor(d) + (eng.get_factor_rows(d, j, 1)[1],) for d in (1, H + 0)])
        for a, b in zip(got[0], got[1]):
            for x, y in zip(a, b):
                assert np.array_equal(x, y), ("ei_flow 1 / 0", i, j)
        for (K, L, alpha, gamma), rows, y in ((got[0][0], p.rows[1], p.vals - p.rows[1, 0]),
                                              (got[0][1], trows[0], log_durs - trows[0, 0])):
            q = p._replace(rows=rows[None, :])
            np.testing.assert_allclose(K, fh.oracle_K(q, 0), rtol=1e-13, atol=0)
            ref = fh.chol_longdouble(K, y)
            dev_max = np.maximum(dev_max, _errors(L, gamma, alpha, ref, j))
            lap_max = np.maximum(lap_max, _errors(*_lapack_solves(K, y), ref=ref, j=j))
    print("N=%d %s device max %s LAPACK max %s ratio %s" % (N, covar, dev_max, lap_max, dev_max / lap_max))
    for name, d, o in zip(("L[j,j]", "row j of L", "gamma", "alpha"), dev_max, lap_max):
        assert d <= max(4 * o, FLOOR), (name, d, o)


@pytest.mark.parametrize("N,covar", fh.REDUCED_TABLE)
def test_barely_positive_definite_loglikelihood_every_form(eng, N, covar):
    """The mirror through every log-likelihood form: every value finite, all forms the same bits, and within the suite's
    rtol = 1e-9, atol = 1e-9 N of the long-double value for the oracle's K; more than 32 rows (row-major) within the same."""
    for i, j in fh.reduced_cases(N):
        p = fh.case_problem(N, covar, i, j, pd=True)
        want =np.array([float(fh.chol_longdouble(fh.oracle_K(p, h), p.vals - p.rows[h, 0])[3]) for h in range(3)])
        base, info = logprob(eng, p)
        assert info[0] < 0 and np.isfinite(base).all(), (i, j, info)
        np.testing.assert_allclose(base, want, rtol=1e-9, atol=1e-9 * N)
        for form in fh.OTHER_FORMS:
            with options(eng, **fh.FORMS[form]):
                lp, info = logprob(eng, p)
            assert info[0] < 0 and np.array_equal(lp, base), (form, i, j, info)
        rows = np.tile(p.rows, (12, 1))                      # 36 rows: k_chol_diag / k_chol_panel
        lp, info = logprob(eng, p, rows)
        assert info[0] < 0 and np.isfinite(lp).all()
        np.testing.assert_allclose(lp, np.tile(want, 12), rtol=1e-9, atol=1e-9 * N)
