"""Every form of the covariance epilogue (csrc/cov_device.h: sqrt_pos, exp_neg, the three *_corr_t with their clamps and the
closing fma that restores NaN) against the 50-digit yardstick of tests/cov_mp.py, element by element, on inputs whose r^2 is
exact in float64 -- so the reference of every element is known whatever the contraction order of the form that produced it:
K* (k_cov MODE 0, k_cov_flat), K (MODE 1), the K the factorisation really consumed (k_lean_flow's own tiles, MODE 3's
tile-major store, the row-major path) through the factor's first column, the fused small-N kernel and the GEMM path through
the predictive mean, the log-likelihood path's K through a closed form, and the forms against each other bit for bit.

The ceilings are derived, not measured (u = (1 + s) 2^-52 k + poly 2^-1074, tests/cov_mp.py):
  Matern kinds  sqrt <= 1 ulp, its product with sqrt5 / sqrt3 <= 1/2 ulp, exp <= 1 ulp (the header's claims), the polynomial's
                <= 3 roundings and the final product: (3 + 1.5 s) 2^-52 relative, <= 3 u.
  ARDSE / SE    exp <= 1 ulp, 0.5 r^2 exact: <= 2 u.
Where amp2 is not a power of two the product amp2 k adds half an ulp of the result.

Measured on an MI355X, worst |got - ref| / u with no slack taken off, ref the yardstick rounded to float64 (Matern52 /
Matern32 / ARDSE; first with amp2 = 1 and 4, then with amp2 = 0.7, whose product adds its half ulp):
  K*       (a)  1.00 / 0.99 / 0.97   and  1.36 / 1.34 / 1.22     (the flat form, amp2 = 0.7: 0.62 / 0.71 / 1.18)
  K        (c)  0.64 / 0.73 / 0.86   and  0.64 / 0.73 / 0.97
  L[:, 0]  (d)  0.62 / 0.72 / 1.19   and  0.66 / 0.79 / 0.96     (before the 4 x 2^-52 of the column's own roundings)
  func_m   (e)  0.64 / 0.86 / 1.34   and  0.66 / 0.72 / 1.86     (before its 6 x 2^-52)
and spx_gp_logprob against the closed form, worst relative error: 4.5e-14 / 2.1e-14 / 1.4e-14 (the oracle's: 4.9e-14 /
2.1e-14 / 1.5e-14).  The float64 oracle's own K* on the same data: 1.03 / 0.92 / 0.52 u.
With exp_neg's ln2_lo step taken out (a scratch build, not committed) test (a) fails in 37 of its 48 cases, at up to
1.2e6 u (Matern kinds) and 8.7e8 u (ARDSE)."""
import os

import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import cov_mp as cv
from tests import pending_helpers as ph
from tests.test_gpu_a_parity import assert_ei_close

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = LD(2.0) ** -52
DEN = LD(2.0) ** -1074
AMP2S = (1.0, 4.0, 0.7)
NOISE = 0.01
FAMILIES = cv.lattice_problems()
WINDOWS = [f for f in FAMILIES if f[0].startswith("window")]
MEASURED = []                                                    # every worst_in_u call's max |got - ref| / u, slack not taken off


@pytest.fixture(scope="module")
def eng():
    from spearmint_amd.engine import Engine
    assert np.finfo(LD).nmant >= 63, "the comparisons below are made in 80-bit extended precision"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "cov_lattice_mp.npz")))


@pytest.fixture(scope="module")
def exact():
    """r^2 of every family, computed once."""
    return {name: cv.exact_r2(X, C, ls) for name, X, C, ls in FAMILIES}


def hyper_rows(ls, amp2s=AMP2S, mean=0.0, noise=NOISE):
    return np.array([np.concatenate(([mean, noise, a], ls)) for a in amp2s])


def load(eng, kind, X, C, ls, vals=None, **kw):
    eng.set_covar(kind)
    eng.set_observations(X, np.zeros(X.shape[0]) if vals is None else vals)
    if C is not None:
        eng.set_candidates(C)
    eng.set_hypers(hyper_rows(ls, **kw))


def worst_in_u(got, k_ref, u, amp2, scale=LD(1), rel_slack=0.0, abs_slack=LD(0)):
    """max of (|got - scale amp2 k_ref| - slack) / (scale amp2 u) in extended precision (so that denormal results and their
    tolerances are compared without rounding either).  slack: half an ulp of the product amp2 k where amp2 is not a power of
    two, plus what the caller's later roundings are allowed (rel_slack in units of 2^-52 of the reference, abs_slack)."""
    ref = LD(amp2) * k_ref.astype(LD) * scale
    slack = rel_slack * EPS * ref + abs_slack
    if np.frexp(amp2)[0] != 0.5:
        slack = slack + LD(0.5) * np.spacing(np.abs((ref / scale).astype(np.float64))).astype(LD) * scale
    err, unit = np.abs(got.astype(LD) - ref), LD(amp2) * u.astype(LD) * scale
    MEASURED.append(float(np.max(err / unit)))                   # (before the slack: what the docstring above reports)
    return float(np.max((err - slack) / unit))


def assert_exact_entries(got, r2, kind, amp2):
    assert np.array_equal(got[r2 == 0.0], np.full(int(np.sum(r2 == 0.0)), amp2))        # a coincident pair: exactly amp2
    past = r2 > cv.CLAMP[kind]
    assert np.array_equal(got[past], np.zeros(int(np.sum(past)))) and not np.any(np.signbit(got[past]))   # +0.0


# ---- a. K* element by element -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cv.KINDS)
@pytest.mark.parametrize("fam", range(len(FAMILIES)), ids=[f[0].replace(" ", "_") for f in FAMILIES])
def test_kstar_is_within_its_ceiling_of_the_yardstick(eng, fixture, exact, kind, fam):
    name, X, C, ls = FAMILIES[fam]
    r2 = exact[name]
    k_ref, u = cv.lookup(fixture, kind, r2)
    load(eng, kind, X, C, ls)
    eng.factor()
    for h, amp2 in enumerate(AMP2S):
        got = eng.get_cross_cov(h)
        w = worst_in_u(got, k_ref, u, amp2)
        print("K* %-9s %-16s amp2 %.1f: worst err / u = %.3f (%.3f)" % (kind, name, amp2, w, MEASURED[-1]))
        assert w <= cv.CEILING[kind]
        assert_exact_entries(got, r2, kind, amp2)


@pytest.mark.parametrize("name", ["line e=0", "window ARDSE"])
def test_se_is_ardse_with_unit_length_scales(eng, name):
    _, X, C, ls = FAMILIES[[f[0] for f in FAMILIES].index(name)]
    assert np.all(ls == 1.0)
    load(eng, "ARDSE", X, C, ls)
    eng.factor()
    ref = [eng.get_cross_cov(h) for h in range(3)]
    load(eng, "SE", X, C, np.array([0.37]))
    eng.factor()
    for h in range(3):
        assert np.array_equal(eng.get_cross_cov(h), ref[h])


# ---- b. the flat form ---------------------------------------------------------------------------------------------------------
def test_flat_form_is_held_and_equals_the_grid_form(eng, fixture):
    n_cu = eng.stat("n_cu")
    X = WINDOWS[0][1]
    base = np.concatenate([C for _, _, C, _ in WINDOWS])
    M = 8 * n_cu * 64 + 64                                     # just over 131 072 rows on 256 compute units
    C = np.resize(base.ravel(), M)[:, None]
    # launch_cov_kind (csrc/cov_kernels.hip) takes the flat form when wgs > 2 n_cu and units >= 8 n_cu.  spx_get_cross_cov
    # launches M rounded up to SPX_BN = 128 columns in 64-column blocks; N <= 128 is Np = 128: rows_per_wg = 128, so one
    # workgroup and one 128-row unit per column block, and wgs = units = column blocks.
    Np, SPX_BN = (X.shape[0] + 127) // 128 * 128, 128
    mc = (M + SPX_BN - 1) // SPX_BN * SPX_BN
    wgs = (mc // 64) * ((Np + 127) // 128) * 1                   # grid.x * grid.y * draws
    units = 1 * (mc // 64) * ((Np + 127) // 128)                 # draws * column blocks * 128-row chunks
    assert Np == 128 and wgs > 2 * n_cu and units >= 8 * n_cu
    r2 = np.tile(cv.exact_r2(X, base, np.ones(1)), (1, M // base.shape[0] + 1))[:, :M]
    for kind in cv.KINDS:
        k_ref, u = cv.lookup(fixture, kind, r2)
        load(eng, kind, X, C, np.ones(1), amp2s=(0.7,))
        eng.factor()
        flat = eng.get_cross_cov(0)
        with ph.options(eng, cov_flat=0):
            grid = eng.get_cross_cov(0)
        w = worst_in_u(flat, k_ref, u, 0.7)
        print("K* flat %-9s: worst err / u = %.3f (%.3f)" % (kind, w, MEASURED[-1]))
        assert w <= cv.CEILING[kind]
        assert_exact_entries(flat, r2, kind, 0.7)
        assert np.array_equal(flat, grid)


# ---- c. K element by element --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cv.KINDS)
@pytest.mark.parametrize("N", [2, 63, 64, 65, 129])
def test_k_is_within_its_ceiling_of_the_yardstick(eng, fixture, kind, N):
    X, ls = cv.factor_problem(N)
    r2 = cv.exact_r2(X, X, ls)
    k_ref, u = cv.lookup(fixture, kind, r2)
    load(eng, kind, X, None, ls)
    eng.factor()
    off = r2 > 0.0
    for h, amp2 in enumerate(AMP2S):
        K = eng.get_factor(h, want_L=False, want_alpha=False)[0]
        w = worst_in_u(K[off], k_ref[off], u[off], amp2)
        print("K  %-9s N %3d amp2 %.1f: worst err / u = %.3f (%.3f)" % (kind, N, amp2, w, MEASURED[-1]))
        assert w <= cv.CEILING[kind]
        assert np.array_equal(K, K.T)             # r^2 is exact, so the two operand orders give the same bits
        eye = np.eye(N)
        same = amp2 * (1.0 + 1e-6 * eye) + NOISE * eye
        assert np.array_equal(K[~off], same[~off])
        past = r2 > cv.CLAMP[kind]
        assert np.array_equal(K[past], np.zeros(int(np.sum(past)))) and not np.any(np.signbit(K[past]))


# ---- d. the K the factorisation really used -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cv.KINDS)
@pytest.mark.parametrize("N", [2, 40, 64, 65, 129, 200])
def test_first_column_of_the_factor_is_the_yardsticks(eng, fixture, kind, N):
    """The first column of a Cholesky factor is K[:, 0] / sqrt(K00) whatever the rest of the matrix is, and for rows in later
    64-blocks L21 = K21 L11^-T has a first column that touches only 1 / L00.  Roundings besides the correlation's own, counted
    in csrc/chol_kernels.hip (factor16_mfma): a = amp2 (1 + 1e-6) + noise is three roundings, halved by the square root (0.75
    ulp); rinv0 = a^-1/2 is v_rsq_f64 + one third-order step (~1 ulp); l = K[i][0] rinv0 is one product (0.5 ulp) -- the same
    rinv0 is entry (0, 0) of the inverse of every enclosing block, and the MFMAs that form the panels add exact zeros to that
    one product.  2.25 ulp, inside the 4 x 2^-52 the first column is allowed; amp2 k is the half ulp worst_in_u adds itself.
    Where the results are denormal the two products (amp2 k, K rinv0) round absolutely, half of 2^-1074 each."""
    X, ls = cv.factor_problem(N)
    r2 = cv.exact_r2(X[1:], X[:1], ls).ravel()
    assert N == 2 or (r2.min() < 1e-3 and r2.max() > 2.1e5)
    k_ref, u = cv.lookup(fixture, kind, r2)
    load(eng, kind, X, None, ls)
    Ls = {}
    for flow in (1, 0):
        for flow_cov in (1, 0):
            with ph.options(eng, ei_flow=flow, lean_flow_cov=flow_cov):
                eng.factor()
                # the path really taken: k_lean_flow with its own tiles / on k_cov's tile-major store / the row-major launches
                assert (eng.stat("last_factor_flow"), eng.stat("last_factor_cov_in_flow")) == (flow, flow and flow_cov)
                Ls[flow, flow_cov] = [eng.get_factor(h, want_K=False, want_alpha=False)[1] for h in range(len(AMP2S))]
    for h, amp2 in enumerate(AMP2S):
        L = Ls[1, 1][h]
        a = LD(amp2) * (LD(1) + LD(1e-6)) + LD(NOISE)
        w = worst_in_u(L[1:, 0], k_ref, u, amp2, scale=1 / np.sqrt(a), rel_slack=4.0, abs_slack=DEN)
        print("L0 %-9s N %3d amp2 %.1f: worst err / u = %.3f (%.3f)" % (kind, N, amp2, w, MEASURED[-1]))
        assert w <= cv.CEILING[kind]
        assert abs(LD(L[0, 0]) - np.sqrt(a)) <= 4 * EPS * np.sqrt(a)
        for key in Ls:
            assert np.array_equal(Ls[key][h], L), key


# ---- e. the fused kernel and the GEMM path, directly --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cv.KINDS)
def test_predictive_mean_of_a_diagonal_k_is_the_yardsticks(eng, fixture, kind):
    """X = {0, 4096}: K is exactly diagonal, so with mean 0 func_m[c] = amp2 k(c) v0 / K00 -- K* as k_ei_fused128's fused_pass
    and as the three-stage path (k_cov + predict GEMM) computed it.  6 x 2^-52 for K00, its factor, the two solves and the dot."""
    X = WINDOWS[0][1][:2]
    C = np.concatenate([C for _, _, C, _ in WINDOWS])
    vals = np.array([1.0, 0.5])
    r2 = cv.exact_r2(X[:1], C, np.ones(1)).ravel()
    k_ref, u = cv.lookup(fixture, kind, r2)
    big = k_ref >= 1e-290
    assert np.sum(big) >= 60 and np.all(cv.exact_r2(X[1:], C, np.ones(1)) > cv.CLAMP[kind])
    load(eng, kind, X, C, np.ones(1), vals=vals)
    runs = {}

    def run(label, **opts):
        with ph.options(eng, **opts):
            eng.factor()
            eng.ei_run(ph.FLAG_KEEP_MOMENTS)
            runs[label] = ([eng.get_moments(h) for h in range(len(AMP2S))], eng.ei_draws(), eng.stat("last_step_fused"))

    run("fused")
    for ns in (1, 2, 3):
        run("gemm%d" % ns, ei_fused=0, streams=ns)
    assert runs["fused"][2] == 1 and all(runs["gemm%d" % ns][2] == 0 for ns in (1, 2, 3))
    for h, amp2 in enumerate(AMP2S):
        a = LD(amp2) * (LD(1) + LD(1e-6)) + LD(NOISE)
        m = runs["fused"][0][h][0]
        w = worst_in_u(m[big], k_ref[big], u[big], amp2, scale=LD(vals[0]) / a, rel_slack=6.0)
        print("func_m %-9s amp2 %.1f: worst err / u = %.3f (%.3f)" % (kind, amp2, w, MEASURED[-1]))
        assert w <= cv.CEILING[kind]
    for label in runs:
        assert np.array_equal(runs[label][1], runs["fused"][1]), label
        for h in range(len(AMP2S)):
            assert np.array_equal(runs[label][0][h][0], runs["fused"][0][h][0]), label
            assert np.array_equal(runs[label][0][h][1], runs["fused"][0][h][1]), label


# ---- f. every form on the lattice data ----------------------------------------------------------------------------------------
def lattice_ei_problem(N, M=700, D=3, seed=29):
    rs = np.random.RandomState(seed + N)
    X = rs.randint(0, 8, (N, D)).astype(np.float64) / 4.0
    C = rs.randint(0, 8, (M, D)).astype(np.float64) / 4.0
    C[::50] = X[rs.randint(0, N, len(C[::50]))]                  # coincident candidates
    C[7::90, 1] += 4096.0                                        # rows past every clamp
    vals = np.sum((X - 0.8) ** 2, axis=1) + 0.05 * rs.randn(N)
    hypers = np.array([[0.3, 0.01, 1.0, 1.0, 2.0, 0.5], [0.1, 0.02, 4.0, 0.5, 0.5, 1.0], [0.5, 0.01, 0.7, 2.0, 1.0, 2.0]])
    return X, C, vals, hypers


@pytest.mark.parametrize("kind", cv.KINDS)
@pytest.mark.parametrize("N", [40, 150])
def test_every_form_gives_the_same_ei_on_lattice_data(eng, kind, N):
    X, C, vals, hypers = lattice_ei_problem(N)
    Np = (N + 127) // 128 * 128
    small = 8 * Np * 256                                         # K* staging for 256 candidates of one draw: three chunks
    eng.set_covar(kind)

    def run(step=False, **opts):
        with ph.options(eng, **opts):
            eng.set_observations(X, vals)
            eng.set_candidates(C)
            eng.set_hypers(hypers)
            if step:
                eng.ei_step(0)
            else:
                eng.factor()
                eng.ei_run(0)
            return eng.ei_draws(), eng.best()

    base, best = run()
    with orc.covar(kind), np.errstate(all="ignore"):
        ref = orc.ei_over_hypers(X, C, vals, hypers)
    assert_ei_close(base, ref)
    assert best[0] == orc.choose(ref)
    variants = [dict(cov_flat=0), dict(cov_flat=1), dict(streams=2), dict(streams=3), dict(streams=3, kstar_corun=0),
                dict(gemm_partial=0), dict(gemm_partial=1), dict(ei_fused=0), dict(ei_fused=1), dict(ei_fused=0, streams=2),
                dict(ei_fused=0, streams=3), dict(kstar_budget_bytes=small), dict(ei_fused=0, kstar_budget_bytes=small),
                dict(ei_fused=0, streams=3, kstar_budget_bytes=small),
                dict(ei_fused=0, streams=3, kstar_corun=0, kstar_budget_bytes=small), dict(step=True),
                dict(step=True, ei_fused=0, streams=3, kstar_budget_bytes=small)]
    for v in variants:
        got, b = run(**v)
        assert np.array_equal(got, base), v
        assert b == best, v


# ---- g. the log-likelihood path's own K ---------------------------------------------------------------------------------------
def path_taken(eng):
    """(one launch, k_lean_flow, K(X,X) built inside it) of the last factorisation."""
    return eng.stat("last_logprob_one_launch"), eng.stat("last_factor_flow"), eng.stat("last_factor_cov_in_flow")


@pytest.mark.parametrize("kind", cv.KINDS)
def test_logprob_of_two_observations_is_the_closed_forms(eng, fixture, kind):
    """Tolerance: twice the pinned error of the float64 oracle against the same closed form (cov_mp.LOGPROB_CEILING, held by tests/test_cov_mp.py) -- the
    device takes the same few operations in another order."""
    mean, noise, amp2 = cv.LP_HYPER
    eng.set_covar(kind)
    worst = 0.0
    for (pair, ls, _), ref in zip(cv.logprob_cases(), fixture["lp_" + kind]):
        row = np.concatenate(([mean, noise, amp2], ls))[None, :]
        eng.set_observations(pair, np.array(cv.LP_VALS))
        eng.set_hypers(row)
        got = eng.gp_logprob()
        assert path_taken(eng) == (1, 1, 1)                      # one launch, k_lean_flow's own tiles
        worst = max(worst, abs(got[0] - ref) / abs(ref))
        for opts, path in ((dict(lean_flow_cov=0), (0, 1, 0)), (dict(lean_one=0), (0, 1, 1)),
                           (dict(lean_flow_cov=0, lean_one=0), (0, 1, 0))):
            with ph.options(eng, **opts):
                assert np.array_equal(eng.gp_logprob(), got), opts
                assert path_taken(eng) == path, opts
        eng.set_hypers(np.repeat(row, 33, axis=0))               # > 32 rows: the row-major factorisation
        assert np.array_equal(eng.gp_logprob(), np.repeat(got, 33))
        assert path_taken(eng) == (0, 0, 0)
    print("logprob %-9s: worst relative error %.3e" % (kind, worst))
    assert worst <= 2 * cv.LOGPROB_CEILING[kind]


# ---- h. non-finite inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cv.KINDS + ("SE",))
def test_non_finite_candidates_give_nan_columns_and_leave_the_others(eng, kind):
    name, X, C, ls = FAMILIES[len(cv.LINE_EXPS)]                 # lattice D = 3: non-negative observations
    assert np.all(X >= 0.0)
    load(eng, kind, X, C, ls)
    eng.factor()
    clean = [eng.get_cross_cov(h) for h in range(len(AMP2S))]
    bad = C.copy()
    bad[11, 1] = np.nan
    bad[70 % len(C), 2] = np.inf
    cols = np.array([11, 70 % len(C)])
    with orc.covar(kind), np.errstate(all="ignore"):
        ref = orc.corr(ls, X, bad)
    assert np.all(np.isnan(ref[:, cols])) and np.sum(np.isnan(ref)) == ref.shape[0] * 2
    eng.set_candidates(bad)
    ok = np.ones(len(C), dtype=bool)
    ok[cols] = False
    for h in range(len(AMP2S)):
        got = eng.get_cross_cov(h)
        assert np.all(np.isnan(got[:, cols]))
        assert np.array_equal(got[:, ok], clean[h][:, ok])
