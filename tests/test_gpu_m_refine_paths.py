"""spx_ei_grad_batch, the objective of the local refinement of GPEIOptChooser / GPEIperSecChooser (and of
GPConstrainedEIChooser while no violation has been seen), in its three arithmetic branches -- plain EI, EI per second, EI
averaged over pending fantasies -- at the shapes where its four kernels (k_point_cov, k_trimv_multi, k_trimvT_multi,
k_point_finish) can go wrong, its invariants bit for bit, central differences, the handle's state machine, the
multi-device handle, and its tails against a 50-digit reference.  The oracle is tests/refine_helpers.oracle, held to
oracle/gp_ei_oracle.py by tests/test_refine_mp.py.  Sorted after test_gpu_l_constrained_refine.py; the older tests of this
call (test_gpu_d_multi.py, test_gpu_y_covar.py) should be read first when both fail."""
import os

import numpy as np
import pytest

from tests import constrained_refine_helpers as hp
from tests import refine_helpers as rh
from tests import refine_mp as rm
from tests.constrained_refine_helpers import assert_close, central_differences
from tests.test_gpu_k_constrained_paths import options

pytestmark = pytest.mark.gpu
BRANCHES = list(rh.BRANCHES)
COVARS = list(rh.COVARS)
FLAG_PER_SEC = 1


@pytest.fixture()
def eng():
    from spearmint_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def fresh(p, pts):
    """What a new engine taken straight to the state of p gives."""
    from spearmint_amd.engine import Engine
    e = Engine(0)
    try:
        rh.setup(e, p)
        return e.ei_grad_batch(pts)
    finally:
        e.close()


def check(eng, p, pts, counts=None):
    """The call at pts[:P] for every P of counts against the batched oracle at the tolerances of this call (value rtol
    1e-7; gradient rtol 1e-6, atol 1e-9 max |g_ref|: tests/constrained_refine_helpers.assert_close)."""
    f_ref, g_ref = rh.oracle(p, pts)
    assert np.all(np.isfinite(f_ref)) and np.all(np.isfinite(g_ref))
    for P in counts or (pts.shape[0],):
        f, g = eng.ei_grad_batch(pts[:P])
        assert_close(f, g, f_ref[:P], g_ref[:P])
    return f, g


# ---- 1. oracle parity, one factor at a time from the base case (N 150, D 4, H 3, 21 points, Matern52, S 5) ----------------
N_SWEEP = [2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 2047, 2048, 2049, 4100]


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("N", N_SWEEP)
def test_observation_counts(eng, N, branch):
    """The wave-strided tails of k_trimv_multi (t + 28 < jn, jb steps of 256) and k_trimvT_multi (i + 192 < Np) below, on
    and above 64, 128, 256 and 2048 resident rows (with fantasies: observations + pending points), and one case above 4096.
    From 2047 on: one draw and 9 points (the oracle's factorisation is what costs); at 4100, 3 points."""
    big = N >= 2047
    p = rh.make_problem(1000 + N, "Matern52", branch, N=N, D=4, H=1 if big else 3)
    rh.setup(eng, p)
    check(eng, p, rh.points(p, N + 1, 3 if N > 4096 else 9 if big else 21))


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("D", [1, 7, 8, 9, 16, 17, 33])
def test_dimensions(eng, D, branch):
    """The boundaries of the gradient's passes of GD = 8 dimensions; with a time model the third accumulator and the xct /
    ilt operands of a second and a fifth pass; the quotient rule at D = 1."""
    p = rh.make_problem(2000 + D, "Matern52", branch, N=150, D=D, H=3)
    rh.setup(eng, p)
    check(eng, p, rh.points(p, D + 1, 21))


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("H", [1, 3, 12])
def test_draws(eng, H, branch):
    p = rh.make_problem(3000 + H, "Matern52", branch, N=150, D=4, H=H)
    rh.setup(eng, p)
    check(eng, p, rh.points(p, H + 1, 21))


@pytest.mark.parametrize("branch", BRANCHES)
def test_points_per_call(eng, branch):
    """SPX_REFINE_PB = 8 points share a pass over W: the last partial group at 9 and at 203 = 25 x 8 + 3."""
    p = rh.make_problem(4000, "Matern52", branch, N=150, D=4, H=3)
    rh.setup(eng, p)
    check(eng, p, rh.points(p, 5, 203), counts=(1, 7, 8, 9, 64, 203))


@pytest.mark.parametrize("S", [1, 5, 128, 129, 2048, 2049, 4096])
def test_fantasy_counts(eng, S):
    """k_point_finish keeps 3 S doubles in LDS: above 48 KB from S = 2049, where launch_point_finish has to opt in, and
    96 KB at S = 4096, the documented maximum.  A device that refuses the LDS must make the call fail with SPX_ERR_HIP and
    the kernel's name (include/spx.h); anything else that goes wrong there is a finding, not a skip."""
    from spearmint_amd.engine import SpxError
    big = S >= 2048
    p = rh.make_problem(5000 + S, "Matern52", "fant", N=40 if big else 150, D=4, H=2 if big else 3, S=S)
    rh.setup(eng, p)
    pts = rh.points(p, S + 1, 9)
    try:
        eng.ei_grad_batch(pts)
    except SpxError as ex:
        assert "k_point_finish" in str(ex), "refused without the kernel's name: %s" % ex
        raise
    check(eng, p, pts)


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("covar", COVARS)
def test_covariances(eng, covar, branch):
    p = rh.make_problem(6000 + len(covar), covar, branch, N=150, D=4, H=3)
    rh.setup(eng, p)
    check(eng, p, rh.points(p, 7, 21))


@pytest.mark.parametrize("branch", BRANCHES)
def test_se_is_ardse_with_unit_length_scales(eng, branch):
    """Beyond the reference: gp.py has no grad_SE, so its refinement raises with covar=SE (and so does the oracle,
    tests/test_refine_mp.py).  The library maps SE onto ARDSE with the length scales replaced by ones, as gp.SE itself
    does for the covariance; that relation is asserted exactly: bit for bit."""
    p = rh.make_problem(6100, "SE", branch, N=150, D=4, H=3)
    pts = rh.points(p, 7, 21)
    rh.setup(eng, p)
    got = eng.ei_grad_batch(pts)
    q = hp.Problem()
    q.__dict__.update(p.__dict__)
    q.covar = "ARDSE"
    q.rows, q.trows = p.rows.copy(), p.trows.copy()
    q.rows[:, 3:] = 1.0
    q.trows[:, 3:] = 1.0
    want = fresh(q, pts)
    assert same(got, want)
    if branch != "fant":           # (p.fant was drawn for covar=SE with p's length scales: not q's fantasies)
        assert_close(got[0], got[1], *rh.oracle(q, pts))


@pytest.mark.parametrize("branch", ["plain", "persec"])
def test_near_duplicate_observations(eng, branch):
    """comp[60:] = comp[:60] + 1e-9 (tests/test_gpu_a_parity.py::test_near_duplicate_observations), one point ON a
    duplicated location.  The float64 oracle against the 50-digit reference on this case (both on the CPU, 11 points,
    value / gradient): plain 6.8e-13 / 5.7e-13, per second 6.8e-13 / 5.7e-13 -- the oracle is five decades inside 1e-7
    here (the jitter and the noise keep the duplicated rows apart), so it stays the reference and the call's own tolerances
    apply."""
    p = near_duplicate_problem(branch)
    rh.setup(eng, p)
    check(eng, p, near_duplicate_points(p))


def near_duplicate_problem(branch):
    p = rh.make_problem(25, "Matern52", branch, N=120, D=4, H=3)
    p.comp[60:] = p.comp[:60] + 1e-9
    p.vals[60:] = p.vals[:60]
    p.log_durs[60:] = p.log_durs[:60]
    p.best = np.min(p.vals)
    return rh.finish(p)


def near_duplicate_points(p):
    pts = rh.points(p, 26, 11)
    pts[4] = p.comp[int(np.argmin(p.vals)) % 60]
    pts[7] = p.comp[3]
    return pts


# ---- 2. invariants, bit for bit ----------------------------------------------------------------------------------------------
def base(branch, **kw):
    args = dict(N=150, D=6, H=4)
    args.update(kw)
    return rh.make_problem(7000, "Matern52", branch, **args)


@pytest.mark.parametrize("branch", BRANCHES)
def test_a_point_does_not_see_its_batch(eng, branch):
    p = base(branch)
    rh.setup(eng, p)
    pts = rh.points(p, 9, 203)
    f, g = eng.ei_grad_batch(pts)
    assert same(eng.ei_grad_batch(pts), (f, g))                      # a call repeated
    for i in (0, 100, 200, 202):                                     # (200 .. 202: the last partial group)
        assert same(eng.ei_grad_batch(pts[i:i + 1]), (f[i:i + 1], g[i:i + 1]))
        f1, g1 = eng.ei_grad(pts[i])                                 # spx_ei_grad is the batch of one
        assert f1 == f[i] and np.array_equal(g1, g[i])
    for pos in range(9):                                             # every position of a group of 8, and the ninth
        batch = pts[20:29].copy()
        batch[pos] = pts[201]
        fb, gb = eng.ei_grad_batch(batch)
        assert fb[pos] == f[201] and np.array_equal(gb[pos], g[201]), pos
    perm = np.random.RandomState(3).permutation(203)
    fp, gp = eng.ei_grad_batch(pts[perm])
    assert np.array_equal(fp, f[perm]) and np.array_equal(gp, g[perm])


@pytest.mark.parametrize("branch", BRANCHES)
def test_a_grid_pass_between_two_calls_changes_nothing(eng, branch):
    """spx_ei_run in between (default, a small staging budget, two streams): another user of the handle's buffers."""
    p = base(branch)
    rh.setup(eng, p, cand=np.random.RandomState(2).rand(3000, p.D))
    pts = rh.points(p, 9, 21)
    first = eng.ei_grad_batch(pts)
    flags = FLAG_PER_SEC if branch == "persec" else 0
    for kw in ({}, dict(kstar_budget_bytes=256 * 128 * 8), dict(streams=2), dict(streams=2, kstar_budget_bytes=256 * 128 * 8)):
        with options(eng, **kw):
            eng.ei_run(flags)
            assert eng.best()[0] >= 0
            assert same(eng.ei_grad_batch(pts), first), sorted(kw)
    if branch == "persec":
        eng.ei_run(0)                                                # (the plain grid pass on a handle with a time model)
        assert same(eng.ei_grad_batch(pts), first)
    assert_close(first[0], first[1], *rh.oracle(p, pts))


@pytest.mark.parametrize("branch", BRANCHES)
def test_a_step_between_two_calls(eng, branch):
    """spx_ei_step factors again.  Plain and per second: the same state, the same bits.  With fantasies set it drops them
    (include/spx.h), and the next call is a fresh engine's on the same observations without fantasies."""
    p = base(branch)
    rh.setup(eng, p)
    pts = rh.points(p, 9, 21)
    first = eng.ei_grad_batch(pts)
    eng.ei_step(FLAG_PER_SEC if branch == "persec" else 0)
    after = eng.ei_grad_batch(pts)
    if branch != "fant":
        assert same(after, first)
        return
    q = rh.make_problem(7000, "Matern52", "plain", N=150, D=6, H=4)
    q.comp = q.compv = p.X
    q.vals = q.valsv = np.concatenate((p.vals, np.zeros(p.pend.shape[0])))
    q.rows = p.rows
    rh.finish(q)
    assert same(after, fresh(q, pts)) and not np.array_equal(after[0], first[0])
    assert_close(after[0], after[1], *rh.oracle(q, pts))


@pytest.mark.parametrize("branch", BRANCHES)
def test_options_that_must_not_change_bits(eng, branch):
    p = base(branch, N=200)                  # (200: three 16-row steps of padding inside Np = 256 for gemm_partial)
    pts = rh.points(p, 9, 21)
    rh.setup(eng, p)
    first = eng.ei_grad_batch(pts)
    for name, values, default in (("gemm_partial", (0, 1), -1), ("stage_copies", (0, 1), -1)):
        for v in values:
            try:
                eng.set_option(name, v)
                rh.setup(eng, p)
                assert same(eng.ei_grad_batch(pts), first), (name, v)
            finally:
                eng.set_option(name, default)


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("covar", ["Matern52", "ARDSE"])
def test_draw_additivity(eng, covar, branch):
    """With H draws resident, neg_ei and grad are the host sum, in draw order from 0.0, of H one-draw calls: each draw's
    workgroups read only that draw's tables.  Measured on an MI355X: bit for bit in every branch."""
    p = rh.make_problem(7100, covar, branch, N=150, D=9, H=5)
    pts = rh.points(p, 9, 21)
    rh.setup(eng, p)
    f, g = eng.ei_grad_batch(pts)
    fs, gs = np.zeros(21), np.zeros((21, p.D))
    for d in range(p.H):
        rh.setup(eng, rh.one_draw(p, d))
        fd, gd = eng.ei_grad_batch(pts)
        fs += fd
        gs = gs + gd
    print(covar, branch, "draw additivity: max |f - sum| %.3g, max |g - sum| %.3g" % (np.max(np.abs(f - fs)), np.max(np.abs(g - gs))))
    assert np.array_equal(f, fs) and np.array_equal(g, gs)


def test_constrained_sum_over_fantasies_is_s_times_the_plain_mean(eng):
    """The two objectives share one fantasy block: with every bests[h][s] equal to one value b and no violation seen, the
    constrained entry (EI against b, SUMMED over the S = 4 fantasies, P = 1) returns exactly 4 times what the plain entry
    (EI against bests[h][s], AVERAGED) returns -- dividing by 4 and by 1 are both exact.  The gradients are not compared:
    their last combines round differently by design (refine_kernels.hip: combine_plain / combine_con)."""
    p = rh.make_problem(7200, "Matern52", "fant", N=70, D=3, H=2, S=4)
    b = float(np.min(p.vals))
    p.bests = np.full((p.H, p.S), b)
    pts = rh.points(p, 9, 9)
    rh.setup(eng, p)
    f_plain, _ = eng.ei_grad_batch(pts)
    crows = np.column_stack((np.full(p.H, 1.5), np.full(p.H, 1e-3), np.ones(p.H), np.ones((p.H, p.D))))
    eng.set_constraint_model(np.zeros((0, p.D)), np.zeros(0), crows)      # no violation seen
    eng.factor()
    eng.set_fantasies(p.fant, p.bests)
    f_con, _ = eng.constrained_ei_grad_batch(pts, b)
    assert np.array_equal(f_con, 4.0 * f_plain)


# ---- 3. it is a gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("covar", COVARS)
def test_central_differences(eng, covar, branch, D):
    """The bar of tests/test_gpu_d_multi.py::test_ei_grad_batch_matches_oracle (rtol 2e-3, atol 1e-9); the oracle's own
    gradient agrees with its own central differences to 1.5e-7 of max |g|, so the bar has four decades of room."""
    p = rh.make_problem(11, covar, branch, N=40, D=D, H=2)
    rh.setup(eng, p)
    dims = range(min(D, 3))
    for x in rh.points(p, 5, 2):                         # one uniform, one near the best observation
        x = np.clip(x, 1e-3, 1 - 1e-3)
        _, g = eng.ei_grad_batch(x[None])
        fd = central_differences(lambda y: eng.ei_grad_batch(y[None])[0][0], x, dims)
        assert np.allclose(fd, g[0][:len(dims)], rtol=2e-3, atol=1e-9), (covar, branch, fd, g[0])


# ---- 4. the handle's state machine -------------------------------------------------------------------------------------------
def final_state(eng, p, pts, oracle=True):
    """The handle's result for the state p against a fresh engine's, bit for bit, and against the oracle."""
    got = eng.ei_grad_batch(pts)
    assert same(got, fresh(p, pts))
    if oracle:
        assert_close(got[0], got[1], *rh.oracle(p, pts))
    return got


def refused(eng, pts):
    with pytest.raises(ValueError):
        eng.ei_grad_batch(pts)


def test_fantasies_replaced_with_the_same_count_then_another_then_cleared(eng):
    """alphaS = K^-1 (fant - mean) is cached across calls (alphaS_valid): a second spx_set_fantasies with the same S must
    not leave the first set's behind."""
    p = rh.make_problem(8000, "Matern52", "fant", N=150, D=4, H=3, S=5)
    pts = rh.points(p, 1, 12)
    rh.setup(eng, p)
    first = final_state(eng, p, pts)
    assert same(eng.ei_grad_batch(pts), first)               # (the cached alphaS is the one just computed)
    q = rh.make_problem(8000, "Matern52", "fant", N=150, D=4, H=3, S=5)
    q.randn = 1.5 * p.randn[:, ::-1] + 0.3
    rh.finish(q)
    eng.set_fantasies(q.fant, q.bests)                       # the same S, other values
    second = final_state(eng, q, pts)
    assert not np.array_equal(second[0], first[0])
    r = rh.make_problem(8001, "Matern52", "fant", N=150, D=4, H=3, S=7)
    r.comp, r.vals, r.pend, r.rows = p.comp, p.vals, p.pend, p.rows
    r.compv, r.valsv, r.best = p.comp, p.vals, p.best
    rh.finish(r)
    eng.set_fantasies(r.fant, r.bests)                       # another S
    final_state(eng, r, pts)
    eng.set_fantasies(p.fant, p.bests)                       # and back
    assert same(eng.ei_grad_batch(pts), first)
    eng.set_fantasies(None, None)                            # cleared: the plain branch over [comp; pend]
    s = rh.make_problem(8000, "Matern52", "plain", N=150, D=4, H=3)
    s.comp = s.compv = p.X
    s.vals = s.valsv = np.concatenate((p.vals, np.zeros(p.pend.shape[0])))
    s.rows = p.rows
    rh.finish(s)
    final_state(eng, s, pts)


def test_time_model_set_then_cleared(eng):
    """nmodels == 2 or pt_kt must not survive a cleared time model: the plain branch's bits."""
    p = rh.make_problem(8100, "Matern52", "persec", N=150, D=4, H=3)
    pts = rh.points(p, 1, 12)
    rh.setup(eng, p)
    per_sec = final_state(eng, p, pts)
    eng.set_time_model(None, None)
    refused(eng, pts)                                        # an invalidating setter: SPX_ERR_ARG until spx_factor
    eng.factor()
    q = rh.make_problem(8100, "Matern52", "plain", N=150, D=4, H=3)
    plain = final_state(eng, q, pts)
    assert not np.array_equal(plain[0], per_sec[0])
    eng.set_time_model(p.log_durs, p.trows)
    refused(eng, pts)
    eng.factor()
    assert same(eng.ei_grad_batch(pts), per_sec)


@pytest.mark.parametrize("branch", BRANCHES)
def test_observations_shrink_and_grow_and_draws_change(eng, branch):
    """300 -> 120 -> 300 rows across the pad boundaries (stale rows of every per-point buffer past the new Np), then
    another number of draws, then another covariance: every state is a fresh engine's."""
    pts = None
    for i, (N, H, covar) in enumerate([(300, 3, "Matern52"), (120, 3, "Matern52"), (300, 3, "Matern52"), (300, 5, "Matern52"),
                                       (300, 2, "Matern52"), (300, 2, "Matern32"), (300, 2, "ARDSE"), (129, 4, "ARDSE")]):
        p = rh.make_problem(8200 + i, covar, branch, N=N, D=4, H=H)
        pts = rh.points(p, 1, 12) if pts is None else pts
        rh.setup(eng, p)
        final_state(eng, p, pts, oracle=(i in (1, 3, 5, 7)))


@pytest.mark.parametrize("branch", BRANCHES)
def test_refused_between_an_invalidating_setter_and_the_factorisation(eng, branch):
    p = base(branch)
    pts = rh.points(p, 1, 12)
    rh.setup(eng, p)
    first = eng.ei_grad_batch(pts)
    for name in ("set_observations", "set_hypers", "set_covar", "gp_logprob"):
        if name == "set_observations":
            eng.set_observations(p.X, np.concatenate((p.vals, np.zeros(p.pend.shape[0]))))
            eng.set_hypers(p.rows)
        elif name == "set_hypers":
            eng.set_hypers(p.rows)
        elif name == "set_covar":
            eng.set_covar("Matern32")
            eng.set_covar("Matern52")
        else:
            # spx_gp_logprob factors the objective GP alone, without W = L^-1 (do_factor(lean): factored = false, the
            # fantasies dropped): it invalidates, so the call is refused -- never other numbers
            assert np.all(np.isfinite(eng.gp_logprob()))
        refused(eng, pts)
        rh.setup(eng, p)
        assert same(eng.ei_grad_batch(pts), first), name


def test_argument_errors(eng):
    from spearmint_amd.engine import SPX_ERR_ARG, MultiEngine, _dp
    p = rh.make_problem(8300, "Matern52", "persec", N=60, D=3, H=2)
    pts = rh.points(p, 1, 4)
    rh.setup(eng, p)
    first = eng.ei_grad_batch(pts)

    def rc(points, P, f=True, g=True):
        fo, go = np.empty(4), np.empty((4, 3))
        r = eng._lib.spx_ei_grad_batch(eng._h, _dp(points), P, _dp(fo) if f else None, _dp(go) if g else None)
        return r, eng._lib.spx_last_error()

    for bad in (rc(pts, 0), rc(pts, -3), rc(None, 4), rc(pts, 4, f=False), rc(pts, 4, g=False)):
        assert bad[0] == SPX_ERR_ARG and bad[1]
        assert same(eng.ei_grad_batch(pts), first)
    # fantasies with a time model: not defined (the reference's per-second refinement ignores pending jobs)
    fant = np.tile(p.vals[None, :, None], (2, 1, 3))
    eng.set_fantasies(fant, np.min(fant, axis=1))
    r, msg = rc(pts, 4)
    assert r == SPX_ERR_ARG and b"time model" in msg
    eng.set_fantasies(None, None)
    assert same(eng.ei_grad_batch(pts), first)
    # the 2-D partition
    m = MultiEngine([0, 0])
    try:
        m.set_partition(2)
        m.set_observations(p.comp, p.vals)
        m.set_hypers(p.rows)
        m.set_candidates(pts)
        m.factor()
        with pytest.raises(ValueError):
            m.ei_grad_batch(pts)
        m.set_partition(1)
        rh.setup(m, p)
        assert same(m.ei_grad_batch(pts), first)
    finally:
        m.close()


# ---- 5. the multi-device handle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", BRANCHES)
def test_three_engines_shard_the_points(eng, branch):
    """Fewer points than devices, as many, one more, and the partial groups of every shard."""
    from spearmint_amd.engine import MultiEngine
    p = base(branch)
    pts = rh.points(p, 9, 203)
    rh.setup(eng, p)
    m = MultiEngine([0, 0, 0])
    try:
        rh.setup(m, p)
        for P in (1, 2, 3, 4, 11, 203):
            assert same(m.ei_grad_batch(pts[:P]), eng.ei_grad_batch(pts[:P])), P
    finally:
        m.close()


# ---- 6. the tails against the 50-digit reference ---------------------------------------------------------------------------
FLOOR = 16 * np.finfo(float).eps      # 3.6e-15: a band where the oracle happens to be exact is not an impossible bar


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("covar", COVARS)
def test_tails_against_50_digits(eng, golden_dir, covar, branch):
    """-EI from 10 down past 1e-300 (tests/golden/refine_tail_mp.npz; mpmath is not needed here): the tail problem of
    tests/refine_mp.py with its values as they are and with one observation lowered.  Per band of log10 |f_ref| --
    [-3, 1], [-20, -3), [-100, -20), [-300, -100) -- the device's max error against the 50-digit reference is at most 4 x
    the float64 oracle's own on the same inputs (computed here), floor 16 ulp; value: relative; gradient: per point
    max_d |g_d - ref_d| / max_d |ref_d|.  Below 1e-300: 0 <= -f <= 1e-290 and a finite gradient.

    Measured on an MI355X, device error / oracle error, value / gradient, per band (bar: 4), the larger of the two value
    sets:
        Matern52 plain  1.03 / 0.52, 1.27 / 1.23, 1.22 / 1.46, 0.88 / 0.92
        Matern52 persec 1.94 / 0.56, 1.28 / 1.22, 1.22 / 1.46, 0.88 / 0.92
        Matern52 fant   1.26 / 0.91, 1.27 / 1.34, 1.79 / 1.89, 0.83 / 0.95
        Matern32 plain  0.68 / 0.67, 1.57 / 2.00, 0.85 / 1.02, 1.01 / 0.91
        Matern32 persec 2.08 / 0.99, 1.55 / 1.98, 0.85 / 1.02, 1.01 / 0.91
        Matern32 fant   0.72 / 2.01, 1.52 / 1.93, 1.21 / 1.02, 0.87 / 0.87
        ARDSE    plain  1.12 / 1.25, 1.36 / 1.33, 1.23 / 1.32, 1.77 / 1.55
        ARDSE    persec 1.26 / 1.55, 1.36 / 1.33, 1.23 / 1.32, 1.77 / 1.55
        ARDSE    fant   1.58 / 2.51, 1.63 / 1.48, 2.02 / 1.40, 1.24 / 1.34
    The device's largest errors over the nine cases: 1.2e-12 / 1.8e-12, 3.5e-11 / 3.1e-11, 1.1e-10 / 1.2e-10,
    1.0e-9 / 1.1e-9 -- the error of func_m amplified by about u^2 / 2, on either side; ndtr_r adds nothing that shows."""
    g = np.load(os.path.join(golden_dir, "refine_tail_mp.npz"))
    p, pts, sets = rm.tail_problem(covar, branch)
    report, failures = [], []
    for which, vs in zip(rm.SETS, sets):
        q = rm.with_values(p, vs)
        f_ref, g_ref, lf = (g[rm.key(covar, branch, which, k)] for k in ("f", "g", "log10f"))
        rh.setup(eng, q)
        f, gr = eng.ei_grad_batch(pts)
        with np.errstate(all="ignore"):
            f_o, g_o = rh.oracle(q, pts)
        e_o, e_d = rm.band_errors(f_o, g_o, f_ref, g_ref, lf), rm.band_errors(f, gr, f_ref, g_ref, lf)
        for band, o, d in zip(rm.TAIL_BANDS, e_o, e_d):
            if o is None:
                continue
            for what, ov, dv in (("value", o[0], d[0]), ("gradient", o[1], d[1])):
                report.append("%s %s %s band %s %s: device %.3g oracle %.3g ratio %.3g" %
                              (covar, branch, which, band, what, dv, ov, dv / ov if ov else np.inf))
                if not dv <= max(4 * ov, FLOOR):
                    failures.append(report[-1])
        deep = lf < -300
        assert np.mean(deep) <= 0.15
        assert np.all((-f[deep] >= 0) & (-f[deep] <= 1e-290)) and np.all(np.isfinite(gr))
        assert np.all(f <= 0)
        # the same points one call each: the same bits as the call of 150
        f1 = np.empty(rm.TAIL_P)
        g1 = np.empty((rm.TAIL_P, rm.TAIL_D))
        for k in range(rm.TAIL_P):
            fk, gk = eng.ei_grad_batch(pts[k:k + 1])
            f1[k], g1[k] = fk[0], gk[0]
        assert np.array_equal(f1, f) and np.array_equal(g1, gr)
    print("\n".join(report))
    assert not failures, "\n".join(report)
