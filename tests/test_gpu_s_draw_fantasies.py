"""spx_draw_fantasies -- the posterior of the pending points, the fantasies, bests and Gamma formed by the library from
P x S standard normals (csrc/fantasy_kernels.hip) -- element by element against the two host forms, through the EI pass
against the oracle of the pending branch at every shape where its two kernels take another path (pending rows across the
64-row tiles of the factor, both storage forms of the factor, P from 1 to 64, S across the 16 columns of a fill
workgroup), against the existing spx_set_fantasies path, its bit-level invariants, the handle's state machine, its error
returns, the multi-device handle and the choosers.  Sorted after test_gpu_n_pending_paths.py, whose helpers it uses."""
import os

import numpy as np
import numpy.random as npr
import pytest
from numpy.linalg import LinAlgError

from spearmint_amd import hostgp
from tests import constrained_refine_helpers as hp
from tests import fantasy_helpers as fh
from tests import pending_helpers as ph
from tests import refine_helpers as rh
from tests.pending_helpers import FLAG_KEEP_MOMENTS, FLAG_PER_SEC, FLAG_TIME_ONLY, options
from tests.test_gpu_a_parity import assert_ei_close
from tests.test_gpu_k_constrained_paths import assert_same, plan_chunks
from tests.test_gpu_n_pending_paths import FANT_RTOL, base_problem, check_oracle, refused, state_problem

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    from spearmint_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def fantasy_bits(eng, H):
    pf, b = fh.device_fantasies(eng, H)
    return {"pend_fant": pf, "bests": b}


def same_fantasies(a, b, what):
    assert np.array_equal(a["pend_fant"], b["pend_fant"], equal_nan=True), what
    assert np.array_equal(a["bests"], b["bests"], equal_nan=True), what


# ---- 1. the fantasies element by element -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(7))
def test_fantasies_element_by_element(eng, k):
    """get_pending_fantasies against hostgp.fantasize_from_factor_rows on the engine's OWN factor rows and gamma, and
    against the reference form hostgp.fantasize_pending: 1e-9 of the fantasies' scale on the four ordinary problems of
    tests/test_host_logic.py, 1e-6 on its three near-singular ones -- the project's bars for two forms of this
    quantity; bests likewise."""
    name, comp, pend, vals, row, covar, z, atol = fh.host_problems()[k]
    n, P = comp.shape[0], pend.shape[0]
    eng.set_covar(covar)
    eng.set_observations(np.concatenate((comp, pend)), np.concatenate((vals, np.zeros(P))))
    eng.set_hypers(row[None, :])
    eng.factor()
    eng.draw_fantasies(z, P)
    assert eng.stat("last_fantasies_device") == 1
    pf, bests = eng.get_pending_fantasies(0)
    l_rows, gam = eng.get_factor_rows(0, n, P)
    f1, b1 = hostgp.fantasize_from_factor_rows(vals, row, l_rows, gam, z)
    chol, _ = fh.host_factor(comp, pend, vals, row, covar)
    f0, b0 = hostgp.fantasize_pending(comp, pend, vals, row, chol[:n, :n], z, covar)
    scale = np.abs(f0).max()
    for which, f, b in (("factor rows", f1, b1), ("reference form", f0, b0)):
        ef, eb = float(np.max(np.abs(pf - f[n:])) / scale), float(np.max(np.abs(bests - b)) / scale)
        print("%s against %s: fantasies %.3g, bests %.3g of their scale (bar %.0e)" % (name, which, ef, eb, atol))
        assert ef <= atol and eb <= atol, (name, which, ef, eb)


def test_a_nan_among_the_values_makes_every_best_nan(eng):
    p = ph.problem(9100, N=70, D=3, H=2, S=5)
    cand = ph.candidates(p, 1, 200)
    vals = ph.padded_vals(p)
    vals[11] = np.nan
    ph.load(eng, p, cand)
    eng.set_observations(p.X, vals)
    eng.set_hypers(p.rows)
    eng.factor()
    eng.draw_fantasies(p.randn, 3)
    _, bests = fh.device_fantasies(eng, p.H)
    assert bests.shape == (2, 5) and np.all(np.isnan(bests))


# ---- 2. shapes against the oracle -----------------------------------------------------------------------------------------------
#          (rows resident, pending, D, H, M, S), one thing varied at a time from (150, 3, 3, 3, 700, 5)
SHAPES = ([(2, 1, 3, 3, 700, 5), (3, 1, 3, 3, 700, 5)]
          + [(n, 4, 3, 3, 700, 5) for n in (64, 65, 66, 67)]
          + [(n, 3, 3, 3, 700, 5) for n in (127, 128, 129, 130, 256, 257)]
          + [(2051, 3, 3, 1, 700, 5)]
          + [(n, P, 3, 3, 700, 5) for n in (150, 300) for P in (1, 2, 7, 63, 64)]
          + [(150, 3, 1, 3, 700, 5), (150, 3, 33, 3, 700, 5)]
          + [(150, 3, 3, 1, 700, 5), (150, 3, 3, 130, 300, 5)]
          + [(150, 3, 3, 3, 700, s) for s in (1, 128, 129)] + [(150, 3, 3, 2, 700, 4096)])


@pytest.mark.parametrize("n_rows,n_pend,D,H,M,S", SHAPES)
def test_shapes_match_oracle(eng, n_rows, n_pend, D, H, M, S):
    """The oracle is the reference chain: fantasies from hostgp's reference form (tests/refine_helpers.finish ->
    orc.fantasize) scored by orc.compute_ei_fantasies; the device gets only the normals."""
    # (H = 130 from the next block of seeds: at 9200 the ORACLE has an EI of 1.6e-297, and check_oracle exempts no value)
    base = 9210 if H == 130 else 9200
    p = ph.problem(base + 7 * n_rows + 5 * n_pend + 3 * D + H + M + S, N=n_rows, D=D, H=H, S=S, n_pend=n_pend)
    assert p.X.shape[0] == n_rows and p.pend.shape[0] == n_pend and p.randn.shape == (n_pend, S)
    cand = ph.candidates(p, n_rows + M, M)
    res = fh.draw_pass(eng, p, cand)
    assert eng.stat("last_fantasies_device") == 1 and eng.stat("last_step_fused") == 0
    check_oracle(res, ph.oracle(p, cand))


@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE", "SE"])
def test_every_covar(eng, covar):
    p = ph.problem(9300 + len(covar), covar, N=247, D=3, H=4, S=9, n_pend=4)
    cand = ph.candidates(p, 11, 900)
    check_oracle(fh.draw_pass(eng, p, cand), ph.oracle(p, cand))


@pytest.mark.parametrize("n_rows,n_pend", [(130, 4), (150, 3), (66, 4)])
def test_both_storage_forms_of_the_factor(eng, n_rows, n_pend):
    """The one-launch factorisation leaves the factor tile-major, ei_flow = 0 row-major: the posterior kernel reads the
    bottom rows of either.  Both against the oracle, and the fantasies of the two within the first test's bar of each
    other (the two factorisations round differently)."""
    p = ph.problem(9400 + n_rows, N=n_rows, D=3, H=3, S=5, n_pend=n_pend)
    cand = ph.candidates(p, 12, 700)
    ref = ph.oracle(p, cand)
    check_oracle(fh.draw_pass(eng, p, cand), ref)
    assert eng.stat("last_factor_flow") == 1
    tiled = fantasy_bits(eng, p.H)
    with options(eng, ei_flow=0):
        check_oracle(fh.draw_pass(eng, p, cand), ref)
        assert eng.stat("last_factor_flow") == 0
        rowmajor = fantasy_bits(eng, p.H)
    scale = np.abs(tiled["pend_fant"]).max()
    assert np.max(np.abs(tiled["pend_fant"] - rowmajor["pend_fant"])) <= 1e-9 * scale


# ---- 3. against the existing path ---------------------------------------------------------------------------------------------
def through_set_fantasies(p, cand, pend_fant, bests, fn=None):
    """The device's fantasies handed to a second engine through spx_set_fantasies."""
    q = hp.Problem()
    q.__dict__.update(p.__dict__)
    q.fant, q.bests = fh.as_fant(p, pend_fant), np.ascontiguousarray(bests)
    return ph.fresh(ph.fant_pass if fn is None else fn, q, cand), q


@pytest.mark.parametrize("n_rows,n_pend,S", [(150, 3, 5), (247, 4, 12), (66, 4, 129)])
def test_against_set_fantasies(eng, n_rows, n_pend, S):
    p = ph.problem(9500 + n_rows, N=n_rows, D=3, H=3, S=S, n_pend=n_pend)
    cand = ph.candidates(p, 13, 1000)
    got = fh.draw_pass(eng, p, cand)
    pf, bests = fh.device_fantasies(eng, p.H)
    want, _ = through_set_fantasies(p, cand, pf, bests)
    assert_ei_close(got["draws"], want["draws"], rtol=FANT_RTOL)
    np.testing.assert_allclose(got["mean"], want["mean"], rtol=FANT_RTOL, atol=0)
    assert got["best"][0] == want["best"][0]


# ---- 4. bit-level invariants ----------------------------------------------------------------------------------------------------
def test_repeats_fresh_handles_and_shared_normals_give_the_same_bits(eng):
    p, cand = state_problem(9600)
    first = fh.draw_pass(eng, p, cand)
    bits = fantasy_bits(eng, p.H)
    eng.draw_fantasies(p.randn, 3)
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "a second call")
    same_fantasies(fantasy_bits(eng, p.H), bits, "a second call")
    ph.scramble(eng, p, cand)
    assert_same(fh.draw_pass(eng, p, cand), first, "after another problem")
    same_fantasies(fantasy_bits(eng, p.H), bits, "after another problem")
    assert_same(ph.fresh(fh.draw_pass, p, cand), first, "fresh")
    ph.scramble(eng, p, cand)
    assert_same(fh.draw_pass(eng, p, cand, z=np.stack([p.randn] * p.H)), first, "per draw")
    same_fantasies(fantasy_bits(eng, p.H), bits, "per draw")
    other = np.stack([p.randn, 2.0 * p.randn, p.randn[::-1]])        # and the draws really read their own
    fh.draw_pass(eng, p, cand, z=other)
    pf, _ = fh.device_fantasies(eng, p.H)
    assert np.array_equal(pf[0], bits["pend_fant"][0]) and not np.array_equal(pf[1], bits["pend_fant"][1])


def test_a_column_does_not_depend_on_the_others(eng):
    p = ph.problem(9610, N=150, D=3, H=3, S=129)
    cand = ph.candidates(p, 14, 300)
    fh.draw_pass(eng, p, cand)
    big = fantasy_bits(eng, p.H)
    fh.draw_pass(eng, p, cand, z=np.ascontiguousarray(p.randn[:, :5]))
    small = fantasy_bits(eng, p.H)
    assert small["pend_fant"].shape == (3, 3, 5)
    assert np.array_equal(small["pend_fant"], big["pend_fant"][:, :, :5]) and np.array_equal(small["bests"], big["bests"][:, :5])


@pytest.mark.parametrize("variant", ["chunks", "streams2", "streams2+chunks", "gemm_partial0", "gemm_partial1",
                                     "stage_copies0", "stage_copies1", "timing", "cov_flat0", "cov_flat1", "cov_flat0+chunks",
                                     "ei_flow1", "keep_moments"])
@pytest.mark.parametrize("name", ["general", "small"])
def test_path_variants_do_not_change_bits(eng, name, variant):
    p, cand, _, budget = base_problem(name)
    base = fh.draw_pass(eng, p, cand)
    check_oracle(base, base_problem(name)[2])
    assert plan_chunks(cand.shape[0], p.X.shape[0], p.H, budget)[0] >= 5
    ph.scramble(eng, p, cand)
    kw = {"chunks": dict(kstar_budget_bytes=budget), "streams2": dict(streams=2),
          "streams2+chunks": dict(streams=2, kstar_budget_bytes=budget), "gemm_partial0": dict(gemm_partial=0),
          "gemm_partial1": dict(gemm_partial=1), "stage_copies0": dict(stage_copies=0), "stage_copies1": dict(stage_copies=1), "timing": dict(timing=1),
          "cov_flat0": dict(cov_flat=0), "cov_flat1": dict(cov_flat=1),
          "cov_flat0+chunks": dict(cov_flat=0, kstar_budget_bytes=budget), "ei_flow1": dict(ei_flow=1),
          "keep_moments": {}}[variant]
    with options(eng, **kw):
        got = fh.draw_pass(eng, p, cand, flags=FLAG_KEEP_MOMENTS if variant == "keep_moments" else 0)
    assert_same(got, base, (name, variant))


# ---- 5. the handle's state machine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["factor", "ei_step", "clear", "clear_set", "set_observations", "set_hypers", "covar_other",
                                 "gp_logprob"])
def test_what_drops_the_fantasies(eng, how):
    p, cand = state_problem()
    first = fh.draw_pass(eng, p, cand)
    assert eng.stat("last_fantasies_device") == 1
    q = p
    if how == "factor":
        eng.factor()
    elif how == "clear":
        eng.draw_fantasies(None, 0)
    elif how == "clear_set":
        eng.set_fantasies(None, None)
    elif how != "ei_step":
        if how == "set_observations":
            eng.set_observations(p.X, ph.padded_vals(p))
            eng.set_hypers(p.rows)
        elif how == "set_hypers":
            eng.set_hypers(p.rows)
        elif how == "covar_other":
            eng.set_covar("Matern32")
            q = ph.with_columns(p, 0, p.S)
            q.covar = "Matern32"
        else:
            assert np.all(np.isfinite(eng.gp_logprob()))
        assert eng.stat("last_fantasies_device") == 0
        refused(eng.ei_run, 0)
        refused(eng.draw_fantasies, p.randn, 3)
        refused(eng.get_pending_fantasies, 0)
        eng.factor()
    if how == "ei_step":
        eng.ei_step(0)
    else:
        eng.ei_run(0)
    assert eng.stat("last_fantasies_device") == 0
    refused(eng.get_pending_fantasies, 0)
    got = ph.collect(eng)
    assert_same(got, ph.fresh(ph.plain_pass, q, cand), how)
    assert not np.array_equal(got["draws"], first["draws"])
    assert_same(fh.draw_pass(eng, p, cand), first, "drawn again")


def test_what_keeps_the_fantasies(eng):
    p, cand = state_problem()
    first = fh.draw_pass(eng, p, cand)
    bits = fantasy_bits(eng, p.H)
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "a second pass")
    eng.set_covar(p.covar)
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "covar set to its own value")
    f, g = eng.ei_grad_batch(rh.points(p, 3, 9))
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "ei_grad_batch in between")
    more = ph.candidates(p, 18, 2500)
    for M in (300, 127, 2500, 129):
        eng.set_candidates(more[:M])
        eng.ei_run(0)
        assert_same(ph.collect(eng), ph.fresh(fh.draw_pass, p, more[:M]), M)
    with_time = fh.draw_pass(eng, p, cand, time_model=True)
    assert_same(with_time, first, "a time model does not change the plain flags' pass")
    eng.ei_run(FLAG_PER_SEC | FLAG_KEEP_MOMENTS | FLAG_TIME_ONLY)
    refused(eng.ei_draws)
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "TIME_ONLY in between")
    assert eng.stat("last_fantasies_device") == 1
    same_fantasies(fantasy_bits(eng, p.H), bits, "still there")


def test_the_stat_follows_who_formed_the_fantasies(eng):
    p, cand = state_problem()
    ph.load(eng, p, cand)
    assert eng.stat("last_fantasies_device") == 0
    refused(eng.draw_fantasies, p.randn, 3)                      # not factored
    eng.ei_step(0)                                               # a step leaves a checked factor behind
    eng.draw_fantasies(p.randn, 3)
    assert eng.stat("last_fantasies_device") == 1
    eng.ei_run(0)
    first = ph.collect(eng)
    assert_same(first, ph.fresh(fh.draw_pass, p, cand), "after a step")
    check_oracle(first, ph.oracle(p, cand))
    eng.set_fantasies(p.fant, p.bests)
    assert eng.stat("last_fantasies_device") == 0
    refused(eng.get_pending_fantasies, 0)
    eng.ei_run(0)
    assert_same(ph.collect(eng), ph.fresh(ph.fant_pass, p, cand), "the host's fantasies")
    eng.draw_fantasies(p.randn, 3)
    assert eng.stat("last_fantasies_device") == 1
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "and back")


def test_counts_grow_and_shrink_on_one_handle(eng):
    for i, (P, S) in enumerate(((3, 5), (3, 300), (7, 5), (1, 1), (64, 40), (2, 4096), (3, 5))):
        p = ph.problem(9700 + P, N=150, D=3, H=2, S=S, n_pend=P)
        cand = ph.candidates(p, 17, 400)
        got = fh.draw_pass(eng, p, cand)
        assert_same(got, ph.fresh(fh.draw_pass, p, cand), (i, P, S))
        if i in (1, 4, 5):
            check_oracle(got, ph.oracle(p, cand))


@pytest.mark.parametrize("covar", ["Matern52", "ARDSE"])
def test_refinement_objective_after_draw_fantasies(eng, covar):
    """spx_ei_grad_batch with the device's fantasies against the same call after spx_set_fantasies of those fantasies
    (a second engine), at the tolerances tests/test_gpu_m_refine_paths.py holds the fantasy branch to its oracle with
    (tests/constrained_refine_helpers.assert_close) -- and against that oracle itself."""
    p = rh.make_problem(9800, covar, "fant", N=150, D=4, H=3, S=5)
    pts = rh.points(p, 4, 21)
    cand = ph.candidates(p, 19, 64)
    ph.load(eng, p, cand)
    eng.factor()
    eng.draw_fantasies(p.randn, p.pend.shape[0])
    f, g = eng.ei_grad_batch(pts)
    pf, bests = fh.device_fantasies(eng, p.H)

    def host_path(e, q, c):
        rh.setup(e, q, cand=c)
        return e.ei_grad_batch(pts)
    (f2, g2), _ = through_set_fantasies(p, cand, pf, bests, host_path)
    hp.assert_close(f, g, f2, g2)
    hp.assert_close(f, g, *rh.oracle(p, pts))


@pytest.mark.parametrize("allvalid", [False, True])
def test_constrained_objective_after_draw_fantasies(eng, allvalid):
    """spx_constrained_ei_grad_batch: the refinement's shared normals (one private RandomState) through draw_fantasies
    against tests/constrained_refine_helpers.setup's spx_set_fantasies, and the host oracle."""
    from spearmint_amd.engine import Engine
    p = hp.make_problem(9900, D=3, n_valid=40 if allvalid else 30, n_full=40, H=2, S=5, n_pend=3)
    pts = hp.points(p, 5, 11)
    ref = Engine(0)
    try:
        hp.setup(ref, p)
        f2, g2 = ref.constrained_ei_grad_batch(pts, p.best)
    finally:
        ref.close()
    hp.setup(eng, p)
    rs = npr.RandomState()
    rs.set_state(p.randomstate)
    eng.draw_fantasies(rs.randn(3, p.S), 3)
    assert eng.stat("last_fantasies_device") == 1
    f, g = eng.constrained_ei_grad_batch(pts, p.best)
    hp.assert_close(f, g, f2, g2)
    hp.assert_close(f, g, *hp.oracle(p, pts))


def test_per_second_with_device_fantasies(eng):
    p = ph.problem(6000, N=247, D=3, H=4, S=12, n_pend=4)
    cand = ph.candidates(p, 16, 3000)
    tmean = np.stack([ph.oracle_time_mean(p, cand, h) for h in range(p.H)], axis=1)
    assert np.max(tmean) / np.min(tmean) > 1.5
    keep = FLAG_PER_SEC | FLAG_KEEP_MOMENTS
    got = fh.draw_pass(eng, p, cand, flags=keep, time_model=True)
    check_oracle(got, ph.oracle(p, cand) / tmean)
    tm = np.stack([eng.get_time_mean(h) for h in range(p.H)], axis=1)
    np.testing.assert_allclose(tm, tmean, rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        eng.get_moments(0)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
def test_arguments_out_of_range_are_refused(eng):
    p = ph.problem(9950, N=150, D=3, H=2, S=5)
    cand = ph.candidates(p, 20, 300)
    rs = np.random.RandomState(0)
    first = fh.draw_pass(eng, p, cand)
    refused(eng.draw_fantasies, np.zeros((0, 5)), 0)             # P = 0
    refused(eng.draw_fantasies, rs.randn(65, 5), 65)             # P = 65
    refused(eng.draw_fantasies, rs.randn(3, 4097), 3)            # S = 4097
    eng.ei_run(0)                                                # the handle is usable, the fantasies still in force
    assert_same(ph.collect(eng), first, "after the refusals")
    small = ph.problem(9951, N=5, D=3, H=2, S=5, n_pend=3)
    ph.load(eng, small, cand)
    eng.factor()
    refused(eng.draw_fantasies, rs.randn(5, 5), 5)               # P = n
    eng.draw_fantasies(rs.randn(4, 5), 4)                        # P = n - 1 is the most


def test_refused_in_the_2d_partition(eng):
    from spearmint_amd.engine import MultiEngine
    p = ph.problem(8100, N=150, D=3, H=4, S=5)
    cand = ph.candidates(p, 20, 1000)
    single = fh.draw_pass(eng, p, cand)
    m = MultiEngine([0, 0])
    try:
        m.set_partition(2)
        ph.load(m, p, cand)
        m.factor()
        with pytest.raises(ValueError, match="partition"):
            m.draw_fantasies(p.randn, 3)
        m.set_partition(1)
        assert_same(fh.draw_pass(m, p, cand), single, "back to candidates only")
    finally:
        m.close()


def test_not_positive_definite_is_an_error_return(eng):
    """P = 1, noise = 4, amp2 = 1e-40, unit length scales: the covariance is 4 I in binary arithmetic, L_S = 2 and
    pend_K = 2 * 2 - 4 = 0, which spla.cholesky refuses.  The device's verdict must be the host form's on the engine's own
    row (one rounding each for P = 1, so the two cannot differ).  Draw 0 is an ordinary one."""
    p = ph.problem(9960, N=40, D=3, H=2, S=5, n_pend=1)
    cand = ph.candidates(p, 21, 300)
    rows = p.rows.copy()
    rows[1] = np.concatenate(([0.2, 4.0, 1e-40], np.ones(3)))
    q = ph.with_columns(p, 0, p.S)
    q.rows = rows
    ph.load(eng, q, cand)
    eng.factor()
    n = p.vals.shape[0]
    l_rows, gam = eng.get_factor_rows(1, n, 1)
    try:
        hostgp.fantasize_from_factor_rows(p.vals, rows[1], l_rows, gam, p.randn)
        host_raises = False
    except LinAlgError:
        host_raises = True
    assert host_raises and l_rows[0, n] == 2.0
    with pytest.raises(LinAlgError):
        eng.draw_fantasies(p.randn, 1)
    assert eng.not_pd_info() == (4 * 2 + 1, 0)
    assert eng.stat("last_fantasies_device") == 0
    refused(eng.get_pending_fantasies, 0)
    eng.ei_run(0)                                                # no fantasies: the plain pass
    assert_same(ph.collect(eng), ph.fresh(ph.plain_pass, q, cand), "the plain pass")
    good = fh.draw_pass(eng, p, cand)                            # and the handle recovers
    assert_same(good, ph.fresh(fh.draw_pass, p, cand), "recovered")
    assert eng.not_pd_info() == (-1, -1)


# ---- 7. the multi-device handle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [12, 300])
def test_three_engines_shard_the_candidates(eng, S):
    from spearmint_amd.engine import MultiEngine
    p = ph.problem(8010 + S, N=247, D=3, H=3, S=S, n_pend=4)
    cand = ph.candidates(p, 19, 1000)
    single = fh.draw_pass(eng, p, cand)
    bits = fantasy_bits(eng, p.H)
    check_oracle(single, ph.oracle(p, cand))
    m = MultiEngine([0, 0, 0])
    try:
        assert_same(fh.draw_pass(m, p, cand), single, "three engines")
        assert m.stat("last_fantasies_device") == 1
        same_fantasies(fantasy_bits(m, p.H), bits, "slot 0")
        m.draw_fantasies(None, 0)
        m.ei_run(0)
        assert_same(ph.collect(m), ph.fresh(ph.plain_pass, p, cand), "cleared")
    finally:
        m.close()


# ---- 8. the choosers ----------------------------------------------------------------------------------------------------------------
def test_opt_chooser_pending_golden_either_way(golden_dir, tmp_path):
    from spearmint_amd.chooser import GPEIOptChooser
    g = np.load(os.path.join(golden_dir, "chooser_next_pending.npz"))
    args = (g["grid"], g["values"], g["durations"], g["candidates"], g["pending"], g["complete"])
    out = {}
    for flag in (1, 0):
        d = tmp_path / str(flag)
        d.mkdir()
        op = GPEIOptChooser.init(str(d), "mcmc_iters=3,burnin=4,grid_subset=3,pending_samples=8,use_multiprocessing=0,"
                                         "gpu_fantasies=%d" % flag)
        npr.seed(int(g["o_seed"]))
        job = op.next(*args)
        st = npr.get_state()
        assert op.engine().stat("last_fantasies_device") == flag
        if int(g["o_is_new"]):
            assert isinstance(job, tuple) and job[0] == int(g["o_index"]) and np.allclose(job[1], g["o_point"], atol=1e-5)
        else:
            assert job == int(g["o_index"])
        out[flag] = (job, st)
        op.engine().close()
    assert np.array_equal(out[0][1][1], out[1][1][1]) and out[0][1][2:] == out[1][1][2:]
    if isinstance(out[0][0], tuple):
        assert out[0][0][0] == out[1][0][0] and np.allclose(out[0][0][1], out[1][0][1], atol=1e-5)
    else:
        assert out[0][0] == out[1][0]


def test_constrained_chooser_pending_golden_either_way(golden_dir, tmp_path):
    """The reference's `nan` sequence of GPConstrainedEIChooser: its third call has a pending job."""
    from spearmint_amd.chooser import GPConstrainedEIChooser
    g = np.load(os.path.join(golden_dir, "constrained_next_nan.npz"))
    out = {}
    for flag in (1, 0):
        d = tmp_path / str(flag)
        d.mkdir()
        c = GPConstrainedEIChooser.init(str(d), str(g["args"]) + ",gpu_fantasies=%d" % flag)
        st = npr.get_state()
        for k in range(int(g["ncalls"])):
            npr.set_state((st[0], g["before%d_key" % k], int(g["before%d_pos" % k]), int(g["before%d_has_gauss" % k]),
                           float(g["before%d_cached" % k])))
            ret = c.next(g["grid"], g["values"], np.ones(g["grid"].shape[0]), g["candidates%d" % k], g["pending%d" % k],
                         g["complete%d" % k])
            st = npr.get_state()
        k = int(g["ncalls"]) - 1
        assert len(g["pending%d" % k]) == 1
        assert c.engine().stat("last_fantasies_device") == flag
        np.testing.assert_allclose(c.last_overall_ei, g["overall_ei%d" % k], rtol=1e-6, atol=1e-12)
        if isinstance(ret, tuple):
            assert ret[0] == int(g["ret_idx%d" % k])
            np.testing.assert_allclose(ret[1], g["ret_pt%d" % k], rtol=1e-6, atol=1e-9)
        else:
            assert ret == int(g["ret_idx%d" % k])
        np.testing.assert_array_equal(st[1], g["after%d_key" % k])
        assert st[2] == int(g["after%d_pos" % k])
        out[flag] = (ret, st)
        c.engine().close()
    assert np.array_equal(out[0][1][1], out[1][1][1]) and out[0][1][2:] == out[1][1][2:]
    assert type(out[0][0]) is type(out[1][0])
