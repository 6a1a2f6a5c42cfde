"""The per-second branch of the grid pass (spx_set_time_model, SPX_FLAG_PER_SEC, SPX_FLAG_TIME_ONLY, spx_get_time_mean -- what
GPEIperSecChooser runs on every call): the predicted duration exp(k_t(x, X)' alpha_t + mean_t) of k_cov<MODE 2> against a
50-digit yardstick (tests/persec_mp.py), every execution path of ei_run_impl bit for bit with more than one chunk, the pad
boundaries against the float64 oracle, the division ei / time_m at inf, 0, denormal and NaN, and the handle's state machine.
Sorted after the parity, pending and yardstick files, which should be read first when they fail too.

1(a), the derived budget (tests/persec_mp.py's docstring has the derivation): with u the unit of tests/cov_mp.py,
    dP = |alpha| amp2 (CEILING u + 2^-1075) + 6.5 x 2^-52 |P| + 2^-1075,   dE = dP + 2^-53 |E|,
    |T - T_ref| <= T expm1(dE) + 1.5 ulp(T)
where 1 of the 1.5 ulp is the exponential's own bound.  The ROCm installation carries no accuracy statement for the device library's
exp, so that bound is the float64 oracle's: np.exp measured against mpmath on the same arguments (0.60 ulp, tests/test_persec_mp.py),
rounded up to the whole ulp.  The budget is at most 1.2e-13 relative over the family.  Measured on an MI355X, worst
|T - T_ref| / budget over the five sizes: Matern52 0.716, Matern32 0.714, ARDSE 0.716 (the float64 oracle: 0.716, 0.712, 0.716);
the denormal durations of section 4 are exact.

1(b): the device's worst relative error per (covar, N, D, draw) against 50 digits on the library's OWN K_t is at most
max(4 x the float64 oracle's on the same K_t, 16 eps) -- the bar and the reasoning of tests/test_gpu_o_factor_pivots.py and
tests/test_gpu_k_constrained_paths.py: both are backward-stable solves that differ in blocking and summation order only.
Measured on an MI355X, worst over N, D and the draws (device / oracle / largest ratio of one draw), cond(K_t) 1.6e1 ... 1.3e5:
Matern52 3.2e-13 / 2.1e-13 / 1.67, Matern32 1.1e-13 / 6.7e-14 / 2.54, ARDSE 7.1e-13 / 5.3e-13 / 3.73, SE 6.8e-13 / 4.1e-13 / 1.88."""
import os

import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import cov_mp as cv
from tests import factor_helpers as fh
from tests import pending_helpers as ph
from tests import persec_helpers as ps
from tests import persec_mp as pm
from tests.persec_helpers import KEEP, KEEP_MOMENTS, PER_SEC, TIME_ONLY
from tests.test_gpu_a_parity import assert_ei_close
from tests.test_gpu_k_constrained_paths import plan_chunks

pytestmark = pytest.mark.gpu
LD = np.longdouble
FLOOR = 16 * np.finfo(float).eps


@pytest.fixture()
def eng():
    from spearmint_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "persec_mp.npz")))


@pytest.fixture(scope="module")
def cov_fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "cov_lattice_mp.npz")))


# ---- 1(a). a diagonal K_t: the derived budget -------------------------------------------------------------------------------
def diag_load(eng, kind, N, means=pm.MEAN_T, denormal=False):
    X, C, owner, delta, ld = pm.diag_problem(N, denormal)
    eng.set_covar(kind)
    eng.set_observations(X, pm.objective_vals(N))
    eng.set_candidates(C)
    eng.set_hypers(pm.objective_rows())
    eng.set_time_model(ld, pm.time_rows(means))
    return owner, delta


@pytest.mark.parametrize("kind", cv.KINDS)
@pytest.mark.parametrize("N", pm.SIZES)
def test_duration_of_a_diagonal_time_model_is_within_its_derived_budget(eng, fixture, cov_fixture, kind, N):
    owner, delta = diag_load(eng, kind, N)
    base = ps.step(eng)
    assert eng.stat("last_step_fused") == int(N <= 128)
    T_ref = fixture["T_%s_%d" % (kind, N)]
    allowed = pm.budget(cov_fixture, kind, N, T_ref)
    err = np.abs(base["tmean"].astype(LD) - T_ref.astype(LD))
    worst = float(np.max(err / allowed))
    print("T diag %-9s N %3d: worst |T - T_ref| / budget = %.3f (budget up to %.2e relative)"
          % (kind, N, worst, float(np.max(allowed / T_ref.astype(LD)))))
    assert worst <= 1.0
    # past the clamp for every observation: the sum is +0.0 and the result exp(mean_t) -- one rounding, the exponential's, the
    # same bits in every block; the library's exp of 0 is exactly 1
    past = (owner < 0) | (delta ** 2 > cv.CLAMP[kind])
    assert np.sum(owner < 0) == 3 and np.sum(past) >= 3
    for h, mean in enumerate(pm.MEAN_T):
        v = base["tmean"][past, h]
        assert np.all(v == v[0]), h
        assert abs(LD(v[0]) - LD(T_ref[-1, h])) <= LD(pm.EXP_ULPS) * LD(np.spacing(T_ref[-1, h]))
        assert mean != 0.0 or v[0] == 1.0
    # the same bits from the fused kernel (which takes time_m as an input), the three-stage path on one, two and three
    # streams, and the time-only pass of each
    runs = {}
    for label, opts in (("default", {}), ("unfused", dict(ei_fused=0)), ("streams2", dict(ei_fused=0, streams=2)),
                        ("streams3", dict(ei_fused=0, streams=3))):
        with ph.options(eng, **opts):
            diag_load(eng, kind, N)
            runs[label] = ps.step(eng)
            assert eng.stat("last_step_fused") == int(N <= 128 and label == "default")
            diag_load(eng, kind, N)
            runs[label + "+time_only"] = ps.step(eng, KEEP | TIME_ONLY)
            with pytest.raises(ValueError):
                eng.ei_draws()
    for label, got in runs.items():
        ps.assert_same(got, base, (kind, N, label))


# ---- 1(b). a full K_t: the bar taken from the float64 oracle ----------------------------------------------------------------
@pytest.mark.parametrize("covar", pm.FULL_COVARS)
@pytest.mark.parametrize("N,D", [(N, D) for N in pm.FULL_N for D in pm.FULL_D])
def test_duration_against_50_digits_on_the_librarys_own_kt(eng, covar, N, D):
    X, C, vals, ld, rows, trows = pm.full_problem(covar, N, D)
    H = rows.shape[0]
    ps.load(eng, (X, C, vals, rows, ld, trows), covar)
    res = ps.step(eng)
    conds, report, failures = [], [], []
    for d in range(H):
        K = eng.get_factor(H + d, want_L=False, want_alpha=False)[0]        # the time model's draws follow the objective's
        assert np.array_equal(K, K.T) and np.allclose(K, pm.host_kt(covar, X, trows[d]), rtol=1e-12, atol=0)
        conds.append(np.linalg.cond(K))
        ref = pm.full_reference(covar, K, X, C, trows[d], ld)
        e_dev = pm.rel_error(res["tmean"][:, d], ref)
        e_orc = pm.rel_error(pm.oracle_time_mean(covar, K, X, C, trows[d], ld), ref)
        report.append("T full %-9s N %2d D %d draw %d cond %.1e: device %.3g oracle %.3g ratio %.3g"
                      % (covar, N, D, d, conds[-1], e_dev, e_orc, e_dev / e_orc if e_orc else np.inf))
        if not e_dev <= max(4 * e_orc, FLOOR):
            failures.append(report[-1])
    print("\n".join(report))
    assert min(conds) <= 1e2 and max(conds) >= 1e4, conds
    assert not failures, "\n".join(report)


# ---- 2. every execution path, bit for bit -----------------------------------------------------------------------------------
#          name: (N, M, D, H, seed, fused)
BASES = {"general": (300, 5000, 7, 5, 1201, False),        # three-stage path, Np = 384
         "fused": (101, 5000, 4, 5, 1202, True),           # k_ei_fused128
         "padskip": (257, 5000, 5, 5, 1203, False),        # one live 16-row tile in the last row block: the GEMM skips the padding
         "big": (1000, 600, 6, 5, 1204, False)}            # Np = 1024: 512 rows per workgroup in k_cov, few candidates


def budgets(name):
    """(chunked budget, its chunk count, the budget of ONE chunk with one draw per group)."""
    N, M, D, H, seed, fused = BASES[name]
    Np, Mp = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    small = 8 * Np * (256 if name == "big" else 1024)
    nchunks, hb = plan_chunks(M, N, H, small)
    assert nchunks >= 3 and hb < H, (nchunks, hb)            # at least 3 chunks, more than one draw group
    groups = 8 * Np * Mp
    assert plan_chunks(M, N, H, groups) == (1, 1)
    return small, nchunks, groups


def default_run(eng, name):
    """The default step of a base, anchored to the oracle; then the handle scrambled and the base loaded again."""
    N, M, D, H, seed, fused = BASES[name]
    prob = ps.problem(N, M, D, H, seed)
    ps.load(eng, prob)
    base = ps.step(eng)
    ei_o, tm_o = ps.oracle(N, M, D, H, seed)
    assert_ei_close(base["draws"], ei_o)
    np.testing.assert_allclose(base["tmean"], tm_o, rtol=1e-9, atol=0)
    assert base["best"][0] == orc.choose(ei_o)
    assert np.array_equal(base["mean"], np.mean(base["draws"], axis=1)) and base["best"][1] == base["mean"][base["best"][0]]
    assert eng.stat("last_step_fused") == int(fused)
    skips = ph.padding_plan(N)[1]
    assert eng.stat("last_step_skipped_padding") == int(skips and not fused) and (skips or name != "padskip")
    rescramble(eng, prob)
    return prob, base


def rescramble(eng, prob):
    ps.scramble(eng, prob)
    ps.load(eng, prob)


#            label: (options; True stands for the base's chunked budget, "groups" for its one-chunk budget), entry, flags
VARIANTS = {"chunks": (dict(kstar_budget_bytes=True), "step", KEEP),
            "one_draw_per_group": (dict(kstar_budget_bytes="groups"), "step", KEEP),
            "streams2": (dict(streams=2), "step", KEEP),
            "streams2+chunks": (dict(streams=2, kstar_budget_bytes=True), "step", KEEP),
            "streams3": (dict(streams=3), "step", KEEP),
            "streams3+chunks": (dict(streams=3, kstar_budget_bytes=True), "step", KEEP),
            "unfused": (dict(ei_fused=0), "step", KEEP),
            "unfused+chunks": (dict(ei_fused=0, kstar_budget_bytes=True), "step", KEEP),
            "no_gemm_partial+chunks": (dict(gemm_partial=0, kstar_budget_bytes=True), "step", KEEP),
            "no_cov_flat": (dict(cov_flat=0), "step", KEEP),
            "no_cov_flat+chunks": (dict(cov_flat=0, kstar_budget_bytes=True), "step", KEEP),
            "ei_flow0+chunks": (dict(ei_flow=0, kstar_budget_bytes=True), "step", KEEP),
            "ei_flow1+chunks": (dict(ei_flow=1, kstar_budget_bytes=True), "step", KEEP),
            "factor+run": ({}, "factor", KEEP),
            "factor+run+chunks": (dict(kstar_budget_bytes=True), "factor", KEEP),
            "factor+run+streams2+chunks": (dict(streams=2, kstar_budget_bytes=True), "factor", KEEP),
            "no_keep_moments+chunks": (dict(kstar_budget_bytes=True), "step", PER_SEC),
            "no_keep_moments+streams2+chunks": (dict(streams=2, kstar_budget_bytes=True), "step", PER_SEC),
            "time_only": ({}, "step", KEEP | TIME_ONLY),
            "time_only+chunks": (dict(kstar_budget_bytes=True), "step", KEEP | TIME_ONLY),
            "time_only+streams2+chunks": (dict(streams=2, kstar_budget_bytes=True), "step", KEEP | TIME_ONLY),
            "time_only+streams3+chunks": (dict(streams=3, kstar_budget_bytes=True), "step", KEEP | TIME_ONLY),
            "time_only+factor+run+chunks": (dict(kstar_budget_bytes=True), "factor", KEEP | TIME_ONLY)}


def _opts(name, opts):
    small, nchunks, groups = budgets(name)
    kw = dict(opts)
    if "kstar_budget_bytes" in kw:
        kw["kstar_budget_bytes"] = small if kw["kstar_budget_bytes"] is True else groups
    return kw


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(BASES))
def test_variants_do_not_change_bits(eng, name, variant):
    prob, base = default_run(eng, name)
    opts, entry, flags = VARIANTS[variant]
    with ph.options(eng, **_opts(name, opts)):
        got = ps.step(eng, flags) if entry == "step" else ps.factor_run(eng, flags)
        if not flags & TIME_ONLY:
            assert eng.stat("last_step_fused") == int(BASES[name][5] and opts.get("ei_fused", -1) != 0)
            if opts.get("streams") == 3:        # the ring is the three-stage path's: a fused pass runs on one stream
                assert (eng.stat("last_kstar_ring") >= 1) == (not BASES[name][5])
    ps.assert_same(got, base, (name, variant))
    if flags & TIME_ONLY:
        with pytest.raises(ValueError):
            eng.best()
    if not flags & KEEP_MOMENTS:
        with pytest.raises(ValueError):
            eng.get_time_mean(0)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("name", sorted(BASES))
def test_step_overlap_with_several_chunks_does_not_change_bits(eng, name, overlap):
    """A step's first chunk puts the duration launches on the main stream with the OTHER parity's scaling buffers while the
    objective's scaling runs on the second stream; chunk 1, which owns that parity, follows on the main stream.  Three times,
    the handle scrambled in between (an ordering that holds by luck does not hold every time)."""
    prob, base = default_run(eng, name)
    small, nchunks, groups = budgets(name)
    for rep in range(3):
        with ph.options(eng, step_overlap=overlap, kstar_budget_bytes=small):
            got = ps.step(eng)
        ps.assert_same(got, base, (name, overlap, rep))
        with ph.options(eng, step_overlap=overlap, kstar_budget_bytes=small):
            rescramble(eng, prob)
            ps.assert_same(ps.step(eng, KEEP | TIME_ONLY), base, (name, overlap, rep, "time only"))
        rescramble(eng, prob)


@pytest.mark.parametrize("name", sorted(BASES))
def test_small_budget_really_chunks(eng, name):
    """The timed form of the pass with the small budget: cross_mean is one launch per chunk (all draws), and the launch
    counts of the three-stage path say that every draw was a group of its own."""
    prob, base = default_run(eng, name)
    N, M, D, H, seed, fused = BASES[name]
    small, nchunks, groups = budgets(name)
    with ph.options(eng, kstar_budget_bytes=small, timing=1):
        got = ps.factor_run(eng)
        t = eng.timings()
    ps.assert_same(got, base, name)
    assert t["cross_mean"][1] == nchunks
    if fused:
        assert t["predict_gemm"][1] == nchunks and t["ei_finalize"][1] == 0 and t["cov_cross"][1] == 0
    else:
        assert t["ei_finalize"][1] == nchunks and t["predict_gemm"][1] == nchunks * H and t["cov_cross"][1] == nchunks * H
    rescramble(eng, prob)
    with ph.options(eng, kstar_budget_bytes=groups, timing=1):
        got = ps.factor_run(eng)
        t = eng.timings()
    ps.assert_same(got, base, (name, "groups"))
    assert t["cross_mean"][1] == 1 and (fused or t["cov_cross"][1] == H)


def test_fantasies_per_second_chunked_in_a_step_with_overlap(eng):
    """Pending jobs with a time model over the same resident rows: the first pass a whole step (with and without the
    overlap, on one and two streams), then the fantasies and the per-second pass, chunked with one draw per group -- so
    k_ei_fant_mean reads time_m + h0 * mc for h0 > 0."""
    p = ph.problem(31, N=150, H=5, S=5)
    cand = ph.candidates(p, 32, 3000)
    small = 8 * 256 * 512
    nchunks, hb = plan_chunks(3000, 150, 5, small)
    assert nchunks >= 3 and hb == 1

    def run(e, entry="factor"):
        res = ph.fant_pass(e, p, cand, flags=KEEP, entry=entry, time_model=True)
        res["tmean"] = np.stack([e.get_time_mean(h) for h in range(p.H)], axis=1)
        with pytest.raises(ValueError):
            e.get_moments(0)
        return res

    base = run(eng)
    tm_o = np.stack([ph.oracle_time_mean(p, cand, h) for h in range(p.H)], axis=1)
    np.testing.assert_allclose(base["tmean"], tm_o, rtol=1e-9, atol=0)
    with np.errstate(all="ignore"):
        ei_o = ph.oracle(p, cand) / tm_o
    assert_ei_close(base["draws"], ei_o)
    assert base["best"][0] == orc.choose(ei_o)
    for kw in (dict(kstar_budget_bytes=small, streams=2, step_overlap=1), dict(kstar_budget_bytes=small, step_overlap=1),
               dict(kstar_budget_bytes=small, step_overlap=0)):
        ph.scramble(eng, p, cand)
        with ph.options(eng, **kw):
            got = run(eng, "step")
        ps.assert_same(got, base, sorted(kw.items()))


# ---- 3. shapes against the oracle -------------------------------------------------------------------------------------------
def check_shape(eng, N, M, D, H, seed, covar="Matern52", prob=None, **opts):
    prob = ps.problem(N, M, D, H, seed) if prob is None else prob
    with ph.options(eng, **opts):
        ps.load(eng, prob, covar)
        res = ps.step(eng)
    ei_o, tm_o = ps.oracle_of(prob, covar)
    np.testing.assert_allclose(res["tmean"], tm_o, rtol=1e-9, atol=0)
    assert_ei_close(res["draws"], ei_o)
    assert res["best"][0] == orc.choose(ei_o)
    assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1))
    assert eng.stat("last_step_fused") == int(N <= 128 and opts.get("ei_fused", -1) != 0)
    return prob, res


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 1025])
def test_observation_counts_across_the_pads(eng, N):
    check_shape(eng, N, 700, 3, 3, 2000 + N)


@pytest.mark.parametrize("N", [70, 150])
@pytest.mark.parametrize("D", [1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 100])
def test_dimensions_across_the_feature_quads(eng, N, D):
    """Dp / 4 = 1, 2, 4, 8 feature quads per lane group and the chunk loop above 32 dimensions, fused and three-stage."""
    check_shape(eng, N, 700, D, 3, 2100 + N + D)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 128, 129, 257])
def test_candidate_counts_across_the_column_blocks(eng, M):
    check_shape(eng, 150, M, 3, 3, 2300 + M)


@pytest.mark.parametrize("N,H,M", [(130, 1, 700), (130, 16, 700), (130, 17, 700), (2049, 2, 200)])
def test_draw_counts_across_the_joint_factorisation(eng, N, H, M):
    """A time model doubles the rows of the factorisation: 2 H = 2, 32, 34 (spx_factor changes form above 32 rows).  Beyond
    it (and at N = 2049) every draw's durations are, bit for bit, those of a handle that holds that draw alone."""
    prob, res = check_shape(eng, N, M, 3, H, 2400 + N + H)
    comp, cand, vals, hypers, ld, th = prob
    if 2 * H <= 32 and N < 2049:
        return
    for d in range(H):
        ps.load(eng, (comp, cand, vals, hypers[d:d + 1], ld, th[d:d + 1]))
        alone = ps.step(eng)
        assert np.array_equal(alone["tmean"][:, 0], res["tmean"][:, d]), d


@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE", "SE"])
def test_every_covar_with_several_chunks(eng, covar):
    N, M, D, H = 300, 5000, 3, 4
    small = 8 * 384 * 1024
    nchunks, hb = plan_chunks(M, N, H, small)
    assert nchunks >= 3 and hb == 1
    prob, res = check_shape(eng, N, M, D, H, 2500, covar, kstar_budget_bytes=small)
    prob, two = check_shape(eng, N, M, D, H, 2500, covar, kstar_budget_bytes=small, streams=2)
    ps.assert_same(two, res, covar)


@pytest.mark.parametrize("N", [90, 260])
def test_a_dimension_the_time_model_does_not_see(eng, N):
    """One time draw with a length scale of 1e12 in one dimension (that dimension vanishes from its K_t) and a noise of
    1e-3 amp2_t."""
    comp, cand, vals, hypers, ld, th = ps.problem(N, 700, 3, 3, 2600 + N)
    th = th.copy()
    th[1, 3 + 1] = fh.FAR_LS
    th[:, 1] = 1e-3 * th[:, 2]
    check_shape(eng, N, 700, 3, 3, None, prob=(comp, cand, vals, hypers, ld, th))


# ---- 4. the division's edges ------------------------------------------------------------------------------------------------
EDGE_BASES = {"fused": (90, 700, 3, 3, 2701), "general": (150, 700, 3, 3, 2702)}


def edge_problem(name, mean_t, far_rows=(), high_mean=False, M=None):
    """The base with log durations around mean_t and draw 1's mean at mean_t: that draw predicts exp(mean_t + O(1)) everywhere.
    The other draws get length scales of 0.02, so that they predict exp(their own mean) away from the observations and
    follow the data near them.  far_rows: candidates moved past every clamp of both models (their K* is +0.0);
    high_mean: the objective's means far above the best value, so that EI there is exactly 0."""
    N, M0, D, H, seed = EDGE_BASES[name]
    comp, cand, vals, hypers, ld, th = ps.problem(N, M or M0, D, H, seed)
    cand, hypers, th = cand.copy(), hypers.copy(), th.copy()
    th[1, 0] = mean_t
    th[[0, 2], 3:] = 0.02
    for r in far_rows:
        cand[r, 0] += 4096.0 * 1024.0
    if high_mean:
        hypers[:, 0] = vals.min() + 200.0
    return comp, cand, vals, hypers, mean_t + 0.3 * ld, th


def robust_mask(prob):
    """[M, H]: where the oracle's plain EI is either well above its underflow (>= 1e-280) or zero by a wide margin
    ((best - func_m) / func_s <= -45: both terms of u Phi(u) + phi(u) are exact zeros).  In between (u from -38.6 to -37.5) the
    two terms are denormal and their sum has no sign to speak of -- an MI355X gives -5e-324 and -0.0 where numpy has 1e-321;
    assert_ei_close's rule for small values is what holds EI there, and a test of the DIVISION stays out of it."""
    comp, cand, vals, hypers, ld, th = prob
    plain_o = ps.oracle_plain(prob)
    robust = np.empty(plain_o.shape, dtype=bool)
    for h in range(hypers.shape[0]):
        st = {}
        orc.compute_ei(comp, cand, vals, hypers[h], stages=st)
        with np.errstate(all="ignore"):
            robust[:, h] = (plain_o[:, h] >= 1e-280) | ((vals.min() - st["func_m"]) / np.sqrt(st["func_v"]) <= -45.0)
    return robust


def edge_run(eng, prob, chunks=False):
    with ph.options(eng, **({"kstar_budget_bytes": 8 * 256 * 128} if chunks else {})):
        ps.load(eng, prob)
        res = ps.step(eng)
        ps.load(eng, prob)
        plain = ps.step(eng, KEEP_MOMENTS)
    # the division itself: IEEE, on the two numbers the library reports
    with np.errstate(all="ignore"):
        assert np.array_equal(res["draws"], plain["draws"] / res["tmean"], equal_nan=True)
    assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1), equal_nan=True)
    return res, plain


@pytest.mark.parametrize("name", sorted(EDGE_BASES))
@pytest.mark.parametrize("chunks", [False, True])
def test_a_duration_that_overflows_gives_zero(eng, name, chunks):
    comp, cand, vals, hypers, ld, th = edge_problem(name, 800.0)
    keep = np.all(robust_mask((comp, cand, vals, hypers, ld, th)), axis=1)      # (candidates chosen by the oracle alone)
    assert np.mean(keep) >= 0.7 and np.all(keep[:10])
    prob = (comp, np.ascontiguousarray(cand[keep]), vals, hypers, ld, th)
    res, plain = edge_run(eng, prob, chunks)
    ei_o, tm_o = ps.oracle_of(prob)
    assert np.all(np.isposinf(tm_o[:, 1])) and np.all(ei_o[:, 1] == 0.0) and not np.any(np.signbit(ei_o[:, 1]))
    assert np.all(np.isposinf(res["tmean"][:, 1]))
    assert np.all(res["draws"][:, 1] == 0.0) and not np.any(np.signbit(res["draws"][:, 1]))
    assert_ei_close(res["draws"], ei_o)
    assert np.array_equal(np.isinf(res["tmean"]), np.isinf(tm_o))
    assert res["best"][0] == orc.choose(ei_o)
    # the other draws: untouched, bit for bit, by what draw 1 predicts
    comp, cand, vals, hypers, ld, th = prob
    th2 = th.copy()
    th2[1, 0] = 0.25
    other, _ = edge_run(eng, (comp, cand, vals, hypers, ld, th2), chunks)
    for h in (0, 2):
        assert np.array_equal(other["draws"][:, h], res["draws"][:, h]) and np.array_equal(other["tmean"][:, h], res["tmean"][:, h])


@pytest.mark.parametrize("name", sorted(EDGE_BASES))
@pytest.mark.parametrize("chunks", [False, True])
def test_a_duration_that_underflows_gives_inf(eng, name, chunks):
    comp, cand, vals, hypers, ld, th = edge_problem(name, -800.0, M=4000)
    plain_o = ps.oracle_plain((comp, cand, vals, hypers, ld, th))
    keep = np.min(plain_o, axis=1) >= 1e-200                  # candidates chosen by the oracle: EI well above 1e-280 in every draw
    assert np.sum(keep) >= 100
    prob = (comp, np.ascontiguousarray(cand[keep]), vals, hypers, ld, th)
    plain_o = plain_o[keep]
    assert np.mean(plain_o[:, 1] >= 1e-280) >= 0.5 and not np.any((plain_o[:, 1] > 0) & (plain_o[:, 1] < 1e-280))
    res, plain = edge_run(eng, prob, chunks)
    ei_o, tm_o = ps.oracle_of(prob)
    assert np.all(tm_o[:, 1] == 0.0) and np.all(res["tmean"][:, 1] == 0.0)
    assert np.all(np.isposinf(res["draws"][plain_o[:, 1] >= 1e-280, 1]))
    assert np.array_equal(np.isposinf(res["draws"]), np.isposinf(ei_o))
    assert np.all(np.isposinf(res["mean"])) and np.all(np.isposinf(np.mean(ei_o, axis=1)))
    assert res["best"] == (int(np.argmax(np.mean(ei_o, axis=1))), np.inf) and res["best"][0] == 0


@pytest.mark.parametrize("name", sorted(EDGE_BASES))
@pytest.mark.parametrize("chunks", [False, True])
def test_zero_ei_over_a_zero_duration_is_nan_and_the_first_one_wins(eng, name, chunks):
    rows = (5, 300)
    prob = edge_problem(name, -800.0, far_rows=rows, high_mean=True)
    res, plain = edge_run(eng, prob, chunks)
    ei_o, tm_o = ps.oracle_of(prob)
    plain_o = ps.oracle_plain(prob)
    for r in rows:
        assert np.all(plain_o[r] == 0.0) and tm_o[r, 1] == 0.0 and np.isnan(ei_o[r, 1])      # from the oracle alone
        assert np.all(plain["draws"][r] == 0.0) and res["tmean"][r, 1] == 0.0
        assert np.isnan(res["draws"][r, 1]) and np.isnan(res["mean"][r])
        assert np.array_equal(res["draws"][r, [0, 2]], [0.0, 0.0])        # 0 over the other draws' exp(mean_t)
    # everywhere else, where the oracle's EI is well above its underflow or zero by a wide margin: NaN exactly where numpy has it
    robust = robust_mask(prob)
    assert np.mean(robust) >= 0.8 and np.all(robust[list(rows)])
    assert np.array_equal(np.isnan(res["draws"])[robust], np.isnan(ei_o)[robust])
    assert res["best"][0] == int(np.argmax(np.mean(ei_o, axis=1))) == rows[0] and np.isnan(res["best"][1])


@pytest.mark.parametrize("kind", cv.KINDS)
def test_a_denormal_duration_stays_within_the_budget(eng, fixture, cov_fixture, kind):
    """Predictions from 1e-315 down through the last quanta (tests/persec_mp.py: the denormal case): the budget of 1(a),
    widened by one quantum 2^-1074 for the exponential's result; the quotient is IEEE's on those durations (edge_run's
    assertion), finite or inf as numpy's."""
    N, means = pm.DENORMAL_N, pm.DENORMAL_MEAN_T
    diag_load(eng, kind, N, means, True)
    res = ps.step(eng)
    diag_load(eng, kind, N, means, True)
    plain = ps.step(eng, KEEP_MOMENTS)
    T_ref = fixture["T_%s_denormal" % kind]
    allowed = pm.budget(cov_fixture, kind, N, T_ref, means, quanta=1, denormal=True)
    worst = float(np.max(np.abs(res["tmean"].astype(LD) - T_ref.astype(LD)) / allowed))
    print("T denormal %-9s: worst |T - T_ref| / budget = %.3f" % (kind, worst))
    assert worst <= 1.0 and np.all(res["tmean"] < 2.0 ** -1022)
    with np.errstate(all="ignore"):
        want = plain["draws"] / res["tmean"]
    assert np.array_equal(res["draws"], want, equal_nan=True)
    assert np.any(np.isposinf(want)) or np.any(np.isfinite(want))
    with ph.options(eng, ei_fused=0):
        diag_load(eng, kind, N, means, True)
        ps.assert_same(ps.step(eng), res, kind)


@pytest.mark.parametrize("name", sorted(EDGE_BASES))
@pytest.mark.parametrize("chunks", [False, True])
def test_non_finite_candidates_are_nan_and_leave_the_others(eng, name, chunks):
    """A NaN coordinate and a +inf one: that candidate's duration and EI are NaN in every draw and the first one wins; every
    other column is the clean run's, bit for bit.  (The oracle's triangular solve refuses non-finite input, so its values are
    taken at the finite candidates and the two rows set by the rule.)"""
    prob = ps.problem(*EDGE_BASES[name])
    comp, cand, vals, hypers, ld, th = prob
    ei_o, tm_o = ps.oracle(*EDGE_BASES[name])
    bad = cand.copy()
    rows = np.array([11, 470])
    bad[rows[0], 1] = np.nan
    bad[rows[1], 2] = np.inf
    ei_bad = ei_o.copy()
    ei_bad[rows] = np.nan
    opts = {"kstar_budget_bytes": 8 * 256 * 128} if chunks else {}
    with ph.options(eng, **opts):
        ps.load(eng, prob)
        clean = ps.step(eng)
        ps.load(eng, (comp, bad, vals, hypers, ld, th))
        res = ps.step(eng)
    assert np.all(np.isnan(res["tmean"][rows])) and np.all(np.isnan(res["draws"][rows])) and np.all(np.isnan(res["mean"][rows]))
    assert res["best"][0] == int(np.argmax(np.mean(ei_bad, axis=1))) == rows[0] and np.isnan(res["best"][1])
    ok = np.ones(len(cand), dtype=bool)
    ok[rows] = False
    for k in ("draws", "mean", "tmean", "func_m", "func_v"):
        assert np.array_equal(res[k][ok], clean[k][ok]), k
    assert_ei_close(res["draws"], ei_bad)


@pytest.mark.parametrize("name", sorted(EDGE_BASES))
def test_nan_in_log_durs_poisons_every_duration_and_a_clean_model_restores_the_handle(eng, name):
    """include/spx.h (spx_set_time_model): log_durs is not checked; a NaN propagates by IEEE rules -- alpha_t of every draw is
    NaN throughout, so every predicted duration and every value is NaN and the winner is index 0, numpy's first NaN.  (The
    reference cannot get there: scipy's check_finite raises.)"""
    prob = ps.problem(*EDGE_BASES[name])
    comp, cand, vals, hypers, ld, th = prob
    ps.load(eng, prob)
    clean = ps.step(eng)
    bad = ld.copy()
    bad[len(ld) // 2] = np.nan
    for entry in (ps.step, ps.factor_run):
        eng.set_time_model(bad, th)
        res = entry(eng)
        assert np.all(np.isnan(res["tmean"])) and np.all(np.isnan(res["draws"])) and np.all(np.isnan(res["mean"]))
        assert res["best"][0] == 0 and np.isnan(res["best"][1])
        assert np.array_equal(res["func_m"], clean["func_m"]) and np.array_equal(res["func_v"], clean["func_v"])
        eng.set_time_model(ld, th)
        ps.assert_same(entry(eng), clean, name)


# ---- 5. staleness through the handle ----------------------------------------------------------------------------------------
def _changed(prob, what):
    comp, cand, vals, hypers, ld, th = prob
    if what == "log_durs":
        return comp, cand, vals, hypers, ld[::-1] * 1.1 + 0.05, th
    if what == "time_hypers":
        th2 = th[::-1].copy()
        th2[:, 0] += 0.1
        return comp, cand, vals, hypers, ld, th2
    if what == "values":
        return comp, cand, vals[::-1] * 0.9 - 0.1, hypers, ld, th
    return prob                                                   # "reset": the time model cleared and set again


def _apply(eng, new, what):
    """Only the call that carries the change (what it drops is the library's business)."""
    comp, cand, vals, hypers, ld, th = new
    if what == "values":
        eng.set_observations(comp, vals)                          # new observations drop the hypers and the time model
        eng.set_hypers(hypers)
        eng.set_time_model(ld, th)
    else:
        if what == "reset":
            eng.set_time_model(None, None)
        eng.set_time_model(ld, th)


@pytest.mark.parametrize("what", ["log_durs", "time_hypers", "values", "reset"])
@pytest.mark.parametrize("name", ["fused", "general"])
@pytest.mark.parametrize("chunks", [False, True])
def test_a_change_between_two_passes_gives_a_fresh_handles_bits(eng, name, chunks, what):
    N, M, D, H, seed, fused = BASES[name]
    prob = ps.problem(N, M, D, H, seed)
    new = _changed(prob, what)
    want = ps.fresh_step(new)
    if what != "reset":
        assert not np.array_equal(want["draws"], ps.fresh_step(prob)["draws"])
    with ph.options(eng, **({"kstar_budget_bytes": budgets(name)[0]} if chunks else {})):
        # between two steps
        ps.load(eng, prob)
        ps.step(eng)
        _apply(eng, new, what)
        ps.assert_same(ps.step(eng), want, (name, what, "step"))
        # between the factorisation and the pass: the table of tests/test_gpu_t_held.py (per_sec; set_observations,
        # set_hypers, set_time_model and its clear form all leave neither a factor nor results) says the pass refuses
        ps.load(eng, prob)
        eng.factor()
        _apply(eng, new, what)
        with pytest.raises(ValueError, match="spx_factor"):
            eng.ei_run(KEEP)
        ps.assert_same(ps.factor_run(eng), want, (name, what, "factor + run"))


@pytest.mark.parametrize("name", sorted(BASES))
def test_a_time_only_pass_between_two_full_passes_changes_nothing(eng, name):
    prob, base = default_run(eng, name)
    small = budgets(name)[0]
    for kw in ({}, dict(kstar_budget_bytes=small), dict(kstar_budget_bytes=small, streams=2)):
        with ph.options(eng, **kw):
            ps.assert_same(ps.step(eng), base, (name, "first"))
            eng.ei_run(KEEP | TIME_ONLY)
            ps.assert_same(ps.collect(eng, KEEP | TIME_ONLY), base, (name, "time only"))
            with pytest.raises(ValueError):
                eng.ei_mean()
            eng.ei_run(KEEP)
            ps.assert_same(ps.collect(eng), base, (name, "second"))
        rescramble(eng, prob)
