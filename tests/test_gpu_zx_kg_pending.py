"""Knowledge gradient over the fantasies of pending jobs (include/spx.h: option "kg_fantasies"; csrc/kg_fant_kernels.hip): every
(draw, candidate) against np.mean over s of tests/kg_oracle.py on the DEVICE'S OWN lines, in the mean over s of the oracle's
unit, at the plain pass's bar -- 4 x the oracle's pinned error of the band of max over s of max |z_k| -- plus (ceil(log2 S) + 1)
2^-53 x the mean for the pairwise mean's roundings; plain KG per fantasy; paths bit for bit; state, refusals, choosers."""
import importlib
import math
import os

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine as spx
from tests import kg_helpers as kh
from tests import kg_mp as km
from tests import kg_oracle as ko
from tests import fantasy_helpers as fh
from tests import pending_helpers as ph
from tests.factor_helpers import chol_longdouble
from tests.helpers import branin
from tests.mes_helpers import same_state
from tests.test_gpu_zv_kg import fx  # noqa: F401  (the fixture: tests/golden/kg_mp.npz)

pytestmark = pytest.mark.gpu
KEEP = spx.FLAG_KEEP_MOMENTS


@pytest.fixture()
def eng():
    e = spx.Engine(0)
    yield e
    e.set_acquisition("EI")
    e.close()


def points_for(p, cand, A, seed):
    pts = np.random.RandomState(seed).rand(A, p.D)
    pts[min(1, A - 1)] = cand[min(3, cand.shape[0] - 1)]      # a point on a candidate
    pts[min(4, A - 1)] = pts[0]                               # a duplicate: two lines of equal slope and intercept
    return pts


def run(e, p, cand, pts, flags=KEEP, entry="factor", draw=False, on=1):
    e.set_option("kg_fantasies", on)
    ph.load(e, p, cand)
    e.set_kg_points(pts)
    e.set_acquisition("KG")
    e.ei_step(0) if entry == "step" else e.factor()
    if draw:
        e.draw_fantasies(p.randn, p.pend.shape[0])
    else:
        e.set_fantasies(p.fant, p.bests)
    e.ei_run(flags)
    assert e.stat("last_kg_fantasies") == p.S and e.stat("last_kg_points") == pts.shape[0]
    out = {"draws": e.ei_draws(), "mean": e.ei_mean(), "best": e.best()}
    out["mu_a"] = np.array([[e.kg_fantasy_lines(d, s, False)[1] for s in range(p.S)] for d in range(p.H)])
    if flags & KEEP:
        out["mu_c"] = np.array([[e.kg_fantasy_lines(d, s)[0] for s in range(p.S)] for d in range(p.H)])
        out["cov"] = [e.kg_lines(d)[1] for d in range(p.H)]
        out["v"] = [e.kg_fantasy_var(d) for d in range(p.H)]
    return out


def assert_same(o, base, what):
    assert np.array_equal(o["draws"], base["draws"], equal_nan=True) and np.array_equal(o["mean"], base["mean"], equal_nan=True), what
    assert o["best"][0] == base["best"][0] and np.array_equal(o["mu_a"], base["mu_a"]), what
    for k in ("mu_c", "v", "cov"):
        if k in o:
            assert np.array_equal(np.array(o[k]), np.array(base[k]), equal_nan=True), (what, k)


def hold_values(fx, out, p, what):
    worst = dict((band, 0.0) for band in km.BANDS)
    M = out["draws"].shape[0]
    for d in range(p.H):
        per_s = [ko.lines(out["mu_c"][d, s], out["v"][d], p.rows[d, 1], out["mu_a"][d, s], out["cov"][d]) for s in range(p.S)]
        got = out["draws"][:, d]
        for c in range(M):
            sets = [(mu[c], b[c]) for mu, b in per_s]
            if not all(np.all(np.isfinite(mu)) and np.all(np.isfinite(b)) for mu, b in sets):
                assert np.isnan(got[c]), (what, d, c)
                continue
            want = float(np.mean([ko.value(mu, b) for mu, b in sets]))
            u = float(np.mean([ko.unit(mu, b) for mu, b in sets]))
            assert got[c] >= 0.0 and not np.signbit(got[c]), (what, d, c, got[c])
            if u == 0.0:
                assert got[c] == 0.0 and want == 0.0, (what, d, c, got[c], want)
                continue
            band = km.band_of(max(ko.zmax(mu, b) for mu, b in sets))
            slack = (math.ceil(math.log2(p.S)) + 1) * 2.0 ** -53 * want / u       # the mean's roundings, in units
            worst[band] = max(worst[band], (abs(got[c] - want) / u - slack) / (kh.MARGIN * km.pinned(fx, band)))
    for band in km.BANDS:
        print("%s, %s: worst error %.3g of its bar" % (what, band, worst[band]))
        assert worst[band] <= 1.0, (what, band, worst[band])
    m = np.mean(out["draws"], axis=1)
    assert np.array_equal(out["mean"], m, equal_nan=True) and out["best"][0] == int(np.argmax(m))


# ---- 1. values.  One row per hazard; N = resident rows.  A = 1 .. 255: n = 2 .. 256, the tile sizes and a uint8 rank at its limit;
#         S: below / at / above a fantasy block, a wave, the mean's eight accumulators; rows 63 + 1, 64 + 3, 126 + 3 across a
#         factor tile; 1030 rows with S = 6: k_kgf_mu's long-column form and its clamped last group of four; every covar.
#         M H S n stays small: the oracle is a Python loop per line set.
SHAPES = [  # A, S, M, N, n_pend, H, D, covar, draw
    (1, 1, 1, 64, 1, 1, 1, "Matern52", False),
    (2, 2, 255, 67, 3, 3, 3, "Matern32", False),
    (63, 7, 257, 129, 3, 1, 3, "ARDSE", False),
    (64, 8, 255, 64, 1, 1, 9, "SE", True),
    (65, 9, 1, 67, 3, 3, 3, "Matern52", False),
    (255, 64, 19, 129, 3, 1, 3, "Matern52", False),
    (3, 6, 33, 1030, 3, 1, 3, "Matern52", False),
    (17, 65, 33, 67, 3, 1, 3, "Matern32", False),
    (5, 100, 257, 64, 1, 1, 3, "Matern52", False),
]


@pytest.mark.parametrize("A,S,M,N,n_pend,H,D,covar,draw", SHAPES)
def test_values_against_the_oracle_on_the_device_s_lines(eng, fx, A, S, M, N, n_pend, H, D, covar, draw):
    p = ph.problem(14000 + A + S, covar, N=N, D=D, H=H, S=S, n_pend=n_pend)
    cand = ph.candidates(p, 3, M)
    if M > 100:
        cand[57, 0] = np.nan                                  # a non-finite mu_c[s]: NaN for that (d, c) alone
    try:
        out = run(eng, p, cand, points_for(p, cand, A, A), draw=draw)
    finally:
        eng.set_covar("Matern52")
    hold_values(fx, out, p, "A=%d S=%d M=%d N=%d H=%d %s" % (A, S, M, N, H, covar))
    assert not np.any(np.isnan(out["draws"][np.arange(M) != 57])) and (M < 100 or np.all(np.isnan(out["draws"][57])))


# ---- 2. it is plain KG per fantasy ---------------------------------------------------------------------------------------------------
def mu_a_yardstick(K, Ka, y, mean):
    """(mu_a in long double, its unit, the bar) as tests/test_gpu_zv_kg.py holds the lines: from the device's own K and K(X, A);
    the bar is 4 x the larger error of two float64 routes (LAPACK's solves; W = L^-1 and products), floor 16 x 2^-52."""
    import scipy.linalg as spla
    from scipy.linalg import lapack
    LD = np.longdouble
    L, gamma, _, _ = chol_longdouble(K, y - mean)
    G = np.zeros(Ka.shape, dtype=LD)
    for i in range(K.shape[0]):
        G[i] = (Ka[i].astype(LD) - np.dot(L[i, :i], G[:i])) / L[i, i]
    ref, unit = np.dot(G.T, gamma) + LD(mean), np.dot(np.abs(G).T, np.abs(gamma)) + abs(LD(mean))
    Lf = lapack.dpotrf(K, lower=1, clean=1)[0]
    W = np.tril(lapack.dtrtri(Lf, lower=1)[0])
    routes = (np.dot(Ka.T, spla.cho_solve((Lf, True), y - mean)) + mean, np.dot(np.dot(W, Ka).T, np.dot(W, y - mean)) + mean)
    return ref, unit, max(4 * max(float(np.max(np.abs(r.astype(LD) - ref) / unit)) for r in routes), 16 * 2.0 ** -52)


@pytest.mark.parametrize("S,cols,N", [(1, (0,), 67), (9, (0, 4, 8), 67), (6, (5,), 1030)])     # (1030 rows: k_kgf_mu's long-column form)
def test_it_is_plain_kg_per_fantasy(eng, fx, S, cols, N):
    """A second handle given (X, fant[d][:, s]): its plain pass gives KG_ds within two bars (both sides carry one), cov and func_v
    bit for bit (stricter than the long-double bar: they do not depend on y), and both handles' mu_a sit within the long-double bar."""
    p = ph.problem(14100 + S, N=N, D=3, H=2, S=S, n_pend=3)
    cand = ph.candidates(p, 4, 130)
    pts = points_for(p, cand, 9, 2)
    full, e2 = run(eng, p, cand, pts), spx.Engine(0)
    try:
        for s in cols:
            one = full if S == 1 else run(eng, ph.with_columns(p, s, s + 1), cand, pts)
            assert np.array_equal(one["mu_a"][:, 0], full["mu_a"][:, s]) and np.array_equal(one["mu_c"][:, 0], full["mu_c"][:, s])
            for d in range(p.H):
                e2.set_observations(p.X, np.ascontiguousarray(p.fant[d][:, s])); e2.set_candidates(cand); e2.set_hypers(p.rows[d:d + 1])
                e2.set_kg_points(pts); e2.set_acquisition("KG")
                e2.ei_step(KEEP)
                plain, (mu_a, cov), (fm, fv) = e2.ei_draws()[:, 0], e2.kg_lines(0), e2.get_moments(0)
                assert np.array_equal(cov, full["cov"][d]) and np.array_equal(fv, full["v"][d]), (s, d)
                mu, b = ko.lines(fm, fv, p.rows[d, 1], mu_a, cov)
                for c in range(cand.shape[0]):
                    u, band = ko.unit(mu[c], b[c]), km.band_of(ko.zmax(mu[c], b[c]))
                    e = km.error(one["draws"][c:c + 1, d], plain[c:c + 1], np.array([u]))
                    assert e <= 2 * kh.MARGIN * km.pinned(fx, band), (s, d, c, one["draws"][c, d], plain[c])
                K = e2.get_factor(0, want_L=False, want_alpha=False)[0]
                e2.set_candidates(pts)
                ref, unit, bar = mu_a_yardstick(K, e2.get_cross_cov(0), p.fant[d][:, s], p.rows[d, 0])
                errs = [float(np.max(np.abs(m.astype(np.longdouble) - ref) / unit)) for m in (full["mu_a"][d, s], mu_a)]
                print("s=%d d=%d: mu_a error over fantasies %.3g, plain %.3g (bar %.3g)" % (s, d, errs[0], errs[1], bar))
                assert max(errs) <= bar, (s, d, errs, bar)
    finally:
        e2.close()


# ---- 3. paths, bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [101, 257, 300])
def test_paths_do_not_change_bits(eng, N):
    p = ph.problem(14200 + N, N=N, D=3, H=3, S=9, n_pend=3)
    cand, Np = ph.candidates(p, 7, 1000), (N + 127) // 128 * 128
    pts = points_for(p, cand, 17, N)
    base = run(eng, p, cand, pts)
    for kw in (dict(kstar_budget_bytes=8 * Np * 256), dict(kstar_budget_bytes=8 * Np * 1024), dict(streams=2),
               dict(streams=3, kstar_budget_bytes=8 * Np * 256), dict(gemm_partial=0)):
        ph.scramble(eng, p, cand)
        with ph.options(eng, **kw):
            assert_same(run(eng, p, cand, pts), base, kw)
    assert_same(run(eng, p, cand, pts, entry="step"), base, "step")
    assert_same(run(eng, p, cand, pts, flags=0), base, "without the moments")
    for d in range(p.H):                                      # a draw alone against the same draw among three
        q = ph.with_columns(p, 0, p.S)
        q.rows, q.fant, q.bests, q.H = p.rows[d:d + 1], p.fant[d:d + 1], p.bests[d:d + 1], 1
        one = run(eng, q, cand, pts)
        assert np.array_equal(one["draws"][:, 0], base["draws"][:, d], equal_nan=True) and np.array_equal(one["mu_a"][0], base["mu_a"][d])
    if N == 101:   # spx_draw_fantasies against spx_set_fantasies given the fantasies it formed: what does not depend on Gamma_s bit
        # for bit; the two form Gamma_s by different routes (factored rows / W (F - mean)), so the intercepts at the project's bar
        # for those routes (tests/test_gpu_n_pending_paths.FANT_RTOL = 1e-6 of the largest)
        drawn = run(eng, p, cand, pts, draw=True)
        q = ph.with_columns(p, 0, p.S)
        q.fant, q.bests = fh.as_fant(p, fh.device_fantasies(eng, p.H)[0]), fh.device_fantasies(eng, p.H)[1]
        fed = run(eng, q, cand, pts)
        assert np.array_equal(np.array(fed["cov"]), np.array(drawn["cov"])) and np.array_equal(np.array(fed["v"]), np.array(drawn["v"]))
        for k in ("mu_a", "mu_c"):
            print("%s: set against draw, largest difference %.3g of the largest" % (k, np.max(np.abs(fed[k] - drawn[k])) / np.max(np.abs(drawn[k]))))
            assert np.max(np.abs(fed[k] - drawn[k])) <= 1e-6 * np.max(np.abs(drawn[k])), k


# ---- 4. state and refusals ----------------------------------------------------------------------------------------------------------------
def test_state_refusals_and_statistics(eng):
    p = ph.problem(14300, N=67, D=2, H=2, S=3, n_pend=3)
    cand, pts = ph.candidates(p, 8, 130), np.random.RandomState(1).rand(5, 2)
    with pytest.raises(ValueError, match="SPX_ACQ_KG is not defined over fantasies"):
        run(eng, p, cand, pts, on=0)
    base = run(eng, p, cand, pts)
    with pytest.raises(ValueError, match="spx_get_kg_fantasy_lines"):          # mu_a != NULL: refused, naming the new getter
        eng._check(eng._lib.spx_get_kg_lines(eng._h, 0, spx._dp(np.empty(5)), None))
    with pytest.raises(ValueError, match="fantasy out of range"):
        eng.kg_fantasy_lines(0, p.S)
    q = ph.with_columns(p, 0, p.S)                            # one NaN in one fantasy of draw 0: its mu_a[s] are NaN, and so is the draw
    q.fant = p.fant.copy()
    q.fant[0, 5, 1] = np.nan
    bad = run(eng, q, cand, pts)
    assert np.all(np.isnan(bad["mu_a"][0, 1])) and np.all(np.isnan(bad["draws"][:, 0])) and np.array_equal(bad["draws"][:, 1], base["draws"][:, 1])
    assert np.array_equal(run(eng, p, cand, pts)["draws"], base["draws"])
    for call in (lambda: eng.ei_run(spx.FLAG_PER_SEC), lambda: eng.ei_run(spx.FLAG_CONSTRAINED), lambda: eng.ei_grad_batch(np.zeros((1, 2))),
                 lambda: eng.ei_run(spx.FLAG_TIME_ONLY | spx.FLAG_PER_SEC | KEEP),
                 lambda: eng.ei_grad(np.zeros(2)), lambda: eng.constrained_ei_grad_batch(np.zeros((1, 2)), 0.0)):
        with pytest.raises(ValueError):
            call()
        assert eng.stat("last_kg_fantasies") == p.S and np.array_equal(eng.ei_draws(), base["draws"])
    eng.ei_run(0)                                             # without the moments: mu_a is served, mu_c is not
    assert eng.kg_fantasy_lines(0, 0, False)[1].shape == (5,)
    with pytest.raises(ValueError, match="KEEP_MOMENTS"):
        eng.kg_fantasy_lines(0, 0)
    # the results go with the fantasies, with the points and with the option
    for drop in (lambda: eng.set_fantasies(p.fant, p.bests), lambda: eng.set_kg_points(pts), lambda: eng.set_option("kg_fantasies", 1)):
        eng.ei_run(0)
        assert eng.stat("last_kg_fantasies") == p.S
        drop()
        assert eng.stat("last_kg_fantasies") == 0
        with pytest.raises(ValueError):
            eng.kg_fantasy_var(0)
    # S + A > 4096, and H S Mp 8 bytes of intercepts above the budget asserted from the message: both from the host's record
    eng.set_fantasies(np.zeros((p.H, 67, 4092)), np.zeros((p.H, 4092)))
    with pytest.raises(ValueError, match=r"S \+ A = 4092 \+ 5"):
        eng.ei_run(0)
    big = np.random.RandomState(1).rand(1100000, 2)
    eng.set_candidates(big)
    eng.set_fantasies(np.zeros((p.H, 67, 256)), np.zeros((p.H, 256)))
    with pytest.raises(ValueError) as ei:
        eng.ei_run(0)
    Mp = (big.shape[0] + 127) // 128 * 128
    assert "%d x %d x %d x 8 = %d bytes of means" % (p.H, 256, Mp, p.H * 256 * Mp * 8) in str(ei.value) and p.H * 256 * Mp * 8 > 4 << 30
    eng.set_fantasies(np.zeros((p.H, 67, 130)), np.zeros((p.H, 130)))         # fits once, not beside a second table of KG_ds
    with pytest.raises(ValueError, match="twice with SPX_FLAG_KEEP_MOMENTS"):
        eng.ei_run(KEEP)
    eng.set_kg_points(np.random.RandomState(2).rand(255, 2))                  # H (A + 1) Mp 9 bytes of ordered slopes
    eng.set_fantasies(p.fant, p.bests)
    with pytest.raises(ValueError, match="%d x 256 x %d x 9 = %d bytes of ordered slopes" % (p.H, Mp, p.H * 256 * Mp * 9)):
        eng.ei_run(0)
    assert min(p.H * 256 * Mp * 9, 2 * p.H * 130 * Mp * 8) > 4 << 30 > p.H * 130 * Mp * 8


@pytest.mark.parametrize("modname,arg", [("GPEIChooser", "mcmc_iters=4"),
                                         ("GPEIOptChooser", "mcmc_iters=3,burnin=5,grid_subset=4,use_multiprocessing=0")])
def test_choosers_score_a_pending_call_with_kg(golden_dir, tmp_path, modname, arg):
    mod = importlib.import_module("spearmint_amd.chooser." + modname)
    with pytest.raises(ValueError, match="kg_pending"):
        mod.init(str(tmp_path), arg + ",acq=EI,kg_pending=1")
    grid = np.array(np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:400], copy=True)
    values = np.full(grid.shape[0], np.nan)
    values[:6] = branin(grid[:6, 0], grid[:6, 1])
    free, pend, done = np.arange(7, grid.shape[0]), np.array([6]), np.arange(6)
    out = {}
    for name, extra in (("kg1", ",acq=KG,acq_par=12,kg_pending=1"), ("ei", ",acq=EI")):
        (tmp_path / name).mkdir()
        ch = mod.init(str(tmp_path / name), arg + extra)
        ch._eng = spx.Engine(0)
        try:
            npr.seed(77)
            job = ch.next(grid, values, np.full(grid.shape[0], np.nan), free, pend, done)
            out[name] = (job, npr.get_state(), ch.last_acq_used, ch.last_kg)
        finally:
            ch._eng.close()
    assert out["kg1"][2] == "KG" and out["ei"][2] == "EI"
    assert out["kg1"][3]["value"] >= 0.0 and out["kg1"][0] == int(free[out["kg1"][3]["grid_index"]]) and len(out["kg1"][3]["points_index"]) == 12
    assert same_state(out["kg1"][1], out["ei"][1])           # (kg_pending=0: tests/test_kg_host.py, the fall-back to EI)
