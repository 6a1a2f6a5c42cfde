"""The knowledge gradient (include/spx.h: SPX_ACQ_KG) on the device.

Values: k_kg_value against tests/kg_oracle.py on the DEVICE'S OWN lines (spx_get_kg_lines, spx_get_moments), every (draw,
candidate), and against the 50-digit yardstick (tests/kg_mp.py) on a fixed subset, at 4 x the oracle's pinned error per band
(tests/golden/kg_mp.npz): the same bar for both comparisons, the band of a set being that of max |z_k| over the oracle's own
envelope.
Lines: mu_a and C(c, a) against a long-double route from the device's own K, K(X, X*), K(X, A) and K(A, X*).
Paths: bit for bit across chunks, draw groups, streams, gemm_partial, step against factor + run, with and without the moments
kept, a draw alone against the same draw among three.  State, refusals, statistics; one next() of each chooser."""
import os

import numpy as np
import pytest

from spearmint_amd import engine as spx
from spearmint_amd.synthetic import synthetic_problem
from tests import kg_helpers as kh
from tests import kg_mp as km
from tests import kg_oracle as ko
from tests.factor_helpers import chol_longdouble

pytestmark = pytest.mark.gpu
KEEP = spx.FLAG_KEEP_MOMENTS
COVARS = ("Matern52", "Matern32", "ARDSE", "SE")
LD = np.longdouble


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "kg_mp.npz")))


@pytest.fixture(scope="module")
def eng():
    e = spx.Engine(0)
    yield e
    e.close()


def points_for(comp, cand, A, seed):
    """A representer points: random ones, with (where A allows) one on a candidate, one on an observation and a duplicate."""
    rs = np.random.RandomState(seed)
    pts = rs.rand(A, comp.shape[1])
    if A >= 2:
        pts[1] = cand[min(3, cand.shape[0] - 1)]
    if A >= 3:
        pts[2] = comp[0]
    if A >= 5:
        pts[4] = pts[0]
    return pts


def kg_pass(e, comp, cand, vals, rows, pts, covar="Matern52", flags=KEEP, entry="step", want_lines=True):
    e.set_covar(covar)
    e.set_observations(comp, vals)
    e.set_candidates(cand)
    e.set_hypers(rows)
    e.set_kg_points(pts)
    e.set_acquisition("KG")
    try:
        if entry == "step":
            e.ei_step(flags)
        else:
            e.factor()
            e.ei_run(flags)
        out = {"draws": e.ei_draws(), "mean": e.ei_mean(), "best": e.best(),
               "stats": tuple(e.stat(k) for k in ("last_kg_points", "kg_points", "last_kg_lines"))}
        if want_lines and (flags & KEEP):
            out["mom"] = [e.get_moments(d) for d in range(rows.shape[0])]
            out["lines"] = [e.kg_lines(d) for d in range(rows.shape[0])]
    finally:
        e.set_acquisition("EI")
        e.set_covar("Matern52")
    return out


def hold_values(fx, out, rows, what, n_mp=12):
    """Every (draw, candidate) against the oracle on the device's own lines; a fixed subset against the yardstick."""
    H = rows.shape[0]
    M = out["draws"].shape[0]
    worst = dict((band, 0.0) for band in km.BANDS)         # error / bar, per band
    mp_sets, mp_got = [], []
    for d in range(H):
        func_m, func_v = out["mom"][d]
        mu_a, cov = out["lines"][d]
        mu, b = ko.lines(func_m, func_v, rows[d, 1], mu_a, cov)
        got = out["draws"][:, d]
        for c in range(M):
            if not (np.all(np.isfinite(mu[c])) and np.all(np.isfinite(b[c]))):
                assert np.isnan(got[c]), (what, d, c)
                continue
            want, u = ko.value(mu[c], b[c]), ko.unit(mu[c], b[c])
            assert got[c] >= 0.0 and not np.signbit(got[c]), (what, d, c, got[c])
            if u == 0.0:
                assert got[c] == 0.0 and want == 0.0, (what, d, c, got[c], want)
            else:
                band = km.band_of(ko.zmax(mu[c], b[c]))
                worst[band] = max(worst[band], abs(got[c] - want) / u)
        for c in np.unique(np.linspace(0, M - 1, n_mp).astype(int)):
            mp_sets.append((mu[c], b[c]))
            mp_got.append(got[c])
    for band in km.BANDS:
        bar = kh.MARGIN * km.pinned(fx, band)
        print("%s: device against the oracle on its own lines, %s: worst %.3g units (bar %.3g)" % (what, band, worst[band], bar))
        assert worst[band] <= bar, (what, band, worst[band], bar)
    kh.held_to_yardstick(fx, np.array(mp_got), mp_sets, what + ", device")
    m = np.mean(out["draws"], axis=1)
    assert np.array_equal(out["mean"], m, equal_nan=True)
    assert out["best"][0] == int(np.argmax(m))


# one case per A; M, N, H, D and the covariance walk their lists beside it
SHAPES = [  # A, M, N, H, D, covar
    (1, 1, 2, 1, 1, "Matern52"),
    (2, 255, 64, 3, 3, "Matern32"),
    (15, 256, 65, 1, 9, "ARDSE"),
    (16, 257, 129, 3, 1, "SE"),
    (17, 1000, 300, 1, 3, "Matern52"),
    (63, 255, 129, 3, 9, "Matern32"),
    (64, 257, 64, 3, 3, "Matern52"),
    (65, 256, 65, 1, 3, "ARDSE"),
    (255, 257, 300, 3, 9, "Matern52"),
]


@pytest.mark.parametrize("A,M,N,H,D,covar", SHAPES)
def test_values_against_oracle_and_yardstick(eng, fx, A, M, N, H, D, covar):
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, 9000 + A, near=min(10, M))
    pts = points_for(comp, cand, A, A)
    out = kg_pass(eng, comp, cand, vals, rows, pts, covar)
    hold_values(fx, out, rows, "A=%d M=%d N=%d H=%d D=%d %s" % (A, M, N, H, D, covar), n_mp=6 if A > 100 else 12)
    assert out["stats"] == (A, A, 1)


def test_edge_inputs(eng, fx):
    """Noiseless draws; a candidate on a representer point; points on observations; a duplicated point; one NaN candidate."""
    N, M, H, D, A = 70, 200, 3, 3, 9
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, 31)
    rows[1, 1] = 0.0                                       # a noiseless draw
    pts = points_for(comp, cand, A, 5)
    pts[6], pts[7] = comp[1], comp[2]
    cand[20] = comp[3]                                     # func_v at the jitter level
    out = kg_pass(eng, comp, cand, vals, rows, pts)
    hold_values(fx, out, rows, "edge inputs")
    for d in range(H):                                     # a coincident pair: the covariance kernel's own r2 = 0 value
        mu_a, cov = out["lines"][d]
        func_m, func_v = out["mom"][d]
        # point 1 IS candidate 3: q(c, a) is the sum of beta^2, so C(c, a) is func_v(c) less the jitter 1e-6 amp2 that only
        # the prior variance carries, and mu_a is func_m(c) (a sanity check: test_lines_against_long_double holds both)
        assert abs((func_v[3] - cov[1, 3]) / rows[d, 2] - 1e-6) < 1e-9
        assert abs(mu_a[1] - func_m[3]) <= 1e-6 * (1.0 + abs(func_m[3]))
        assert np.array_equal(cov[4], cov[0]) and mu_a[4] == mu_a[0]    # a duplicated point: the same line, bit for bit
    # the duplicate changes nothing: the pass without it gives the same bits
    keep = [a for a in range(A) if a != 4]
    out2 = kg_pass(eng, comp, cand, vals, rows, pts[keep])
    assert np.array_equal(out2["draws"], out["draws"])
    # one NaN candidate: that column alone is NaN, and the argmax goes to it by numpy's rule
    cand2 = cand.copy()
    cand2[57, 1] = np.nan
    out3 = kg_pass(eng, comp, cand2, vals, rows, pts)
    assert np.all(np.isnan(out3["draws"][57])) and out3["best"][0] == 57 and np.isnan(out3["best"][1])
    ok = np.arange(M) != 57
    assert np.array_equal(out3["draws"][ok], out["draws"][ok])


def test_a_point_and_a_candidate_far_from_everything(eng):
    """One representer point past every correlation's underflow: every covariance with it is exactly zero and mu_a is the prior
    mean.  A candidate out there too has func_m = the prior mean and func_v = the prior variance: two lines through one
    intercept, slopes b_0 = func_v / s_c and 0, the breakpoint at z = 0, and the value b_0 f(0) = b_0 / sqrt(2 pi)."""
    comp, cand, vals, rows = synthetic_problem(40, 130, 2, 2, 77)
    cand[5] = 1e3
    out = kg_pass(eng, comp, cand, vals, rows, np.full((1, 2), -1e3))
    for d in range(2):
        mu_a, cov = out["lines"][d]
        func_m, func_v = out["mom"][d]
        assert np.all(cov == 0.0) and mu_a[0] == rows[d, 0] and func_m[5] == rows[d, 0]
        want = func_v[5] / np.sqrt(func_v[5] + rows[d, 1]) / ko.SQRT_2PI
        assert abs(out["draws"][5, d] - want) <= 4 * 2.0 ** -52 * want
    assert np.all(out["draws"] >= 0.0) and not np.any(np.signbit(out["draws"]))


def test_lines_against_long_double(eng):
    """mu_a and C(c, a) from the device against long double on the device's own K, K(X, X*), K(X, A) and K(A, X*); the bar is
    4 x the larger error of two float64 routes (LAPACK's solves; W = L^-1 by dtrtri and products), floor 16 x 2^-52, in units
    of sum_i |Gamma_a[i] gamma[i]| + |mean| resp. sum_i |beta_c[i] Gamma_a[i]| + |amp2 k(c, a)|."""
    import scipy.linalg as spla
    from scipy.linalg import lapack
    N, M, H, D, A = 129, 300, 2, 4, 17
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, 8123)
    pts = points_for(comp, cand, A, 3)[[0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]]      # (no duplicate: K(A, A) is factored below)
    A = pts.shape[0]
    out = kg_pass(eng, comp, cand, vals, rows, pts)
    e2 = spx.Engine(0)
    try:
        ratios = []
        for d in range(H):
            # the device's own matrices: K and K(X, X*) of the pass's handle, K(X, A) with the points as its candidates,
            # K(A, X*) from a handle whose rows are the points (the launch the pass itself makes)
            eng.set_observations(comp, vals); eng.set_candidates(cand); eng.set_hypers(rows); eng.factor()
            K = eng.get_factor(d, want_L=False, want_alpha=False)[0]
            Kc = eng.get_cross_cov(d)
            eng.set_candidates(pts)
            Ka = eng.get_cross_cov(d)
            e2.set_observations(pts, np.zeros(A)); e2.set_candidates(cand); e2.set_hypers(rows); e2.factor()
            Kac = e2.get_cross_cov(d)
            mean = rows[d, 0]
            y = vals - mean
            L, gamma, _, _ = chol_longdouble(K, y)

            def fwd(Ks):
                B = np.zeros((N, Ks.shape[1]), dtype=LD)
                for i in range(N):
                    B[i] = (Ks[i].astype(LD) - np.dot(L[i, :i], B[:i])) / L[i, i]
                return B
            B, G = fwd(Kc), fwd(Ka)
            mu_ld = np.dot(G.T, gamma) + LD(mean)
            C_ld = Kac.astype(LD) - np.dot(G.T, B)
            u_mu = np.dot(np.abs(G).T, np.abs(gamma)) + abs(LD(mean))
            u_C = np.dot(np.abs(G).T, np.abs(B)) + np.abs(Kac).astype(LD)
            # the two float64 routes
            Lf = lapack.dpotrf(K, lower=1, clean=1)[0]
            alpha = spla.cho_solve((Lf, True), y)
            r1_mu = np.dot(Ka.T, alpha) + mean
            r1_C = Kac - np.dot(Ka.T, spla.cho_solve((Lf, True), Kc))
            W = np.tril(lapack.dtrtri(Lf, lower=1)[0])
            Gf, Bf, gf = np.dot(W, Ka), np.dot(W, Kc), np.dot(W, y)
            r2_mu = np.dot(Gf.T, gf) + mean
            r2_C = Kac - np.dot(Gf.T, Bf)

            def err(got, ref, unit):
                return float(np.max(np.abs(np.asarray(got).astype(LD) - ref) / unit))
            mu_a, cov = out["lines"][d]
            bar_mu = max(4 * max(err(r1_mu, mu_ld, u_mu), err(r2_mu, mu_ld, u_mu)), 16 * 2.0 ** -52)
            bar_C = max(4 * max(err(r1_C, C_ld, u_C), err(r2_C, C_ld, u_C)), 16 * 2.0 ** -52)
            e_mu, e_C = err(mu_a, mu_ld, u_mu), err(cov, C_ld, u_C)
            ratios.append((e_mu / bar_mu, e_C / bar_C))
            print("draw %d: mu_a error %.3g (bar %.3g), C error %.3g (bar %.3g)" % (d, e_mu, bar_mu, e_C, bar_C))
            assert e_mu <= bar_mu and e_C <= bar_C
        print("lines against long double: worst error / bar  mu_a %.3g  C %.3g" % (max(r[0] for r in ratios), max(r[1] for r in ratios)))
    finally:
        e2.close()


@pytest.mark.parametrize("N", [101, 257, 300])
def test_bit_for_bit_across_paths(eng, N):
    M, H, D, A = 1000, 3, 3, 17
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, 600 + N)
    pts = points_for(comp, cand, A, N)
    Np = (N + 127) // 128 * 128
    base = kg_pass(eng, comp, cand, vals, rows, pts)

    def same(o, what, lines=True):
        assert np.array_equal(o["draws"], base["draws"], equal_nan=True), what
        assert np.array_equal(o["mean"], base["mean"], equal_nan=True) and o["best"] == base["best"], what
        if lines and "lines" in o:
            for d in range(H):
                assert np.array_equal(o["lines"][d][0], base["lines"][d][0]) and np.array_equal(o["lines"][d][1], base["lines"][d][1]), what
                assert np.array_equal(o["mom"][d][0], base["mom"][d][0]) and np.array_equal(o["mom"][d][1], base["mom"][d][1]), what
    variants = [("four chunks, one draw per group", {"kstar_budget_bytes": 8 * Np * 256}),
                ("one draw per group", {"kstar_budget_bytes": 8 * Np * 1024}),
                ("streams 2", {"streams": 2}), ("streams 3", {"streams": 3, "kstar_budget_bytes": 8 * Np * 256}),
                ("gemm_partial 0", {"gemm_partial": 0})]
    defaults = {"kstar_budget_bytes": 0, "streams": 1, "gemm_partial": -1}
    for what, opts in variants:
        try:
            for k, v in opts.items():
                eng.set_option(k, v)
            same(kg_pass(eng, comp, cand, vals, rows, pts), what)
            if "chunks" in what:
                assert eng.stat("last_step_fused") == 0
        finally:
            for k in opts:
                eng.set_option(k, defaults[k])
    same(kg_pass(eng, comp, cand, vals, rows, pts, entry="factor"), "factor + run")
    same(kg_pass(eng, comp, cand, vals, rows, pts, flags=0), "without the moments")
    for d in range(H):                                     # a draw alone against the same draw among three
        one = kg_pass(eng, comp, cand, vals, rows[d:d + 1], pts)
        assert np.array_equal(one["draws"][:, 0], base["draws"][:, d]), d
        assert np.array_equal(one["lines"][0][1], base["lines"][d][1]) and np.array_equal(one["lines"][0][0], base["lines"][d][0])
    # the position of a candidate and M: a slice of the candidates gives the same bits
    part = kg_pass(eng, comp, cand[300:557], vals, rows, pts)
    assert np.array_equal(part["draws"], base["draws"][300:557])


def test_state_refusals_and_statistics(eng):
    N, M, H, D, A = 70, 130, 2, 2, 5
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, 11)
    pts = points_for(comp, cand, A, 1)
    eng.set_observations(comp, vals); eng.set_candidates(cand); eng.set_hypers(rows)
    eng.set_kg_points(None)
    eng.ei_step(KEEP)
    ei = (eng.ei_draws(), eng.get_moments(1))
    out = kg_pass(eng, comp, cand, vals, rows, pts)
    # func_m / func_v are the EI pass's (column 0 of the S > 0 branch adds its two half-block partials in another association:
    # the last bits may differ)
    assert np.allclose(out["mom"][1][0], ei[1][0], rtol=0, atol=1e-11 * np.max(np.abs(ei[1][0])))
    assert np.allclose(out["mom"][1][1], ei[1][1], rtol=0, atol=1e-12 * rows[1, 2])
    eng.ei_step(KEEP)                                      # an EI pass behind a KG pass: the same bits as before it
    assert np.array_equal(eng.ei_draws(), ei[0]) and np.array_equal(eng.get_moments(1)[0], ei[1][0])
    assert eng.stat("last_kg_points") == 0 and eng.stat("kg_points") == A and np.array_equal(eng.get_kg_points(), pts)
    with pytest.raises(ValueError):
        eng.kg_lines(0)
    # setting the points drops the results only: the factor stays and the next run needs no factorisation
    eng.set_kg_points(pts[:3])
    with pytest.raises(ValueError):
        eng.ei_mean()
    eng.set_acquisition("KG")
    eng.ei_run(0)
    three = eng.ei_draws()
    assert eng.stat("last_kg_points") == 3 and eng.stat("last_kg_lines") == 0
    with pytest.raises(ValueError):
        eng.kg_lines(0)                                    # (the covariances were not kept; mu_a alone is served)
    assert eng.kg_lines(0, want_cov=False)[0].shape == (3,)
    # every refusal leaves the handle usable and the results held
    for call in (lambda: eng.ei_run(spx.FLAG_PER_SEC), lambda: eng.ei_run(spx.FLAG_CONSTRAINED), lambda: eng.ei_step(spx.FLAG_TIME_ONLY | KEEP | spx.FLAG_PER_SEC),
                 lambda: eng.ei_grad_batch(np.zeros((1, D))), lambda: eng.ei_grad(np.zeros(D)),
                 lambda: eng.constrained_ei_grad_batch(np.zeros((1, D)), 0.0),
                 lambda: eng.set_kg_points(np.full((2, D), np.nan)), lambda: eng.set_kg_points(np.zeros((256, D)))):
        with pytest.raises(ValueError):
            call()
        assert np.array_equal(eng.ei_draws(), three) and eng.stat("kg_points") == 3
    with pytest.raises(ValueError) as ei_:
        eng.ei_grad(np.zeros(D))
    assert "SPX_ACQ_KG" in str(ei_.value)
    # a 2-D partition set behind the acquisition: the pass refuses (spx_set_partition itself takes the results, nothing else);
    # without it the same factor serves the same bits
    eng.set_partition(2, 4 * M, 2 * H)
    for call in (eng.ei_run, eng.ei_step):
        with pytest.raises(ValueError) as ei_:
            call(0)
        assert "2-D partition" in str(ei_.value)
    eng.set_partition(1, 0, 0)
    eng.ei_run(0)
    assert np.array_equal(eng.ei_draws(), three)
    # ... and set in front of it: spx_set_acquisition refuses, the setting stays
    eng.set_acquisition("EI")
    eng.set_partition(2, 4 * M, 2 * H)
    with pytest.raises(ValueError) as ei_:
        eng.set_acquisition("KG")
    assert "2-D partition" in str(ei_.value) and eng.get_acquisition() == (spx.ACQ_EI, 0.0)
    eng.set_partition(1, 0, 0)
    eng.set_acquisition("KG")
    eng.ei_run(0)
    assert np.array_equal(eng.ei_draws(), three)
    # fantasies held: refused, and they stay
    rs = np.random.RandomState(2)
    eng.set_fantasies(rs.randn(H, N, 2), np.zeros((H, 2)))
    with pytest.raises(ValueError) as ei_:
        eng.ei_run(0)
    assert "fantasies" in str(ei_.value)
    eng.set_fantasies(None, None)
    eng.ei_run(0)
    assert np.array_equal(eng.ei_draws(), three)
    # without points: refused; observations of another D drop them
    eng.set_kg_points(None)
    for call in (eng.ei_run, eng.ei_step):
        with pytest.raises(ValueError) as ei_:
            call(0)
        assert "representer points" in str(ei_.value)
    eng.set_kg_points(pts)
    eng.set_option("timing", 1)
    try:
        eng.ei_step(0)
        t = eng.timings()
        assert t["kg"][1] >= 2 and t["kg"][0] > 0.0           # (k_kg_mu once, and the two kernels of the one work item)
    finally:
        eng.set_option("timing", 0)
    c3, d3, v3, r3 = synthetic_problem(20, 130, 3, 2, 4)
    eng.set_observations(c3, v3)
    assert eng.get_kg_points() is None and eng.stat("kg_points") == 0
    eng.set_acquisition("EI")


@pytest.mark.parametrize("name", ["GPEIChooser", "GPEIOptChooser"])
def test_chooser_next_against_the_oracle_engine(name, golden_dir, tmp_path):
    import importlib
    from tests.helpers import branin
    mod = importlib.import_module("spearmint_amd.chooser." + name)
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:400]
    arg = "mcmc_iters=3,acq=KG,acq_par=12" + (",burnin=3,grid_subset=3,use_multiprocessing=0" if name == "GPEIOptChooser" else "")
    values = np.full(grid.shape[0], np.nan)
    done = np.arange(8)
    values[done] = branin(grid[done, 0], grid[done, 1])
    cand = np.arange(8, grid.shape[0])
    res = []
    for k, make in enumerate((None, kh.make_oracle_engine())):
        d = tmp_path / str(k)
        d.mkdir()
        ch = mod.init(str(d), arg)
        if make:
            ch._eng = make()
        np.random.seed(123)
        job = ch.next(grid, values, np.full(grid.shape[0], np.nan), cand, np.zeros(0, dtype=int), done)
        res.append((job, ch.last_kg, ch.last_acq_used, np.array(ch.last_ei_mean)))
    (job, lk, used, mean), (ojob, olk, oused, omean) = res
    assert used == oused == "KG" and job == ojob and np.array_equal(lk["points_index"], olk["points_index"])
    assert abs(lk["value"] - olk["value"]) <= 1e-6 * abs(olk["value"]) and np.allclose(mean, omean, rtol=1e-5, atol=1e-12)


def test_kept_covariances_beyond_4_gib_are_refused(eng):
    """H A Mp 8 bytes of kept covariances above SPX_KG_MAX_LINE_BYTES: the pass with the moments kept is refused from the host's
    record before anything is queued -- 1 x 255 x 2 200 064 x 8 = 4.49e9 > 4 GiB -- and the handle runs a smaller pass right after."""
    N, M, D, A = 20, 2200000, 1, 255
    comp, cand, vals, rows = synthetic_problem(N, 300, D, 1, 3)
    big = np.random.RandomState(1).rand(M, D)
    pts = np.linspace(0.0, 1.0, A)[:, None]
    eng.set_observations(comp, vals); eng.set_candidates(big); eng.set_hypers(rows)
    eng.set_kg_points(pts)
    eng.factor()
    eng.set_acquisition("KG")
    try:
        for call in (eng.ei_step, eng.ei_run):
            with pytest.raises(ValueError) as ei_:
                call(KEEP)
            assert "kept covariances" in str(ei_.value)
        assert eng.stat("kg_points") == A and eng.get_acquisition() == (spx.ACQ_KG, 0.0)
        eng.set_candidates(cand)
        eng.ei_step(KEEP)
        assert eng.stat("last_kg_lines") == 1 and eng.kg_lines(0)[1].shape == (A, 300)
    finally:
        eng.set_acquisition("EI")


def _comm_case():
    """Two ranks on one device through the thread-rendezvous stand-in: with a communicator attached spx_set_acquisition refuses
    KG, and a handle that chose KG before it was attached refuses the pass; both then run an EI step together."""
    import threading
    from spearmint_amd.engine import Engine
    comp, cand, vals, rows = synthetic_problem(60, 512, 2, 2, 17)
    pts = cand[:4]
    eng = Engine(0)
    one = eng.ei_grid(comp, vals, cand, rows)
    uid = eng.comm_unique_id()
    P = 2
    res, errs = [None] * P, [None] * P

    def rank_main(r):
        try:
            e = Engine(0)
            e.set_observations(comp, vals)
            e.set_kg_points(pts)
            if r == 0:
                e.set_acquisition("KG")                 # chosen BEFORE the communicator
            e.comm_attach(uid, P, r)
            e.set_hypers(rows); e.set_candidates(cand[r * 256:(r + 1) * 256], index_base=r * 256)
            msgs = []
            if r == 0:
                try:
                    e.ei_step(0)
                    msgs.append("accepted")
                except ValueError as ex:
                    msgs.append(str(ex))
                e.set_acquisition("EI")
            try:
                e.set_acquisition("KG")
                msgs.append("accepted")
            except ValueError as ex:
                msgs.append(str(ex))
            e.ei_step(0)                                # the collective: both ranks, usable handles
            res[r] = (msgs, e.best(), e.get_acquisition(), e.stat("kg_points"))
            e.close()
        except BaseException as ex:
            errs[r] = "%s: %s" % (type(ex).__name__, ex)
    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    eng.close()
    return {"errors": [e for e in errs if e], "alive": any(t.is_alive() for t in th), "res": res, "one": (one[0], one[1])}


@pytest.mark.timeout(300)
def test_a_communicator_refuses_kg():
    from tests.test_gpu_d2_fake_rccl import _in_child
    out = _in_child(_comm_case)
    assert not out["errors"] and not out["alive"], out
    (m0, b0, a0, k0), (m1, b1, a1, k1) = out["res"]
    assert len(m0) == 2 and len(m1) == 1
    for m in m0 + m1:
        assert "SPX_ACQ_KG" in m and "communicator" in m, m
    assert a0 == a1 == (spx.ACQ_EI, 0.0) and k0 == k1 == 4
    assert b0 == b1 and b0[0] == out["one"][0] and b0[1] == out["one"][1]
