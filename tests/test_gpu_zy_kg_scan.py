"""Option "kg_scan" (include/spx.h; csrc/kg_scan_kernels.hip), A up to 1023: values against tests/kg_oracle.py on the DEVICE'S OWN
lines at the plain test's bar (tests/test_gpu_zv_kg.py: hold_values); against the all-pairs pass: lines bit for bit, values within
two bars (both rules carry one); exact cases; paths bit for bit; state and refusals."""
import numpy as np
import pytest

from spearmint_amd import engine as spx
from spearmint_amd.synthetic import synthetic_problem
from tests import kg_helpers as kh
from tests import kg_mp as km
from tests import kg_oracle as ko
from tests.test_gpu_zv_kg import fx, hold_values, kg_pass, points_for  # noqa: F401  (fx: the fixture, tests/golden/kg_mp.npz)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = spx.Engine(0)
    e.set_option("kg_scan", 1)
    yield e
    e.close()


# every A beside two values of M and of N; n = A + 1 = 2, 3 (the smallest networks), 64, 65 (a power of two and one past it), 256,
# 257 (the first index a byte cannot hold), 258, 1024 (the last word of the bit set full); M = 1, 255, 257: below / across a scan
# workgroup and an order tile; N = 2, 65, 300: one, one and three row blocks
SHAPES = [  # A, M, N, H, D, covar
    (1, 1, 2, 1, 1, "Matern52"), (1, 255, 65, 3, 9, "SE"),
    (2, 255, 2, 3, 9, "Matern32"), (2, 257, 300, 1, 1, "ARDSE"),
    (63, 257, 65, 1, 9, "ARDSE"), (63, 1, 300, 3, 1, "Matern52"),
    (64, 255, 300, 3, 1, "SE"), (64, 257, 2, 1, 9, "Matern32"),
    (255, 257, 65, 1, 1, "Matern52"), (255, 1, 2, 3, 9, "SE"),
    (256, 255, 300, 1, 9, "Matern32"), (256, 257, 65, 3, 1, "ARDSE"),
    (257, 1, 300, 3, 9, "ARDSE"), (257, 255, 2, 1, 1, "Matern52"),
    (1023, 257, 65, 1, 9, "SE"), (1023, 1, 300, 3, 1, "Matern32"),
]


@pytest.mark.parametrize("A,M,N,H,D,covar", SHAPES)
def test_values_against_oracle_and_yardstick(eng, fx, A, M, N, H, D, covar):
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, 15000 + A, near=min(10, M))
    out = kg_pass(eng, comp, cand, vals, rows, points_for(comp, cand, A, A), covar)
    hold_values(fx, out, rows, "kg_scan A=%d M=%d N=%d H=%d D=%d %s" % (A, M, N, H, D, covar), n_mp=4 if A > 100 else 12)
    assert out["stats"] == (A, A, 1)


@pytest.mark.parametrize("A,M,N", [(2, 255, 65), (64, 257, 300), (255, 255, 65)])
def test_against_the_all_pairs_pass(eng, fx, A, M, N):
    comp, cand, vals, rows = synthetic_problem(N, M, 3, 3, 15100 + A)
    pts = points_for(comp, cand, A, A)
    scan = kg_pass(eng, comp, cand, vals, rows, pts)
    eng.set_option("kg_scan", 0)
    try:
        plain = kg_pass(eng, comp, cand, vals, rows, pts)
    finally:
        eng.set_option("kg_scan", 1)
    worst = 0.0
    for d in range(3):
        for k in (0, 1):
            assert np.array_equal(scan["lines"][d][k], plain["lines"][d][k]) and np.array_equal(scan["mom"][d][k], plain["mom"][d][k])
        mu, b = ko.lines(scan["mom"][d][0], scan["mom"][d][1], rows[d, 1], *scan["lines"][d])
        for c in range(M):
            u, band = ko.unit(mu[c], b[c]), km.band_of(ko.zmax(mu[c], b[c]))
            e = km.error(scan["draws"][c:c + 1, d], plain["draws"][c:c + 1, d], np.array([u]))
            worst = max(worst, e / (kh.MARGIN * km.pinned(fx, band)))
    print("A=%d: scan against all pairs, worst difference %.3g bars" % (A, worst))
    assert worst <= 2.0


@pytest.mark.parametrize("A", [9, 256, 1023])
def test_exact_cases(eng, A):
    """Every point a duplicate of one: the pass with that point alone, bit for bit (the tie rule drops A - 1 lines); under a draw
    whose prior mean lies 1e9 above the data the one breakpoint is beyond f's underflow: +0.0 exactly; a NaN coordinate in one
    candidate: NaN for that (d, c) alone; no value is negative."""
    comp, cand, vals, rows = synthetic_problem(70, 200, 3, 3, 15200 + A)
    cand[57, 1] = np.nan
    rows[2, 0] = 1e9
    pts = np.tile(np.full((1, 3), -1e3), (A, 1))                 # past every correlation's underflow: cov = 0, mu_a = the prior mean
    out, one = kg_pass(eng, comp, cand, vals, rows, pts), kg_pass(eng, comp, cand, vals, rows, pts[:1])
    ok = np.arange(200) != 57
    assert np.all(np.isnan(out["draws"][57])) and not np.any(np.isnan(out["draws"][ok]))
    assert np.array_equal(out["draws"], one["draws"], equal_nan=True)
    assert np.all(out["draws"][ok] >= 0.0) and not np.any(np.signbit(out["draws"][ok])) and np.any(out["draws"][ok][:, :2] > 0.0)
    func_m, func_v = out["mom"][2]                              # (the breakpoint of draw 2 from the device's own moments)
    far = ok & ((1e9 - func_m) * np.sqrt(func_v + rows[2, 1]) > 40.0 * func_v)
    assert np.sum(far) > 100 and np.all(out["draws"][far, 2] == 0.0)
    pts = points_for(comp, cand, A, 3)                           # ... and among ordinary lines
    out = kg_pass(eng, comp, cand, vals, rows[:2], pts)
    assert np.all(np.isnan(out["draws"][57])) and np.all(out["draws"][ok] >= 0.0) and not np.any(np.signbit(out["draws"][ok]))


@pytest.mark.parametrize("N", [101, 257, 300])
def test_bit_for_bit_across_paths(eng, N):
    M, H, D, A = 1000, 3, 3, 300
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, 15300 + N)
    pts = points_for(comp, cand, A, N)
    Np = (N + 127) // 128 * 128
    base = kg_pass(eng, comp, cand, vals, rows, pts)

    def same(o, what):
        assert np.array_equal(o["draws"], base["draws"]) and np.array_equal(o["mean"], base["mean"]) and o["best"] == base["best"], what
        for d in range(H if "lines" in o else 0):
            for k in (0, 1):
                assert np.array_equal(o["lines"][d][k], base["lines"][d][k]) and np.array_equal(o["mom"][d][k], base["mom"][d][k]), what
    defaults = {"kstar_budget_bytes": 0, "streams": 1, "gemm_partial": -1}
    for opts in ({"kstar_budget_bytes": 8 * Np * 512}, {"kstar_budget_bytes": 8 * Np * 1024}, {"streams": 2},
                 {"streams": 3, "kstar_budget_bytes": 8 * Np * 512}, {"gemm_partial": 0}):    # two chunks of one draw; one draw per group
        try:
            for k, v in opts.items():
                eng.set_option(k, v)
            same(kg_pass(eng, comp, cand, vals, rows, pts), opts)
        finally:
            for k in opts:
                eng.set_option(k, defaults[k])
    same(kg_pass(eng, comp, cand, vals, rows, pts, entry="factor"), "factor + run")
    same(kg_pass(eng, comp, cand, vals, rows, pts, flags=0), "without the moments")
    for d in range(H):                                           # a draw alone against the same draw among three
        one = kg_pass(eng, comp, cand, vals, rows[d:d + 1], pts)
        assert np.array_equal(one["draws"][:, 0], base["draws"][:, d]) and np.array_equal(one["lines"][0][1], base["lines"][d][1]), d


def test_state_refusals_and_statistics(eng):
    comp, cand, vals, rows = synthetic_problem(70, 130, 2, 2, 15400)
    pts = np.random.RandomState(1).rand(1024, 2)
    eng.set_observations(comp, vals); eng.set_candidates(cand); eng.set_hypers(rows)
    eng.set_acquisition("KG")
    stats = lambda: (eng.stat("last_kg_scan"), eng.stat("last_kg_points"))

    def refused(call, words):
        with pytest.raises(ValueError, match=words):
            call()
    try:
        eng.set_option("kg_scan", 0)
        refused(lambda: eng.set_kg_points(pts[:256]), "1 .. 255")
        eng.set_kg_points(pts[:5])
        eng.ei_step(0)
        assert stats() == (0, 5)
        for _ in range(2):                                       # setting the option, an unchanged value too, drops the results alone
            eng.set_option("kg_scan", 1)
            assert stats() == (0, 0) and eng.stat("kg_points") == 5
            refused(eng.ei_mean, "")
            eng.ei_run(0)                                        # (the factor stayed)
            assert stats() == (1, 5)
        eng.set_kg_points(pts[:256])
        refused(lambda: eng.set_kg_points(pts), "1 .. 1023")
        eng.set_kg_points(pts[:300])
        eng.set_option("kg_scan", 0)                             # 300 points stay held: the all-pairs pass refuses, naming the option
        refused(lambda: eng.ei_run(0), "300 representer points.*kg_scan")
        eng.set_option("kg_scan", 1)
        eng.ei_run(0)
        for call in (lambda: eng.ei_run(spx.FLAG_PER_SEC), lambda: eng.ei_run(spx.FLAG_CONSTRAINED), lambda: eng.ei_grad(np.zeros(2))):
            refused(call, "")
            assert stats() == (1, 300)
        eng.set_fantasies(np.zeros((2, 70, 3)), np.zeros((2, 3)))
        refused(lambda: eng.ei_run(0), "not defined over fantasies")
        eng.set_option("kg_fantasies", 1)
        eng.set_kg_points(pts[:256])
        refused(lambda: eng.ei_run(0), "256 representer points.*kg_fantasies")
    finally:
        eng.set_fantasies(None, None)
        eng.set_option("kg_fantasies", 0)
        eng.set_option("kg_scan", 1)
        eng.set_acquisition("EI")
