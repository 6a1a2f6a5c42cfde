"""The predicted-duration yardstick itself, on the CPU (tests/persec_mp.py, tests/golden/persec_mp.npz): the fixture is what the
generator gives, the diag family is what the GPU tests rely on (K exactly diagonal, each observation the sole contributor
to its block with a contribution that shows, every wave / lane group / row of the tile / 64-row block / chunk owned once,
both sides of every clamp, denormal correlations and denormal durations), the full family's conditions span 1e2 .. 1e4, and
the float64 oracle's own error against the yardstick is pinned per family.

Measured here (numpy 2 / scipy / glibc): the oracle's worst |T - T_ref| over the diag family is 0.72 of the derived budget
under every kind; np.exp against mpmath on the family's own exponents 0.60 ulp (persec_mp.EXP_ULPS = 1); on the full
family at N = 24 with the host's K_t the oracle's worst relative error is 1.2e-13 (Matern52), 9.4e-14 (Matern32), 3.9e-13
(ARDSE), 2.1e-13 (SE), at cond(K_t) = 7e4.  The ceilings in tests/persec_mp.py are 1.5 x those, rounded up."""
import os

import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import cov_mp as cv
from tests import persec_mp as pm

LD = np.longdouble


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "persec_mp.npz")))


@pytest.fixture(scope="module")
def cov_fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "cov_lattice_mp.npz")))


def test_fixture_is_what_the_generator_gives(fixture):
    """A sampled slice, bit for bit: two sizes of one kind, the denormal case of another."""
    assert sorted(fixture) == sorted(["T_%s_%d" % (k, n) for k in cv.KINDS for n in pm.SIZES]
                                     + ["T_%s_denormal" % k for k in cv.KINDS])
    assert np.array_equal(pm.diag_reference("Matern52", 5), fixture["T_Matern52_5"])
    assert np.array_equal(pm.diag_reference("ARDSE", 65), fixture["T_ARDSE_65"])
    assert np.array_equal(pm.diag_reference("Matern32", pm.DENORMAL_N, pm.DENORMAL_MEAN_T, True), fixture["T_Matern32_denormal"])
    for key, val in fixture.items():
        N = pm.DENORMAL_N if key.endswith("denormal") else int(key.rsplit("_", 1)[1])
        assert val.shape == (pm.PER_BLOCK * N + 3, 3) and np.all(val >= 0.0), key


@pytest.mark.parametrize("N", pm.SIZES)
def test_diag_problem_is_diagonal_and_every_block_has_one_owner(N):
    X, C, owner, delta, ld = pm.diag_problem(N)
    ones = np.ones(1)
    xx = cv.exact_r2(X, X, ones)                                   # (raises if a distance is not exact)
    assert np.all(xx[~np.eye(N, dtype=bool)] >= pm.STEP ** 2) and pm.STEP ** 2 > max(cv.CLAMP.values())
    xc = cv.exact_r2(X, C, ones)
    assert np.array_equal(orc.dist2(ones, X, C), xc)               # the oracle's Gram form sees the same numbers
    for c in range(C.shape[0]):
        others = np.arange(N) != owner[c]
        assert np.all(xc[others, c] > max(cv.CLAMP.values())), c
        if owner[c] >= 0:
            assert xc[owner[c], c] == delta[c] ** 2
    assert np.array_equal(np.bincount(owner[owner >= 0], minlength=N), np.full(N, pm.PER_BLOCK)) and np.sum(owner < 0) == 3
    for kind in cv.KINDS:                                          # the time model's K, from the oracle: exactly diagonal
        for tr in pm.time_rows():
            K = pm.host_kt(kind, X, tr)
            assert np.array_equal(K, np.diag(np.full(N, tr[2] * (1.0 + 1e-6) + tr[1])))
    assert np.all(np.abs(ld) >= 5.0) and np.all(np.abs(ld) <= 30.0) and np.all(ld * 8 == np.round(ld * 8))
    assert all(np.all(np.abs(ld - m) >= 1.0) for m in pm.MEAN_T)


@pytest.mark.parametrize("kind", cv.KINDS)
def test_diag_family_reaches_what_the_gpu_tests_rely_on(cov_fixture, kind):
    owners = set()
    for N in pm.SIZES:
        X, C, owner, delta, ld = pm.diag_problem(N)
        E, alpha, k, u = pm.exponent(cov_fixture, kind, N)
        means = np.array(pm.MEAN_T, dtype=LD)[None, :]
        shows = np.abs(E - means) >= 0.5                           # a contribution no rounding could hide
        for j in range(N):
            assert np.all(np.any(shows[owner == j], axis=0)), (N, j)       # ... from every observation, in every draw
            owners.add((j // 16 % 4, j % 4, j % 16 // 4, j // 64 % 2, j // 128))
        near = owner >= 0
        r2 = delta[near] ** 2
        assert np.any(r2 == 0.0)
        if N >= 64:
            assert np.any((r2 < cv.CLAMP[kind]) & (r2 > 0.99 * cv.CLAMP[kind])) and np.any((r2 > cv.CLAMP[kind]) & (r2 < 1.01 * cv.CLAMP[kind]))
            kk = k[near].astype(np.float64)
            assert np.sum((kk > 0) & (kk < 2.0 ** -1022)) >= 3      # denormal correlations
            assert np.sum((kk == 0) & (r2 < cv.CLAMP[kind])) >= 1   # ... and ones that round to 0 inside the clamp
        assert np.all(np.abs(E) <= 60.0) and np.max(np.abs(E)) >= (10.0 if N > 2 else 3.0)
    # (wave, lane group g, r, 64-row block, 128-row chunk) of the sole contributor: all 4 x 4 x 4 x 2 of the first chunk, and
    # the second chunk
    assert len({o[:4] for o in owners if o[4] == 0}) == 128 and any(o[4] == 1 for o in owners)


@pytest.mark.parametrize("kind", cv.KINDS)
def test_denormal_case_is_denormal(fixture, kind):
    T = fixture["T_%s_denormal" % kind]
    assert np.all(T < 2.0 ** -1022) and np.sum(T > 0) >= T.size // 2 and np.any((T > 0) & (T <= 64 * 2.0 ** -1074))


@pytest.mark.parametrize("kind", cv.KINDS)
def test_oracle_error_on_the_diag_family_is_pinned(fixture, cov_fixture, kind):
    mp = pm._mp()
    worst, worst_exp = 0.0, 0.0
    for N in pm.SIZES:
        X, C, owner, delta, ld = pm.diag_problem(N)
        T = fixture["T_%s_%d" % (kind, N)]
        b = pm.budget(cov_fixture, kind, N, T)
        E = pm.exponent(cov_fixture, kind, N)[0].astype(np.float64)
        for h, tr in enumerate(pm.time_rows()):
            got = pm.oracle_time_mean(kind, pm.host_kt(kind, X, tr), X, C, tr, ld)
            worst = max(worst, float(np.max(np.abs(got.astype(LD) - T[:, h].astype(LD)) / b[:, h])))
            far = owner < 0
            assert np.array_equal(got[far], np.full(3, np.exp(tr[0])))
        with mp.workdps(pm.DPS):                                    # np.exp's own error on the family's exponents, in ulp
            for e in np.unique(E)[::7]:
                ref = mp.exp(mp.mpf(float(e)))
                worst_exp = max(worst_exp, float(abs(mp.mpf(float(np.exp(e))) - ref) / mp.mpf(float(np.spacing(float(ref))))))
    print("%s: oracle worst |T - T_ref| / budget = %.3f, np.exp worst %.3f ulp" % (kind, worst, worst_exp))
    assert worst <= pm.ORACLE_DIAG_CEILING[kind]
    assert worst_exp <= pm.EXP_ULPS


@pytest.mark.parametrize("covar", pm.FULL_COVARS)
@pytest.mark.parametrize("D", pm.FULL_D)
def test_full_family_spans_the_conditions_and_pins_the_oracle(covar, D):
    worst = 0.0
    for N in pm.FULL_N:
        X, C, vals, ld, rows, trows = pm.full_problem(covar, N, D)
        conds = []
        for d in range(3):
            K = pm.host_kt(covar, X, trows[d])
            conds.append(np.linalg.cond(K))
            assert trows[d, 1] >= 3e-4 * trows[d, 2]
            if N == pm.FULL_N[0]:
                ref = pm.full_reference(covar, K, X, C, trows[d], ld)
                worst = max(worst, pm.rel_error(pm.oracle_time_mean(covar, K, X, C, trows[d], ld), ref))
        assert min(conds) <= 1e2 and max(conds) >= 1e4, (N, conds)
        assert np.any(cv.exact_r2(X, C, np.ones(D)) == 0.0)        # a coincident candidate
    print("%s D=%d: oracle worst relative error %.3e" % (covar, D, worst))
    assert worst <= pm.ORACLE_FULL_CEILING[covar]


def test_full_yardstick_agrees_with_the_oracle_on_a_mild_problem():
    X, C, vals, ld, rows, trows = pm.full_problem("Matern52", 24, 3)
    K = pm.host_kt("Matern52", X, trows[0])
    ref = pm.full_reference("Matern52", K, X, C, trows[0], ld)
    got = pm.oracle_time_mean("Matern52", K, X, C, trows[0], ld)
    assert pm.rel_error(got, ref) <= 1e-14
    assert pm.rel_error(got * (1 + 1e-12), ref) >= 5e-13           # ... and rel_error sees an error that is there
