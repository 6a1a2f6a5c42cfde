"""The covariance yardstick itself, on the CPU (tests/cov_mp.py, tests/golden/cov_lattice_mp.npz): the fixture is what the
generator gives, the lattice inputs really have exact squared distances, they reach the edges the GPU tests rely on, and the
float64 oracle is within a pinned distance of the 50-digit values.

Measured here (numpy 2 / glibc), worst |oracle - k| / u over every distinct r^2 of every family, denormal results and results
that round to 0 included:   Matern52 1.03,  Matern32 0.92,  ARDSE 0.52.
Worst relative error of orc.gp_logprob against the closed form of two observations:   Matern52 4.9e-14,  Matern32 2.1e-14,
ARDSE 1.5e-14 (a^2 - b^2 cancels about two digits where k is near 1).
The ceilings (tests/cov_mp.py: ORACLE_CEILING, LOGPROB_CEILING) are 1.5 x those, rounded up: another libm may differ in an exp by an ulp, but will not lose a digit."""
import os

import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import cov_mp as cv

ORACLE_CEILING, LOGPROB_CEILING = cv.ORACLE_CEILING, cv.LOGPROB_CEILING


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "cov_lattice_mp.npz")))


@pytest.fixture(scope="module")
def families():
    return [(name, X, C, ls, cv.exact_r2(X, C, ls)) for name, X, C, ls in cv.lattice_problems()]


def test_fixture_is_what_the_generator_gives(fixture):
    ref = cv.reference()
    assert sorted(ref) == sorted(fixture)
    for key in ref:
        assert np.array_equal(ref[key], fixture[key]), key
    assert fixture["r2"].size <= 6000 and np.all(np.diff(fixture["r2"]) > 0)
    assert all(np.all(fixture["u_" + k] > 0) for k in cv.KINDS)


def test_oracle_distance_is_the_exact_one(families):
    for name, X, C, ls, ex in families:
        assert np.array_equal(orc.dist2(ls, X, C), ex), name
        assert np.array_equal(orc.dist2(ls, X), cv.exact_r2(X, X, ls)), name
    X, ls = cv.factor_problem(cv.FACTOR_NMAX)
    ex = cv.exact_r2(X, X, ls)
    assert np.array_equal(orc.dist2(ls, X), ex)
    # row 0 of the factor problem: from < 1e-3 to past every clamp already within its first three neighbours
    assert ex[0, 1] < 1e-3 and ex[0, 2] > 2.1e5 and ex[1, 3] == 0.0
    assert np.array_equal(np.concatenate([cv.exact_r2(p[:1], p[1:], ls).ravel() for p, ls, _ in cv.logprob_cases()]),
                          [r2 for _, _, r2 in cv.logprob_cases()])


def test_families_have_what_the_issue_asks(families):
    for name, X, C, ls, ex in families:
        assert np.any(ex == 0.0), name                                                    # a candidate equal to an observation
        assert np.any(np.triu(cv.exact_r2(X, X, ls) == 0.0, 1)), name                     # a pair of equal observations
        assert 2 <= X.shape[0] <= 40 and 64 <= C.shape[0] <= 192, name
    assert sorted({X.shape[1] for _, X, _, _, _ in families}) == [1, 3, 5, 8, 17, 33, 100]


@pytest.mark.parametrize("kind", cv.KINDS)
def test_coverage_of_the_edges(fixture, families, kind):
    r2, k = fixture["r2"], fixture["k_" + kind]
    s = {"Matern52": np.sqrt(5.0 * r2), "Matern32": np.sqrt(3.0 * r2), "ARDSE": 0.5 * r2}[kind]    # the exponential's argument
    denormal_exp = (s > 708.4) & (s < 744.4)                                  # exp(-s) in (2^-1074, 2^-1022)
    assert np.sum(denormal_exp) >= 20 and np.sum(denormal_exp & (k > 0)) >= 20
    below_clamp = r2 < cv.CLAMP[kind]
    assert np.sum((k == 0.0) & below_clamp) >= 5                              # results that round to 0 just past the denormals
    assert np.sum(below_clamp & (r2 > 0.99 * cv.CLAMP[kind])) >= 2 and np.sum(~below_clamp & (r2 < 1.01 * cv.CLAMP[kind])) >= 2
    assert np.all(k[~below_clamp] == 0.0)                                     # what cov_device.h says of its upper clamps
    assert np.sum((r2 > 0) & (r2 < 1e-8)) >= 10 and np.sum((r2 > 0) & (r2 < 1e-290)) >= 1
    assert np.all(k[(r2 < 1e-300)] == 1.0) and k[0] == 1.0 and r2[0] == 0.0   # ... and of the lower one
    assert sum(int(np.sum(ex == 0.0)) for _, _, _, _, ex in families) >= 10
    if kind == "ARDSE":
        assert 1600.0 in r2


@pytest.mark.parametrize("kind", cv.KINDS)
def test_oracle_error_is_pinned(families, kind):
    worst = 0.0
    for name, X, C, ls, ex in families:
        with orc.covar(kind), np.errstate(all="ignore"):
            k = orc.corr(ls, X, C).ravel()
        ur, first = np.unique(ex.ravel(), return_index=True)
        ref = [cv.corr_mp(kind, float(v))[0] for v in ur]
        err = cv.err_in_u(k[first], ref, [cv.u(kind, float(v)) for v in ur])
        worst = max(worst, float(err.max()))
        assert np.all(k[ex.ravel() == 0.0] == 1.0), name
    print("%s: oracle worst err / u = %.3f" % (kind, worst))
    assert worst <= ORACLE_CEILING[kind]


@pytest.mark.parametrize("kind", cv.KINDS)
def test_oracle_logprob_error_is_pinned(fixture, kind):
    mean, noise, amp2 = cv.LP_HYPER
    worst = 0.0
    for (pair, ls, _), ref in zip(cv.logprob_cases(), fixture["lp_" + kind]):
        with orc.covar(kind):
            got = orc.gp_logprob(pair, np.array(cv.LP_VALS), mean, amp2, noise, ls)
        worst = max(worst, abs(got - ref) / abs(ref))
    print("%s: orc.gp_logprob worst relative error %.3e" % (kind, worst))
    assert worst <= LOGPROB_CEILING[kind]


@pytest.mark.parametrize("kind", cv.KINDS + ("SE",))
def test_yardstick_agrees_with_oracle_on_a_mild_problem(kind):
    rs = np.random.RandomState(3)
    X, C, ls = rs.rand(12, 4), rs.rand(20, 4), rs.uniform(0.3, 1.5, 4)
    with orc.covar(kind):
        k = orc.corr(ls, X, C)
        r2 = orc.dist2(np.ones(4) if kind == "SE" else ls, X, C)
    ref = np.array([[float(cv.corr_mp(kind, float(v))[0]) for v in row] for row in r2])
    assert np.max(np.abs(k - ref) / ref) <= 1e-14


def test_lookup_refuses_values_outside_the_fixture(fixture):
    k, uu = cv.lookup(fixture, "SE", np.array([[0.0, 1600.0]]))
    assert np.array_equal(k, [[1.0, 0.0]]) and uu.shape == (1, 2)
    with pytest.raises(KeyError):
        cv.lookup(fixture, "Matern52", np.array([0.123456789]))
    with pytest.raises(KeyError):
        cv.lookup(fixture, "Matern52", np.array([1e30]))
