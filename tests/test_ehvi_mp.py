"""The float64 oracle of the expected hypervolume improvement (tests/ehvi_oracle.py) against its 50-digit yardstick
(tests/ehvi_mp.py, committed as tests/golden/ehvi_mp.npz), against Monte Carlo, and its n = 0 case against the product of two
EIs.  CPU only; the GPU side is tests/test_gpu_z_ehvi.py, whose bars are four times the errors pinned here."""
import os

import numpy as np
import pytest

from tests import acq_oracle as ao
from tests import ehvi_mp as em
from tests import ehvi_oracle as eo


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ehvi_mp.npz")))


def test_fixture_holds_the_generators_cases(fx):
    for band, (m1, v1, m2, v2, a, b, r1, r2) in em.cases().items():
        for key, v in zip(("_m1", "_v1", "_m2", "_v2", "_a", "_b"), (m1, v1, m2, v2, a, b)):
            assert np.array_equal(fx[band + key], v), band + key
        assert np.array_equal(fx[band + "_ref"], [r1, r2])
        assert np.array_equal(fx[band + "_scale"], em.scale(m1, v1, m2, v2, a, b, r1, r2))
        # the sub-normal allowance is exactly zero wherever no strip lies below u = -37.5: it covers nothing in the normal range
        _, allow, u_min = em.scale(m1, v1, m2, v2, a, b, r1, r2, parts=True)
        assert np.all(allow[u_min >= em.SUBNORMAL_BELOW] == 0.0) and np.all(allow >= 0.0), band
    assert sorted(em.cases()) == sorted(em.BANDS)
    assert np.sum(em.scale(*em.cases()["n0"], parts=True)[2] >= em.SUBNORMAL_BELOW) >= 30          # (most candidates are such)
    # a band small enough to go through mpmath again here: the stored values are what the generator gives
    m1, v1, m2, v2, a, b, r1, r2 = em.cases()["ulp"]
    vals, units = em.ehvi_mp(m1, v1, m2, v2, a, b, r1, r2)
    assert np.array_equal(fx["ulp_ehvi"], em.to_float64(vals)) and np.array_equal(fx["ulp_unit"], em.to_float64(units))
    assert np.all(fx["ulp_scale"] >= em.U * fx["ulp_unit"])            # the natural scale, weighted by factors >= 1
    # the lattice reaches from u = +8 down past -37, and the ulp band has neighbours one ulp apart in both objectives
    assert max(em.US) == 8.0 and min(em.US) < -37.0
    assert np.nextafter(fx["ulp_a"][0], np.inf) == fx["ulp_a"][1] and np.nextafter(fx["ulp_b"][0], -np.inf) == fx["ulp_b"][1]
    assert [len(fx[b + "_a"]) for b in ("n0", "n1", "n2", "n7", "n4096")] == [0, 1, 2, 7, 4096]


def test_strip_sum_is_the_integral_of_the_improvement(fx):
    """At 50 digits, on a two-point front: the sum over the strips against the quadrature of I(u, v) itself."""
    assert abs(float(fx["direct_integral"]) - float(fx["direct_strips"])) <= 2e-16 * float(fx["direct_strips"])
    d = em.DIRECT_CASE
    got = eo.ehvi(np.array([d[0]]), np.array([d[1]]), np.array([d[2]]), np.array([d[3]]), d[4], d[5], d[6], d[7])[0]
    assert abs(got - float(fx["direct_integral"])) <= 16 * em.U * float(fx["direct_integral"])


def test_float64_oracle_error_per_band(fx):
    for band in em.BANDS:
        got = eo.ehvi(fx[band + "_m1"], fx[band + "_v1"], fx[band + "_m2"], fx[band + "_v2"], fx[band + "_a"], fx[band + "_b"],
                      *fx[band + "_ref"])
        e = em.error(got, fx[band + "_ehvi"], fx[band + "_scale"])
        print("float64 oracle, %s: worst error %.3g units (pinned %.3g)" % (band, e, em.pinned(fx, band)))
        assert e <= em.pinned(fx, band), (band, e, em.pinned(fx, band))
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0)


@pytest.mark.parametrize("mom", [(0.8, 0.25, 1.2, 0.36), (0.1, 0.04, 2.6, 1.0), (1.6, 0.01, 0.4, 0.09)])
def test_against_monte_carlo(mom):
    a, b, r1, r2 = np.array([0.3, 0.9, 1.5]), np.array([2.2, 1.1, 0.2]), 2.0, 3.0
    m1, v1, m2, v2 = mom
    rng = np.random.RandomState(20261021)
    n = 4000000
    imp = eo.improvement(m1 + np.sqrt(v1) * rng.randn(n), m2 + np.sqrt(v2) * rng.randn(n), a, b, r1, r2)
    mc, se = float(np.mean(imp)), float(np.std(imp) / np.sqrt(n))
    got = float(eo.ehvi(np.array([m1]), np.array([v1]), np.array([m2]), np.array([v2]), a, b, r1, r2)[0])
    print("EHVI %.9g, Monte Carlo %.9g +- %.3g (%.2f standard errors)" % (got, mc, se, (got - mc) / se))
    assert abs(got - mc) <= 4.0 * se


def test_no_front_is_the_product_of_two_eis_bit_for_bit():
    rng = np.random.RandomState(7)
    m1, m2 = rng.randn(500), rng.randn(500) * 3.0
    v1, v2 = rng.rand(500) + 1e-3, rng.rand(500) * 4.0 + 1e-3
    v1[:3] = -1e-9                                                     # func_v < 0: NaN, as EI has it
    r1, r2 = 0.7, -0.2
    got = eo.ehvi(m1, v1, m2, v2, [], [], r1, r2)
    want = eo.g(m1, v1, r1) * eo.g(m2, v2, r2)                         # ei_device.h's EI, restated
    assert np.array_equal(got, want, equal_nan=True) and np.all(np.isnan(got[:3])) and not np.any(np.isnan(got[3:]))
    assert np.array_equal(np.signbit(got), np.signbit(want))
    # ... which is the EI of the other oracles up to how scipy.stats wraps the same two functions
    other = ao.value(ao.EI, 0.0, m1, v1, r1) * ao.value(ao.EI, 0.0, m2, v2, r2)
    assert np.allclose(got[3:], other[3:], rtol=1e-13, atol=0.0)
