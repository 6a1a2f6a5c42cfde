"""The 50-digit yardstick of PI and LCB (tests/acq_mp.py) and its committed results (tests/golden/acq_tail_mp.npz): the
fixture is exactly what the generator gives, and the float64 oracle's own error against it (tests/acq_oracle.py) is
pinned per band of log10 PI.  CPU only; the GPU side is tests/test_gpu_u_acquisition.py."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import acq_mp as am
from tests import acq_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Max relative error of the float64 oracle against the 50-digit PI, per band of log10 PI -- [-3, 0], [-20, -3),
# [-100, -20), [-300, -100) -- measured for this seed, the maximum over both draws and both xi: 4.1e-11, 1.4e-10, 9.2e-10,
# 9.7e-10 (the test prints all sixteen figures).  The ceilings are twice that, rounded up: another BLAS may sum K* alpha in
# another order, it will not lose another digit.
ORACLE_CEILING = [1e-10, 3e-10, 2e-9, 2e-9]
# LCB where kappa func_s is within 1e-6 of func_m: |oracle - reference| in units of eps (|func_m| + kappa func_s), the
# scale the parity tests use; measured 4.6e3 (the prior mean of 40 sits in func_m = k' alpha + mean), ceiling twice that.
LCB_CEILING_EPS = 1e4


@pytest.fixture(scope="module")
def generated():
    spec = importlib.util.spec_from_file_location("make_golden_acq_tail", os.path.join(ROOT, "scripts", "make_golden_acq_tail.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.generate()


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "acq_tail_mp.npz"))


def test_fixture_is_what_the_generator_gives(generated, g):
    assert sorted(g.files) == sorted(generated)
    for k in g.files:       # everything is a function of the seeded inputs alone, through mpmath: exact
        np.testing.assert_array_equal(g[k], generated[k], err_msg=k)


def test_tail_problem_covers_every_band(g):
    for h in range(g["rows"].shape[0]):
        for k in range(len(am.XIS)):
            lp = g["log10PI"][:, h, k]
            for i, (lo, hi) in enumerate(am.TAIL_BANDS):
                assert np.sum((lp >= lo) & ((lp <= hi) if i == 0 else (lp < hi))) >= 5, (h, k, lo, hi)
            deep = np.sum(lp < -300)
            assert 1 <= deep <= lp.size // 3
            assert np.all(g["PI_ref"][lp < -330, h, k] == 0.0)      # below the denormals the rounded reference is 0
    # u really starts near 0: some candidate of some draw has PI within [0.05, 0.95]
    assert np.any((g["PI_ref"] > 0.05) & (g["PI_ref"] < 0.95))


def oracle_pi(g, h, k):
    with orc.covar("Matern52"):
        func_m, func_v = ao.moments(g["comp"], g["cand"], g["vals"], g["rows"][h])
    return ao.value(ao.PI, g["xis"][k], func_m, func_v, np.min(g["vals"]))


def test_float64_oracle_error_per_band(g):
    seen = []
    for h in range(g["rows"].shape[0]):
        for k in range(len(am.XIS)):
            got = oracle_pi(g, h, k)
            ref, lp = g["PI_ref"][:, h, k], g["log10PI"][:, h, k]
            errs = am.band_errors(got, ref, lp)
            seen.append(errs)
            for e, ceil in zip(errs, ORACLE_CEILING):
                assert e is None or e <= ceil, (h, k, errs)
            deep = lp < -300
            assert np.all((got[deep] >= 0) & (got[deep] <= 1e-290))
    print("float64 oracle, max relative PI error per band, (draw, xi) in order:", seen)
    # the yardstick is not trivially equal to the oracle: in the tail the oracle is visibly off
    assert max(e for errs in seen for e in errs[1:] if e is not None) > 1e-12


def test_float64_oracle_lcb_where_it_cancels(g):
    eps = np.finfo(float).eps
    worst = 0.0
    for i, kappa in enumerate(g["lcb_kappa"]):
        c = int(g["lcb_cand"][i])
        m, s = g["func_m"][c, 0], g["func_s"][c, 0]
        assert abs(kappa * s - m) <= 1e-6 * abs(m) and kappa >= 0          # the case cancels as designed
        for h in range(g["rows"].shape[0]):
            with orc.covar("Matern52"):
                func_m, func_v = ao.moments(g["comp"], g["cand"], g["vals"], g["rows"][h])
            got = ao.value(ao.LCB, kappa, func_m, func_v, np.min(g["vals"]))
            scale = np.abs(g["func_m"][:, h]) + kappa * g["func_s"][:, h]
            worst = max(worst, float(np.max(np.abs(got - g["lcb_ref"][i, :, h]) / (eps * scale))))
    print("float64 oracle, LCB: max |error| / (eps (|func_m| + kappa func_s)) = %.3g" % worst)
    assert worst <= LCB_CEILING_EPS


def test_mp_matches_oracle_where_the_oracle_is_good():
    """A small mild problem per covariance: the two restatements agree to the oracle's precision (same formulas)."""
    rs = np.random.RandomState(5)
    comp, cand, vals = rs.rand(9, 3), rs.rand(11, 3), rs.randn(9)
    for covar in ("Matern52", "Matern32", "ARDSE"):
        hyper = np.concatenate(([0.1, 1e-2, 0.9], rs.uniform(0.4, 1.2, 3)))
        func_m, func_s = am.moments_mp(covar, comp, vals, hyper, cand)
        with orc.covar(covar):
            m_o, v_o = ao.moments(comp, cand, vals, hyper)
        best = np.min(vals)
        np.testing.assert_allclose(ao.value(ao.PI, 0.01, m_o, v_o, best), am.to_float64(am.pi_mp(func_m, func_s, best, 0.01)),
                                   rtol=1e-9, atol=0)
        np.testing.assert_allclose(ao.value(ao.LCB, 2.0, m_o, v_o, best), am.to_float64(am.lcb_mp(func_m, func_s, 2.0)),
                                   rtol=1e-9, atol=1e-12)
