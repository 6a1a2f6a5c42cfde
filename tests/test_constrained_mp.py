"""The 50-digit yardstick of P(feasible) (tests/constrained_mp.py) and its committed results
(tests/golden/constrained_tail_mp.npz): the fixture is exactly what the generator gives, and the float64 oracle's own
error against it is pinned per band of log10 P.  CPU only; the GPU side is tests/test_gpu_k_constrained_paths.py."""
import importlib.util
import os

import numpy as np
import pytest

from tests import constrained_mp as cm
from tests import constrained_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Max relative error of the float64 oracle (numpy / scipy) against the 50-digit value, per band of log10 P -- [-3, 0],
# [-20, -3), [-100, -20), [-300, -100) -- measured for this seed: 9.7e-11, 3.0e-10, 1.05e-9, 9.4e-10 (draw 0, gain 3) and
# 3.4e-11, 4.5e-11, 5.1e-11 (draw 1, gain 0.75, nothing below 1e-22).  The ceilings are twice the larger of the two,
# rounded up: another BLAS may sum K* alpha in another order, it will not lose another digit.
ORACLE_CEILING = [2e-10, 6e-10, 2.2e-9, 2e-9]


@pytest.fixture(scope="module")
def generated():
    spec = importlib.util.spec_from_file_location("make_golden_constrained_tail",
                                                  os.path.join(ROOT, "scripts", "make_golden_constrained_tail.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.generate()


def test_fixture_is_what_the_generator_gives(generated, golden_dir):
    g = np.load(os.path.join(golden_dir, "constrained_tail_mp.npz"))
    assert sorted(g.files) == sorted(generated)
    for k in ("comp", "labels", "ff", "cand", "vals", "crows", "rows"):
        np.testing.assert_array_equal(g[k], generated[k], err_msg=k)
    # the valid-only GP's EI is float64 numpy: another BLAS build may differ in the last bits, nothing more
    np.testing.assert_allclose(g["ei_ref"], generated["ei_ref"], rtol=1e-11, atol=0)
    # everything that comes from mpmath is a function of the inputs (and of the stored EI) alone: exact
    ref = cm.tail_reference({k: g[k] for k in ("comp", "ff", "cand", "crows")}, g["ei_ref"])
    for k, v in ref.items():
        np.testing.assert_array_equal(g[k], v, err_msg=k)


def test_tail_problem_covers_every_band(golden_dir):
    g = np.load(os.path.join(golden_dir, "constrained_tail_mp.npz"))
    lp = g["log10P"][:, 0]
    for i, (lo, hi) in enumerate(cm.TAIL_BANDS):
        assert np.sum((lp >= lo) & ((lp <= hi) if i == 0 else (lp < hi))) >= 5, (lo, hi)
    below = np.sum(g["log10P"] < -300, axis=0)
    assert below[0] >= 1 and np.all(below <= 0.15 * lp.size)      # some, and at most 15 % of the candidates
    assert np.sum(1.0 - g["P_ref"][:, 0] <= 1e-12) >= 20             # the upper tail is there too
    assert np.all(g["P_ref"][g["log10P"] < -330] == 0.0)            # below the denormals the rounded reference is 0


def test_float64_oracle_error_per_band(golden_dir):
    g = np.load(os.path.join(golden_dir, "constrained_tail_mp.npz"))
    seen = []
    for h in range(g["crows"].shape[0]):
        P_o = co.constraint_prob("Matern52", g["comp"], g["ff"], g["crows"][h], g["cand"], False)
        errs = cm.band_errors(P_o, g["P_ref"][:, h], g["log10P"][:, h])
        seen.append(errs)
        for e, ceil in zip(errs, ORACLE_CEILING):
            assert e is None or e <= ceil, (h, errs)
        deep = g["log10P"][:, h] < -300
        assert np.all((P_o[deep] >= 0) & (P_o[deep] <= 1e-290))
    print("float64 oracle, max relative error per band and draw:", seen)
    # the yardstick is not trivially equal to the oracle: in the tail the oracle is visibly off
    assert max(e for e in seen[0][1:] if e is not None) > 1e-12


def test_mp_matches_oracle_where_the_oracle_is_good():
    """A small mild problem per covariance: the two restatements agree to the oracle's precision (same formula)."""
    rs = np.random.RandomState(3)
    comp, cand, ff = rs.rand(9, 3), rs.rand(11, 3), rs.randn(9)
    for covar in ("Matern52", "Matern32", "ARDSE", "SE"):
        ch = np.concatenate(([1.3, 1e-3, 0.9], rs.uniform(0.4, 1.2, 3)))
        got = cm.to_float64(cm.constraint_prob_mp(covar, comp, ff, ch, cand)["P"])
        np.testing.assert_allclose(co.constraint_prob(covar, comp, ff, ch, cand, False), got, rtol=1e-10, atol=0)
    got = cm.to_float64(cm.constraint_prob_mp("Matern52", comp, ff, ch, cand, all_valid=True)["P"])
    np.testing.assert_allclose(got, co.constraint_prob("Matern52", comp, ff, ch, cand, True), rtol=1e-15)
