"""The 50-digit yardstick of the refinement objective (tests/refine_mp.py), its committed results
(tests/golden/refine_tail_mp.npz) and the batched host oracle the GPU tests use (tests/refine_helpers.py): the fixture is
exactly what the generator gives, the tail problem covers every band, the float64 oracle's own error against the yardstick
is pinned per band, and both restatements are held to oracle/gp_ei_oracle.py.  CPU only; the GPU side is
tests/test_gpu_m_refine_paths.py."""
import importlib.util
import os

import numpy as np
import pytest

from tests import refine_helpers as rh
from tests import refine_mp as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Max error of the float64 oracle (tests/refine_helpers.oracle: numpy / scipy) against the 50-digit reference per band of
# log10 |f| -- [-3, 1], [-20, -3), [-100, -20), [-300, -100) --, value (relative) and gradient (max_d |g_d - ref_d| /
# max_d |ref_d| per point), the largest over the nine covariance x branch cases and the two value sets, measured with
# this fixture:
#     value     1.75e-12, 2.77e-11, 9.07e-11, 6.90e-10
#     gradient  2.65e-12, 2.71e-11, 8.78e-11, 6.96e-10
# The ceilings are twice that, rounded up: another BLAS may add the same terms in another order, it will not lose another
# digit.
ORACLE_CEILING_VALUE = [3.6e-12, 5.6e-11, 1.9e-10, 1.4e-9]
ORACLE_CEILING_GRAD = [5.4e-12, 5.5e-11, 1.8e-10, 1.4e-9]
CASES = [(c, b) for c in rh.COVARS for b in rh.BRANCHES]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "refine_tail_mp.npz"))


def _rel(f, g, f0, g0):
    return (float(np.max(np.abs(f - f0) / np.abs(f0))),
            float(np.max(np.max(np.abs(g - g0), axis=1) / np.max(np.abs(g0), axis=1))))


def test_fixture_is_what_the_generator_gives(golden):
    """Everything in the file comes from mpmath and the seeded inputs alone: exact."""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_refine_tail",
                                                  os.path.join(ROOT, "scripts", "make_golden_refine_tail.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    generated = mod.generate()
    assert sorted(golden.files) == sorted(generated)
    for k, v in generated.items():
        np.testing.assert_array_equal(golden[k], v, err_msg=k)


@pytest.mark.parametrize("covar,branch", CASES)
def test_tail_problem_covers_every_band(golden, covar, branch):
    lf = np.concatenate([golden[rm.key(covar, branch, w, "log10f")] for w in rm.SETS])
    idx = rm.band_of(lf)
    for i in range(len(rm.TAIL_BANDS)):
        assert np.sum(idx == i) >= 5, (rm.TAIL_BANDS[i], int(np.sum(idx == i)))
    for w in rm.SETS:
        lw, f, g = (golden[rm.key(covar, branch, w, k)] for k in ("log10f", "f", "g"))
        assert f.shape == (rm.TAIL_P,) and g.shape == (rm.TAIL_P, rm.TAIL_D)
        assert np.all(f <= 0) and np.all(np.isfinite(g))
        assert np.all(f[lw < -330] == 0.0)                 # below the denormals the rounded reference is 0
    deep = np.sum(golden[rm.key(covar, branch, "tail", "log10f")] < -300)
    assert 1 <= deep <= 0.15 * rm.TAIL_P                   # some, and at most 15 % of the points


@pytest.mark.parametrize("covar,branch", CASES)
def test_float64_oracle_error_per_band(golden, covar, branch):
    p, pts, sets = rm.tail_problem(covar, branch)
    seen = []
    for w, vs in zip(rm.SETS, sets):
        f_ref, g_ref, lf = (golden[rm.key(covar, branch, w, k)] for k in ("f", "g", "log10f"))
        with np.errstate(all="ignore"):
            f, g = rh.oracle(rm.with_values(p, vs), pts)
        errs = rm.band_errors(f, g, f_ref, g_ref, lf)
        seen.append(errs)
        for e, cv, cg in zip(errs, ORACLE_CEILING_VALUE, ORACLE_CEILING_GRAD):
            assert e is None or (e[0] <= cv and e[1] <= cg), (w, errs)
        deep = lf < -300
        assert np.all((-f[deep] >= 0) & (-f[deep] <= 1e-290)) and np.all(np.isfinite(g))
    print(covar, branch, "float64 oracle, (value, gradient) error per band and value set:", seen)
    # the yardstick is not trivially equal to the oracle: in the tail the oracle is visibly off
    assert max(e[0] for e in seen[1] if e is not None) > 1e-12


@pytest.mark.parametrize("covar,branch", CASES)
def test_mp_matches_oracle_where_the_oracle_is_good(covar, branch):
    """A small mild problem per covariance and branch, two draws: the 50-digit restatement agrees with
    orc.grad_optimize_ei_over_hypers to the oracle's precision (same formula).  Without the 1e-6 amp2 jitter on the
    diagonal the two would differ at 1e-4."""
    pytest.importorskip("mpmath")
    p = rh.make_problem(3, covar, branch, N=9, D=3, H=2, S=3, n_pend=2)
    pts = rh.points(p, 3, 5)
    f, g = rm.neg_ei_and_grad_mp(p, pts)
    f, g = rm.to_float64(f), np.array([rm.to_float64(r) for r in g])
    f0, g0 = rh.orc_reference(p, pts)
    ev, eg = _rel(f0, g0, f, g)
    assert ev <= 1e-10 and eg <= 1e-10, (ev, eg)


@pytest.mark.parametrize("D", [1, 3, 9])
@pytest.mark.parametrize("covar,branch", CASES)
def test_batched_oracle_equals_the_oracle(covar, branch, D):
    """tests/refine_helpers.oracle (one factorisation per draw, every point against it) against
    orc.grad_optimize_ei_over_hypers (one per point and draw).  The bar: the GPU tests compare with the batched oracle at
    1e-7 / 1e-6, so it has to sit within 1e-10 of the oracle proper for that comparison to mean the same thing; what
    separates the two is the order of a few sums (measured: 7e-12 at worst)."""
    p = rh.make_problem(5 + D, covar, branch, N=23, D=D, H=2)
    pts = rh.points(p, 3, 6)
    f, g = rh.oracle(p, pts)
    f0, g0 = rh.orc_reference(p, pts)
    assert np.all(np.isfinite(f0)) and np.all(np.isfinite(g0))
    ev, eg = _rel(f, g, f0, g0)
    assert ev <= 1e-10 and eg <= 1e-10, (ev, eg)


def test_se_has_no_gradient_in_the_oracle():
    """gp.py defines no grad_SE: the reference's refinement raises with covar=SE, and so do both restatements.  (The
    library maps SE onto ARDSE with unit length scales; tests/test_gpu_m_refine_paths.py asserts that relation.)"""
    p = rh.make_problem(1, "SE", "plain", N=9, D=2, H=1)
    with pytest.raises(AttributeError):
        rh.oracle(p, rh.points(p, 1, 2))
    with pytest.raises(AttributeError):
        rh.orc_reference(p, rh.points(p, 1, 2))
