"""The 50-digit fixture of the refinement objective (tests/golden/refine_tail_mp.npz) is a reference of the GRID pass
too: with one draw, -f at the fixture's 150 points is what spx_ei_run returns for candidates = those points, in all
three branches.  Here the grid pass's float64 oracle (oracle/gp_ei_oracle.py: compute_ei, compute_ei_per_s,
compute_ei_fantasies) is held to the fixture per band, under the ceilings tests/test_refine_mp.py pins for the
refinement's oracle, and the host restatements tests/pending_helpers.py makes of the pass's plans are checked against
the cases csrc/ documents.  CPU only; the GPU side is tests/test_gpu_n_pending_paths.py."""
import os

import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import pending_helpers as ph
from tests import refine_helpers as rh
from tests import refine_mp as rm
from tests.test_refine_mp import CASES, ORACLE_CEILING_VALUE


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "refine_tail_mp.npz"))


@pytest.mark.parametrize("covar,branch", CASES)
def test_grid_oracle_against_the_50_digit_fixture(golden, covar, branch):
    """Measured (largest over the covariances and the two value sets, per band): fantasies 7.8e-13, 2.8e-11, 8.4e-11,
    6.9e-10; plain and per second 1.7e-12, 2.7e-11, 9.1e-11, 6.1e-10."""
    p, pts, sets = rm.tail_problem(covar, branch)
    seen = []
    for which, vs in zip(rm.SETS, sets):
        q = rm.with_values(p, vs)
        f_ref, lf = golden[rm.key(covar, branch, which, "f")], golden[rm.key(covar, branch, which, "log10f")]
        ei = ph.tail_oracle(q, pts)
        errs = ph.value_band_errors(ei, -f_ref, lf)
        seen.append(errs)
        for e, ceiling in zip(errs, ORACLE_CEILING_VALUE):
            assert e is None or e <= ceiling, (which, errs)
        deep = lf < -300
        assert np.mean(deep) <= 0.15
        assert np.all((ei[deep] >= 0) & (ei[deep] <= 1e-290))
        assert np.all(ei >= 0)
    print(covar, branch, "grid oracle against 50 digits, error per band and value set:", seen)
    assert any(e is not None for e in seen[1][2:])          # the tail set reaches the two deep bands


def test_helper_oracle_is_the_pending_branch_of_the_oracle():
    """ph.oracle (fantasy columns given) against orc.compute_ei_pending (columns drawn inside) on the same normals."""
    p = ph.problem(3, N=23, D=3, H=2, S=6, n_pend=2)
    cand = ph.candidates(p, 4, 40)
    ref = ph.oracle(p, cand)
    for h in range(p.H):
        want = orc.compute_ei_pending(p.comp, p.pend, cand, p.vals, p.rows[h], p.randn)
        np.testing.assert_allclose(ref[:, h], want, rtol=1e-12, atol=0)
    # one column at a time is the column's EI itself: the identity the mean-over-S test of the GPU file rests on
    cols = np.stack([ph.oracle(ph.with_columns(p, s, s + 1), cand) for s in range(p.S)], axis=2)
    np.testing.assert_allclose(np.mean(cols, axis=2), ref, rtol=1e-13, atol=0)


def test_time_mean_helper_is_the_oracles():
    p = ph.problem(5, N=30, D=2, H=2, S=3, n_pend=2)
    cand = ph.candidates(p, 6, 25)
    ld = ph.log_durs(p)
    assert ld.shape == (30,)
    for h in range(p.H):
        ei = orc.compute_ei(p.X, cand, ph.padded_vals(p), p.rows[h])
        per_s = orc.compute_ei_per_s(p.X, cand, ph.padded_vals(p), ld, p.rows[h], p.trows[h])
        np.testing.assert_allclose(ei / ph.oracle_time_mean(p, cand, h), per_s, rtol=1e-13, atol=0)


def test_padding_plan_restatement():
    """The cases csrc/predict_kernels.hip and the issue name: 1 .. 6 live tiles are skipped at 129 .. 224 and 257 .. 352
    rows and in the only row block up to 96; 97 .. 128, 230 and 600 decline."""
    for n, lt in ((16, 1), (17, 2), (33, 3), (64, 4), (65, 5), (96, 6), (129, 1), (144, 1), (145, 2), (224, 6), (257, 1),
                  (352, 6)):
        assert ph.padding_plan(n) == (lt, True), n
    for n in (97, 128, 225, 230, 247, 256, 600):
        assert not ph.padding_plan(n)[1], n
    assert rh.BRANCHES[2] == "fant"
