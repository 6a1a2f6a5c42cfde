"""spx_constrained_ei_grad_batch: the constrained chooser's refinement objective, -(sum over draws of EI x P(feasible))
and its gradient, on the GPU -- against the reference's own vectors (tests/golden/constrained_refine.npz), against the
host restatement (constrained.RefineModel), its invariants bit for bit, central differences, the error codes, and the
chooser with gpu_refine=1 against gpu_refine=0."""
import os

import numpy as np
import numpy.random as npr
import pytest

from tests import constrained_refine_helpers as hp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def eng():
    from spearmint_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


# -- 1. the reference's own output ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nopend", "pend", "allvalid"])
def test_matches_reference_golden(eng, golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "constrained_refine.npz"))
    npr.seed(int(g["rng_seed"]))
    p = hp.Problem()
    p.covar = "Matern52"
    p.comp, p.vals, p.labels, p.pend, p.ff = (g[tag + "_comp"], g[tag + "_vals"], g[tag + "_labels"], g[tag + "_pend"],
                                              g[tag + "_ff"])
    p.rows, p.chyp = g[tag + "_rows"], g[tag + "_crows"]
    p.D, p.H = p.comp.shape[1], p.rows.shape[0]
    p.S = int(g["pending_samples"]) if p.pend.shape[0] else 0
    p.randomstate = npr.get_state()
    good = p.labels > 0
    p.compv, p.valsv = p.comp[good], p.vals[good]
    hp.setup(eng, p)
    f, gr = eng.constrained_ei_grad_batch(g[tag + "_pts"], np.min(p.valsv))
    print(tag, "value rel err", np.max(np.abs(f / g[tag + "_f"] - 1)), "grad abs err", np.max(np.abs(gr - g[tag + "_g"])))
    assert np.allclose(f, g[tag + "_f"], rtol=1e-7, atol=1e-300)
    assert np.allclose(gr, g[tag + "_g"], rtol=1e-6, atol=1e-9 * np.abs(g[tag + "_g"]).max())


# -- 2. the host oracle --------------------------------------------------------------------------------------------
COVARS = ["Matern52", "Matern32", "ARDSE"]
SIZES = [(100, 127), (128, 129), (214, 256), (257, 300)]      # valid / completed: across the pad boundaries, unequal
DIMS = [1, 8, 33]
FANT = [0, 1, 100]
DRAWS = [1, 20]


@pytest.mark.parametrize("H", DRAWS)
@pytest.mark.parametrize("S", FANT)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("covar", COVARS)
def test_matches_host_oracle(eng, covar, size, D, S, H):
    """RefineModel summed over the draws, tolerances of test_ei_grad_batch_matches_oracle.  At D = 1 with S = 100 the
    reference's arithmetic has no result to compare with (its np.squeeze drops the dimension axis and the pending branch
    returns S numbers): the oracle there is RefineModel on the same problem embedded in two dimensions
    (constrained_refine_helpers.models)."""
    seed = 1000 + 97 * size[0] + 13 * D + 7 * S + H + 31 * len(covar)
    p = hp.make_problem(seed, covar=covar, D=D, n_valid=size[0], n_full=size[1], H=H, S=S, n_pend=3 if S else 0)
    hp.setup(eng, p)
    pts = hp.points(p, seed + 1, 21)          # uniform and comp[best] + 1e-3 randn, interleaved
    f_ref, g_ref = hp.oracle(p, pts)
    for P in (1, 8, 9, 21):                   # SPX_REFINE_PB is 8
        f, g = eng.constrained_ei_grad_batch(pts[:P], p.best)
        hp.assert_close(f, g, f_ref[:P], g_ref[:P])


@pytest.mark.parametrize("covar,S", [("Matern52", 1), ("Matern32", 100), ("ARDSE", 7)])
def test_no_violation_with_fantasies_matches_host_oracle(eng, covar, S):
    """Nc = 0 with pending jobs: P = 1, and the fantasies are still summed, not averaged."""
    p = hp.make_problem(77 + S, covar=covar, D=5, n_valid=140, n_full=140, H=3, S=S, n_pend=4)
    hp.setup(eng, p)
    pts = hp.points(p, 3, 9)
    f, g = eng.constrained_ei_grad_batch(pts, p.best)
    f_ref, g_ref = hp.oracle(p, pts)
    hp.assert_close(f, g, f_ref, g_ref)


# -- 3. invariants, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 5])
def test_a_point_alone_equals_the_point_in_a_batch(eng, S):
    p = hp.make_problem(5, D=6, n_valid=150, n_full=190, H=4, S=S, n_pend=3 if S else 0)
    hp.setup(eng, p)
    pts = hp.points(p, 9, 21)
    f, g = eng.constrained_ei_grad_batch(pts, p.best)
    for i in (0, 7, 8, 15, 16, 20):
        fi, gi = eng.constrained_ei_grad_batch(pts[i:i + 1], p.best)
        assert fi[0] == f[i] and np.array_equal(gi[0], g[i])
    f9, g9 = eng.constrained_ei_grad_batch(pts[5:14], p.best)
    assert np.array_equal(f9, f[5:14]) and np.array_equal(g9, g[5:14])


@pytest.mark.parametrize("covar", COVARS)
def test_no_violation_equals_ei_grad_batch(eng, covar):
    p = hp.make_problem(21, covar=covar, D=4, n_valid=131, n_full=131, H=5)
    hp.setup(eng, p)
    pts = hp.points(p, 2, 11)
    f, g = eng.constrained_ei_grad_batch(pts, p.best)
    f0, g0 = eng.ei_grad_batch(pts)
    assert np.array_equal(f, f0) and np.array_equal(g, g0)


def test_state_keeping_activity_keeps_the_bits_and_state_changes_rebuild(eng):
    from spearmint_amd.engine import Engine, FLAG_CONSTRAINED

    def fresh(q, pts):
        e = Engine(0)
        try:
            hp.setup(e, q)
            return e.constrained_ei_grad_batch(pts, q.best)
        finally:
            e.close()

    p = hp.make_problem(31, D=3, n_valid=90, n_full=120, H=3)
    hp.setup(eng, p)
    pts = hp.points(p, 4, 10)
    f, g = eng.constrained_ei_grad_batch(pts, p.best)
    eng.ei_step(FLAG_CONSTRAINED)                    # another grid pass: the state is the same
    f2, g2 = eng.constrained_ei_grad_batch(pts, p.best)
    assert np.array_equal(f, f2) and np.array_equal(g, g2)
    f_ref, g_ref = hp.oracle(p, pts)
    hp.assert_close(f, g, f_ref, g_ref)

    # new hypers (same sizes): the cached factor over the constraint model's points must not be reused
    q = hp.make_problem(31, D=3, n_valid=90, n_full=120, H=3)
    q.rows = p.rows * np.concatenate(([1.0, 1.0, 1.3], np.full(3, 0.8)))
    eng.set_hypers(q.rows)
    eng.set_constraint_model(q.comp, q.ff, hp.crows(q))
    eng.ei_step(FLAG_CONSTRAINED)
    got = eng.constrained_ei_grad_batch(pts, q.best)
    want = fresh(q, pts)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[0], f)

    # new observations (another set of valid points of the same completed set)
    r = hp.make_problem(31, D=3, n_valid=90, n_full=120, H=3)
    r.rows = q.rows
    r.labels = np.roll(q.labels, 5)
    good = r.labels > 0
    r.compv, r.valsv = r.comp[good], r.vals[good]
    r.best = np.min(r.valsv)
    eng.set_observations(r.compv, r.valsv)
    eng.set_hypers(r.rows)
    eng.set_constraint_model(r.comp, r.ff, hp.crows(r))
    eng.ei_step(FLAG_CONSTRAINED)
    got = eng.constrained_ei_grad_batch(pts, r.best)
    want = fresh(r, pts)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    # a changed X_c alone (same count, same objective state)
    t = hp.make_problem(31, D=3, n_valid=90, n_full=120, H=3)
    t.rows, t.labels, t.compv, t.valsv, t.best = r.rows, r.labels, r.compv, r.valsv, r.best
    t.comp = r.comp.copy()
    bad = np.nonzero(t.labels <= 0)[0]
    t.comp[bad] = np.clip(t.comp[bad] + 0.05, 0, 1)          # (only violating points move: the valid rows stay)
    eng.set_constraint_model(t.comp, t.ff, hp.crows(t))
    eng.ei_step(FLAG_CONSTRAINED)
    got_t = eng.constrained_ei_grad_batch(pts, t.best)
    want = fresh(t, pts)
    assert np.array_equal(got_t[0], want[0]) and np.array_equal(got_t[1], want[1])
    assert not np.array_equal(got_t[0], got[0])

    # option covar
    t.covar = "Matern32"
    eng.set_covar("Matern32")
    eng.ei_step(FLAG_CONSTRAINED)
    got_c = eng.constrained_ei_grad_batch(pts, t.best)
    want = fresh(t, pts)
    assert np.array_equal(got_c[0], want[0]) and np.array_equal(got_c[1], want[1])
    assert not np.array_equal(got_c[0], got_t[0])


# -- 4. it is a gradient ------------------------------------------------------------------------------------------------
# tests/test_constrained_refine_abi.py::test_host_restatement_is_the_gradient_of_its_value runs the same check on
# RefineModel for each branch on the CPU: every branch passes there (the variance taken from another factor than the
# mean and the sign of the constraint term included), so every branch is asserted here.
BRANCHES = {"nopend": dict(n_valid=30, n_full=40), "allvalid": dict(n_valid=40, n_full=40),
            "pend": dict(n_valid=30, n_full=40, S=5, n_pend=3), "pend_allvalid": dict(n_valid=40, n_full=40, S=5, n_pend=3)}


@pytest.mark.parametrize("branch", sorted(BRANCHES))
@pytest.mark.parametrize("covar", COVARS)
def test_central_differences(eng, branch, covar):
    p = hp.make_problem(11, covar=covar, D=4, H=2, **BRANCHES[branch])
    hp.setup(eng, p)
    for x in hp.points(p, 5, 4):
        x = np.clip(x, 1e-3, 1 - 1e-3)
        _, g = eng.constrained_ei_grad_batch(x[None], p.best)
        fd = hp.central_differences(lambda y: eng.constrained_ei_grad_batch(y[None], p.best)[0][0], x, range(3))
        assert np.allclose(fd, g[0][:3], rtol=2e-3, atol=1e-9), (branch, covar, fd, g[0][:3])


# -- 5. errors ------------------------------------------------------------------------------------------------------------
def _rc(eng, pts, P, best=0.0, f=True, g=True):
    from spearmint_amd.engine import _dp
    fo = np.empty(max(P, 1))
    go = np.empty((max(P, 1), pts.shape[1] if pts is not None else 1))
    rc = eng._lib.spx_constrained_ei_grad_batch(eng._h, _dp(pts), P, float(best), _dp(fo) if f else None,
                                                _dp(go) if g else None)
    return rc, eng._lib.spx_last_error()


def test_argument_errors(eng):
    from spearmint_amd.engine import SPX_ERR_ARG, MultiEngine
    p = hp.make_problem(2, D=3, n_valid=20, n_full=28, H=2)
    pts = hp.points(p, 1, 4)
    eng.set_observations(p.compv, p.valsv)
    eng.set_candidates(pts)
    eng.set_hypers(p.rows)
    rc, msg = _rc(eng, pts, 4)
    assert rc == SPX_ERR_ARG and msg                         # not factored
    eng.factor()
    rc, msg = _rc(eng, pts, 4)
    assert rc == SPX_ERR_ARG and b"spx_set_constraint_model" in msg          # no constraint model
    eng.set_constraint_model(p.comp, p.ff, hp.crows(p))
    rc, msg = _rc(eng, pts, 4)
    assert rc == SPX_ERR_ARG and b"not factored" in msg      # the model was set after the factorisation
    with pytest.raises(ValueError):
        eng.constrained_ei_grad_batch(pts, p.best)
    eng.factor()
    for bad in (_rc(eng, pts, 0), _rc(eng, pts, -3), _rc(eng, None, 4), _rc(eng, pts, 4, f=False), _rc(eng, pts, 4, g=False)):
        assert bad[0] == SPX_ERR_ARG and bad[1]
    f, g = eng.constrained_ei_grad_batch(pts, p.best)          # and the handle works
    hp.assert_close(f, g, *hp.oracle(p, pts))
    m = MultiEngine([0], None)
    try:
        m.set_observations(p.compv, p.valsv)
        m.set_candidates(pts)
        m.set_hypers(p.rows)
        m.factor()
        with pytest.raises(ValueError):
            m.constrained_ei_grad_batch(pts, p.best)
    finally:
        m.close()


def test_not_positive_definite_full_covariance(eng):
    """The valid points and the constraint GP factor; the objective's hypers over ALL completed points do not: two
    violating points coincide and draw 1's noise is tiny and negative (-1.5e-6 amp2: it cancels the jitter, so the
    duplicated rows' 2 x 2 block has the eigenvalue -5e-7 amp2, while the 24 spread-out valid points, at length scale
    0.1, stay well conditioned).  An ordinary status code of an ordinary call."""
    p = hp.make_problem(8, D=2, n_valid=24, n_full=30, H=3)
    bad = np.nonzero(p.labels <= 0)[0]
    p.comp[bad[1]] = p.comp[bad[0]]
    p.rows[:, 3:] = 0.1
    good_noise = p.rows[1, 1]
    p.rows[1, 1] = -1.5e-6 * p.rows[1, 2]
    hp.setup(eng, p)                      # the valid points have no duplicate: the step itself succeeds
    pts = hp.points(p, 1, 3)
    with pytest.raises(np.linalg.LinAlgError):
        eng.constrained_ei_grad_batch(pts, p.best)
    draw, pivot = eng.not_pd_info()
    assert draw == 3 * p.H + 1 and pivot == max(bad[0], bad[1])
    # the handle works afterwards
    p.rows[1, 1] = good_noise
    hp.setup(eng, p)
    f, g = eng.constrained_ei_grad_batch(pts, p.best)
    hp.assert_close(f, g, *hp.oracle(p, pts))


# -- 6. the chooser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nan", "mixed_noiseless", "allvalid"])
def test_chooser_gpu_refine_equals_host_refine(golden_dir, tmp_path, name):
    from spearmint_amd.chooser import GPConstrainedEIChooser as mod
    g = np.load(os.path.join(golden_dir, "constrained_next_%s.npz" % name))
    out = {}
    for flag in (1, 0):
        d = tmp_path / ("r%d" % flag)
        d.mkdir()
        c = mod.init(str(d), str(g["args"]) + ",gpu_refine=%d" % flag)
        st = npr.get_state()
        rets = []
        for k in range(int(g["ncalls"])):
            npr.set_state((st[0], g["before%d_key" % k], int(g["before%d_pos" % k]), int(g["before%d_has_gauss" % k]),
                           float(g["before%d_cached" % k])))
            ret = c.next(g["grid"], g["values"], np.ones(g["grid"].shape[0]), g["candidates%d" % k], g["pending%d" % k],
                         g["complete%d" % k])
            st = npr.get_state()
            rets.append((ret, st))
        out[flag] = rets
    for (a, sa), (b, sb) in zip(out[1], out[0]):
        assert isinstance(a, tuple) == isinstance(b, tuple)
        if isinstance(a, tuple):
            assert a[0] == b[0]
            np.testing.assert_allclose(a[1], b[1], rtol=1e-6, atol=1e-9)
        else:
            assert a == b
        np.testing.assert_array_equal(sa[1], sb[1])
        assert sa[2:] == sb[2:]
