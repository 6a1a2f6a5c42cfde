"""Value and gradient of posterior sample paths off the grid on the GPU (include/spx.h: spx_thompson_grad_batch;
csrc/ts_grad_kernels.hip, ts_device.h) against tests/ts_grad_oracle.py and a long-double route.  Sorted after
test_gpu_zt_thompson.py, whose tests of spx_thompson should be read first when both fail.

Shapes: N in {2, 65, 130, 257} (one row pair, both sides of the 64-row tile, the 256-thread stride of the update kernel),
M = 257, D in {1, 3, 5, 9, 33} (Dp = 4, 8, 16 with the points in registers and Dp = 64, which re-reads them and walks the gradient
in two groups of 32 dimensions), F in {16, 48, 1024}, S in {1, 17}, H in {1, 3}, per_draw both ways, P in {1, 15, 16, 17, 65}
(the tails of the 16-point tile and of the 64-point workgroup), every covar -- each axis crossed at least once in CASES.

What is asserted:
  prior       at points equal to candidate rows and to observation rows, each under a path of its own: == spx_get_thompson_prior
              bit for bit
  prior grad  with mean = 0, eps = 0 and the observed values set to the prior of one path at the observations that path's
              Gamma and alpha are exactly zero, so its value is the prior and its gradient the prior's gradient, bit for bit;
              held to ts_grad_oracle.grad_bound, the largest share printed (measured on an MI355X: see README.md)
  update      value - prior and grad - gp (gp from the oracle) against long double on the device's own K and K*: 4 x the
              larger error of the two float64 reference routes, floor 16 x 2^-52, in units of sum_j |k_j alpha_j| and
              sum_j |dk_j/dx alpha_j|; value - prior against path - prior of the resident path within the sum of both bars
  LCB         w = 0, eps = 0, H = 1: value and grad against spx_ei_grad_batch under LCB with kappa = 0 (func_m and HALF its gradient)
  gradient    central differences of the device's own value (step 1e-6, rtol 2e-3, atol 1e-9: test_gpu_m_refine_paths.py)
  bits        a point alone, at another position, among points of other paths and draws, S = 1 against S = 17, a second call
              (the cached alpha), after the handle held a problem of another padded size
  state       paths, priors and a following EI pass unchanged; whatever drops results makes the call refuse; a refused call
              changes nothing; a fresh spx_thompson rebuilds alpha
  special     a NaN and a +inf coordinate give NaN for that point alone
  refusals    each with its message
  chooser     GPEIOptChooser with ts_refine=1 on the 300-row Branin grid, 0 and 2 pending jobs
"""
import ctypes
import os

import numpy as np
import pytest
import scipy.linalg as spla
from scipy.linalg import lapack

from spearmint_amd import engine as spx
from spearmint_amd.chooser import GPEIOptChooser
from tests import constrained_refine_helpers as crh
from tests import moments_ld as ml
from tests import ts_grad_oracle as tgo
from tests import ts_oracle as tso
from tests.factor_helpers import chol_longdouble
from tests.helpers import branin
from tests.mes_helpers import same_state
from tests.test_gpu_zt_thompson import load, padded_dim, problem, scramble

pytestmark = pytest.mark.gpu
LD = np.longdouble
M = 257
SHARES = {"prior gradient": [], "update value": [], "update gradient": []}


@pytest.fixture(scope="module")
def eng():
    e = spx.Engine(0)
    yield e
    e.set_covar("Matern52")
    e.close()


#        covar       N    D   F     S   H  per_draw P
CASES = [("Matern52", 2, 1, 16, 1, 1, False, 1),
         ("Matern32", 65, 3, 48, 17, 3, False, 15),
         ("ARDSE", 130, 9, 1024, 1, 3, True, 16),
         ("SE", 257, 33, 48, 17, 1, False, 17),
         ("Matern52", 257, 5, 1024, 17, 3, True, 65),
         ("Matern32", 130, 33, 16, 1, 1, False, 65)]


def setup(eng, covar, N, D, F, S, H, per_draw, seed, mean0=False):
    P = problem(N, M, D, H, seed)
    if mean0:
        P[3][:, 0] = 0.0
    load(eng, covar, P)
    R = spx.thompson_randoms(np.random.RandomState(seed + 1), covar, D, H, N, F, S, per_draw)
    eng.thompson(S=S, F=F, randoms=R, per_draw=per_draw)
    return P, R


def paths_for(rs, n, H, S):
    """A path per point: the first and the last path always named when there is room."""
    po = rs.randint(0, H * S, n).astype(np.int32)
    po[0] = H * S - 1
    if n > 1:
        po[-1] = 0
    return po


# ---- 1. the prior, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("covar,N,D,F,S,H,per_draw,P", CASES)
def test_prior_bit_for_bit(eng, covar, N, D, F, S, H, per_draw, P):
    (comp, cand, vals, rows), R = setup(eng, covar, N, D, F, S, H, per_draw, 100 + N + D)
    rs = np.random.RandomState(N + P)
    priors = {}

    def prior_of(k):
        if k not in priors:
            priors[k] = eng.thompson_prior(k // S, k % S)
        return priors[k]
    for rows_x, which, n in ((cand, 0, P), (comp, 1, min(P, N))):
        pick = rs.permutation(rows_x.shape[0])[:n]
        po = paths_for(rs, n, H, S)
        f, g, pr = eng.thompson_grad_batch(rows_x[pick], po, want_prior=True)
        want = np.array([prior_of(int(k))[which][i] for k, i in zip(po, pick)])
        assert np.array_equal(pr, want), (which, pr - want)
        assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    f0, g0, p0 = eng.thompson_grad_batch(cand[:P], None, want_prior=True)                # path_of = NULL: path 0 of draw 0
    assert np.array_equal(p0, prior_of(0)[0][:P])
    f1, g1, p1 = eng.thompson_grad_batch(cand[:P], np.zeros(P, dtype=np.int32), want_prior=True)
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1) and np.array_equal(p0, p1)


# ---- 3. the prior's gradient at its derived bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("covar,N,D,F,S,H,per_draw,P", CASES)
def test_prior_gradient_within_the_derived_bound(eng, covar, N, D, F, S, H, per_draw, P):
    """mean = 0, eps = 0, vals = the prior of path k at the observations: rhs_k = (vals - prior) - sig 0 = 0 exactly, so Gamma_k and
    alpha_k are zero, m = 0 and gu = 0: value == prior and grad == gp bit for bit, for that path."""
    seed = 200 + N + D
    (comp, cand, vals, rows), R = setup(eng, covar, N, D, F, S, H, per_draw, seed, mean0=True)
    R["eps"][...] = 0.0
    k = H * S - 1
    d, s = divmod(k, S)
    po = eng.thompson_prior(d, s)[1]
    eng.set_observations(comp, po)
    eng.factor()
    eng.thompson(S=S, F=F, randoms=R, per_draw=per_draw)
    assert np.array_equal(eng.thompson_prior(d, s)[1], po)                       # (the prior does not read the values)
    rs = np.random.RandomState(seed)
    x = np.vstack((cand[:P // 2], rs.rand(P - P // 2, D)))
    f, g, pr = eng.thompson_grad_batch(x, np.full(P, k, dtype=np.int32), want_prior=True)
    assert np.array_equal(f, pr)
    pth = tgo.Path(covar, comp, po, rows[d], R, s, d, per_draw)                  # (only its prior is read)
    p_ref, gp_ref, sn = pth.prior(x)
    bound = tgo.grad_bound(rows[d], pth.w, pth.nu, pth.phase, x, padded_dim(D), sn)
    share = float(np.max(np.abs(g.astype(LD) - gp_ref) / bound))
    SHARES["prior gradient"].append(share)
    print("prior gradient %s N=%d D=%d F=%d S=%d H=%d P=%d: largest share of the bound %.4f" % (covar, N, D, F, S, H, P, share))
    assert share <= 1.0
    # and it is the gradient of what k_ts_prior computes: the sign convention, by central differences of the prior itself
    h = 1e-6
    for j in range(min(D, 3)):
        e = np.zeros(D)
        e[j] = h
        fp = eng.thompson_grad_batch(x + e, np.full(P, k, dtype=np.int32), want_prior=True)[2]
        fm = eng.thompson_grad_batch(x - e, np.full(P, k, dtype=np.int32), want_prior=True)[2]
        assert np.allclose((fp - fm) / (2 * h), g[:, j], rtol=2e-3, atol=1e-8), j


# ---- 2. + 4a. the update term against long double -----------------------------------------------------------------------------------
def route_errors(K, y, kx, dk, ref_m, ref_g, s_m, s_g):
    """Largest errors of the two float64 reference routes -- LAPACK's (dpotrf, cho_solve) and the library's algorithm in numpy
    (W = L^-1 by dtrtri, alpha = W^T (W y)) -- for k' alpha and dk' alpha, in units of the natural scales."""
    L, info = lapack.dpotrf(np.asarray(K, dtype=np.float64), lower=1, clean=1, overwrite_a=0)
    assert info == 0
    W = np.tril(lapack.dtrtri(L, lower=1, unitdiag=0, overwrite_c=0)[0])
    out = []
    for alpha in (spla.cho_solve((L, True), y), np.dot(W.T, np.dot(W, y))):
        m = np.dot(kx, alpha)
        g = np.einsum("ijd,j->id", dk, alpha)
        out.append((float(np.max(np.abs(m.astype(LD) - ref_m) / s_m)), float(np.max(np.abs(g.astype(LD) - ref_g) / s_g))))
    return out


@pytest.mark.parametrize("covar,N", [("Matern52", 65), ("Matern52", 130), ("ARDSE", 257), ("Matern32", 257)])
def test_update_term_against_long_double(eng, covar, N):
    assert np.finfo(np.longdouble).nmant >= 63
    H, S, F, D = 1, 3, 48, 3
    (comp, cand, vals, rows), R = setup(eng, covar, N, D, F, S, H, False, 300 + N)
    K = eng.get_factor(0, want_L=False, want_alpha=False)[0]
    Ks = np.ascontiguousarray(eng.get_cross_cov(0))                              # (N, M): the device's own K*
    mean = float(rows[0][0])
    _, dk_ld = tgo.kernel_ld(covar, rows[0], comp, cand)                         # (M, N, D)
    dk64 = dk_ld.astype(np.float64)
    for s in range(S):
        pc, po = eng.thompson_prior(0, s)
        path = eng.thompson_path(0, s)
        f, g, pr = eng.thompson_grad_batch(cand, np.full(M, s, dtype=np.int32), want_prior=True)
        assert np.array_equal(pr, pc)
        rhs = (vals - po) - tso.sig_of(rows[0]) * R["eps"][s]                   # k_ts_rhs, operation for operation
        y = rhs - mean
        _, _, alpha, _ = chol_longdouble(K, y)
        terms = Ks.T.astype(LD) * alpha[None, :]
        ref_m, s_m = np.sum(terms, axis=1), np.sum(np.abs(terms), axis=1)
        gterms = dk_ld * alpha[None, :, None]
        ref_g, s_g = np.sum(gterms, axis=1), np.sum(np.abs(gterms), axis=1)
        (ml_, gl_), (mb_, gb_) = route_errors(K, y, Ks.T, dk64, ref_m, ref_g, s_m, s_g)
        bar_m = max(4.0 * max(ml_, mb_), 16 * 2.0 ** -52)
        bar_g = max(4.0 * max(gl_, gb_), 16 * 2.0 ** -52)
        got_m = ((f - pr) - mean).astype(LD)
        dev_m = float(np.max(np.abs(got_m - ref_m) / s_m))
        pth = tgo.Path(covar, comp, vals, rows[0], R, s)
        gp_ref = pth.prior(cand)[1]
        dev_g = float(np.max(np.abs((g.astype(LD) - gp_ref) - ref_g) / s_g))
        SHARES["update value"].append(dev_m / bar_m)
        SHARES["update gradient"].append(dev_g / bar_g)
        print("update %s N=%d s=%d: value device %.2e lapack %.2e as built %.2e (device / bar %.3f); gradient device %.2e "
              "lapack %.2e as built %.2e (device / bar %.3f)" % (covar, N, s, dev_m, ml_, mb_, dev_m / bar_m, dev_g, gl_, gb_, dev_g / bar_g))
        assert dev_m <= bar_m and dev_g <= bar_g
        # the resident path is another sum of the same number (beta . Gamma), held to long double by test_gpu_zt_thompson.py at a
        # bar formed the same way in units of |B|_2 |Gamma|_2 + |mean|: the two agree within the sum of the two routes' bars
        args = (K, Ks, y, mean, ml.prior_v_of(rows[0]))
        ref = ml.moments_longdouble(*args)
        bar_p = max(4.0 * max(ml.errors(*ml.moments_lapack(*args), ref=ref)[0], ml.errors(*ml.moments_as_built(*args), ref=ref)[0]),
                    16 * 2.0 ** -52)
        gap = np.abs((f - pr) - (path - pc))
        assert np.all(gap <= bar_m * s_m.astype(np.float64) + bar_p * ref.s_m.astype(np.float64))


# ---- 4b. against spx_ei_grad_batch under LCB ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("covar,N,D", [("Matern52", 65, 3), ("Matern32", 130, 9), ("ARDSE", 257, 5)])
def test_zero_randoms_give_the_lcb_objective(eng, covar, N, D):
    """w = 0 and eps = 0: the path is the posterior mean.  spx_ei_grad_batch under LCB with kappa = 0 returns func_m and HALF its
    gradient (the reference's scaling, refine_kernels.hip); two different sums of one number, so within that call's own
    tolerances (tests/constrained_refine_helpers.py) plus 32 x 2^-52 of the natural scales."""
    F, S, H, P = 48, 1, 1, 21
    (comp, cand, vals, rows), R = setup(eng, covar, N, D, F, S, H, False, 400 + N)
    R["w"][...] = 0.0
    R["eps"][...] = 0.0
    eng.thompson(S=S, F=F, randoms=R)
    x = np.vstack((cand[:10], np.random.RandomState(N).rand(P - 10, D)))
    f, g, pr = eng.thompson_grad_batch(x, want_prior=True)
    assert np.all(pr == 0.0)
    prev = eng.get_acquisition()
    try:
        eng.set_acquisition(spx.ACQ_LCB, 0.0)
        f_l, g_l = eng.ei_grad_batch(x)
    finally:
        eng.set_acquisition(*prev)
    pth = tgo.Path(covar, comp, vals, rows[0], R, 0)
    k_ld, dk_ld = tgo.kernel_ld(covar, rows[0], comp, x)
    s_m = np.sum(np.abs(k_ld * pth.alpha[None, :]), axis=1).astype(np.float64)
    s_g = np.sum(np.abs(dk_ld * pth.alpha[None, :, None]), axis=1).astype(np.float64)
    floor = 32 * 2.0 ** -52
    assert np.all(np.abs(f - f_l) <= crh.VALUE_RTOL * np.abs(f_l) + floor * (s_m + abs(rows[0][0])))
    assert np.all(np.abs(g - 2.0 * g_l) <= crh.GRAD_RTOL * np.abs(2.0 * g_l) + crh.GRAD_ATOL_REL * np.max(np.abs(2.0 * g_l)) + floor * s_g)
    # and against the oracle's own path
    f_o, g_o = pth(x)
    assert np.allclose(f, f_o, rtol=1e-9, atol=1e-9 * np.max(s_m)) and np.allclose(g, g_o, rtol=1e-8, atol=1e-9 * np.max(s_g))


# ---- 5. it is a gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE", "SE"])
def test_central_differences(eng, covar, D):
    """Step and tolerance of tests/test_gpu_m_refine_paths.py::test_central_differences (1e-6; rtol 2e-3, atol 1e-9), without
    the factor one half: grad is the TRUE derivative of value."""
    N, F, S, H = 40, 48, 2, 2
    (comp, cand, vals, rows), R = setup(eng, covar, N, D, F, S, H, True, 500 + D)
    rs = np.random.RandomState(D)
    po = np.array([3], dtype=np.int32)
    for x in (rs.rand(D), comp[int(np.argmin(vals))] + 0.01 * rs.randn(D)):
        x = np.clip(x, 1e-3, 1 - 1e-3)
        f, g = eng.thompson_grad_batch(x[None], po)
        f_o, g_o = tgo.value_grad(covar, comp, vals, rows[1], R, 1, x[None], d=1, per_draw=True)
        assert np.allclose(f, f_o, rtol=1e-9, atol=1e-9) and np.allclose(g, g_o, rtol=1e-7, atol=1e-8)
        for j in range(min(D, 3)):
            e = np.zeros(D)
            e[j] = 1e-6
            fd = (eng.thompson_grad_batch((x + e)[None], po)[0][0] - eng.thompson_grad_batch((x - e)[None], po)[0][0]) / 2e-6
            assert np.allclose(fd, g[0][j], rtol=2e-3, atol=1e-9), (covar, D, j, fd, g[0])


# ---- 6. invariants, bit for bit -------------------------------------------------------------------------------------------------------
def test_a_points_numbers_do_not_depend_on_the_call(eng):
    covar, N, D, F, S, H = "Matern52", 130, 5, 48, 17, 3
    P0 = problem(N, M, D, H, 600)
    comp, cand, vals, rows = P0
    R = spx.thompson_randoms(np.random.RandomState(6), covar, D, H, N, F, S)
    load(eng, covar, P0)
    eng.thompson(S=S, F=F, randoms=R)
    rs = np.random.RandomState(61)
    x = rs.rand(65, D)
    po = paths_for(rs, 65, H, S)
    base = eng.thompson_grad_batch(x, po, want_prior=True)
    again = eng.thompson_grad_batch(x, po, want_prior=True)                       # the cached alpha
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    for i in (0, 15, 16, 37, 64):                                                 # alone
        one = eng.thompson_grad_batch(x[i:i + 1], po[i:i + 1], want_prior=True)
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(one, base)), i
    perm = rs.permutation(65)                                                     # at another position, among other paths
    moved = eng.thompson_grad_batch(x[perm], po[perm], want_prior=True)
    assert all(np.array_equal(a, b[perm]) for a, b in zip(moved, base))
    mixed = eng.thompson_grad_batch(x, np.roll(po, 1), want_prior=True)           # every neighbour under another path
    same = np.roll(po, 1) == po
    redo = eng.thompson_grad_batch(x[::-1][:17], po[::-1][:17], want_prior=True)
    assert all(np.array_equal(a, b[::-1][:17]) for a, b in zip(redo, base)) and len(mixed[0]) == 65 and not np.all(same)
    # S = 1 against S = 17 for the same randoms: path (d, 0) of the wide call is path d of the narrow one
    sel = np.nonzero(po % S == 0)[0]
    sel = np.concatenate((sel, [0]))
    xs, ds = x[sel], (po[sel] // S).astype(np.int32)
    wide = eng.thompson_grad_batch(xs, (ds * S).astype(np.int32), want_prior=True)
    R1 = dict(R, w=R["w"][:1], eps=R["eps"][:1])
    eng.thompson(S=1, F=F, randoms=R1)
    narrow = eng.thompson_grad_batch(xs, ds, want_prior=True)
    assert all(np.array_equal(a, b) for a, b in zip(wide, narrow))
    # a draw alone (H = 1) against the same draw among three
    load(eng, covar, (comp, cand, vals, rows[2:3]))
    eng.thompson(S=S, F=F, randoms=R)
    k2 = np.nonzero(po // S == 2)[0]
    alone = eng.thompson_grad_batch(x[k2], (po[k2] - 2 * S).astype(np.int32), want_prior=True)
    assert len(k2) > 0 and all(np.array_equal(a, b[k2]) for a, b in zip(alone, base))
    # after the handle held a problem of another padded size
    scramble(eng, 62)
    eng.thompson_grad_batch(np.random.RandomState(1).rand(70, 5), np.arange(70, dtype=np.int32) % 4)
    load(eng, covar, P0)
    eng.thompson(S=S, F=F, randoms=R)
    after = eng.thompson_grad_batch(x, po, want_prior=True)
    assert all(np.array_equal(a, b) for a, b in zip(after, base))


# ---- 7. state ---------------------------------------------------------------------------------------------------------------------------
def test_state(eng):
    covar, N, D, F, S, H = "Matern52", 130, 3, 32, 2, 2
    P0 = problem(N, M, D, H, 700)
    comp, cand, vals, rows = P0
    R = spx.thompson_randoms(np.random.RandomState(7), covar, D, H, N, F, S)
    R2 = spx.thompson_randoms(np.random.RandomState(8), covar, D, H, N, F, S)
    load(eng, covar, P0)
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    ei_before = (eng.best(), eng.ei_mean(), eng.ei_draws())
    x = np.random.RandomState(71).rand(20, D)
    po = (np.arange(20) % (H * S)).astype(np.int32)
    with pytest.raises(ValueError) as ei:                                          # an EI pass holds no paths
        eng.thompson_grad_batch(x, po)
    assert "call spx_thompson first" in str(ei.value)
    assert eng.best() == ei_before[0] and np.array_equal(eng.ei_mean(), ei_before[1])
    eng.set_acquisition(spx.ACQ_PI, 0.25)
    eng.thompson(S=S, F=F, randoms=R)
    held = lambda: ([eng.thompson_path(d, s) for d in range(H) for s in range(S)],            # noqa: E731
                    [eng.thompson_prior(d, s) for d in range(H) for s in range(S)])
    before = held()
    v1 = eng.thompson_grad_batch(x, po, want_prior=True)
    now = held()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], now[0]))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before[1], now[1]))
    assert eng.get_acquisition() == (spx.ACQ_PI, 0.25) and eng.stat("last_ts_paths") == S
    # a refused call leaves the handle as it was
    for bad in (np.full(20, H * S, dtype=np.int32), np.full(20, -1, dtype=np.int32)):
        with pytest.raises(ValueError) as ei:
            eng.thompson_grad_batch(x, bad)
        assert "path_of" in str(ei.value)
    assert all(np.array_equal(a, b) for a, b in zip(eng.thompson_grad_batch(x, po, want_prior=True), v1))
    # a fresh spx_thompson rebuilds alpha: the values follow the new randoms, and come back with the old ones
    eng.thompson(S=S, F=F, randoms=R2)
    v2 = eng.thompson_grad_batch(x, po, want_prior=True)
    f_o, g_o = tgo.value_grad(covar, comp, vals, rows[1], R2, 1, x[3:4], d=1)
    assert po[3] == 3 and np.allclose(v2[0][3], f_o[0], rtol=1e-9, atol=1e-9) and np.allclose(v2[1][3], g_o[0], rtol=1e-7, atol=1e-8)
    assert not np.array_equal(v2[0], v1[0])
    eng.thompson(S=S, F=F, randoms=R)
    assert all(np.array_equal(a, b) for a, b in zip(eng.thompson_grad_batch(x, po, want_prior=True), v1))
    # an EI pass afterwards gives the bits it gave before
    eng.set_acquisition(spx.ACQ_EI, 0.0)
    eng.thompson(S=S, F=F, randoms=R)
    eng.thompson_grad_batch(x, po)
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    assert eng.best() == ei_before[0] and np.array_equal(eng.ei_mean(), ei_before[1]) and np.array_equal(eng.ei_draws(), ei_before[2])
    # whatever drops a pass's results drops the paths and alpha with them
    for drop in (lambda: eng.set_observations(comp, vals), lambda: eng.set_hypers(rows), lambda: eng.set_candidates(cand),
                 lambda: eng.factor(), lambda: eng.ei_run(), lambda: eng.set_acquisition(spx.ACQ_EI, 0.0)):
        load(eng, covar, P0)
        eng.thompson(S=S, F=F, randoms=R)
        assert all(np.array_equal(a, b) for a, b in zip(eng.thompson_grad_batch(x, po, want_prior=True), v1))
        drop()
        with pytest.raises(ValueError) as ei:
            eng.thompson_grad_batch(x, po)
        assert "call spx_thompson first" in str(ei.value)


# ---- 8. special values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("covar", ["Matern52", "ARDSE"])
def test_nan_and_inf_coordinates(eng, covar):
    N, D, F, S, H = 65, 3, 48, 2, 2
    (comp, cand, vals, rows), R = setup(eng, covar, N, D, F, S, H, False, 800)
    x = np.random.RandomState(81).rand(33, D)
    po = (np.arange(33) % (H * S)).astype(np.int32)
    base = eng.thompson_grad_batch(x, po, want_prior=True)
    bad = x.copy()
    bad[5, 1] = np.nan
    bad[17, 0] = np.inf
    got = eng.thompson_grad_batch(bad, po, want_prior=True)
    ok = np.ones(33, dtype=bool)
    ok[[5, 17]] = False
    assert np.all(np.isnan(got[0][~ok])) and np.all(np.isnan(got[1][~ok]))
    assert all(np.array_equal(a[ok], b[ok]) for a, b in zip(got, base))


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    covar, N, D, F, S, H = "Matern52", 65, 3, 16, 2, 2
    (comp, cand, vals, rows), R = setup(eng, covar, N, D, F, S, H, False, 900)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))            # noqa: E731
    big = spx.TS_GRAD_MAX_POINTS
    assert big == 65535
    x = np.zeros((big + 1, D))
    f, g = np.empty(big + 1), np.empty((big + 1, D))
    ref = eng.thompson_grad_batch(cand[:5])
    call = lambda xs, n, fs, gs: eng._lib.spx_thompson_grad_batch(eng._h, xs, None, n, fs, gs, None)     # noqa: E731
    err = lambda: eng._lib.spx_last_error().decode()                            # noqa: E731
    for args, word in (((None, 1, dp(f), dp(g)), "NULL"), ((dp(x), 1, None, dp(g)), "NULL"), ((dp(x), 1, dp(f), None), "NULL"),
                       ((dp(x), 0, dp(f), dp(g)), "P=0"), ((dp(x), -3, dp(f), dp(g)), "P=-3"),
                       ((dp(x), big + 1, dp(f), dp(g)), "P=%d" % (big + 1))):
        assert call(*args) == spx.SPX_ERR_ARG and "spx_thompson_grad_batch" in err() and word in err(), (word, err())
    assert call(dp(x), big, dp(f), dp(g)) == spx.SPX_OK                          # the cap itself runs
    assert np.array_equal(f[:big], np.full(big, f[0]))
    for bad in ([0, 0, 0, 0, H * S], [-1, 0, 0, 0, 0]):
        with pytest.raises(ValueError) as ei:
            eng.thompson_grad_batch(cand[:5], np.array(bad, dtype=np.int32))
        assert "path_of[" in str(ei.value) and "allowed" in str(ei.value)
    with pytest.raises(ValueError):
        eng.thompson_grad_batch(cand[:5, :2])
    now = eng.thompson_grad_batch(cand[:5])
    assert np.array_equal(now[0], ref[0]) and np.array_equal(now[1], ref[1])
    fresh = spx.Engine(0)
    try:
        with pytest.raises(ValueError) as ei:
            fresh.D = D
            fresh.thompson_grad_batch(cand[:5])
        assert "call spx_thompson first" in str(ei.value)
    finally:
        fresh.close()
    multi = spx.MultiEngine([0, 0])
    try:
        with pytest.raises(ValueError) as ei:
            multi.thompson_grad_batch(cand[:5])
        assert "multi-device" in str(ei.value)
    finally:
        multi.close()


# ---- 10. the chooser on the device --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pend", [0, 2])
def test_chooser_refines_the_path(n_pend, golden_dir, tmp_path):
    """The properties of the CPU chooser test, asserted with the ORACLE's value of the proposed point: L-BFGS-B need not follow
    the stand-in's iterates under last-place differences, so nothing here compares trajectories."""
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:300]
    values = np.zeros(grid.shape[0]) + np.nan
    done = np.arange(12)
    values[done] = branin(grid[done, 0], grid[done, 1])
    pend = np.arange(12, 12 + n_pend)
    free = np.arange(12 + n_pend, grid.shape[0])
    arg = "mcmc_iters=3,burnin=4,grid_subset=3,acq=TS,acq_par=64"
    out = {}
    for name, extra in (("plain", ""), ("refine", ",ts_refine=1,loo=1")):
        d = tmp_path / name
        d.mkdir()
        ch = GPEIOptChooser.init(str(d), arg + extra)
        np.random.seed(11)
        job = ch.next(grid, values, np.zeros(grid.shape[0]), free, pend, done)
        out[name] = (job, dict(ch.last_thompson), np.random.get_state(), ch)
    (job0, t0, st0, c0), (job1, t1, st1, c1) = out["plain"], out["refine"]
    try:
        assert isinstance(job0, int) and same_state(st0, st1)                    # the refinement draws no random numbers
        assert all(t1[k] == t0[k] for k in ("draw", "grid_index", "path_min", "features"))
        assert c1.last_loo is not None and c1.last_acq_used == "TS"
        # the oracle's path under the same draw and the same randoms (numpy's generator, replayed)
        rows = c0.hyper_rows()
        np.random.seed(11)
        (tmp_path / "oracle").mkdir()
        c2 = GPEIOptChooser.init(str(tmp_path / "oracle"), arg)
        from tests.ts_grad_helpers import TsGradOracleEngine
        c2._eng = TsGradOracleEngine()
        assert c2.next(grid, values, np.zeros(grid.shape[0]), free, pend, done) == job0
        o = c2._eng
        assert rows.shape[0] == 3
        if t1["refined"]:
            numcand, x = job1
            assert numcand == len(free) and np.all(x >= 0.0) and np.all(x <= 1.0) and np.array_equal(x, t1["x"])
            f_o = o.thompson_grad_batch(x[None, :])[0][0]
            grid_min = float(np.min(o.paths[0, 0]))
            assert f_o <= grid_min + 1e-8 * (1.0 + abs(grid_min))                # no greater than the grid minimum
            assert abs(f_o - t1["value"]) <= 1e-8 * (1.0 + abs(f_o))
            assert t1["value"] < t1["path_min"] + 1e-8 * (1.0 + abs(t1["path_min"]))
        else:
            assert job1 == job0 and np.array_equal(t1["x"], grid[job0])
        assert t1["refined"]                                                     # Branin's sample paths are smooth: the minimum is off the grid
    finally:
        c0._eng.close()
        c1._eng.close()


def test_zz_report():
    for k, v in SHARES.items():
        if v:
            print("%s: largest measured share of its bar over all cases %.4f" % (k, max(v)))
