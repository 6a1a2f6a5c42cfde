"""Shared by the tests that hold what spx_draw_fantasies forms (csrc/fantasy_kernels.hip: k_fant_posterior<TILED>, k_fant_fill) -- the
posterior mean of the pending points pend_m, pend_K = L_S L_S^T - noise I, its Cholesky factor C, T = L_S^-1 C, the fantasies
C z + pend_m, bests and the tail rows T z of Gamma -- to a long-double yardstick: the yardstick of the two kernels alone
(posterior_longdouble, on the bottom rows of a factor and gamma taken as exact inputs), the yardstick of the whole chain from K
and K* to the conditional mean of every candidate under every fantasy (chain_longdouble), two float64 reference chains whose
own error against it is the unit of the bar (chain_reference_route: dpotrf, hostgp.fantasize_from_factor_rows, cho_solve of
its own fantasies, K*^T alpha + mean; chain_as_built: dpotrf, tests/fantasy_helpers.factored_form, W = dtrtri(L), beta = W K*,
beta^T Gamma + mean), the seeded problems and the table of cases tests/test_gpu_s_fantasy_yardstick.py runs.  It imports neither
the engine nor mpmath and needs no GPU: tests/test_fantasy_ld.py holds both long-double functions to 40 digits and qualifies
every problem of the table on the CPU.  Both yardsticks compute in double words of np.longdouble (a pair hi + lo, about 128
bits; the section below says why a single long double does not do) and round each result to one long double at the end.

Units.  The fantasies of one draw are counted relative to max |pend_fant - pend_m| + max |pend_m| of the yardstick (the two
terms of the sum that forms them), pend_m relative to the same, C relative to max |C|, Gamma's tail relative to max |T z|, and
the conditional mean m_s[c] = B[:, c]^T Gamma_s + mean relative to s_m = |B[:, c]|_2 |Gamma_s|_2 + |mean| as in
tests/moments_ld.py.  The chain takes z as the exact input, not the rounded fantasies: a reference that re-solved
L_S^-1 (pend_fant - ...) from rounded fantasies would count input rounding, amplified by L_S^-1, as device error."""
import collections

import numpy as np
import scipy.linalg as spla
from scipy.linalg import lapack

from spearmint_amd import hostgp
from tests import fantasy_helpers as fh

LD = np.longdouble
D, H = 4, 3
BANDS = (None, 1e-9, 1.0)        # noise / amp2 of draw 0, 1, 2 (None: as drawn, 1e-4 ... 1e-2); noise = amp2 is where
                                 # L_S L_S^T - noise I cancels hardest
NEAR_OBS, NEAR_PEND = 1e-4, 1e-5
SPECIAL_K = 5                    # candidates on pending points, as many 1e-9 beside them, as many on observations
FAR = 3                          # candidates with every coordinate 1e3: their K* column is exactly zero
FAR_COORD = 1e3
NEAR_STEP = 1e-9
M_CAND = 48
S_MAX = 33

Posterior = collections.namedtuple("Posterior", "pend_m pend_K C T pend_fant tail min_pivot")
Chain = collections.namedtuple("Chain", "m s_m post gamma")
Problem = collections.namedtuple("Problem", "comp pend vals rows covar z cand n_pend_cand n_far")


# ---- double-word arithmetic in np.longdouble ------------------------------------------------------------------------------------
# A value is a pair (hi, lo) of np.longdouble arrays with |lo| <= ulp(hi) / 2, about 128 significant bits.  Every operation
# below is np.longdouble arithmetic: error-free transformations (TwoSum, Veltkamp's split at 2^32 + 1, Dekker's TwoProduct; the
# x87 format rounds every operation to its 64-bit significand, which is all they need) and the double-word sum, product,
# quotient and square root made of them.  Why a plain long double is not enough: L_S L_S^T - noise I cancels up to six digits
# (noise = amp2 against pivots of 2e-6 amp2), and the map from K to the fantasies is as ill-conditioned wherever two pending
# points are 1e-5 apart, so one rounding at 2^-64 is 2^-64 x 1e6 = 5e-14 in a pivot -- measured against 40 digits, a plain
# long-double restatement of the same steps (with tests/factor_helpers.chol_longdouble for the chain) was off by up to 1.1e-16 in
# C and in m_s, thirty times the 2^-58 the yardstick is held to (tests/test_fantasy_ld.py).
_SPLIT = LD(2.0) ** 32 + LD(1.0)


def _split(a):
    c = _SPLIT * a
    h = c - (c - a)
    return h, a - h


def _fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def dd(a):
    """An exact float64 or long-double array as a double word."""
    a = np.asarray(a).astype(LD)
    return a, np.zeros_like(a)


def dd_add(a, b):
    s, e = _two_sum(a[0], b[0])
    return _fast_two_sum(s, e + (a[1] + b[1]))


def dd_sub(a, b):
    return dd_add(a, (-b[0], -b[1]))


def dd_mul(a, b):
    a1, a2 = _split(a[0])
    b1, b2 = _split(b[0])
    p = a[0] * b[0]
    e = ((a1 * b1 - p) + a1 * b2 + a2 * b1) + a2 * b2
    return _fast_two_sum(p, e + (a[0] * b[1] + a[1] * b[0]))


def dd_div(a, b):
    q1 = a[0] / b[0]
    r = dd_sub(a, dd_mul(b, (q1, np.zeros_like(q1))))
    q2 = r[0] / b[0]
    r = dd_sub(r, dd_mul(b, (q2, np.zeros_like(q2))))
    q3 = r[0] / b[0]
    return dd_add(_fast_two_sum(q1, q2), (q3, np.zeros_like(q3)))


def dd_sqrt(a):
    s = np.sqrt(a[0])
    r = dd_sub(a, dd_mul((s, np.zeros_like(s)), (s, np.zeros_like(s))))
    return _fast_two_sum(s, r[0] / (s + s))


def dd_sum(a, axis):
    """The sum along one axis as a pairwise tree of double-word additions."""
    h, l = np.moveaxis(a[0], axis, -1), np.moveaxis(a[1], axis, -1)
    if h.shape[-1] == 0:
        return np.zeros(h.shape[:-1], dtype=LD), np.zeros(h.shape[:-1], dtype=LD)
    while h.shape[-1] > 1:
        n = h.shape[-1]
        k = n // 2
        sh, sl = dd_add((h[..., :k], l[..., :k]), (h[..., k:2 * k], l[..., k:2 * k]))
        if n % 2:
            sh, sl = np.concatenate((sh, h[..., -1:]), axis=-1), np.concatenate((sl, l[..., -1:]), axis=-1)
        h, l = sh, sl
    return h[..., 0], l[..., 0]


def dd_matmul(a, b):
    """a (m, k) times b (k, n)."""
    prod = dd_mul((a[0][:, :, None], a[1][:, :, None]), (b[0][None, :, :], b[1][None, :, :]))
    return dd_sum(prod, 1)


def dd_cholesky(a, what):
    """Column Cholesky of a double-word matrix: (L, the pivots' high words)."""
    n = a[0].shape[0]
    lh, ll = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    piv = np.zeros(n, dtype=LD)
    for j in range(n):
        dot = dd_sum(dd_mul((lh[j:, :j], ll[j:, :j]), (lh[j:j + 1, :j], ll[j:j + 1, :j])), 1)
        v = dd_sub((a[0][j:, j], a[1][j:, j]), dot)
        assert v[0][0] > 0, "%s: pivot %d is not positive" % (what, j)
        piv[j] = v[0][0]
        r = dd_sqrt((v[0][:1], v[1][:1]))
        lh[j:, j], ll[j:, j] = dd_div(v, r)
        lh[j, j], ll[j, j] = r[0][0], r[1][0]
    return (lh, ll), piv


def dd_forward(l, b):
    """L^-1 b for a lower triangular double-word L and b (n, m), one row at a time."""
    n = l[0].shape[0]
    xh, xl = np.zeros_like(b[0]), np.zeros_like(b[1])
    for i in range(n):
        dot = dd_sum(dd_mul((l[0][i, :i, None], l[1][i, :i, None]), (xh[:i], xl[:i])), 0)
        xh[i], xl[i] = dd_div(dd_sub((b[0][i], b[1][i]), dot), (l[0][i, i], l[1][i, i]))
    return xh, xl


# ---- the yardstick of the two kernels ----------------------------------------------------------------------------------------
def _posterior_dd(n, mean, noise, l_rows, gamma, z):
    """The steps of posterior_longdouble on double words: (pend_m, pend_K, C, T, pend_fant, tail, smallest pivot)."""
    p = l_rows[0].shape[0]
    tri = np.tril(np.ones((p, p), dtype=LD))
    l21 = (l_rows[0][:, :n], l_rows[1][:, :n])
    ls_ = (l_rows[0][:, n:n + p] * tri, l_rows[1][:, n:n + p] * tri)
    g = (gamma[0][:n, None], gamma[1][:n, None])
    pm = dd_add(dd_matmul(l21, g), (mean[0].reshape(1, 1), mean[1].reshape(1, 1)))            # (p, 1)
    eye = np.eye(p, dtype=LD)
    pend_k = dd_sub(dd_matmul(ls_, (ls_[0].T, ls_[1].T)), (noise[0] * eye, noise[1] * eye))
    c, piv = dd_cholesky(pend_k, "posterior_longdouble: pend_K")
    t = dd_forward(ls_, c)
    fant = dd_add(dd_matmul(c, z), pm)
    return pm, pend_k, c, t, fant, dd_matmul(t, z), piv.min()


def posterior_longdouble(vals, mean, noise, l_rows, gamma, z):
    """Everything k_fant_posterior and k_fant_fill form, in np.longdouble (double words, above), from the bottom P rows of the
    factor (P x n, n = N + P), gamma (its first N entries are read), mean, noise and z (P x S) as exact inputs:
    pend_m = L21 gamma[:N] + mean, pend_K = tril(L_S) tril(L_S)^T - noise I, its column Cholesky C, T = L_S^-1 C by forward
    substitution, pend_fant = C z + pend_m and Gamma's tail T z, each rounded to one long double at the end; min_pivot is the
    smallest pivot of the Cholesky (a square of C's diagonal)."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is not the x87 extended format on this machine"
    n = np.asarray(vals).shape[0]
    pm, pend_k, c, t, fant, tail, piv = _posterior_dd(n, dd(mean), dd(noise), dd(l_rows), dd(gamma), dd(z))
    return Posterior(pm[0][:, 0], pend_k[0], c[0], t[0], fant[0], tail[0], piv)


def fant_unit(post):
    """max |pend_fant - pend_m| + max |pend_m| of one draw's yardstick."""
    return np.max(np.abs(post.pend_fant - post.pend_m[:, None])) + np.max(np.abs(post.pend_m))


def fant_error(got, post):
    """max |got - pend_fant| in units of fant_unit, evaluated in long double."""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - post.pend_fant)) / fant_unit(post))


def tail_error(got, post):
    """max |got - T z| relative to max |T z|."""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - post.tail)) / np.max(np.abs(post.tail)))


def lapack_form(vals, mean, noise, l_rows, gamma, z):
    """(pend_fant, Gamma's tail) of hostgp.fantasize_from_factor_rows; the tail is what the reference's route makes of its own
    fantasies, L_S^-1 (pend_fant - mean - L21 gamma[:N]) by dtrtrs."""
    n, p = vals.shape[0], l_rows.shape[0]
    fant, _ = hostgp.fantasize_from_factor_rows(vals, np.array([mean, noise]), l_rows, gamma, z)
    pf = fant[n:]
    rhs = pf - mean - np.dot(l_rows[:, :n], gamma[:n])[:, None]
    return pf, spla.solve_triangular(np.tril(l_rows[:, n:n + p]), rhs, lower=True)


def built_form(vals, mean, noise, l_rows, gamma, z):
    """(pend_fant, Gamma's tail) of tests/fantasy_helpers.factored_form, the algorithm as built."""
    n = vals.shape[0]
    pf, _, big = fh.factored_form(vals, mean, noise, l_rows, gamma, z)
    return pf, big[n:]


# ---- the yardstick of the chain and the two float64 chains -------------------------------------------------------------------
def chain_longdouble(K, Ks, vals, mean, noise, prior_v, z, P):
    """From K ((N + P)^2), K* ((N + P) x M), vals (N), mean, noise and z (P x S) as exact inputs, in double words throughout: the
    column Cholesky of K (the algorithm of tests/factor_helpers.chol_longdouble), gamma, the posterior above from that factor's
    bottom rows, Gamma_s = [gamma[:N]; T z_s], B = L^-1 K* and, per fantasy column, m_s = B^T Gamma_s + mean with its unit
    s_m = |B[:, c]|_2 |Gamma_s|_2 + |mean|: Chain(m (S, M), s_m (S, M), the Posterior, gamma), rounded to one long double at the end.
    prior_v is the added term of the variance the same B gives (prior_v - sum B^2 is tests/moments_ld.py's business); it is
    converted and otherwise unused."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is not the x87 extended format on this machine"
    N = np.asarray(vals).shape[0]
    y = dd_sub(dd(np.concatenate((np.asarray(vals, dtype=np.float64), np.zeros(P)))), dd(np.float64(mean)))
    y[0][N:], y[1][N:] = 0, 0                                                      # the placeholders: gamma[:N] does not read them
    L, _ = dd_cholesky(dd(np.asarray(K, dtype=np.float64)), "chain_longdouble: K")
    gamma = dd_forward(L, (y[0][:, None], y[1][:, None]))
    gamma = gamma[0][:, 0], gamma[1][:, 0]
    mean_dd, _ = dd(np.float64(mean)), LD(np.float64(prior_v))
    pm, pend_k, c, t, fant, tail, piv = _posterior_dd(N, mean_dd, dd(np.float64(noise)), (L[0][N:], L[1][N:]), gamma, dd(z))
    post = Posterior(pm[0][:, 0], pend_k[0], c[0], t[0], fant[0], tail[0], piv)
    B = dd_forward(L, dd(np.asarray(Ks, dtype=np.float64)))
    S = tail[0].shape[1]
    big = (np.concatenate((np.tile(gamma[0][:N, None], (1, S)), tail[0])),
           np.concatenate((np.tile(gamma[1][:N, None], (1, S)), tail[1])))             # (n, S)
    m = dd_add(dd_matmul((big[0].T, big[1].T), B), (mean_dd[0].reshape(1, 1), mean_dd[1].reshape(1, 1)))
    s_m = np.sqrt(np.sum(big[0] * big[0], axis=0))[:, None] * np.sqrt(np.sum(B[0] * B[0], axis=0))[None, :] + abs(mean_dd[0])
    return Chain(m[0], s_m, post, gamma[0])


def chain_error(got, chain):
    """max over fantasy columns and candidates of |got - m_s| / s_m; got is (S, M)."""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - chain.m) / chain.s_m))


def _dpotrf(K):
    L, info = lapack.dpotrf(np.asarray(K, dtype=np.float64), lower=1, clean=1, overwrite_a=0)
    assert info == 0, "dpotrf info %d" % info
    return L


def chain_reference_route(K, Ks, vals, mean, noise, z, P):
    """m (S, M) by the reference program's route: dpotrf, hostgp.fantasize_from_factor_rows, cho_solve of
    [vals; its own fantasies] - mean, K*^T alpha + mean."""
    N = vals.shape[0]
    L = _dpotrf(K)
    gamma = spla.solve_triangular(L, np.concatenate((vals, np.full(P, mean))) - mean, lower=True)
    fant, _ = hostgp.fantasize_from_factor_rows(vals, np.array([mean, noise]), L[N:], gamma, z)
    alpha = spla.cho_solve((L, True), fant - mean)
    return (np.dot(Ks.T, alpha) + mean).T


def chain_as_built(K, Ks, vals, mean, noise, z, P):
    """m (S, M) by the algorithm as built: dpotrf, tests/fantasy_helpers.factored_form, W = dtrtri(L), beta = W K*,
    beta^T Gamma + mean.  Reads nothing of the library."""
    N = vals.shape[0]
    L = _dpotrf(K)
    W, info = lapack.dtrtri(L, lower=1, unitdiag=0, overwrite_c=0)
    assert info == 0, "dtrtri info %d" % info
    W = np.tril(W)
    gamma = np.dot(W, np.concatenate((vals, np.full(P, mean))) - mean)
    _, _, big = fh.factored_form(vals, mean, noise, L[N:], gamma, z)
    return (np.dot(np.dot(W, Ks).T, big) + mean).T


# ---- the problems ------------------------------------------------------------------------------------------------------------
def problem(N, P, covar, seed):
    """In the style of tests/fantasy_helpers.host_problems, at D = 4 with H = 3 draws: pend[0] = comp[min(3, N - 1)] + 1e-4;
    pend[1] = pend[2] + 1e-5 when P > 2; the last pending point exactly ON comp[0] when P > 1, and with P = 1 the one point
    is on comp[0] where N is odd and 1e-4 beside an observation where it is even.  Draw 0 keeps the noise as drawn
    (1e-4 ... 1e-2 amp2), draw 1 has noise = 1e-9 amp2 and draw 2 noise = amp2.  z is (H, P, S_MAX): a case reads its first S columns,
    and z[0] is the shared array.
    The candidates of the chain (M_CAND rows): k = min(5, P) on pending points, k more 1e-9 beside them, five (at most N) on
    observations, the last three at 1e3 in every coordinate, seeded uniform ones between."""
    rs = np.random.RandomState(seed)
    comp, pend = rs.rand(N, D), rs.rand(P, D)
    vals = np.sin(3 * comp).sum(axis=1) + 0.01 * rs.randn(N)
    rows = np.empty((H, 3 + D))
    for h in range(H):
        amp2 = np.exp(0.5 * rs.randn())
        frac = 10.0 ** rs.uniform(-4, -2)
        rows[h] = np.concatenate(([vals.mean(), (frac if BANDS[h] is None else BANDS[h]) * amp2, amp2], rs.uniform(0.3, 2.0, D)))
    z = rs.randn(H, P, S_MAX)
    cand = rs.rand(M_CAND, D)
    if P > 1:
        pend[P - 1] = comp[0]
    if P > 2:
        pend[1] = pend[2] + NEAR_PEND
    if P > 1 or N % 2 == 0:
        pend[0] = comp[min(3, N - 1)] + NEAR_OBS
    else:
        pend[0] = comp[0]
    k = min(SPECIAL_K, P)
    cand[:k] = pend[P - k:]
    cand[k:2 * k] = pend[P - k:] + NEAR_STEP
    n_obs = min(SPECIAL_K, N)
    cand[2 * k:2 * k + n_obs] = comp[:n_obs]
    cand[M_CAND - FAR:] = FAR_COORD
    return Problem(comp, pend, vals, rows, covar, z, cand, k, FAR)


def far_columns(p):
    M = p.cand.shape[0]
    return np.arange(M - p.n_far, M)


def prior_v_of(row):
    return float(np.float64(row[2]) * (1 + 1e-6))


def z_of(p, h, S, per_draw):
    """The (P, S) normals of draw h."""
    return np.ascontiguousarray((p.z[h] if per_draw else p.z[0])[:, :S])


def host_inputs(p, h):
    """(K, K*, the host factor's bottom rows, gamma) of draw h from spearmint_amd.hostgp alone."""
    row = p.rows[h]
    cp = np.concatenate((p.comp, p.pend))
    K = hostgp.obs_cov(row[2], row[1], row[3:], cp, p.covar)
    Ks = row[2] * hostgp.corr(p.covar, row[3:], cp, p.cand)
    chol, gamma = fh.host_factor(p.comp, p.pend, p.vals, row, p.covar)
    return K, Ks, chol[p.comp.shape[0]:], gamma


# ---- the table of tests/test_gpu_s_fantasy_yardstick.py ----------------------------------------------------------------------
#   (N completed, P, covar, S, per_draw): the smallest sizes at which the kernels change path -- P = n - 1 (5, 4); pending rows that
#   straddle the factor's 64-row tiles 0 / 1 (60, 7), (62, 4) and row 128 (100, 64), so that L_S has entries in an off-diagonal
#   tile; L_S a whole diagonal tile (64, 64); the strided loops of the in-LDS Cholesky and the per-thread column solve up to
#   P = 64; S either side of FANT_COLS = 16
CASES = (
    (1, 1, "Matern52", 1, 0), (2, 1, "Matern52", 15, 1), (5, 4, "Matern52", 16, 0), (60, 7, "Matern52", 17, 1),
    (62, 4, "Matern52", 33, 0), (63, 1, "Matern52", 16, 1), (64, 1, "Matern52", 17, 0), (64, 64, "Matern52", 15, 1),
    (100, 64, "Matern52", 33, 0), (127, 3, "Matern52", 1, 1), (128, 16, "Matern52", 16, 0), (130, 63, "Matern52", 17, 1),
    (130, 63, "ARDSE", 15, 0), (130, 63, "Matern32", 33, 1), (190, 64, "Matern52", 16, 1), (257, 33, "Matern52", 17, 0),
)
CHAIN_CASES = ((60, 7, "Matern52"), (64, 64, "Matern52"), (100, 64, "Matern52"), (130, 63, "Matern52"), (257, 33, "Matern52"))
CHAIN_S = 3                                     # fantasy columns of a chain case (the first three of the problem's z)
CHAIN_STORAGE = (130, 63, "Matern52")           # the chain case run under both storage forms of the factor
UNIT_COLUMN_PS = (1, 7, 16, 63, 64)             # z = [0 | 2^40 I_P]; N = 70 completed
UNIT_COLUMN_N = 70
SEEDS = {}                                      # (N, P, covar) -> seed, where the default does not qualify


def key_of(case):
    return tuple(case[:3])


def seed_of(key):
    N, P, covar = key
    return SEEDS.get(key, 7300 + 11 * N + P + 1000 * (("Matern52", "ARDSE", "Matern32").index(covar)))


def case_problem(case):
    """The problem of a row of CASES or CHAIN_CASES: one per (N, P, covar)."""
    N, P, covar = key_of(case)
    return problem(N, P, covar, seed_of((N, P, covar)))


def unit_column_problem(P):
    """N = 70 completed and P pending with z = [0 | 2^40 I_P] for every draw."""
    p = problem(UNIT_COLUMN_N, P, "Matern52", seed_of((UNIT_COLUMN_N, P, "Matern52")))
    z = np.concatenate((np.zeros((P, 1)), 2.0 ** 40 * np.eye(P)), axis=1)
    return p._replace(z=np.stack([z] * H))


def case_id(case):
    return "-".join(str(x) for x in case)
