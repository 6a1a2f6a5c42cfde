"""Shared by the tests of the blocked Cholesky's failure edge (csrc/chol_kernels.hip: diag_block / factor16_mfma and their
five callers): problems whose covariance stops being positive definite at a CHOSEN pivot, their barely positive definite
mirror, LAPACK's verdict on them, an extended-precision factorisation to measure accuracy against, and the option sets that
select each form of the factorisation.  No GPU is needed to import it: tests/test_factor_reference.py holds every table entry
to the reference alone, on the CPU.

The construction.  Row i of a seeded X is copied into row j > i and the draw's noise is -1.5e-6 amp2, so that
K = amp2 (k + 1e-6 I) + noise I has the diagonal amp2 (1 - 0.5e-6).  The Schur complement at pivot j is
-1e-6 amp2 - (0.5e-6 amp2)^2 (A^-1)_ii: negative by ~1e-6 amp2 -- ten orders above rounding -- whenever the leading j x j
block A is positive definite, so dpotrf returns info == j + 1 and the library's 0-based pivot must be j.  The leading block
itself must stay clear of the 0.5e-6 amp2 shift: MIN_LEADING_EIG (forty times the shift) is asserted on every entry.  With
noise = 0 (pd=True) the same pivot is about +2e-6 amp2 and LAPACK succeeds."""
import collections
import contextlib
import re

import numpy as np
import scipy.linalg as spla
from scipy.linalg import lapack

from oracle import gp_ei_oracle as orc

# per covariance: (D of the correlated tables, length scale of a failing draw, factor on X); gp.SE ignores its length scales
BASE = {"Matern52": (4, 0.35, 1.0), "Matern32": (4, 0.35, 1.0), "ARDSE": (4, 0.25, 1.0), "SE": (4, 1.0, 4.0)}
BAD_NOISE = -1.5e-6           # x amp2
MIN_LEADING_EIG = 2e-5        # x amp2: forty times the 0.5e-6 amp2 by which the diagonal is lowered
FAR_LS = 1e12                 # own_pair: the length scale that makes one dimension vanish for one draw

DupProblem = collections.namedtuple("DupProblem", "X vals rows expected pivots covar bad_draws pairs")


def dup_problem(N, D, H, covar, pairs, seed, bad_draws, pd=False, own_pair=False):
    """X[N, D] with row i copied into row j for every (i, j) of `pairs` (i < j), values[N], hyper rows[H, 3 + D]
    ([mean, noise, amp2, ls...]) and the expected spx_not_pd_info() == (lowest failing draw, its pivot).  The rows of
    `bad_draws` get the table's length scale and the noise -1.5e-6 amp2 (pd=True: 0, the barely positive definite mirror,
    expected (-1, -1)); the other rows are ordinary draws with their own length scales, amplitudes and noise.  `pivots`
    maps every failing draw to its pivot: the lowest j of `pairs`.

    own_pair: the k-th bad draw fails at pair k's j instead (pairs are used cyclically) -- pair p is a duplicate in every
    dimension but p, and only its own draw has a length scale (1e12) that makes dimension p vanish."""
    rs = np.random.RandomState(seed)
    _, ls0, xf = BASE[covar]
    X = xf * rs.rand(N, D)
    vals = rs.randn(N)
    pairs = [(int(i), int(j)) for i, j in pairs]
    bad_draws = sorted(int(b) for b in bad_draws)
    assert all(0 <= i < j < N for i, j in pairs) and all(0 <= b < H for b in bad_draws)
    assert not own_pair or (covar != "SE" and len(pairs) <= D)
    for p, (i, j) in enumerate(pairs):
        X[j] = X[i]
        if own_pair:
            X[j, p] = (X[i, p] + 0.5) % 1.0
    rows = np.empty((H, 3 + D))
    for h in range(H):
        amp2 = 0.5 + 1.5 * rs.rand()
        rows[h, 0] = 0.2 * rs.randn()
        rows[h, 1] = amp2 * (1e-3 + 9e-3 * rs.rand())
        rows[h, 2] = amp2
        rows[h, 3:] = ls0 * (0.8 + 0.6 * rs.rand(D))
    pivots = {}
    for k, b in enumerate(bad_draws):
        rows[b, 1] = 0.0 if pd else BAD_NOISE * rows[b, 2]
        rows[b, 3:] = ls0
        if own_pair:
            p = k % len(pairs)
            rows[b, 3 + p] = FAR_LS
            pivots[b] = pairs[p][1]
        else:
            pivots[b] = min(j for _, j in pairs)
    if pd:
        pivots = {}
    expected = (bad_draws[0], pivots[bad_draws[0]]) if pivots else (-1, -1)
    return DupProblem(X, vals, rows, expected, pivots, covar, tuple(bad_draws), tuple(pairs))


def good_rows(p, seed=991):
    """The problem's hyper rows with the failing ones replaced by ordinary draws (the other rows unchanged)."""
    rs = np.random.RandomState(seed)
    rows = p.rows.copy()
    ls0 = BASE[p.covar][1]
    for b in p.bad_draws:
        amp2 = 0.5 + 1.5 * rs.rand()
        rows[b] = np.concatenate(([0.1 * rs.randn(), amp2 * (1e-3 + 9e-3 * rs.rand()), amp2], ls0 * (0.8 + 0.6 * rs.rand(p.X.shape[1]))))
    return rows


def oracle_K(p, h, X=None):
    """The reference's covariance of draw h: amp2 (k + 1e-6 I) + noise I (GPEIChooser.py:186-189)."""
    X = p.X if X is None else X
    _, noise, amp2, ls = orc.unpack_hyper(p.rows[h])
    with orc.covar(p.covar):
        return orc.cov(amp2, ls, X) + noise * np.eye(X.shape[0])


def lapack_info(K):
    """dpotrf's info for the lower triangle of K: 0, or the 1-based order of the leading minor that is not positive definite."""
    _, info = lapack.dpotrf(np.asarray(K, dtype=np.float64), lower=1, clean=1, overwrite_a=0)
    return int(info)


def scipy_minor(K):
    """The number in scipy.linalg.cholesky's "%d-th leading minor of the array is not positive definite" for K."""
    try:
        spla.cholesky(K, lower=True)
    except np.linalg.LinAlgError as ex:
        return minor_in(ex)
    return 0


def minor_in(ex):
    m = re.match(r"\s*(\d+)-th leading minor of the array is not positive definite", str(ex))
    assert m, str(ex)
    return int(m.group(1))


def leading_min_eig(K, j):
    return float(np.linalg.eigvalsh(K[:j, :j])[0]) if j > 0 else np.inf


def check_inputs(p):
    """The two conditions every failing problem must meet, from the reference alone: dpotrf stops at the expected pivot of
    every failing draw, and the leading block in front of it is at least MIN_LEADING_EIG amp2 away from failing earlier."""
    for b, j in p.pivots.items():
        K = oracle_K(p, b)
        info = lapack_info(K)
        assert info == j + 1, (p.covar, p.X.shape[0], p.pairs, b, info, j + 1)
        eig = leading_min_eig(K, j) / p.rows[b, 2]
        assert eig >= MIN_LEADING_EIG, (p.covar, p.X.shape[0], p.pairs, b, eig)
    for h in range(p.rows.shape[0]):
        if h not in p.pivots:
            assert lapack_info(oracle_K(p, h)) == 0, (p.covar, p.X.shape[0], p.pairs, h)


def chol_longdouble(K, y=None):
    """Column Cholesky of K in np.longdouble (x87 extended: 64-bit significand): (L, gamma, alpha, lp) with
    gamma = L^-1 y, alpha = L^-T gamma and lp = -sum log diag L - 0.5 |gamma|^2 (gamma, alpha, lp None without y)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not the x87 extended format on this machine"
    A = np.asarray(K, dtype=np.longdouble)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = A[j:, j] - np.dot(L[j:, :j], L[j, :j])
        assert v[0] > 0, "chol_longdouble: pivot %d is not positive" % j
        L[j:, j] = v / np.sqrt(v[0])
    if y is None:
        return L, None, None, None
    y = np.asarray(y, dtype=np.longdouble)
    gamma = np.zeros(n, dtype=np.longdouble)
    for j in range(n):
        gamma[j] = (y[j] - np.dot(L[j, :j], gamma[:j])) / L[j, j]
    alpha = np.zeros(n, dtype=np.longdouble)
    for j in range(n - 1, -1, -1):
        alpha[j] = (gamma[j] - np.dot(L[j + 1:, j], alpha[j + 1:])) / L[j, j]
    lp = -np.sum(np.log(np.diag(L))) - np.longdouble(0.5) * np.dot(gamma, gamma)
    return L, gamma, alpha, lp


# ---- the forms of the factorisation, each by the options that reach it ----------------------------------------------------
OPTION_DEFAULTS = {"lean_one": -1, "lean_merge": -1, "lean_flow_cov": -1, "lean_flow_cu": -1, "lean_flow_yield": -1,
                   "lean_flow": -1, "lean_ps": -1, "lean_lazy": -1, "lean_zc": -1, "ei_flow": -1, "streams": 1,
                   "step_overlap": -1}
# spx_gp_logprob with at most 32 rows
FORMS = collections.OrderedDict([
    ("a_one_launch", {}),
    ("b_three_launches", {"lean_one": 0}),
    ("c_four_launches", {"lean_one": 0, "lean_merge": 0}),
    ("d_cov_launch", {"lean_flow_cov": 0}),
    ("e_one_per_cu", {"lean_flow_cu": 1}),
    ("f_two_per_cu_yield", {"lean_flow_cu": 0, "lean_flow_yield": 1}),
    ("g_two_per_cu", {"lean_flow_cu": 0, "lean_flow_yield": 0}),
    ("h_step_ps", {"lean_flow": 0, "lean_ps": 1}),
    ("i_step", {"lean_flow": 0, "lean_ps": 0, "lean_lazy": 0}),
    ("j_step2", {"lean_flow": 0, "lean_ps": 0, "lean_lazy": 1}),
    ("k_zc0", {"lean_zc": 0}),
    ("k_zc1", {"lean_zc": 1}),
])
FLOW_FORMS = tuple(k for k, v in FORMS.items() if v.get("lean_flow", -1) != 0)     # k_lean_flow: the hand-offs of one launch
IN_LAUNCH_FORMS = FLOW_FORMS + ("h_step_ps",)                                     # diag_block<true>: atomicCAS / atomicMin
PER_LAUNCH_FORMS = ("i_step", "j_step2")                                          # diag_block<false>: the first writer
OTHER_FORMS = tuple(k for k in FORMS if k != "a_one_launch")


@contextlib.contextmanager
def options(eng, **kw):
    try:
        for k, v in kw.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in kw:
            eng.set_option(k, OPTION_DEFAULTS[k])


# ---- the tables ------------------------------------------------------------------------------------------------------------
FULL_NS = (17, 64, 65, 130, 200, 300)
FULL_JS = (1, 2, 15, 16, 17, 31, 32, 47, 48, 62, 63, 64, 65, 79, 80, 127, 128, 129, 191, 192)
REDUCED_NS = (130, 300)
REDUCED_JS = (1, 16, 17, 63, 64, 65, 129)
OTHER_COVARS = ("Matern32", "ARDSE", "SE")
# Matern52 throughout; the other three at N = 130
REDUCED_TABLE = tuple((N, "Matern52") for N in REDUCED_NS) + tuple((130, c) for c in OTHER_COVARS)


def full_pivots(N):
    return sorted(set(j for j in FULL_JS + (N - 2, N - 1) if 1 <= j < N))


def reduced_pivots(N):
    return sorted(set(j for j in REDUCED_JS + (N - 1,) if 1 <= j < N))


def partners(j):
    """The rows whose copy row j is: the first row, its neighbour, and the last row of the previous 64-block."""
    return sorted(set(i for i in (0, j - 1, 64 * (j // 64) - 1) if 0 <= i < j))


def full_cases(N):
    return [(i, j) for j in full_pivots(N) for i in partners(j)]


def reduced_cases(N):
    """One partner per pivot, taking turns among the three kinds."""
    out = []
    for n, j in enumerate(reduced_pivots(N)):
        ps = partners(j)
        out.append((ps[n % len(ps)], j))
    return out


def case_seed(N, i, j):
    return 7000 + 1000 * (N % 7) + 3 * j + i


def case_problem(N, covar, i, j, H=3, bad_draws=(1,), pd=False):
    return dup_problem(N, BASE[covar][0], H, covar, [(i, j)], case_seed(N, i, j), bad_draws, pd=pd)


# two failing pairs in ONE draw (N = 300): the lower pivot is the answer.  Same 16-row sub-block, different sub-blocks of one
# 64-block (first and a later block column), different block columns.
TWO_PAIRS_N = 300
TWO_PAIRS = ((((0, 33), (5, 38)), 33), (((130, 131), (3, 142)), 131),
             (((0, 5), (17, 50)), 5), (((64, 70), (2, 120)), 70),
             (((1, 70), (69, 200)), 70), (((9, 10), (63, 257)), 10))
# three draws of one batch fail at three different pivots (own_pair): the lowest DRAW is reported, with its own pivot
THREE_PAIRS = ((0, 200), (63, 70), (15, 17))          # k-th bad draw -> j = 200, 70, 17: the lowest draw has the highest pivot
BATCH_HS = (1, 3, 12, 32, 33)


def spread_bad_draws(H):
    """Row 0, the middle and the last row (fewer where H is small)."""
    return sorted(set((0, H // 2, H - 1)))


def batch_problem(H, N=130, covar="Matern52"):
    """Bad draws at row 0, in the middle and at the last row, each failing at its own pivot (N = 130: 129 / 70 / 17)."""
    bad = spread_bad_draws(H)
    pairs = ((0, 129), (63, 70), (15, 17))
    return dup_problem(N, BASE[covar][0], H, covar, pairs[:max(len(bad), 1)], 4100 + H, bad, own_pair=True)
