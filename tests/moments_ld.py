"""Shared by the tests that hold the posterior moments -- func_m = beta^T gamma + mean and func_v = prior_v - sum beta^2, the two
numbers per candidate that W = L^-1 (k_trinv), beta = W K* (k_predict_gemm*, k_ei_fused128), the epilogue's sums and
k_ei_finalize produce -- to a long-double yardstick: the yardstick itself (moments_longdouble), two float64 reference
algorithms whose own error against it is the unit of the bar (moments_lapack: the reference's route, GPEIChooser.py:195-199
as oracle/gp_ei_oracle.compute_ei restates it; moments_as_built: DESIGN.md section 2's algorithm in plain numpy), the seeded
problems, and the table of cases tests/test_gpu_q_moments_yardstick.py runs.  It imports neither the engine nor mpmath and
needs no GPU: tests/test_moments_ld.py holds the yardstick to 40 digits and qualifies every problem of the table on the CPU.

Units.  Every function takes K (N x N), K* (N x M), y = vals - mean, mean and prior_v as EXACT float64 inputs (prior_v is the
double amp2 * (1 + 1e-6) of the library's hyper table, converted, not recomputed).  An error of func_m is counted relative
to s_m[c] = |B[:, c]|_2 |gamma|_2 + |mean| -- the Cauchy-Schwarz bound of the dot product plus the added mean: a relative error
of func_m itself would be unbounded where it crosses zero -- and an error of func_v relative to s_v = prior_v, the term that
cancels: at a candidate that lies on an observation func_v is 1e-6 prior_v, and an error of 1e-11 there in units of func_v
is 1e-17 in units of what was computed."""
import collections

import numpy as np
import scipy.linalg as spla
from scipy.linalg import lapack

from spearmint_amd.synthetic import synthetic_problem
from tests.factor_helpers import chol_longdouble

LD = np.longdouble
BANDS = {"a": None, "b": 1e-6, "c": 1e-9}        # noise / amp2 of every draw (a: the sampled noise, as drawn)
SPECIAL_K = 5                                    # candidates on an observation, and as many 1e-9 beside one
FAR = 3                                          # candidates with every coordinate 1e3: their K* column is exactly zero
FAR_COORD = 1e3
NEAR_STEP = 1e-9
MAX_COLUMNS = 300

Ref = collections.namedtuple("Ref", "m v s_m s_v")
Problem = collections.namedtuple("Problem", "comp cand vals rows covar k n_on n_near n_far")


# ---- the yardstick and the two reference algorithms -------------------------------------------------------------------------
def moments_longdouble(K, Ks, y, mean, prior_v):
    """Column Cholesky of K, B = L^-1 K* by forward substitution one row at a time (all candidates at once) and
    gamma = L^-1 y, all in np.longdouble: Ref(m = B^T gamma + mean, v = prior_v - sum B^2, s_m, s_v)."""
    L, gamma, _, _ = chol_longdouble(K, y)
    Ks = np.asarray(Ks, dtype=np.float64)
    n = L.shape[0]
    B = np.zeros((n, Ks.shape[1]), dtype=LD)
    for i in range(n):
        B[i] = (Ks[i].astype(LD) - np.dot(L[i, :i], B[:i])) / L[i, i]
    mean, prior_v = LD(np.float64(mean)), LD(np.float64(prior_v))
    m = np.dot(B.T, gamma) + mean
    ss = np.sum(B * B, axis=0)
    s_m = np.sqrt(ss) * np.sqrt(np.dot(gamma, gamma)) + abs(mean)
    return Ref(m, prior_v - ss, s_m, prior_v)


def moments_lapack(K, Ks, y, mean, prior_v):
    """(func_m, func_v) by the reference's route: dpotrf, cho_solve for alpha, solve_triangular for beta,
    func_m = K*^T alpha + mean, func_v = prior_v - sum beta^2."""
    L, info = lapack.dpotrf(np.asarray(K, dtype=np.float64), lower=1, clean=1, overwrite_a=0)
    assert info == 0, "moments_lapack: dpotrf info %d" % info
    alpha = spla.cho_solve((L, True), y)
    beta = spla.solve_triangular(L, Ks, lower=True)
    return np.dot(Ks.T, alpha) + mean, prior_v - np.sum(beta ** 2, axis=0)


def moments_as_built(K, Ks, y, mean, prior_v):
    """(func_m, func_v) by the algorithm of DESIGN.md section 2 in plain float64 numpy: L by dpotrf, W = L^-1 by dtrtri,
    beta = W K*, gamma = W y, func_m = beta^T gamma + mean, func_v = prior_v - sum beta^2.  Reads nothing of the library."""
    L, info = lapack.dpotrf(np.asarray(K, dtype=np.float64), lower=1, clean=1, overwrite_a=0)
    assert info == 0, "moments_as_built: dpotrf info %d" % info
    W, info = lapack.dtrtri(L, lower=1, unitdiag=0, overwrite_c=0)
    assert info == 0, "moments_as_built: dtrtri info %d" % info
    W = np.tril(W)
    beta = np.dot(W, Ks)
    gamma = np.dot(W, y)
    return np.dot(beta.T, gamma) + mean, prior_v - np.sum(beta ** 2, axis=0)


def errors(got_m, got_v, ref):
    """(max_c |got_m - m_ref| / s_m, max_c |got_v - v_ref| / s_v), evaluated in long double."""
    em = np.abs(np.asarray(got_m).astype(LD) - ref.m) / ref.s_m
    ev = np.abs(np.asarray(got_v).astype(LD) - ref.v) / ref.s_v
    return float(np.max(em)), float(np.max(ev))


# ---- the problems ------------------------------------------------------------------------------------------------------------
def problem(N, M, D, H, band, covar, seed):
    """spearmint_amd.synthetic.synthetic_problem (ten candidates jittered around the incumbent) with three kinds of candidate
    rows written over it, k = min(5, N): rows [0, k) = comp[:k] exactly (a candidate ON an observation: func_v falls to the
    noise level, which is where prior_v - ss cancels), rows [k, 2k) = comp[:k] + 1e-9, the last three rows 1e3 in every
    coordinate (past every correlation's underflow: their K* column is exactly zero).  Where M cannot hold them all they go
    last to first: no far rows below 2k + 3, no near rows below 2k, and the first min(k, M) observations.
    Band a keeps the sampled noise, b sets noise = 1e-6 amp2 and c noise = 1e-9 amp2 in every draw."""
    comp, cand, vals, rows = synthetic_problem(N, M, D, H, seed, near=min(10, M))
    k = min(SPECIAL_K, N)
    n_on = min(k, M)
    n_near = k if M >= 2 * k else 0
    n_far = FAR if M >= 2 * k + FAR else 0
    cand[:n_on] = comp[:n_on]
    if n_near:
        cand[k:2 * k] = comp[:k] + NEAR_STEP
    if n_far:
        cand[M - FAR:] = FAR_COORD
    if BANDS[band] is not None:
        rows[:, 1] = BANDS[band] * rows[:, 2]
    return Problem(comp, cand, vals, rows, covar, k, n_on, n_near, n_far)


def far_columns(p):
    M = p.cand.shape[0]
    return np.arange(M - p.n_far, M)


def prior_v_of(row):
    """amp2 * (1 + 1e-6) as spx_set_hypers forms it (one float64 product with the rounded constant)."""
    return float(np.float64(row[2]) * (1 + 1e-6))


def yardstick_columns(M):
    """The candidates whose moments are held to the yardstick: all of them up to 300; beyond, a fixed sorted set of at most 300 with
    every edge of a 128-candidate tile (0, 127, 128, 255, 256, every multiple of 128 and the column in front of it), M - 1,
    the special rows of problem() (the first ten and the last three) and a seeded random fill."""
    if M <= MAX_COLUMNS:
        return np.arange(M)
    keep = {0, 127, 128, 255, 256, M - 1}
    for c in range(128, M, 128):
        keep.update((c - 1, c))
    keep.update(range(2 * SPECIAL_K))
    keep.update(range(M - FAR, M))
    keep = sorted(c for c in keep if 0 <= c < M)
    rest = np.setdiff1d(np.arange(M), keep)
    fill = np.random.RandomState(4242 + M).permutation(rest)[:MAX_COLUMNS - len(keep)]
    return np.sort(np.concatenate((np.array(keep, dtype=np.int64), fill)))


# ---- the table of tests/test_gpu_q_moments_yardstick.py ---------------------------------------------------------------------
D, H, M_DEFAULT = 4, 3, 300
FUSED_NS = (2, 16, 17, 96, 127, 128)                   # k_ei_fused128
ONE_BLOCK_TAIL_NS = (16, 17, 33, 65, 96)               # ei_fused=0: k_predict_gemm_tail<1, 1, 2, 3, 3> alone
ONE_BLOCK_PADDED_NS = (97, 128)                        # ei_fused=0: k_predict_gemm_tri, one row block
TWO_BLOCK_TAIL_NS = (129, 145, 161, 177, 193, 224)     # 1 ... 6 live tiles in the tail kernel + tri
TWO_BLOCK_PADDED_NS = (225, 256)
THREE_BLOCK_NS = (257, 300, 353, 384)                  # tail with 1 and 3 live tiles; padded; full
NOT_SKIPPED_NS = (129, 300)                            # gemm_partial=0
FACTOR_STORAGE_NS = (130, 300)                         # ei_flow=0
VARIANT_NS = (130, 300)
VARIANTS = (4, 8, 14, 18, 24, 32)                      # gemm_waves
TILE_N, TILE_MS = 130, (1, 129, 1100)                  # 1, 2 and 9 candidate tiles
CHUNK_N, CHUNK_M = 130, 1100
STEP_NS = (128, 177)
ARDSE_CASES = ((130, "c"), (300, "b"))
SEEDS = {}                                             # (N, M, band, covar) -> seed, where the default does not qualify


def key_of(N, band, M=M_DEFAULT, covar="Matern52"):
    return (N, M, band, covar)


def seed_of(key):
    N, M, band, covar = key
    return SEEDS.get(key, 8100 + 7 * N + M % 13 + (covar != "Matern52"))


def table_problem(key):
    N, M, band, covar = key
    return problem(N, M, D, H, band, covar, seed_of(key))


def table_keys():
    """Every problem the GPU file runs, once."""
    ns = sorted(set(FUSED_NS + ONE_BLOCK_TAIL_NS + ONE_BLOCK_PADDED_NS + TWO_BLOCK_TAIL_NS + TWO_BLOCK_PADDED_NS
                    + THREE_BLOCK_NS + NOT_SKIPPED_NS + FACTOR_STORAGE_NS + VARIANT_NS + STEP_NS + (TILE_N, CHUNK_N)))
    keys = [key_of(N, band) for N in ns for band in sorted(BANDS)]
    keys += [key_of(TILE_N, band, M=M) for M in TILE_MS for band in sorted(BANDS)]
    keys += [key_of(N, band, covar="ARDSE") for N, band in ARDSE_CASES]
    return keys
