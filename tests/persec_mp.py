"""50-digit yardstick (mpmath) of the predicted duration of the per-second grid pass, exp(k_t(x, X)' alpha_t + mean_t)
(GPEIperSecChooser.py:452-458; k_cov<MODE 2> of csrc/cov_kernels.hip), in two families.

diag     Observations on cov_mp's lattice in one dimension, row j at 4096 j, length scale 1: every pair is 2^24 apart in r^2,
         past every clamp, so the time model's K is exactly diagonal with a = amp2_t (1 + 1e-6) + noise_t, and
         alpha_j = (ld_j - mean_t) / a.  Candidates come in blocks: block j lies within 460 of observation j and at least 3600
         from every other one, so observation j is the SOLE contributor to its block and
             E = amp2_t k(r^2) (ld_j - mean_t) / a + mean_t,     T = exp(E)
         with k at 50 digits at the exact r^2 = delta^2 (a value of tests/golden/cov_lattice_mp.npz: the offsets are the
         window families' candidates).  Sizes 2, 5, 64, 65, 130: every wave, every lane group g, every r of the 16-row
         accumulator tile, both 64-row blocks of a 128-row chunk, the second chunk and the pad rows up to Np are each the
         sole contributor (or all there is) once.  Candidates 2048 from the nearest observation have E = mean_t exactly.

full     Lattice data of tests/test_gpu_q_cov_yardstick.lattice_ei_problem's recipe (integers over a power of two, length
         scales that are powers of two: r^2 exact), a dense K_t GIVEN as float64 (the library's own, or the host's): alpha is
         solved at 50 digits, the cross terms are taken at the exact r^2, exp at 50 digits.

The budget of the diag family is derived (budget() below), not measured.  In units of eps = 2^-52, per rounding half an eps:
    a = fl(fl(amp2 fl(1 + 1e-6)) + noise)                          1.5
    rinv = a^-1/2: the hardware's reciprocal square root and one step (1 eps), a's error halved   1.75
    rho = fl(ld_j - mean_t)                                        0.5
    gamma = fl(rho rinv), alpha = fl(gamma rinv)                   0.5 + 1.75 each: alpha is within 5 eps
    amp2 c, and its product with alpha                             0.5 each
(every other term of the column sum, of the two shuffles and of the four-way reduction is an exact zero), 6 eps; REL_EPS = 6.5
leaves half an eps for the second-order terms.  The correlation c itself is within cov_mp.CEILING[kind] of cov_mp's unit
u = (1 + s) 2^-52 k + poly 2^-1074, and the two products round absolutely by half of 2^-1074 where they are denormal.  So
    dP = |alpha| amp2 (CEILING u + 2^-1075) + REL_EPS eps |P| + 2^-1075         P = amp2 k alpha
    dE = dP + 2^-53 |E|                                              the sum with the mean
and the result is allowed  T expm1(dE)  +  (EXP_ULPS + 1/2) ulp(T):  dE relative, the exp's own bound, and half an ulp for the
reference's rounding to float64.  EXP_ULPS = 1: the ROCm installation carries no accuracy statement for the device library's exp, so
the bound is the float64 oracle's -- np.exp on the same arguments is measured against mpmath in tests/test_persec_mp.py
(0.60 ulp at worst here, glibc documents < 1) -- rounded up to the whole ulp.

Test code only: nothing in spearmint_amd imports this module, and the diag family's GPU tests read tests/golden/persec_mp.npz
instead of importing mpmath."""
import numpy as np

from tests import cov_mp as cv

DPS = 50
LD = np.longdouble
EPS = LD(2.0) ** -52
DEN = LD(2.0) ** -1074
SEED = 17
SIZES = (2, 5, 64, 65, 130)
AMP2_T = (1.0, 4.0, 0.7)
NOISE_T = (0.01, 0.02, 0.005)
MEAN_T = (0.0, 3.5, -20.0)
DENORMAL_MEAN_T = (-730.0, -738.5, -744.0)      # exp(.) from 8.9e-318 down to two quanta (the denormal case, N = 5)
DENORMAL_N = 5
STEP = 4096.0
FAR = 2048.0
REL_EPS = 6.5
EXP_ULPS = 1.0
PER_BLOCK = 8
# the float64 oracle's own error against the yardstick, pinned by tests/test_persec_mp.py: 1.5 x what was measured there, rounded up
ORACLE_DIAG_CEILING = {"Matern52": 1.1, "Matern32": 1.1, "ARDSE": 1.1}      # in units of budget()
ORACLE_FULL_CEILING = {"Matern52": 2.0e-13, "Matern32": 1.5e-13, "ARDSE": 6.0e-13, "SE": 3.5e-13}    # relative, host K_t, N = 24
FULL_N = (24, 40)
FULL_D = (3, 9)
FULL_M = 96
FULL_COVARS = ("Matern52", "Matern32", "ARDSE", "SE")


def _mp():
    import mpmath
    return mpmath.mp


# ---- the diag family --------------------------------------------------------------------------------------------------------------
def offsets():
    """(mild, window): |delta| of the window families' candidates -- 1/8 ... 8, where every kind's k is an ordinary number,
    and the rest (each kind's denormal window, results that round to 0, both sides of each clamp)."""
    cands = np.unique(np.concatenate([C.ravel() for name, _, C, _ in cv.lattice_problems() if name.startswith("window")]))
    cands = cands[cands > 0.0]
    return cands[cands <= 8.0], cands[cands > 8.0]


def diag_problem(N, denormal=False):
    """(X[N, 1], C[M, 1], owner[M], delta[M], log_durs[N]): block j is PER_BLOCK candidates at X_j +- delta -- the coincident
    one, three mild offsets (one of them <= 1, where no kind's k is below 0.2), four of the windows --, owner j; then three
    candidates FAR from the nearest observation, owner -1.  Log durations are multiples of 1/8 between 5 and 30 in size, of
    either sign, at least 1 away from every mean of MEAN_T; in the denormal case they are -735 + ld / 8 (with
    DENORMAL_MEAN_T: predictions from 1e-315 down through the last quanta to 0)."""
    rs = np.random.RandomState(SEED + N)
    mild, window = offsets()
    near = mild[mild <= 1.0]
    X = STEP * np.arange(N, dtype=np.float64)[:, None]
    ld = np.round(8.0 * rs.uniform(5.0, 30.0, N)) / 8.0 * np.where(rs.rand(N) < 0.5, -1.0, 1.0)
    ld[np.abs(ld + 20.0) < 1.0] = -17.5
    if denormal:
        ld = -735.0 + ld / 8.0
    C, owner, delta = [], [], []
    for j in range(N):
        d = np.concatenate(([0.0, near[(3 * j) % near.size], mild[(5 * j + 1) % mild.size], mild[(11 * j + 7) % mild.size]],
                            window[(np.arange(4) * 97 + 29 * j) % window.size]))
        sign = np.where((np.arange(PER_BLOCK) + j) % 2 == 0, 1.0, -1.0)
        C.extend(X[j, 0] + sign * d)
        owner.extend([j] * PER_BLOCK)
        delta.extend(d)
    for x in (-FAR, X[N // 2, 0] + FAR, X[N - 1, 0] + FAR):
        C.append(x)
        owner.append(-1)
        delta.append(FAR)
    return X, np.array(C)[:, None], np.array(owner), np.array(delta), ld


def time_rows(means=MEAN_T):
    """Time hyper rows [mean_t, noise_t, amp2_t, ls = 1] of the three draws."""
    return np.array([[m, n, a, 1.0] for m, n, a in zip(means, NOISE_T, AMP2_T)])


def objective_rows():
    """The objective's rows: another mean, noise, amplitude and length scale in every draw (its K is diagonal too)."""
    return np.array([[0.2, 0.03, 1.7, 2.0], [-0.4, 0.015, 0.9, 0.5], [1.1, 0.04, 2.3, 4.0]])


def objective_vals(N):
    return np.cos(1.7 * np.arange(N)) + 0.1 * np.arange(N) % 0.7


def diag_reference(kind, N, means=MEAN_T, denormal=False):
    """T[M, 3]: the 50-digit predicted durations rounded to float64."""
    mp = _mp()
    X, C, owner, delta, ld = diag_problem(N, denormal)
    out = np.empty((C.shape[0], len(means)))
    with mp.workdps(DPS):
        f = lambda v: mp.mpf(float(v))      # noqa: E731
        kk = {float(d): cv.corr_mp(kind, float(d) * float(d))[0] for d in np.unique(delta)}
        for h, (mean, noise, amp2) in enumerate(zip(means, NOISE_T, AMP2_T)):
            a = f(amp2) * (1 + f(1e-6)) + f(noise)
            for c in range(C.shape[0]):
                E = f(mean)
                if owner[c] >= 0:
                    E = f(amp2) * kk[float(delta[c])] * (f(ld[owner[c]]) - f(mean)) / a + f(mean)
                out[c, h] = float(mp.exp(E))
    return out


def exponent(fixture, kind, N, means=MEAN_T, denormal=False):
    """(E, alpha, k, u)[M, 3] in extended precision from the covariance fixture (k rounded to float64: 2^-53 relative, far
    inside what the bound forgives -- this is for the SIZE of the bound, the reference itself is diag_reference)."""
    X, C, owner, delta, ld = diag_problem(N, denormal)
    near = owner >= 0
    k, u = cv.lookup(fixture, kind, np.where(near, delta * delta, 0.0))
    k, u = np.where(near, k, 0.0).astype(LD), np.where(near, u, 0.0).astype(LD)
    E, A = [], []
    for mean, noise, amp2 in zip(means, NOISE_T, AMP2_T):
        a = LD(amp2) * (LD(1) + LD(1e-6)) + LD(noise)
        alpha = np.where(near, (ld[np.maximum(owner, 0)].astype(LD) - LD(mean)) / a, LD(0))
        E.append(LD(amp2) * k * alpha + LD(mean))
        A.append(alpha)
    return np.stack(E, axis=1), np.stack(A, axis=1), k, u


def budget(fixture, kind, N, T_ref, means=MEAN_T, quanta=0, denormal=False):
    """The allowed |T - T_ref| [M, 3] (module docstring), in extended precision; quanta: further multiples of 2^-1074."""
    E, alpha, k, u = exponent(fixture, kind, N, means, denormal)
    amp2 = np.array(AMP2_T, dtype=LD)[None, :]
    P = amp2 * k[:, None] * alpha
    dP = np.abs(alpha) * amp2 * (LD(cv.CEILING[kind]) * u[:, None] + DEN / 2) + LD(REL_EPS) * EPS * np.abs(P) + DEN / 2
    dE = dP + EPS / 2 * np.abs(E)
    T = T_ref.astype(LD)
    ulp = np.spacing(T_ref).astype(LD)
    return T * np.expm1(dE) + LD(EXP_ULPS + 0.5) * ulp + quanta * DEN


def diag_fixture():
    out = {}
    for kind in cv.KINDS:
        for N in SIZES:
            out["T_%s_%d" % (kind, N)] = diag_reference(kind, N)
        out["T_%s_denormal" % kind] = diag_reference(kind, DENORMAL_N, DENORMAL_MEAN_T, True)
    return out


# ---- the full family --------------------------------------------------------------------------------------------------------------
def full_problem(covar, N, D, M=FULL_M, seed=29):
    """(X, C, vals, log_durs, rows, trows): integers below 8 over 4 (SE, whose length scales are ones: over 8 at D = 3 and over
    16 at D = 9, so that its K_t is as dense as the others'), coincident candidates, rows far away, three draws.  The time
    draws' length scales 2^e (2^(e+1) in the odd dimensions) and noises 0.1 / 0.01 / 0.0003 amp2_t take cond(K_t) from below
    1e2 to above 1e4; under SE the noise alone does (0.5 / 0.03 / 0.0003)."""
    rs = np.random.RandomState(seed + N + 7 * D)
    den = 4.0 if covar != "SE" else (8.0 if D == 3 else 16.0)
    X = rs.randint(0, 8, (N, D)).astype(np.float64) / den
    C = rs.randint(0, 8, (M, D)).astype(np.float64) / den
    C[::16] = X[rs.randint(0, N, len(C[::16]))]
    C[7::30, 1] += 4096.0
    vals = np.sum((X - 0.8) ** 2, axis=1) + 0.05 * rs.randn(N)
    log_durs = 0.7 * np.sum(X, axis=1) * den / (4.0 * D) + 0.1 * rs.randn(N)
    rows = np.empty((3, 3 + D))
    rows[:, :3] = [[0.3, 0.01, 1.0], [0.1, 0.02, 4.0], [0.5, 0.01, 0.7]]
    rows[:, 3:] = np.array([1.0, 0.5, 2.0])[:, None]
    rows[:, 4::2] *= 2.0
    exps = (-1, 0, 1) if D == 3 else (0, 2, 3)
    ratio = (0.1, 0.01, 3e-4) if covar != "SE" else (0.5, 0.03, 3e-4)
    trows = np.empty((3, 3 + D))
    for d, (mean, amp2) in enumerate(((0.4, 1.3), (-1.5, 0.7), (2.0, 4.0))):
        trows[d, :3] = [mean, ratio[d] * amp2, amp2]
        trows[d, 3:] = 2.0 ** exps[d]
        trows[d, 4::2] *= 2.0
    return X, C, vals, log_durs, rows, trows


def host_kt(covar, X, trow):
    """K_t as the float64 oracle forms it (GPEIperSecChooser.py:445-449)."""
    from oracle import gp_ei_oracle as orc
    with orc.covar(covar):
        return orc.cov(trow[2], trow[3:], X) + trow[1] * np.eye(X.shape[0])


def oracle_time_mean(covar, K, X, C, trow, log_durs):
    """tests/helpers.OracleEngine.get_time_mean's arithmetic on a GIVEN K_t."""
    import scipy.linalg as spla
    from oracle import gp_ei_oracle as orc
    with orc.covar(covar), np.errstate(all="ignore"):
        chol = spla.cholesky(K, lower=True)
        alpha = spla.cho_solve((chol, True), log_durs - trow[0])
        return np.exp(np.dot(orc.cov(trow[2], trow[3:], X, C).T, alpha) + trow[0])


def full_reference(covar, K, X, C, trow, log_durs):
    """The predicted durations as a list of mpf: K (float64, taken exactly) solved at 50 digits, the cross terms amp2_t k at
    the exact r^2 (cov_mp.exact_r2 raises if one is not a float64), exp at 50 digits."""
    mp = _mp()
    ls = np.ones(X.shape[1]) if covar == "SE" else trow[3:]
    r2 = cv.exact_r2(X, C, ls)
    uniq, inv = np.unique(r2, return_inverse=True)
    inv = inv.reshape(r2.shape)
    n = X.shape[0]
    with mp.workdps(DPS):
        f = lambda v: mp.mpf(float(v))      # noqa: E731
        kk = [cv.corr_mp(covar, float(v))[0] for v in uniq]
        Km = mp.matrix([[f(K[i, j]) for j in range(n)] for i in range(n)])
        alpha = mp.lu_solve(Km, mp.matrix([f(v) - f(trow[0]) for v in log_durs]))
        amp2, mean = f(trow[2]), f(trow[0])
        return [mp.exp(amp2 * mp.fsum(kk[inv[j, c]] * alpha[j] for j in range(n)) + mean) for c in range(C.shape[0])]


def rel_error(got, want_mp):
    """max |got - want| / want, at 50 digits."""
    mp = _mp()
    with mp.workdps(DPS):
        return float(max(abs(mp.mpf(float(g)) - w) / w for g, w in zip(got, want_mp)))


if __name__ == "__main__":
    import os
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "persec_mp.npz"), **diag_fixture())
