"""numpy / scipy restatement of the Thompson-sampling contract of include/spx.h (spx_thompson): pathwise conditioning of a
random-Fourier-feature prior sample on the exact posterior update.  From the same base randoms
(spearmint_amd.engine.thompson_randoms) it forms what the library forms, operation for operation where the contract fixes
one (frequencies, phase reduction, scale, sig, the right-hand sides); the dot products, the cosine and the solves are numpy's
and scipy's own, so the comparison with the device is at a derived bound, not bit for bit.  No engine, no GPU."""
import numpy as np
import scipy.linalg as spla

from oracle import gp_ei_oracle as orc

TWO_PI = 6.283185307179586          # include/spx.h: TWO_PI == 2 * np.pi
TWO_NU = {"Matern52": 5.0, "Matern32": 3.0}
LD = np.longdouble
COS_ULPS = 4                        # csrc/ts_device.h: SPX_TS_COS_ULPS


def frequencies(covar, row, omega_z, chi):
    """nu (F, D) in turns for one hyper row [mean, noise, amp2, ls...]: (omega_z t_f) / (TWO_PI ls), one rounding each."""
    omega_z = np.asarray(omega_z, dtype=np.float64)
    ls = np.ones(omega_z.shape[1]) if covar == "SE" else np.asarray(row[3:], dtype=np.float64)
    if covar in TWO_NU:
        t = np.sqrt(TWO_NU[covar] / np.asarray(chi, dtype=np.float64))
    else:
        t = np.ones(omega_z.shape[0])
    return (omega_z * t[:, None]) / (TWO_PI * ls)[None, :]


def phases(nu, phase, X):
    """r (n, F): u = X nu^T + phase reduced by r = u - rint(u) (exact)."""
    u = np.dot(np.asarray(X, dtype=np.float64), nu.T) + np.asarray(phase)[None, :]
    with np.errstate(invalid="ignore"):
        return u - np.rint(u)


def cos2pi(r):
    """cos(2 pi r) of a reduced phase, evaluated in long double and rounded once."""
    two_pi = LD(2) * LD("3.14159265358979323846264338327950288")
    return np.cos(two_pi * np.asarray(r).astype(LD)).astype(np.float64)


def features(nu, phase, X):
    return cos2pi(phases(nu, phase, X))


def scale_of(row, F):
    return np.sqrt((2.0 * np.float64(row[2])) / np.float64(F))


def sig_of(row):
    return np.sqrt(np.float64(row[1]) + 1e-6 * np.float64(row[2]))


def prior(row, w, c):
    """p (S, n) = scale (sum_f w[s][f] c[x][f])."""
    return scale_of(row, c.shape[1]) * np.dot(np.asarray(w, dtype=np.float64), c.T)


def draw_randoms(randoms, d, per_draw):
    """(w (S, F), eps (S, N)) of draw d."""
    return (randoms["w"][d], randoms["eps"][d]) if per_draw else (randoms["w"], randoms["eps"])


def rhs_of(row, vals, p_obs, eps):
    """rhs (S, N) = (y - p(X)) - sig eps."""
    return (np.asarray(vals)[None, :] - p_obs) - sig_of(row) * np.asarray(eps)


def paths(covar, comp, cand, vals, row, randoms, d=0, per_draw=False, parts=False):
    """The S sample paths (S, M) of draw `row` over cand, the reference's route for the update (scipy's Cholesky and
    cho_solve on the chooser covariance amp2 (k + 1e-6 I) + noise I).  parts=True: also (prior_cand, prior_obs, rhs)."""
    mean, noise, amp2, ls = orc.unpack_hyper(row)
    w, eps = draw_randoms(randoms, d, per_draw)
    nu = frequencies(covar, row, randoms["omega_z"], randoms["chi"])
    p_obs = prior(row, w, features(nu, randoms["phase"], comp))
    p_cand = prior(row, w, features(nu, randoms["phase"], cand))
    rhs = rhs_of(row, vals, p_obs, eps)
    with orc.covar(covar):
        K = orc.cov(amp2, ls, comp) + noise * np.eye(comp.shape[0])
        Ks = orc.cov(amp2, ls, comp, cand)
    L = spla.cholesky(K, lower=True)
    alpha = spla.cho_solve((L, True), (rhs - mean).T)            # (N, S)
    out = (np.dot(Ks.T, alpha).T + mean) + p_cand
    return (out, p_cand, p_obs, rhs) if parts else out


def np_argmin(path):
    """numpy's rule: the first NaN wins, else the first minimum."""
    return int(np.argmin(path))


def feature_kernel(covar, row, omega_z, chi, phase, x1, x2):
    """amp2 (2 / F) sum_f c_f(x) c_f(x'): what the prior's covariance is for a given set of features."""
    nu = frequencies(covar, row, omega_z, chi)
    c1, c2 = features(nu, phase, x1), features(nu, phase, x2)
    return np.float64(row[2]) * (2.0 / c1.shape[1]) * np.dot(c1, c2.T)


def prior_bound(row, w, nu, phase, X, Dp, c):
    """The derived bound of the device's prior against this oracle's, per (s, row):
    |dp| <= scale sum_f |w_f| (2 pi (Dp + 3) 2^-53 (sum_j |nu_j x_j| + 1) + eps_cos) + 2^-53 (F + 1) scale sum_f |w_f c_f|:
    the dot product of Dp terms plus the phase and the reduction move u by at most (Dp + 3) half-ulps of the magnitudes
    summed, the cosine's slope is at most 2 pi, eps_cos = COS_ULPS 2^-53 is ts_device.h's budget (|c| <= 1), and the sum over F
    features plus the scaling is (F + 1) roundings of the magnitudes summed."""
    u = 2.0 ** -53
    F = nu.shape[0]
    mag = np.dot(np.abs(np.asarray(X, dtype=np.float64)), np.abs(nu).T) + 1.0           # (n, F)
    per_f = 2 * np.pi * (Dp + 3) * u * mag + COS_ULPS * u
    aw = np.abs(np.asarray(w, dtype=np.float64))
    sc = scale_of(row, F)
    return sc * np.dot(aw, per_f.T) + u * (F + 1) * sc * np.dot(aw, np.abs(c).T)
