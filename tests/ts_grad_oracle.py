"""numpy / scipy restatement of spx_thompson_grad_batch (include/spx.h): value and gradient of a posterior sample path at
arbitrary points.  The prior p(x) and its gradient are evaluated in long double from tests/ts_oracle.py's own frequencies and
reduced phases; the update term k(x, X)' alpha uses alpha by scipy's Cholesky route on the chooser covariance, as
ts_oracle.paths does.  No engine, no GPU."""
import numpy as np
import scipy.linalg as spla

from oracle import gp_ei_oracle as orc
from tests import ts_oracle as tso

LD = np.longdouble
SIN_ULPS = 4                        # csrc/ts_device.h: SPX_TS_SIN_ULPS
PI_LD = LD("3.14159265358979323846264338327950288")
SQRT5, SQRT3 = np.sqrt(LD(5)), np.sqrt(LD(3))


def kernel_ld(covar, row, comp, X):
    """(k (n, N), dk/dx (n, N, D)) of k(x_i, X_j) = amp2 corr(r) in long double: the TRUE partial derivatives with respect to
    the point, dk/dx_d = amp2 (d corr / d r^2) 2 (x_d - X_jd) / ls_d^2."""
    _, _, amp2, ls = orc.unpack_hyper(row)
    ls = (np.ones(comp.shape[1]) if covar == "SE" else np.asarray(ls, dtype=np.float64)).astype(LD)
    diff = (np.asarray(X, dtype=np.float64).astype(LD)[:, None, :] - np.asarray(comp, dtype=np.float64).astype(LD)[None, :, :]) / ls
    r2 = np.sum(diff * diff, axis=2)
    r = np.sqrt(r2)
    if covar == "Matern52":
        e = np.exp(-SQRT5 * r)
        c, dc = (1 + SQRT5 * r + LD(5) / 3 * r2) * e, -(LD(5) / 6) * e * (1 + SQRT5 * r)
    elif covar == "Matern32":
        e = np.exp(-SQRT3 * r)
        c, dc = (1 + SQRT3 * r) * e, -LD(1.5) * e
    else:
        e = np.exp(-r2 / 2)
        c, dc = e, -e / 2
    a = LD(np.float64(amp2))
    return a * c, a * dc[:, :, None] * (2 * diff / ls)


class Path(object):
    """Sample path s of draw `row` (index d of the randoms when per_draw) as a function of x."""

    def __init__(self, covar, comp, vals, row, randoms, s=0, d=0, per_draw=False):
        self.covar, self.comp, self.row = covar, np.asarray(comp, dtype=np.float64), np.asarray(row, dtype=np.float64)
        mean, noise, amp2, ls = orc.unpack_hyper(row)
        w, eps = tso.draw_randoms(randoms, d, per_draw)
        self.w = np.asarray(w[s], dtype=np.float64)
        self.nu = tso.frequencies(covar, row, randoms["omega_z"], randoms["chi"])
        self.phase = np.asarray(randoms["phase"], dtype=np.float64)
        p_obs = tso.prior(row, w, tso.features(self.nu, self.phase, comp))
        rhs = tso.rhs_of(row, vals, p_obs, eps)[s]
        with orc.covar(covar):
            K = orc.cov(amp2, ls, self.comp) + noise * np.eye(self.comp.shape[0])
        self.alpha = spla.cho_solve((spla.cholesky(K, lower=True), True), rhs - mean)
        self.mean, self.amp2, self.ls = float(mean), amp2, ls
        self.scale = tso.scale_of(row, self.nu.shape[0])

    def prior(self, X):
        """(p (n,), gp (n, D), sn (n, F)) in long double from the float64 reduced phases of ts_oracle.phases."""
        r = tso.phases(self.nu, self.phase, X).astype(LD)
        c, sn = np.cos(2 * PI_LD * r), np.sin(2 * PI_LD * r)
        sc, w, nu = LD(self.scale), self.w.astype(LD), self.nu.astype(LD)
        p = sc * np.dot(c, w)
        gp = -(sc * 2 * PI_LD) * np.dot(sn * w[None, :], nu)
        return p, gp, sn

    def update(self, X):
        """(m (n,), gu (n, D)): k' alpha with numpy's float64 covariance, and the long-double derivative against alpha."""
        with orc.covar(self.covar):
            Ks = orc.cov(self.amp2, self.ls, self.comp, np.asarray(X, dtype=np.float64))          # (N, n)
        _, dk = kernel_ld(self.covar, self.row, self.comp, X)
        return np.dot(Ks.T, self.alpha), np.einsum("ijd,j->id", dk, self.alpha.astype(LD))

    def __call__(self, X, parts=False):
        """(value (n,), grad (n, D)) as float64; parts=True: also (prior, gp, m, gu).  Every point is evaluated on its own, so a
        point's numbers do not depend on the batch."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        out = [[], [], [], [], [], []]
        for i in range(X.shape[0]):
            x = X[i:i + 1]
            if not np.all(np.isfinite(x)):
                nan = np.full(X.shape[1], np.nan)
                vals = (np.nan, nan, np.nan, nan, np.nan, nan)
            else:
                p, gp, _ = self.prior(x)
                m, gu = self.update(x)
                p0, gp0, gu0 = np.float64(p[0]), gp[0].astype(np.float64), gu[0].astype(np.float64)
                vals = ((m[0] + self.mean) + p0, gu0 + gp0, p0, gp0, m[0], gu0)
            for o, v in zip(out, vals):
                o.append(v)
        out = [np.array(o, dtype=np.float64) for o in out]
        return tuple(out) if parts else (out[0], out[1])


def value_grad(covar, comp, vals, row, randoms, s, X, d=0, per_draw=False, parts=False):
    return Path(covar, comp, vals, row, randoms, s, d, per_draw)(X, parts)


def grad_bound(row, w, nu, phase, X, Dp, sn):
    """The derived bound of the device's prior gradient against Path.prior's, per (point, dimension), with u = 2^-53:
      |d gp_j| <= scale 2 pi ( sum_f |nu_fj w_f| (2 pi (Dp + D + 5) u (sum_j |nu_fj x_j| + 1) + (SIN_ULPS + 1) u)
                              + (F + 4) u sum_f |nu_fj w_f sn_f| ).
    The phase: the device's dot product of Dp terms plus the phase and the reduction move u_f by at most (Dp + 3) half-ulps of
    the magnitudes summed (ts_oracle.prior_bound), and the float64 dot product of D terms plus the phase this oracle starts
    from by (D + 2) more; the sine's slope is at most 2 pi.  The sine: SIN_ULPS u is ts_device.h's budget (|sin| <= 1), one more u
    for the product w sin.  The sum: F roundings of the magnitudes summed on the MFMA, the product scale * TWO_PI, the final
    product, and TWO_PI against 2 pi (0.35 u): (F + 4) u.  w (F,), nu (F, D), sn (n, F): the sines of the oracle."""
    u = 2.0 ** -53
    F, D = nu.shape
    X = np.asarray(X, dtype=np.float64)
    mag = np.dot(np.abs(X), np.abs(nu).T) + 1.0                                                  # (n, F)
    per_f = 2 * np.pi * (Dp + D + 5) * u * mag + (SIN_ULPS + 1) * u                              # (n, F)
    anw = np.abs(nu) * np.abs(np.asarray(w, dtype=np.float64))[:, None]                          # (F, D)
    sc = tso.scale_of(row, F) * 2 * np.pi
    return sc * (np.dot(per_f, anw) + (F + 4) * u * np.dot(np.abs(np.asarray(sn, dtype=np.float64)), anw))
