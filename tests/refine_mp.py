"""50-digit restatement (mpmath) of the refinement objective spx_ei_grad_batch computes: -(sum over draws of EI) and its
gradient in the three branches -- plain, per second, averaged over pending fantasies.  It is the chooser's arithmetic
(csrc/refine_kernels.hip:11-20): the covariance WITH its 1e-6 amp2 diagonal jitter, Cholesky, the two triangular solves
t = L^-1 k and z = L^-T t, func_v = amp2 (1 + 1e-6) - |t|^2, Phi and phi, the gradient with the reference's factor one
half, the per-second quotient rule and the mean over fantasies.  Every input is converted from float64 exactly; the
distance is the plain sum of squared differences, not the expanded GEMM form.

It is the yardstick where the float64 oracle itself loses digits: once EI leaves the range of the golden vectors, u is
large and negative and the error of func_m is amplified by about u^2 / 2 in EI.

Test code only.  The GPU tests read its results from tests/golden/refine_tail_mp.npz (scripts/make_golden_refine_tail.py)
and never import mpmath; everything here that needs it imports it inside the function."""
import numpy as np

from tests import constrained_refine_helpers as hp
from tests import refine_helpers as rh

DPS = 50


def _corr_mp(mp, covar, r2):
    """(corr, d corr / d r2) at the squared scaled distance r2 (gp.py:95-132)."""
    if covar == "Matern52":
        r = mp.sqrt(r2)
        e = mp.exp(-mp.sqrt(5) * r)
        return (1 + mp.sqrt(5) * r + (mp.mpf(5) / 3) * r2) * e, -(mp.mpf(5) / 6) * e * (1 + mp.sqrt(5) * r)
    if covar == "Matern32":
        r = mp.sqrt(r2)
        e = mp.exp(-mp.sqrt(3) * r)
        return (1 + mp.sqrt(3) * r) * e, -mp.mpf(3) / 2 * e
    if covar == "ARDSE":
        e = mp.exp(-r2 / 2)
        return e, -e / 2
    raise AttributeError("no gradient of the covariance function %r" % (covar,))


class _Draw(object):
    """One GP (objective or log-duration) of one draw over the rows X: its factor, and at every point the vectors
    k, t = L^-1 k, z = L^-T t, G[j][d] = dk/dr2 (r_j) 2 (X_jd - x_d) / ls_d^2 and func_s."""

    def __init__(self, mp, covar, X, hyper, pts):
        f = lambda v: mp.mpf(float(v))      # noqa: E731  (exact: a float64 is a dyadic rational)
        self.mp = mp
        self.mean, noise, self.amp2 = f(hyper[0]), f(hyper[1]), f(hyper[2])
        ls = [f(v) for v in hyper[3:]]
        n, D = X.shape
        self.n, self.D = n, D
        Xm = [[f(X[i, d]) for d in range(D)] for i in range(n)]
        r2 = lambda a, b: mp.fsum(((a[d] - b[d]) / ls[d]) ** 2 for d in range(D))      # noqa: E731
        K = [[self.amp2 * _corr_mp(mp, covar, r2(Xm[i], Xm[j]))[0] for j in range(i + 1)] for i in range(n)]
        for i in range(n):
            K[i][i] = self.amp2 * (1 + f(1e-6)) + noise      # corr(0) = 1, + the jitter, + the noise
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1):
                s = K[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))
                L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
        self.L = L
        self.k, self.t, self.z, self.G, self.s = [], [], [], [], []
        for x in pts:
            xm = [f(v) for v in x]
            cd = [_corr_mp(mp, covar, r2(Xm[j], xm)) for j in range(n)]
            k = [self.amp2 * c for c, _ in cd]
            t = self.fwd(k)
            self.k.append(k)
            self.t.append(t)
            self.z.append(self.bwd(t))
            self.G.append([[dk * 2 * (Xm[j][d] - xm[d]) / ls[d] ** 2 for d in range(D)] for j, (_, dk) in enumerate(cd)])
            self.s.append(mp.sqrt(self.amp2 * (1 + f(1e-6)) - mp.fsum(v * v for v in t)))

    def fwd(self, b):
        mp, L, y = self.mp, self.L, []
        for i in range(self.n):
            y.append((b[i] - mp.fsum(L[i][k] * y[k] for k in range(i))) / L[i][i])
        return y

    def bwd(self, b):
        mp, L, n = self.mp, self.L, self.n
        y = [mp.mpf(0)] * n
        for i in reversed(range(n)):
            y[i] = (b[i] - mp.fsum(L[k][i] * y[k] for k in range(i + 1, n))) / L[i][i]
        return y

    def alpha(self, y):
        """K^-1 (y - mean)."""
        return self.bwd(self.fwd([self.mp.mpf(float(v)) - self.mean for v in y]))

    def dot_G(self, w, p):
        """[w . G[:, d] for every d] at point p."""
        mp = self.mp
        return [mp.fsum(w[j] * self.G[p][j][d] for j in range(self.n)) for d in range(self.D)]


def _ei(mp, best, func_m, func_s):
    u = (best - func_m) / func_s
    cdf, pdf = mp.ncdf(u), mp.npdf(u)
    return func_s * (u * cdf + pdf), -cdf, pdf / (2 * func_s)


def neg_ei_and_grad_mp(p, pts, value_sets=None):
    """The refinement objective of the problem p (tests/refine_helpers.make_problem) at DPS digits: (f, g) with f a list
    of mpf per point and g a list of D mpf per point, summed over the draws.  value_sets: a list of (vals, fant, bests)
    to evaluate against the same factors (the factors do not depend on the values); the result is then a list of
    (f, g), one per set."""
    import mpmath
    mp = mpmath.mp
    single = value_sets is None
    if single:
        value_sets = [(p.vals, getattr(p, "fant", None), getattr(p, "bests", None))]
    P, D = pts.shape
    with mp.workdps(DPS):
        out = [([mp.mpf(0)] * P, [[mp.mpf(0)] * D for _ in range(P)]) for _ in value_sets]
        for h in range(p.H):
            dr = _Draw(mp, p.covar, p.X, p.rows[h], pts)
            if p.branch == "persec":
                tm = _Draw(mp, p.covar, p.X, p.trows[h], pts)
                a_t = tm.alpha(p.log_durs)
            half_amp2 = dr.amp2 / 2
            for (vals, fant, bests), (fo, go) in zip(value_sets, out):
                if p.branch == "fant":
                    S = fant.shape[2]
                    alphas = [dr.alpha(fant[h][:, s]) for s in range(S)]
                    best_s = [mp.mpf(float(b)) for b in bests[h]]
                else:
                    alphas = [dr.alpha(vals)]
                    best_s = [mp.mpf(float(np.min(vals)))]
                for k in range(P):
                    gv = dr.dot_G([-2 * v for v in dr.z[k]], k)
                    ei_sum, g_sum = mp.mpf(0), [mp.mpf(0)] * D
                    for a, b in zip(alphas, best_s):
                        func_m = mp.fsum(x * y for x, y in zip(dr.k[k], a)) + dr.mean
                        ei, g_m, g_s2 = _ei(mp, b, func_m, dr.s[k])
                        gm = dr.dot_G(a, k)
                        ei_sum += ei
                        g_sum = [gs + half_amp2 * (gm[d] * g_m + gv[d] * g_s2) for d, gs in enumerate(g_sum)]
                    ei, g = ei_sum / len(alphas), [v / len(alphas) for v in g_sum]
                    if p.branch == "persec":
                        time_m = mp.exp(mp.fsum(x * y for x, y in zip(tm.k[k], a_t)) + tm.mean)
                        gt = [tm.amp2 / 2 * v * time_m for v in tm.dot_G(a_t, k)]
                        g = [(time_m * g[d] - ei * gt[d]) / time_m ** 2 for d in range(D)]
                        ei = ei / time_m
                    fo[k] = fo[k] - ei
                    go[k] = [go[k][d] + g[d] for d in range(D)]
    return out[0] if single else out


def to_float64(vals):
    """Round a list of mpf to float64 (values below the denormal range become 0.0)."""
    return np.array([float(v) for v in vals], dtype=np.float64)


def log10_abs_mp(vals):
    """log10 |v| of a list of non-zero mpf, as float64 -- defined where v itself is below float64's range."""
    import mpmath
    with mpmath.mp.workdps(DPS):
        return np.array([float(mpmath.log10(abs(v))) for v in vals], dtype=np.float64)


# ---- the tail problem (one definition for the generator, the CPU test and the GPU test) --------------------------------
TAIL_SEED, TAIL_N, TAIL_D, TAIL_P, TAIL_S, TAIL_NPEND = 11, 48, 2, 150, 5, 2
TAIL_BANDS = [(-3.0, 1.0), (-20.0, -3.0), (-100.0, -20.0), (-300.0, -100.0)]   # log10 |f|; the first closed, the others [lo, hi)
# How far the observation nearest (0.8, 0.8) is lowered in the "tail" value set, per covariance: chosen by counting, with
# the float64 oracle, the points per band and below 1e-300 -- at least one and at most 15 % of the points below 1e-300 in
# every branch (plain branch: Matern52 1 of 150; 2.5 gives 26.  Matern32 5.  ARDSE 7; 1.3 gives none, 1.5 gives 27).
# scripts/make_golden_refine_tail.py prints the counts of the 50-digit reference; tests/test_refine_mp.py asserts them.
TAIL_SHIFT = {"Matern52": 2.0, "Matern32": 3.0, "ARDSE": 1.4}
SETS = ("mild", "tail")


def tail_problem(covar, branch):
    """48 observations in 2 dimensions, one draw and a time draw of its own, 2 pending points with 5 fantasies, 150 points
    (120 uniform, 30 at comp[low] + 0.03 randn clipped to the unit box).  Returns (p, pts, value_sets): p carries the mild
    values; value_sets = [(vals, fant, bests) mild, the same with observation `low` lowered by TAIL_SHIFT[covar]].  The
    fantasy columns are elementwise (the observed values, and 0.3 + 0.3 randn at the pending points), so the fixture's
    inputs do not depend on a BLAS."""
    rs = np.random.RandomState(TAIL_SEED)
    n, D, S = TAIL_N, TAIL_D, TAIL_S
    p = hp.Problem()
    p.covar, p.branch, p.D, p.H = covar, branch, D, 1
    p.S = S if branch == "fant" else 0
    p.comp = rs.rand(n, D)
    p.vals = np.sum((p.comp - 0.4) ** 2, axis=1) + 0.02 * rs.randn(n)
    p.rows = np.column_stack((rs.uniform(0.1, 0.3, 1), rs.uniform(1e-3, 1e-2, 1), rs.uniform(0.5, 1.5, 1),
                              rs.uniform(0.3, 1.5, (1, D))))
    p.trows = np.column_stack((rs.uniform(-0.4, 0.4, 1), rs.uniform(1e-3, 1e-2, 1), rs.uniform(0.3, 0.9, 1),
                               rs.uniform(0.4, 2.0, (1, D))))
    p.log_durs = 0.7 * np.sum(p.comp, axis=1) / D + 0.1 * rs.randn(n)
    pend = rs.rand(TAIL_NPEND, D)
    pend_fant = 0.3 + 0.3 * rs.randn(TAIL_NPEND, S)
    low = int(np.argmin(np.sum((p.comp - 0.8) ** 2, axis=1)))
    pts = np.concatenate((rs.rand(120, D), np.clip(p.comp[low] + 0.03 * rs.randn(30, D), 0.0, 1.0)))
    assert pts.shape[0] == TAIL_P
    p.pend = pend if branch == "fant" else np.zeros((0, D))
    p.X = np.concatenate((p.comp, p.pend))
    p.compv, p.valsv, p.low = p.comp, p.vals, low
    sets = []
    for shift in (0.0, TAIL_SHIFT[covar]):
        vals = p.vals.copy()
        vals[low] -= shift
        if branch == "fant":
            fant = np.concatenate((np.tile(vals[:, None], (1, S)), pend_fant))[None]
            sets.append((vals, fant, np.min(fant[0], axis=0)[None]))
        else:
            sets.append((vals, None, None))
    p.vals, p.fant, p.bests = sets[0]
    p.valsv, p.best = p.vals, np.min(p.vals)
    return p, pts, sets


def with_values(p, value_set):
    """The problem p with another value set (the tail problem's second)."""
    q = hp.Problem()
    q.__dict__.update(p.__dict__)
    q.vals, q.fant, q.bests = value_set
    q.valsv, q.best = q.vals, np.min(q.vals)
    return q


def key(covar, branch, which, what):
    return "%s_%s_%s_%s" % (covar, branch, which, what)


def tail_reference(covars=rh.COVARS, branches=rh.BRANCHES):
    """The fixture's arrays: per covariance, branch and value set the 50-digit f and g rounded to float64 and
    log10 |f| (defined below float64's range too)."""
    out = {}
    for covar in covars:
        for branch in branches:
            p, pts, sets = tail_problem(covar, branch)
            for which, (f, g) in zip(SETS, neg_ei_and_grad_mp(p, pts, sets)):
                out[key(covar, branch, which, "f")] = to_float64(f)
                out[key(covar, branch, which, "g")] = np.array([to_float64(row) for row in g])
                out[key(covar, branch, which, "log10f")] = log10_abs_mp(f)
    return out


def band_of(log10f):
    """Index of the band of every point (-1: in none -- above 10, or below 1e-300)."""
    idx = np.full(log10f.shape, -1)
    for i, (lo, hi) in enumerate(TAIL_BANDS):
        idx[(log10f >= lo) & ((log10f <= hi) if i == 0 else (log10f < hi))] = i
    return idx


def band_errors(f, g, f_ref, g_ref, log10f):
    """Per band of log10 |f_ref|: (max relative error of the value, max over the points of
    max_d |g_d - ref_d| / max_d |ref_d|); None for an empty band."""
    idx = band_of(log10f)
    out = []
    for i in range(len(TAIL_BANDS)):
        sel = idx == i
        if not sel.any():
            out.append(None)
            continue
        ev = np.max(np.abs(f[sel] - f_ref[sel]) / np.abs(f_ref[sel]))
        eg = np.max(np.max(np.abs(g[sel] - g_ref[sel]), axis=1) / np.max(np.abs(g_ref[sel]), axis=1))
        out.append((float(ev), float(eg)))
    return out
