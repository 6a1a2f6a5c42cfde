"""50-digit yardstick (mpmath) of leave-one-out cross-validation on a GIVEN float64 covariance matrix K: the entries of K, y
and the mean are taken exactly, K is inverted at 50 digits, and
    kinv_diag_i = (K^-1)_ii     loo_var_i = 1 / kinv_diag_i     loo_mean_i = y_i - (K^-1 (y - mean))_i / kinv_diag_i.
With cond(K) up to 1e7 the yardstick itself is good to some 40 digits.  Test code only: nothing in spearmint_amd imports this
module.  tests/golden/loo_mp.npz holds the CPU cases: inputs, the yardstick's values rounded to float64 and the float64
oracle's recorded errors (make_fixture below wrote it)."""
import numpy as np

DPS = 50
# the cases of tests/test_loo_host.py: N x covar x noise, D = 3, one hyper row each
CASE_N = (1, 2, 24, 40)
CASE_NOISE = (0.1, 1e-2, 1e-3)
SEED = 23


def _mp():
    import mpmath
    return mpmath.mp


def loo_mp(K, y, mean):
    """(loo_mean, loo_var, kinv_diag) as lists of mpf."""
    mp = _mp()
    with mp.workdps(DPS):
        n = len(y)
        Km = mp.matrix([[mp.mpf(float(K[i][j])) for j in range(n)] for i in range(n)])
        Ki = mp.inverse(Km)
        r = mp.matrix([mp.mpf(float(v)) - mp.mpf(float(mean)) for v in y])
        alpha = Ki * r
        c = [Ki[i, i] for i in range(n)]
        return [mp.mpf(float(y[i])) - alpha[i] / c[i] for i in range(n)], [1 / ci for ci in c], c


def errors(got, want_mp, y, mean):
    """The three relative errors the bounds are stated in, of float64 arrays got = (loo_mean, loo_var, kinv_diag) against the
    yardstick's mpf lists: loo_mean relative to max|y - mean|, the other two relative to the value."""
    mp = _mp()
    with mp.workdps(DPS):
        scale = max(abs(mp.mpf(float(v)) - mp.mpf(float(mean))) for v in y)
        e_mean = max(abs(mp.mpf(float(g)) - w) for g, w in zip(got[0], want_mp[0])) / scale
        e_var = max(abs(mp.mpf(float(g)) - w) / abs(w) for g, w in zip(got[1], want_mp[1]))
        e_c = max(abs(mp.mpf(float(g)) - w) / abs(w) for g, w in zip(got[2], want_mp[2]))
        return float(e_mean), float(e_var), float(e_c)


def rounded(want_mp):
    return tuple(np.array([float(v) for v in part]) for part in want_mp)


def cases():
    """(name, comp, y, hyper_row, covar) of every CPU case."""
    from tests import loo_oracle as lo
    out = []
    for ci, covar in enumerate(lo.COVARS):
        for N in CASE_N:
            for ni, noise in enumerate(CASE_NOISE):
                comp, y, rows = lo.problem(N, 3, 1, SEED + 100 * ci + 10 * ni + N, noise=noise)
                rows[0, 1] = noise
                out.append(("%s_N%d_n%d" % (covar, N, ni), comp, y, rows[0], covar))
    return out


def make_fixture(path):
    """Writes tests/golden/loo_mp.npz: per case the inputs, the yardstick (on K as the host formula gives it) rounded to
    float64, the float64 oracle's three errors against it and cond(K)."""
    from tests import loo_oracle as lo
    data = {}
    for name, comp, y, row, covar in cases():
        K = lo.k_host(comp, row, covar)
        want = loo_mp(K, y, row[0])
        err = errors(lo.loo_from_k(K, y, row[0]), want, y, row[0])
        r = rounded(want)
        data[name + "_comp"], data[name + "_y"], data[name + "_row"] = comp, y, row
        data[name + "_mean"], data[name + "_var"], data[name + "_c"] = r
        data[name + "_err"] = np.array(err + (np.linalg.cond(K),))
    np.savez_compressed(path, **data)


if __name__ == "__main__":
    import os
    make_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_mp.npz"))
