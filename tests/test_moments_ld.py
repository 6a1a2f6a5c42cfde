"""The yardstick of the posterior moments itself, on the CPU (tests/moments_ld.py): the long-double computation against a
40-digit restatement, the LAPACK route against the oracle the goldens pin, and every problem of the GPU table
(tests/test_gpu_q_moments_yardstick.py) qualified from the references alone -- on the oracle's K and K*, before any device
result exists: dpotrf succeeds, the far candidates' K* columns are exactly zero, the smallest func_v / prior_v lies in
(1e-7, 1e-2) so that the cancellation is exercised, both float64 reference algorithms are within 1e-11 of the long-double
values in both units (so the bar the GPU file derives from them is at least 25 x tighter than the suite's 1e-9), and the
as-built restatement returns exactly (mean, prior_v) for the far candidates."""
import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import moments_ld as ml

LD = np.longdouble
LD_BAR = 2.0 ** -58                 # six bits of room over the 2^-64 of the extended format
REF_CAP = 1e-11                     # either float64 reference algorithm against the long-double values, both units
V_LOW, V_HIGH = 1e-7, 1e-2          # the smallest func_v / prior_v of a draw


def key_id(key):
    return "%d-%d-%s-%s" % key


def oracle_inputs(p, h):
    """(K, K*, y, mean, prior_v) of draw h as the oracle forms them (GPEIChooser.py:186-189, :195)."""
    mean, noise, amp2, ls = orc.unpack_hyper(p.rows[h])
    with orc.covar(p.covar):
        K = orc.cov(amp2, ls, p.comp) + noise * np.eye(p.comp.shape[0])
        Ks = orc.cov(amp2, ls, p.comp, p.cand)
    return K, Ks, p.vals - mean, float(mean), ml.prior_v_of(p.rows[h])


# ---- a. the long-double helper against 40 digits -----------------------------------------------------------------------------
def moments_mp(K, Ks, y, mean, prior_v, dps=40):
    """The same quantities with mpmath at `dps` digits from the same float64 inputs: (m, v, s_m, s_v) as lists of mpf."""
    import mpmath as mp
    with mp.workdps(dps):
        n, M = K.shape[0], Ks.shape[1]
        A = [[mp.mpf(float(K[i, j])) for j in range(n)] for i in range(n)]
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for j in range(n):
            d = A[j][j] - mp.fsum(L[j][t] ** 2 for t in range(j))
            assert d > 0
            L[j][j] = mp.sqrt(d)
            for i in range(j + 1, n):
                L[i][j] = (A[i][j] - mp.fsum(L[i][t] * L[j][t] for t in range(j))) / L[j][j]
        gamma = []
        for i in range(n):
            gamma.append((mp.mpf(float(y[i])) - mp.fsum(L[i][t] * gamma[t] for t in range(i))) / L[i][i])
        gnorm = mp.sqrt(mp.fsum(g * g for g in gamma))
        m, v, s_m = [], [], []
        for c in range(M):
            b = []
            for i in range(n):
                b.append((mp.mpf(float(Ks[i, c])) - mp.fsum(L[i][t] * b[t] for t in range(i))) / L[i][i])
            ss = mp.fsum(x * x for x in b)
            m.append(mp.fsum(x * g for x, g in zip(b, gamma)) + mp.mpf(mean))
            v.append(mp.mpf(prior_v) - ss)
            s_m.append(mp.sqrt(ss) * gnorm + abs(mp.mpf(mean)))
        return m, v, s_m, mp.mpf(prior_v)


def to_mp(x):
    """A long double as an exact mpf: its float64 head plus the float64 of what is left (64 significant bits in all)."""
    import mpmath as mp
    hi = np.float64(x)
    return mp.mpf(float(hi)) + mp.mpf(float(np.float64(x - LD(hi))))


@pytest.mark.parametrize("band", ["a", "c"])
@pytest.mark.parametrize("N", [5, 20])
def test_longdouble_moments_against_forty_digits(N, band):
    import mpmath as mp
    p = ml.problem(N, 12, ml.D, ml.H, band, "Matern52", 8100 + N)
    assert p.n_on == 5 and p.n_near == 5 and p.n_far == 0
    for h in range(ml.H):
        args = oracle_inputs(p, h)
        ref = ml.moments_longdouble(*args)
        m, v, s_m, s_v = moments_mp(*args)
        with mp.workdps(40):
            em = max(abs(to_mp(ref.m[c]) - m[c]) / s_m[c] for c in range(12))
            ev = max(abs(to_mp(ref.v[c]) - v[c]) / s_v for c in range(12))
            es = max(abs(to_mp(ref.s_m[c]) - s_m[c]) / s_m[c] for c in range(12))
        print("N %d band %s draw %d: long double against 40 digits: func_m %.2e func_v %.2e s_m %.2e (bar %.2e)"
              % (N, band, h, float(em), float(ev), float(es), LD_BAR))
        assert float(em) <= LD_BAR and float(ev) <= LD_BAR
        assert float(es) <= 2.0 ** -40           # (a scale: an error of it is a relative error of the errors counted in it)
        assert ref.s_v == LD(args[4])


# ---- b. the LAPACK helper is the oracle's route ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [ml.key_of(17, "a"), ml.key_of(130, "c"), ml.key_of(300, "b", covar="ARDSE")], ids=key_id)
def test_lapack_moments_are_the_oracles(key):
    p = ml.table_problem(key)
    for h in range(ml.H):
        K, Ks, y, mean, prior_v = oracle_inputs(p, h)
        st = {}
        with orc.covar(p.covar), np.errstate(all="ignore"):
            orc.compute_ei(p.comp, p.cand, p.vals, p.rows[h], stages=st)
        assert np.array_equal(st["K"], K) and np.array_equal(st["Kstar"], Ks)
        m, v = ml.moments_lapack(K, Ks, y, mean, prior_v)
        ref = ml.moments_longdouble(K, Ks, y, mean, prior_v)
        s_m = ref.s_m.astype(np.float64)
        np.testing.assert_allclose(m / s_m, st["func_m"] / s_m, rtol=1e-14, atol=0)
        np.testing.assert_allclose(v / prior_v, st["func_v"] / prior_v, rtol=1e-14, atol=0)


# ---- c. the inputs qualify ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ml.table_keys(), ids=key_id)
def test_every_problem_of_the_gpu_table_qualifies(key):
    p = ml.table_problem(key)
    N, M = p.comp.shape[0], p.cand.shape[0]
    assert p.n_on == min(p.k, M) and (M == 1 or (p.n_near == p.k and p.n_far == ml.FAR))
    far = ml.far_columns(p)
    worst = np.zeros(4)
    for h in range(ml.H):
        K, Ks, y, mean, prior_v = oracle_inputs(p, h)
        assert np.array_equal(Ks[:, far], np.zeros((N, len(far))))
        ref = ml.moments_longdouble(K, Ks, y, mean, prior_v)
        lap = ml.moments_lapack(K, Ks, y, mean, prior_v)           # (asserts dpotrf's info == 0)
        built = ml.moments_as_built(K, Ks, y, mean, prior_v)
        low = float(np.min(ref.v / ref.s_v))
        worst = np.maximum(worst, ml.errors(*lap, ref=ref) + ml.errors(*built, ref=ref))
        print("%s draw %d: min func_v / prior_v %.2e; lapack m %.2e v %.2e; as built m %.2e v %.2e"
              % ((key, h, low) + ml.errors(*lap, ref=ref) + ml.errors(*built, ref=ref)))
        assert V_LOW < low < V_HIGH, (key, h, low)
        assert np.array_equal(built[0][far], np.full(len(far), mean))
        assert np.array_equal(built[1][far], np.full(len(far), prior_v))
        assert np.array_equal(lap[1][far], np.full(len(far), prior_v))
    assert np.all(worst <= REF_CAP), (key, worst)
