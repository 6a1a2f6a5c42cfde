"""The yardstick of the device-formed fantasies itself, on the CPU (tests/fantasy_ld.py): both long-double functions against a
40-digit restatement, and every problem of the GPU table (tests/test_gpu_s_fantasy_yardstick.py) qualified from the references
alone -- on the host's K, K* and factor (tests/fantasy_helpers.host_factor), before any device result exists: dpotrf and both
float64 forms succeed, the smallest pivot of the long-double pend_K is at least 1e-6 amp2 (the jitter: positive definiteness is
never in question), both float64 forms are within 1e-11 of the yardstick for the fantasies and for Gamma's tail, both float64
chains within 1e-10 for the conditional means, and the far candidates' K* columns are exactly zero with m_s == mean in both
chains.  A problem that does not qualify gets another seed in fantasy_ld.SEEDS; none has needed one.

Measured here.  The float64 forms over the whole table of 21 problems x 3 draws (bar 1e-11): fantasies LAPACK form 1.2e-13, as
built 2.3e-13; Gamma's tail 5.7e-12 and 5.6e-12 (Matern-3/2, noise = 1e-9 amp2); the chains (bar 1e-10) 1.9e-12 and 1.9e-12 (ARDSE);
the smallest pivot of pend_K 1.3e-6 amp2 (ARDSE, noise = 1e-9 amp2), 2.0e-6 amp2 in most draws.

Long double against 40 digits (bar 2^-58 = 3.47e-18), (60, 7) as drawn / (64, 64) noise = amp2 / (130, 63) noise = 1e-9 amp2:
pend_m 3.1e-20 / 3.0e-20 / 2.7e-20; C 2.7e-20 / 2.8e-20 / 2.2e-20; T 2.2e-20 / 2.4e-20 / 2.7e-20; fantasies 3.1e-20 / 3.0e-20 /
2.7e-20; Gamma's tail 1.6e-20 / 4.2e-20 / 2.7e-20; the chain's fantasies 3.0e-20 / 3.0e-20 / 2.7e-20 and m_s 8.0e-21 / 1.5e-20 /
4.1e-21 -- the closing rounding to one long double (2^-64 = 5.4e-20) and nothing else.  The yardstick computes in double words of
np.longdouble (tests/fantasy_ld.py says why): the same steps in a plain long double, with tests/factor_helpers.chol_longdouble
for the chain, missed this bar in four of the six tests -- C 1.1e-16 and the fantasies 1.1e-17 at (64, 64) with noise = amp2, m_s
1.9e-17 / 7.1e-18 / 1.1e-16 -- because one rounding at 2^-64 meets a cancellation of six digits."""
import functools

import numpy as np
import pytest

from tests import fantasy_ld as fl

LD = np.longdouble
LD_BAR = 2.0 ** -58
FORM_CAP = 1e-11
CHAIN_CAP = 1e-10
PIVOT_FLOOR = 1e-6


# ---- a. the long-double functions against 40 digits ---------------------------------------------------------------------------
def to_mp(x):
    """A long double as an exact mpf: its float64 head plus the float64 of what is left (64 significant bits in all)."""
    import mpmath as mp
    hi = np.float64(x)
    return mp.mpf(float(hi)) + mp.mpf(float(np.float64(x - LD(hi))))


def chol_mp(A):
    import mpmath as mp
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        d = A[j][j] - mp.fsum(L[j][t] ** 2 for t in range(j))
        assert d > 0
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - mp.fsum(L[i][t] * L[j][t] for t in range(j))) / L[j][j]
    return L


def posterior_mp(n, mean, noise, l_rows, gamma, z):
    """fantasy_ld.posterior_longdouble restated with mpf entries (l_rows, gamma, z: lists of mpf): (pend_m, C, T, pend_fant, tail)."""
    import mpmath as mp
    p, S = len(l_rows), len(z[0])
    ls_ = [[l_rows[i][n + k] if k <= i else mp.mpf(0) for k in range(p)] for i in range(p)]
    pend_m = [mp.fsum(l_rows[i][j] * gamma[j] for j in range(n)) + mean for i in range(p)]
    pend_k = [[mp.fsum(ls_[i][k] * ls_[j][k] for k in range(min(i, j) + 1)) - (noise if i == j else 0) for j in range(p)]
              for i in range(p)]
    c = chol_mp(pend_k)
    t = [[mp.mpf(0)] * p for _ in range(p)]
    for j in range(p):
        for i in range(j, p):
            t[i][j] = (c[i][j] - mp.fsum(ls_[i][k] * t[k][j] for k in range(j, i))) / ls_[i][i]
    fant = [[mp.fsum(c[i][k] * z[k][s] for k in range(i + 1)) + pend_m[i] for s in range(S)] for i in range(p)]
    tail = [[mp.fsum(t[i][k] * z[k][s] for k in range(i + 1)) for s in range(S)] for i in range(p)]
    return pend_m, c, t, fant, tail


def mpf_rows(a):
    import mpmath as mp
    return [[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(a)]


def worst(ld, ref, unit):
    """max |ld - ref| / unit over a 2-d long-double array and its nested list of mpf."""
    import mpmath as mp
    ld = np.atleast_2d(ld)
    return float(max(abs(to_mp(ld[i, j]) - ref[i][j]) for i in range(ld.shape[0]) for j in range(ld.shape[1])) / mp.mpf(float(unit)))


MP_CASES = [((60, 7, "Matern52"), 0), ((64, 64, "Matern52"), 2), ((130, 63, "Matern52"), 1)]
MP_IDS = ["60-7-as-drawn", "64-64-noise-amp2", "130-63-1e-9"]


@functools.lru_cache(maxsize=None)
def forty_digits(key, h):
    """posterior_longdouble on the host factor's rows and chain_longdouble on the host's K and K* (the special candidates and
    three seeded ones), each against the same steps at 40 digits from the same float64 inputs: the worst differences by name."""
    import mpmath as mp
    p = fl.case_problem(key)
    N, P = p.comp.shape[0], p.pend.shape[0]
    mean, noise = float(p.rows[h, 0]), float(p.rows[h, 1])
    K, Ks, l_rows, gamma = fl.host_inputs(p, h)
    z = fl.z_of(p, h, fl.CHAIN_S, 1)
    cols = np.concatenate((np.arange(2 * p.n_pend_cand + fl.SPECIAL_K + 3), fl.far_columns(p)))
    Ks = np.ascontiguousarray(Ks[:, cols])
    post = fl.posterior_longdouble(p.vals, mean, noise, l_rows, gamma, z)
    chain = fl.chain_longdouble(K, Ks, p.vals, mean, noise, fl.prior_v_of(p.rows[h]), z, P)
    e = {}
    with mp.workdps(40):
        mpm, mpn = mp.mpf(mean), mp.mpf(noise)
        zz = mpf_rows(z)
        pm, c, t, fant, tail = posterior_mp(N, mpm, mpn, mpf_rows(l_rows), mpf_rows(gamma)[0], zz)
        unit = fl.fant_unit(post)
        e["pend_m"] = worst(post.pend_m[None, :], [pm], unit)
        e["C"] = worst(post.C, c, np.max(np.abs(post.C)))
        e["T"] = worst(post.T, t, np.max(np.abs(post.T)))
        e["fantasies"] = worst(post.pend_fant, fant, unit)
        e["tail"] = worst(post.tail, tail, np.max(np.abs(post.tail)))
        # the chain: Cholesky of K, gamma, the posterior from ITS bottom rows, B = L^-1 K*, m_s = B^T Gamma_s + mean
        n = N + P
        L = chol_mp(mpf_rows(K))
        y = [mp.mpf(float(v)) - mpm for v in p.vals] + [mp.mpf(0)] * P
        g = []
        for i in range(n):
            g.append((y[i] - mp.fsum(L[i][k] * g[k] for k in range(i))) / L[i][i])
        _, _, _, fant2, tail2 = posterior_mp(N, mpm, mpn, L[N:], g, zz)
        e["chain fantasies"] = worst(chain.post.pend_fant, fant2, fl.fant_unit(chain.post))
        e_ms, e_scale = mp.mpf(0), mp.mpf(0)
        for ci in range(len(cols)):
            b = []
            for i in range(n):
                b.append((mp.mpf(float(Ks[i, ci])) - mp.fsum(L[i][k] * b[k] for k in range(i))) / L[i][i])
            bn = mp.sqrt(mp.fsum(x * x for x in b))
            for s in range(fl.CHAIN_S):
                big = g[:N] + [tail2[i][s] for i in range(P)]
                m_s = mp.fsum(x * w for x, w in zip(b, big)) + mpm
                s_m = bn * mp.sqrt(mp.fsum(w * w for w in big)) + abs(mpm)
                e_ms = max(e_ms, abs(to_mp(chain.m[s, ci]) - m_s) / s_m)
                e_scale = max(e_scale, abs(to_mp(chain.s_m[s, ci]) - s_m) / s_m)
        e["m_s"], e["s_m"] = float(e_ms), float(e_scale)
    print("%s draw %d: long double against 40 digits (bar %.2e): %s" % (key, h, LD_BAR, ", ".join("%s %.2e" % kv for kv in e.items())))
    return e


@pytest.mark.parametrize("key,h", MP_CASES, ids=MP_IDS)
def test_posterior_longdouble_against_forty_digits(key, h):
    """pend_m and the fantasies in the fantasies' unit, C in units of max |C|, T and Gamma's tail relative to their own largest
    entry: all at 2^-58."""
    e = forty_digits(key, h)
    for name in ("pend_m", "C", "T", "fantasies", "tail"):
        assert e[name] <= LD_BAR, (name, e[name])


@pytest.mark.parametrize("key,h", MP_CASES, ids=MP_IDS)
def test_chain_longdouble_against_forty_digits(key, h):
    """The chain's fantasies in their unit and m_s in units of s_m at 2^-58 (s_m itself, a scale formed from the high words, at
    2^-40)."""
    e = forty_digits(key, h)
    assert e["s_m"] <= 2.0 ** -40
    assert e["chain fantasies"] <= LD_BAR and e["m_s"] <= LD_BAR, (e["chain fantasies"], e["m_s"])


# ---- b. the inputs qualify -------------------------------------------------------------------------------------------------------
def all_keys():
    keys = []
    for c in fl.CASES + fl.CHAIN_CASES + tuple((fl.UNIT_COLUMN_N, P, "Matern52") for P in fl.UNIT_COLUMN_PS):
        if fl.key_of(c) not in keys:
            keys.append(fl.key_of(c))
    return keys


def test_the_table_is_the_one_asked_for():
    assert [c[:2] for c in fl.CASES if c[2] == "Matern52"] == [(1, 1), (2, 1), (5, 4), (60, 7), (62, 4), (63, 1), (64, 1), (64, 64),
                                                                (100, 64), (127, 3), (128, 16), (130, 63), (190, 64), (257, 33)]
    assert sorted(c[2] for c in fl.CASES if c[:2] == (130, 63)) == ["ARDSE", "Matern32", "Matern52"]
    assert {c[3] for c in fl.CASES} == {1, 15, 16, 17, 33} and {c[4] for c in fl.CASES} == {0, 1}
    assert [c[:2] for c in fl.CHAIN_CASES] == [(60, 7), (64, 64), (100, 64), (130, 63), (257, 33)]
    assert all(c in [fl.key_of(x) for x in fl.CASES] for c in fl.CHAIN_CASES)


@pytest.mark.parametrize("key", all_keys(), ids=fl.case_id)
def test_every_problem_of_the_gpu_table_qualifies(key):
    unit_columns = key[0] == fl.UNIT_COLUMN_N
    p = fl.unit_column_problem(key[1]) if unit_columns else fl.case_problem(key)
    N, P = p.comp.shape[0], p.pend.shape[0]
    assert (N, P) == key[:2] and p.rows.shape[0] == fl.H
    # the placements
    assert P == 1 or np.array_equal(p.pend[P - 1], p.comp[0])
    assert P <= 2 or np.allclose(p.pend[1] - p.pend[2], fl.NEAR_PEND, rtol=1e-9, atol=0)
    if P > 1 or N % 2 == 0:
        assert np.allclose(p.pend[0] - p.comp[min(3, N - 1)], fl.NEAR_OBS, rtol=1e-9, atol=0)
    else:
        assert np.array_equal(p.pend[0], p.comp[0])
    assert np.allclose(p.rows[:, 1] / p.rows[:, 2], [p.rows[0, 1] / p.rows[0, 2], 1e-9, 1.0], rtol=1e-15, atol=0)
    assert 1e-4 <= p.rows[0, 1] / p.rows[0, 2] <= 1e-2
    far = fl.far_columns(p)
    w_form, w_tail, w_chain = np.zeros(2), np.zeros(2), np.zeros(2)
    for h in range(fl.H):
        mean, noise, amp2 = float(p.rows[h, 0]), float(p.rows[h, 1]), float(p.rows[h, 2])
        K, Ks, l_rows, gamma = fl.host_inputs(p, h)               # (spla.cholesky: dpotrf succeeded)
        assert np.array_equal(Ks[:, far], np.zeros((N + P, len(far))))
        z = p.z[h]
        post = fl.posterior_longdouble(p.vals, mean, noise, l_rows, gamma, z)
        piv = float(post.min_pivot) / amp2
        forms = (fl.lapack_form(p.vals, mean, noise, l_rows, gamma, z), fl.built_form(p.vals, mean, noise, l_rows, gamma, z))
        ef = np.array([fl.fant_error(f[0], post) for f in forms])
        et = np.array([fl.tail_error(f[1], post) for f in forms])
        zc = fl.z_of(p, h, min(fl.CHAIN_S, z.shape[1]), 1)
        chain = fl.chain_longdouble(K, Ks, p.vals, mean, noise, fl.prior_v_of(p.rows[h]), zc, P)
        routes = (fl.chain_reference_route(K, Ks, p.vals, mean, noise, zc, P), fl.chain_as_built(K, Ks, p.vals, mean, noise, zc, P))
        ec = np.array([fl.chain_error(r, chain) for r in routes])
        print("%s draw %d: smallest pivot %.2e amp2; fantasies lapack %.2e as built %.2e; Gamma's tail %.2e %.2e; chain reference "
              "route %.2e as built %.2e" % (key, h, piv, ef[0], ef[1], et[0], et[1], ec[0], ec[1]))
        assert piv >= PIVOT_FLOOR, (key, h, piv)
        for r in routes:
            assert np.array_equal(r[:, far], np.full((r.shape[0], len(far)), mean)), (key, h)
        w_form, w_tail, w_chain = np.maximum(w_form, ef), np.maximum(w_tail, et), np.maximum(w_chain, ec)
    assert np.all(w_form <= FORM_CAP) and np.all(w_tail <= FORM_CAP), (key, w_form, w_tail)
    assert np.all(w_chain <= CHAIN_CAP), (key, w_chain)
