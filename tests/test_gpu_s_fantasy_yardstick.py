"""What spx_draw_fantasies forms (csrc/fantasy_kernels.hip: k_fant_posterior<TILED>, k_fant_fill) -- pend_m, pend_K = L_S L_S^T - noise I,
its Cholesky factor C, T = L_S^-1 C, the fantasies, bests and the tail rows of Gamma -- against the long-double yardstick of
tests/fantasy_ld.py, at P = 1 ... 64 and every (N, P) where the two kernels take another path.  Sorted after
tests/test_gpu_s_draw_fantasies.py, which holds the same kernels at 1e-9 / 1e-6 of the fantasies' scale for P <= 6 and through EI
values beyond.

(a) The two kernels alone: per case factor(), draw_fantasies(), get_pending_fantasies() and get_factor_rows(d, N, P); the
    yardstick and the two float64 forms (hostgp.fantasize_from_factor_rows: LAPACK; fantasy_helpers.factored_form: as built)
    take the ENGINE's own rows and gamma as exact inputs, under both storage forms of the factor (ei_flow 1 / 0, asserted
    from last_factor_flow), each against its own rows.  Unit, per draw: max |pend_fant - pend_m| + max |pend_m| of the yardstick.
    Bar, per draw: err_device <= max(4 x max(err_lapack_form, err_as_built_form), 16 x 2^-52) -- the factor and the floor DESIGN.md
    section 5 uses for the factorisation and the moments.
(b) pend_m and C one rounding at a time: z = [0 | 2^40 I_P].  Column 0 is pend_m exactly (unit max |pend_m|); (column q + 1 -
    column 0) 2^-40 is C[:, q] after one rounding of 2^40 C + pend_m (unit max |C|); rows above the diagonal come back as pend_m
    bit for bit.  The two float64 forms go through the same extraction; the bar is (a)'s.
(c) Exact, array_equal with equal_nan: bests is numpy's min over np.min(vals[:N]) and the device's own fantasies on every case of
    (a); a NaN and a +inf in single entries of z change their own column from that row down and nothing else; equal columns at 15
    and 16 (two workgroups of k_fant_fill) give equal results; shared z equals the same array stacked H times with per_draw = 1.
(d) Gamma's tail rows through the pass: under LCB with kappa = 0 a pass with ONE fantasy column returns -(bg + mean) = -m_s of
    every candidate exactly, so S one-column passes read the device's m_s back (the S-column pass must be np.mean of them bit for
    bit).  Held to fantasy_ld.chain_longdouble on the device's OWN K (spx_get_factor) and K* (spx_get_cross_cov) in units of
    s_m = |B[:, c]| |Gamma_s| + |mean|; bar max(4 x max(err_reference_route, err_as_built_route), 16 x 2^-52) per draw.  The
    candidates: on pending points, 1e-9 beside them, on observations, and three at 1e3 in every coordinate whose K* column is
    exactly zero and whose m_s == mean.  The same columns through spx_set_fantasies on a second engine, fed the device's
    fantasies, are held to the same bar in one S-column pass (the mean over s, in the mean of the units).

tests/test_fantasy_ld.py qualifies every problem on the CPU (both float64 forms within 2.3e-13 of the yardstick for the fantasies,
5.7e-12 for Gamma's tail, the chains within 1.9e-12; smallest pivot of pend_K 1.3e-6 amp2) and holds the yardstick itself, which
computes in double words of long double, to 40 digits (4.2e-20 against a bar of 2^-58).

Measured on an MI355X (51 tests, 11 s, most of it the double-word chains on the host).  Per group: the worst device / max(references) of a draw (bar 4); the worst errors
device; LAPACK form or reference route; as built:
  fantasies, 16 cases x 3 draws, ei_flow=1          1.22    4.3e-14; 3.6e-14; 1.2e-13
  fantasies, ei_flow=0 (row-major factor)           1.22    4.3e-14; 3.6e-14; 1.2e-13    (the two factors are the same bits)
  pend_m from z = [0 | 2^40 I], P = 1, 7, 16, 63, 64   0.19    1.7e-16; 2.2e-16; 2.9e-16    (both storage forms)
  C from the same                                   1.01    3.0e-13; 2.8e-13; 3.0e-13
  m_s through one-column LCB passes, 6 cases        1.84    1.6e-13; 3.5e-13; 3.0e-13
  the same columns through spx_set_fantasies        1.76    1.3e-13; 1.3e-13; 1.4e-13
No defect found: no product code changed.

Shown to bite, one scratch build run once and not committed: the low 16 mantissa bits of every entry of C and T cleared as
k_fant_posterior stores them to `post` (about 1.5e-11 relative).  48 of the 51 tests here fail -- all 32 cases of (a) (the fantasies at
up to 928 x the references' error, 1.8e-12 of their unit), all 10 of (b) (C at 1 060 ... 8 300 x; pend_m, which the mutation does not
touch, stays at 0.19 x), all 6 of (d) (m_s at 4.6 ... 7.4 x: Gamma's tail is a small part of |Gamma_s|, so the chain sees T only
just beyond the bar); the two exact tests of (c) and the report pass, as they must.  tests/test_gpu_s_draw_fantasies.py passes
with that build in all of its 100 tests.
"""
import numpy as np
import pytest

from tests import fantasy_ld as fl
from tests.pending_helpers import options

pytestmark = pytest.mark.gpu
LD = np.longdouble
FACTOR = 4.0
FLOOR = 16 * 2.0 ** -52
MEASURED = []             # (group, case, flow, draw, quantity, device, lapack / reference route, as built)
FLOWS = (1, 0)            # ei_flow: k_lean_flow's tile-major store, the left-looking launches' row-major one


@pytest.fixture(scope="module")
def eng():
    from spearmint_amd.engine import Engine
    assert np.finfo(LD).nmant >= 63, "the yardstick needs the 80-bit extended format"
    e = Engine(0)
    yield e
    e.set_acquisition("EI", 0.0)
    e.set_covar("Matern52")
    e.close()


def load(e, p, with_candidates=False):
    P = p.pend.shape[0]
    e.set_covar(p.covar)
    e.set_observations(np.concatenate((p.comp, p.pend)), np.concatenate((p.vals, np.zeros(P))))
    if with_candidates:
        e.set_candidates(p.cand)
    e.set_hypers(p.rows)


def factor_as(e, flow):
    e.factor()
    assert e.stat("last_factor_flow") == flow


def hold(group, case, flow, h, what, dev, ref_a, ref_b):
    """The bar, one quantity of one draw."""
    MEASURED.append((group, case, flow, h, what, dev, ref_a, ref_b))
    own = max(ref_a, ref_b)
    print("%-24s %s flow %d draw %d %-10s device %.2e references %.2e %.2e (x%.2f of the larger)"
          % (group, fl.case_id(case), flow, h, what, dev, ref_a, ref_b, dev / max(own, FLOOR / FACTOR)))
    assert dev <= max(FACTOR * own, FLOOR), (group, case, flow, h, what, dev, ref_a, ref_b)


def drawn(e, p, z, flow):
    """factor() in the given storage form and draw_fantasies(z): per draw (pend_fant, bests, l_rows, gamma)."""
    N, P = p.comp.shape[0], p.pend.shape[0]
    load(e, p)
    factor_as(e, flow)
    e.draw_fantasies(z, P)
    assert e.stat("last_fantasies_device") == 1
    out = []
    for h in range(fl.H):
        pf, bests = e.get_pending_fantasies(h)
        l_rows, gam = e.get_factor_rows(h, N, P)
        assert pf.shape == (P, z.shape[-1]) and l_rows.shape == (P, N + P)
        out.append((pf, bests, l_rows, gam))
    return out


def assert_bests(p, pf, bests):
    want = np.minimum(np.min(p.vals), np.min(pf, axis=0))
    assert np.array_equal(bests, want, equal_nan=True)


# ---- (a) the two kernels alone, (c) bests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("case", fl.CASES, ids=fl.case_id)
def test_fantasies_against_the_yardstick(eng, case, flow):
    N, P, covar, S, per_draw = case
    p = fl.case_problem(case)
    z = np.stack([fl.z_of(p, h, S, 1) for h in range(fl.H)]) if per_draw else fl.z_of(p, 0, S, 0)
    with options(eng, ei_flow=flow):
        got = drawn(eng, p, z, flow)
    for h, (pf, bests, l_rows, gam) in enumerate(got):
        mean, noise = float(p.rows[h, 0]), float(p.rows[h, 1])
        zh = fl.z_of(p, h, S, per_draw)
        assert np.all(np.isfinite(pf))
        assert_bests(p, pf, bests)
        post = fl.posterior_longdouble(p.vals, mean, noise, l_rows, gam, zh)
        lap = fl.lapack_form(p.vals, mean, noise, l_rows, gam, zh)
        built = fl.built_form(p.vals, mean, noise, l_rows, gam, zh)
        hold("fantasies, ei_flow=%d" % flow, case, flow, h, "pend_fant", fl.fant_error(pf, post), fl.fant_error(lap[0], post), fl.fant_error(built[0], post))


# ---- (b) pend_m and C, one rounding at a time -----------------------------------------------------------------------------------
def unit_columns(pf):
    """(pend_m, C) read out of the fantasies of z = [0 | 2^40 I]: column 0, and (column q + 1 - column 0) 2^-40 in long double."""
    pf = np.asarray(pf).astype(LD)
    return pf[:, 0], (pf[:, 1:] - pf[:, :1]) * LD(2.0) ** -40


@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("P", fl.UNIT_COLUMN_PS)
def test_pend_m_and_c_one_rounding_at_a_time(eng, P, flow):
    p = fl.unit_column_problem(P)
    case = (fl.UNIT_COLUMN_N, P, "Matern52", P + 1, 0)
    z = p.z[0]
    assert z.shape == (P, P + 1) and np.array_equal(z[:, 1:], 2.0 ** 40 * np.eye(P)) and not z[:, 0].any()
    with options(eng, ei_flow=flow):
        got = drawn(eng, p, z, flow)
    upper = np.triu(np.ones((P, P), dtype=bool), 1)
    for h, (pf, bests, l_rows, gam) in enumerate(got):
        mean, noise = float(p.rows[h, 0]), float(p.rows[h, 1])
        assert_bests(p, pf, bests)
        # C is lower triangular: above the diagonal the fantasies are pend_m, bit for bit
        assert np.array_equal(pf[:, 1:][upper], np.broadcast_to(pf[:, :1], (P, P))[upper]), (P, flow, h)
        post = fl.posterior_longdouble(p.vals, mean, noise, l_rows, gam, z)
        m_unit, c_unit = np.max(np.abs(post.pend_m)), np.max(np.abs(post.C))
        errs = []
        for f in (pf, fl.lapack_form(p.vals, mean, noise, l_rows, gam, z)[0], fl.built_form(p.vals, mean, noise, l_rows, gam, z)[0]):
            m, c = unit_columns(f)
            errs.append((float(np.max(np.abs(m - post.pend_m)) / m_unit), float(np.max(np.abs(c - post.C)) / c_unit)))
        hold("unit columns, ei_flow=%d" % flow, case, flow, h, "pend_m", errs[0][0], errs[1][0], errs[2][0])
        hold("unit columns, ei_flow=%d" % flow, case, flow, h, "C", errs[0][1], errs[1][1], errs[2][1])


# ---- (c) exact properties ----------------------------------------------------------------------------------------------------------
EXACT_CASE = (60, 7, "Matern52", 33, 0)


def fantasies_of(e, p, z):
    got = drawn(e, p, z, 1)
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


def test_a_nan_and_an_inf_in_z_stay_in_their_column(eng):
    """NaN at (row 3, column 20) and +inf at (row 5, column 25): columns 16 ... 31 share a workgroup of k_fant_fill."""
    p = fl.case_problem(EXACT_CASE)
    P, S = 7, 33
    z = fl.z_of(p, 0, S, 0)
    base_f, base_b = fantasies_of(eng, p, z)
    bad = z.copy()
    bad[3, 20], bad[5, 25] = np.nan, np.inf
    f, b = fantasies_of(eng, p, bad)
    others = np.setdiff1d(np.arange(S), [20, 25])
    assert np.array_equal(f[:, :, others], base_f[:, :, others]) and np.array_equal(b[:, others], base_b[:, others])
    assert np.array_equal(f[:, :3, 20], base_f[:, :3, 20]) and np.all(np.isnan(f[:, 3:, 20])) and np.all(np.isnan(b[:, 20]))
    assert np.array_equal(f[:, :5, 25], base_f[:, :5, 25]) and np.all(f[:, 5, 25] == np.inf)
    for h in range(fl.H):
        assert_bests(p, f[h], b[h])


def test_equal_columns_in_two_workgroups_and_shared_against_stacked_normals(eng):
    p = fl.case_problem(EXACT_CASE)
    z = fl.z_of(p, 0, 33, 0)
    z[:, 16] = z[:, 15]
    f, b = fantasies_of(eng, p, z)
    assert np.array_equal(f[:, :, 15], f[:, :, 16]) and np.array_equal(b[:, 15], b[:, 16])
    assert not np.array_equal(f[:, :, 14], f[:, :, 15])
    f2, b2 = fantasies_of(eng, p, np.stack([z] * fl.H))
    assert np.array_equal(f2, f) and np.array_equal(b2, b)
    own = np.stack([fl.z_of(p, h, 33, 1) for h in range(fl.H)])                 # and the draws really read their own
    f3, _ = fantasies_of(eng, p, own)
    assert not np.array_equal(f3[1], f[1])


# ---- (d) Gamma's tail rows, through the pass --------------------------------------------------------------------------------------
def chain_pass(e, p, flow):
    """LCB with kappa = 0: S one-column passes give the device's m_s [H][S][M]; the S-column pass must be np.mean of them.  Also
    per draw the device's K, K*, fantasies and bests."""
    N, P, S, M = p.comp.shape[0], p.pend.shape[0], fl.CHAIN_S, p.cand.shape[0]
    z = np.stack([fl.z_of(p, h, S, 1) for h in range(fl.H)])
    load(e, p, with_candidates=True)
    e.set_acquisition("LCB", 0.0)
    factor_as(e, flow)
    A = np.empty((M, fl.H, S))
    for s in range(S):
        e.draw_fantasies(np.ascontiguousarray(z[:, :, s:s + 1]), P)
        e.ei_run(0)
        assert e.stat("last_step_fused") == 0
        A[:, :, s] = e.ei_draws()
    e.draw_fantasies(z, P)
    e.ei_run(0)
    whole = e.ei_draws()
    want = np.stack([np.mean(np.ascontiguousarray(A[:, h, :]), axis=1) for h in range(fl.H)], axis=1)
    assert np.array_equal(whole, want), "the S-column pass is not the mean of the one-column passes"
    assert not np.array_equal(A[:, :, 0], A[:, :, 1])
    out = []
    for h in range(fl.H):
        pf, bests = e.get_pending_fantasies(h)
        K = e.get_factor(h, want_L=False, want_alpha=False)[0]
        out.append((-A[:, h, :].T, K, e.get_cross_cov(h), pf, bests))
    return z, out


def chain_cases():
    return [(c, 1) for c in fl.CHAIN_CASES] + [(fl.CHAIN_STORAGE, 0)]


@pytest.mark.parametrize("case,flow", chain_cases(), ids=lambda v: fl.case_id(v) if isinstance(v, tuple) else "flow%d" % v)
def test_conditional_means_against_the_chain(eng, case, flow):
    from spearmint_amd.engine import Engine
    p = fl.case_problem(case)
    N, P, S = p.comp.shape[0], p.pend.shape[0], fl.CHAIN_S
    far = fl.far_columns(p)
    try:
        with options(eng, ei_flow=flow):
            z, got = chain_pass(eng, p, flow)
    finally:
        eng.set_acquisition("EI", 0.0)
    # the existing path beside it: the device's fantasies through spx_set_fantasies on a second engine, one S-column pass
    second = Engine(0)
    try:
        load(second, p, with_candidates=True)
        second.set_acquisition("LCB", 0.0)
        with options(second, ei_flow=flow):
            factor_as(second, flow)
            top = np.tile(p.vals[None, :, None], (fl.H, 1, S))
            second.set_fantasies(np.ascontiguousarray(np.concatenate((top, np.array([g[3] for g in got])), axis=1)),
                                 np.ascontiguousarray(np.array([g[4] for g in got])))
            second.ei_run(0)
            assert second.stat("last_fantasies_device") == 0
            host_path = -second.ei_draws()                                  # (M, H): the mean over s of m_s
    finally:
        second.close()
    for h, (m_dev, K, Ks, pf, bests) in enumerate(got):
        mean, noise = float(p.rows[h, 0]), float(p.rows[h, 1])
        assert K.shape == (N + P, N + P) and Ks.shape == (N + P, p.cand.shape[0]) and np.all(np.isfinite(m_dev))
        assert np.array_equal(Ks[:, far], np.zeros((N + P, len(far))))
        assert np.array_equal(m_dev[:, far], np.full((S, len(far)), mean)), (case, flow, h)
        assert np.array_equal(host_path[far, h], np.full(len(far), -np.mean(np.full(S, -mean)))), (case, flow, h)
        chain = fl.chain_longdouble(K, Ks, p.vals, mean, noise, fl.prior_v_of(p.rows[h]), z[h], P)
        ref = fl.chain_reference_route(K, Ks, p.vals, mean, noise, z[h], P)
        built = fl.chain_as_built(K, Ks, p.vals, mean, noise, z[h], P)
        hold("chain", case, flow, h, "m_s", fl.chain_error(m_dev, chain), fl.chain_error(ref, chain), fl.chain_error(built, chain))
        mean_m, mean_unit = np.mean(chain.m, axis=0), np.mean(chain.s_m, axis=0)

        def mean_error(m):
            return float(np.max(np.abs(np.asarray(m).astype(LD) - mean_m) / mean_unit))
        hold("set_fantasies", case, flow, h, "mean m_s", mean_error(host_path[:, h]), mean_error(np.mean(ref, axis=0)),
             mean_error(np.mean(built, axis=0)))


# ---- what was measured ------------------------------------------------------------------------------------------------------------
def test_zz_report_the_measured_ratios():
    """Per group and quantity: the worst device / max(references) of a draw, and the three worst errors."""
    assert MEASURED, "no yardstick case ran before the report"
    seen = []
    for m in MEASURED:
        if (m[0], m[4]) not in seen:
            seen.append((m[0], m[4]))
    for group, what in seen:
        rows = [m for m in MEASURED if (m[0], m[4]) == (group, what)]
        ratio = max(m[5] / max(m[6], m[7], FLOOR / FACTOR) for m in rows)
        print("%-24s %-10s %3d draws: worst ratio %.2f (bar %.0f); worst errors device %.1e; lapack / reference route %.1e; as built %.1e"
              % (group, what, len(rows), ratio, FACTOR, max(m[5] for m in rows), max(m[6] for m in rows), max(m[7] for m in rows)))
