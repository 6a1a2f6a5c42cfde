"""Thompson sampling on the GPU (include/spx.h: spx_thompson; csrc/ts_kernels.hip, ts_device.h) against tests/ts_oracle.py.

Shapes: the smallest at which each piece can go wrong -- N in {2, 65, 130, 257} (the 64-row tiles, the 128-row pad, the tail
kernel), D in {1, 3, 9, 33} (every register form of k_ts_prior and the one that re-reads its rows), F in {16, 48, 1024},
S in {1, 3, 17} (past one MFMA column block), M in {1, 255, 257, 1000} with a staging budget that cuts the pass into at least
three chunks, H in {1, 3}, every covar.

What is asserted:
  prior       spx_get_thompson_prior over candidates and observations against the oracle at the DERIVED bound
              (ts_oracle.prior_bound); the largest share of the bound that was used is printed (measured on an MI355X: 0.015)
  cos2pi      D = 1, F = 16, one-hot w: u is one product and one sum, bit-equal to numpy's; against 50 digits at the CPU test's
              budget of 4 ulp plus the one rounding of the scaling
  update      path - prior against the long-double route of tests/moments_ld.py on the device's own K and K*, with rhs as the
              observation vector; bar: 4 x the larger error of the two float64 reference routes (floor 16 x 2^-52), exactly as
              tests/test_gpu_q_moments_yardstick.py holds func_m -- nothing is added for the rounding of the path's last
              addition or of this test's subtraction of the prior (measured: at most 0.62 of the bar)
  bits        w = 0, eps = 0, S = 1 equals minus the LCB (kappa = 0) values of a pass over fantasies = vals; path s of an
              S-path call equals the one-path call with that column; per_draw against a handle holding the draw alone; chunks,
              streams 1 / 2 / 3, gemm_partial 0 / 1, cov_flat 0 / 1, a factorisation made by spx_ei_step, a scrambled handle
  argmin      numpy's rule on the returned path; a NaN coordinate wins as the first NaN; a duplicated row returns the first
              index; index_base is added
  state       every refusal -- range, chi, phase, each NULL pointer, fantasies held, H S Mp 8 bytes above 4 GiB, H S above 65535 --
              leaves the last pass's results readable bit for bit; no factorisation and no candidates are refused; afterwards spx_get_best refuses and an EI step
              gives the bits it gave before; new observations, hypers, candidates or a factorisation drop the paths
  choosers    a seeded next() with acq=TS of both choosers proposes what the oracle engine proposes from the same generator state
"""
import os

import numpy as np
import pytest

from spearmint_amd import engine as spx
from spearmint_amd.chooser import GPEIChooser, GPEIOptChooser
from spearmint_amd.synthetic import synthetic_problem
from tests import moments_ld as ml
from tests import ts_oracle as tso
from tests.helpers import branin
from tests.mes_helpers import same_state
from tests.pending_helpers import options
from tests.test_gpu_k_constrained_paths import plan_chunks
from tests.ts_helpers import TsOracleEngine

pytestmark = pytest.mark.gpu
SHARES = []


@pytest.fixture(scope="module")
def eng():
    e = spx.Engine(0)
    yield e
    e.set_covar("Matern52")
    e.close()


def problem(N, M, D, H, seed):
    return synthetic_problem(N, M, D, H, seed, near=min(10, M))


def padded_dim(D):
    return 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else (D + 31) // 32 * 32


def small_budget(N):
    return 8 * ((N + 127) // 128 * 128) * 128          # one 128-candidate tile of one draw per staging slot


def load(e, covar, P, step=False):
    comp, cand, vals, rows = P
    e.set_covar(covar)
    e.set_observations(comp, vals)
    e.set_candidates(cand)
    e.set_hypers(rows)
    if step:
        e.ei_step()
    else:
        e.factor()


def all_paths(e, H, S):
    return np.array([[e.thompson_path(d, s) for s in range(S)] for d in range(H)])


def check_argmin(idx, mn, paths, base=0):
    for d in range(paths.shape[0]):
        for s in range(paths.shape[1]):
            k = int(np.argmin(paths[d, s]))               # numpy's rule: the first NaN, else the first minimum
            assert idx[d, s] == base + k, (d, s, idx[d, s], k)
            assert mn[d, s] == paths[d, s][k] or (np.isnan(mn[d, s]) and np.isnan(paths[d, s][k]))


# ---- prior and paths against the oracle ---------------------------------------------------------------------------------------
CASES = [("Matern52", 2, 1, 16, 1, 1, 1, False),
         ("Matern32", 65, 3, 48, 3, 255, 3, False),
         ("ARDSE", 130, 9, 1024, 17, 1000, 3, True),
         ("SE", 257, 33, 48, 3, 257, 1, False),
         ("Matern52", 257, 3, 1024, 3, 1000, 3, False),
         ("Matern32", 130, 33, 16, 17, 255, 1, True)]


@pytest.mark.parametrize("covar,N,D,F,S,M,H,per_draw", CASES)
def test_prior_and_paths_against_the_oracle(eng, covar, N, D, F, S, M, H, per_draw):
    P = problem(N, M, D, H, 100 + N + D)
    comp, cand, vals, rows = P
    budget = small_budget(N)
    if M >= 384:
        assert plan_chunks(M, N, H, budget)[0] >= 3
    with options(eng, kstar_budget_bytes=budget):
        load(eng, covar, P)
        idx, mn, R = eng.thompson(S=S, F=F, rng=np.random.RandomState(7 + N), per_draw=per_draw)
        assert eng.stat("last_ts_paths") == S and eng.stat("last_ts_features") == F
        paths = all_paths(eng, H, S)
        check_argmin(idx, mn, paths)
        share = 0.0
        for d in range(H):
            ref, pc, po, _ = tso.paths(covar, comp, cand, vals, rows[d], R, d, per_draw, parts=True)
            nu = tso.frequencies(covar, rows[d], R["omega_z"], R["chi"])
            w, _ = tso.draw_randoms(R, d, per_draw)
            bc = tso.prior_bound(rows[d], w, nu, R["phase"], cand, padded_dim(D), tso.features(nu, R["phase"], cand))
            bo = tso.prior_bound(rows[d], w, nu, R["phase"], comp, padded_dim(D), tso.features(nu, R["phase"], comp))
            for s in range(S):
                gc, go = eng.thompson_prior(d, s)
                share = max(share, float(np.max(np.abs(gc - pc[s]) / bc[s])), float(np.max(np.abs(go - po[s]) / bo[s])))
                # the whole path: the update term is held to its yardstick below; here, that the pieces are put together
                scale = np.max(np.abs(ref[s])) + np.max(np.abs(pc[s])) + abs(rows[d][0])
                assert np.max(np.abs(paths[d, s] - ref[s])) <= 1e-8 * scale, (d, s)
    SHARES.append(share)
    print("prior %s N=%d D=%d F=%d S=%d M=%d H=%d: largest share of the bound %.4f" % (covar, N, D, F, S, M, H, share))
    assert share <= 1.0


def test_cos2pi_on_the_device(eng):
    """D = 1, F = 16, w one-hot (S = 16): p_s(x) = scale cos2pi(fl(fl(nu_s x) + phase_s) reduced).  Six features have
    frequency 0 and the phases 1/4, 3/4, 1/2, 0, 1/8, 3/8: the zeros and the ends of the range."""
    import mpmath as mp
    M, F = 1000, 16
    comp, _, vals, rows = problem(65, M, 1, 1, 5)
    cand = (np.arange(M, dtype=np.float64) / 256.0)[:, None]                 # a lattice: 0 .. 3.9
    R = spx.thompson_randoms(np.random.RandomState(4), "ARDSE", 1, 1, 65, F, 16)
    R["omega_z"][:6] = 0.0
    R["omega_z"][6:] *= 8.0
    R["phase"][:6] = [0.25, 0.75, 0.5, 0.0, 0.125, 0.375]
    R["w"] = np.eye(16)
    load(eng, "ARDSE", (comp, cand, vals, rows))
    eng.thompson(S=16, F=F, randoms=R)
    nu = tso.frequencies("ARDSE", rows[0], R["omega_z"], None)
    u = nu[:, 0][None, :] * cand + R["phase"][None, :]                         # one product, one sum
    r = u - np.rint(u)
    scale = tso.scale_of(rows[0], F)
    worst = 0.0
    with mp.workdps(50):
        for s in range(16):
            got = eng.thompson_prior(0, s)[0]
            for i in range(M):
                c = mp.mpf(0) if abs(r[i, s]) == 0.25 else mp.cos(2 * mp.pi * mp.mpf(float(r[i, s])))
                err = abs(float(mp.mpf(float(got[i])) - mp.mpf(float(scale)) * c))
                bar = tso.COS_ULPS * np.spacing(abs(float(c))) * scale + 0.5 * np.spacing(abs(got[i]))
                worst = max(worst, err / bar)
                assert err <= bar, (s, i, r[i, s], got[i], err, bar)
    assert eng.thompson_prior(0, 0)[0][0] == 0.0                               # r = 1/4: an exact zero
    print("cos2pi on the device: largest error / (4 ulp + the scaling's rounding) = %.3f" % worst)


# ---- the update term against the long-double yardstick --------------------------------------------------------------------------
@pytest.mark.parametrize("covar,N,M", [("Matern52", 65, 255), ("Matern52", 130, 1000), ("ARDSE", 257, 257)])
def test_update_term_against_long_double(eng, covar, N, M):
    assert np.finfo(np.longdouble).nmant >= 63
    H, S, F, D = 1, 3, 48, 3
    P = problem(N, M, D, H, 300 + N)
    comp, cand, vals, rows = P
    with options(eng, kstar_budget_bytes=small_budget(N)):
        load(eng, covar, P)
        _, _, R = eng.thompson(S=S, F=F, rng=np.random.RandomState(N))
        cols = ml.yardstick_columns(M)
        K = eng.get_factor(0, want_L=False, want_alpha=False)[0]
        Ks = np.ascontiguousarray(eng.get_cross_cov(0)[:, cols])
        mean = float(rows[0][0])
        worst = 0.0
        for s in range(S):
            pc, po = eng.thompson_prior(0, s)
            path = eng.thompson_path(0, s)
            rhs = (vals - po) - tso.sig_of(rows[0]) * R["eps"][s]               # k_ts_rhs, operation for operation
            args = (K, Ks, rhs - mean, mean, ml.prior_v_of(rows[0]))
            ref = ml.moments_longdouble(*args)
            e_l = ml.errors(*ml.moments_lapack(*args), ref=ref)[0]
            e_b = ml.errors(*ml.moments_as_built(*args), ref=ref)[0]
            got = (path - pc)[cols]
            dev = np.abs(got.astype(np.longdouble) - ref.m) / ref.s_m
            bar = max(4.0 * max(e_l, e_b), 16 * 2.0 ** -52)
            ratio = float(np.max(dev)) / bar
            worst = max(worst, ratio)
            print("update %s N=%d s=%d: device %.2e lapack %.2e as built %.2e, device / bar %.3f"
                  % (covar, N, s, float(np.max(dev)), e_l, e_b, ratio))
            assert ratio <= 1.0
    print("update term %s N=%d M=%d: largest device / bar %.3f" % (covar, N, M, worst))


# ---- bit-for-bit invariants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 130, 257])
def test_zero_randoms_give_the_fantasy_pass_over_the_values(eng, N):
    H = 2
    P = problem(N, 1000, 3, H, 400 + N)
    comp, cand, vals, rows = P
    load(eng, "Matern52", P)
    R = spx.thompson_randoms(np.random.RandomState(1), "Matern52", 3, H, N, 48, 1)
    R["w"][:] = 0.0
    R["eps"][:] = 0.0
    eng.thompson(S=1, F=48, randoms=R)
    paths = all_paths(eng, H, 1)
    prev = eng.get_acquisition()
    try:
        eng.set_fantasies(np.tile(vals[None, :, None], (H, 1, 1)), np.full((H, 1), vals.min()))
        eng.set_acquisition(spx.ACQ_LCB, 0.0)
        eng.ei_run()
        draws = eng.ei_draws()
    finally:
        eng.set_fantasies(None, None)
        eng.set_acquisition(*prev)
    for d in range(H):
        assert np.array_equal(paths[d, 0], -draws[:, d]), d


def test_a_path_does_not_depend_on_the_other_paths_or_draws(eng):
    N, M, D, H, S, F = 130, 1000, 3, 3, 17, 48
    P = problem(N, M, D, H, 500)
    comp, cand, vals, rows = P
    load(eng, "Matern52", P)
    R = spx.thompson_randoms(np.random.RandomState(2), "Matern52", D, H, N, F, S, per_draw=True)
    eng.thompson(S=S, F=F, randoms=R, per_draw=True)
    full = all_paths(eng, H, S)
    priors = [[eng.thompson_prior(d, s) for s in range(S)] for d in range(H)]
    # path s of the S-path call == the one-path call with that column (same handle, same draws)
    for s in (0, 15, 16):
        R1 = dict(R, w=R["w"][:, s:s + 1], eps=R["eps"][:, s:s + 1])
        eng.thompson(S=1, F=F, randoms=R1, per_draw=True)
        for d in range(H):
            assert np.array_equal(eng.thompson_path(d, 0), full[d, s]), (d, s)
            pc, po = eng.thompson_prior(d, 0)
            assert np.array_equal(pc, priors[d][s][0]) and np.array_equal(po, priors[d][s][1]), (d, s)
    # a draw's paths with per_draw == those of a handle holding that draw alone
    for d in (0, 2):
        load(eng, "Matern52", (comp, cand, vals, rows[d:d + 1]))
        Rd = dict(R, w=R["w"][d], eps=R["eps"][d])
        eng.thompson(S=S, F=F, randoms=Rd)
        assert np.array_equal(all_paths(eng, 1, S)[0], full[d]), d


def scramble(e, seed):
    """A problem of another padded size, through the same call: every buffer holds another shape."""
    P = problem(70, 300, 5, 2, seed)
    load(e, "Matern32", P)
    e.thompson(S=2, F=32, rng=np.random.RandomState(seed))


@pytest.mark.parametrize("N", [130, 257])
def test_path_variants_do_not_change_bits(eng, N):
    M, D, H, S, F = 1000, 3, 3, 3, 48
    P = problem(N, M, D, H, 600 + N)
    R = spx.thompson_randoms(np.random.RandomState(3), "Matern52", D, H, N, F, S)

    def run(step=False, **kw):
        with options(eng, **kw):
            load(eng, "Matern52", P, step=step)
            idx, mn, _ = eng.thompson(S=S, F=F, randoms=R)
            return idx, mn, all_paths(eng, H, S)
    base = run()
    budget = small_budget(N)
    assert plan_chunks(M, N, H, budget)[0] >= 3
    variants = [dict(kstar_budget_bytes=budget), dict(streams=2), dict(streams=3), dict(streams=3, kstar_budget_bytes=budget),
                dict(gemm_partial=0), dict(cov_flat=0)]
    for i, kw in enumerate(variants):
        scramble(eng, 700 + i)
        got = run(**kw)
        for a, b in zip(got, base):
            assert np.array_equal(a, b), kw
    scramble(eng, 750)
    got = run(step=True)                         # the factorisation of a preceding spx_ei_step instead of spx_factor
    for a, b in zip(got, base):
        assert np.array_equal(a, b), "step"


# ---- argmin ---------------------------------------------------------------------------------------------------------------------
def test_argmin_rules(eng):
    N, M, D, H, S, F = 65, 1000, 3, 2, 3, 48
    comp, cand, vals, rows = problem(N, M, D, H, 800)
    R = spx.thompson_randoms(np.random.RandomState(8), "Matern52", D, H, N, F, S)
    load(eng, "Matern52", (comp, cand, vals, rows))
    idx0, mn0, _ = eng.thompson(S=S, F=F, randoms=R)
    paths0 = all_paths(eng, H, S)
    check_argmin(idx0, mn0, paths0)
    # a duplicate of every path's minimiser placed BEHIND it (and one in front of another's): the first index is returned
    cand2 = cand.copy()
    k = int(idx0[0, 0])
    dup = M - 1 if k < M - 1 else M - 2
    cand2[dup] = cand2[k]
    eng.set_candidates(cand2, index_base=5000)
    idx, mn, _ = eng.thompson(S=S, F=F, randoms=R)
    paths = all_paths(eng, H, S)
    assert paths[0, 0][dup] == paths[0, 0][k]                       # (a row's value does not depend on its position)
    check_argmin(idx, mn, paths, base=5000)
    assert idx[0, 0] == 5000 + min(k, dup)
    # a candidate with a NaN coordinate wins as the first NaN, in every path
    cand3 = cand.copy()
    cand3[700, 1] = np.nan
    cand3[300, 0] = np.nan
    eng.set_candidates(cand3)
    idx, mn, _ = eng.thompson(S=S, F=F, randoms=R)
    paths = all_paths(eng, H, S)
    assert np.all(idx == 300) and np.all(np.isnan(mn))
    assert np.all(np.isnan(paths[:, :, 300])) and np.all(np.isnan(paths[:, :, 700]))
    ok = np.ones(M, dtype=bool)
    ok[[300, 700]] = False
    assert np.array_equal(paths[:, :, ok], paths0[:, :, ok])


def raw_thompson(e, R, F, S, H, null):
    """spx_thompson itself with one pointer NULL: the status."""
    import ctypes
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    keep = dict((k, np.ascontiguousarray(R[k], dtype=np.float64)) for k in ("omega_z", "chi", "phase", "w", "eps"))
    idx, mn = np.empty((H, S), dtype=np.int64), np.empty((H, S))
    ptr = dict((k, dp(v)) for k, v in keep.items())
    ptr["idx_out"], ptr["min_out"] = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), dp(mn)
    ptr[null] = None
    return e._lib.spx_thompson(e._h, F, S, ptr["omega_z"], ptr["chi"], ptr["phase"], ptr["w"], ptr["eps"], 0, ptr["idx_out"],
                               ptr["min_out"])


# ---- state ------------------------------------------------------------------------------------------------------------------------
def test_state(eng):
    N, M, D, H, S, F = 130, 257, 3, 2, 2, 32
    comp, cand, vals, rows = problem(N, M, D, H, 900)
    R = spx.thompson_randoms(np.random.RandomState(9), "Matern52", D, H, N, F, S)
    load(eng, "Matern52", (comp, cand, vals, rows))
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    before = (eng.best(), eng.ei_mean(), eng.ei_draws(), eng.get_moments(1))

    def unchanged():
        now = (eng.best(), eng.ei_mean(), eng.ei_draws(), eng.get_moments(1))
        assert now[0] == before[0] and np.array_equal(now[1], before[1]) and np.array_equal(now[2], before[2])
        assert np.array_equal(now[3][0], before[3][0]) and np.array_equal(now[3][1], before[3][1])
        assert eng.stat("last_ts_paths") == 0
    bad = [dict(F=8), dict(F=24), dict(F=8208), dict(S=0), dict(S=257),
           dict(randoms=dict(R, chi=np.where(np.arange(F) == 3, 0.0, R["chi"]))),
           dict(randoms=dict(R, chi=np.where(np.arange(F) == 3, np.inf, R["chi"]))),
           dict(randoms=dict(R, chi=np.where(np.arange(F) == 3, np.nan, R["chi"]))),
           dict(randoms=dict(R, chi=None)),
           dict(randoms=dict(R, phase=np.where(np.arange(F) == 5, 1.0, R["phase"]))),
           dict(randoms=dict(R, phase=np.where(np.arange(F) == 5, -1e-9, R["phase"])))]
    for kw in bad:
        args = dict(S=S, F=F, randoms=R)
        args.update(kw)
        if "randoms" not in kw:
            args["randoms"] = spx.thompson_randoms(np.random.RandomState(1), "Matern52", D, H, N, args["F"], args["S"])
        with pytest.raises(ValueError) as ei:
            eng.thompson(**args)
        assert "spx_thompson" in str(ei.value), kw
        unchanged()
    # a NULL pointer where one is read, on this handle while it holds the results
    for name in ("omega_z", "chi", "phase", "w", "eps", "idx_out", "min_out"):
        assert raw_thompson(eng, R, F, S, H, null=name) == spx.SPX_ERR_ARG, name
        assert "spx_thompson" in eng._lib.spx_last_error().decode() and "NULL" in eng._lib.spx_last_error().decode()
        unchanged()
    eng.set_fantasies(np.tile(vals[None, :, None], (H, 1, 1)), np.full((H, 1), vals.min()))    # fantasies held: refused
    eng.ei_run()
    fant_before = (eng.best(), eng.ei_draws())
    with pytest.raises(ValueError) as ei:
        eng.thompson(S=S, F=F, randoms=R)
    assert "fantasies" in str(ei.value)
    assert eng.best() == fant_before[0] and np.array_equal(eng.ei_draws(), fant_before[1])
    eng.set_fantasies(None, None)
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    unchanged()
    # the call: EI results are gone, paths are held; the setting is not read and stays
    eng.set_acquisition(spx.ACQ_PI, 0.25)
    eng.thompson(S=S, F=F, randoms=R)
    assert eng.get_acquisition() == (spx.ACQ_PI, 0.25)
    eng.set_acquisition(spx.ACQ_EI, 0.0)
    eng.thompson(S=S, F=F, randoms=R)
    for getter in (eng.best, eng.ei_mean, eng.ei_draws, lambda: eng.get_moments(0)):
        with pytest.raises(ValueError):
            getter()
    paths = all_paths(eng, H, S)
    with pytest.raises(ValueError):
        eng.thompson_path(H, 0)
    with pytest.raises(ValueError):
        eng.thompson_path(0, S)
    # an EI pass afterwards gives the bits it gave before; it drops the paths
    eng.ei_run(spx.FLAG_KEEP_MOMENTS)
    unchanged()
    with pytest.raises(ValueError):
        eng.thompson_path(0, 0)
    eng.ei_step(spx.FLAG_KEEP_MOMENTS)
    unchanged()
    # whatever drops a pass's results drops the paths
    for drop in (lambda: eng.set_observations(comp, vals), lambda: eng.set_hypers(rows), lambda: eng.set_candidates(cand),
                 lambda: eng.factor(), lambda: eng.set_acquisition(spx.ACQ_EI, 0.0)):
        load(eng, "Matern52", (comp, cand, vals, rows))
        eng.thompson(S=S, F=F, randoms=R)
        assert np.array_equal(eng.thompson_path(1, 1), paths[1, 1]) and eng.stat("last_ts_paths") == S
        drop()
        assert eng.stat("last_ts_paths") == 0 and eng.stat("last_ts_features") == 0
        with pytest.raises(ValueError):
            eng.thompson_path(0, 0)
    # timing: the two stages
    load(eng, "Matern52", (comp, cand, vals, rows))
    with options(eng, timing=1):
        eng.thompson(S=S, F=F, randoms=R)
        t = eng.timings()
    assert t["ts_prior"][1] >= 2 and t["ts_prior"][0] > 0.0 and t["ts_finish"][1] >= 2 and t["ts_finish"][0] > 0.0
    assert np.array_equal(all_paths(eng, H, S), paths)


def test_size_and_call_order_refusals():
    """H S Mp 8 bytes above 4 GiB (S = 256 paths over 2 097 153 candidates: one 128-candidate tile beyond 4 GiB) and H S above
    65535 are refused with the last pass's results readable bit for bit; a handle without a factorisation or without candidates
    is refused."""
    e = spx.Engine(0)
    try:
        rs = np.random.RandomState(3)
        comp, vals = rs.rand(2, 1), rs.randn(2)
        for H, M, S in ((1, 2097153, 256), (257, 5, 256)):
            cand = rs.rand(M, 1)
            rows = np.tile(np.array([[0.1, 0.01, 1.0, 0.5]]), (H, 1)) * (1.0 + 0.001 * np.arange(H))[:, None]
            load(e, "Matern52", (comp, cand, vals, rows))
            e.ei_run()
            before = (e.best(), e.ei_mean(), e.ei_draws())
            with pytest.raises(ValueError) as ei:
                e.thompson(S=S, F=16, rng=np.random.RandomState(1))
            assert "spx_thompson" in str(ei.value) and "bytes of paths" in str(ei.value)
            assert e.best() == before[0] and np.array_equal(e.ei_mean(), before[1]) and np.array_equal(e.ei_draws(), before[2])
            assert e.stat("last_ts_paths") == 0
        idx, mn, _ = e.thompson(S=255, F=16, rng=np.random.RandomState(1))          # H S = 65535: the largest grid
        assert idx.shape == (257, 255) and np.array_equal(mn[256, 254], e.thompson_path(256, 254)[idx[256, 254]])
        # call order: candidates but no factorisation; a factorisation but no candidates
        cand = rs.rand(5, 1)
        e.set_observations(comp, vals)
        e.set_candidates(cand)
        e.set_hypers(np.array([[0.1, 0.01, 1.0, 0.5]]))
        with pytest.raises(ValueError) as ei:
            e.thompson(S=1, F=16, rng=np.random.RandomState(1))
        assert "spx_factor" in str(ei.value)
    finally:
        e.close()
    f = spx.Engine(0)
    try:
        f.set_observations(comp, vals)
        f.set_hypers(np.array([[0.1, 0.01, 1.0, 0.5]]))
        f.factor()
        with pytest.raises(ValueError) as ei:
            f.thompson(S=1, F=16, rng=np.random.RandomState(1))
        assert "no candidates" in str(ei.value)
    finally:
        f.close()


# ---- choosers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pend", [0, 2])
@pytest.mark.parametrize("mod,arg", [(GPEIChooser, "mcmc_iters=3"), (GPEIOptChooser, "mcmc_iters=3,burnin=4,grid_subset=3")])
def test_choosers_propose_the_oracles_argmin(mod, arg, n_pend, golden_dir, tmp_path):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:300]
    values = np.zeros(grid.shape[0]) + np.nan
    done = np.arange(12)
    values[done] = branin(grid[done, 0], grid[done, 1])
    pend = np.arange(12, 12 + n_pend)
    free = np.arange(12 + n_pend, grid.shape[0])
    out = {}
    for name in ("gpu", "oracle"):
        d = tmp_path / name
        d.mkdir()
        ch = mod.init(str(d), arg + ",acq=TS,acq_par=64,loo=%d" % (name == "gpu"))
        if name == "oracle":
            ch._eng = TsOracleEngine()
        np.random.seed(11)
        job = ch.next(grid, values, np.zeros(grid.shape[0]), free, pend, done)
        out[name] = (job, ch.last_thompson, np.random.get_state(), ch.last_acq_used)
        if name == "gpu":
            assert ch.last_loo is not None
            ch._eng.close()
    g, o = out["gpu"], out["oracle"]
    assert g[0] == o[0] and g[3] == o[3] == "TS" and same_state(g[2], o[2])
    assert g[1]["draw"] == o[1]["draw"] and g[1]["grid_index"] == o[1]["grid_index"] and g[1]["features"] == 64
    assert abs(g[1]["path_min"] - o[1]["path_min"]) <= 1e-8 * (1.0 + abs(o[1]["path_min"]))


def test_zz_report():
    if SHARES:
        print("largest share of the prior's derived bound over all cases: %.4f" % max(SHARES))
