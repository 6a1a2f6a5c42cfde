"""The acquisitions beside EI (include/spx.h: spx_set_acquisition -- probability of improvement, the negated lower
confidence bound) and the choosers' model-mean recommendation, on the GPU: parity with the float64 oracle
(tests/acq_oracle.py) at the shapes where the pass changes path, over pending fantasies, bit for bit across execution
paths / the multi-device handle / a group of ranks, EI left exactly as it was, the refinement objective, the tails
against the 50-digit reference (tests/golden/acq_tail_mp.npz), the handle's state machine and every refusal, and the
choosers' acq= / recommend= arguments against a host run.  Sorted after the other GPU files on purpose: when an EI test
and one of these fail together, read the EI one first."""
import functools
import os

import numpy as np
import numpy.random as npr
import pytest

from oracle import gp_ei_oracle as orc
from spearmint_amd import engine as spx
from spearmint_amd.synthetic import synthetic_problem
from tests import acq_mp as am
from tests import acq_oracle as ao
from tests import pending_helpers as ph
from tests import refine_helpers as rh
from tests.acq_helpers import host_opt_next
from tests.constrained_refine_helpers import assert_close, central_differences
from tests.pending_helpers import FLAG_KEEP_MOMENTS, FLAG_PER_SEC, FLAG_TIME_ONLY, options
from tests.test_gpu_a_parity import EI_RTOL, assert_ei_close
from tests.test_gpu_k_constrained_paths import assert_same, plan_chunks
from tests.test_gpu_n_pending_paths import FANT_RTOL

pytestmark = pytest.mark.gpu
FLAG_CONSTRAINED = 16
ACQS = [(ao.PI, 0.0), (ao.PI, 0.01), (ao.LCB, 0.0), (ao.LCB, 2.0)]
FLOOR = 16 * np.finfo(float).eps      # 3.6e-15: a band where the oracle happens to be exact is not an impossible bar
# Hundreds of observations packed on the unit INTERVAL (D = 1) are the ill-conditioned family of tests/test_gpu_e_illcond.py:
# at (N, D) = (257, 1) cond(K) is 1.7e6 and the float64 oracle itself is 2.4e-8 away from an 80-bit restatement of the same
# formulas.  LCB is linear in the moments and keeps EI_RTOL there.  PI = Phi(u) and EI carry the error du of
# u = (best - func_m) / func_s multiplied by |d log Phi / du| ~ |u + 1 / u| and |d log EI / du| ~ |u + 2 / u|: the same factor
# to 1 / u^2.  So at that one shape PI is held to the DEVICE'S OWN EI error on the same problem -- at most twice its maximum --
# and only where the amplification can explain a miss of EI_RTOL: an entry with |u| < 20 (du would have to exceed 1e-7 / 20,
# a thousand times the moments' error) stays at EI_RTOL.  The family's bar of tests/test_gpu_e_illcond.py caps it all.
ILLCOND_RTOL = 2e-6
ILLCOND_U = 20.0


@pytest.fixture()
def eng():
    e = spx.Engine(0)
    yield e
    e.close()


def collect(e):
    return {"draws": e.ei_draws(), "mean": e.ei_mean(), "best": e.best()}


def assert_acq_close(kind, par, got, ref, func_m, func_s, rtol):
    """PI: EI's own rule (relative, NaN positions equal, below 1e-280 small).  LCB cancels: |got - ref| against rtol times
    (|func_m| + kappa func_s)."""
    if kind == ao.PI:
        return assert_ei_close(got, ref, rtol=rtol)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    ok = np.isfinite(ref)
    scale = np.abs(func_m) + par * func_s
    assert np.all(np.abs(got[ok] - ref[ok]) <= rtol * scale[ok]), float(np.max(np.abs(got[ok] - ref[ok]) / scale[ok]))


def run_plain(e, comp, vals, cand, hypers, kind, par, covar="Matern52", entry="step", flags=0):
    e.set_covar(covar)
    e.set_observations(comp, vals); e.set_candidates(cand); e.set_hypers(hypers)
    e.set_acquisition(kind, par)
    if entry == "step":
        e.ei_step(flags)
    else:
        e.factor()
        e.ei_run(flags)
    return collect(e)


def check_plain(e, comp, vals, cand, hypers, covar="Matern52", fused=None):
    """All four acquisitions of one problem against the oracle: every value, numpy's mean over draws, the winner."""
    with orc.covar(covar), np.errstate(all="ignore"):
        mom = [ao.moments(comp, cand, vals, h) for h in hypers]
    func_m = np.stack([m[0] for m in mom], axis=1)
    func_v = np.stack([m[1] for m in mom], axis=1)
    with np.errstate(all="ignore"):
        func_s = np.sqrt(func_v)
    for kind, par in ACQS:
        ref = ao.value(kind, par, func_m, func_v, np.min(vals))
        res = run_plain(e, comp, vals, cand, hypers, kind, par, covar)
        if fused is not None:
            assert e.stat("last_step_fused") == int(fused)
        assert_acq_close(kind, par, res["draws"], ref, func_m, func_s, EI_RTOL)
        assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1), equal_nan=True)
        assert res["best"][0] == ao.choose(ref), (kind, par)
        assert res["best"][1] == res["mean"][res["best"][0]] or np.isnan(res["best"][1])
        assert e.get_acquisition() == (kind, par)


# ---- 1. parity with the oracle ------------------------------------------------------------------------------------------
#          (N, M, D, H), one thing varied at a time: the fused path (N <= 128) and its boundary, the 64-row factor tiles, the
#          GEMM tail; M around the 128-candidate tile; one draw; D = 1 and 9 (the Dp padding)
SHAPES = ([(n, 700, 3, 3) for n in (2, 64, 65, 128, 129, 257)]
          + [(n, m, 3, 3) for n in (65, 257) for m in (1, 127, 128, 129)]
          + [(65, 700, 3, 1), (257, 700, 3, 1)] + [(n, 700, d, 3) for n in (65, 257) for d in (1, 9)])


@pytest.mark.parametrize("N,M,D,H", SHAPES)
def test_shapes_match_oracle(eng, N, M, D, H):
    comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 9000 + 7 * N + 3 * M + D + H, near=min(10, M))
    if not (D == 1 and N > 128):
        return check_plain(eng, comp, vals, cand, hypers, fused=N <= 128)
    # the ill-conditioned shape (the comment at ILLCOND_RTOL): LCB at EI_RTOL, PI against the device's own EI error
    with orc.covar("Matern52"), np.errstate(all="ignore"):
        ei_ref = orc.ei_over_hypers(comp, cand, vals, hypers)
        mom = [ao.moments(comp, cand, vals, h) for h in hypers]
    func_m, func_v = np.stack([m[0] for m in mom], axis=1), np.stack([m[1] for m in mom], axis=1)
    func_s = np.sqrt(func_v)
    ei_got = run_plain(eng, comp, vals, cand, hypers, ao.EI, 0.0)["draws"]
    big = ei_ref >= 1e-280
    ei_err = float(np.max(np.abs(ei_got[big] - ei_ref[big]) / ei_ref[big]))
    print("N %d D 1: EI max relative error %.3g" % (N, ei_err))
    assert np.array_equal(np.isnan(ei_got), np.isnan(ei_ref)) and ei_err <= ILLCOND_RTOL
    for kind, par in ACQS:
        ref = ao.value(kind, par, func_m, func_v, np.min(vals))
        res = run_plain(eng, comp, vals, cand, hypers, kind, par)
        assert eng.stat("last_step_fused") == 0
        if kind == ao.LCB:
            assert_acq_close(kind, par, res["draws"], ref, func_m, func_s, EI_RTOL)
        else:
            assert np.array_equal(np.isnan(res["draws"]), np.isnan(ref))
            u = (np.min(vals) - par - func_m) / func_s
            big = ref >= 1e-280
            err = np.abs(res["draws"][big] - ref[big]) / ref[big]
            print("N %d D 1: PI(%g) max relative error %.3g, %d of %d entries above %g, the largest |u| below %g among them: %s"
                  % (N, par, float(err.max()), int(np.sum(err > EI_RTOL)), err.size, EI_RTOL, ILLCOND_U,
                     float(np.max(err[np.abs(u[big]) < ILLCOND_U]))))
            assert err.max() <= min(max(EI_RTOL, 2 * ei_err), ILLCOND_RTOL)
            assert np.all(err[np.abs(u[big]) < ILLCOND_U] <= EI_RTOL)
            assert np.all(res["draws"][np.isfinite(ref) & ~big] <= 1e-270)
        assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1), equal_nan=True)
        assert res["best"][0] == ao.choose(ref), (kind, par)


@pytest.mark.parametrize("N", [65, 257])
@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE", "SE"])
def test_every_covar(eng, covar, N):
    comp, cand, vals, hypers = synthetic_problem(N, 700, 3, 3, 9100 + N + len(covar))
    check_plain(eng, comp, vals, cand, hypers, covar=covar)


def test_three_stage_path_at_small_n_equals_the_fused_one(eng):
    """ei_fused on and off at N <= 128: the same sums in the same order, so the same bits, for every acquisition."""
    comp, cand, vals, hypers = synthetic_problem(100, 3000, 4, 3, 9200)
    for kind, par in ACQS:
        with options(eng, ei_fused=1):
            a = run_plain(eng, comp, vals, cand, hypers, kind, par)
            assert eng.stat("last_step_fused") == 1
        with options(eng, ei_fused=0):
            b = run_plain(eng, comp, vals, cand, hypers, kind, par)
            assert eng.stat("last_step_fused") == 0
        assert_same(a, b, (kind, par))


# ---- 2. pending fantasies -------------------------------------------------------------------------------------------------
def fant_scale(p, cand, par):
    """mean over S of |func_m_s| + kappa func_s per (candidate, draw): the size of what LCB's mean over S is made of."""
    out = np.empty((cand.shape[0], p.H))
    with orc.covar(p.covar):
        for h in range(p.H):
            m = -ao.fantasy_values(ao.LCB, 0.0, p.X, cand, p.rows[h], p.fant[h], p.bests[h])
            s = ao.fantasy_values(ao.LCB, 1.0, p.X, cand, p.rows[h], p.fant[h], p.bests[h]) + m
            out[:, h] = np.mean(np.abs(m), axis=1) + par * np.mean(s, axis=1)
    return out


def run_fant(e, p, cand, kind, par, device=False, entry="factor"):
    ph.load(e, p, cand)
    e.set_acquisition(kind, par)
    if entry == "step":
        e.ei_step(0)
    else:
        e.factor()
    if device:
        e.draw_fantasies(p.randn, p.pend.shape[0])
    else:
        e.set_fantasies(p.fant, p.bests)
    e.ei_run(0)
    return collect(e)


@pytest.mark.parametrize("n_rows", [70, 200])
@pytest.mark.parametrize("S", [1, 5, 130])
def test_fantasies_match_oracle(eng, S, n_rows):
    """spx_set_fantasies with the oracle's own columns, and spx_draw_fantasies from the same normals: PI of every fantasy
    against bests[s], LCB with func_m_s, averaged over S."""
    p = ph.problem(9300 + S + n_rows, N=n_rows, D=3, H=3, S=S)
    cand = ph.candidates(p, S, 700)
    for kind, par in ACQS:
        with orc.covar(p.covar):
            ref = ao.over_hypers_fantasies(kind, par, p.X, cand, p.rows, p.fant, p.bests)
        scale = fant_scale(p, cand, par)
        for device in (False, True):
            res = run_fant(eng, p, cand, kind, par, device=device)
            assert eng.stat("last_step_fused") == 0
            assert_acq_close(kind, par, res["draws"], ref, scale, 0.0 * scale, FANT_RTOL)
            assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1))
            assert res["best"][0] == ao.choose(ref), (kind, par, device)


@pytest.mark.parametrize("S", [5, 130])
def test_mean_over_fantasies_is_numpys(eng, S):
    """tests/test_gpu_n_pending_paths.py's argument for EI: a pass with ONE column returns that column's value exactly, so S
    one-column passes give A[M, H, S] and the S-column pass must return np.mean(A[:, h, :], axis=1) bit for bit."""
    H, M = 2, 300
    p = ph.problem(9400 + S, N=135, D=3, H=H, S=S)
    cand = ph.candidates(p, S, M)
    for kind, par in ((ao.PI, 0.01), (ao.LCB, 2.0)):
        ph.load(eng, p, cand)
        eng.set_acquisition(kind, par)
        eng.factor()
        A = np.empty((M, H, S))
        for s in range(S):
            q = ph.with_columns(p, s, s + 1)
            eng.set_fantasies(q.fant, q.bests)
            eng.ei_run(0)
            A[:, :, s] = eng.ei_draws()
        want = np.stack([np.mean(np.ascontiguousarray(A[:, h, :]), axis=1) for h in range(H)], axis=1)
        budget = 8 * 256 * 128
        assert plan_chunks(M, 135, H, budget) == (3, 1)
        for kw in (dict(), dict(kstar_budget_bytes=budget)):
            with options(eng, **kw):
                got = run_fant(eng, p, cand, kind, par)
            assert np.array_equal(got["draws"], want), (kind, S, sorted(kw))
        assert not np.array_equal(A[:, :, 0], A[:, :, 1])


# ---- 3. execution paths, bit for bit, on bases anchored to the oracle --------------------------------------------------------
#          name: (N, M, D, H, small staging budget)
#          "padded": 200 rows leave 5 live 16-row tiles in the last row block, so the predict GEMM skips its padding
#          (ph.padding_plan) unless gemm_partial = 0 says no; "general" (247: 8 live tiles) and "fused" have nothing to skip
BASES = {"general": (247, 5000, 3, 5, 256 * 1024 * 8), "fused": (100, 5000, 4, 5, 128 * 1024 * 8),
         "padded": (200, 5000, 3, 5, 256 * 1024 * 8)}
SKIPS = {"general": False, "fused": False, "padded": True}
PATH_ACQS = [(ao.PI, 0.01), (ao.LCB, 2.0)]


@functools.lru_cache(maxsize=None)
def base_problem(name):
    N, M, D, H, budget = BASES[name]
    return synthetic_problem(N, M, D, H, 9500 + N) + (budget,)


def default_run(e, name, kind, par):
    comp, cand, vals, hypers, budget = base_problem(name)
    with orc.covar("Matern52"):
        ref, mom = ao.over_hypers(kind, par, comp, cand, vals, hypers, want_moments=True)
    base = run_plain(e, comp, vals, cand, hypers, kind, par)
    assert e.stat("last_step_fused") == int(name == "fused")
    assert ph.padding_plan(comp.shape[0])[1] == SKIPS[name]
    assert e.stat("last_step_skipped_padding") == int(SKIPS[name])
    func_m = np.stack([m[0] for m in mom], axis=1)
    assert_acq_close(kind, par, base["draws"], ref, func_m, np.sqrt(np.stack([m[1] for m in mom], axis=1)), EI_RTOL)
    assert base["best"][0] == ao.choose(ref)
    nchunks, hb = plan_chunks(cand.shape[0], comp.shape[0], hypers.shape[0], budget)
    assert nchunks >= 5 and hb == 1, (nchunks, hb)
    return comp, cand, vals, hypers, budget, base


def scramble_plain(e, comp, vals, cand, hypers, kind, par):
    """A pass on other data of the same sizes, so that every buffer the next pass should write holds wrong values of the
    right shape: a variant that skips a store cannot pass on what the run before it left behind."""
    run_plain(e, comp[::-1].copy(), vals[::-1] * 1.1, cand[::-1].copy(), hypers[::-1] * 1.05, kind, par)


VARIANTS = {"chunks": dict(kstar_budget_bytes=True), "streams2": dict(streams=2),
            "streams2+chunks": dict(streams=2, kstar_budget_bytes=True), "gemm_partial0": dict(gemm_partial=0),
            "gemm_partial1": dict(gemm_partial=1), "gemm_partial1+chunks": dict(gemm_partial=1, kstar_budget_bytes=True),
            "gemm_partial0+chunks": dict(gemm_partial=0, kstar_budget_bytes=True), "gemm_partial0+streams2": dict(gemm_partial=0, streams=2),
            "ei_fused0": dict(ei_fused=0), "ei_fused1": dict(ei_fused=1), "ei_fused0+chunks": dict(ei_fused=0, kstar_budget_bytes=True)}


@pytest.mark.parametrize("kind,par", PATH_ACQS)
@pytest.mark.parametrize("name", sorted(BASES))
def test_path_variants_do_not_change_bits(eng, name, kind, par):
    """Five or more chunks with one draw per group, a second stream, the GEMM's padding skip and the fused form on and off,
    spx_factor + spx_ei_run against spx_ei_step: the default pass's bits."""
    comp, cand, vals, hypers, budget, base = default_run(eng, name, kind, par)
    for variant in sorted(VARIANTS):
        kw = dict(VARIANTS[variant])
        if kw.get("kstar_budget_bytes"):
            kw["kstar_budget_bytes"] = budget
        for entry in ("step", "factor"):
            scramble_plain(eng, comp, vals, cand, hypers, kind, par)
            with options(eng, **kw):
                got = run_plain(eng, comp, vals, cand, hypers, kind, par, entry=entry)
                fused = eng.stat("last_step_fused")
                skipped = eng.stat("last_step_skipped_padding")
            assert fused == int(kw.get("ei_fused", 1) != 0 and name == "fused")
            # the padding is skipped exactly where the plan has something to skip, the pass runs the GEMM and the option allows it
            three_stage_skips = ph.padding_plan(comp.shape[0])[1] and not fused
            assert skipped == int(three_stage_skips and kw.get("gemm_partial", 1) != 0), (name, variant, entry)
            assert_same(got, base, (name, variant, entry))


@pytest.mark.parametrize("kind,par", PATH_ACQS)
@pytest.mark.parametrize("n_rows", [247, 200])
def test_fantasy_path_variants_do_not_change_bits(eng, n_rows, kind, par):
    """The same with pending fantasies (never fused); 200 resident rows: the GEMM's fantasy epilogue with the padding skipped."""
    p = ph.problem(9600 + n_rows, N=n_rows, D=3, H=5, S=12, n_pend=4)
    cand = ph.candidates(p, 9, 5000)
    budget = 256 * 1024 * 8
    nchunks, hb = plan_chunks(5000, n_rows, 5, budget)
    assert nchunks >= 5 and hb == 1
    skips = ph.padding_plan(n_rows)[1]
    assert skips == (n_rows == 200)
    base = run_fant(eng, p, cand, kind, par)
    assert eng.stat("last_step_skipped_padding") == int(skips)
    for kw in (dict(kstar_budget_bytes=budget), dict(streams=2), dict(streams=2, kstar_budget_bytes=budget), dict(gemm_partial=0),
               dict(gemm_partial=1), dict(gemm_partial=1, kstar_budget_bytes=budget), dict(gemm_partial=0, kstar_budget_bytes=budget)):
        for entry in ("factor", "step"):
            ph.scramble(eng, p, cand)
            with options(eng, **kw):
                got = run_fant(eng, p, cand, kind, par, entry=entry)
                assert eng.stat("last_step_fused") == 0
                assert eng.stat("last_step_skipped_padding") == int(skips and kw.get("gemm_partial", 1) != 0)
            assert_same(got, base, (sorted(kw), entry))


def _emulate_2d(e, comp, vals, cand, hypers, n, nph, kind, par):
    """tests/test_gpu_d_multi.py::_emulate_2d with the acquisition set: every (candidate shard, draw shard) block on a
    one-GPU engine, np.sum over the block's draws, the zero-padded M-vectors added in rank order."""
    from spearmint_amd import dist as sd
    M, H = cand.shape[0], hypers.shape[0]
    full = np.zeros(M)
    blocks = np.zeros((M, H))
    for r in range(n):
        (c0, c1), (h0, h1) = sd.shard_2d(M, H, n, r, nph)
        a = run_plain(e, comp, vals, cand[c0:c1], hypers[h0:h1], kind, par)["draws"]
        blocks[c0:c1, h0:h1] = a
        part = np.zeros(M)
        part[c0:c1] = np.sum(a, axis=1)
        full = part if r == 0 else full + part
    mean = full / float(H)
    return int(np.argmax(mean)), mean, blocks


@pytest.mark.parametrize("kind,par", PATH_ACQS)
def test_multi_device_handle_and_2d_partition(eng, kind, par):
    """MultiEngine([0, 0]): the setting reaches every device slot, and the results are the one-GPU handle's bit for bit.
    The 2-D partition: per-draw values bit for bit, the mean equal to the rank-order emulation bit for bit and to the
    one-GPU mean within the rounding of a sum taken in another order (1e-14 of the mean size of its terms: PI's terms have
    one sign, LCB's need not)."""
    comp, cand, vals, hypers = synthetic_problem(150, 2111, 5, 6, 9700)
    one = run_plain(eng, comp, vals, cand, hypers, kind, par)
    me = spx.MultiEngine([0, 0])
    try:
        many = run_plain(me, comp, vals, cand, hypers, kind, par)
        assert me.get_acquisition() == (kind, par)
        assert_same(many, one, "multi")
        pts = cand[:5]
        eng.factor(); me.factor()
        f1, g1 = eng.ei_grad_batch(pts)
        f2, g2 = me.ei_grad_batch(pts)
        assert np.array_equal(f1, f2) and np.array_equal(g1, g2)
        me.set_partition(2)
        me.set_observations(comp, vals); me.set_hypers(hypers); me.set_candidates(cand)
        me.factor(); me.ei_run()
        idx, mean, blocks = _emulate_2d(eng, comp, vals, cand, hypers, 2, 2, kind, par)
        assert me.best() == (idx, mean[idx]) and np.array_equal(me.ei_mean(), mean)
        assert np.array_equal(me.ei_draws(), blocks) and np.array_equal(blocks, one["draws"])
        assert idx == one["best"][0]
        assert np.all(np.abs(me.ei_mean() - one["mean"]) <= 1e-14 * np.mean(np.abs(one["draws"]), axis=1))
        # a new setting drops the front's results too
        me.set_acquisition(spx.ACQ_EI)
        with pytest.raises(ValueError):
            me.best()
    finally:
        me.close()


def _attach_case(P, kind, par):
    import threading
    from spearmint_amd import dist as sd
    comp, cand, vals, hypers = synthetic_problem(180, 4003, 6, 6, 9800)
    M, H = cand.shape[0], hypers.shape[0]
    e0 = spx.Engine(0)
    one = run_plain(e0, comp, vals, cand, hypers, kind, par)
    uid = e0.comm_unique_id()
    res, errs = [None] * P, [None] * P

    def rank_main(r):
        try:
            e = spx.Engine(0)
            e.comm_attach(uid, P, r)
            c0, c1 = sd.shard_bounds(M, P, r)
            e.set_acquisition(kind, par)
            e.set_observations(comp, vals); e.set_hypers(hypers); e.set_candidates(cand[c0:c1], index_base=c0)
            e.ei_step(0)
            res[r] = (e.best(), e.stat("ranks_seen"), e.ei_mean(), (c0, c1))
            e.close()
        except BaseException as ex:
            errs[r] = "%s: %s" % (type(ex).__name__, ex)

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    out = {"errors": [x for x in errs if x], "alive": any(t.is_alive() for t in th)}
    if not out["errors"] and not out["alive"]:
        out["ranks_seen"] = [r[1] for r in res]
        out["winner_bits"] = all(r[0] == one["best"] for r in res)
        out["mean_bits"] = all(np.array_equal(r[2], one["mean"][r[3][0]:r[3][1]]) for r in res)
    e0.close()
    return out


@pytest.mark.parametrize("kind,par", PATH_ACQS)
def test_group_of_ranks_through_the_stand_in_rccl(kind, par):
    """Four ranks, one per host thread, attached through tests/c/fake_rccl.hip (tests/test_gpu_d2_fake_rccl.py): every
    rank sets the acquisition on its own handle; the record all-gather returns the one-GPU winner, bit for bit."""
    from tests.test_gpu_d2_fake_rccl import _in_child
    out = _in_child(_attach_case, 4, kind, par)
    assert not out["errors"] and not out["alive"], out
    assert out["ranks_seen"] == [4] * 4 and out["winner_bits"] and out["mean_bits"], out


# ---- 4. EI is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,fant", [(100, False), (257, False), (200, True)])
def test_ei_is_untouched(N, fant):
    """A handle that never heard of the setting, one that set SPX_ACQ_EI, one that went EI -> PI -> EI (with a PI pass and a
    PI refinement call in between): draws, mean, winner and spx_ei_grad_batch's output, element by element."""
    if fant:
        p = ph.problem(9900, N=N, D=3, H=3, S=7)
        cand = ph.candidates(p, 3, 1500)
        pts = rh.points(p, 2, n=5)

        def go(e, kind, par):
            res = run_fant(e, p, cand, kind, par)
            return res, e.ei_grad_batch(pts)
    else:
        comp, cand, vals, hypers = synthetic_problem(N, 1500, 4, 3, 9900 + N)
        pts = cand[:5].copy()

        def go(e, kind, par):
            res = run_plain(e, comp, vals, cand, hypers, kind, par)
            return res, e.ei_grad_batch(pts)
    out = []
    for mode in ("never", "set", "round_trip"):
        e = spx.Engine(0)
        try:
            if mode == "never":
                e.set_acquisition = lambda kind, par=0.0: None
            if mode == "round_trip":
                a, _ = go(e, ao.PI, 0.01)
                assert not np.array_equal(a["draws"], a["draws"] * 0)
            out.append(go(e, ao.EI, 0.0))
            if mode != "never":
                assert e.get_acquisition() == (spx.ACQ_EI, 0.0)
        finally:
            e.close()
    for res, (f, g) in out[1:]:
        assert_same(res, out[0][0])
        assert np.array_equal(f, out[0][1][0]) and np.array_equal(g, out[0][1][1])


# ---- 5. the refinement objective -------------------------------------------------------------------------------------------
def refine_setup(e, p, kind, par):
    rh.setup(e, p)
    e.set_acquisition(kind, par)


#          (N rows resident, D, H, S), one thing varied at a time; S = 0: no fantasies
REFINE_SHAPES = ([(n, 3, 3, s) for n in (2, 64, 65, 129, 257) for s in (0, 5)] + [(150, d, 3, s) for d in (1, 8, 9) for s in (0, 5)]
                 + [(150, 3, 3, 1), (150, 3, 1, 0)])


@pytest.mark.parametrize("N,D,H,S", REFINE_SHAPES)
def test_refinement_objective_matches_oracle(eng, N, D, H, S):
    """spx_ei_grad_batch for PI and LCB against the oracle's value and gradient at the tolerances its EI tests use
    (tests/constrained_refine_helpers.assert_close), for 1 and 5 points per call."""
    p = rh.make_problem(10000 + 7 * N + 3 * D + H + S, branch="fant" if S else "plain", N=N, D=D, H=H, S=max(S, 1))
    pts = rh.points(p, N + D, n=5)
    for kind, par in ACQS:
        refine_setup(eng, p, kind, par)
        f_ref, g_ref = ao.grad_oracle(p, pts, kind, par)
        for P in (1, 5):
            f, g = eng.ei_grad_batch(pts[:P])
            assert_close(f, g, f_ref[:P], g_ref[:P])


@pytest.mark.parametrize("covar", rh.COVARS)
@pytest.mark.parametrize("branch", ["plain", "fant"])
def test_refinement_central_differences(eng, covar, branch):
    """The gradient against central differences of the returned value, at the bar of
    tests/test_gpu_m_refine_paths.py::test_central_differences (rtol 2e-3, atol 1e-9)."""
    p = rh.make_problem(10100 + len(covar), covar=covar, branch=branch, N=150, D=4, H=3, S=5)
    for kind, par in ACQS:
        refine_setup(eng, p, kind, par)
        for x in rh.points(p, 4, n=2):
            _, g = eng.ei_grad_batch(x[None])
            fd = central_differences(lambda y: eng.ei_grad_batch(y[None])[0][0], x, range(p.D))
            assert np.allclose(fd, g[0], rtol=2e-3, atol=1e-9), (covar, branch, kind, par, fd, g[0])


@pytest.mark.parametrize("branch", ["plain", "fant"])
def test_a_point_does_not_see_its_batch(eng, branch):
    p = rh.make_problem(10200, branch=branch, N=150, D=4, H=3, S=5)
    pts = rh.points(p, 6, n=11)
    for kind, par in PATH_ACQS:
        refine_setup(eng, p, kind, par)
        f, g = eng.ei_grad_batch(pts)
        fr, gr = eng.ei_grad_batch(pts[::-1].copy())
        assert np.array_equal(f, fr[::-1]) and np.array_equal(g, gr[::-1])
        for k in (0, 4, 10):
            f1, g1 = eng.ei_grad_batch(pts[k:k + 1])
            assert f1[0] == f[k] and np.array_equal(g1[0], g[k])


# ---- 6. the tails against the 50-digit reference -----------------------------------------------------------------------------
def tail_pass(e, g, branch, kind, par):
    e.set_covar("Matern52")
    e.set_observations(g["comp"], g["vals"]); e.set_candidates(g["cand"]); e.set_hypers(g["rows"])
    e.set_acquisition(kind, par)
    with options(e, ei_fused=int(branch == "fused")):
        e.factor()
        if branch == "fant":      # two fantasy columns that ARE the observations: each value twice, (x + x) / 2 = x
            H, n = g["rows"].shape[0], g["vals"].shape[0]
            e.set_fantasies(np.repeat(np.repeat(g["vals"][None, :, None], H, axis=0), 2, axis=2), np.full((H, 2), np.min(g["vals"])))
        e.ei_run(0)
        assert e.stat("last_step_fused") == int(branch == "fused")
    return e.ei_draws()


@pytest.mark.parametrize("branch", ["plain", "fused", "fant"])
def test_pi_tail_against_50_digits(eng, golden_dir, branch):
    """PI from about 1 down past 1e-300 in k_ei_finalize, k_ei_fused128 and k_ei_fant_values: per band of log10 PI the
    device stays within 4x the float64 oracle's own error (the project's rule for P(feasible) and the EI tails)."""
    g = np.load(os.path.join(golden_dir, "acq_tail_mp.npz"))
    report, failures = [], []
    for k, xi in enumerate(g["xis"]):
        draws = tail_pass(eng, g, branch, ao.PI, float(xi))
        for h in range(g["rows"].shape[0]):
            ref, lp = g["PI_ref"][:, h, k], g["log10PI"][:, h, k]
            with orc.covar("Matern52"), np.errstate(all="ignore"):
                func_m, func_v = ao.moments(g["comp"], g["cand"], g["vals"], g["rows"][h])
            o_all = ao.value(ao.PI, float(xi), func_m, func_v, np.min(g["vals"]))
            e_o, e_d = am.band_errors(o_all, ref, lp), am.band_errors(draws[:, h], ref, lp)
            for band, o, d in zip(am.TAIL_BANDS, e_o, e_d):
                if o is None:
                    continue
                report.append("xi %g draw %d band %s: device %.3g oracle %.3g" % (xi, h, band, d, o))
                if not d <= max(4 * o, FLOOR):
                    failures.append(report[-1])
            deep = lp < -300
            assert np.all((draws[deep, h] >= 0) & (draws[deep, h] <= 1e-290))
    print("\n".join(report))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("branch", ["plain", "fused"])
def test_lcb_where_it_cancels(eng, golden_dir, branch):
    """kappa func_s within 1e-6 of func_m: the parity rule, EI_RTOL times (|func_m| + kappa func_s), against 50 digits."""
    g = np.load(os.path.join(golden_dir, "acq_tail_mp.npz"))
    for i, kappa in enumerate(g["lcb_kappa"]):
        draws = tail_pass(eng, g, branch, ao.LCB, float(kappa))
        scale = np.abs(g["func_m"]) + kappa * g["func_s"]
        assert np.all(np.abs(draws - g["lcb_ref"][i]) <= EI_RTOL * scale)
        c = int(g["lcb_cand"][i])
        assert abs(draws[c, 0]) <= 2e-6 * scale[c, 0]            # the case really cancels


# ---- 7. the handle's state machine, every refusal --------------------------------------------------------------------------
def test_setting_drops_the_results_and_nothing_else(eng):
    p = ph.problem(10300, N=150, D=3, H=3, S=5)
    cand = ph.candidates(p, 1, 600)
    ei = run_fant(eng, p, cand, ao.EI, 0.0)
    pts = rh.points(p, 1, n=3)
    eng.ei_grad_batch(pts)                                         # (alpha_s is built here)
    eng.set_acquisition(spx.ACQ_PI, 0.01)
    for getter in (eng.best, eng.ei_mean, eng.ei_draws):
        with pytest.raises(ValueError):
            getter()
    eng.ei_run(0)                       # the fantasies stay, and so does the factor: no spx_set_fantasies, no spx_factor
    with orc.covar(p.covar):
        ref = ao.over_hypers_fantasies(ao.PI, 0.01, p.X, cand, p.rows, p.fant, p.bests)
    assert_ei_close(eng.ei_draws(), ref, rtol=FANT_RTOL)
    f, g = eng.ei_grad_batch(pts)
    f_ref, g_ref = ao.grad_oracle(p, pts, ao.PI, 0.01)
    assert_close(f, g, f_ref, g_ref)
    eng.set_acquisition(spx.ACQ_EI)                                # and back: EI's bits
    eng.ei_run(0)
    assert_same(collect(eng), ei)
    # setting what is already set drops the results all the same (one rule)
    eng.set_acquisition(spx.ACQ_EI)
    with pytest.raises(ValueError):
        eng.best()


def test_every_refused_combination_leaves_the_handle_usable(eng):
    comp, cand, vals, hypers, log_durs, th = synthetic_problem(90, 500, 3, 2, 10400, per_sec=True)
    run_plain(eng, comp, vals, cand, hypers, ao.LCB, 2.0)
    good = collect(eng)

    def refused(fn, *a):
        with pytest.raises(ValueError) as ei:
            fn(*a)
        assert eng._lib.spx_last_error()                           # SPX_ERR_ARG with a message
        return str(ei.value)

    for kind, par in ((7, 0.0), (spx.ACQ_PI, -1.0), (spx.ACQ_LCB, float("nan")), (spx.ACQ_EI, 1.0)):
        refused(eng.set_acquisition, kind, par)
        assert eng.get_acquisition() == (spx.ACQ_LCB, 2.0)
        assert_same(collect(eng), good)                            # a refused setting drops nothing
    # the flags of the other objectives
    eng.set_time_model(log_durs, th)
    eng.factor()
    for flags in (FLAG_PER_SEC, FLAG_PER_SEC | FLAG_KEEP_MOMENTS | FLAG_TIME_ONLY):
        assert "SPX_ACQ_EI only" in refused(eng.ei_run, flags)
        assert "SPX_ACQ_EI only" in refused(eng.ei_step, flags)
    assert "time model" in refused(eng.ei_grad_batch, cand[:2])   # a time model is factored
    eng.set_time_model(None, None)
    eng.set_constraint_model(np.zeros((0, 3)), np.zeros(0), np.column_stack((np.ones(2), np.full(2, 1e-3), np.ones(2), np.ones((2, 3)))))
    eng.factor()
    assert "SPX_ACQ_EI only" in refused(eng.ei_run, FLAG_CONSTRAINED)
    assert "SPX_ACQ_EI only" in refused(eng.constrained_ei_grad_batch, cand[:2], float(np.min(vals)))
    # ... and the handle works: the same LCB pass, then EI with the very flags that were refused
    assert_same(run_plain(eng, comp, vals, cand, hypers, ao.LCB, 2.0), good)
    eng.set_acquisition(spx.ACQ_EI)
    eng.ei_step(FLAG_CONSTRAINED)
    eng.constrained_ei_grad_batch(cand[:2], float(np.min(vals)))


def test_nan_candidate_and_negative_variance(eng):
    """The oracle's NaN rule: a NaN candidate is NaN under every acquisition and wins (first NaN).  func_v < 0: with a noise
    of -3e-6 amp2 the covariance is still positive definite (the jitter and the spread of the points see to that), and a
    candidate ON an observation has func_v = -1e-6 amp2 to first order -- NaN where np.sqrt makes it so, kappa = 0 included,
    on the three-stage path (N = 130) and the fused one (N = 20)."""
    comp, cand, vals, hypers = synthetic_problem(100, 400, 3, 2, 10500)
    cand[37, 1] = np.nan
    for kind, par in ACQS:
        res = run_plain(eng, comp, vals, cand, hypers, kind, par)
        assert np.all(np.isnan(res["draws"][37])) and res["best"][0] == 37 and np.isnan(res["best"][1])
        assert np.sum(np.isnan(res["draws"])) == hypers.shape[0]
    for N in (20, 130):
        comp, cand, vals, hypers = synthetic_problem(N, 400, 3, 2, 10500 + N, near=0)
        hypers[:, 1] = -3e-6 * hypers[:, 2]
        cand[100], cand[37] = comp[7], comp[5]
        with orc.covar("Matern52"), np.errstate(all="ignore"):
            mom = [ao.moments(comp, cand, vals, h) for h in hypers]
        func_m, func_v = np.stack([m[0] for m in mom], axis=1), np.stack([m[1] for m in mom], axis=1)
        neg = func_v < 0
        assert np.array_equal(np.nonzero(neg[:, 0])[0], [37, 100]) and np.array_equal(neg[:, 0], neg[:, 1])
        assert np.all(func_v[neg] < -1e-7 * np.min(hypers[:, 2]))          # (far from a rounding accident)
        for kind, par in ACQS:
            with np.errstate(all="ignore"):
                ref = ao.value(kind, par, func_m, func_v, np.min(vals))
            res = run_plain(eng, comp, vals, cand, hypers, kind, par)
            assert np.array_equal(np.isnan(res["draws"]), neg) and np.array_equal(np.isnan(ref), neg)
            assert res["best"][0] == 37 and np.isnan(res["best"][1])
            assert_acq_close(kind, par, res["draws"], ref, func_m, np.sqrt(np.where(neg, 0.0, func_v)), EI_RTOL)


# ---- 8. the choosers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acq,par", [("LCB", 2.0), ("PI", 0.0)])
def test_opt_chooser_proposes_what_the_host_run_proposes(golden_dir, tmp_path, acq, par):
    from spearmint_amd.chooser import GPEIOptChooser
    g = np.load(os.path.join(golden_dir, "chooser_next.npz"))
    seed = int(g["opt_seed"])
    ch = GPEIOptChooser.init(str(tmp_path), "mcmc_iters=4,burnin=6,grid_subset=5,use_multiprocessing=0,acq=%s,acq_par=%g" % (acq, par))
    npr.seed(seed)
    job = ch.next(g["grid"], g["values"], g["durations"], g["candidates"], g["pending"], g["complete"])
    assert ch.engine().get_acquisition() == (spx.ACQ[acq], par)
    rows = ch.hyper_rows()
    comp, vals = g["grid"][g["complete"]], g["values"][g["complete"]]
    npr.seed(seed)
    sprayed = npr.randn(10, comp.shape[1]) * 0.001 + comp[np.argmin(vals)]
    want, allm, refined = host_opt_next(g["grid"], g["values"], g["candidates"], g["complete"], rows, spx.ACQ[acq], par, 5, sprayed)
    if isinstance(want, tuple):
        assert isinstance(job, tuple) and job[0] == want[0]
        assert np.allclose(job[1], want[1], atol=2e-5), (job[1], want[1])
    else:
        assert job == want
    ch.engine().close()


def test_recommendation_on_branin(golden_dir, tmp_path):
    """recommend=1: GPEIChooser returns the grid minimiser of the oracle's mean of means, GPEIOptChooser a point at least
    as good, with `mean` and `std` as the oracle has them at that point; the proposal and numpy's generator state are what
    recommend=0 leaves."""
    from spearmint_amd.chooser import GPEIChooser, GPEIOptChooser
    g = np.load(os.path.join(golden_dir, "chooser_next.npz"))
    grid, values, complete = g["grid"], g["values"], g["complete"]
    comp, vals = grid[complete], values[complete]
    for mod, args in ((GPEIChooser, "mcmc_iters=4"), (GPEIOptChooser, "mcmc_iters=4,burnin=6,grid_subset=5,use_multiprocessing=0")):
        jobs, states, seen = [], [], []
        for r in (0, 1):
            d = tmp_path / ("%s_%d" % (mod.__name__.split(".")[-1], r))
            d.mkdir()
            ch = mod.init(str(d), args + ",recommend=%d" % r)
            inner = ch._recommend

            def spy(grid_, comp_, vals_, rows_, **kw):
                seen.append(np.array(rows_, copy=True))
                return inner(grid_, comp_, vals_, rows_, **kw)
            ch._recommend = spy
            npr.seed(11)
            jobs.append(ch.next(grid, values, g["durations"], g["candidates"], g["pending"], complete))
            states.append(npr.get_state())
            rec, rec_file = ch.last_recommendation, ch.recommendation_file
            assert ch.engine().get_acquisition() == (spx.ACQ_EI, 0.0)
            ch.engine().close()
            if r == 0:
                assert rec is None and not seen and not os.path.exists(rec_file)
        a, b = jobs
        assert type(a) is type(b) and ((a[0] == b[0] and np.array_equal(a[1], b[1])) if isinstance(a, tuple) else a == b)
        assert np.array_equal(states[0][1], states[1][1]) and states[0][2:] == states[1][2:]
        assert len(open(rec_file).read().splitlines()) == 1 and len(seen) == 1
        rows = seen[0]
        with orc.covar("Matern52"):
            mom_grid = [ao.moments(comp, grid, vals, h) for h in rows]
            mom_x = [ao.moments(comp, rec["x"][None, :], vals, h) for h in rows]
        gm = np.mean([m[0] for m in mom_grid], axis=0)
        fm, fv = np.array([m[0][0] for m in mom_x]), np.array([m[1][0] for m in mom_x])
        assert np.isclose(rec["mean"], np.mean(fm), rtol=1e-7, atol=1e-9)
        assert np.isclose(rec["std"], np.sqrt(np.mean(fv) + np.var(fm)), rtol=1e-6)
        if mod is GPEIChooser:
            assert rec["grid_index"] == int(np.argmin(gm)) and np.array_equal(rec["x"], grid[rec["grid_index"]])
        else:
            assert rec["mean"] <= gm.min() + 1e-7 * max(abs(gm.min()), 1.0)
            assert rec["grid_index"] in (-1, int(np.argmin(gm)))


def test_recommendation_skips_nan_rows_of_the_grid(golden_dir, tmp_path):
    """The device returns NaN for a NaN candidate and its argmax names it first; the recommendation never does: NaN rows are
    neither refined nor recommended, and the result is the one of the grid without them."""
    from spearmint_amd.chooser import GPEIOptChooser
    g = np.load(os.path.join(golden_dir, "chooser_next.npz"))
    grid, complete = g["grid"], g["complete"]
    comp, vals = grid[complete], g["values"][complete]
    rows = np.array(g["opt_hypers"])
    ch = GPEIOptChooser.init(str(tmp_path), "grid_subset=4,recommend=1")
    try:
        clean = dict(ch._recommend(grid, comp, vals, rows, refine_count=4))
        bad = grid.copy()
        holes = [5, 77, clean["grid_index"] if clean["grid_index"] >= 0 else 200]
        bad[holes, 1] = np.nan
        rec = ch._recommend(bad, comp, vals, rows, refine_count=4)
        assert np.isfinite(rec["mean"]) and np.isfinite(rec["std"]) and np.all(np.isfinite(rec["x"])) and rec["grid_index"] not in holes
        want = ch._recommend(np.delete(bad, holes, axis=0), comp, vals, rows, refine_count=4)
        assert want["mean"] == rec["mean"] and np.array_equal(want["x"], rec["x"])
        assert ch._recommend(np.full((3, grid.shape[1]), np.nan), comp, vals, rows, refine_count=4) is None
        assert len(open(ch.recommendation_file).read().splitlines()) == 3
    finally:
        ch.engine().close()
