"""The pending branch of the grid pass -- spx_set_fantasies followed by spx_ei_run, what every chooser runs while a job is
still out -- on every execution path of ei_run_impl, at the shapes and counts where its own code (k_gamma over S columns,
the fantasy epilogues of k_predict_gemm_tri / k_predict_gemm_tail<ML> / k_predict_gemm<4,1,0>, k_ei_fant_values,
k_ei_fant_mean, the second chunk / draw-group plan) can go wrong, its mean over S against numpy's bit for bit, the plan's
two limits (grid.y and the memory budget) with the launch counts as evidence, its tail against the 50-digit reference,
per second, through the handle's state machine and on the multi-device handle.  The oracle of one draw is
oracle/gp_ei_oracle.compute_ei_fantasies (tests/pending_helpers.oracle).  Sorted after test_gpu_m_refine_paths.py; the
older tests of this branch (test_gpu_a_parity.py::test_fantasies_against_oracle, test_golden_pending_fantasies) should be
read first when both fail."""
import functools
import os

import numpy as np
import pytest
from numpy.linalg import LinAlgError

from oracle import gp_ei_oracle as orc
from tests import pending_helpers as ph
from tests import refine_helpers as rh
from tests import refine_mp as rm
from tests.pending_helpers import FLAG_KEEP_MOMENTS, FLAG_PER_SEC, FLAG_TIME_ONLY, options
from tests.test_gpu_a_parity import assert_ei_close
from tests.test_gpu_k_constrained_paths import assert_same, plan_chunks

pytestmark = pytest.mark.gpu
FANT_RTOL = 1e-6          # the bar of test_fantasies_against_oracle / test_golden_pending_fantasies; plain passes: EI_RTOL


@pytest.fixture()
def eng():
    from spearmint_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def check_oracle(res, ref, rtol=FANT_RTOL):
    """assert_ei_close with nothing exempted (no reference value below 1e-280), the oracle's winner, numpy's mean."""
    assert np.all(np.isfinite(ref)) and np.min(ref) >= 1e-280, float(np.min(ref))
    assert_ei_close(res["draws"], ref, rtol=rtol)
    assert res["best"][0] == orc.choose(ref)
    assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1))
    assert res["best"][1] == res["mean"][res["best"][0]]


# ---- 1. execution paths, bit for bit against the default path ---------------------------------------------------------------
#          name: (problem arguments, M, small staging budget)
BASES = {"general": (dict(seed=101, N=247, D=3, H=5, S=12, n_pend=4), 5000, 256 * 1024 * 8),     # Np = 256, nothing to skip
         "small": (dict(seed=102, N=63, D=3, H=5, S=12, n_pend=3), 5000, 128 * 1024 * 8)}        # Np = 128: the tail kernel alone


@functools.lru_cache(maxsize=None)
def base_problem(name):
    kw, M, budget = BASES[name]
    p = ph.problem(**kw)
    cand = ph.candidates(p, 9, M)
    return p, cand, ph.oracle(p, cand), budget


def default_run(eng, name):
    p, cand, ref, budget = base_problem(name)
    base = ph.fant_pass(eng, p, cand)
    check_oracle(base, ref)
    assert eng.stat("last_step_fused") == 0                  # never fused with fantasies, N <= 128 included
    assert eng.stat("last_step_skipped_padding") == int(ph.padding_plan(p.X.shape[0])[1])
    nchunks, hb = plan_chunks(cand.shape[0], p.X.shape[0], p.H, budget)
    assert nchunks >= 5 and hb == 1, (nchunks, hb)           # what "small budget" means below
    ph.scramble(eng, p, cand)
    return p, cand, base, budget, nchunks


VARIANTS = {"chunks": dict(kstar_budget_bytes=True), "streams2": dict(streams=2),
            "streams2+chunks": dict(streams=2, kstar_budget_bytes=True), "timing": dict(timing=1),
            "gemm_partial0": dict(gemm_partial=0), "gemm_partial1": dict(gemm_partial=1),
            "cov_flat0": dict(cov_flat=0), "cov_flat1": dict(cov_flat=1), "ei_flow0": dict(ei_flow=0),
            "ei_flow1": dict(ei_flow=1), "stage_copies0": dict(stage_copies=0), "stage_copies1": dict(stage_copies=1),
            "cov_flat0+chunks": dict(cov_flat=0, kstar_budget_bytes=True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(BASES))
def test_path_variants_do_not_change_bits(eng, name, variant):
    p, cand, base, budget, _ = default_run(eng, name)
    kw = dict(VARIANTS[variant])
    if kw.get("kstar_budget_bytes"):
        kw["kstar_budget_bytes"] = budget
    with options(eng, **kw):
        got = ph.fant_pass(eng, p, cand)
        assert eng.stat("last_step_fused") == 0
        skipped = eng.stat("last_step_skipped_padding")
    assert_same(got, base, (name, variant))
    if "gemm_partial" in kw:
        assert skipped == int(kw["gemm_partial"] and ph.padding_plan(p.X.shape[0])[1])


@pytest.mark.parametrize("name", sorted(BASES))
def test_small_budget_really_chunks(eng, name):
    """timing=1 with the small budget: ei_finalize runs once per (chunk, draw group) with fantasies, so its launch count is
    chunks x groups = chunks x H here, and so are K(X*,X)'s and the GEMM's."""
    p, cand, base, budget, nchunks = default_run(eng, name)
    for kw in (dict(), dict(streams=2)):
        with options(eng, kstar_budget_bytes=budget, timing=1, **kw):
            got = ph.fant_pass(eng, p, cand)
            t = eng.timings()
        assert_same(got, base, (name, sorted(kw)))
        assert t["ei_finalize"][1] == nchunks * p.H
        assert t["predict_gemm"][1] == nchunks * p.H and t["cov_cross"][1] == nchunks * p.H
        ph.scramble(eng, p, cand)


@pytest.mark.parametrize("name", sorted(BASES))
def test_step_then_fantasies_equals_factor_then_fantasies(eng, name):
    """spx_ei_step (a chooser's first pass), set_fantasies, ei_run -- against spx_factor first.  And once the fantasies are
    cleared the pass of the small problem is the fused one again."""
    p, cand, base, budget, _ = default_run(eng, name)
    for kw in (dict(), dict(kstar_budget_bytes=budget), dict(streams=2, kstar_budget_bytes=budget)):
        with options(eng, **kw):
            got = ph.fant_pass(eng, p, cand, entry="step")
        assert_same(got, base, (name, sorted(kw)))
        ph.scramble(eng, p, cand)
    ph.fant_pass(eng, p, cand)
    assert eng.stat("last_step_fused") == 0
    eng.set_fantasies(None, None)
    eng.ei_run(0)
    assert eng.stat("last_step_fused") == int(name == "small")
    plain = ph.collect(eng)
    assert_same(plain, ph.fresh(ph.plain_pass, p, cand), "cleared")
    assert_ei_close(plain["draws"], ph.oracle_plain(p, cand))


V14_BOUND = 1.2e-9    # 10 x the largest relative difference measured between variants 14 and 0 (the docstring below)


@pytest.mark.parametrize("name", sorted(BASES))
def test_gemm_variants_with_fantasies(eng, name):
    """Only k_predict_gemm<4,1,0> (variant 14) of the rectangular kernels has the fantasy epilogue, so launch_predict_gemm
    maps a request for 4, 8, 18 or 24 onto it while fantasies are set: the four give variant 14's bits.  Variant 14 is
    "the production kernel without the skipping" (csrc/predict_kernels.hip), and the variants "agree to rounding": it is
    NOT bit-identical to variant 0.  Measured on an MI355X, the largest relative difference of a per-draw EI between the
    two: 1.19e-10 on the general problem (22 820 of 25 000 values differ; the smallest reference EI there is 1e-92, where a
    rounding of func_m is amplified by about u^2 / 2), 1.2e-11 on the small one (22 716 of 25 000).  The two differ in the
    order of one 256-term sum per row block; asserted: 10 x the larger figure, 1.2e-9."""
    p, cand, base, budget, _ = default_run(eng, name)
    ref = base_problem(name)[2]
    with options(eng, gemm_waves=14):
        v14 = ph.fant_pass(eng, p, cand)
        assert eng.stat("last_step_skipped_padding") == 0        # (the plan is the production kernel's alone)
    check_oracle(v14, ref)
    for v in (4, 8, 18, 24):
        ph.scramble(eng, p, cand)
        for kw in (dict(), dict(kstar_budget_bytes=budget)):
            with options(eng, gemm_waves=v, **kw):
                assert_same(ph.fant_pass(eng, p, cand), v14, (name, v, sorted(kw)))
    diff = float(np.max(np.abs(v14["draws"] - base["draws"]) / base["draws"]))
    print("%s: variant 14 against variant 0 with fantasies: max relative difference %.3g, %d of %d values differ"
          % (name, diff, int(np.sum(v14["draws"] != base["draws"])), base["draws"].size))
    assert diff <= V14_BOUND
    assert v14["best"][0] == base["best"][0]


# rows resident (observations + 3 pending, 1 at N = 2 ... ) by live 16-row tiles of the last row block
TAIL_ROWS = ([16, 17, 33, 64, 65, 96, 97]                                                   # the only row block: nrb_main = 0
             + [129, 144, 145, 160, 161, 176, 177, 192, 193, 208, 209, 224, 230]            # two row blocks; 230 declines
             + [257, 272, 273, 288, 289, 304, 305, 320, 321, 336, 337, 352, 600])           # three; 600 (five) declines


@pytest.mark.parametrize("n_rows", TAIL_ROWS)
def test_tail_kernel_with_fantasies(eng, n_rows):
    """k_predict_gemm_tail<ML>'s fantasy epilogue at every ML and at both fills of its last pair of tiles: 1 .. 6 live
    tiles of the last row block, N = 0 and 1 mod 16; with at most 96 rows it is the pass's ONLY GEMM launch.  gemm_partial=1
    against 0 bit for bit, both against the oracle; where the plan declines (97, 230, 600) the stat says so."""
    lt, skips = ph.padding_plan(n_rows)
    assert skips == (n_rows not in (97, 230, 600)) and (not skips or 1 <= lt <= 6)
    p = ph.problem(1500 + n_rows, N=n_rows, D=3, H=2, S=7)
    cand = ph.candidates(p, n_rows, 700)
    ref = ph.oracle(p, cand)
    base = ph.fant_pass(eng, p, cand)
    assert eng.stat("last_step_skipped_padding") == int(skips)
    check_oracle(base, ref)
    for on in (0, 1):
        ph.scramble(eng, p, cand)
        with options(eng, gemm_partial=on):
            got = ph.fant_pass(eng, p, cand)
            assert eng.stat("last_step_skipped_padding") == int(on and skips)
        assert_same(got, base, (n_rows, on))
    budget = 8 * ((n_rows + 127) // 128 * 128) * 128          # six chunks of 128, one draw per group
    assert plan_chunks(700, n_rows, 2, budget) == (6, 1)
    for on in (0, 1):
        ph.scramble(eng, p, cand)
        with options(eng, gemm_partial=on, kstar_budget_bytes=budget):
            assert_same(ph.fant_pass(eng, p, cand), base, (n_rows, on, "chunks"))


# ---- 2. the mean over S is numpy's, bit for bit ----------------------------------------------------------------------------
S_LIST = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 255, 256, 257, 300, 1000]


@pytest.mark.parametrize("n_rows,M", [(70, 300), (135, 333)])
@pytest.mark.parametrize("S", S_LIST)
def test_mean_over_fantasies_is_numpys(eng, S, n_rows, M):
    """include/spx.h: "averages over S in numpy's summation order".  A pass with ONE fantasy column returns that column's
    EI exactly ((0.0 + x) / 1.0), and no stage mixes columns (one k_gamma block row, one sidx of the GEMM epilogue, one
    thread of k_ei_fant_values per column), so S one-column passes give E[M, H, S] and the S-column pass must return
    np.mean(E[:, h, :], axis=1) -- eight accumulators below 128 terms, the pairwise tree above -- with array_equal.  The
    same with several chunks and one draw per group, where np_pairwise's stride is a chunk's Mc and not Mp."""
    H = 2
    p = ph.problem(2000 + S + n_rows, N=n_rows, D=3, H=H, S=S)
    cand = ph.candidates(p, S, M)
    ph.load(eng, p, cand)
    eng.factor()
    E = np.empty((M, H, S))
    for s in range(S):
        q = ph.with_columns(p, s, s + 1)
        eng.set_fantasies(q.fant, q.bests)
        eng.ei_run(0)
        E[:, :, s] = eng.ei_draws()
    want = np.stack([np.mean(np.ascontiguousarray(E[:, h, :]), axis=1) for h in range(H)], axis=1)
    budget = 8 * ((n_rows + 127) // 128 * 128) * 128
    assert plan_chunks(M, n_rows, H, budget) == (3, 1)
    for kw in (dict(), dict(kstar_budget_bytes=budget)):
        ph.scramble(eng, p, cand)
        with options(eng, **kw):
            got = ph.fant_pass(eng, p, cand)
        wrong = got["draws"] != want
        assert np.array_equal(got["draws"], want), (S, sorted(kw), int(np.sum(wrong)))
        assert np.array_equal(got["mean"], np.mean(got["draws"], axis=1))
    if S > 1:
        assert not np.array_equal(E[:, :, 0], E[:, :, 1])


# ---- 3. shapes and counts against the oracle ---------------------------------------------------------------------------------
#          (rows resident, pending, D, H, M, S), one thing varied at a time from (150, 3, 3, 3, 700, 5)
SHAPES = ([(n, 3, 3, 3, 700, 5) for n in (2, 3, 64, 65, 127, 128, 129, 130, 255, 256, 257, 300)]
          + [(1000, 3, 3, 1, 700, 5), (2051, 3, 3, 1, 700, 5)]
          + [(150, 1, 3, 3, 700, 5), (150, 2, 3, 3, 700, 5), (150, 7, 3, 3, 700, 5), (300, 7, 3, 3, 700, 5)]
          + [(150, 3, d, 3, 600, 5) for d in (1, 8, 9, 33)] + [(260, 3, 1, 3, 600, 5), (260, 3, 33, 3, 600, 5)]
          + [(150, 3, 3, 1, 700, 5), (90, 3, 3, 130, 300, 5), (200, 3, 3, 130, 300, 5)]
          + [(150, 3, 3, 3, m, 5) for m in (1, 127, 128, 129)] + [(260, 3, 3, 3, m, 5) for m in (1, 129)]
          + [(150, 3, 3, 3, 700, s) for s in (1, 128, 129)] + [(150, 3, 3, 2, 700, 1000), (150, 3, 3, 2, 700, 4096),
                                                                (60, 3, 3, 2, 700, 4096)])


@pytest.mark.parametrize("n_rows,n_pend,D,H,M,S", SHAPES)
def test_shapes_match_oracle(eng, n_rows, n_pend, D, H, M, S):
    """Pad boundaries of the resident rows (64, 128, 256; 2048 + 3: one row block more than the benchmark's), pending
    points, D = 1 / 33 (the Dp padding), H = 1 / 130, M around 128, S from 1 to the ABI's 4096."""
    p = ph.problem(3000 + 7 * n_rows + 5 * n_pend + 3 * D + H + M + S, N=n_rows, D=D, H=H, S=S, n_pend=n_pend)
    assert p.X.shape[0] == n_rows and p.fant.shape == (H, n_rows, S)
    cand = ph.candidates(p, n_rows + M, M)
    res = ph.fant_pass(eng, p, cand)
    check_oracle(res, ph.oracle(p, cand))
    assert eng.stat("last_step_fused") == 0


@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE", "SE"])
def test_every_covar_with_several_chunks(eng, covar):
    p = ph.problem(3570 + len(covar), covar, N=247, D=3, H=4, S=9, n_pend=4)
    cand = ph.candidates(p, 11, 5000)
    budget = 256 * 1024 * 8
    nchunks, hb = plan_chunks(5000, 247, 4, budget)
    assert nchunks >= 5 and hb == 1
    ref = ph.oracle(p, cand)
    base = ph.fant_pass(eng, p, cand)
    check_oracle(base, ref)
    for kw in (dict(kstar_budget_bytes=budget), dict(kstar_budget_bytes=budget, streams=2)):
        ph.scramble(eng, p, cand)
        with options(eng, **kw):
            assert_same(ph.fant_pass(eng, p, cand), base, (covar, sorted(kw)))
    if covar == "SE":       # SE is ARDSE with unit length scales: bit for bit, as the refinement tests assert it
        q = ph.with_columns(p, 0, p.S)
        q.covar, q.rows = "ARDSE", p.rows.copy()
        q.rows[:, 3:] = 1.0
        assert_same(ph.fant_pass(eng, q, cand), base, "SE as ARDSE")


@pytest.mark.parametrize("chunks", [False, True])
def test_nan_candidates(eng, chunks):
    """Two candidates with a NaN coordinate: EI of a NaN point is NaN in every draw (the oracle's triangular solve refuses
    non-finite input, so its EI is taken at the finite candidates and the two rows set by that rule), np.argmax of the mean
    returns the FIRST NaN, and every other candidate keeps its bits."""
    p = ph.problem(3600, N=150, D=3, H=3, S=5)
    cand = ph.candidates(p, 12, 700)
    first, second = 467, 600
    bad = cand.copy()
    bad[first, p.D - 1] = np.nan
    bad[second, 0] = np.nan
    ref = ph.oracle(p, cand)
    ref_bad = ref.copy()
    ref_bad[[first, second]] = np.nan
    budget = 8 * 256 * 128
    assert plan_chunks(700, 150, 3, budget) == (6, 1)          # the two rows sit in chunks 3 and 4
    with options(eng, **({"kstar_budget_bytes": budget} if chunks else {})):
        clean = ph.fant_pass(eng, p, cand)
        res = ph.fant_pass(eng, p, bad)
    check_oracle(clean, ref)
    assert_ei_close(res["draws"], ref_bad, rtol=FANT_RTOL)
    assert np.all(np.isnan(res["draws"][[first, second]])) and np.all(np.isnan(res["mean"][[first, second]]))
    assert res["best"][0] == int(np.argmax(np.mean(ref_bad, axis=1))) == first and np.isnan(res["best"][1])
    keep = np.ones(700, dtype=bool)
    keep[[first, second]] = False
    assert np.array_equal(res["draws"][keep], clean["draws"][keep]) and np.array_equal(res["mean"][keep], clean["mean"][keep])


# ---- 4. the fantasy plan's own limits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,H,groups", [(4096, 15, 1), (4096, 16, 2), (4096, 20, 2), (3000, 21, 1), (3000, 22, 2)])
def test_grid_y_limit_splits_the_draws(eng, S, H, groups):
    """k_ei_fant_values runs on a grid of (Mc / 256, draws of the group x S) and grid.y ends at 65535: ei_run_impl caps a
    group at 65535 / S draws (15 at S = 4096, 21 at S = 3000).  One chunk of 128 candidates, so ei_finalize's launch count
    IS the number of groups.  Every draw against the oracle, and draws on either side of the cut equal to themselves run
    alone."""
    p = ph.problem(4000 + S + H, N=60, D=2, H=H, S=S)
    cand = ph.candidates(p, 13, 128)
    with options(eng, timing=1):
        res = ph.fant_pass(eng, p, cand)
        t = eng.timings()
    assert t["ei_finalize"][1] == groups and t["predict_gemm"][1] == groups, (t["ei_finalize"], t["predict_gemm"])
    check_oracle(res, ph.oracle(p, cand))
    assert_same(ph.fant_pass(eng, p, cand), res, "untimed")
    cut = 65535 // S
    for d in sorted({0, cut - 1, min(cut, H - 1), H - 1}):
        alone = ph.fant_pass(eng, rh.one_draw(p, d), cand)
        assert np.array_equal(alone["draws"][:, 0], res["draws"][:, d]), d


def test_memory_budget_cuts_the_chunks(eng):
    """S = 4096 over 300 resident rows (three row blocks): the per-fantasy partial means take 3 x 2 x 4096 x 8 = 196 608
    bytes per candidate, so the pass's 2 GB budget (less on a fuller device) holds at most 10 880 of the 20 000 candidates:
    the plan's single chunk is cut and the draws run one per group -- ei_finalize launches > H is the evidence.  About
    2.5 GB on the device for a moment."""
    H, M = 2, 20000
    p = ph.problem(4500, N=300, D=3, H=H, S=4096)
    cand = ph.candidates(p, 14, M)
    assert plan_chunks(M, 300, H, 512 << 20) == (1, H)           # without fantasies: one chunk, both draws together
    with options(eng, timing=1):
        res = ph.fant_pass(eng, p, cand)
        t = eng.timings()
    print("memory budget: ei_finalize launches %d, predict_gemm launches %d" % (t["ei_finalize"][1], t["predict_gemm"][1]))
    assert t["ei_finalize"][1] > H and t["ei_finalize"][1] % H == 0
    sub = np.r_[0:500, M - 500:M]
    ref = ph.oracle(p, cand[sub])
    assert np.min(ref) >= 1e-280
    assert_ei_close(res["draws"][sub], ref, rtol=FANT_RTOL)
    assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1))
    assert res["best"][0] == int(np.argmax(res["mean"])) and res["best"][1] == res["mean"][res["best"][0]]
    budget = 8 * 384 * 2048
    assert plan_chunks(M, 300, H, budget) == (10, 1)
    ph.scramble(eng, ph.with_columns(p, 0, 8), cand)
    with options(eng, kstar_budget_bytes=budget, timing=1):
        small = ph.fant_pass(eng, p, cand)
        assert eng.timings()["ei_finalize"][1] == 10 * H
    assert_same(small, res, "smaller chunks")


def test_more_than_4096_fantasies_are_refused(eng):
    p = ph.problem(4600, N=60, D=2, H=2, S=4097)
    cand = ph.candidates(p, 15, 300)
    ok = ph.with_columns(p, 0, 4096)
    first = ph.fant_pass(eng, ok, cand)
    with pytest.raises(ValueError, match="4096"):
        eng.set_fantasies(p.fant, p.bests)
    eng.ei_run(0)                                                # the handle is usable, the 4096 columns still in force
    assert_same(ph.collect(eng), first, "after the refusal")
    assert_same(first, ph.fresh(ph.fant_pass, ok, cand), "fresh")
    check_oracle(first, ph.oracle(ok, cand))


# ---- 5. the tail against the 50-digit reference -----------------------------------------------------------------------------
FLOOR = 16 * np.finfo(float).eps      # 3.6e-15: a band where the oracle happens to be exact is not an impossible bar


@pytest.mark.parametrize("branch", list(rh.BRANCHES))
@pytest.mark.parametrize("covar", list(rh.COVARS))
def test_grid_tails_against_50_digits(eng, golden_dir, covar, branch):
    """tests/golden/refine_tail_mp.npz holds -EI of ONE draw at 150 points from 10 down past 1e-300: with H = 1 that is the
    grid pass at candidates = those points (tests/test_pending_mp.py holds the grid oracle to it).  Per band of log10 EI --
    [-3, 1], [-20, -3), [-100, -20), [-300, -100) -- the device's max relative error against the 50-digit value is at most
    4 x the float64 oracle's own on the same inputs (computed here), floor 16 ulp; below 1e-300: 0 <= EI <= 1e-290.
    Fantasies through the three-stage path; plain and per second (48 rows) through the fused kernel AND the three-stage
    path, which agree bit for bit.

    Measured on an MI355X, device error / oracle error per band (bar: 4), the larger of the two value sets:
        Matern52 plain  2.17, 1.41, 1.37, 1.12        Matern52 persec 2.15, 1.39, 1.37, 1.12
        Matern52 fant   1.52, 1.48, 1.79, 0.82        Matern32 plain  0.85, 1.28, 0.70, 0.96
        Matern32 persec 0.82, 1.27, 0.70, 0.96        Matern32 fant   0.73, 1.32, 1.24, 0.82
        ARDSE    plain  0.92, 1.11, 1.30, 1.30        ARDSE    persec 1.04, 1.11, 1.30, 1.30
        ARDSE    fant   1.38, 1.91, 2.03, 1.12
    The device's largest errors over the nine cases: 1.5e-12, 2.7e-11, 1.2e-10, 7.8e-10 -- the refinement objective's
    (tests/test_gpu_m_refine_paths.py), as it should be: the same func_m error amplified by about u^2 / 2."""
    g = np.load(os.path.join(golden_dir, "refine_tail_mp.npz"))
    p, pts, sets = rm.tail_problem(covar, branch)
    flags = FLAG_PER_SEC if branch == "persec" else 0
    report, failures = [], []
    for which, vs in zip(rm.SETS, sets):
        q = rm.with_values(p, vs)
        f_ref, lf = g[rm.key(covar, branch, which, "f")], g[rm.key(covar, branch, which, "log10f")]
        runs = []
        for fused in ((None,) if branch == "fant" else (1, 0)):
            with options(eng, **({} if fused is None else {"ei_fused": fused})):
                rh.setup(eng, q, cand=pts)
                eng.ei_run(flags)
                assert eng.stat("last_step_fused") == int(bool(fused))
                runs.append(ph.collect(eng))
        if len(runs) == 2:
            assert_same(runs[0], runs[1], "ei_fused 1 / 0")
        ei = runs[0]["draws"][:, 0]
        e_o = ph.value_band_errors(ph.tail_oracle(q, pts), -f_ref, lf)
        e_d = ph.value_band_errors(ei, -f_ref, lf)
        for band, o, d in zip(rm.TAIL_BANDS, e_o, e_d):
            if o is None:
                continue
            report.append("%s %s %s band %s: device %.3g oracle %.3g ratio %.3g" % (covar, branch, which, band, d, o, d / o if o else np.inf))
            if not d <= max(4 * o, FLOOR):
                failures.append(report[-1])
        deep = lf < -300
        assert np.mean(deep) <= 0.15
        assert np.all((ei[deep] >= 0) & (ei[deep] <= 1e-290))
        assert np.all(ei >= 0)
    print("\n".join(report))
    assert not failures, "\n".join(report)


# ---- 6. per second with fantasies -----------------------------------------------------------------------------------------------
def test_per_second_with_fantasies(eng):
    """SPX_FLAG_PER_SEC with fantasies set (include/spx.h: defined; a time model over the same resident rows):
    k_ei_fant_mean divides the mean over S by time_m[h0 * mc + c].  Several chunks and one draw per group, so h0 > 0 is
    read.  spx_get_time_mean after such a pass is the plain per-second pass's, and spx_get_moments refuses."""
    p = ph.problem(6000, N=247, D=3, H=4, S=12, n_pend=4)
    cand = ph.candidates(p, 16, 3000)
    budget = 256 * 1024 * 8
    assert plan_chunks(3000, 247, 4, budget) == (3, 1)
    tmean = np.stack([ph.oracle_time_mean(p, cand, h) for h in range(p.H)], axis=1)
    assert np.max(tmean) / np.min(tmean) > 1.5                   # (a division that would be missed shows)
    ref = ph.oracle(p, cand) / tmean
    keep = FLAG_PER_SEC | FLAG_KEEP_MOMENTS
    with options(eng, kstar_budget_bytes=budget, timing=1):
        got = ph.fant_pass(eng, p, cand, flags=keep, time_model=True)
        assert eng.timings()["ei_finalize"][1] == 3 * p.H
    check_oracle(got, ref)
    tm = np.stack([eng.get_time_mean(h) for h in range(p.H)], axis=1)
    with pytest.raises(ValueError):
        eng.get_moments(0)
    np.testing.assert_allclose(tm, tmean, rtol=1e-9, atol=0)
    ph.scramble(eng, p, cand)
    for kw in (dict(), dict(streams=2, kstar_budget_bytes=budget)):
        with options(eng, **kw):
            assert_same(ph.fant_pass(eng, p, cand, flags=FLAG_PER_SEC, time_model=True), got, sorted(kw))
    eng.set_fantasies(None, None)                                # the plain per-second pass over the same rows
    eng.ei_run(keep)
    plain = ph.collect(eng)
    assert np.array_equal(np.stack([eng.get_time_mean(h) for h in range(p.H)], axis=1), tm)
    assert_ei_close(plain["draws"], ph.oracle_plain(p, cand) / tmean)
    assert not np.array_equal(plain["draws"], got["draws"])


# ---- 7. the handle's state machine ----------------------------------------------------------------------------------------------
def state_problem(seed=7000, **kw):
    args = dict(N=150, D=3, H=3, S=5)
    args.update(kw)
    p = ph.problem(seed, **args)
    return p, ph.candidates(p, 17, 1000)


def refused(fn, *args):
    with pytest.raises(ValueError):
        fn(*args)


def test_set_fantasies_needs_a_factorisation(eng):
    p, cand = state_problem()
    ph.load(eng, p, cand)
    refused(eng.set_fantasies, p.fant, p.bests)
    eng.ei_step(0)                                               # a step leaves a checked factor behind
    eng.set_fantasies(p.fant, p.bests)
    eng.ei_run(0)
    got = ph.collect(eng)
    assert_same(got, ph.fresh(ph.fant_pass, p, cand), "after a step")
    check_oracle(got, ph.oracle(p, cand))


@pytest.mark.parametrize("how", ["factor", "ei_step", "clear", "set_observations", "set_hypers", "covar_other", "gp_logprob"])
def test_what_drops_the_fantasies(eng, how):
    """The next pass is the plain pass over the resident rows, by bits a handle's that never had fantasies.  Between a call
    that invalidates the factorisation and the new spx_factor, spx_ei_run and spx_set_fantasies refuse -- never a pass on a
    stale Gamma."""
    p, cand = state_problem()
    first = ph.fant_pass(eng, p, cand)
    q = p
    if how == "factor":
        eng.factor()
    elif how == "clear":
        eng.set_fantasies(None, None)
    elif how != "ei_step":
        if how == "set_observations":
            eng.set_observations(p.X, ph.padded_vals(p))
            eng.set_hypers(p.rows)
        elif how == "set_hypers":
            eng.set_hypers(p.rows)
        elif how == "covar_other":
            eng.set_covar("Matern32")
            q = ph.with_columns(p, 0, p.S)
            q.covar = "Matern32"
        else:
            assert np.all(np.isfinite(eng.gp_logprob()))        # leaves no EI factor behind
        refused(eng.ei_run, 0)
        refused(eng.set_fantasies, p.fant, p.bests)
        refused(eng.ei_draws)
        eng.factor()
    if how == "ei_step":
        eng.ei_step(0)
    else:
        eng.ei_run(0)
    got = ph.collect(eng)
    assert_same(got, ph.fresh(ph.plain_pass, q, cand), how)
    assert not np.array_equal(got["draws"], first["draws"])
    assert_ei_close(got["draws"], ph.oracle_plain(q, cand))
    assert_same(ph.fant_pass(eng, p, cand), first, "set again")


def test_what_keeps_the_fantasies(eng):
    p, cand = state_problem()
    first = ph.fant_pass(eng, p, cand)
    assert_same(first, ph.fresh(ph.fant_pass, p, cand), "fresh")
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "a second pass")
    eng.set_covar(p.covar)                                       # the value it has: nothing is invalidated
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "covar set to its own value")
    f, g = eng.ei_grad_batch(rh.points(p, 3, 9))                 # the refinement's own use of Gamma (alpha_S) in between
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "ei_grad_batch in between")
    more = ph.candidates(p, 18, 2500)
    for M in (300, 128, 127, 2500, 129, 1000):                   # smaller, larger, across 128
        sub = more[:M]
        eng.set_candidates(sub)
        eng.ei_run(0)
        assert_same(ph.collect(eng), ph.fresh(ph.fant_pass, p, sub), M)
    # a SPX_FLAG_TIME_ONLY pass in between, on a handle with a time model
    with_time = ph.fant_pass(eng, p, cand, time_model=True)
    assert_same(with_time, first, "a time model does not change the plain flags' pass")
    eng.ei_run(FLAG_PER_SEC | FLAG_KEEP_MOMENTS | FLAG_TIME_ONLY)
    refused(eng.ei_draws)
    tm = eng.get_time_mean(1)
    np.testing.assert_allclose(tm, ph.oracle_time_mean(p, cand, 1), rtol=1e-9, atol=0)
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "TIME_ONLY in between")


def test_fantasy_count_grows_and_shrinks(eng):
    """S 5 -> 300 -> 5 -> 1 -> 4096 -> 5 on one handle (buffers that only grow; the budget asked again when S changes):
    every pass is a fresh handle's."""
    p5, cand = state_problem(7300, H=2)
    ph.load(eng, p5, cand)
    eng.factor()
    for i, S in enumerate((5, 300, 5, 1, 4096, 5)):
        p = ph.problem(7300, N=150, D=3, H=2, S=S)
        assert np.array_equal(p.X, p5.X) and np.array_equal(p.rows, p5.rows)
        eng.set_fantasies(p.fant, p.bests)
        eng.ei_run(0)
        got = ph.collect(eng)
        assert_same(got, ph.fresh(ph.fant_pass, p, cand), (i, S))
        if i in (1, 3, 4):
            check_oracle(got, ph.oracle(p, cand))


def test_keep_moments_with_fantasies(eng):
    """The pass keeps no func_m / func_v with fantasies (there is one mean per fantasy): same results, and
    spx_get_moments refuses instead of returning the previous pass's."""
    p, cand = state_problem()
    ph.plain_pass(eng, p, cand, flags=FLAG_KEEP_MOMENTS)
    m, v = eng.get_moments(0)
    assert np.all(np.isfinite(m)) and np.all(v > 0)
    eng.set_fantasies(p.fant, p.bests)
    eng.ei_run(FLAG_KEEP_MOMENTS)
    got = ph.collect(eng)
    refused(eng.get_moments, 0)
    assert_same(got, ph.fresh(ph.fant_pass, p, cand), "KEEP_MOMENTS")
    eng.set_fantasies(None, None)
    eng.ei_run(FLAG_KEEP_MOMENTS)
    m2, v2 = eng.get_moments(0)
    assert np.array_equal(m2, m) and np.array_equal(v2, v)


@pytest.mark.parametrize("entry", ["factor", "step"])
def test_not_pd_with_pending_points(eng, entry):
    """A negative amp2 in draw 1: spx_factor / spx_ei_step answer SPX_ERR_NOT_PD (LinAlgError) and leave the handle
    unfactored (finish_factor), so spx_set_fantasies and spx_ei_run refuse -- no results of the earlier, good
    factorisation -- and with good hypers the handle is a fresh one's again."""
    p, cand = state_problem()
    first = ph.fant_pass(eng, p, cand)
    bad = p.rows.copy()
    bad[1, 2] = -1.0
    eng.set_hypers(bad)
    with pytest.raises(LinAlgError):
        eng.factor() if entry == "factor" else eng.ei_step(0)
    assert eng.not_pd_info()[0] == 1
    refused(eng.set_fantasies, p.fant, p.bests)
    refused(eng.ei_run, 0)
    refused(eng.ei_draws)
    eng.set_hypers(p.rows)
    refused(eng.ei_run, 0)
    eng.factor()
    eng.set_fantasies(p.fant, p.bests)
    eng.ei_run(0)
    assert_same(ph.collect(eng), first, "recovered")
    assert_same(first, ph.fresh(ph.fant_pass, p, cand), "fresh")


# ---- 8. the multi-device handle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [12, 300])
def test_three_engines_shard_the_candidates(eng, S):
    """spx_multi_set_fantasies replicates the fantasies, spx_multi_ei_run shards the candidates (1000 over three engines:
    334 + 333 + 333): draws, mean and winner of the single handle, bit for bit; cleared, the plain pass."""
    from spearmint_amd.engine import MultiEngine
    p = ph.problem(8010 + S, N=247, D=3, H=3, S=S, n_pend=4)
    cand = ph.candidates(p, 19, 1000)
    single = ph.fant_pass(eng, p, cand)
    check_oracle(single, ph.oracle(p, cand))
    m = MultiEngine([0, 0, 0])
    try:
        assert_same(ph.fant_pass(m, p, cand), single, "three engines")
        m.ei_run(0)
        assert_same(ph.collect(m), single, "again")
        m.set_candidates(cand[:2])                               # fewer candidates than engines
        m.ei_run(0)
        assert_same(ph.collect(m), ph.fresh(ph.fant_pass, p, cand[:2]), "two candidates")
        m.set_candidates(cand)
        m.set_fantasies(None, None)
        m.ei_run(0)
        plain = ph.collect(m)
        assert_same(plain, ph.fresh(ph.plain_pass, p, cand), "cleared")
        assert not np.array_equal(plain["draws"], single["draws"])
    finally:
        m.close()


def test_fantasies_are_refused_in_the_2d_partition(eng):
    from spearmint_amd.engine import MultiEngine
    p = ph.problem(8100, N=150, D=3, H=4, S=5)
    cand = ph.candidates(p, 20, 1000)
    single = ph.fant_pass(eng, p, cand)
    m = MultiEngine([0, 0])
    try:
        m.set_partition(2)
        ph.load(m, p, cand)
        m.factor()
        with pytest.raises(ValueError, match="partition"):
            m.set_fantasies(p.fant, p.bests)
        m.ei_run(0)                                              # the handle survives: the partitioned plain pass
        np.testing.assert_allclose(m.ei_mean(), np.mean(ph.oracle_plain(p, cand), axis=1), rtol=1e-7, atol=0)
        m.set_partition(1)
        assert_same(ph.fant_pass(m, p, cand), single, "back to candidates only")
    finally:
        m.close()
