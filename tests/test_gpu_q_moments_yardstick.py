"""func_m and func_v -- the two numbers per candidate that every acquisition, LOO, main effects and the constrained and
per-second passes read -- against the long-double yardstick of tests/moments_ld.py, path by path: W = L^-1 (k_trinv<true/false>),
beta = W K* (k_ei_fused128, k_predict_gemm_tail<1..3>, k_predict_gemm_tri, the rectangular k_predict_gemm variants), the
epilogue's sum beta^2 and sum beta gamma, their sum over row blocks and prior_v - ss in k_ei_finalize.

One case: set_observations / set_candidates / set_hypers with three draws, factor(), ei_run(KEEP_MOMENTS); per draw the
references take the DEVICE's K (spx_get_factor) and K* (spx_get_cross_cov, on moments_ld.yardstick_columns) as exact inputs, so
the covariance's rounding stays out (tests/test_gpu_q_cov_yardstick.py holds it; K is still asserted to be the oracle's to 1e-13).
Units (tests/moments_ld.py): func_m relative to |B[:, c]| |gamma| + |mean|, func_v relative to prior_v.  Bar, for each of the two
over the three draws and the columns: err_device <= max(4 x max(err_lapack, err_as_built), 16 x 2^-52) -- the factor and the
floor of tests/test_gpu_o_factor_pivots.py -- where err_lapack is the reference's route (dpotrf, cho_solve, solve_triangular)
and err_as_built a plain numpy restatement of W = L^-1, beta = W K* on the same inputs, each against the long-double values.
Exact, in every path: a candidate with every coordinate 1e3 has a K* column of zeros, func_m == mean and func_v == prior_v.
Which path ran is asserted from spx_get_stat and tests/pending_helpers.padding_plan, not assumed.  The problems put candidates
ON observations and 1e-9 beside them (func_v ~ 1e-6 prior_v: where prior_v - ss cancels), in three noise bands
(as drawn, 1e-6 amp2, 1e-9 amp2); tests/test_moments_ld.py qualifies every one of them on the CPU.

Measured on an MI355X (144 cases, 9 s).  Per group: the worst device / max(lapack, as built) of a case for func_m, func_v
(bar 4); then the worst errors device; lapack; as built of func_m -- of func_v:
  fused, N = 2 ... 128                    2.75, 2.26    1.8e-13; 6.6e-14; 6.0e-14 -- 2.1e-14; 8.1e-15; 1.5e-14
  one row block, tail alone, 16 ... 96    1.58, 1.50    5.4e-14; 3.8e-14; 4.6e-14 -- 9.4e-15; 6.2e-15; 6.5e-15
  one row block, padded, 97 and 128       2.75, 2.26    1.8e-13; 6.6e-14; 6.0e-14 -- 2.1e-14; 8.1e-15; 1.5e-14
  two row blocks, tail, 129 ... 224       1.12, 2.35    2.5e-13; 2.4e-13; 2.6e-13 -- 2.8e-14; 2.0e-14; 1.8e-14
  two row blocks, padded, 225 and 256     1.83, 1.53    2.6e-13; 1.8e-13; 2.3e-13 -- 1.6e-14; 1.2e-14; 1.9e-14
  three row blocks, 257 ... 384           1.26, 1.76    2.9e-13; 3.6e-13; 3.9e-13 -- 1.9e-14; 3.7e-14; 2.6e-14
  ARDSE, 130 (band c) and 300 (band b)    1.64, 2.65    3.4e-12; 2.0e-12; 2.1e-12 -- 5.0e-13; 1.9e-13; 1.9e-13
  gemm_waves 4, 14, 24 / 8, 18 / 32       1.26, 1.07 / 1.26, 1.11 / 1.26, 1.09      2.9e-13; 2.6e-13; 2.7e-13 -- 1.7e-14; 2.3e-14; 1.5e-14
  candidate tiles, M = 1, 129, 1100       1.80, 1.70    4.7e-14; 4.0e-14; 4.0e-14 -- 7.8e-15; 6.2e-15; 6.0e-15
(the fused kernel and the one-block tri kernel give the same bits at N = 128, hence the same worst case).

Shown to bite, two scratch builds, each run once and not committed.  (1) beta's low 16 mantissa bits cleared before it is squared
and multiplied by gamma in k_predict_gemm_tri's and k_ei_fused128's epilogues (a relative error of about 1.5e-11, always
towards zero): 83 of the 144 cases fail -- fused 18 of 18, one row block padded 6 of 6, two row blocks 18 + 6, three row blocks
12, ARDSE 2, candidate tiles 9, gemm_waves=32 6, and the gemm_partial=0 identity 6 (the tail kernel is not the mutated one);
func_v at 600 ... 26 000 x the references' error, func_m at 50 ... 9 900 x.  The tail kernel alone, the rectangular kernels and
the identities between two mutated passes pass, as they must.  tests/test_gpu_a_parity.py::test_oracle_stages fails with that
build too, in all 12 cases -- not at its rtol = 1e-9 on the moments but at the EI bound of 1e-7 (1.4e-7 ... 4.7e-6): a one-sided
error of ss is amplified by prior_v / func_v ~ 1e4 at the candidates jittered around the incumbent.  (2) Only the low 8 bits
cleared (about 5.7e-14): test_oracle_stages passes in all 12 cases; this file fails in 78 -- func_v at 15 ... 101 x the
references' in every fused, tri and tail + tri group (ARDSE and three of the three-row-block cases stay inside), func_m inside
except in the fused group (38 x).
"""
import numpy as np
import pytest

from oracle import gp_ei_oracle as orc
from tests import moments_ld as ml
from tests import pending_helpers as ph
from tests.pending_helpers import FLAG_KEEP_MOMENTS, options
from tests.test_gpu_k_constrained_paths import plan_chunks

pytestmark = pytest.mark.gpu
FACTOR = 4.0
FLOOR = 16 * 2.0 ** -52
REFS = {}                 # problem key -> the device's K and K* of every draw with the three reference computations on them
MEASURED = []             # (group, key, options, device (m, v), lapack (m, v), as built (m, v))
BANDS = sorted(ml.BANDS)


@pytest.fixture(scope="module")
def eng():
    from spearmint_amd.engine import Engine
    assert np.finfo(np.longdouble).nmant >= 63, "the yardstick needs the 80-bit extended format"
    e = Engine(0)
    yield e
    e.set_covar("Matern52")
    e.close()


def expected_path(N, opts):
    """(fused, padding skipped) of the pass, from the plan's rules (csrc/spx_plan.h: plan_ei, predict_gemm_padding_plan)."""
    fused = N <= 128 and opts.get("ei_fused", -1) != 0
    production = opts.get("gemm_waves", 0) in (0, 32)
    skipped = not fused and production and opts.get("gemm_partial", -1) != 0 and ph.padding_plan(N)[1]
    return fused, skipped


def run_pass(eng, key, step=False, **opts):
    """One pass under `opts`: per draw K, K* on the yardstick columns, func_m and func_v of every candidate -- after the path
    has been asserted and the far candidates have been held exactly."""
    p = ml.table_problem(key)
    N, M = p.comp.shape[0], p.cand.shape[0]
    cols, far = ml.yardstick_columns(M), ml.far_columns(p)
    out = {"K": [], "Ks": [], "m": [], "v": [], "cols": cols}
    with options(eng, **opts):
        eng.set_covar(p.covar)
        eng.set_observations(p.comp, p.vals)
        eng.set_candidates(p.cand)
        eng.set_hypers(p.rows)
        if step:
            eng.ei_step(FLAG_KEEP_MOMENTS)
        else:
            eng.factor()
            eng.ei_run(FLAG_KEEP_MOMENTS)
        fused, skipped = expected_path(N, opts)
        assert eng.stat("last_step_fused") == int(fused), (key, opts)
        assert eng.stat("last_step_skipped_padding") == int(skipped), (key, opts)
        if "ei_flow" in opts:
            assert eng.stat("last_factor_flow") == opts["ei_flow"]
        for h in range(ml.H):
            m, v = eng.get_moments(h)
            Ks = eng.get_cross_cov(h)
            out["m"].append(m)
            out["v"].append(v)
            out["Ks"].append(np.ascontiguousarray(Ks[:, cols]))
            out["K"].append(eng.get_factor(h, want_L=False, want_alpha=False)[0])
            assert M == 1 or len(far) == ml.FAR
            assert np.array_equal(Ks[:, far], np.zeros((N, len(far)))), (key, opts, h)
            assert np.array_equal(m[far], np.full(len(far), p.rows[h, 0])), (key, opts, h)
            assert np.array_equal(v[far], np.full(len(far), ml.prior_v_of(p.rows[h]))), (key, opts, h)
    return out


def references(key, got):
    """The three reference computations on the device's K and K* of the problem, made once; a later case of the same problem
    must have produced the same K and K* bit for bit."""
    p = ml.table_problem(key)
    if key in REFS:
        r = REFS[key]
        for h in range(ml.H):
            assert np.array_equal(got["K"][h], r["K"][h]) and np.array_equal(got["Ks"][h], r["Ks"][h]), (key, h)
        return r
    r = {"K": got["K"], "Ks": got["Ks"], "ref": [], "lapack": np.zeros(2), "built": np.zeros(2)}
    for h in range(ml.H):
        mean, noise, amp2, ls = orc.unpack_hyper(p.rows[h])
        with orc.covar(p.covar):
            K_orc = orc.cov(amp2, ls, p.comp) + noise * np.eye(p.comp.shape[0])
        np.testing.assert_allclose(got["K"][h], K_orc, rtol=1e-13, atol=0)
        args = (got["K"][h], got["Ks"][h], p.vals - mean, float(mean), ml.prior_v_of(p.rows[h]))
        ref = ml.moments_longdouble(*args)
        r["ref"].append(ref)
        r["lapack"] = np.maximum(r["lapack"], ml.errors(*ml.moments_lapack(*args), ref=ref))
        r["built"] = np.maximum(r["built"], ml.errors(*ml.moments_as_built(*args), ref=ref))
    REFS[key] = r
    return r


def hold(group, key, got, opts):
    """The bar."""
    r = references(key, got)
    cols = got["cols"]
    dev = np.zeros(2)
    for h in range(ml.H):
        dev = np.maximum(dev, ml.errors(got["m"][h][cols], got["v"][h][cols], r["ref"][h]))
    own = np.maximum(r["lapack"], r["built"])
    with np.errstate(divide="ignore", invalid="ignore"):
        rl, rb = dev / r["lapack"], dev / r["built"]
    print("%-22s %s %s: func_m device %.2e lapack %.2e as built %.2e (x%.2f, x%.2f); func_v device %.2e lapack %.2e "
          "as built %.2e (x%.2f, x%.2f)"
          % (group, key, opts, dev[0], r["lapack"][0], r["built"][0], rl[0], rb[0],
             dev[1], r["lapack"][1], r["built"][1], rl[1], rb[1]))
    MEASURED.append((group, key, dict(opts), dev, r["lapack"].copy(), r["built"].copy()))
    for name, d, o in zip(("func_m", "func_v"), dev, own):
        assert d <= max(FACTOR * o, FLOOR), (group, key, opts, name, d, o)


def same_moments(a, b, what):
    for h in range(ml.H):
        assert np.array_equal(a["m"][h], b["m"][h]) and np.array_equal(a["v"][h], b["v"][h]), (what, h)


def with_bands(ns):
    return [(N, band) for N in ns for band in BANDS]


# ---- the yardstick, group by group -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,band", with_bands(ml.FUSED_NS))
def test_fused_kernel(eng, N, band):
    """k_ei_fused128, 1 ... 8 live row tiles."""
    key = ml.key_of(N, band)
    got = run_pass(eng, key)
    assert eng.stat("last_step_fused") == 1
    hold("fused", key, got, {})


@pytest.mark.parametrize("N,band", with_bands(ml.ONE_BLOCK_TAIL_NS))
def test_one_row_block_tail_kernel_alone(eng, N, band):
    """ei_fused=0 at N <= 96: k_predict_gemm_tail<1, 1, 2, 3, 3> is the pass's only GEMM launch."""
    lt, skips = ph.padding_plan(N)
    assert skips and (lt + 1) // 2 == {16: 1, 17: 1, 33: 2, 65: 3, 96: 3}[N]
    key = ml.key_of(N, band)
    hold("one row block", key, run_pass(eng, key, ei_fused=0), dict(ei_fused=0))


@pytest.mark.parametrize("N,band", with_bands(ml.ONE_BLOCK_PADDED_NS))
def test_one_row_block_padded(eng, N, band):
    """ei_fused=0 at N = 97 and 128: k_predict_gemm_tri on one row block (the plan declines to skip 7 and 8 live tiles)."""
    assert not ph.padding_plan(N)[1]
    key = ml.key_of(N, band)
    hold("one row block, padded", key, run_pass(eng, key, ei_fused=0), dict(ei_fused=0))


@pytest.mark.parametrize("N,band", with_bands(ml.TWO_BLOCK_TAIL_NS))
def test_two_row_blocks_tail(eng, N, band):
    """The tail kernel with 1 ... 6 live tiles and k_predict_gemm_tri on the full block: two partial sums per candidate."""
    lt, skips = ph.padding_plan(N)
    assert skips and lt == ml.TWO_BLOCK_TAIL_NS.index(N) + 1
    key = ml.key_of(N, band)
    hold("two row blocks, tail", key, run_pass(eng, key), {})


@pytest.mark.parametrize("N,band", with_bands(ml.TWO_BLOCK_PADDED_NS))
def test_two_row_blocks_padded(eng, N, band):
    assert not ph.padding_plan(N)[1]
    key = ml.key_of(N, band)
    hold("two row blocks, padded", key, run_pass(eng, key), {})


@pytest.mark.parametrize("N,band", with_bands(ml.THREE_BLOCK_NS))
def test_three_row_blocks(eng, N, band):
    """257 and 300: the tail with 1 and 3 live tiles; 353: padded (7 live tiles); 384: full."""
    assert ph.padding_plan(N) == {257: (1, True), 300: (3, True), 353: (7, False), 384: (8, False)}[N]
    key = ml.key_of(N, band)
    hold("three row blocks", key, run_pass(eng, key), {})


@pytest.mark.parametrize("N,band", ml.ARDSE_CASES)
def test_ardse(eng, N, band):
    key = ml.key_of(N, band, covar="ARDSE")
    hold("ARDSE", key, run_pass(eng, key), {})


@pytest.mark.parametrize("N,band", with_bands(ml.VARIANT_NS))
@pytest.mark.parametrize("variant", ml.VARIANTS)
def test_rectangular_kernels(eng, variant, N, band):
    """gemm_waves = 4 / 8 / 14 / 18 / 24: each rectangular k_predict_gemm<NW, STG> held on its own (they are not the production
    kernel's bits and never skip the padding); 32 is the production kernel: held, and the default's bits."""
    key = ml.key_of(N, band)
    got = run_pass(eng, key, gemm_waves=variant)
    hold("gemm_waves=%d" % variant, key, got, dict(gemm_waves=variant))
    if variant == 32:
        same_moments(got, run_pass(eng, key), "gemm_waves 32 against 0")


@pytest.mark.parametrize("M,band", [(M, band) for M in ml.TILE_MS for band in BANDS])
def test_candidate_tiles(eng, M, band):
    """N = 130 with 1, 2 and 9 candidate tiles of 128 (M = 1, 129, 1100: ncbx = 2 with empty XCD slots), on the yardstick
    columns: every tile edge, the special rows and a seeded fill."""
    key = ml.key_of(ml.TILE_N, band, M=M)
    cols = ml.yardstick_columns(M)
    assert len(cols) == min(M, ml.MAX_COLUMNS) and (M < 129 or {127, 128, M - 1} <= set(cols.tolist()))
    hold("candidate tiles", key, run_pass(eng, key), {})


# ---- the same bits on the other paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,band", with_bands(ml.NOT_SKIPPED_NS))
def test_padding_not_skipped_gives_the_same_bits(eng, N, band):
    """gemm_partial=0: k_predict_gemm_tri on the padded last row block."""
    assert ph.padding_plan(N)[1]
    key = ml.key_of(N, band)
    base = run_pass(eng, key)
    same_moments(run_pass(eng, key, gemm_partial=0), base, "gemm_partial=0")


@pytest.mark.parametrize("N,band", with_bands(ml.FACTOR_STORAGE_NS))
def test_factor_storage_gives_the_same_bits(eng, N, band):
    """ei_flow=0: the row-major factorisation and k_trinv<false> against k_lean_flow's tile-major store and k_trinv<true>."""
    key = ml.key_of(N, band)
    a, b = run_pass(eng, key, ei_flow=1), run_pass(eng, key, ei_flow=0)
    same_moments(b, a, "ei_flow=0")
    for h in range(ml.H):
        assert np.array_equal(a["K"][h], b["K"][h]) and np.array_equal(a["Ks"][h], b["Ks"][h])


@pytest.mark.parametrize("band", BANDS)
def test_chunks_give_the_same_bits(eng, band):
    """A staging budget of one 128-column tile of one draw: nine chunks, c0 > 0 in k_ei_finalize."""
    key = ml.key_of(ml.CHUNK_N, band, M=ml.CHUNK_M)
    budget = 8 * ((ml.CHUNK_N + 127) // 128 * 128) * 128
    assert plan_chunks(ml.CHUNK_M, ml.CHUNK_N, ml.H, budget) == (9, 1)
    base = run_pass(eng, key)
    same_moments(run_pass(eng, key, kstar_budget_bytes=budget), base, "chunks")


@pytest.mark.parametrize("N,band", with_bands(ml.STEP_NS))
def test_step_gives_the_same_bits(eng, N, band):
    """spx_ei_step(KEEP_MOMENTS) against spx_factor + spx_ei_run: fused (128) and tail + tri (177)."""
    key = ml.key_of(N, band)
    base = run_pass(eng, key)
    same_moments(run_pass(eng, key, step=True), base, "step")


# ---- what was measured -----------------------------------------------------------------------------------------------------------
def test_zz_report_the_measured_ratios():
    """Per group: the worst device error, the two references' worst, and the worst device / max(lapack, as built) of a case."""
    assert MEASURED, "no yardstick case ran before the report"
    groups = []
    for g in (m[0] for m in MEASURED):
        if g not in groups:
            groups.append(g)
    for g in groups:
        rows = [m for m in MEASURED if m[0] == g]
        dev = np.max([m[3] for m in rows], axis=0)
        lap = np.max([m[4] for m in rows], axis=0)
        built = np.max([m[5] for m in rows], axis=0)
        ratio = np.max([m[3] / np.maximum(np.maximum(m[4], m[5]), FLOOR / FACTOR) for m in rows], axis=0)
        print("%-22s %3d cases: func_m device %.1e lapack %.1e as built %.1e worst ratio %.2f | func_v device %.1e lapack %.1e "
              "as built %.1e worst ratio %.2f (bar %.0f)"
              % (g, len(rows), dev[0], lap[0], built[0], ratio[0], dev[1], lap[1], built[1], ratio[1], FACTOR))
