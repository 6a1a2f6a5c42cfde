"""Max-value entropy search over the fantasies of pending jobs (include/spx.h: option "mes_fantasies"; csrc/mes_fant_kernels.hip),
held as tests/test_gpu_y_mes.py holds the plain pass: every stage of every (draw, fantasy) against tests/mes_oracle.py run on
the device's own inputs of that stage, with that file's bars -- bracket and fit bit for bit; G within (e_dev + e_orc +
ceil(log2 M) + 2) u |G|; y* within 16 u (|a| + |b| (1 + |w|)); a value within the sum over its levels of max(4 e_orc_h, 4) u
unit(gamma) plus the roundings of its sums, here the mean over the S fantasies of those bars plus S u mean|MES_ds| for the
mean itself (any order of S additions).  The means are held bit for bit to the pending EI branch's own, every execution path
to the default path's bits."""
import importlib
import math
import os

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine as spx
from tests import mes_oracle as mo
from tests import pending_helpers as ph
from tests.helpers import branin
from tests.mes_helpers import same_state
from tests.test_gpu_k_constrained_paths import plan_chunks
from tests.test_gpu_y_mes import U, h_tolerance, measured_e_dev, same_bits

pytestmark = pytest.mark.gpu
REFUSAL = "SPX_ACQ_MES is not defined over fantasies"        # spx_ei_run's text with the option off


@pytest.fixture()
def eng():
    e = spx.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mes_tail_mp.npz")))


def run(e, p, cand, K=10, J=256, entry="factor", draw=False, on=1):
    """The handle through a MES pass over the problem's fantasies; returns bests (H, S) as the pass read them."""
    e.set_option("mes_grid", J)
    e.set_option("mes_fantasies", on)
    e.set_acquisition(spx.ACQ_MES, K)
    ph.load(e, p, cand)
    e.ei_step(0) if entry == "step" else e.factor()
    if draw:
        e.draw_fantasies(p.randn, p.pend.shape[0])
        bests = np.array([e.get_pending_fantasies(d)[1] for d in range(p.H)])
    else:
        e.set_fantasies(p.fant, p.bests)
        bests = p.bests
    e.ei_run(0)
    assert e.stat("last_mes_fantasies") == p.S and e.stat("last_mes_samples") == K
    return bests


def collect(e, p):
    out = {"draws": e.ei_draws(), "mean": e.ei_mean(), "best": e.best()}
    out["rec"] = {(d, s): e.mes_fantasy_moments(d, s) + (e.mes_fantasy_info(d, s),) for d in range(p.H) for s in range(p.S)}
    return out


def assert_same(got, ref, what=""):
    assert same_bits(got["draws"], ref["draws"]) and same_bits(got["mean"], ref["mean"]), what
    assert got["best"][0] == ref["best"][0], what
    for key, (m, v, info) in ref["rec"].items():
        m2, v2, info2 = got["rec"][key]
        assert same_bits(m, m2) and same_bits(v, v2), (what, key)
        assert all(same_bits(info[k], info2[k]) for k in ("ystar", "fit", "G")), (what, key)


def one_draw(p, d):
    q = ph.with_columns(p, 0, p.S)
    q.rows, q.fant, q.bests, q.H = p.rows[d:d + 1], q.fant[d:d + 1], q.bests[d:d + 1], 1
    return q


# ---- 1. every stage against the oracle on the device's own inputs ----------------------------------------------------------------
#         (N, D, M, H, S, K, J, draw): M = 1 and around the 512-candidate tile of k_mes_fant_logsurv, 1025 = a second tile of the
#         bounds; S = 1, 2, 3, 9 = one above the block of 8 (and the eight accumulators of the mean plus a tail), 130 = the mean's
#         tree; K = 1024: the levels of 3 fantasies do not fit the values kernel's LDS block at once; N = 130: two row blocks
SHAPES = [(2, 2, 1, 1, 1, 1, 8, False), (130, 3, 511, 3, 2, 10, 256, False), (2, 2, 512, 1, 3, 10, 8, False),
          (130, 3, 513, 3, 9, 1, 256, False), (130, 3, 1025, 1, 9, 10, 8, False), (2, 2, 1, 1, 3, 1024, 8, False),
          (130, 3, 2, 1, 130, 1, 8, False), (130, 3, 513, 1, 3, 10, 256, True)]


@pytest.mark.parametrize("N,D,M,H,S,K,J,draw", SHAPES)
def test_stages_match_oracle(eng, fx, N, D, M, H, S, K, J, draw):
    p = ph.problem(13000 + N + M + S, N=N, D=D, H=H, S=S, n_pend=2 if draw else 3)
    cand = ph.candidates(p, 5, M)
    bests = run(eng, p, cand, K, J, draw=draw)
    res = collect(eng, p)
    e_dev, e_orc = max(measured_e_dev()[0]), float(np.max(fx["orc_err_log_ndtr"][1:]))
    w = np.log(-np.log1p(-((np.arange(K) + 0.5) / K)))
    for d in range(H):
        vals, tols = [], []
        for s in range(S):
            m, v, info = res["rec"][(d, s)]
            lo, hi = mo.bounds(m, v)
            assert same_bits(np.array([lo, hi]), info["fit"][:2]), (d, s)
            G_ref = mo.logsurv(m, v, mo.grid(lo, hi, J))
            bound = (e_dev + e_orc + math.ceil(math.log2(max(M, 2))) + 2) * U * np.abs(G_ref)
            assert np.all(np.abs(info["G"] - G_ref) <= bound), (d, s)
            ys_ref, fit_ref = mo.fit(lo, hi, info["G"], K, bests[d, s], p.rows[d][1])
            assert same_bits(fit_ref, info["fit"]), (d, s, fit_ref, info["fit"])
            ytol = 16 * U * (abs(fit_ref[5]) + abs(fit_ref[6]) * (1 + np.abs(w)))
            assert np.all(np.abs(info["ystar"] - ys_ref) <= ytol) and np.all(info["ystar"] <= fit_ref[7]), (d, s)
            ref = mo.values(m, v, info["ystar"])
            g = (m[:, None] - info["ystar"][None, :]) / np.sqrt(v)[:, None]
            vals.append(ref)
            tols.append(np.sum(h_tolerance(g, fx), axis=1) / K + (K + 1) * U * np.abs(ref))
        ref = np.mean(np.array(vals), axis=0)
        tol = np.mean(np.array(tols), axis=0) + S * U * np.mean(np.abs(vals), axis=0)
        err = np.abs(res["draws"][:, d] - ref)
        print("draw %d: worst value error %.3g of its bound" % (d, float(np.max(err / np.maximum(tol, 1e-320)))))
        assert np.all(err <= tol) and not np.any(np.signbit(res["draws"][:, d])), d
    assert np.array_equal(res["mean"], np.mean(res["draws"], axis=1))
    assert res["best"][0] == int(np.argmax(res["mean"]))


# ---- 2. / 3. bit for bit ------------------------------------------------------------------------------------------------------------
def chunked(p, M):
    budget = 128 * ((p.X.shape[0] + 127) // 128 * 128) * 8 * 2
    nchunks, hb = plan_chunks(M, p.X.shape[0], p.H, budget)
    assert nchunks >= 3 and hb == 1, (nchunks, hb)
    return dict(kstar_budget_bytes=budget)


def test_means_are_the_pending_ei_branch_s(eng):
    """mu[d][s] against the mean the pending EI pass itself forms for that column: the same handle holding column s alone,
    SPX_ACQ_LCB with kappa = 0 (its value is 0 sigma - func_m), negated.  Two row blocks, at least three chunks."""
    p = ph.problem(13100, N=130, S=3)
    cand = ph.candidates(p, 6, 1000)
    with ph.options(eng, **chunked(p, 1000)):
        run(eng, p, cand)
        mu = {k: r[0] for k, r in collect(eng, p)["rec"].items()}
        eng.set_acquisition(spx.ACQ_LCB, 0.0)
        for s in range(p.S):
            eng.set_fantasies(p.fant[:, :, s:s + 1], p.bests[:, s:s + 1])
            eng.ei_run(0)
            draws = eng.ei_draws()
            for d in range(p.H):
                assert same_bits(-draws[:, d], mu[(d, s)]), (d, s)


def test_paths_do_not_change_bits(eng):
    p = ph.problem(13200, N=130, S=3)
    cand = ph.candidates(p, 7, 1000)
    run(eng, p, cand)
    base = collect(eng, p)
    for kw in (chunked(p, 1000), dict(streams=2), dict(streams=3), dict(gemm_partial=0)):
        ph.scramble(eng, p, cand)
        with ph.options(eng, **kw):
            run(eng, p, cand)
            assert_same(collect(eng, p), base, kw)
    ph.scramble(eng, p, cand)
    run(eng, p, cand, entry="step")
    assert_same(collect(eng, p), base, "step")
    for d in range(p.H):                                   # a draw alone against the same draw among three
        q = one_draw(p, d)
        run(eng, q, cand)
        one = collect(eng, q)
        assert same_bits(one["draws"][:, 0], base["draws"][:, d])
        for s in range(p.S):
            assert all(same_bits(one["rec"][(0, s)][2][k], base["rec"][(d, s)][2][k]) for k in ("ystar", "fit", "G"))


# ---- 4. invalid candidates ------------------------------------------------------------------------------------------------------------
def test_invalid_candidates(eng):
    """A NaN candidate row is left out of every fit and is NaN itself (M <= 512: one partial sum, whose order skipping a
    candidate does not change).  One fantasy column NaN at one observation: every mean under it is NaN, that (d, s) has no
    valid candidate and is NaN throughout, and so is the draw; the other draws are what they were."""
    p = ph.problem(13300, N=130, S=3)
    cand = ph.candidates(p, 8, 400)
    bad = cand.copy()
    bad[37, 1] = np.nan
    run(eng, p, bad)
    res = collect(eng, p)
    run(eng, p, np.delete(cand, 37, axis=0))
    ref = collect(eng, p)
    assert np.all(np.isnan(res["draws"][37])) and res["best"][0] == 37
    assert same_bits(np.delete(res["draws"], 37, axis=0), ref["draws"])
    for key in ref["rec"]:
        assert all(same_bits(res["rec"][key][2][k], ref["rec"][key][2][k]) for k in ("ystar", "fit", "G")), key
    q = ph.with_columns(p, 0, p.S)
    q.fant = p.fant.copy()
    q.fant[1, 0, 1] = np.nan
    run(eng, q, np.delete(cand, 37, axis=0))
    got = collect(eng, q)
    info = got["rec"][(1, 1)][2]
    assert np.all(np.isnan(got["rec"][(1, 1)][0])) and np.all(np.isnan(info["ystar"])) and np.all(np.isnan(info["G"]))
    assert np.all(np.isnan(info["fit"][:7])) and np.all(np.isnan(got["draws"][:, 1]))
    assert same_bits(got["draws"][:, [0, 2]], ref["draws"][:, [0, 2]])


# ---- 5. state and refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["off", "set_fantasies", "draw_fantasies", "option", "mes_grid", "set_acquisition",
                                  "set_candidates", "readers", "budget"])
def test_state_and_refusals(eng, case):
    p = ph.problem(13400, N=20, S=2)
    cand = ph.candidates(p, 9, 40)
    if case == "off":
        with pytest.raises(ValueError, match=REFUSAL):
            run(eng, p, cand, on=0)
        with pytest.raises(ValueError):
            eng.mes_fantasy_info(0, 0)
        return
    if case == "budget":        # H S Mp 8 = 3 x 4096 x 44032 x 8 bytes > 4 GiB: refused from the host's record, nothing reserved
        q = ph.with_columns(p, 0, p.S)
        q.fant, q.bests, q.S = np.zeros((p.H, p.X.shape[0], 4096)), np.zeros((p.H, 4096)), 4096
        with pytest.raises(ValueError, match="bytes of means"):
            run(eng, q, np.zeros((44000, p.D)))
        assert eng.stat("last_mes_fantasies") == 0
        return
    run(eng, p, cand)
    if case == "readers":
        with pytest.raises(ValueError, match="spx_get_mes_fantasy"):
            eng.mes_info(0)
        with pytest.raises(ValueError, match="fantasy"):
            eng.ei_grad_batch(cand[:2])
        with pytest.raises(ValueError):
            eng.mes_fantasy_info(0, p.S)
        assert eng.stat("last_mes_fantasies") == p.S        # readers: the table is still held
        return
    {"set_fantasies": lambda: eng.set_fantasies(p.fant, p.bests), "draw_fantasies": lambda: eng.draw_fantasies(p.randn, 3),
     "option": lambda: eng.set_option("mes_fantasies", 1), "mes_grid": lambda: eng.set_option("mes_grid", 256),
     "set_acquisition": lambda: eng.set_acquisition(spx.ACQ_MES, 10), "set_candidates": lambda: eng.set_candidates(cand)}[case]()
    assert eng.stat("last_mes_fantasies") == 0
    with pytest.raises(ValueError):
        eng.mes_fantasy_moments(0, 0)


# ---- 6. the choosers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modname,arg", [("GPEIChooser", "mcmc_iters=4"),
                                         ("GPEIOptChooser", "mcmc_iters=3,burnin=5,grid_subset=4,use_multiprocessing=0")])
def test_choosers_score_a_pending_call_with_mes(golden_dir, tmp_path, modname, arg):
    mod = importlib.import_module("spearmint_amd.chooser." + modname)
    grid = np.array(np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:400], copy=True)
    values = np.full(grid.shape[0], np.nan)
    values[:6] = branin(grid[:6, 0], grid[:6, 1])
    free, pend, done = np.arange(7, grid.shape[0]), np.array([6]), np.arange(6)
    out = {}
    for name, extra in (("mes1", ",acq=MES,mes_pending=1"), ("mes0", ",acq=MES"), ("ei", ",acq=EI")):
        d = tmp_path / name
        d.mkdir()
        ch = mod.init(str(d), arg + extra)
        ch._eng = spx.Engine(0)
        try:
            npr.seed(77)
            job = ch.next(grid, values, np.full(grid.shape[0], np.nan), free, pend, done)
            out[name] = (job, npr.get_state(), ch.last_acq_used, int(free[ch._eng.best()[0]]) if name == "mes1" else None)
        finally:
            ch._eng.close()
    assert out["mes1"][2] == "MES" and out["mes0"][2] == "EI" and out["ei"][2] == "EI"
    assert out["mes1"][0] == out["mes1"][3]                  # the grid point of the engine's own argmax
    assert same_state(out["mes1"][1], out["ei"][1]) and same_state(out["mes0"][1], out["ei"][1])
    a, b = out["mes0"][0], out["ei"][0]                      # mes_pending=0: today's proposal, a grid index or (index, point)
    assert (a[0] == b[0] and np.array_equal(a[1], b[1])) if isinstance(b, tuple) else a == b
    with pytest.raises(ValueError):
        mod.init(str(tmp_path), arg + ",acq=EI,mes_pending=1")
