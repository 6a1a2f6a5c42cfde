"""KG over pending fantasies in the wide form (option "kg_fantasies" = 2; csrc/kg_fant_scan_kernels.hip), A up to 1023: values against
tests/kg_oracle.py at tests/test_gpu_zx_kg_pending.py's bar; bit for bit against the narrow form; plain KG per fantasy; paths; state."""
import functools
import importlib
import os
import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine as spx
from tests import kg_helpers as kh
from tests import kg_mp as km
from tests import kg_oracle as ko
from tests import pending_helpers as ph
from tests.helpers import branin
from tests.mes_helpers import same_state
from tests.test_gpu_zv_kg import fx  # noqa: F401  (the fixture: tests/golden/kg_mp.npz)
from tests.test_gpu_zx_kg_pending import KEEP, assert_same, eng, hold_values, points_for, run  # noqa: F401

pytestmark = pytest.mark.gpu
wide = functools.partial(run, on=2)


def scan_points(e, pts):                                      # (points beyond 255 are taken while "kg_scan" is 1)
    e.set_option("kg_scan", 1 if pts.shape[0] > 255 else 0)
    return pts


# A, S, M, N, H, covar, draw: 8-bit index / ninth stack word; the pad boundary, S = 33, a full wave; n = 1024; S = 1; S = 100; small n
SHAPES = [
    (256, 3, 19, 67, 1, "Matern52", False),
    (511, 33, 9, 67, 1, "Matern32", False),
    (512, 64, 9, 67, 1, "Matern52", False),
    (1023, 65, 5, 129, 1, "Matern52", False),
    (1023, 1, 33, 67, 1, "Matern32", False),
    (300, 100, 17, 67, 1, "Matern52", False),
    (5, 2, 257, 67, 3, "Matern52", False),
    (64, 8, 255, 129, 1, "Matern32", True),
]


@pytest.mark.parametrize("A,S,M,N,H,covar,draw", SHAPES)
def test_values_against_the_oracle_on_the_device_s_lines(eng, fx, A, S, M, N, H, covar, draw):
    p = ph.problem(15000 + A + S, covar, N=N, D=3, H=H, S=S, n_pend=3)
    cand = ph.candidates(p, 3, M)
    if M > 100:
        cand[57, 0] = np.nan                                  # a non-finite mu_c[s]: NaN for that (d, c) alone
    try:
        out = wide(eng, p, cand, scan_points(eng, points_for(p, cand, A, A)), draw=draw)
        assert eng.stat("last_kg_scan") == 1
    finally:
        eng.set_covar("Matern52")
        eng.set_option("kg_scan", 0)
    hold_values(fx, out, p, "A=%d S=%d M=%d N=%d H=%d %s" % (A, S, M, N, H, covar))
    assert not np.any(np.isnan(out["draws"][np.arange(M) != 57])) and (M < 100 or np.all(np.isnan(out["draws"][57])))


@pytest.mark.parametrize("A", [2, 64, 255])
@pytest.mark.parametrize("S", [9, 64])
def test_bit_for_bit_against_the_narrow_form(eng, A, S):
    p = ph.problem(15100 + A + S, N=67, D=3, H=2, S=S, n_pend=3)
    cand = ph.candidates(p, 5, 131)
    cand[57, 1] = np.nan
    pts = points_for(p, cand, A, A)
    assert_same(wide(eng, p, cand, pts), run(eng, p, cand, pts), (A, S))


@pytest.mark.parametrize("S,cols", [(1, (0,)), (9, (0, 8))])
def test_it_is_plain_kg_per_fantasy(eng, fx, S, cols):
    """A second handle given ([completed; pending], fant[d][:, s]), kg_scan=1: KG_ds within two bars, cov and func_v bit for bit."""
    p = ph.problem(15200 + S, N=67, D=3, H=2, S=S, n_pend=3)
    cand = ph.candidates(p, 4, 40)
    pts = scan_points(eng, points_for(p, cand, 300, 2))
    full, e2 = wide(eng, p, cand, pts), spx.Engine(0)
    try:
        e2.set_option("kg_scan", 1)
        for s in cols:
            for d in range(p.H):
                e2.set_observations(p.X, np.ascontiguousarray(p.fant[d][:, s])); e2.set_candidates(cand); e2.set_hypers(p.rows[d:d + 1])
                e2.set_kg_points(pts); e2.set_acquisition("KG")
                e2.ei_step(KEEP)
                plain, (mu_a, cov), (fm, fv) = e2.ei_draws()[:, 0], e2.kg_lines(0), e2.get_moments(0)
                assert np.array_equal(cov, full["cov"][d]) and np.array_equal(fv, full["v"][d]), (s, d)
                mu, b = ko.lines(fm, fv, p.rows[d, 1], mu_a, cov)
                one = full["draws"][:, d] if S == 1 else wide(eng, ph.with_columns(p, s, s + 1), cand, pts)["draws"][:, d]
                for c in range(cand.shape[0]):
                    u, band = ko.unit(mu[c], b[c]), km.band_of(ko.zmax(mu[c], b[c]))
                    assert km.error(one[c:c + 1], plain[c:c + 1], np.array([u])) <= 2 * kh.MARGIN * km.pinned(fx, band), (s, d, c)
    finally:
        e2.close()
        eng.set_option("kg_scan", 0)


def test_paths_do_not_change_bits(eng):
    p = ph.problem(15300, N=101, D=3, H=3, S=9, n_pend=3)
    cand, Np = ph.candidates(p, 7, 1000), 128
    pts = scan_points(eng, points_for(p, cand, 300, 3))
    try:
        base = wide(eng, p, cand, pts)
        for kw in (dict(kstar_budget_bytes=8 * Np * 256), dict(kstar_budget_bytes=8 * Np * 1024), dict(streams=2),
                   dict(streams=3, kstar_budget_bytes=8 * Np * 256), dict(gemm_partial=0)):
            ph.scramble(eng, p, cand)
            with ph.options(eng, **kw):
                assert_same(wide(eng, p, cand, pts), base, kw)
        assert_same(wide(eng, p, cand, pts, entry="step"), base, "step")
        assert_same(wide(eng, p, cand, pts, flags=0), base, "without the moments")
        for d in range(p.H):                                  # a draw alone against the same draw among three
            q = ph.with_columns(p, 0, p.S)
            q.rows, q.fant, q.bests, q.H = p.rows[d:d + 1], p.fant[d:d + 1], p.bests[d:d + 1], 1
            one = wide(eng, q, cand, pts)
            assert np.array_equal(one["draws"][:, 0], base["draws"][:, d], equal_nan=True) and np.array_equal(one["mu_a"][0], base["mu_a"][d])
    finally:
        eng.set_option("kg_scan", 0)


def test_state_refusals_and_statistics(eng):
    p = ph.problem(15400, N=67, D=2, H=2, S=3, n_pend=3)
    cand, pts = ph.candidates(p, 8, 130), np.random.RandomState(1).rand(256, 2)
    try:
        eng.set_option("kg_scan", 1)
        with pytest.raises(ValueError, match="256 representer points.*kg_fantasies"):
            run(eng, p, cand, pts, on=1)
        base = wide(eng, p, cand, pts)                        # (run() asserts last_kg_fantasies == S and last_kg_points == A)
        assert eng.stat("last_kg_scan") == 1
        eng.set_option("kg_scan", 0)                          # the wide form orders its lines itself
        eng.ei_run(KEEP)
        assert np.array_equal(eng.ei_draws(), base["draws"])
        for call in (lambda: eng.ei_run(spx.FLAG_PER_SEC), lambda: eng.ei_run(spx.FLAG_CONSTRAINED), lambda: eng.ei_grad_batch(np.zeros((1, 2))),
                     lambda: eng.ei_grad(np.zeros(2)), lambda: eng.constrained_ei_grad_batch(np.zeros((1, 2)), 0.0)):
            with pytest.raises(ValueError):
                call()
            assert eng.stat("last_kg_fantasies") == p.S and np.array_equal(eng.ei_draws(), base["draws"])
        eng.set_option("kg_fantasies", 2)                     # setting the option drops the results
        assert eng.stat("last_kg_fantasies") == 0 and eng.stat("last_kg_scan") == 0
        eng.set_fantasies(np.zeros((p.H, 67, 3841)), np.zeros((p.H, 3841)))
        with pytest.raises(ValueError, match=r"S \+ A = 3841 \+ 256"):
            eng.ei_run(0)
        eng.set_candidates(np.random.RandomState(1).rand(1100000, 2))
        eng.set_fantasies(p.fant, p.bests)
        with pytest.raises(ValueError, match="2 x 257 x 1100032 x 10 = %d bytes of ordered slopes" % (2 * 257 * 1100032 * 10)):
            eng.ei_run(0)
    finally:
        eng.set_option("kg_scan", 0)


@pytest.mark.parametrize("modname,arg", [("GPEIChooser", "mcmc_iters=4"),
                                         ("GPEIOptChooser", "mcmc_iters=3,burnin=5,grid_subset=4,use_multiprocessing=0")])
def test_choosers_score_a_pending_call_with_kg(golden_dir, tmp_path, modname, arg):
    mod = importlib.import_module("spearmint_amd.chooser." + modname)
    grid = np.array(np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:400], copy=True)
    values = np.full(grid.shape[0], np.nan)
    values[:6] = branin(grid[:6, 0], grid[:6, 1])
    free, pend, done = np.arange(7, grid.shape[0]), np.array([6]), np.arange(6)
    out = {}
    for name, extra in (("obs", ",acq=KG,kg_scan=1,kg_points=observed,kg_pending=2"),
                        ("grid", ",acq=KG,kg_scan=1,acq_par=300,kg_pending=2"), ("ei", ",acq=EI")):
        (tmp_path / name).mkdir()
        ch = mod.init(str(tmp_path / name), arg + extra)
        ch._eng = spx.Engine(0)
        try:
            npr.seed(77)
            job = ch.next(grid, values, np.full(grid.shape[0], np.nan), free, pend, done)
            out[name] = (job, npr.get_state(), ch.last_acq_used, ch.last_kg)
        finally:
            ch._eng.close()
    assert out["ei"][2] == "EI" and len(out["obs"][3]["points_index"]) == 6 and len(out["grid"][3]["points_index"]) == 300
    for name in ("obs", "grid"):
        job, state, used, kg = out[name]
        assert used == "KG" and kg["value"] >= 0.0 and job == int(free[kg["grid_index"]]) and same_state(state, out["ei"][1])
