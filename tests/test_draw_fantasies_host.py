"""spx_draw_fantasies without a GPU: the header and the binding declare it, the choosers hand the library the very normals
the reference draws (and nothing else) when gpu_fantasies is on, the host path when it is off or there are more pending
points than the library takes, and the factored form of Gamma the kernels write equals the dense triangular solve."""
import os
import re

import numpy as np
import numpy.random as npr
import scipy.linalg as spla

from spearmint_amd import hostgp
from spearmint_amd.chooser import GPEIChooser, GPEIOptChooser
from tests import fantasy_helpers as fh
from tests.helpers import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_entry_points():
    from spearmint_amd import engine
    text = open(os.path.join(ROOT, "include", "spx.h")).read()
    assert re.search(r"#define\s+SPX_MAX_PENDING\s+64\b", text)
    assert re.search(r"int\s+spx_draw_fantasies\(spx_handle\*\s*h,\s*int32_t\s+P,\s*const double\*\s*z,\s*int32_t\s+per_draw,"
                     r"\s*int32_t\s+S\);", text)
    assert re.search(r"int\s+spx_get_pending_fantasies\(spx_handle\*\s*h,\s*int32_t\s+draw,\s*double\*\s*pend_fant,"
                     r"\s*double\*\s*bests\);", text)
    assert "last_fantasies_device" in text
    assert engine.MAX_PENDING == 64
    assert "spx_draw_fantasies" in engine.ABI and "spx_get_pending_fantasies" in engine.ABI
    assert callable(engine.Engine.draw_fantasies) and callable(engine.Engine.get_pending_fantasies)


class Recorder(OracleEngine):
    """The oracle engine with a draw_fantasies of its own (the host form on its own factor rows), counting who is asked
    for what."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.drawn, self.rows_asked, self.fant_set = [], 0, 0

    def draw_fantasies(self, z, n_pend):
        z = np.asarray(z, float)
        self.drawn.append((z.copy(), int(n_pend)))
        n = self.comp.shape[0] - n_pend
        H = self.hypers.shape[0]
        fb = []
        for h in range(H):
            l_rows, gam = OracleEngine.get_factor_rows(self, h, n, n_pend)
            fb.append(hostgp.fantasize_from_factor_rows(self.vals[:n], self.hypers[h], l_rows, gam, z[h] if z.ndim == 3 else z))
        OracleEngine.set_fantasies(self, np.array([x[0] for x in fb]), np.array([x[1] for x in fb]))

    def get_factor_rows(self, *a, **kw):
        self.rows_asked += 1
        return OracleEngine.get_factor_rows(self, *a, **kw)

    def set_fantasies(self, fant, bests):
        self.fant_set += 1
        OracleEngine.set_fantasies(self, fant, bests)


def _opt_pending(golden_dir, tmp_path, extra):
    g = np.load(os.path.join(golden_dir, "chooser_next_pending.npz"))
    tmp_path.mkdir()
    ch = GPEIOptChooser.init(str(tmp_path), "mcmc_iters=3,burnin=4,grid_subset=3,pending_samples=8,use_multiprocessing=0" + extra)
    eng = Recorder()
    ch._eng = eng
    npr.seed(int(g["o_seed"]))
    job = ch.next(g["grid"], g["values"], g["durations"], g["candidates"], g["pending"], g["complete"])
    if int(g["o_is_new"]):
        assert isinstance(job, tuple) and job[0] == int(g["o_index"])
        assert np.allclose(job[1], g["o_point"], atol=1e-6)
    else:
        assert job == int(g["o_index"])
    passes = [c for c in eng.calls if c[0] == "ei_run"]
    return g, ch, eng, passes, npr.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_opt_chooser_hands_the_library_the_reference_normals(golden_dir, tmp_path):
    """The reference's pending golden next() of GPEIOptChooser with gpu_fantasies=1: draw_fantasies once per pass with
    (H, P, S) normals, every draw's the replay of the state the reference restores before each fantasy draw
    (GPEIOptChooser.py:588); no factor row and no H x n x S array is asked for.  gpu_fantasies=0: the opposite, the same
    job and the global generator left in the same state."""
    g, ch, eng, passes, state1 = _opt_pending(golden_dir, tmp_path / "dev", ",gpu_fantasies=1")
    P = len(g["pending"])
    assert len(eng.drawn) == len(passes) >= 2 and eng.rows_asked == 0 and eng.fant_set == 0
    rs = npr.RandomState()
    rs.set_state(ch.randomstate)
    want = rs.randn(P, 8)
    for z, n_pend in eng.drawn:
        assert z.shape == (3, P, 8) and n_pend == P
        for d in range(3):
            assert np.array_equal(z[d], want)
    _, _, host, passes0, state0 = _opt_pending(golden_dir, tmp_path / "host", ",gpu_fantasies=0")
    assert host.drawn == [] and host.fant_set == len(passes0) == len(passes) and host.rows_asked == 3 * len(passes0)
    assert _same_state(state0, state1)
    _, _, auto, _, _ = _opt_pending(golden_dir, tmp_path / "auto", "")
    assert len(auto.drawn) == len(passes) and auto.fant_set == 0          # auto: the library where it can


def test_gpei_chooser_passes_the_normals_in_the_order_they_were_drawn(golden_dir, tmp_path, monkeypatch):
    """GPEIChooser draws one (P, S) array right after each hyper sample (GPEIChooser.py:238): the arrays npr.randn
    returned, in that order, are z[0], z[1], z[2] of the one draw_fantasies call, and the job is the golden one."""
    g = np.load(os.path.join(golden_dir, "chooser_next_pending.npz"))
    P = len(g["pending"])
    ch = GPEIChooser.init(str(tmp_path), "mcmc_iters=3,pending_samples=9,gpu_fantasies=1")
    eng = Recorder()
    ch._eng = eng
    seen = []
    real = npr.randn

    def randn(*shape):
        out = real(*shape)
        if shape == (P, 9):
            seen.append(out.copy())
        return out
    monkeypatch.setattr(npr, "randn", randn)
    npr.seed(int(g["g_seed"]))
    job = ch.next(g["grid"], g["values"], g["durations"], g["candidates"], g["pending"], g["complete"])
    assert job == int(g["g_job"])
    assert len(eng.drawn) == 1 and eng.rows_asked == 0 and eng.fant_set == 0 and len(seen) == 3
    assert np.array_equal(eng.drawn[0][0], np.array(seen))
    assert np.allclose(ch.last_overall_ei, g["g_ei"], rtol=1e-8, atol=1e-300)


def test_more_pending_points_than_the_library_takes_fall_back_to_the_host(tmp_path):
    rs = np.random.RandomState(3)
    for n_pend, device in ((64, True), (65, False)):
        comp, pend = rs.rand(12, 2), rs.rand(n_pend, 2)
        vals = np.sum(comp ** 2, axis=1)
        rows = np.array([[0.3, 1e-2, 1.0, 0.8, 1.1]])
        ch = GPEIChooser.init(str(tmp_path), "gpu_fantasies=1")
        eng = Recorder()
        ch._eng = eng
        z = [rs.randn(n_pend, 4)]
        ch.ei_over_hypers_gpu(comp, pend, rs.rand(30, 2), vals, rows, randn=z)
        assert (len(eng.drawn), eng.fant_set) == ((1, 0) if device else (0, 1))
        assert eng.calls[-1] == ("ei_run", 30, 1, 4)


def test_shared_normals_go_up_as_one_array(tmp_path):
    """The constrained chooser's refinement shares one (P, S) array between the draws: it is passed as it is."""
    rs = np.random.RandomState(5)
    comp, pend = rs.rand(12, 2), rs.rand(3, 2)
    vals = np.sum(comp ** 2, axis=1)
    rows = np.array([[0.3, 1e-2, 1.0, 0.8, 1.1], [0.2, 2e-2, 0.7, 1.0, 0.5]])
    ch = GPEIChooser.init(str(tmp_path), "")
    eng = Recorder()
    eng.set_observations(np.concatenate((comp, pend)), np.concatenate((vals, np.zeros(3))))
    eng.set_hypers(rows)
    eng.factor()
    z = rs.randn(3, 6)
    ch._set_fantasies(eng, vals, rows, 12, 3, 6, z, per_draw=False)
    assert len(eng.drawn) == 1 and eng.drawn[0][0].shape == (3, 6) and np.array_equal(eng.drawn[0][0], z)
    ch.gpu_fantasies = "0"
    ch._set_fantasies(eng, vals, rows, 12, 3, 6, z, per_draw=False)
    assert len(eng.drawn) == 1 and eng.fant_set == 1 and eng.rows_asked == 2


def test_factored_gamma_equals_the_dense_solve():
    """Gamma_s = L^-1 (F_s - mean) with F_s = [vals; pend_fant_s]: rows < N are gamma[:N], rows N.. are L_S^-1 C z_s.  The
    numpy restatement of what the kernels write (tests/fantasy_helpers.factored_form) against the dense
    solve_triangular on the seven problems of tests/test_host_logic.py's fantasy tests: 1e-12 of max |Gamma| (seen: 2e-14
    and less); its fantasies against fantasize_from_factor_rows and fantasize_pending at those tests' own bars."""
    worst = 0.0
    for name, comp, pend, vals, row, covar, z, atol in fh.host_problems():
        n = comp.shape[0]
        chol, gamma = fh.host_factor(comp, pend, vals, row, covar)
        pf, bests, big = fh.factored_form(vals, row[0], row[1], chol[n:, :], gamma, z)
        f1, b1 = hostgp.fantasize_from_factor_rows(vals, row, chol[n:, :], gamma, z)
        f0, b0 = hostgp.fantasize_pending(comp, pend, vals, row, chol[:n, :n], z, covar)
        scale = np.abs(f0).max()
        for f, b in ((f1, b1), (f0, b0)):
            assert np.allclose(pf, f[n:], rtol=0, atol=atol * scale), name
            assert np.allclose(bests, b, rtol=0, atol=atol * scale), name
        F = np.concatenate((np.tile(vals[:, None], (1, z.shape[1])), pf))
        dense = spla.solve_triangular(chol, F - row[0], lower=True)
        err = float(np.max(np.abs(big - dense)) / np.max(np.abs(dense)))
        worst = max(worst, err)
        assert err <= 1e-12, (name, err)
    print("factored Gamma against the dense solve: worst %.3g of max |Gamma|" % worst)
