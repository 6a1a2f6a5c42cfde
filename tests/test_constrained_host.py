"""GPConstrainedEIChooser, host side: the oracle, the constraint / objective samplers and the refinement objective
against vectors the reference itself produced (tests/golden/constrained_*.npz, scripts/make_golden_constrained.py),
argument parsing and the state pickle.  No GPU."""
import os
import pickle

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import constrained as con
from spearmint_amd.chooser import GPConstrainedEIChooser as mod
from tests import constrained_oracle as co

STAGES = ["nopend", "pend", "allvalid", "matern32", "ardse", "se"]


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, "constrained_%s.npz" % name))


@pytest.mark.parametrize("case", STAGES)
def test_oracle_matches_reference_stage_arrays(golden_dir, case):
    g = _g(golden_dir, "stage_" + case)
    npr.seed(int(g["rng_seed"]))
    randn = npr.randn(g["pend"].shape[0], int(g["pending_samples"])) if g["pend"].shape[0] else None
    covar = str(g["covar"])
    ei = co.compute_constrained_ei(covar, g["comp"], g["vals"], g["labels"], g["pend"], g["cand"], g["ff"],
                                   g["hyper"], g["chyper"], randn)
    np.testing.assert_allclose(ei, g["ei"], rtol=1e-12, atol=0)
    if "prob" in g:
        p = co.constraint_prob(covar, g["comp"], g["ff"], g["chyper"], g["cand"], False)
        np.testing.assert_allclose(p, g["prob"], rtol=1e-12, atol=0)


def test_samplers_reproduce_reference_trace(golden_dir, tmp_path):
    """sample_constraint_hypers + sample_hypers, six iterations from a seed: every sample and the RNG state after every
    iteration equal the reference's."""
    g = _g(golden_dir, "trace")
    comp, y, labels = g["comp"], g["vals"], g["labels"]
    good = labels > 0
    c = mod.GPConstrainedEIChooser(str(tmp_path), gpu_logprob=0)
    npr.seed(int(g["seed"]))
    c._real_init(2, y)
    for it in range(g["rows"].shape[0]):
        c.sample_constraint_hypers(comp, labels)
        c.sample_hypers(comp[good], y[good])
        np.testing.assert_array_equal(np.concatenate(([c.mean, c.noise, c.amp2], c.ls)), g["rows"][it])
        np.testing.assert_array_equal(np.concatenate(([c.cst.gain, c.cst.amp2], c.cst.ls)), g["crows"][it])
        np.testing.assert_array_equal(c.cst.ff, g["ff"][it])
        st = npr.get_state()
        np.testing.assert_array_equal(st[1], g["rng_key"][it])
        assert st[2] == g["rng_pos"][it][0] and st[3] == g["rng_pos"][it][1]


@pytest.mark.parametrize("tag", ["nopend", "pend", "allvalid"])
def test_refinement_objective_matches_reference(golden_dir, tag):
    g = _g(golden_dir, "refine")
    npr.seed(int(g["rng_seed"]))
    rs = npr.get_state()
    models = [con.RefineModel(g[tag + "_comp"], g[tag + "_pend"], g[tag + "_vals"], g[tag + "_labels"],
                              (r[0], r[1], r[2], r[3:]), (c[0], c[1], c[2], c[3:]), g[tag + "_ff"], "Matern52",
                              int(g["pending_samples"]), rs) for r, c in zip(g[tag + "_rows"], g[tag + "_crows"])]
    before = npr.get_state()[1].copy()
    for k, x in enumerate(g[tag + "_pts"]):
        f, grad = 0.0, 0.0
        for m in models:
            e, gr = m.neg_ei_and_grad(x)
            f += e
            grad = grad + gr
        np.testing.assert_allclose(f, g[tag + "_f"][k], rtol=1e-12)
        np.testing.assert_allclose(grad, g[tag + "_g"][k], rtol=1e-10, atol=1e-14)
    np.testing.assert_array_equal(npr.get_state()[1], before)     # the caller's stream is untouched


def test_arguments_and_defaults(tmp_path):
    c = mod.init(str(tmp_path), "covar=Matern32,mcmc_iters=7,pending_samples=12,constraint_violating_value=99.5,"
                                "noiseless=1,burnin=3,grid_subset=5,visualize2D=1,verbosity=1")
    assert (c.covar, c.mcmc_iters, c.pending_samples, c.bad_value) == ("Matern32", 7, 12, 99.5)
    assert c.noiseless and c.burnin == 3 and c.grid_subset == 5 and c.verbosity == 1
    d = mod.init(str(tmp_path), "")
    assert (d.mcmc_iters, d.burnin, d.grid_subset, d.pending_samples) == (20, 100, 20, 100)
    assert d.bad_value == np.inf and not d.noiseless
    assert d.state_pkl.endswith("GPConstrainedEIChooser.pkl")


def test_too_few_jobs_return_first_candidate(tmp_path):
    c = mod.GPConstrainedEIChooser(str(tmp_path))
    grid = np.random.RandomState(0).rand(10, 2)
    vals = np.array([1.0, np.nan, np.inf, 0.5] + [0.0] * 6)
    cands = np.arange(4, 10)
    assert c.next(grid, vals, np.ones(10), cands, np.array([], dtype=int), np.array([0])) == 4
    # three completed, one valid
    assert c.next(grid, vals, np.ones(10), cands, np.array([], dtype=int), np.array([0, 1, 2])) == 4
    assert c.D == -1                      # nothing initialised yet, as in the reference


def test_pickle_round_trip_with_and_without_gain(tmp_path):
    c = mod.GPConstrainedEIChooser(str(tmp_path))
    c._real_init(3, np.array([1.0, 2.0, np.nan, 0.5]))
    assert not os.path.exists(c.state_pkl)
    c.cst.gain, c.cst.amp2, c.cst.ls = 2.5, 0.7, np.array([0.1, 0.2, 0.3])
    c.hyper_samples = [(c.mean, c.noise, c.amp2, c.ls)]
    c.dump_hypers()
    state = pickle.load(open(c.state_pkl, "rb"))
    # the reference's keys, plus constraint_gain
    assert set(state) == {"dims", "ls", "amp2", "noise", "mean", "constraint_ls", "constraint_amp2",
                          "constraint_noise", "constraint_mean", "constraint_gain"}
    assert os.path.exists(c.stats_file)
    r = mod.GPConstrainedEIChooser(str(tmp_path))
    r._real_init(3, np.array([1.0]))
    assert r.cst.gain == 2.5 and r.cst.amp2 == 0.7 and not r.needs_burnin and r.cst.ff is None
    np.testing.assert_array_equal(r.cst.ls, [0.1, 0.2, 0.3])
    # a pickle as the reference writes it: no constraint_gain -> gain 1
    del state["constraint_gain"]
    pickle.dump(state, open(c.state_pkl, "wb"), protocol=2)
    q = mod.GPConstrainedEIChooser(str(tmp_path))
    q._real_init(3, np.array([1.0]))
    assert q.cst.gain == 1 and q.cst.amp2 == 0.7


def test_mcmc_iters_zero_raises(tmp_path):
    c = mod.GPConstrainedEIChooser(str(tmp_path), mcmc_iters=0)
    grid = np.random.RandomState(1).rand(8, 2)
    vals = np.array([1.0, 0.5, 0.7, np.nan] + [0.0] * 4)
    with pytest.raises(Exception, match="mcmc_iters <= 0"):
        c.next(grid, vals, np.ones(8), np.arange(4, 8), np.array([], dtype=int), np.arange(4))


def test_dropin_shim_names_the_reference_module():
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "dropin"))
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "chooser" or k.startswith("chooser.")}
    try:
        m = importlib.import_module("chooser.GPConstrainedEIChooser")
    finally:
        # the reference's own `chooser` package is imported by other tests: leave sys.modules as it was
        sys.path.remove(os.path.join(root, "dropin"))
        for k in [k for k in sys.modules if k == "chooser" or k.startswith("chooser.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert m.GPConstrainedEIChooser.__module__ == "chooser.GPConstrainedEIChooser"
    assert issubclass(m.GPConstrainedEIChooser, mod.GPConstrainedEIChooser)
