"""spx_constrained_ei_grad_batch without a GPU: the symbol is declared, exported and bound; the host restatement of the
objective (constrained.RefineModel, the oracle of the GPU tests) is the gradient of its own value on every branch; and
the chooser with gpu_refine=0 still reproduces the reference's vectors without touching the library."""
import os
import re

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine
from tests import constrained_refine_helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.default_lib_path()):
        import __graft_entry__ as g
        g.build()
    return engine.load_library()


def test_header_declares_and_library_exports_the_symbol(lib):
    src = open(os.path.join(ROOT, "include", "spx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+spx_constrained_ei_grad_batch\s*\(([^)]*)\)", src)
    assert m, "include/spx.h does not declare spx_constrained_ei_grad_batch"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6 and args[0].startswith("spx_handle*") and args[2].startswith("int32_t")
    assert args[3].startswith("double best")
    assert hasattr(lib, "spx_constrained_ei_grad_batch")
    res, argtypes = engine.ABI["spx_constrained_ei_grad_batch"]
    assert len(argtypes) == 6 and lib.spx_constrained_ei_grad_batch.argtypes == argtypes


def test_engine_has_the_method_and_checks_shapes(lib):
    assert callable(getattr(engine.Engine, "constrained_ei_grad_batch", None))
    eng = engine.Engine(0)                    # lazy: no GPU is touched
    try:
        eng.D = 3
        with pytest.raises(ValueError):
            eng.constrained_ei_grad_batch(np.zeros((2, 4)), 0.0)
        # a null handle / null buffers are argument errors with a text, before any device work
        rc = lib.spx_constrained_ei_grad_batch(None, None, 1, 0.0, None, None)
        assert rc == engine.SPX_ERR_ARG and b"spx_constrained_ei_grad_batch" in lib.spx_last_error()
    finally:
        eng.close()


BRANCHES = {"nopend": dict(n_valid=30, n_full=40), "allvalid": dict(n_valid=40, n_full=40),
            "pend": dict(n_valid=30, n_full=40, S=5, n_pend=3), "pend_allvalid": dict(n_valid=40, n_full=40, S=5, n_pend=3)}


@pytest.mark.parametrize("branch", sorted(BRANCHES))
@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE"])
def test_host_restatement_is_the_gradient_of_its_value(branch, covar):
    """Central differences (step 1e-6, the reference's factor one half) on RefineModel.  Every branch passes -- the
    variance from another factor than the mean (no pending jobs) and the sign of the constraint term are consistent
    with the value -- so tests/test_gpu_l_constrained_refine.py::test_central_differences asserts all of them."""
    p = hp.make_problem(11, covar=covar, D=4, H=2, **BRANCHES[branch])
    ms = hp.models(p)
    for x in hp.points(p, 5, 4):
        x = np.clip(x, 1e-3, 1 - 1e-3)
        _, g = hp.oracle(p, x[None], ms)
        fd = hp.central_differences(lambda y: hp.oracle(p, y[None], ms)[0][0], x, range(3))
        assert np.allclose(fd, g[0][:3], rtol=2e-3, atol=1e-9), (branch, covar, fd, g[0][:3])


@pytest.mark.parametrize("tag", ["nopend", "pend", "allvalid"])
def test_host_refine_path_reproduces_reference_without_the_library(golden_dir, tmp_path, tag, monkeypatch):
    """gpu_refine=0, gpu_logprob=0: _refine's objective is RefineModel, pinned to the reference's output, and no engine
    is created."""
    from spearmint_amd import refine
    from spearmint_amd.chooser import GPConstrainedEIChooser as mod
    g = np.load(os.path.join(golden_dir, "constrained_refine.npz"))
    c = mod.GPConstrainedEIChooser(str(tmp_path), gpu_refine=0, gpu_logprob=0, mcmc_iters=g[tag + "_rows"].shape[0],
                                   pending_samples=int(g["pending_samples"]))

    def no_engine():
        raise AssertionError("the host refinement path must not load the library")
    monkeypatch.setattr(c, "engine", no_engine)
    npr.seed(int(g["rng_seed"]))
    c.randomstate = npr.get_state()
    c.D = g[tag + "_comp"].shape[1]
    c.hyper_samples = [(r[0], r[1], r[2], r[3:]) for r in g[tag + "_rows"]]
    c.constraint_hyper_samples = [(r[0], r[1], r[2], r[3:]) for r in g[tag + "_crows"]]
    from spearmint_amd import constrained as con
    c.cst = con.ConstraintState(c.D)
    c.cst.ff = g[tag + "_ff"]
    seen = {}

    def capture(batch, points, bounds, log=None, serial=None):
        seen["f"], seen["g"] = batch(np.asarray(points))
        seen["serial"] = serial
        return np.asarray(points)
    monkeypatch.setattr(refine, "lbfgs_many", capture)
    c._refine(g[tag + "_pts"], g[tag + "_comp"], g[tag + "_pend"], g[tag + "_vals"], g[tag + "_labels"])
    np.testing.assert_allclose(seen["f"], g[tag + "_f"], rtol=1e-12)
    np.testing.assert_allclose(seen["g"], g[tag + "_g"], rtol=1e-10, atol=1e-14)
    assert seen["serial"] is True


def test_gpu_refine_is_the_default_and_zero_keeps_the_host_path(tmp_path):
    from spearmint_amd.chooser import GPConstrainedEIChooser as mod
    c = mod.GPConstrainedEIChooser(str(tmp_path))
    assert c.gpu_refine == "auto" and c._use_gpu_refine(10)
    assert hasattr(c, "_refine_gpu")
    assert not mod.GPConstrainedEIChooser(str(tmp_path), gpu_refine=0)._use_gpu_refine(10)
