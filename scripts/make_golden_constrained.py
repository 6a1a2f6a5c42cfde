"""Record tests/golden/constrained_*.npz from the reference's own GPConstrainedEIChooser (build container only).

Reuses oracle.ref_py3: load() converts the reference's gp.py / util.py / Locker.py for Python 3 into a scratch tree;
this script adds GPConstrainedEIChooser.py to that tree with the same lib2to3 run and the same _patch edits, plus one
more: its module-level `import matplotlib.pyplot as plt` is dropped (only visualize2D=1 plots).  multiprocessing.Pool
is replaced by a serial stand-in that saves and restores numpy's global RNG state around every optimize_pt, which is
what a forked worker amounts to for the parent's stream.

Writes numeric arrays only (no object arrays):
  constrained_stage_<case>.npz   compute_constrained_ei for fixed hypers and ff (cases: nopend / pend / allvalid /
                                 one per covar=), with P from pred_constraint_voilation where defined
  constrained_trace.npz          seeded sample_constraint_hypers + sample_hypers, RNG state and samples per iteration
  constrained_next_<case>.npz    seeded next() sequences on one chooser object
  constrained_refine.npz         grad_optimize_ei_over_hypers values and gradients at fixed points

Run:  python scripts/make_golden_constrained.py"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import numpy.random as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_py3  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def load_constrained():
    mods = ref_py3.load()
    scratch = mods["_scratch"]
    dst = os.path.join(scratch, "chooser", "GPConstrainedEIChooser.py")
    shutil.copy(os.path.join(ref_py3._S, "chooser", "GPConstrainedEIChooser.py"), dst)
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", dst],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ref_py3._patch(dst)
    src = open(dst).read().replace("import matplotlib.pyplot as plt", "plt = None  # matplotlib: visualize2D only")
    open(dst, "w").write(src)
    sys.path.insert(0, scratch)
    sys.path.insert(0, os.path.join(scratch, "chooser"))
    import importlib
    m = importlib.import_module("chooser.GPConstrainedEIChooser")

    class _Res(object):
        def __init__(self, v):
            self.v = v

        def get(self, timeout=None):
            return self.v

    class _Pool(object):
        def __init__(self, n):
            pass

        def apply_async(self, f, args=()):
            st = npr.get_state()
            try:
                return _Res(f(*args))
            finally:
                npr.set_state(st)

        def close(self):
            pass

    class _MP(object):
        Pool = _Pool

    m.multiprocessing = _MP()
    return m, mods


def rng_arrays(prefix):
    st = npr.get_state()
    return {prefix + "_key": np.asarray(st[1], dtype=np.uint32), prefix + "_pos": np.int64(st[2]),
            prefix + "_has_gauss": np.int64(st[3]), prefix + "_cached": np.float64(st[4])}


def problem(seed, n, D=2, n_bad=3, bad="nan"):
    rs = np.random.RandomState(seed)
    X = rs.rand(n, D)
    y = np.sum((X - 0.4) ** 2, axis=1) + 0.05 * rs.randn(n)
    badidx = rs.choice(n, n_bad, replace=False) if n_bad else np.zeros(0, dtype=int)
    for k, i in enumerate(badidx):
        y[i] = {"nan": np.nan, "inf": np.inf if k % 2 == 0 else -np.inf, "user": 99.0}[bad if bad != "mix" else
                                                                                     ("nan", "inf", "user")[k % 3]]
    return X, y


def stage_cases(m):
    tmp = tempfile.mkdtemp(prefix="spx_gold_c_")
    for case, covar, npend, nbad in (("nopend", "Matern52", 0, 4), ("pend", "Matern52", 3, 4), ("allvalid", "Matern52", 0, 0),
                                     ("matern32", "Matern32", 0, 4), ("ardse", "ARDSE", 0, 4), ("se", "SE", 0, 4)):
        rs = np.random.RandomState(7)
        D = 3
        comp = rs.rand(23, D)
        vals = np.sum((comp - 0.3) ** 2, axis=1) + 0.01 * rs.randn(23)
        labels = np.ones(23)
        if nbad:
            bad = rs.choice(23, nbad, replace=False)
            vals[bad] = np.nan
            labels[bad] = 0
        cand = rs.rand(150, D)
        pend = rs.rand(npend, D)
        c = m.GPConstrainedEIChooser(tmp, covar=covar, pending_samples=7)
        c.mean, c.noise, c.amp2, c.ls = 0.2, 0.003, 0.8, np.array([0.4, 0.7, 1.1])
        c.constraint_mean, c.constraint_gain, c.constraint_amp2 = 0.5, 1.7, 1.3
        c.constraint_ls = np.array([0.6, 0.9, 0.5])
        c.constraint_noise = 1e-3
        c.ff = rs.randn(23)
        npr.seed(11)
        ei = c.compute_constrained_ei(comp, pend, cand, vals, labels)
        rec = dict(comp=comp, vals=vals, labels=labels, cand=cand, pend=pend, ff=c.ff,
                   hyper=np.concatenate(([c.mean, c.noise, c.amp2], c.ls)),
                   chyper=np.concatenate(([c.constraint_gain, c.constraint_noise, c.constraint_amp2], c.constraint_ls)),
                   covar=np.array(covar), pending_samples=np.int64(7), rng_seed=np.int64(11), ei=np.asarray(ei, dtype=float))
        if nbad and covar != "SE":     # (pred_constraint_voilation asks gp for grad_SE, which does not exist)
            rec["prob"] = c.pred_constraint_voilation(cand, comp, labels).flatten()
        np.savez_compressed(os.path.join(OUT, "constrained_stage_%s.npz" % case), **rec)
    shutil.rmtree(tmp, ignore_errors=True)


def trace_case(m):
    tmp = tempfile.mkdtemp(prefix="spx_gold_c_")
    comp, y = problem(3, 18, D=2, n_bad=4, bad="nan")
    labels = np.isfinite(y).astype(float)
    good = labels > 0
    c = m.GPConstrainedEIChooser(tmp)
    npr.seed(5)
    c._real_init(2, y, np.ones(18))
    rec = dict(comp=comp, vals=y, labels=labels, seed=np.int64(5))
    rows, crows, ffs, keys, poss = [], [], [], [], []
    for it in range(6):
        c.sample_constraint_hypers(comp, labels)
        c.sample_hypers(comp[good], y[good])
        rows.append(np.concatenate(([c.mean, c.noise, c.amp2], c.ls)))
        crows.append(np.concatenate(([c.constraint_gain, c.constraint_amp2], c.constraint_ls)))
        ffs.append(c.ff.copy())
        st = npr.get_state()
        keys.append(np.asarray(st[1], dtype=np.uint32))
        poss.append(np.array([st[2], st[3]], dtype=np.int64))
    rec.update(rows=np.array(rows), crows=np.array(crows), ff=np.array(ffs), rng_key=np.array(keys), rng_pos=np.array(poss))
    np.savez_compressed(os.path.join(OUT, "constrained_trace.npz"), **rec)
    shutil.rmtree(tmp, ignore_errors=True)


def refine_case(m):
    tmp = tempfile.mkdtemp(prefix="spx_gold_c_")
    rec = {}
    for tag, npend, nbad in (("nopend", 0, 4), ("pend", 2, 4), ("allvalid", 0, 0)):
        rs = np.random.RandomState(9)
        D = 2
        comp = rs.rand(20, D)
        vals = np.sum((comp - 0.3) ** 2, axis=1) + 0.01 * rs.randn(20)
        labels = np.ones(20)
        if nbad:
            bad = rs.choice(20, nbad, replace=False)
            vals[bad] = np.nan
            labels[bad] = 0
        pend = rs.rand(npend, D)
        c = m.GPConstrainedEIChooser(tmp, mcmc_iters=2, pending_samples=6)
        hs = [(0.2, 0.002, 0.7, np.array([0.5, 0.8])), (0.25, 0.004, 0.9, np.array([0.7, 0.4]))]
        cs = [(0.5, 1.4, 1.1, np.array([0.6, 0.9])), (0.5, 0.8, 1.6, np.array([0.3, 0.5]))]
        c.hyper_samples, c.constraint_hyper_samples = hs, cs
        c.ff = rs.randn(20)
        c.constraint_noise = 1e-3
        npr.seed(17)
        c.randomstate = npr.get_state()
        pts = rs.rand(5, D)
        f, g = [], []
        for x in pts:
            e, gr = c.grad_optimize_ei_over_hypers(x, comp, pend, vals, labels)
            f.append(e)
            g.append(np.asarray(gr, dtype=float).ravel())
        rec.update({tag + "_comp": comp, tag + "_vals": vals, tag + "_labels": labels, tag + "_pend": pend,
                    tag + "_ff": c.ff, tag + "_rows": np.array([np.concatenate(([h[0], h[1], h[2]], h[3])) for h in hs]),
                    tag + "_crows": np.array([np.concatenate(([h[0], h[1], h[2]], h[3])) for h in cs]),
                    tag + "_pts": pts, tag + "_f": np.array(f, dtype=float), tag + "_g": np.array(g)})
    rec["rng_seed"] = np.int64(17)
    rec["pending_samples"] = np.int64(6)
    np.savez_compressed(os.path.join(OUT, "constrained_refine.npz"), **rec)
    shutil.rmtree(tmp, ignore_errors=True)


def next_case(m, name, args, seed, bad, sizes, pend_last, n_bad=3):
    """One chooser object, len(sizes) next() calls; sizes[i] completed jobs; the last call gets `pend_last` pending."""
    tmp = tempfile.mkdtemp(prefix="spx_gold_c_")
    D = 2
    Xall, yall = problem(seed, max(sizes) + 4, D=D, n_bad=n_bad, bad=bad)
    gs = np.random.RandomState(seed + 100).rand(60, D)
    grid = np.vstack((Xall, gs))
    values = np.concatenate((yall, np.zeros(60)))
    c = m.init(tmp, args)
    c.pending_samples = int(c.pending_samples)   # the reference keeps the arg string's str and randn raises: our int()
    last = {}
    orig = c.ei_over_hypers

    def spy(*a):
        r = orig(*a)
        last["oe"] = np.array(r, dtype=float)
        return r
    c.ei_over_hypers = spy
    npr.seed(seed)
    rec = {"args": np.array(args), "grid": grid, "values": values, "ncalls": np.int64(len(sizes))}
    for k, n in enumerate(sizes):
        complete = np.arange(n)
        npend = pend_last if k == len(sizes) - 1 else 0
        pending = np.arange(n, n + npend)
        candidates = np.arange(Xall.shape[0], grid.shape[0])
        rec.update(rng_arrays("before%d" % k))
        ret = c.next(grid, values, np.ones(grid.shape[0]), candidates, pending, complete)
        rec.update(rng_arrays("after%d" % k))
        rec["complete%d" % k] = complete
        rec["pending%d" % k] = pending
        rec["candidates%d" % k] = candidates
        if isinstance(ret, tuple):
            rec["ret_idx%d" % k] = np.int64(ret[0])
            rec["ret_pt%d" % k] = np.asarray(ret[1], dtype=float)
        else:
            rec["ret_idx%d" % k] = np.int64(ret)
        rec["overall_ei%d" % k] = last["oe"]
    np.savez_compressed(os.path.join(OUT, "constrained_next_%s.npz" % name), **rec)
    shutil.rmtree(tmp, ignore_errors=True)


def main():
    m, _ = load_constrained()
    stage_cases(m)
    trace_case(m)
    refine_case(m)
    common = "mcmc_iters=3,burnin=8,grid_subset=4,pending_samples=5"
    next_case(m, "nan", common, 21, "nan", (14, 16, 16), 1)
    next_case(m, "mixed_noiseless", common + ",noiseless=1,constraint_violating_value=99.0", 22, "mix", (15, 17), 0, n_bad=4)
    next_case(m, "allvalid", common, 23, "nan", (12,), 0, n_bad=0)


if __name__ == "__main__":
    main()
