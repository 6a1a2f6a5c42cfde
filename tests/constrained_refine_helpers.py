"""Shared by the tests of spx_constrained_ei_grad_batch: seeded problems, the handle set up as the chooser leaves it
after its first grid pass, and the host oracle (constrained.RefineModel summed over the draws in draw order)."""
import numpy as np
import numpy.random as npr

from spearmint_amd import constrained as con
from spearmint_amd import hostgp

VALUE_RTOL = 1e-7          # tests/test_gpu_d_multi.py::test_ei_grad_batch_matches_reference_golden
GRAD_RTOL = 1e-6
GRAD_ATOL_REL = 1e-9       # times max |g| of the reference


class Problem(object):
    pass


def make_problem(seed, covar="Matern52", D=3, n_valid=30, n_full=40, H=2, S=0, n_pend=0):
    """n_full completed points of which n_valid are valid (n_valid == n_full: no violation seen), H draws, S fantasies
    over n_pend pending points (S = 0: none)."""
    rs = np.random.RandomState(seed)
    p = Problem()
    p.covar, p.D, p.H, p.S = covar, D, H, S
    p.comp = rs.rand(n_full, D)
    p.vals = np.sum((p.comp - 0.4) ** 2, axis=1) + 0.02 * rs.randn(n_full)
    p.labels = np.ones(n_full)
    if n_valid < n_full:
        p.labels[rs.choice(n_full, n_full - n_valid, replace=False)] = 0
    p.rows = np.column_stack((rs.uniform(0.1, 0.3, H), rs.uniform(1e-3, 1e-2, H), rs.uniform(0.5, 1.5, H),
                              rs.uniform(0.3, 1.5, (H, D))))
    # reference layout of a constraint sample: (mean, gain, amp2_c, ls_c)
    p.chyp = np.column_stack((np.full(H, 0.5), rs.uniform(0.5, 3.0, H), rs.uniform(0.5, 2.0, H),
                              rs.uniform(0.3, 1.5, (H, D))))
    p.ff = rs.randn(n_full) * 1.5
    p.pend = rs.rand(n_pend, D) if S > 0 else np.zeros((0, D))
    p.randomstate = np.random.RandomState(seed + 7919).get_state()
    good = p.labels > 0
    p.compv, p.valsv = p.comp[good], p.vals[good]
    p.best = np.min(p.valsv)
    return p


def points(p, seed, n=21):
    """Half near the best valid observation (comp[best] + 1e-3 randn), half uniform, interleaved."""
    rs = np.random.RandomState(seed)
    near = p.compv[np.argmin(p.valsv)] + 1e-3 * rs.randn(n, p.D)
    uni = rs.rand(n, p.D)
    pts = np.where((np.arange(n) % 2 == 0)[:, None], uni, near)
    return np.clip(pts, 0.0, 1.0)


def crows(p):
    """Engine layout of the constraint hypers: [gain, noise_c, amp2_c, ls_c...] (noise_c is fixed at 1e-3)."""
    return np.column_stack((p.chyp[:, 1], np.full(p.H, 1e-3), p.chyp[:, 2], p.chyp[:, 3:]))


def refine_fantasies(eng, p):
    """What RefineModel draws: the same normals for every draw, from a private generator restarted at p.randomstate."""
    rs = npr.RandomState()
    rs.set_state(p.randomstate)
    randn = rs.randn(p.pend.shape[0], p.S)
    n = p.valsv.shape[0]
    fant = np.empty((p.H, n + p.pend.shape[0], p.S))
    bests = np.empty((p.H, p.S))
    for h in range(p.H):
        l_rows, gam = eng.get_factor_rows(h, n, p.pend.shape[0])
        fant[h], bests[h] = hostgp.fantasize_from_factor_rows(p.valsv, p.rows[h], l_rows, gam, randn)
    return fant, bests


def setup(eng, p, cand=None):
    """The handle as GPConstrainedEIChooser.ei_over_hypers leaves it, with the refinement's fantasies set."""
    from spearmint_amd.engine import FLAG_CONSTRAINED
    eng.set_covar(p.covar)
    if p.S > 0:
        eng.set_observations(np.concatenate((p.compv, p.pend)), np.concatenate((p.valsv, np.zeros(p.pend.shape[0]))))
    else:
        eng.set_observations(p.compv, p.valsv)
    eng.set_candidates(np.random.RandomState(1).rand(64, p.D) if cand is None else cand)
    eng.set_hypers(p.rows)
    if np.all(p.labels > 0):
        eng.set_constraint_model(np.zeros((0, p.D)), np.zeros(0), crows(p))
    else:
        eng.set_constraint_model(p.comp, p.ff, crows(p))
    if p.S > 0:
        eng.factor()
        fant, bests = refine_fantasies(eng, p)
        eng.set_fantasies(fant, bests)
    else:
        eng.ei_step(FLAG_CONSTRAINED)


def _embedded_in_two_dims(p):
    """The same problem with a second input dimension that is 0 everywhere: every distance, hence every covariance, and
    the derivative along the first dimension are unchanged."""
    q = Problem()
    q.__dict__.update(p.__dict__)
    pad = lambda a: np.column_stack((a, np.zeros(a.shape[0])))
    q.comp, q.pend, q.D = pad(p.comp), pad(p.pend), 2
    q.rows = np.column_stack((p.rows, np.ones(p.H)))
    q.chyp = np.column_stack((p.chyp, np.ones(p.H)))
    return q


def models(p):
    if p.D == 1 and p.S > 1:
        # RefineModel keeps the reference's np.squeeze of the correlation's gradient, which at D = 1 drops the dimension
        # axis too: with more than one fantasy its pending branch then broadcasts (S,) against (S, 1) and returns S
        # numbers (the reference does the same: it has no refinement at D = 1 with pending jobs).  The oracle for that
        # corner is the same arithmetic on the problem embedded in two dimensions; oracle() drops the padding again.
        p = _embedded_in_two_dims(p)
    return [con.RefineModel(p.comp, p.pend, p.vals, p.labels, (r[0], r[1], r[2], r[3:]), (c[0], c[1], c[2], c[3:]),
                            p.ff, p.covar, p.S, p.randomstate) for r, c in zip(p.rows, p.chyp)]


def oracle(p, pts, ms=None):
    ms = models(p) if ms is None else ms
    D = pts.shape[1]
    if ms[0].comp.shape[1] != D:          # (the embedded D = 1 problem, see models())
        pts = np.column_stack((pts, np.zeros(pts.shape[0])))
    f = np.zeros(pts.shape[0])
    g = np.zeros(pts.shape)
    for k in range(pts.shape[0]):
        for m in ms:
            e, gk = m.neg_ei_and_grad(pts[k])
            f[k] += e
            g[k] = g[k] + gk
    return f, g[:, :D]


def assert_close(f, g, f_ref, g_ref):
    for k in range(f_ref.shape[0]):
        assert np.isclose(f[k], f_ref[k], rtol=VALUE_RTOL, atol=1e-300), (k, f[k], f_ref[k])
        assert np.allclose(g[k], g_ref[k], rtol=GRAD_RTOL, atol=GRAD_ATOL_REL * max(np.abs(g_ref[k]).max(), 1e-300)), \
            (k, g[k], g_ref[k])


def central_differences(value_fn, x, dims, step=1e-6):
    """0.5 (f(x + e) - f(x - e)) / (2 step) per dimension: the reference's gradient carries the factor one half."""
    out = []
    for d in dims:
        e = np.zeros(x.shape[0])
        e[d] = step
        out.append(0.5 * (value_fn(x + e) - value_fn(x - e)) / (2 * step))
    return np.array(out)
