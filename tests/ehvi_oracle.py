"""Float64 oracle (numpy / scipy) of the expected hypervolume improvement (include/spx.h: SPX_ACQ_EHVI), operation for
operation as spearmint_amd/csrc/ehvi_device.h has it: G = the EI formula of ei_device.h with best = y, the strips summed
sequentially in i = 0 .. n, G1 of an edge evaluated once and carried over as the next strip's lower edge, the first strip
assigned (not added to a zero), no strip skipped.

    EHVI = sum_{i=0..n} [G1(a_{i+1}) - G1(a_i)] G2(b_i),   a_0 = -inf (G1 := +0.0), a_{n+1} = r1, b_0 = r2

The natural scale of its error is unit = sum_i [G1(a_{i+1}) + G1(a_i)] G2(b_i): the differences cancel when front points are
close.  Test code only: nothing in spearmint_amd imports this module."""
import numpy as np
from scipy.special import ndtr

from oracle import gp_ei_oracle as orc
from tests import acq_oracle as ao

EHVI = 4                                  # include/spx.h SPX_ACQ_EHVI
SQRT_2PI = 2.50662827463100050242         # ei_device.h's literal


def g(func_m, func_v, y):
    """ei_dev(func_m, func_v, best = y): NaN for func_v < 0 (np.sqrt), as on the device."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        func_s = np.sqrt(func_v)
        u = (y - func_m) / func_s
        ncdf = ndtr(u)
        npdf = np.exp(-(u * u) / 2.0) / SQRT_2PI
        return func_s * (u * ncdf + npdf)


def strips(a, b, r1, r2):
    """(edges, levels) of the n + 1 strips, as spx_set_pareto_front hands them to the kernel."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return np.concatenate((a, [r1])), np.concatenate(([r2], b))


def ehvi(m1, v1, m2, v2, a, b, r1, r2, want_unit=False):
    """EHVI of every candidate (arrays m1, v1, m2, v2 of one shape) against the front (a, b) and reference point (r1, r2)."""
    m1, v1, m2, v2 = (np.asarray(x, dtype=np.float64) for x in (m1, v1, m2, v2))
    edges, levels = strips(a, b, r1, r2)
    g_lo = np.zeros(m1.shape)
    acc = unit = None
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(edges.shape[0]):
            g_hi = g(m1, v1, edges[i])
            g2 = g(m2, v2, levels[i])
            term = (g_hi - g_lo) * g2
            acc = term if i == 0 else acc + term
            if want_unit:
                t = (np.abs(g_hi) + np.abs(g_lo)) * np.abs(g2)
                unit = t if i == 0 else unit + t
            g_lo = g_hi
    return (acc, unit) if want_unit else acc


def over_hypers(comp, cand, vals, second, rows, trows, a, b, r1, r2, want_moments=False):
    """[M, H] as orc.ei_over_hypers lays EI out, and the moments [(m1, v1, m2, v2)] per draw: the objective's GP over
    (comp, vals, rows[d]), the second objective's over (comp, second, trows[d])."""
    rows, trows = np.atleast_2d(rows), np.atleast_2d(trows)
    out = np.zeros((cand.shape[0], rows.shape[0]))
    mom = []
    for d in range(rows.shape[0]):
        m1, v1 = ao.moments(comp, cand, vals, rows[d])
        m2, v2 = ao.moments(comp, cand, second, trows[d])
        mom.append((m1, v1, m2, v2))
        out[:, d] = ehvi(m1, v1, m2, v2, a, b, r1, r2)
    return (out, mom) if want_moments else out


def improvement(u, v, a, b, r1, r2):
    """I(u, v): the area a new point (u, v) adds to what the front dominates (arrays u, v broadcast)."""
    edges, levels = strips(a, b, r1, r2)
    lower = np.concatenate(([-np.inf], edges[:-1]))
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    out = np.zeros(np.broadcast(u, v).shape)
    for i in range(edges.shape[0]):
        out = out + np.maximum(edges[i] - np.maximum(u, lower[i]), 0.0) * np.maximum(levels[i] - v, 0.0)
    return out


covar = orc.covar
