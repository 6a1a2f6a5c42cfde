"""Two objectives, both minimised: pure host helpers of the Pareto chooser (chooser/GPParetoChooser.py) -- the front of a
set of points in the order the engine takes it (include/spx.h: spx_set_pareto_front), the automatic reference point, and
the hypervolume a front dominates.  numpy only; nothing here touches a device."""
from __future__ import absolute_import

import numpy as np


def pareto_front(v1, v2):
    """Indices (into v1 / v2) of the non-dominated points, ordered as the engine wants them: v1 strictly increasing and v2
    strictly decreasing along the result.  A point is dominated when another one is no worse in both objectives and better
    in one; of exact duplicates the first survives.  Points with a non-finite coordinate are never members."""
    v1 = np.asarray(v1, dtype=np.float64).ravel()
    v2 = np.asarray(v2, dtype=np.float64).ravel()
    if v1.shape != v2.shape:
        raise ValueError("pareto_front: v1 and v2 must have the same length")
    ok = np.nonzero(np.isfinite(v1) & np.isfinite(v2))[0]
    order = ok[np.lexsort((ok, v2[ok], v1[ok]))]          # by v1, then v2, then index
    keep = []
    lowest = np.inf
    for i in order:
        if v2[i] < lowest:                                 # strictly better in the second objective than everything left of it
            keep.append(int(i))
            lowest = v2[i]
    return np.array(keep, dtype=np.int64)


def reference_point(v1, v2):
    """r_k = max_k + 0.1 (max_k - min_k), or max_k + 1 where the range is zero: every point lies strictly inside."""
    out = []
    for v in (v1, v2):
        v = np.asarray(v, dtype=np.float64).ravel()
        if v.size == 0 or not np.all(np.isfinite(v)):
            raise ValueError("reference_point: needs at least one point, all finite")
        hi, lo = float(np.max(v)), float(np.min(v))
        out.append(hi + 0.1 * (hi - lo) if hi > lo else hi + 1.0)
    return out[0], out[1]


def dominated_hypervolume(front, ref):
    """The area between a front ((n, 2), ordered as pareto_front orders it) and the reference point: the sum over the front's
    points of (a_{i+1} - a_i) (r2 - b_i) with a_{n+1} = r1.  An empty front dominates nothing."""
    front = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    r1, r2 = float(ref[0]), float(ref[1])
    n = front.shape[0]
    if n == 0:
        return 0.0
    a, b = front[:, 0], front[:, 1]
    if np.any(np.diff(a) <= 0) or np.any(np.diff(b) >= 0) or not (a[-1] < r1 and b[0] < r2):
        raise ValueError("dominated_hypervolume: the front must be strictly ordered and lie inside the reference point")
    edges = np.concatenate((a[1:], [r1]))
    return float(np.sum((edges - a) * (r2 - b)))
