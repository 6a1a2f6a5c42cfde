"""50-digit restatement (mpmath) of the probability of improvement and of the lower confidence bound where float64 has the
least to spare: PI = Phi(u) from u about 0 down to where it passes 1e-300 (the error of func_m is amplified by about u^2
in the lower tail of Phi), and LCB = kappa func_s - func_m at kappa chosen so that kappa func_s is within 1e-6 relative
of func_m (the difference cancels six digits).  The GP is tests/refine_mp._Draw: plain sums of squared differences, an
mpf Cholesky, every input converted from the float64 arrays exactly.

Test code only: nothing in spearmint_amd imports this module, and the GPU tests read its results from
tests/golden/acq_tail_mp.npz (scripts/make_golden_acq_tail.py) instead of importing mpmath."""
import numpy as np

from tests import refine_mp as rm

DPS = rm.DPS
TAIL_SEED, TAIL_N, TAIL_M, TAIL_D = 23, 24, 320, 2
TAIL_BANDS = [(-3.0, 0.0), (-20.0, -3.0), (-100.0, -20.0), (-300.0, -100.0)]    # log10 PI; the first closed, the others [lo, hi)
XIS = (0.0, 0.01)
LCB_CASES = 6              # candidates whose func_m / func_s gives a kappa at which LCB cancels
LCB_REL = 1e-6             # kappa func_s = func_m (1 + LCB_REL / 2), up to the rounding of kappa


def tail_problem():
    """The observations sit in one corner of the unit square with values about 0 (the lowest -1.5) under draws whose prior
    mean is 40 and 38 (amp2 about 1, so func_s <= 1): along rays away from the corner func_m climbs from the data to the
    prior mean and u = (best - xi - func_m) / func_s runs from about 0 to below -40."""
    rs = np.random.RandomState(TAIL_SEED)
    n, D, M = TAIL_N, TAIL_D, TAIL_M
    comp = 0.25 * rs.rand(n, D)
    vals = 0.3 * rs.randn(n)
    vals[0] = -1.5
    ang = rs.uniform(0, 0.5 * np.pi, M)
    rad = rs.uniform(0.0, 0.95, M)
    cand = np.clip(0.12 + rad[:, None] * np.column_stack((np.cos(ang), np.sin(ang))), 0.0, 1.0)
    near = M // 3                  # ... and a third of them close to the lowest observation, where u is about 0
    cand[:near] = np.clip(comp[0] + (10.0 ** rs.uniform(-4.0, -1.6, near))[:, None] * rs.randn(near, D), 0.0, 1.0)
    rows = np.column_stack(([40.0, 38.0], rs.uniform(1e-4, 5e-4, 2), rs.uniform(0.8, 1.2, 2),
                            rs.uniform(0.15, 0.3, (2, D))))
    return {"comp": comp, "vals": vals, "cand": cand, "rows": rows}


def moments_mp(covar, comp, vals, hyper, cand):
    """(func_m, func_s) per candidate, lists of mpf."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(DPS):
        dr = rm._Draw(mp, covar, comp, hyper, cand)
        a = dr.alpha(vals)
        func_m = [mp.fsum(x * y for x, y in zip(dr.k[c], a)) + dr.mean for c in range(cand.shape[0])]
        return func_m, list(dr.s)


def pi_mp(func_m, func_s, best, xi):
    import mpmath
    mp = mpmath.mp
    with mp.workdps(DPS):
        b, x = mp.mpf(float(best)), mp.mpf(float(xi))
        return [mp.ncdf((b - x - m) / s) for m, s in zip(func_m, func_s)]


def lcb_mp(func_m, func_s, kappa):
    import mpmath
    mp = mpmath.mp
    with mp.workdps(DPS):
        k = mp.mpf(float(kappa))
        return [k * s - m for m, s in zip(func_m, func_s)]


def to_float64(vals):
    return rm.to_float64(vals)


def log10_mp(vals):
    return rm.log10_abs_mp(vals)


def tail_reference(prob, covar="Matern52"):
    """The fixture's reference arrays: PI rounded to float64 and as log10, (M, H, len(XIS)); the moments rounded; and for
    LCB_CASES candidates of draw 0 with func_m > 0 the kappa at which kappa func_s is within LCB_REL of func_m, with LCB of
    EVERY candidate and draw at that kappa, (cases, M, H)."""
    import mpmath
    M, H = prob["cand"].shape[0], prob["rows"].shape[0]
    best = np.min(prob["vals"])
    out = {"PI_ref": np.empty((M, H, len(XIS))), "log10PI": np.empty((M, H, len(XIS))), "func_m": np.empty((M, H)),
           "func_s": np.empty((M, H))}
    mom = []
    for h in range(H):
        func_m, func_s = moments_mp(covar, prob["comp"], prob["vals"], prob["rows"][h], prob["cand"])
        mom.append((func_m, func_s))
        out["func_m"][:, h], out["func_s"][:, h] = to_float64(func_m), to_float64(func_s)
        for k, xi in enumerate(XIS):
            p = pi_mp(func_m, func_s, best, xi)
            out["PI_ref"][:, h, k] = to_float64(p)
            out["log10PI"][:, h, k] = log10_mp(p)
    pos = np.nonzero(out["func_m"][:, 0] > 1e-3)[0]      # (kappa >= 0 needs func_m > 0)
    pick = pos[np.linspace(0, pos.size - 1, LCB_CASES).astype(int)]
    kappas = np.empty(LCB_CASES)
    lcb = np.empty((LCB_CASES, M, H))
    for i, c in enumerate(pick):
        with mpmath.mp.workdps(DPS):
            kappas[i] = float(mom[0][0][c] / mom[0][1][c] * (1 + mpmath.mpf(LCB_REL) / 2))
        for h in range(H):
            lcb[i, :, h] = to_float64(lcb_mp(mom[h][0], mom[h][1], kappas[i]))
    out["lcb_cand"], out["lcb_kappa"], out["lcb_ref"] = pick.astype(np.int64), kappas, lcb
    return out


def band_errors(got, ref, log10ref):
    """Max relative error of `got` against ref per band of log10 PI (TAIL_BANDS), over the entries whose reference is at
    least 1e-300; None for an empty band."""
    out = []
    for i, (lo, hi) in enumerate(TAIL_BANDS):
        sel = (log10ref >= lo) & ((log10ref <= hi) if i == 0 else (log10ref < hi)) & (ref >= 1e-300)
        out.append(float(np.max(np.abs(got[sel] - ref[sel]) / ref[sel])) if sel.any() else None)
    return out
