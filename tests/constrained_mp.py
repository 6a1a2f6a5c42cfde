"""50-digit restatement (mpmath) of tests/constrained_oracle.constraint_prob: the yardstick of P(feasible) in its tails,
where the float64 oracle itself loses digits (the error of the latent mean m is amplified by about u^2 = (gain m)^2 in
the lower tail of Phi).  Every input is converted from the float64 arrays exactly (mpf(float) is exact); the distance is
the plain sum of squared differences, not the expanded GEMM form, so there is no cancellation to speak of.

Test code only: nothing in spearmint_amd imports this module, and the GPU tests read its results from
tests/golden/constrained_tail_mp.npz (scripts/make_golden_constrained_tail.py) instead of importing mpmath."""
import numpy as np

DPS = 50


def _corr_mp(mp, covar, r2):
    if covar == "Matern52":
        r = mp.sqrt(r2)
        return (1 + mp.sqrt(5) * r + (mp.mpf(5) / 3) * r2) * mp.exp(-mp.sqrt(5) * r)
    if covar == "Matern32":
        r = mp.sqrt(r2)
        return (1 + mp.sqrt(3) * r) * mp.exp(-mp.sqrt(3) * r)
    if covar in ("ARDSE", "SE"):
        return mp.exp(-r2 / 2)
    raise AttributeError("no covariance function %r" % (covar,))


def constraint_prob_mp(covar, comp_full, ff, chyper, cand, all_valid=False):
    """constrained_oracle.constraint_prob at DPS digits.  Returns a dict of lists of mpf, one entry per candidate:
    P = Phi(gain m), u = gain m, and absdot = sum_i |k_i alpha_i| (the condition of the sum m = k' alpha, for a forward
    bound of what a float64 evaluation of it can lose)."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(DPS):
        f = lambda v: mp.mpf(float(v))      # noqa: E731  (exact: a float64 is a dyadic rational)
        gain, noise_c, amp2_c = f(chyper[0]), f(chyper[1]), f(chyper[2])
        M = cand.shape[0]
        if all_valid:
            p = mp.ncdf(gain * 1)
            return {"P": [p] * M, "u": [gain * 1] * M, "absdot": [mp.mpf(0)] * M}
        ls = [mp.mpf(1) if covar == "SE" else f(v) for v in chyper[3:]]
        n, D = comp_full.shape
        X = [[f(comp_full[i, d]) / ls[d] for d in range(D)] for i in range(n)]
        C = [[f(cand[c, d]) / ls[d] for d in range(D)] for c in range(M)]

        def k(a, b):
            return _corr_mp(mp, covar, mp.fsum((a[d] - b[d]) ** 2 for d in range(D)))

        K = mp.matrix(n, n)
        for i in range(n):
            for j in range(i + 1):
                v = amp2_c * k(X[i], X[j])
                if i == j:
                    v = amp2_c * (k(X[i], X[j]) + f(1e-6)) + noise_c
                K[i, j] = v
                K[j, i] = v
        alpha = mp.cholesky_solve(K, mp.matrix([f(v) for v in ff]))
        P, U, A = [], [], []
        for c in range(M):
            terms = [amp2_c * k(X[i], C[c]) * alpha[i] for i in range(n)]
            u = gain * mp.fsum(terms)
            U.append(u)
            P.append(mp.ncdf(u))
            A.append(mp.fsum(abs(t) for t in terms))
        return {"P": P, "u": U, "absdot": A}


def to_float64(vals):
    """Round a list of mpf to float64 (values below the denormal range become 0.0)."""
    return np.array([float(v) for v in vals], dtype=np.float64)


def log10_mp(vals):
    """log10 of a list of positive mpf, as float64 -- defined where the value itself is below float64's range."""
    import mpmath
    with mpmath.mp.workdps(DPS):
        return np.array([float(mpmath.log10(v)) for v in vals], dtype=np.float64)


# ---- the tail problem (one definition for the generator, the CPU test and the GPU test) --------------------------------
TAIL_SEED, TAIL_N, TAIL_NBAD, TAIL_M, TAIL_D = 7, 48, 16, 400, 2
TAIL_BANDS = [(-3.0, 0.0), (-20.0, -3.0), (-100.0, -20.0), (-300.0, -100.0)]    # log10 P; the first closed, the others [lo, hi)


def tail_problem():
    """ff = 6 sign (0.5 + U) with sign = +1 at the valid and -1 at the violating observations, gain 3, noise_c 1e-3,
    amp2_c 1.2, Matern52: P from 1 down past 1e-300.  Draw 1 is the mild companion (ff read with gain 0.75)."""
    rs = np.random.RandomState(TAIL_SEED)
    n, D, M = TAIL_N, TAIL_D, TAIL_M
    comp = rs.rand(n, D)
    labels = np.ones(n)
    labels[rs.choice(n, TAIL_NBAD, replace=False)] = 0
    ff = 6.0 * np.where(labels > 0, 1.0, -1.0) * (0.5 + rs.rand(n))
    cand = rs.rand(M, D)
    vals = np.sum((comp - 0.4) ** 2, axis=1) + 0.02 * rs.randn(n)
    crows = np.array([np.concatenate(([3.0, 1e-3, 1.2], rs.uniform(0.3, 1.5, D))),
                      np.concatenate(([0.75, 1e-3, 1.2], rs.uniform(0.3, 1.5, D)))])
    rows = np.column_stack((rs.uniform(0.1, 0.3, 2), rs.uniform(1e-3, 1e-2, 2), rs.uniform(0.5, 1.5, 2),
                            rs.uniform(0.3, 1.5, (2, D))))
    return {"comp": comp, "labels": labels, "ff": ff, "cand": cand, "vals": vals, "crows": crows, "rows": rows}


def tail_reference(prob, ei):
    """The fixture's reference arrays from the inputs and the float64 EI of the valid-only GP (M, H): P rounded to float64,
    log10 P, u = gain m rounded, the forward bound's factor absdot, and EI x P rounded after the product."""
    import mpmath
    H = prob["crows"].shape[0]
    out = {k: np.empty((prob["cand"].shape[0], H)) for k in ("P_ref", "log10P", "u_ref", "absdot", "prod_ref")}
    for h in range(H):
        r = constraint_prob_mp("Matern52", prob["comp"], prob["ff"], prob["crows"][h], prob["cand"])
        out["P_ref"][:, h] = to_float64(r["P"])
        out["log10P"][:, h] = log10_mp(r["P"])
        out["u_ref"][:, h] = to_float64(r["u"])
        out["absdot"][:, h] = to_float64(r["absdot"])
        with mpmath.mp.workdps(DPS):
            out["prod_ref"][:, h] = to_float64([mpmath.mpf(float(e)) * p for e, p in zip(ei[:, h], r["P"])])
    return out


def band_errors(got, P_ref, log10P):
    """Max relative error of `got` against P_ref per band of log10 P (TAIL_BANDS), over the candidates whose reference
    is at least 1e-300; None for an empty band."""
    out = []
    for i, (lo, hi) in enumerate(TAIL_BANDS):
        sel = (log10P >= lo) & ((log10P <= hi) if i == 0 else (log10P < hi))
        out.append(float(np.max(np.abs(got[sel] - P_ref[sel]) / P_ref[sel])) if sel.any() else None)
    return out
