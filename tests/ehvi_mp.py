"""50-digit yardstick (mpmath) of the expected hypervolume improvement (include/spx.h: SPX_ACQ_EHVI), as the strip sum

    EHVI = sum_{i=0..n} [G1(a_{i+1}) - G1(a_i)] G2(b_i),   G_k(y) = s_k (u Phi(u) + phi(u)), u = (y - m_k) / s_k

and, on one small case, directly as the integral of I(u, v) = sum_i (a_{i+1} - max(u, a_i))+ (b_i - v)+ against the two
Gaussian densities (direct_integral), which is what the strip sum is derived from.

`python -m tests.ehvi_mp` writes tests/golden/ehvi_mp.npz: per band the candidates' moments (m1, v1, m2, v2), the front and the
reference point, the 50-digit values rounded to float64, the size of one unit of error per candidate (scale(): the natural
scale sum_i [G1(a_{i+1}) + G1(a_i)] G2(b_i) in units of u = 2^-53, weighted by the conditioning of the EI formula in its
lower tail, plus what the sub-normal range leaves open), and the float64 oracle's (tests/ehvi_oracle.py) own worst error
against them in those units, as measured when the fixture was made.  The PINNED error of a band is max(measured, 1): the
yardstick itself is stored rounded to float64, half a unit of its own last place, so no float64 result can be held to less
than about one unit, and a band where the oracle happened to land under it says nothing about what another correctly rounded
library would give.

Bands:
    n0        no front: the product G1(r1) G2(r2); u_k = (r_k - m_k) / s_k from +8 down to -38.2
    n1 n2 n7  fronts of 1, 2 and 7 points under the same candidates
    ulp       7 points, neighbours 1 ulp apart in either objective
    place     7 points; candidates that dominate the whole front, that are dominated by all of it, and that sit on a front point
    n4096     the largest front the engine takes

Test code only: nothing in spearmint_amd imports this module."""
import os

import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1074
BANDS = ("n0", "n1", "n2", "n7", "ulp", "place", "n4096")
US = (8.0, 5.0, 2.0, 0.5, 0.0, -0.5, -2.0, -5.0, -8.0, -12.0, -20.0, -30.0, -37.0, -37.6, -38.2)


def _front(n, a0=0.2, a1=1.7, b0=-0.4, b1=2.3):
    t = (np.arange(n) + 0.5) / max(n, 1)
    return a0 + (a1 - a0) * t, b1 - (b1 - b0) * np.sqrt(t), a1 + 0.1 * (a1 - a0), b1 + 0.1 * (b1 - b0)


def _lattice(r1, r2, s1=0.3, s2=0.45):
    """Candidates whose u_1 / u_2 against the reference point walk US: both together, then each against a central other."""
    m1, m2 = [], []
    for u in US:
        m1 += [r1 - u * s1, r1 - u * s1, r1 - 0.5 * s1]
        m2 += [r2 - u * s2, r2 - 0.5 * s2, r2 - u * s2]
    m1, m2 = np.array(m1), np.array(m2)
    return m1, np.full(m1.shape, s1 * s1), m2, np.full(m2.shape, s2 * s2)


def cases():
    """{band: (m1, v1, m2, v2, a, b, r1, r2)}, every number a float64 fixed by this text."""
    out = {}
    for n in (0, 1, 2, 7):
        a, b, r1, r2 = _front(n)
        out["n%d" % n] = _lattice(r1, r2) + (a, b, r1, r2)

    def up(x, k=1):
        return x if k == 0 else up(float(np.nextafter(x, np.inf)), k - 1)

    def dn(x, k=1):
        return x if k == 0 else dn(float(np.nextafter(x, -np.inf)), k - 1)
    a = np.array([1.0, up(1.0), up(1.0, 2), 1.5, 2.0, up(2.0), 2.5])
    b = np.array([3.0, dn(3.0), dn(3.0, 2), 2.0, 1.5, dn(1.5), 1.0])
    m1 = np.array([1.0, 1.0, 0.9, 2.0, 2.0, 1.5, 3.2, 1.0000000000000002])
    s1 = np.array([1e-3, 0.5, 0.2, 1e-8, 0.7, 0.1, 0.6, 1e-12])
    m2 = np.array([3.0, 2.9, 3.0, 1.5, 1.4, 2.0, 0.5, 2.9999999999999996])
    s2 = np.array([1e-3, 0.5, 0.3, 1e-8, 0.9, 0.1, 0.8, 1e-12])
    out["ulp"] = (m1, s1 * s1, m2, s2 * s2, a, b, 2.75, 3.25)
    a, b, r1, r2 = _front(7)
    m1 = np.array([-3.0, -0.5, 0.1, 2.5, 1.9, 5.0, a[3], a[0], a[6], a[3]])
    s1 = np.array([0.5, 0.05, 1e-3, 0.2, 0.01, 1.0, 0.1, 1e-6, 0.3, 1e-9])
    m2 = np.array([-4.0, -1.0, -0.5, 3.0, 2.7, 6.0, b[3], b[0], b[6], b[3]])
    s2 = np.array([0.5, 0.05, 1e-3, 0.2, 0.01, 1.0, 0.1, 1e-6, 0.3, 1e-9])
    out["place"] = (m1, s1 * s1, m2, s2 * s2, a, b, r1, r2)
    n = 4096
    a = np.arange(1, n + 1) / 4096.0
    b = 1.0 / (a + 0.1)
    m1 = np.array([0.5, -1.0, 2.0, a[1023], 0.5, 1.0])
    s1 = np.array([0.2, 0.1, 0.1, 0.05, 1.0, 0.01])
    m2 = np.array([2.0, 0.0, 20.0, b[1023], 3.0, 1.0])
    s2 = np.array([0.5, 0.1, 0.1, 0.05, 2.0, 0.01])
    out["n4096"] = (m1, s1 * s1, m2, s2 * s2, a, b, 1.1, float(b[0]) + 1.0)
    return out


def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def g_mp(y, m, v):
    mp = _mp()
    s = mp.sqrt(mp.mpf(float(v)))
    u = (mp.mpf(float(y)) - mp.mpf(float(m))) / s
    return s * (u * (mp.erfc(-u / mp.sqrt(2)) / 2) + mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi))


def ehvi_mp(m1, v1, m2, v2, a, b, r1, r2):
    """(values, units) as lists of mpf: the strip sum at 50 digits for every candidate."""
    mp = _mp()
    edges = list(a) + [r1]
    levels = [r2] + list(b)
    vals, units = [], []
    for c in range(len(m1)):
        g_lo, acc, unit = mp.mpf(0), mp.mpf(0), mp.mpf(0)
        for e, l in zip(edges, levels):
            g_hi = g_mp(e, m1[c], v1[c])
            g2 = g_mp(l, m2[c], v2[c])
            acc += (g_hi - g_lo) * g2
            unit += (abs(g_hi) + abs(g_lo)) * abs(g2)
            g_lo = g_hi
        vals.append(acc); units.append(unit)
    return vals, units


def direct_integral(m1, v1, m2, v2, a, b, r1, r2):
    """E[I(f1, f2)] by quadrature of I against the two Gaussian densities, cell by cell of the front's staircase (mpf).  I is
    bilinear inside a cell and zero outside the reference box, so Gauss-Legendre panels between the breakpoints converge fast."""
    mp = _mp()
    edges = [mp.mpf(float(x)) for x in list(a) + [r1]]
    levels = [mp.mpf(float(x)) for x in [r2] + list(b)]
    m1, m2 = mp.mpf(float(m1)), mp.mpf(float(m2))
    s1, s2 = mp.sqrt(mp.mpf(float(v1))), mp.sqrt(mp.mpf(float(v2)))
    lower = [None] + edges[:-1]

    def pdf(x, m, s):
        return mp.exp(-((x - m) / s) ** 2 / 2) / (s * mp.sqrt(2 * mp.pi))

    def area(u, v):
        t = mp.mpf(0)
        for lo, hi, lv in zip(lower, edges, levels):
            w = hi - (u if lo is None else max(u, lo))
            if w > 0 and lv > v:
                t += w * (lv - v)
        return t
    ucuts = [m1 - 60 * s1] + [e for e in edges if e > m1 - 60 * s1]
    vcuts = [m2 - 60 * s2] + sorted(l for l in levels if l > m2 - 60 * s2)
    # finer panels around each mean so that a narrow density is resolved
    for cuts, m, s in ((ucuts, m1, s1), (vcuts, m2, s2)):
        extra = [m + k * s for k in (-12, -8, -5, -3, -1.5, 0, 1.5, 3, 5, 8, 12) if cuts[0] < m + k * s < cuts[-1]]
        cuts[:] = sorted(set(cuts + extra))
    return mp.quad(lambda u, v: area(u, v) * pdf(u, m1, s1) * pdf(v, m2, s2), ucuts, vcuts)


DIRECT_CASE = (0.9, 0.09, 1.4, 0.16, (0.5, 1.2), (2.0, 0.8), 1.6, 2.4)      # m1, v1, m2, v2, a, b, r1, r2: a two-point front


def to_float64(v):
    return np.array([float(x) for x in v])


DBL_MIN = 2.0 ** -1022
SUBNORMAL_BELOW = -37.5


def scale(m1, v1, m2, v2, a, b, r1, r2, parts=False):
    """The size of one unit of error per candidate (float64, from the oracle's own G: a scale needs no 50 digits):

        u [ sum_i (c(u1_{i+1}) G1(a_{i+1}) + c(u1_i) G1(a_i)) G2(b_i) + (G1(a_{i+1}) + G1(a_i)) c(u2_i) G2(b_i) ] + 2^-1074 + A

    1. The natural scale sum_i [G1(a_{i+1}) + G1(a_i)] G2(b_i): the strip differences cancel when front points are close.
    2. c(u) = 1 + 2 u^4 for u < 0 (1 otherwise), the conditioning of G = s (u Phi(u) + phi(u)) -- ei_device.h's formula, which
       EHVI is required to use as it is -- in its lower tail: the two terms are each about s phi(u) and cancel to s phi(u) / u^2.
       phi = exp(-u^2 / 2) carries the rounding of its argument, u^2 / 2 units of its own last place, Phi through erfc's
       argument u^2 units, and either library's function error comes on top; divided by what is left after the cancellation
       that is (3/2 u^2 + a few) u^2 <= 2 u^4 + 1 units of G.  A strip whose G sits at u = -8 is therefore known to 8e3 units
       and one at u = -35 to 3e6, whatever the candidate's distance to the reference point is: a candidate just below a
       front point has its whole value in such a strip.
    3. One sub-normal quantum, all a float64 keeps of the deepest values.
    4. A, what the number format leaves open below the normal range.  From u = -37.5 down Phi(u), and a little further
       phi(u), are sub-normal, and a library may round such a result to zero wherever it likes: scipy's ndtr (cephes) returns
       0 from u = -37.68 on, glibc's erfc from -38.5 on, exp keeps its sub-normals down to -38.6.  Each of G's two terms is
       then off by up to s (1 + |u|) 2^-1022, and A is that amount carried through the strip sum:
       2^-1022 sum_i [(f1(a_{i+1}) + f1(a_i)) G2(b_i) + (G1(a_{i+1}) + G1(a_i)) f2(b_i)], f_k(y) = s_k (1 + |u|) if u < -37.5 else 0.
       It is exactly zero for a candidate none of whose strips has u < -37.5, so it cannot cover an error in the normal range;
       parts=True returns (scale, A, the smallest u over every strip of both objectives) for the tests that assert this."""
    from tests import ehvi_oracle as eo
    m1, v1, m2, v2 = (np.asarray(x, dtype=np.float64) for x in (m1, v1, m2, v2))
    edges, levels = eo.strips(a, b, r1, r2)

    def strip_parts(y, m, v):
        with np.errstate(all="ignore"):
            s = np.sqrt(v)
            u = (y - m) / s
            c = np.where(u < 0.0, 1.0 + 2.0 * u ** 4, 1.0)
            f = np.where(u < SUBNORMAL_BELOW, s * (1.0 + np.abs(u)), 0.0)
            return np.abs(eo.g(m, v, y)), c, f, u
    unit, allow = np.zeros(m1.shape), np.zeros(m1.shape)
    g_lo, c_lo, f_lo = np.zeros(m1.shape), np.ones(m1.shape), np.zeros(m1.shape)
    u_min = np.full(m1.shape, np.inf)
    with np.errstate(all="ignore"):
        for e, l in zip(edges, levels):
            g_hi, c_hi, f_hi, u1 = strip_parts(e, m1, v1)
            g2, c2, f2, u2 = strip_parts(l, m2, v2)
            u_min = np.fmin(u_min, np.fmin(u1, u2))
            unit = unit + (c_hi * g_hi + c_lo * g_lo) * g2 + (g_hi + g_lo) * c2 * g2
            allow = allow + (f_hi + f_lo) * g2 + (g_hi + g_lo) * f2
            g_lo, c_lo, f_lo = g_hi, c_hi, f_hi
    unit = np.nan_to_num(unit, nan=0.0, posinf=0.0)
    allow = np.nan_to_num(allow, nan=0.0, posinf=0.0)
    out = U * unit + TINY + DBL_MIN * allow
    return (out, DBL_MIN * allow, u_min) if parts else out


def error(got, ref, scale_):
    """Worst |got - ref| in units of scale()."""
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(got - ref) / scale_))


def pinned(fx, band):
    """max(measured, 1)."""
    return max(float(fx[band + "_orc_err"]), 1.0)


def generate():
    from tests import ehvi_oracle as eo
    fx = {}
    for band, (m1, v1, m2, v2, a, b, r1, r2) in cases().items():
        vals, units = ehvi_mp(m1, v1, m2, v2, a, b, r1, r2)
        fx[band + "_m1"], fx[band + "_v1"], fx[band + "_m2"], fx[band + "_v2"] = m1, v1, m2, v2
        fx[band + "_a"], fx[band + "_b"], fx[band + "_ref"] = np.asarray(a, float), np.asarray(b, float), np.array([r1, r2])
        fx[band + "_ehvi"], fx[band + "_unit"] = to_float64(vals), to_float64(units)
        fx[band + "_scale"] = scale(m1, v1, m2, v2, a, b, r1, r2)
        fx[band + "_orc_err"] = np.array(error(eo.ehvi(m1, v1, m2, v2, a, b, r1, r2), fx[band + "_ehvi"], fx[band + "_scale"]))
    d = DIRECT_CASE
    fx["direct_integral"] = np.array(float(direct_integral(*d)))
    fx["direct_strips"] = np.array(float(ehvi_mp([d[0]], [d[1]], [d[2]], [d[3]], d[4], d[5], d[6], d[7])[0][0]))
    return fx


if __name__ == "__main__":
    fx = generate()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ehvi_mp.npz")
    np.savez(path, **fx)
    for band in BANDS:
        print(band, "oracle error %.3g units over %d candidates" % (float(fx[band + "_orc_err"]), len(fx[band + "_m1"])))
    print("direct integral %.17g, strip sum %.17g" % (float(fx["direct_integral"]), float(fx["direct_strips"])))
    print("->", path)
