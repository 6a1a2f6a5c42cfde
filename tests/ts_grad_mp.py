"""The 50-digit yardstick of sin2pi (spearmint_amd/csrc/ts_device.h): reduced phases r in [-1/2, 1/2] and sin(2 pi r) of each as
a double-double (hi = the correctly rounded float64, lo = the rest), as tests/ts_mp.py does for cos2pi.
`python -m tests.ts_grad_mp` rewrites tests/golden/ts_sin_mp.npz (data only: r, hi, lo); tests/test_ts_grad_host.py regenerates
a part of the table where mpmath is installed and compares.  Needs mpmath; nothing else imports it."""
import os

import numpy as np

DIGITS = 50
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ts_sin_mp.npz")
TINY = 2.2250738585072014e-308          # the smallest normal number


def points():
    """Edge cases first -- +-0, +-1/2 (zeros of the sine), +-1/4 (where the minimum switches sides) and four float64 neighbours
    on BOTH sides of each, +-1/8, +-3/8, every power of two from 2^-1 down to the smallest sub-normal 2^-1074 with both signs
    on every eighth, 1.5 and 1.75 times some of them -- then a dense sweep: a lattice of 4001 points over [-1/2, 1/2] and a
    seeded fill, uniform, logarithmic towards 0 and logarithmic towards +-1/4 and +-1/2."""
    edge = [0.0, -0.0, 0.5, -0.5, 0.25, -0.25, 0.125, -0.125, 0.375, -0.375]
    for c in (0.25, 0.5, 0.125, 0.375):
        x = c
        for _ in range(4):
            x = np.nextafter(x, 0.0)
            edge += [x, -x]
    for c in (0.25, 0.125, 0.375, 0.0):
        x = c
        for _ in range(4):
            x = np.nextafter(x, 1.0)
            edge += [x, -x]
    for k in range(1, 1075):
        v = 2.0 ** -k
        edge.append(v)
        if k % 8 == 0:
            edge += [-v, 1.5 * v, -1.75 * v]
    edge += [TINY, -TINY, np.nextafter(TINY, 0.0), 3 * 5e-324, -7 * 5e-324, 1e-300, 1e-310, -1e-320]
    rs = np.random.RandomState(20241021)
    fill = [np.linspace(-0.5, 0.5, 4001),
            rs.uniform(-0.5, 0.5, 3000),
            rs.choice([-1.0, 1.0], 600) * 10.0 ** rs.uniform(-18, np.log10(0.5), 600),
            rs.choice([-1.0, 1.0], 600) * (0.25 + rs.choice([-1.0, 1.0], 600) * 10.0 ** rs.uniform(-17, np.log10(0.25), 600)),
            rs.choice([-1.0, 1.0], 300) * (0.5 - 10.0 ** rs.uniform(-17, np.log10(0.25), 300))]
    r = np.concatenate([np.array(edge)] + fill)
    return r[np.abs(r) <= 0.5]


def reference(r):
    """(hi, lo) of sin(2 pi r) at DIGITS digits; the zeros at 0 and +-1/2 are exact and carry r's sign."""
    import mpmath as mp
    hi, lo = np.empty(len(r)), np.empty(len(r))
    with mp.workdps(DIGITS):
        for i, x in enumerate(r):
            x = float(x)
            if x == 0.0 or abs(x) == 0.5:
                hi[i], lo[i] = np.copysign(0.0, x), 0.0
                continue
            v = mp.sin(2 * mp.pi * mp.mpf(x))
            hi[i] = float(v)
            lo[i] = float(v - mp.mpf(hi[i]))
    return hi, lo


def ulp_errors(got, hi, lo):
    """|got - ref| in ulps of the reference (the spacing of float64 at |hi|: for a sub-normal reference and at hi = 0 that is
    the quantum 2^-1074)."""
    sp = np.spacing(np.abs(hi))
    return np.abs((np.asarray(got) - hi) - lo) / sp


if __name__ == "__main__":
    r = points()
    hi, lo = reference(r)
    np.savez_compressed(FIXTURE, r=r, hi=hi, lo=lo)
    print("wrote %s: %d points" % (FIXTURE, len(r)))
