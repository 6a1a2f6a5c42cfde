"""The 50-digit yardstick of cos2pi (spearmint_amd/csrc/ts_device.h): reduced phases r in [-1/2, 1/2] and cos(2 pi r) of each as
a double-double (hi = the correctly rounded float64, lo = the rest), so that an error can be counted in ulps of the result to
a small fraction of one.  `python -m tests.ts_mp` rewrites tests/golden/ts_cos_mp.npz (data only: r, hi, lo);
tests/test_ts_mp.py regenerates the table and compares.  Needs mpmath; nothing else imports it."""
import os

import numpy as np

DIGITS = 50
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ts_cos_mp.npz")


def points():
    """Edge cases first -- 0, +-1/2, +-1/4 (the zeros of the cosine) and their float64 neighbours, +-1/8 (where 1/4 - |r| stops
    being exact) and its neighbours, the smallest normal and denormal numbers -- then a seeded fill: uniform on [-1/2, 1/2],
    logarithmic towards 0 and logarithmic towards the zeros at +-1/4."""
    edge = [0.0, 0.5, -0.5, 0.25, -0.25, 0.125, -0.125, 0.375, -0.375]
    for c in (0.25, 0.125, 0.5, 0.375):
        x = c
        for _ in range(4):
            x = np.nextafter(x, 0.0)
            edge += [x, -x]
    x = 0.25
    for _ in range(4):
        x = np.nextafter(x, 1.0)
        edge += [x, -x]
    edge += [5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, 1e-200, 1e-100, 2.0 ** -30, 2.0 ** -53]
    rs = np.random.RandomState(20240611)
    fill = [rs.uniform(-0.5, 0.5, 3000),
            rs.choice([-1.0, 1.0], 600) * 10.0 ** rs.uniform(-18, np.log10(0.5), 600),
            rs.choice([-1.0, 1.0], 800) * (0.25 + rs.choice([-1.0, 1.0], 800) * 10.0 ** rs.uniform(-17, np.log10(0.25), 800))]
    r = np.concatenate([np.array(edge)] + fill)
    return r[np.abs(r) <= 0.5]


def reference(r):
    """(hi, lo) of cos(2 pi r) at DIGITS digits."""
    import mpmath as mp
    hi, lo = np.empty(len(r)), np.empty(len(r))
    with mp.workdps(DIGITS):
        for i, x in enumerate(r):
            v = mp.mpf(0) if abs(float(x)) == 0.25 else mp.cos(2 * mp.pi * mp.mpf(float(x)))      # (the zeros are exact)
            hi[i] = float(v)
            lo[i] = float(v - mp.mpf(hi[i]))
    return hi, lo


def ulp_errors(got, hi, lo):
    """|got - ref| in ulps of the reference (the spacing of float64 at |hi|; at hi = 0: the smallest denormal)."""
    sp = np.spacing(np.abs(hi))
    return np.abs((np.asarray(got) - hi) - lo) / sp


if __name__ == "__main__":
    r = points()
    hi, lo = reference(r)
    np.savez_compressed(FIXTURE, r=r, hi=hi, lo=lo)
    print("wrote %s: %d points" % (FIXTURE, len(r)))
