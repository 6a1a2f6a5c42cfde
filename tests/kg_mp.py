"""50-digit yardstick (mpmath) of the knowledge gradient of a set of lines (include/spx.h: SPX_ACQ_KG),

    KG = sum_k (b_k - b_{k+1}) f(-|z_k|),   f(z) = phi(z) + z Phi(z),

over the EXACT lower envelope: the lines are sorted by slope and scanned at 50 digits, so which lines are on it and where they
meet is decided without float64 rounding.

`python -m tests.kg_mp` writes tests/golden/kg_mp.npz: the line sets (n, mu, b: every number a float64 fixed by this text), the
50-digit values rounded to float64, max |z_k| of the exact envelope, the size of one unit of error per set, and the float64
oracle's (tests/kg_oracle.py) worst error per band in those units, as measured when the fixture was made.

THE UNIT the errors are counted in, and why.  A term is db f(-|z|) with f = phi(z) - |z| Phi(-|z|): two parts that cancel (to
phi / z^2 in the tail), each evaluated to about one rounding, and a breakpoint z that carries a few roundings of its own
(two subtractions and a division of float64 inputs taken as exact), which move f by f'(z) dz = Phi(-|z|) |z| x a few 2^-53.  Both
are of the size of the UNCANCELLED parts; and each part is an exponential of -z^2 / 2, whose argument carries one rounding of
its own, z^2 / 2 x 2^-53 relative in the result (ei_device.h's EI formula in its lower tail: the weight tests/ehvi_mp.py uses).  So
    unit = 2^-53 sum_k db_k p_k (1 + z_k^2 / 2)  +  sum_{|z_k| > 37.5} db_k p_k  +  8 x 2^-1074 sum_k db_k,
    db_k = b_k - b_{k+1},   p_k = phi(z_k) + |z_k| Phi(-|z_k|):
the natural scale sum_k db f(-|z_k|) with the cancellation inside f undone, which is also what the rounding of the breakpoints
moves it by.  The second and third parts are what the sub-normal range leaves open: beyond |z| = 37.5 phi and Phi are sub-normal
and a library's erfc may flush Phi to zero there (scipy's does), which leaves phi alone standing -- the whole of p_k; and every
part of f is a multiple of 2^-1074.  Both are exactly zero for a set without a breakpoint beyond 37.5 resp. without any.  A set
whose exact value is 0 (one line on the envelope) has unit 0: only +0.0 is right.
The PINNED error of a band is max(measured, 1), as for the other yardsticks: the yardstick itself is stored rounded to float64.

Bands, by max |z_k| over the exact envelope:  z2: below 2,  z8: 2 to 8,  z30: 8 to 30,  z40: beyond 30 (out to 40, past the
underflow of f at 38.6).  A set without a breakpoint (value 0) belongs to z2.

Test code only: nothing in spearmint_amd imports this module."""
import os

import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1074
BANDS = ("z2", "z8", "z30", "z40")
SIZES = (1, 2, 3, 16, 17, 64, 65, 256)
SUBNORMAL_BEYOND = 37.5
FAR = (2.5, 5.0, 8.0, 12.0, 20.0, 30.0, 37.0, 37.6, 38.2, 38.6, 40.0)


def up(x, k=1):
    for _ in range(k):
        x = float(np.nextafter(x, np.inf))
    return x


def cases():
    """[(name, mu, b)]: line 0 first, every number a float64 fixed by this text (numpy's legacy generator is frozen)."""
    out = []
    rng = np.random.RandomState(20261021)
    for n in SIZES:
        for rep, spread in enumerate((1.0, 0.05, 8.0)):
            out.append(("rand_n%d_%d" % (n, rep), rng.randn(n) * spread, rng.randn(n)))
    # exact cases
    out.append(("equal_slopes", np.array([0.3, -1.0, 2.0, -1.0]), np.full(4, 0.7)))
    out.append(("equal_slopes_zero", np.array([0.3, -1.0, 2.0]), np.zeros(3)))
    out.append(("duplicates", np.array([0.0, 0.5, 0.5, -0.25, -0.25, 0.0]), np.array([1.0, 0.25, 0.25, -0.5, -0.5, 1.0])))
    out.append(("parallel", np.array([0.0, 0.5, 0.25, -0.25, 0.75]), np.array([1.0, 0.25, 0.25, -0.5, -0.5])))
    # three (and five) lines through one point (z0, y0), exactly: dyadic slopes, mu_i = y0 - b_i z0
    z0, y0 = 0.5, -0.75
    b3 = np.array([1.0, 0.25, -0.5])
    out.append(("three_through_a_point", y0 - b3 * z0, b3))
    b5 = np.array([0.125, 2.0, -1.0, 0.5, -0.25])
    out.append(("five_through_a_point", y0 - b5 * z0, b5))
    out.append(("three_and_a_lower_one", np.append(y0 - b3 * z0, -2.0), np.append(b3, 0.0)))
    # slopes one ulp apart
    out.append(("ulp_slopes", np.array([0.0, 1e-17, -1e-17, 0.5]), np.array([1.0, up(1.0), up(1.0, 2), 0.0])))
    out.append(("ulp_slopes_far", np.array([0.0, 4e-16, 0.3]), np.array([0.5, up(0.5), -0.5])))
    # a zero slope for line 0 (func_v = 0: a candidate on a noiseless observation)
    out.append(("zero_slope_line0", np.array([0.1, 0.0, -0.2, 0.4]), np.array([0.0, 0.3, -0.6, 0.05])))
    out.append(("zero_slope_line0_alone", np.array([-3.0, 0.0, 0.2]), np.array([0.0, 1e-3, -1e-3])))
    # breakpoints out to |z| = 40: line 0 = Z, line 1 = the constant -z (they meet at Z = -z), and with a third line between
    for z in FAR:
        out.append(("far_%g" % z, np.array([0.0, -z]), np.array([1.0, 0.0])))
        out.append(("far3_%g" % z, np.array([0.0, -z, -0.5 * z - 0.125]), np.array([1.0, 0.0, 0.5])))
        out.append(("farpos_%g" % z, np.array([0.0, z * 0.25]), np.array([-0.25, 0.0])))
    return out


def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def kg_mp(mu, b):
    """(value, unit, max |z_k|) of one set as mpf: sort, stack scan, sum -- all at 50 digits."""
    mp = _mp()
    mu = [mp.mpf(float(x)) for x in mu]
    b = [mp.mpf(float(x)) for x in b]
    order = sorted(range(len(b)), key=lambda i: (-b[i], mu[i], i))
    keep = []
    for k in order:
        if keep and b[k] == b[keep[-1]]:
            continue
        keep.append(k)
    stack, zs = [keep[0]], []
    for k in keep[1:]:
        while True:
            j = stack[-1]
            z = (mu[k] - mu[j]) / (b[j] - b[k])
            if zs and z <= zs[-1]:
                stack.pop()
                zs.pop()
                continue
            break
        stack.append(k)
        zs.append(z)
    val, unit, sub, zmax, flushed = mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(0)
    for i, z in enumerate(zs):
        db = b[stack[i]] - b[stack[i + 1]]
        az = abs(z)
        phi = mp.exp(-az * az / 2) / mp.sqrt(2 * mp.pi)
        tail = az * mp.erfc(az / mp.sqrt(2)) / 2
        val += db * (phi - tail)
        unit += db * (phi + tail) * (1 + az * az / 2)
        if az > SUBNORMAL_BEYOND:
            flushed += db * (phi + tail)
        sub += db
        zmax = max(zmax, az)
    return val, mp.mpf(U) * unit + flushed + 8 * mp.mpf(TINY) * sub, zmax


def band_of(zmax):
    return BANDS[0] if zmax < 2.0 else BANDS[1] if zmax < 8.0 else BANDS[2] if zmax < 30.0 else BANDS[3]


def error(got, want, unit):
    """Worst error in units; a set of unit 0 must be +0.0 exactly."""
    got, want, unit = (np.asarray(x, dtype=np.float64) for x in (got, want, unit))
    e = np.zeros(got.shape)
    pos = unit > 0.0
    e[pos] = np.abs(got[pos] - want[pos]) / unit[pos]
    zero_ok = (got == 0.0) & ~np.signbit(got)
    e[~pos & ~zero_ok] = np.inf
    e[np.isnan(got)] = np.inf
    return float(np.max(e)) if e.size else 0.0


def pinned(fx, band):
    return max(float(fx["oracle_err_" + band]), 1.0)


def sets_of(fx):
    """[(name, mu, b)] as stored."""
    off = np.concatenate(([0], np.cumsum(fx["n"])))
    return [(str(fx["names"][i]), fx["mu"][off[i]:off[i + 1]], fx["b"][off[i]:off[i + 1]]) for i in range(len(fx["n"]))]


def main():
    from tests import kg_oracle as ko
    cs = cases()
    vals, units, zmaxs = [], [], []
    for _, mu, b in cs:
        v, u, z = kg_mp(mu, b)
        vals.append(float(v)); units.append(float(u)); zmaxs.append(float(z))
    fx = {"names": np.array([c[0] for c in cs]), "n": np.array([len(c[1]) for c in cs]),
          "mu": np.concatenate([c[1] for c in cs]), "b": np.concatenate([c[2] for c in cs]),
          "kg": np.array(vals), "unit": np.array(units), "zmax": np.array(zmaxs)}
    got = np.array([ko.value(mu, b) for _, mu, b in cs])
    bands = np.array([band_of(z) for z in zmaxs])
    for band in BANDS:
        sel = bands == band
        fx["oracle_err_" + band] = error(got[sel], fx["kg"][sel], fx["unit"][sel])
        print("float64 oracle, %s: %d sets, worst error %.3g units" % (band, int(np.sum(sel)), fx["oracle_err_" + band]))
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kg_mp.npz"), **fx)


if __name__ == "__main__":
    main()
