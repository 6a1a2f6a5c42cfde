"""tests/golden/ts_cos_mp.npz is what tests/ts_mp.py writes: regenerated at 50 digits and compared, and the long-double cosine
of tests/ts_oracle.py held to it."""
import numpy as np
import pytest

from tests import ts_mp, ts_oracle as tso

mp = pytest.importorskip("mpmath")


def test_fixture_is_what_the_generator_writes():
    fx = np.load(ts_mp.FIXTURE)
    r = ts_mp.points()
    assert np.array_equal(r, fx["r"])
    assert set(fx.files) == {"r", "hi", "lo"}                     # data only
    sub = np.r_[0:60, 60:len(r):37]
    hi, lo = ts_mp.reference(r[sub])
    assert np.array_equal(hi, fx["hi"][sub]) and np.array_equal(lo, fx["lo"][sub])
    for x in (0.0, 0.5, -0.5, 0.25, -0.25, 5e-324, -5e-324):
        assert x in r
    assert np.all(np.abs(r) <= 0.5)


def test_oracle_cosine_against_50_digits():
    """The oracle's cos2pi (long double, rounded once): absolute error at most 2^-53 + 2 pi 2^-64 everywhere -- it is the
    reference of the GPU prior test's bound, whose eps_cos is absolute."""
    fx = np.load(ts_mp.FIXTURE)
    err = np.abs((tso.cos2pi(fx["r"]) - fx["hi"]) - fx["lo"])
    assert np.max(err) <= 2.0 ** -53 + 2 * np.pi * 2.0 ** -64, np.max(err)
