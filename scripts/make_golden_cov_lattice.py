"""Write tests/golden/cov_lattice_mp.npz: the sorted unique exact r^2 of the lattice problems of tests/cov_mp.py and, per
kind (Matern52, Matern32, ARDSE), the 50-digit correlation rounded to float64 with its error unit u, plus the 50-digit
log-likelihood of the two-observation cases.  The inputs themselves are rebuilt from their seeds.  The GPU tests read this
file and never import mpmath; tests/test_cov_mp.py regenerates the arrays and asserts the file holds exactly them.

Run:  python scripts/make_golden_cov_lattice.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cov_mp as cv  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cov_lattice_mp.npz")


def generate():
    return cv.reference()


if __name__ == "__main__":
    g = generate()
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    r2 = g["r2"]
    print("%d distinct r^2: %d zeros, positive from %.3g to %.3g" % (r2.size, int(np.sum(r2 == 0)), r2[r2 > 0].min(), r2.max()))
    for kind in cv.KINDS:
        k = g["k_" + kind]
        print("%-9s %d denormal results, %d zeros below the clamp, %d past it" %
              (kind, int(np.sum((k > 0) & (k < 2.0 ** -1022))), int(np.sum((k == 0) & (r2 < cv.CLAMP[kind]))),
               int(np.sum(r2 >= cv.CLAMP[kind]))))
