"""Write tests/golden/refine_tail_mp.npz: the 50-digit reference (mpmath, tests/refine_mp.py) of the refinement objective
spx_ei_grad_batch on the tail problem of tests/refine_mp.py -- per covariance, branch (plain, per second, fantasies) and
value set (mild, tail) the value f and the gradient g rounded to float64, and log10 |f| (defined below float64's range
too).  The inputs are not stored: tests/refine_mp.tail_problem rebuilds them from its seed without mpmath.  The GPU tests
read this file and never import mpmath; tests/test_refine_mp.py regenerates the arrays and asserts the file holds
exactly them.

Run:  python scripts/make_golden_refine_tail.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import refine_helpers as rh  # noqa: E402
from tests import refine_mp as rm  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "refine_tail_mp.npz")


def generate():
    return rm.tail_reference()


if __name__ == "__main__":
    g = generate()
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    for covar in rh.COVARS:
        for branch in rh.BRANCHES:
            for which in rm.SETS:
                lf = g[rm.key(covar, branch, which, "log10f")]
                idx = rm.band_of(lf)
                print("%-8s %-6s %-4s points per band %s, below 1e-300: %d, log10 |f| from %.1f to %.2f" %
                      (covar, branch, which, [int(np.sum(idx == i)) for i in range(len(rm.TAIL_BANDS))],
                       int(np.sum(lf < -300)), lf.min(), lf.max()))
