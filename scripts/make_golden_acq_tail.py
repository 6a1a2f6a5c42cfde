"""Write tests/golden/acq_tail_mp.npz: the tail problem of tests/acq_mp.py (probability of improvement from about 1/2 down
past 1e-300, and the lower confidence bound where kappa func_s cancels func_m), its inputs and the 50-digit references
(mpmath) rounded to float64, with log10 PI (defined below float64's range too).  The GPU tests read this file and never
import mpmath; tests/test_acq_mp.py regenerates the arrays and asserts the file holds exactly them.

Run:  python scripts/make_golden_acq_tail.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import acq_mp as am  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "acq_tail_mp.npz")


def generate():
    prob = am.tail_problem()
    out = dict(prob)
    out["xis"] = np.array(am.XIS)
    out.update(am.tail_reference(prob))
    return out


if __name__ == "__main__":
    g = generate()
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    for h in range(g["PI_ref"].shape[1]):
        lp = g["log10PI"][:, h, 0]
        print("draw %d: log10 PI from %.1f to %.3g; %d of %d below 1e-300, %d below 1e-100" %
              (h, lp.min(), lp.max(), int(np.sum(lp < -300)), lp.size, int(np.sum(lp < -100))))
        for lo, hi in am.TAIL_BANDS:
            print("   band [%g, %g): %d" % (lo, hi, int(np.sum((lp >= lo) & (lp < hi)))))
    print("LCB kappas", g["lcb_kappa"], "at candidates", g["lcb_cand"])
