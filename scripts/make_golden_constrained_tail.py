"""Write tests/golden/constrained_tail_mp.npz: the tail problem of tests/constrained_mp.py (P(feasible) from 1 down past
1e-300), its inputs, the float64 EI of the valid-only GP, and the 50-digit reference of P (mpmath) -- rounded to float64,
as log10 P (defined below float64's range too), the latent u = gain m, the forward bound's sum |k_i alpha_i|, and EI x P
rounded after the product.  The GPU tests read this file and never import mpmath; tests/test_constrained_mp.py regenerates
the 50-digit arrays and asserts the file holds exactly them.

Run:  python scripts/make_golden_constrained_tail.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import constrained_mp as cm  # noqa: E402
from tests import constrained_oracle as co  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "constrained_tail_mp.npz")


def generate():
    prob = cm.tail_problem()
    good = prob["labels"] > 0
    ei = np.stack([co.ei_nopend("Matern52", prob["comp"][good], prob["vals"][good], prob["rows"][h], prob["cand"])
                   for h in range(prob["rows"].shape[0])], axis=1)
    out = dict(prob)
    out["ei_ref"] = ei
    out.update(cm.tail_reference(prob, ei))
    return out


if __name__ == "__main__":
    g = generate()
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    for h in range(g["P_ref"].shape[1]):
        lp = g["log10P"][:, h]
        print("draw %d: log10 P from %.1f to %.3g; %d of %d below 1e-300, %d below 1e-100" %
              (h, lp.min(), lp.max(), int(np.sum(lp < -300)), lp.size, int(np.sum(lp < -100))))
