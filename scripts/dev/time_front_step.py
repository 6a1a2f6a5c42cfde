"""Dev: wall time of one spx_ei_step on the front of a two-slot multi-device handle (MultiEngine([0, 0])), two builds of the
library in ONE process, interleaved: 15 rounds, in each the median of STEPS steps per engine.  The first library is loaded
for two engines, so that its own run-to-run spread (engine against engine, round against round) is measured in the same
session; a median of the second library inside that spread is no slower and no faster than can be told here
(profiles/multi_held_time.log).
   python scripts/dev/time_front_step.py PARENT_LIB CHILD_LIB|- [abc|cab|...]     (- : the in-tree library; the order in which the
                                                                           engines parent a, parent b, child are created)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from spearmint_amd.engine import MultiEngine  # noqa: E402
from spearmint_amd.synthetic import synthetic_problem  # noqa: E402

ROUNDS = 15
SHAPES = [("held_helpers", 70, 130, 2, 2, 200), ("N=256 M=20000 H=10", 256, 20000, 8, 10, 40)]      # name, N, M, D, H, steps a round


def main(parent, child, order="abc"):
    libs = {"a": ("parent a", parent), "b": ("parent b", parent), "c": ("child", None if child == "-" else child)}
    libs = [libs[k] for k in order]     # the order in which the engines are created: it shows (the first is the fastest)
    print("engines created in the order: " + ", ".join(label for label, _ in libs))
    for name, N, M, D, H, steps in SHAPES:
        comp, cand, vals, hypers = synthetic_problem(N, M, D, H, 7)
        engines = []
        for label, lib in libs:
            e = MultiEngine([0, 0], lib=lib)
            e.set_observations(comp, vals)
            e.set_candidates(cand)
            e.set_hypers(hypers)
            for _ in range(steps):              # warm
                e.ei_step(0)
            engines.append((label, e))
        med = {label: [] for label, _ in engines}
        for r in range(ROUNDS):
            for label, e in engines[r % 3:] + engines[:r % 3]:       # (no engine always first)
                ts = []
                for _ in range(steps):
                    t = time.perf_counter()
                    e.ei_step(0)
                    ts.append(time.perf_counter() - t)
                med[label].append(np.median(ts) * 1e6)
        best = [e.best() for _, e in engines]
        assert best[0] == best[1] == best[2], best
        for _, e in engines:
            e.close()
        par = np.array(med["parent a"] + med["parent b"])
        ch = np.array(med["child"])
        print("== %s: %d rounds x median of %d ei_step, us" % (name, ROUNDS, steps))
        for label in med:
            print("  %-9s %s   median %.1f" % (label, " ".join("%.1f" % v for v in med[label]), np.median(med[label])))
        inside = int(((ch >= par.min()) & (ch <= par.max())).sum())
        print("  parent against parent: %.1f .. %.1f us (spread %.1f %% of its median %.1f); child medians inside: %d of %d; "
              "child median of medians %.1f (%+.2f %% against the parent's)" % (
                  par.min(), par.max(), 100 * (par.max() - par.min()) / np.median(par), np.median(par), inside, ROUNDS,
                  np.median(ch), 100 * (np.median(ch) / np.median(par) - 1)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
