"""Shared by tests/test_kg_host.py (CPU) and tests/test_gpu_zv_kg.py: csrc/kg_device.h compiled for the host, the bars against the
50-digit yardstick, and KgOracleEngine -- what the choosers need of an engine under acq=KG, computed by numpy."""
import os
import subprocess
import tempfile

import numpy as np

from tests import kg_mp as km
from tests import kg_oracle as ko

MARGIN = 4.0          # the project's margin over the oracle's pinned error, everywhere
_client = []


def device_header_on_host(sets):
    """The knowledge gradient of every (mu, b) of `sets` from spearmint_amd/csrc/kg_device.h compiled for the host
    (tests/c/kg_client.cpp, no contraction, with the address and undefined-behaviour sanitizers), or None without a compiler."""
    from tests import plan_helpers as ph
    if not _client:
        cxx = ph.compiler()
        exe = None
        if cxx:
            exe = os.path.join(tempfile.mkdtemp(prefix="spx_kg_client_"), "kg_client")
            subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                                   os.path.join(ph.ROOT, "tests", "c", "kg_client.cpp")])
        _client.append(exe)
    if _client[0] is None:
        return None
    text = []
    for mu, b in sets:
        text.append("%d\n" % len(mu))
        text += ["%s %s\n" % (float(m).hex(), float(s).hex()) for m, s in zip(mu, b)]
    out = subprocess.run([_client[0]], input="".join(text).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split()
    return np.array([float.fromhex(v) for v in out])


def yardstick(mu, b):
    """(value, unit, band) of one line set at 50 digits, as float64."""
    v, u, z = km.kg_mp(mu, b)
    return float(v), float(u), km.band_of(float(z))


def held_to_yardstick(fx, got, sets, what):
    """Every value of `got` against the 50-digit value of its set at MARGIN x the oracle's pinned error of the set's band;
    prints the worst error per band first.  sets: [(mu, b)]."""
    worst = {}
    bad = []
    for k, (mu, b) in enumerate(sets):
        if not (np.all(np.isfinite(mu)) and np.all(np.isfinite(b))):
            if not np.isnan(got[k]):
                bad.append((k, "not NaN"))
            continue
        v, u, band = yardstick(mu, b)
        e = km.error(np.array([got[k]]), np.array([v]), np.array([u]))
        worst[band] = max(worst.get(band, 0.0), e)
        if not e <= MARGIN * km.pinned(fx, band):
            bad.append((k, band, e, got[k], v))
    for band in sorted(worst):
        print("%s, %s: worst error %.3g units (bar %.3g)" % (what, band, worst[band], MARGIN * km.pinned(fx, band)))
    assert not bad, (what, bad[:5])
    return worst


def choose_points(mean_over_draws, A):
    """Indices of the A rows with the lowest mean, stable, NaN rows skipped, fewer if fewer exist."""
    m = np.asarray(mean_over_draws, dtype=np.float64)
    order = np.argsort(m, kind="stable")
    order = order[~np.isnan(m[order])]
    return order[:A]


KG = 5      # include/spx.h SPX_ACQ_KG


def make_oracle_engine():
    """KgOracleEngine: tests/acq_helpers.AcqOracleEngine + SPX_ACQ_KG with the library's semantics -- points are a setting, KG
    is refused without them and over fantasies; every other acquisition goes through the parent's code untouched."""
    from oracle import gp_ei_oracle as orc
    from tests.acq_helpers import AcqOracleEngine

    class KgOracleEngine(AcqOracleEngine):
        def __init__(self, covar="Matern52"):
            AcqOracleEngine.__init__(self, covar)
            self.kg_points = None

        def set_kg_points(self, points):
            self.kg_points = None if points is None else np.array(points, dtype=float)
            self.calls.append(("set_kg_points", 0 if points is None else len(points)))

        def get_kg_points(self):
            return self.kg_points

        def ei_run(self, flags=0):
            if self.acq[0] != KG:
                return AcqOracleEngine.ei_run(self, flags)
            if self.kg_points is None:
                raise ValueError("spx_ei_run: SPX_ACQ_KG needs representer points (spx_set_kg_points)")
            if self.fant is not None:
                raise ValueError("spx_ei_run: SPX_ACQ_KG is not defined over fantasies")
            with orc.covar(self.covar):
                self._ei = ko.over_hypers(self.comp, self.cand, self.vals, self.kg_points, self.hypers)
            self.calls.append(("ei_run", self.cand.shape[0], self.hypers.shape[0], None))

        def ei_grad_batch(self, points):
            if self.acq[0] == KG:
                raise ValueError("spx_ei_grad_batch: not defined under SPX_ACQ_KG")
            return AcqOracleEngine.ei_grad_batch(self, points)
    return KgOracleEngine
