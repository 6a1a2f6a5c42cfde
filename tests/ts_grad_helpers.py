"""Shared by the CPU and GPU tests of the sample-path gradient: the test-only engine (tests/ts_grad_oracle.py behind
Engine.thompson_grad_batch, on top of tests/ts_helpers.TsOracleEngine) and the host build of sin2pi of csrc/ts_device.h.  The
product never imports this file."""
import os
import subprocess
import tempfile

import numpy as np

from tests import ts_grad_oracle as tgo
from tests.ts_helpers import TsOracleEngine


class TsGradOracleEngine(TsOracleEngine):
    """TsOracleEngine + thompson_path / thompson_grad_batch by the oracle, with the library's refusals."""

    def thompson(self, S=1, F=1024, rng=None, per_draw=False, randoms=None):
        idx, mn, randoms = TsOracleEngine.thompson(self, S=S, F=F, rng=rng, per_draw=per_draw, randoms=randoms)
        self._ts = (randoms, per_draw, S, np.array(self.comp, copy=True), np.array(self.vals, copy=True),
                    np.array(self.hypers, copy=True))
        self._ts_paths = {}
        return idx, mn, randoms

    def thompson_path(self, d, s):
        if getattr(self, "_ts", None) is None:
            raise ValueError("spx_get_thompson_path: no sample paths are held (call spx_thompson first)")
        return np.array(self.paths[d, s], copy=True)

    def path_fn(self, k):
        randoms, per_draw, S, comp, vals, rows = self._ts
        if k not in self._ts_paths:
            d, s = divmod(int(k), S)
            self._ts_paths[k] = tgo.Path(self.covar, comp, vals, rows[d], randoms, s, d, per_draw)
        return self._ts_paths[k]

    def thompson_grad_batch(self, points, path_of=None, want_prior=False):
        if getattr(self, "_ts", None) is None:
            raise ValueError("spx_thompson_grad_batch: no sample paths are held (call spx_thompson first)")
        x = np.atleast_2d(np.asarray(points, dtype=np.float64))
        if x.ndim != 2 or x.shape[1] != self.comp.shape[1]:
            raise ValueError("points must be (P, D)")
        po = np.zeros(x.shape[0], dtype=np.int64) if path_of is None else np.asarray(path_of)
        f, g, pr = np.empty(x.shape[0]), np.empty(x.shape), np.empty(x.shape[0])
        for i in range(x.shape[0]):
            v, gr, p, _, _, _ = self.path_fn(po[i])(x[i:i + 1], parts=True)
            f[i], g[i], pr[i] = v[0], gr[0], p[0]
        self.calls.append(("thompson_grad_batch", x.shape[0]))
        return (f, g, pr) if want_prior else (f, g)


_client = []


def sin2pi_on_host(r):
    """sin2pi of spearmint_amd/csrc/ts_device.h compiled for the host (tests/c/ts_grad_client.cpp: a stand-alone program with
    its own main, no contraction, with the address and undefined-behaviour sanitizers) at every entry of r, run as a child
    process; None without a host C++ compiler."""
    from tests import plan_helpers as ph
    if not _client:
        cxx = ph.compiler()
        exe = None
        if cxx:
            exe = os.path.join(tempfile.mkdtemp(prefix="spx_ts_grad_client_"), "ts_grad_client")
            subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                                   os.path.join(ph.ROOT, "tests", "c", "ts_grad_client.cpp")])
        _client.append(exe)
    if _client[0] is None:
        return None
    text = "".join(float(x).hex() + "\n" for x in r)
    out = subprocess.run([_client[0]], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert all(v == "1" for v in out[1::2])           # the value does not depend on the lock-step width
    return np.array([float.fromhex(v) for v in out[0::2]])
