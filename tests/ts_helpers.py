"""Shared by the CPU and GPU tests of Thompson sampling: the test-only engine (tests/ts_oracle.py behind the Engine interface,
with the library's semantics) and the host build of csrc/ts_device.h.  The product never imports this file."""
import os
import subprocess
import tempfile

import numpy as np

from spearmint_amd import engine as spx
from tests import ts_oracle as tso
from tests.mes_helpers import MesOracleEngine


class TsOracleEngine(MesOracleEngine):
    """tests/mes_helpers.MesOracleEngine + Engine.thompson by the oracle; every other call goes through the parents' code."""

    def thompson(self, S=1, F=1024, rng=None, per_draw=False, randoms=None):
        H, N, D = self.hypers.shape[0], self.comp.shape[0], self.comp.shape[1]
        if randoms is None:
            randoms = spx.thompson_randoms(rng, self.covar, D, H, N, F, S, per_draw)
        self.paths = np.array([tso.paths(self.covar, self.comp, self.cand, self.vals, self.hypers[d], randoms, d, per_draw)
                               for d in range(H)])
        idx = np.argmin(self.paths, axis=2)
        mn = np.take_along_axis(self.paths, idx[:, :, None], axis=2)[:, :, 0]
        self.calls.append(("thompson", self.cand.shape[0], H, S, F))
        return idx.astype(np.int64), mn, randoms


_client = []


def cos2pi_on_host(r):
    """cos2pi of spearmint_amd/csrc/ts_device.h compiled for the host (tests/c/ts_client.cpp, no contraction, with the address
    and undefined-behaviour sanitizers) at every entry of r, or None without a host C++ compiler."""
    from tests import plan_helpers as ph
    if not _client:
        cxx = ph.compiler()
        exe = None
        if cxx:
            exe = os.path.join(tempfile.mkdtemp(prefix="spx_ts_client_"), "ts_client")
            subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                                   os.path.join(ph.ROOT, "tests", "c", "ts_client.cpp")])
        _client.append(exe)
    if _client[0] is None:
        return None
    text = "".join(float(x).hex() + "\n" for x in r)
    out = subprocess.run([_client[0]], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert all(v == "1" for v in out[1::2])           # the value does not depend on the lock-step width
    return np.array([float.fromhex(v) for v in out[0::2]])


# ---- acq=EI is where it was: numpy's generator after every call ----------------------------------------------------------------
EI_STATE_RUNS = [("g", "GPEIChooser", "mcmc_iters=4,acq=EI", 5, "g_seed", 0, None),
                 ("o", "GPEIOptChooser", "mcmc_iters=3,burnin=5,grid_subset=4,use_multiprocessing=0,acq=EI", 3, "o_seed", 0, None),
                 ("p", "GPEIChooser", "mcmc_iters=3,pending_samples=5,gpu_fantasies=0,acq=EI", 6, 77, 1, 300)]


def ei_state_runs(golden_dir, tmp_dir, make_engine):
    """The seeded acq=EI runs whose proposals and generator states tests/golden/ts_ei_states.npz records (written by
    write_ei_states below on the commit BEFORE acq=TS existed, through tests/mes_helpers.MesOracleEngine): name ->
    (proposal indices, the 624 key words of numpy's generator after every call, pos, has_gauss, cached_gaussian)."""
    import importlib
    from tests.mes_helpers import branin_sequence
    g = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))
    out = {}
    for name, mod, arg, iters, seed, n_pend, rows in EI_STATE_RUNS:
        d = os.path.join(str(tmp_dir), "ei_state_" + name)
        os.makedirs(d)
        grid = g["grid"] if rows is None else g["grid"][:rows]
        runs = branin_sequence(importlib.import_module("spearmint_amd.chooser." + mod), arg, d, grid, iters, int(g[seed]) if isinstance(seed, str) else seed,
                               make_engine, n_pending=n_pend)
        out[name + "_idx"] = np.array([r[0] for r in runs], dtype=np.int64)
        out[name + "_key"] = np.array([r[2][1] for r in runs], dtype=np.uint32)
        out[name + "_pos"] = np.array([r[2][2] for r in runs], dtype=np.int64)
        out[name + "_has_gauss"] = np.array([r[2][3] for r in runs], dtype=np.int64)
        out[name + "_gauss"] = np.array([r[2][4] for r in runs], dtype=np.float64)
    return out


def write_ei_states(path):
    from tests.mes_helpers import MesOracleEngine
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    np.savez_compressed(path, **ei_state_runs(golden, tempfile.mkdtemp(prefix="spx_ei_states_"), MesOracleEngine))
