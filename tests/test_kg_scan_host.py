"""Option "kg_scan" without a GPU: csrc/kg_fant_device.h with 16-bit line indices (tests/c/kgs_client.cpp) on the crafted line sets
of tests/kg_mp.py repeated out to n = 257 and 1024, at the plain header's bar against 50 digits; the library's argument checks; the
choosers' arguments and the `observed` representer rule on the oracle engine.  GPU: tests/test_gpu_zy_kg_scan.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from spearmint_amd import engine
from spearmint_amd.chooser import GPEIChooser, GPEIOptChooser
from tests import kg_helpers as kh
from tests import kg_mp as km
from tests import kg_oracle as ko
from tests import plan_helpers as ph
from tests.helpers import branin


def scan_on_host(sets):
    """(values, [line indices by rank]) of every (mu, b) from kg_fant_device.h's KgsLines on the host."""
    exe = os.path.join(tempfile.mkdtemp(prefix="spx_kgs_client_"), "kgs_client")
    subprocess.check_call([ph.compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ph.ROOT, "tests", "c", "kgs_client.cpp")])
    text = []
    for mu, b in sets:
        text.append("%d\n" % len(mu))
        text += ["%s %s\n" % (float(m).hex(), float(s).hex()) for m, s in zip(mu, b)]
    rows = subprocess.run([exe], input="".join(text).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    rows = [r.split() for r in rows]
    return np.array([float.fromhex(r[0]) for r in rows]), [np.array(r[1:], dtype=int) for r in rows]


@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_scan_with_16_bit_indices_against_50_digits(golden_dir):
    """A repeated line is a duplicate: off the envelope by the tie rule, so the yardstick of the long set is that of the crafted
    one and every rank from 256 up -- the second byte of an index, the last word of the bit set -- carries a line."""
    fx = dict(np.load(os.path.join(golden_dir, "kg_mp.npz")))
    named = km.sets_of(fx)
    sets = [(np.resize(mu, n), np.resize(b, n)) for n in (257, 1024) for _, mu, b in named]
    got, perms = scan_on_host(sets)
    kh.held_to_yardstick(fx, got, sets, "KgsLines on the host, n = 257 and 1024")
    for k, (mu, b) in enumerate(sets):
        assert np.array_equal(perms[k], np.lexsort((np.arange(len(b)), -np.asarray(b)))), k
    assert np.all(got >= 0.0) and not np.any(np.signbit(got))
    for n, off in ((257, 0), (1024, len(named))):
        for k, (name, _, _) in enumerate(named):
            if name in ("equal_slopes", "equal_slopes_zero", "rand_n1_0", "far_40"):
                assert got[off + k] == 0.0, (n, name)                                  # exactly +0.0
    # every line on the envelope, n = 1024: the stack at its deepest, all 32 words of the bit set full
    k = np.arange(1024.0)
    deep, _ = scan_on_host([(k ** 2 / 1024.0, -k)])
    kh.held_to_yardstick(fx, deep, [(k ** 2 / 1024.0, -k)], "1024 lines on the envelope")


def test_library_argument_checks_touch_no_gpu():
    eng = engine.Engine(0)
    assert engine.KG_SCAN_MAX_POINTS == 1023
    for bad in (2, -1):
        with pytest.raises(ValueError, match="kg_scan"):
            eng.set_option("kg_scan", bad)
    with pytest.raises(ValueError, match="unknown option 'lean_flwo'"):
        eng.set_option("lean_flwo", 1)
    assert eng.stat("last_kg_scan") == 0
    lib, h, pts = eng._lib, eng._h, np.zeros((1024, 2))
    err = lambda: lib.spx_last_error().decode()
    assert lib.spx_set_kg_points(h, engine._dp(pts), 256) == engine.SPX_ERR_ARG and "1 .. 255" in err()
    eng.set_option("kg_scan", 1)
    assert lib.spx_set_kg_points(h, engine._dp(pts), 1024) == engine.SPX_ERR_ARG and "1 .. 1023" in err()
    assert lib.spx_set_kg_points(h, engine._dp(pts), 0) == engine.SPX_ERR_ARG and "1 .. 1023" in err()
    assert lib.spx_set_kg_points(h, engine._dp(pts), 256) == engine.SPX_ERR_ARG and "dimension" in err()    # (in range: D is unknown)
    eng.close()


@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_arguments(mod, tmp_path):
    ch = mod.init(str(tmp_path), "acq=KG,kg_scan=1,acq_par=1023,kg_points=observed")
    assert (ch.kg_scan, ch.acq_par, ch.kg_points) == (1, 1023.0, "observed")
    assert (mod.init(str(tmp_path), "acq=KG").kg_scan, mod.init(str(tmp_path), "acq=KG").kg_points) == (0, "grid")
    for args, word in (("acq=EI,kg_scan=1", "kg_scan"), ("acq=KG,kg_points=observed", "kg_scan=1"), ("acq=KG,kg_scan=2", "kg_scan"),
                       ("acq=KG,kg_scan=1,kg_points=best", "kg_points"), ("acq=KG,kg_scan=1,acq_par=1024", "1 .. 1023"),
                       ("acq=KG,acq_par=256", "1 .. 255"), ("acq=KG,kg_scan=1,acq_par=256,kg_pending=1", "kg_pending")):
        with pytest.raises(ValueError) as ei:
            mod.init(str(tmp_path), args)
        assert "allowed" in str(ei.value) and word in str(ei.value), args


def test_observed_points_are_the_completed_points_in_order(golden_dir, tmp_path):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:150]
    values = np.full(grid.shape[0], np.nan)
    done = np.array([7, 2, 11, 0, 5, 3])                   # the order of `complete` is the order of the points
    values[done] = branin(grid[done, 0], grid[done, 1])
    cand = np.setdiff1d(np.arange(grid.shape[0]), done)

    class Eng(kh.make_oracle_engine()):
        def set_option(self, name, value):
            self.calls.append(("set_option", name, value))
    out = {}
    for name, extra in (("obs", ",kg_scan=1,kg_points=observed"), ("grid1", ",kg_scan=1"), ("grid0", "")):
        (tmp_path / name).mkdir()
        ch = GPEIChooser.init(str(tmp_path / name), "mcmc_iters=2,acq=KG,acq_par=5" + extra)
        eng = ch._eng = Eng()
        np.random.seed(5)
        job = ch.next(grid, values, np.full(grid.shape[0], np.nan), cand, np.zeros(0, dtype=int), done)
        out[name] = (job, ch.last_kg, eng, np.random.get_state())
    job, lk, eng, _ = out["obs"]
    assert np.array_equal(lk["points"], grid[done]) and np.array_equal(lk["points_index"], np.arange(6))
    assert ("set_option", "kg_scan", 1) in eng.calls and not [c for c in out["grid0"][2].calls if c[0] == "set_option"]
    from oracle import gp_ei_oracle as orc
    with orc.covar("Matern52"):
        val = np.mean(ko.over_hypers(grid[done], grid[cand], values[done], grid[done], eng.hypers), axis=1)
    assert job == cand[int(np.argmax(val))] and lk["value"] == float(np.max(val))
    # kg_points=grid: today's rule, and today's proposal and generator state with the option on or off
    assert out["grid1"][0] == out["grid0"][0] and np.array_equal(out["grid1"][1]["points_index"], out["grid0"][1]["points_index"])
    assert all(np.array_equal(a, b) for a, b in zip(out["grid1"][3], out["grid0"][3]))
