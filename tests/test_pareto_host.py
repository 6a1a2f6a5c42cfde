"""Two objectives without a GPU: the host helpers of spearmint_amd/pareto.py, the argument checks of the C ABI that are
decided before any device is touched, what the held record does with the new items, GPParetoChooser's arguments and whole
next() calls on an oracle-backed engine (tests/ehvi_helpers.py), and csrc/ehvi_device.h compiled for the host."""
import os

import numpy as np
import numpy.random as npr
import pytest

from spearmint_amd import engine
from spearmint_amd import pareto
from spearmint_amd.chooser import GPEIperSecChooser, GPParetoChooser
from tests import ehvi_helpers as eh
from tests import ehvi_mp as em
from tests import ehvi_oracle as eo
from tests import plan_helpers as ph
from tests.helpers import OracleEngine


# ---- spearmint_amd/pareto.py ------------------------------------------------------------------------------------------------
def _dominated(i, v1, v2):
    return np.any((v1 <= v1[i]) & (v2 <= v2[i]) & ((v1 < v1[i]) | (v2 < v2[i])))


def test_front_extraction():
    rng = np.random.RandomState(5)
    v1, v2 = np.round(rng.rand(60) * 8) / 8, np.round(rng.rand(60) * 8) / 8          # many ties in either objective
    v1[10], v2[10] = v1[3], v2[3]                                                   # an exact duplicate
    idx = pareto.pareto_front(v1, v2)
    assert np.all(np.diff(v1[idx]) > 0) and np.all(np.diff(v2[idx]) < 0)            # the engine's order, strictly
    want = {(v1[i], v2[i]) for i in range(60) if not _dominated(i, v1, v2)}
    assert {(v1[i], v2[i]) for i in idx} == want and len(idx) == len(want)          # one survivor per duplicate
    first = {p: min(i for i in range(60) if (v1[i], v2[i]) == p) for p in want}
    assert sorted(idx) == sorted(first.values())                                    # ... the first of them
    # all dominated by one point; a single point; nothing; ties along one objective; non-finite points take no part
    assert list(pareto.pareto_front([1.0, 0.0, 2.0], [1.0, 0.0, 3.0])) == [1]
    assert list(pareto.pareto_front([4.0], [2.0])) == [0] and pareto.pareto_front([], []).shape == (0,)
    assert list(pareto.pareto_front([1.0, 1.0, 1.0], [3.0, 2.0, 2.5])) == [1]
    assert list(pareto.pareto_front([3.0, 2.0, 2.5], [1.0, 1.0, 1.0])) == [1]
    assert list(pareto.pareto_front([0.0, np.nan, 1.0, -np.inf], [1.0, 0.0, 0.0, 5.0])) == [0, 2]
    with pytest.raises(ValueError):
        pareto.pareto_front([1.0, 2.0], [1.0])


def test_reference_point_rule():
    assert pareto.reference_point([1.0, 3.0, 2.0], [-4.0, -4.0, -4.0]) == (3.0 + 0.1 * 2.0, -3.0)
    assert pareto.reference_point([5.0], [7.0]) == (6.0, 8.0)
    for bad in ([], [1.0, np.nan]):
        with pytest.raises(ValueError):
            pareto.reference_point(bad, bad)


def test_hypervolume_against_a_grid_count():
    rng = np.random.RandomState(9)
    v1, v2 = rng.rand(30), rng.rand(30)
    idx = pareto.pareto_front(v1, v2)
    front, ref = np.stack((v1[idx], v2[idx]), axis=1), (1.25, 1.5)
    hv = pareto.dominated_hypervolume(front, ref)
    n = 1500                                                                        # cell midpoints of an n x n raster of the box
    x = (np.arange(n) + 0.5) / n * ref[0]
    y = (np.arange(n) + 0.5) / n * ref[1]
    covered = np.zeros((n, n), dtype=bool)
    for a, b in front:
        covered |= (x[:, None] >= a) & (y[None, :] >= b)
    count = covered.sum() * (ref[0] / n) * (ref[1] / n)
    assert abs(hv - count) <= 2.0 * (len(idx) + 1) * max(ref) / n                   # a staircase of 2 (n + 1) segments, one cell wide
    assert pareto.dominated_hypervolume(np.zeros((0, 2)), ref) == 0.0
    assert pareto.dominated_hypervolume([[0.25, 0.5]], (1.25, 1.5)) == 1.0
    for bad in ([[0.0, 1.0], [0.0, 0.5]], [[0.0, 1.0], [1.0, 1.0]], [[2.0, 0.0]]):
        with pytest.raises(ValueError):
            pareto.dominated_hypervolume(bad, ref)
    # EHVI of a certain point is the hypervolume it adds
    a, b = front[:, 0], front[:, 1]
    u, v = 0.3, 0.2
    both = pareto.pareto_front(np.append(a, u), np.append(b, v))
    added = pareto.dominated_hypervolume(np.stack((np.append(a, u)[both], np.append(b, v)[both]), axis=1), ref) - hv
    assert abs(float(eo.improvement(u, v, a, b, *ref)) - added) < 1e-14
    assert abs(float(eo.ehvi(np.array([u]), np.array([1e-24]), np.array([v]), np.array([1e-24]), a, b, *ref)[0]) - added) < 1e-12


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------
def test_front_and_acquisition_argument_checks_touch_no_gpu():
    eng = engine.Engine(0)
    assert eng.get_pareto_front() is None
    for par in (1.0, 0.5, float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            eng.set_acquisition(engine.ACQ_EHVI, par)
        assert eng.get_acquisition() == (engine.ACQ_EI, 0.0)
    eng.set_acquisition("EHVI")
    assert eng.get_acquisition() == (engine.ACQ_EHVI, 0.0)
    good = np.array([[0.0, 2.0], [1.0, 1.0], [2.0, 0.0]])
    bad = [(good[::-1], (3.0, 3.0)),                                   # a decreasing / b increasing
           ([[0.0, 2.0], [0.0, 1.0]], (3.0, 3.0)), ([[0.0, 2.0], [1.0, 2.0]], (3.0, 3.0)),      # not strict
           (good, (2.0, 3.0)), (good, (3.0, 2.0)), (good, (1.5, 3.0)),                          # a_n >= r1 / b_1 >= r2
           ([[0.0, np.nan]], (3.0, 3.0)), ([[np.inf, 0.0]], (3.0, 3.0)), (good, (np.nan, 3.0)), (good, (3.0, np.inf)),
           (np.stack((np.arange(4097.0), -np.arange(4097.0)), axis=1), (5000.0, 1.0))]          # n out of range
    for front, ref in bad:
        with pytest.raises(ValueError) as ei:
            eng.set_pareto_front(front, ref)
        assert "spx_set_pareto_front" in str(ei.value)
        assert eng.get_pareto_front() is None
    eng.set_pareto_front(None, None)                                   # clearing what is not set is not an error
    # EHVI refuses the refinement entry points and a pass without its model, all from the host's record
    for call in (lambda: eng.ei_grad_batch(np.zeros((1, 2))), lambda: eng.ei_run(), lambda: eng.ei_step()):
        with pytest.raises(ValueError):
            call()
    eng.close()


def test_held_record_of_the_new_items():
    if ph.client("held_client") is None:
        pytest.skip("no host C++ compiler")
    T = {n: i for i, n in enumerate(["OBS", "CAND", "HYP", "TIME", "CON", "FACTOR", "CON_FACTOR", "FULL_FACTOR", "FANT", "ALPHA_S",
                                      "RESULTS", "COVAR", "PARTITION", "FRONT", "SEC", "SEC_CAND"])}

    def bits(*names):
        return sum(1 << T[n] for n in names)

    def ask(b, op, thing):
        got = ph.ask("held_client", "%d 0 %s %d 0\n" % (b, op, T[thing]))[0].split()
        return int(got[0]), int(got[2])
    full = bits("OBS", "CAND", "HYP", "TIME", "FACTOR", "RESULTS", "FRONT", "SEC", "SEC_CAND")
    assert ask(full, "drop", "FRONT") == (full & ~bits("FRONT", "RESULTS"), 1)                 # a new front: the results alone
    assert ask(full, "drop", "CAND") == (full & ~bits("CAND", "RESULTS", "SEC_CAND"), 1)
    assert ask(full, "drop", "TIME") == (full & ~bits("TIME", "FACTOR", "RESULTS", "SEC"), 1)
    assert ask(full, "drop", "HYP") == (bits("OBS", "CAND", "FRONT", "SEC_CAND"), 1)
    assert ask(full, "drop", "COVAR") == (full & ~bits("FACTOR", "RESULTS"), 1)                # (the internal handle drops its own factor)
    assert ask(bits("OBS", "HYP"), "set", "SEC") == (bits("OBS", "HYP"), 0)                    # no second model to copy
    assert ask(bits("OBS", "HYP", "TIME"), "set", "SEC") == (bits("OBS", "HYP", "TIME", "SEC"), 1)
    assert ask(0, "set", "SEC_CAND") == (0, 0) and ask(0, "set", "FRONT") == (bits("FRONT"), 1)


# ---- the chooser ----------------------------------------------------------------------------------------------------------------
def test_chooser_argument_errors(tmp_path):
    d = str(tmp_path)
    for kw in ({"acq": "EI"}, {"acq": "PI"}, {"acq_par": 1}, {"recommend": 1}, {"importance": 1}, {"loo": 1}, {"ndev": 2},
               {"ref1": "high"}, {"ref2": "nan"}, {"ref1": "inf"}, {"ref_compat": 1}):
        with pytest.raises(ValueError):
            GPParetoChooser.GPParetoChooser(d, **kw)
    ch = GPParetoChooser.init(d, "ref1=2.5,ref2=auto,mcmc_iters=3")
    assert ch.ref1 == 2.5 and ch.ref2 is None and ch.mcmc_iters == 3
    grid = np.random.RandomState(0).rand(10, 2)
    vals, durs = np.arange(10.0), np.ones(10)
    assert ch.next(grid, vals, durs, np.arange(1, 10), np.zeros(0, int), np.arange(1)) == 1     # too little data: no model yet
    for bad in (0.0, -1.0, np.nan):
        durs2 = durs.copy()
        durs2[1] = bad
        with pytest.raises(ValueError):
            ch.next(grid, vals, durs2, np.arange(3, 10), np.zeros(0, int), np.arange(3))
    import importlib.util
    spec = importlib.util.spec_from_file_location("chooser_GPParetoChooser_shim", os.path.join(ph.ROOT, "dropin", "chooser",
                                                                                                "GPParetoChooser.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    assert isinstance(shim.init(d, "mcmc_iters=2"), GPParetoChooser.GPParetoChooser)


@pytest.fixture(scope="module")
def toy_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("pareto_toy")
    return eh.pareto_sequence(lambda: GPParetoChooser.GPParetoChooser(str(d), mcmc_iters=3, burnin=3), eh.EhviOracleEngine, iters=4,
                              pending_at=(2,))


def test_next_proposes_the_oracles_argmax(toy_run):
    assert [len(r["pending"]) for r in toy_run] == [0, 0, 2, 0]
    for r in toy_run:
        grid, complete, cand, pend = r["grid"], r["complete"], r["cand"], r["pending"]
        vals, ldurs = r["values"][complete], np.log(r["durations"][complete])
        rows, trows = r["rows"]
        lp = r["last_pareto"]
        idx = pareto.pareto_front(vals, ldurs)
        ref = pareto.reference_point(vals, ldurs)
        assert np.array_equal(lp["front_index"], complete[idx]) and lp["ref"] == ref       # completed jobs only
        assert np.array_equal(lp["front"], np.stack((vals[idx], ldurs[idx]), axis=1))
        assert lp["hypervolume"] == pareto.dominated_hypervolume(lp["front"], ref)
        a, b = lp["front"][:, 0], lp["front"][:, 1]
        comp = grid[complete]
        if len(pend):      # the believer rule: np.mean over the draws of both GPs' func_m at the pending rows
            _, mom = eo.over_hypers(comp, grid[pend], vals, ldurs, rows, trows, a, b, ref[0], ref[1], want_moments=True)
            comp = np.concatenate((comp, grid[pend]))
            vals = np.concatenate((vals, np.mean(np.array([m[0] for m in mom]), axis=0)))
            ldurs = np.concatenate((ldurs, np.mean(np.array([m[2] for m in mom]), axis=0)))
        mean = np.mean(eo.over_hypers(comp, grid[cand], vals, ldurs, rows, trows, a, b, ref[0], ref[1]), axis=1)
        assert r["job"] == int(cand[int(np.argmax(mean))])
        assert r["engine"].calls[-1] == ("ehvi_grid", len(cand), 3, len(complete) + len(pend))
        assert r["job"] not in pend


def test_pareto_txt_is_well_formed(toy_run):
    for r in toy_run:
        lines = r["text"].splitlines()
        lp = r["last_pareto"]
        head = lines[0].split()
        assert head[0] == "#" and head[1] == "completed=%d" % len(r["complete"]) and head[2] == "front=%d" % len(lp["front_index"])
        assert head[3] == "ref=%.17g" % lp["ref"][0] and float(head[4]) == lp["ref"][1]
        assert head[5] == "hypervolume=%.17g" % lp["hypervolume"] and len(lines) == 1 + len(lp["front_index"])
        rows = [ln.split() for ln in lines[1:]]
        assert [int(x[0]) for x in rows] == list(lp["front_index"])
        assert [float(x[1]) for x in rows] == list(lp["front"][:, 0]) == sorted(lp["front"][:, 0])      # in order of value
        assert [float(x[2]) for x in rows] == [r["durations"][i] for i in lp["front_index"]]            # seconds, every digit


def test_generator_state_is_what_the_per_second_chooser_leaves(toy_run, tmp_path):
    """Same seed, same completed jobs, all three from a fresh state: GPEIperSecChooser's own next() (no pending jobs) leaves
    numpy's generator where GPParetoChooser leaves it, with or without pending jobs -- the believer rule draws nothing -- and
    the two choosers sampled the same hyper chains."""
    r = toy_run[2]
    free = np.sort(np.concatenate((r["pending"], r["cand"])).astype(int))
    none = np.zeros(0, dtype=int)
    got = []
    for name, cls, eng, cand, pend in (("persec", GPEIperSecChooser.GPEIperSecChooser, OracleEngine, free, none),
                                       ("plain", GPParetoChooser.GPParetoChooser, eh.EhviOracleEngine, free, none),
                                       ("pending", GPParetoChooser.GPParetoChooser, eh.EhviOracleEngine, r["cand"], r["pending"])):
        d = tmp_path / name
        d.mkdir()
        ch = cls(str(d), mcmc_iters=3, burnin=3, grid_subset=1)
        ch._eng = eng()
        npr.seed(77)
        ch.next(r["grid"], r["values"], r["durations"], cand, pend, r["complete"])
        got.append((npr.get_state(), ch._paired_samples()))
    assert len(r["pending"]) == 2
    for state, rows in got[1:]:
        assert eh.same_rng_state(state, got[0][0])
        assert np.array_equal(rows[0], got[0][1][0]) and np.array_equal(rows[1], got[0][1][1])


# ---- the device header's own text on the host -----------------------------------------------------------------------------------
@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_device_header_on_the_host_equals_the_oracle(golden_dir):
    """csrc/ehvi_device.h compiled for the host against tests/ehvi_oracle.py on the golden vectors.  The two are the same text
    over two libraries' erf / erfc / exp (glibc against scipy's cephes ndtr and numpy's exp), so the bar is the one the device
    is held to: four times the oracle's pinned error against the 50-digit values per band, in the units of tests/ehvi_mp.scale,
    both for the difference between the two and for the header's own error against the 50-digit values.  Measured: 127 of the
    204 candidates differ from the oracle in some bit; the worst difference per band is n0 0.79, n1 0.30, n2 0.63, n7 0.57, ulp
    0.16, place 0.40, n4096 0.007 units (bars 5.3, 4, 5.2, 4, 4, 4, 4), and the header's own worst error against the 50-digit
    values n0 1.32, n1 0.82, n2 1.29, n7 0.56, ulp 0.93, place 0.99, n4096 0.017.  Order of operations, tiling (the n4096 band
    crosses 17 tiles) and NaN rule carry over."""
    fx = dict(np.load(os.path.join(golden_dir, "ehvi_mp.npz")))
    for band in em.BANDS:
        m1, v1, m2, v2 = (fx[band + k] for k in ("_m1", "_v1", "_m2", "_v2"))
        edges, levels = eo.strips(fx[band + "_a"], fx[band + "_b"], *fx[band + "_ref"])
        got = eh.device_header_on_host(edges, levels, m1, v1, m2, v2)
        want = eo.ehvi(m1, v1, m2, v2, fx[band + "_a"], fx[band + "_b"], *fx[band + "_ref"])
        bar = 4.0 * em.pinned(fx, band)
        diff = em.error(got, want, fx[band + "_scale"])
        e = em.error(got, fx[band + "_ehvi"], fx[band + "_scale"])
        print("ehvi_device.h on the host, %s: %d of %d differ from the oracle, worst %.3g units; against 50 digits %.3g (bar %.3g)"
              % (band, int(np.sum(got != want)), len(got), diff, e, bar))
        assert diff <= bar and e <= bar, (band, diff, e, bar)
    # func_v < 0 in either GP: NaN; no front: the product, sign of zero included
    got = eh.device_header_on_host([0.5], [0.25], [0.0, 0.0, 0.1], [-1.0, 1.0, 0.04], [0.0, 0.0, -0.3], [1.0, -1.0, 0.09])
    assert np.isnan(got[0]) and np.isnan(got[1])
    assert got[2] == eo.g(0.1, 0.04, 0.5) * eo.g(-0.3, 0.09, 0.25) or abs(got[2] / (eo.g(0.1, 0.04, 0.5) * eo.g(-0.3, 0.09, 0.25)) - 1) < 8 * em.U


# ---- scripts/time_ehvi.py as far as a CPU takes it ---------------------------------------------------------------------------------
def test_time_script_arguments_and_no_device():
    import subprocess
    import sys

    def run(*args):
        return subprocess.run([sys.executable, os.path.join(ph.ROOT, "scripts", "time_ehvi.py")] + list(args), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, timeout=120)
    assert run("--shapes", "c9").returncode == 2 and run("--fronts", "5000").returncode == 2 and run("--fronts", "x").returncode == 2
    if engine.device_count() > 0:
        return
    r = run("--child", "--shapes", "small", "--fronts", "2")
    assert r.returncode == 2 and b"no usable HIP device" in r.stderr and r.stdout == b""
