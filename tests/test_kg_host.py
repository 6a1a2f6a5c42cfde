"""The knowledge gradient without a GPU: the float64 oracle (tests/kg_oracle.py) against quadrature of E[min] and against its
50-digit yardstick (tests/kg_mp.py, committed as tests/golden/kg_mp.npz); csrc/kg_device.h compiled for the host on the crafted
line sets, held to the yardstick at four times the oracle's pinned error per band; the argument checks of the C ABI (decided
before any device is touched); the choosers' arguments and refusals; a seeded Branin sequence through an oracle engine; and
the new thing's row of the held-state table.  The GPU side is tests/test_gpu_zv_kg.py."""
import os

import numpy as np
import pytest

from spearmint_amd import engine
from spearmint_amd.chooser import GPConstrainedEIChooser, GPEIChooser, GPEIOptChooser, GPEIperSecChooser, GPParetoChooser
from tests import kg_helpers as kh
from tests import kg_mp as km
from tests import kg_oracle as ko
from tests import plan_helpers as ph
from tests.acq_helpers import AcqStandinEngine
from tests.mes_helpers import branin_sequence, same_state


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "kg_mp.npz")))


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_quadrature_of_e_min():
    """n = 1 .. 40 random line sets, equal slopes included: the sum over the envelope against Simpson's rule on E[min] itself.
    The bar is the quadrature's own error: h^2 = (24 / 2^18)^2 = 8.4e-9 times the slope jumps at the kinks (their sum is at
    most max b - min b) / 12, a factor 4 over it."""
    rng = np.random.RandomState(11)
    worst = 0.0
    for n in range(1, 41):
        mu, b = rng.randn(n), rng.randn(n)
        if n % 5 == 0:
            b[n // 2:] = b[0]                      # a block of equal slopes
        got = ko.value(mu, b)
        want = float(np.min(mu)) - ko.e_min_quadrature(mu, b)
        bar = 4.0 * (24.0 / (1 << 18)) ** 2 * (np.max(b) - np.min(b) + 1.0) / 12.0 + 1e-13
        worst = max(worst, abs(got - want) / bar)
        assert abs(got - want) <= bar, (n, got, want)
    print("oracle against quadrature: worst error %.3g of the quadrature's bar" % worst)


def test_fixture_holds_the_generators_cases(fx):
    cs = km.cases()
    sets = km.sets_of(fx)
    assert [c[0] for c in cs] == [s[0] for s in sets]
    for (_, mu, b), (_, fmu, fb) in zip(cs, sets):
        assert np.array_equal(mu, fmu) and np.array_equal(b, fb)
    # a few sets go through mpmath again here: the stored values are what the generator gives
    for k in (0, 5, 30, len(cs) - 1):
        v, u, z = km.kg_mp(cs[k][1], cs[k][2])
        assert float(v) == fx["kg"][k] and float(u) == fx["unit"][k] and float(z) == fx["zmax"][k]
    assert sorted(set(fx["n"])) == list(km.SIZES[:3]) + [4, 5, 6] + list(km.SIZES[3:])
    assert max(km.FAR) >= 38.6 and np.max(fx["zmax"]) > 38.0
    for band in km.BANDS:
        assert np.sum([km.band_of(z) == band for z in fx["zmax"]]) >= 5, band


def test_float64_oracle_error_per_band(fx):
    sets = km.sets_of(fx)
    got = np.array([ko.value(mu, b) for _, mu, b in sets])
    bands = np.array([km.band_of(z) for z in fx["zmax"]])
    for band in km.BANDS:
        sel = bands == band
        e = km.error(got[sel], fx["kg"][sel], fx["unit"][sel])
        print("float64 oracle, %s: worst error %.3g units (pinned %.3g)" % (band, e, km.pinned(fx, band)))
        assert e <= km.pinned(fx, band), (band, e)
    assert np.all(got >= 0.0) and not np.any(np.signbit(got))


# ---- the device header's own text on the host --------------------------------------------------------------------------------
@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_device_header_against_50_digits(fx):
    """csrc/kg_device.h compiled for the host on every crafted set -- n = 1, 2, 3, 16, 17, 64, 65, 256; equal slopes; duplicates;
    parallel lines; three and five lines through one point; slopes one ulp apart; breakpoints out to |z| = 40; a zero slope for
    line 0 -- per band at most 4 x the oracle's pinned error."""
    named = km.sets_of(fx)
    sets = [(mu, b) for _, mu, b in named]
    got = kh.device_header_on_host(sets)
    assert got.shape == (len(sets),)
    kh.held_to_yardstick(fx, got, sets, "kg_device.h on the host")
    by_name = {n: g for (n, _, _), g in zip(named, got)}
    for name in ("equal_slopes", "equal_slopes_zero", "rand_n1_0", "zero_slope_line0_alone", "far_40"):
        assert by_name[name] == 0.0 and not np.signbit(by_name[name]), name          # exactly +0.0
    assert np.all(got >= 0.0) and not np.any(np.signbit(got))
    # duplicated lines change nothing: the set without its duplicates gives the same bits
    mu, b = dict((n, (m, s)) for n, m, s in named)["duplicates"]
    assert kh.device_header_on_host([(mu[[0, 1, 3]], b[[0, 1, 3]])])[0] == by_name["duplicates"]
    # ... and neither does a parallel line above another
    mu, b = dict((n, (m, s)) for n, m, s in named)["parallel"]
    assert kh.device_header_on_host([(mu[[0, 2, 3]], b[[0, 2, 3]])])[0] == by_name["parallel"]
    # three lines through one point: the middle one is off the envelope, the value is that of the outer two
    mu, b = dict((n, (m, s)) for n, m, s in named)["three_through_a_point"]
    assert kh.device_header_on_host([(mu[[0, 2]], b[[0, 2]])])[0] == by_name["three_through_a_point"]


@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_device_header_order_nan_and_random_sets(fx):
    rng = np.random.RandomState(3)
    sets = []
    for n in (2, 3, 7, 16, 17, 33, 64, 65, 129, 256):
        for spread in (1.0, 0.01):
            sets.append((rng.randn(n) * spread, rng.randn(n) * rng.choice([1.0, 1e-3, 50.0])))
    got = kh.device_header_on_host(sets)
    kh.held_to_yardstick(fx, got, sets, "kg_device.h on the host, random sets")
    # a NaN or infinite line: NaN for that set alone
    bad = [(np.array([0.0, np.nan, 1.0]), np.array([1.0, 0.5, 0.0])), (np.array([0.0, 0.2, 1.0]), np.array([1.0, np.inf, 0.0])),
           (np.array([0.0, 0.2]), np.array([-np.inf, 0.0])), sets[3]]
    out = kh.device_header_on_host(bad)
    assert np.all(np.isnan(out[:3])) and out[3] == got[3]
    # permuting the representer lines moves the value by the order of the additions at most: within the bar, and the set of
    # envelope lines is the same
    mu, b = sets[8]
    p = np.concatenate(([0], 1 + rng.permutation(len(mu) - 1)))
    kh.held_to_yardstick(fx, kh.device_header_on_host([(mu[p], b[p])]), [(mu[p], b[p])], "permuted")


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------
def test_abi_argument_checks_touch_no_gpu():
    eng = engine.Engine(0)
    assert engine.ACQ["KG"] == engine.ACQ_KG == 5 and engine.KG_MAX_POINTS == 255
    eng.set_acquisition(engine.ACQ_LCB, 2.0)
    for par in (1.0, 64.0, float("nan"), -1.0):
        with pytest.raises(ValueError) as ei:
            eng.set_acquisition(engine.ACQ_KG, par)
        assert "spx_set_acquisition" in str(ei.value)
        assert eng.get_acquisition() == (engine.ACQ_LCB, 2.0)
    with pytest.raises(ValueError):
        eng.set_acquisition(6, 0.0)                                      # the next number is unknown
    eng.set_acquisition("KG")
    assert eng.get_acquisition() == (engine.ACQ_KG, 0.0)
    # no dimension yet, no points, A out of range, a non-finite coordinate: all refused, nothing held
    lib, h = eng._lib, eng._h
    pts = np.zeros((256, 2))
    assert lib.spx_set_kg_points(h, engine._dp(pts), 3) == engine.SPX_ERR_ARG          # (no observations or candidates: D unknown)
    assert lib.spx_set_kg_points(h, engine._dp(pts), 0) == engine.SPX_ERR_ARG
    assert lib.spx_set_kg_points(h, engine._dp(pts), 256) == engine.SPX_ERR_ARG
    assert lib.spx_set_kg_points(h, None, 3) == engine.SPX_ERR_ARG
    assert lib.spx_set_kg_points(h, None, -1) == 0                                      # clearing what is not set is not an error
    assert eng.get_kg_points() is None and eng.stat("kg_points") == 0 and eng.stat("last_kg_points") == 0
    with pytest.raises(ValueError):
        eng.kg_lines(0)
    assert lib.spx_get_kg_lines(h, 0, None, None) == engine.SPX_ERR_ARG
    # KG refuses the refinement entry points and a pass without points, all from the host's record
    x, f, g = np.zeros((1, 2)), np.zeros(1), np.zeros((1, 2))     # (the library itself: Engine's wrappers check shapes against data first)
    for call, word in ((lambda: eng._check(lib.spx_ei_grad_batch(h, engine._dp(x), 1, engine._dp(f), engine._dp(g))), "SPX_ACQ_KG"),
                       (lambda: eng._check(lib.spx_ei_grad(h, engine._dp(x), engine._dp(f), engine._dp(g))), "SPX_ACQ_KG"),
                       (lambda: eng.ei_step(), "representer points"), (lambda: eng.ei_step(engine.FLAG_PER_SEC), "chose KG"),
                       (lambda: eng._check(lib.spx_constrained_ei_grad_batch(h, engine._dp(x), 1, 0.0, engine._dp(f), engine._dp(g))),
                        "SPX_ACQ_EI only")):
        with pytest.raises(ValueError) as ei:
            call()
        assert word in str(ei.value), (word, str(ei.value))          # the new check is the one that fires
    assert eng.get_acquisition() == (engine.ACQ_KG, 0.0)
    eng.close()


def test_a_partition_refuses_kg_in_either_order():
    eng = engine.Engine(0)
    eng.set_partition(2, 1000, 4)                                      # (a plain handle takes it; no device is touched)
    with pytest.raises(ValueError) as ei:
        eng.set_acquisition("KG")
    assert "SPX_ACQ_KG" in str(ei.value) and "2-D partition" in str(ei.value) and eng.get_acquisition() == (engine.ACQ_EI, 0.0)
    eng.set_partition(1, 0, 0)
    eng.set_acquisition("KG")
    eng.set_partition(2, 1000, 4)                                      # behind the acquisition: the pass refuses
    with pytest.raises(ValueError) as ei:
        eng.ei_step()
    assert "SPX_ACQ_KG" in str(ei.value) and "2-D partition" in str(ei.value) and eng.get_acquisition() == (engine.ACQ_KG, 0.0)
    eng.close()


def test_multi_device_handle_refuses_kg():
    eng = engine.MultiEngine([0, 0])       # (repeated ids: the host transport; creation touches no GPU)
    eng.set_acquisition(engine.ACQ_PI, 0.25)
    with pytest.raises(ValueError) as ei:
        eng.set_acquisition(engine.ACQ_KG, 0)
    assert "multi-device" in str(ei.value)
    assert eng.get_acquisition() == (engine.ACQ_PI, 0.25)
    with pytest.raises(ValueError):
        eng.set_kg_points(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        eng.kg_lines(0)
    assert eng._lib.spx_set_kg_points(eng._h, engine._dp(np.zeros((2, 2))), 2) == engine.SPX_ERR_ARG
    assert eng._lib.spx_get_kg_lines(eng._h, 0, None, None) == engine.SPX_ERR_ARG
    eng.close()


# ---- chooser arguments -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_accepts_kg(mod, tmp_path):
    ch = mod.init(str(tmp_path), "acq=KG")
    assert (ch.acq, ch.acq_par) == ("KG", 64.0)                        # acq_par = 0, the default, means A = 64
    assert mod.init(str(tmp_path), "acq=kg,acq_par=7").acq_par == 7.0
    assert mod.init(str(tmp_path), "acq=KG,acq_par=255").acq_par == 255.0
    eng = AcqStandinEngine()
    ch._apply_acquisition(eng)
    assert eng.acq_calls == [(engine.ACQ_KG, 0.0)] and ch.last_acq_used == "KG"     # (A is the chooser's: the handle takes par 0)
    ch._apply_acquisition(eng, pending=True)                           # pending jobs: EI over the fantasies, set explicitly
    assert eng.acq_calls[-1] == (engine.ACQ_EI, 0.0) and ch.last_acq_used == "EI"
    assert ch.last_kg is None


@pytest.mark.parametrize("args", ["acq=KG,acq_par=0.5", "acq=KG,acq_par=256", "acq=KG,acq_par=-1", "acq=KG,acq_par=nan",
                                  "acq=KG,ndev=2"])
@pytest.mark.parametrize("mod", [GPEIChooser, GPEIOptChooser])
def test_chooser_refuses_bad_kg_arguments(mod, args, tmp_path):
    with pytest.raises(ValueError) as ei:
        mod.init(str(tmp_path), args)
    # the new range checks are the ones that fire (not "acq=KG is not available")
    word = "ndev" if "ndev" in args else "out of range" if args.endswith(("-1", "nan")) else "representer points"
    assert "allowed" in str(ei.value) and word in str(ei.value) and "not available on" not in str(ei.value)


@pytest.mark.parametrize("mod", [GPEIperSecChooser, GPConstrainedEIChooser, GPParetoChooser])
def test_the_other_choosers_refuse_kg(mod, tmp_path):
    with pytest.raises(ValueError):
        mod.init(str(tmp_path), "acq=KG")
    assert getattr(mod, mod.__name__.rsplit(".", 1)[1]).kg_allowed is False
    # ... while the two grid choosers list it: the refusal above is a decision, not an unknown name
    assert GPEIChooser.GPEIChooser.kg_allowed and GPEIOptChooser.GPEIOptChooser.kg_allowed


# ---- a seeded Branin sequence through the oracle engine ------------------------------------------------------------------------------
@pytest.mark.parametrize("mod,arg", [(GPEIChooser, "mcmc_iters=3"), (GPEIOptChooser, "mcmc_iters=2,burnin=3,grid_subset=3,use_multiprocessing=0")])
def test_kg_proposals_are_reproducible_and_draw_no_random_numbers(mod, arg, golden_dir, tmp_path):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:200]
    Eng = kh.make_oracle_engine()
    runs = {}
    for name, acq in (("EI", "EI"), ("KG", "KG,acq_par=9"), ("KG2", "KG,acq_par=9")):
        d = tmp_path / name
        d.mkdir()
        engines = []

        def make():
            engines.append(Eng())
            return engines[-1]
        runs[name] = branin_sequence(mod, arg + ",acq=" + acq, d, grid, 4, 41, make)
        runs[name + "_engines"] = engines
    # reproducible: the same seeds, the same proposals and generator states
    for a, b in zip(runs["KG"], runs["KG2"]):
        assert a[0] == b[0] and same_state(a[2], b[2])
    assert [r[3] for r in runs["KG"][2:]] == ["KG"] * 2 and all(r[0] < grid.shape[0] for r in runs["KG"])     # grid points only
    # the first GP call sees the same data under both acquisitions: numpy's generator ends where acq=EI's ends
    assert same_state(runs["EI"][2][2], runs["KG"][2][2])
    # what the chooser asked of the engine: the mean pass over the whole grid, 9 points, the KG pass over the candidates
    eng = runs["KG_engines"][2]
    assert ("set_kg_points", 9) in eng.calls and eng.kg_points.shape == (9, 2)
    assert [c for c in eng.calls if c[0] == "ei_run"][0][1] == grid.shape[0]
    assert eng.get_acquisition()[0] == engine.ACQ_EI                    # ... and the handle's setting restored


def test_kg_points_are_the_rows_of_the_lowest_mean(golden_dir, tmp_path):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:150]
    Eng = kh.make_oracle_engine()
    ch = GPEIChooser.init(str(tmp_path), "mcmc_iters=2,acq=KG,acq_par=5")
    eng = ch._eng = Eng()
    from tests.helpers import branin
    values = np.full(grid.shape[0], np.nan)
    done = np.arange(6)
    values[done] = branin(grid[done, 0], grid[done, 1])
    np.random.seed(5)
    cand = np.arange(6, grid.shape[0])
    job = ch.next(grid, values, np.full(grid.shape[0], np.nan), cand, np.zeros(0, dtype=int), done)
    lk = ch.last_kg
    assert ch.last_acq_used == "KG" and job == cand[lk["grid_index"]]
    # the oracle's own model mean over the grid under the chooser's hyper rows
    from oracle import gp_ei_oracle as orc
    from tests import acq_oracle as ao
    with orc.covar("Matern52"):
        mean = -np.mean(ao.over_hypers(ao.LCB, 0.0, grid[done], grid, values[done], eng.hypers), axis=1)
    assert np.array_equal(lk["points_index"], kh.choose_points(mean, 5)) and np.array_equal(lk["points"], grid[lk["points_index"]])
    with orc.covar("Matern52"):
        val = np.mean(ko.over_hypers(grid[done], grid[cand], values[done], lk["points"], eng.hypers), axis=1)
    assert lk["grid_index"] == int(np.argmax(val)) and lk["value"] == float(np.max(val))
    # recommend=1 behind the KG call: the model-mean pass over the grid runs ONCE and serves both; the recommendation is the
    # first representer point, the grid row of the lowest mean
    (tmp_path / "rec").mkdir()
    ch2 = GPEIChooser.init(str(tmp_path / "rec"), "mcmc_iters=2,acq=KG,acq_par=5,recommend=1")
    eng2 = ch2._eng = Eng()
    np.random.seed(5)
    assert ch2.next(grid, values, np.full(grid.shape[0], np.nan), cand, np.zeros(0, dtype=int), done) == job
    assert [c[1] for c in eng2.calls if c[0] == "ei_run"].count(grid.shape[0]) == 1
    rec = ch2.last_recommendation
    assert rec["grid_index"] == lk["points_index"][0] and abs(rec["mean"] - mean[rec["grid_index"]]) <= 1e-9 * (1 + abs(rec["mean"]))
    assert eng2.get_acquisition()[0] == engine.ACQ_EI
    assert kh.choose_points(np.array([3.0, np.nan, 1.0, 1.0, np.nan, 0.5]), 3).tolist() == [5, 2, 3]
    assert kh.choose_points(np.array([np.nan, 2.0]), 4).tolist() == [1]


def test_pending_calls_fall_back_to_ei(golden_dir, tmp_path):
    grid = np.load(os.path.join(golden_dir, "branin_trajectory.npz"))["grid"][:300]
    arg = "mcmc_iters=3,pending_samples=5,gpu_fantasies=0"
    Eng = kh.make_oracle_engine()
    runs = {}
    for acq in ("EI", "KG"):
        d = tmp_path / acq
        d.mkdir()
        runs[acq] = branin_sequence(GPEIChooser, arg + ",acq=" + acq, d, grid, 6, 77, Eng, n_pending=1)
    assert [r[3] for r in runs["KG"][3:]] == ["EI"] * 3
    for a, b in zip(runs["EI"], runs["KG"]):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and same_state(a[2], b[2])
    # and the stand-in engine refuses what the library refuses
    eng = Eng()
    eng.set_acquisition(engine.ACQ_KG, 0)
    eng.comp, eng.vals, eng.cand, eng.hypers = np.zeros((2, 2)), np.zeros(2), np.zeros((1, 2)), np.zeros((1, 5))
    with pytest.raises(ValueError):
        eng.ei_run()                                                   # no points
    eng.set_kg_points(np.zeros((1, 2)))
    eng.fant = np.zeros((1, 2, 1))
    with pytest.raises(ValueError):
        eng.ei_run()                                                   # fantasies


# ---- the held-state table --------------------------------------------------------------------------------------------------------
def test_held_record_of_the_representer_points():
    if ph.client("held_client") is None:
        pytest.skip("no host C++ compiler")
    T = {n: i for i, n in enumerate(["OBS", "CAND", "HYP", "TIME", "CON", "FACTOR", "CON_FACTOR", "FULL_FACTOR", "FANT", "ALPHA_S",
                                      "RESULTS", "COVAR", "PARTITION", "FRONT", "SEC", "SEC_CAND", "KGPTS"])}

    def bits(*names):
        return sum(1 << T[n] for n in names)

    def ask(b, op, thing):
        got = ph.ask("held_client", "%d 0 %s %d 0\n" % (b, op, T[thing]))[0].split()
        return int(got[0]), int(got[2])
    full = bits("OBS", "CAND", "HYP", "FACTOR", "FANT", "RESULTS", "KGPTS")
    assert ask(full, "drop", "KGPTS") == (full & ~bits("KGPTS", "RESULTS"), 1)                 # new points: the results alone
    assert ask(full, "drop", "CAND") == (full & ~bits("CAND", "RESULTS"), 1)                    # ... and they outlive everything else
    assert ask(full, "drop", "HYP") == (bits("OBS", "CAND", "KGPTS"), 1)
    assert ask(full, "drop", "OBS") == (bits("CAND", "HYP", "KGPTS"), 1)
    assert ask(full, "drop", "COVAR") == (full & ~bits("FACTOR", "FANT", "RESULTS"), 1)
    assert ask(full, "drop", "FRONT") == (full & ~bits("RESULTS"), 1)
    assert ask(0, "set", "KGPTS") == (bits("KGPTS"), 1)                                         # made from nothing
    assert ask(bits("OBS", "HYP", "FACTOR", "CAND"), "set", "RESULTS") == (bits("OBS", "HYP", "FACTOR", "CAND", "RESULTS"), 1)


# ---- scripts/time_kg.py as far as a CPU takes it -----------------------------------------------------------------------------------
def test_timing_script_parses_its_arguments_and_refuses_without_a_device():
    import importlib.util
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "scripts", "time_kg.py")
    spec = importlib.util.spec_from_file_location("time_kg", script)
    tk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tk)
    bench = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
    bm = importlib.util.module_from_spec(bench)
    bench.loader.exec_module(bm)
    for name in ("c2", "c3"):
        assert tk.SHAPES[name] == {k: bm.WORKLOADS[name][k] for k in ("N", "M", "D", "H")}

    def run(*args):
        return subprocess.run([sys.executable, script] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run("--help").returncode == 0
    r = run("--shapes", "c9")
    assert r.returncode == 2 and b"no shape" in r.stderr
    if engine.device_count() == 0:
        r = run("--shapes", "small", "--steps", "1", "--rounds", "1")
        assert r.returncode == 2 and b"no HIP device" in r.stderr and r.stdout == b""
