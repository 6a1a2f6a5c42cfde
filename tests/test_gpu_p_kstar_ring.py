"""Option streams=3: K(X*,X) produced ahead of the predict GEMM on a low-priority stream, through a ring of staging slots
(ei_run_impl), by the kernel form that fits beside two GEMM workgroups (k_cov_corun).  Scheduling only: every result is
compared bit for bit with a one-stream handle -- best index, best EI, EI mean, EI per draw, and whatever else the pass
keeps.  Shapes follow test_gpu_a_parity.py::test_two_stream_mode_is_bit_identical: the small K(X*,X) budget gives several
chunks and one draw per work item, so a pass has 5 x (chunks) items and every ring depth below wraps round."""
import numpy as np
import pytest

from spearmint_amd.engine import (FLAG_CONSTRAINED, FLAG_KEEP_MOMENTS, FLAG_PER_SEC, FLAG_TIME_ONLY, Engine,
                                  MultiEngine)
from spearmint_amd.synthetic import synthetic_problem

pytestmark = pytest.mark.gpu
BUDGET = 384 * 1024 * 8
D, H = 7, 5


@pytest.fixture(scope="module")
def one():
    e = Engine(0)
    e.set_option("kstar_budget_bytes", BUDGET)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ring():
    e = Engine(0)
    e.set_option("kstar_budget_bytes", BUDGET)
    e.set_option("streams", 3)
    yield e
    e.close()


def _problem(N, M, seed, D=D):
    comp, cand, vals, hypers, log_durs, th = synthetic_problem(N, M, D, H, seed, per_sec=True)
    rs = np.random.RandomState(seed + 1)
    crows = np.column_stack((rs.uniform(0.5, 3.0, H), np.full(H, 1e-3), rs.uniform(0.5, 2.0, H),
                             rs.uniform(0.3, 1.5, (H, D))))
    ff = rs.randn(N) * 1.5
    fant = rs.randn(H, N, 3)
    bests = np.min(fant, axis=1) - 0.1
    return dict(comp=comp, cand=cand, vals=vals, hypers=hypers, log_durs=log_durs, th=th, crows=crows, ff=ff, fant=fant,
                bests=bests)


def _run(e, p, kind, step=False):
    """One pass of `kind` on engine e; everything the pass leaves behind, as a dict of arrays."""
    e.set_observations(p["comp"], p["vals"])
    e.set_candidates(p["cand"])
    e.set_hypers(p["hypers"])
    e.set_time_model(p["log_durs"], p["th"]) if kind in ("per_sec", "time_only") else e.set_time_model(None, None)
    e.set_constraint_model(p["comp"], p["ff"], p["crows"]) if kind == "constrained" else e.set_constraint_model(None, None, None)
    flags = {"plain": 0, "per_sec": FLAG_PER_SEC | FLAG_KEEP_MOMENTS, "constrained": FLAG_CONSTRAINED | FLAG_KEEP_MOMENTS,
             "fantasies": 0, "keep_moments": FLAG_KEEP_MOMENTS,
             "time_only": FLAG_PER_SEC | FLAG_KEEP_MOMENTS | FLAG_TIME_ONLY}[kind]
    if step and kind != "fantasies":
        e.ei_step(flags)
    else:
        e.factor()
        if kind == "fantasies":
            e.set_fantasies(p["fant"], p["bests"])
        e.ei_run(flags)
    out = {}
    if kind != "time_only":
        idx, val = e.best()
        out.update(idx=np.array(idx), val=np.array(val), mean=e.ei_mean(), draws=e.ei_draws())
    if kind in ("per_sec", "time_only"):
        out["tmean"] = np.stack([e.get_time_mean(d) for d in range(H)])
    if kind == "keep_moments":
        mv = [e.get_moments(d) for d in range(H)]
        out["func_m"] = np.stack([m for m, _ in mv])
        out["func_v"] = np.stack([v for _, v in mv])
    if kind == "constrained":
        out["cprob"] = np.stack([e.get_constraint_prob(d) for d in range(H)])
    return out


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


CASES = [(N, M) for N in (130, 260, 390, 1029) for M in (5000, 4999)] + [(170, 4999), (210, 4999), (256, 4999)]


@pytest.mark.parametrize("N,M", CASES)
def test_ring_mode_is_bit_identical_at_every_tail(one, ring, N, M):
    """N = 130 / 260 / 390 / 1029: one live 16-row tile in the last of 2 / 3 / 4 / 9 row blocks (k_predict_gemm_tail<1>);
    170 and 210: three and six live tiles (tail<2>, tail<3>); 256: no padding.  M = 5000 (padded to 5120) and the prime
    4999.  Plain and per-second passes."""
    p = _problem(N, M, 900 + N + M)
    for kind in ("plain", "per_sec"):
        want = _run(one, p, kind)
        got = _run(ring, p, kind)
        assert ring.stat("last_kstar_ring") >= 1 and one.stat("last_kstar_ring") == 0
        assert ring.stat("last_corun_launches") >= 4 and one.stat("last_corun_launches") == 0   # every item but the first
        _same(got, want, (N, M, kind))


@pytest.mark.parametrize("R", [1, 2, 3, H, 64])
def test_every_ring_depth(one, ring, R):
    """R = 1 (the producer waits for every GEMM), 2, 3, one per draw, and more slots than the pass has items (capped)."""
    p = _problem(260, 4999, 77)
    want = _run(one, p, "plain")
    try:
        ring.set_option("kstar_ring", R)
        got = _run(ring, p, "plain")
        used = ring.stat("last_kstar_ring")
        got2 = _run(ring, p, "plain")          # again on the slots (and events) the first pass left behind
    finally:
        ring.set_option("kstar_ring", 0)
    items = H * 5                               # Np = 384: the budget holds 1024 candidates of one draw -- 5 chunks x 5 draws
    assert used == min(R, items), (used, R)
    _same(got, want, R)
    _same(got2, want, (R, "second pass"))


@pytest.mark.parametrize("kind", ["plain", "per_sec", "constrained", "fantasies", "keep_moments", "time_only"])
@pytest.mark.parametrize("R", [0, 2])
def test_every_pass_kind(one, ring, kind, R):
    p = _problem(390, 4999, 1234)
    want = _run(one, p, kind)
    try:
        ring.set_option("kstar_ring", R)
        got = _run(ring, p, kind)
    finally:
        ring.set_option("kstar_ring", 0)
    _same(got, want, (kind, R))


@pytest.mark.parametrize("covar", ["Matern52", "Matern32", "ARDSE"])
@pytest.mark.parametrize("dims", [3, 7, 16, 32, 40])
def test_every_corun_instantiation(one, ring, covar, dims):
    """The co-resident K(X*,X) kernel in every form the launcher picks: D = 3 / 7 / 16 -> one chunk of 1 / 2 / 4 feature
    quads, D = 32 (the headline workload's) -> two chunks of four where the stand-alone kernel takes one of eight, D = 40
    (padded to 64) -> four chunks where it takes two; each with the three correlation functions.  The stat shows that the
    launches took that kernel and not the stand-alone one."""
    p = _problem(260, 4999, 300 + dims, D=dims)
    try:
        for e in (one, ring):
            e.set_covar(covar)
        want = _run(one, p, "plain")
        got = _run(ring, p, "plain")
        items = ring.stat("last_kstar_ring")
        assert items >= 2 and ring.stat("last_corun_launches") >= items - 1 > 0
    finally:
        for e in (one, ring):
            e.set_covar("Matern52")
    _same(got, want, (covar, dims))


def test_corun_form_off_is_the_same_bits(one, ring):
    """Option kstar_corun=0: the ring with k_cov_flat as the producer (the attribution build's path)."""
    p = _problem(1029, 5000, 4321)
    want = _run(one, p, "plain")
    try:
        ring.set_option("kstar_corun", 0)
        got = _run(ring, p, "plain")
        assert ring.stat("last_corun_launches") == 0 and ring.stat("last_kstar_ring") >= 2
        ring.set_option("kstar_corun", -1)
        ring.set_option("cov_flat", 0)          # "always the 3-D grid" holds for the ring's launches too
        got3 = _run(ring, p, "plain")
        assert ring.stat("last_corun_launches") == 0
    finally:
        ring.set_option("kstar_corun", -1)
        ring.set_option("cov_flat", -1)
    _same(got, want, "kstar_corun=0")
    _same(got3, want, "cov_flat=0")


def test_ring_step_waits_for_the_pending_factorisation(one, ring):
    """ADVICE r04's race on the new path: spx_ei_step queues the factorisation on the main stream and the producer stream
    runs ahead of it; every call changes observations, hyper draws and the padded size."""
    for rep in range(6):
        N = 260 + 130 * (rep % 3)
        p = _problem(N, 5000, 7100 + rep)
        for kind in ("plain", "per_sec"):
            want = _run(one, p, kind, step=True)
            got = _run(ring, p, kind, step=True)
            _same(got, want, (rep, kind))


def test_one_handle_through_every_stream_count(one):
    """The staging slots and their events are one set for every stream count: a handle that goes 1 -> 2 -> 3 -> 2 -> 1 -> 3
    -> 1 streams (ring depths from the budget, 2 and 64) runs each pass on what the pass before left behind, with two
    problems whose slots differ in size (Np = 256 and 512; with fantasies a slot carries partial means too)."""
    probs = [_problem(130, 4999, 8100), _problem(390, 4999, 8101)]
    runs = (("plain", False), ("fantasies", False), ("plain", True))
    want = [[_run(one, p, kind, step) for kind, step in runs] for p in probs]
    e = Engine(0)
    try:
        e.set_option("kstar_budget_bytes", BUDGET)
        for i, (streams, depth) in enumerate(((1, 0), (2, 0), (3, 0), (3, 2), (2, 0), (1, 0), (3, 64), (1, 0))):
            e.set_option("streams", streams)
            e.set_option("kstar_ring", depth)
            for j, (kind, step) in enumerate(runs):
                got = _run(e, probs[i % 2], kind, step)
                used = e.stat("last_kstar_ring")
                assert used >= 1 if streams == 3 else used == 0, (i, streams, depth, kind, used)
                _same(got, want[i % 2][j], (i, streams, depth, kind, step))
    finally:
        e.close()


def test_fused_path_is_untouched(one, ring):
    p = _problem(100, 4999, 55)
    want = _run(one, p, "plain")
    got = _run(ring, p, "plain")
    assert ring.stat("last_step_fused") == 1 and ring.stat("last_kstar_ring") == 0
    _same(got, want, "N = 100")


def test_timing_mode_runs_in_order(one, ring):
    """timing=1: per-launch events, one stream, no ring -- the stage table stays attributable to single kernels."""
    p = _problem(260, 4999, 56)
    want = _run(one, p, "plain")
    try:
        ring.set_option("timing", 1)
        got = _run(ring, p, "plain")
        assert ring.stat("last_kstar_ring") == 0 and ring.stat("last_corun_launches") == 0
    finally:
        ring.set_option("timing", 0)
    _same(got, want, "timing")


def test_multi_device_handle_passes_the_options_through(one):
    p = _problem(260, 4999, 57)
    want = _run(one, p, "plain")
    m = MultiEngine([0])
    try:
        m.set_option("kstar_budget_bytes", BUDGET)
        m.set_option("streams", 3)
        m.set_option("kstar_ring", 3)
        m.set_observations(p["comp"], p["vals"])
        m.set_candidates(p["cand"])
        m.set_hypers(p["hypers"])
        m.factor()
        m.ei_run(0)
        idx, val = m.best()
        got = dict(idx=np.array(idx), val=np.array(val), mean=m.ei_mean(), draws=m.ei_draws())
    finally:
        m.close()
    _same(got, want, "multi")
