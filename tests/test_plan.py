"""Which form of a call runs is decided by two pure functions, plan_factor and plan_ei (csrc/spx_plan.h), before anything
is reserved or queued.  Every "same bits in every form" test forces a form through options and trusts that decision; here
it is pinned without a GPU, through tests/c/plan_client.cpp (a stand-alone host program over the header alone, built with
the address and undefined-behaviour sanitizers).  Each expected value carries its derivation from the rules of do_factor /
ei_run_impl as they stood before the planner existed.  The option table is checked through the real library
(spx_create touches no device)."""
import itertools
import os
import re

import pytest

from spearmint_amd import engine
from tests import plan_helpers as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_cxx = pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")

PER_SEC, KEEP_MOMENTS, TIMING, TIME_ONLY = 1, 2, 4, 8


def lean(N, H, D=2, dest=1, **kw):
    """spx_gp_logprob's factorisation: lean, queued (defer), pinned destinations supplied."""
    return ph.plan("factor", N=N, H=H, D=D, lean=1, defer=1, dest=dest, **kw)


def eifac(N, H, D=2, **kw):
    return ph.plan("factor", N=N, H=H, D=D, **kw)


def flags_of(p, *names):
    return tuple(bool(p[n]) for n in names)


# ---- the log-likelihood call, defaults ---------------------------------------------------------------------------------
@needs_cxx
def test_logprob_defaults_small():
    # lean with nh = 1 <= 32 draws: the tile-major forms (rl), N padded to 64: Np = 64, one block.  rl and lean_flow != 0 and
    # not demoted -> flow; lean_flow_cov != 0 -> cov_in_flow; with lean_merge != 0 -> merged_prologue; lean_one != 0, destinations,
    # Dp = 4 <= 64, nblk = 1 <= 16 -> fused.  Items: (nblk + 1) / 2 + sum_i (i + 2) / 2 = 1 + 1 = 2; nh * items = 2 <= 256 and
    # timing off -> zero_copy.  Load nh * nblk^1.5 = 1 <= 800 -> flow_alone.  4 nh Np^2 = 16 384 B <= 300e6 -> not lazy; ps
    # needs !flow -> 0.
    p = lean(17, 1)
    assert (p["Np"], p["nblk"], p["fused_items"], p["nh"], p["nm"]) == (64, 1, 2, 1, 1)
    assert flags_of(p, "rl", "flow", "tiled", "cov_in_flow", "merged_prologue", "fused", "zero_copy", "flow_alone",
                    "zero_in_kernel") == (True,) * 9
    assert flags_of(p, "lazy", "ps", "bracket", "step") == (False,) * 4
    # the one-launch call's completion is polled in its pinned flags (lean_poll != 0) unless per-launch events are on
    assert p["poll"] == 1 and lean(17, 1, lean_poll=0)["poll"] == 0 and lean(17, 1, timing=1)["poll"] == 0
    assert lean(17, 1, lean_one=0)["poll"] == 0 and lean(17, 1, lean_one=0, lean_poll=1)["poll"] == 0


@needs_cxx
def test_logprob_padding_to_64():
    assert (lean(65, 1)["Np"], lean(65, 1)["nblk"]) == (128, 2)          # ceil(65 / 64) = 2 blocks
    p = lean(130, 32)                                                   # 32 draws: still the tile-major forms, 3 blocks <= 16
    assert (p["Np"], p["nblk"], p["fused"]) == (192, 3, 1)


@needs_cxx
def test_logprob_beyond_32_draws_takes_the_left_looking_launches():
    # nh = 33 > 32: not rl, so the handle's Np (130 -> 256); flow = (rl or (not lean and ei_flow)) and ... = false; nothing of
    # the one-launch family, and k_scale_rows zeroes info
    p = lean(130, 33)
    assert p["Np"] == 256 and p["nblk"] == 4
    assert flags_of(p, "rl", "flow", "tiled", "fused", "zero_in_kernel", "merged_prologue", "cov_in_flow", "ps") == (False,) * 8


# ---- boundaries of `fused` ------------------------------------------------------------------------------------------------
@needs_cxx
def test_fused_boundaries():
    # N = 1025 -> Np = 1088, nblk = 17 > 16: by default (lean_one = -1) only up to two draws
    assert lean(1025, 2)["nblk"] == 17
    assert lean(1025, 2)["fused"] == 1
    p = lean(1025, 3)
    assert (p["fused"], p["merged_prologue"]) == (0, 1)
    assert lean(1025, 3, lean_one=1)["fused"] == 1                      # asked for: any size
    assert lean(1025, 2, lean_one=0)["fused"] == 0
    # Dp: D = 64 -> 64 (fits the kernel's LDS tile), D = 65 -> round_up(65, 32) = 96
    assert (lean(17, 1, D=64)["Dp"], lean(17, 1, D=64)["fused"]) == (64, 1)
    assert (lean(17, 1, D=65)["Dp"], lean(17, 1, D=65)["fused"]) == (96, 0)
    assert lean(17, 1, D=65)["merged_prologue"] == 1
    assert lean(17, 1, dest=0)["fused"] == 0                            # nowhere to reduce into
    p = lean(17, 1, demoted=1)                                          # after a hand-off time-out: the launches
    assert flags_of(p, "flow", "merged_prologue", "fused", "cov_in_flow") == (False,) * 4 and p["rl"] == 1 and p["ps"] == 1


# ---- boundaries of `zero_copy` --------------------------------------------------------------------------------------------
@needs_cxx
def test_zero_copy_boundaries():
    # N = 300 -> Np = 320, nblk = 5; items = 3 + (1 + 1 + 2 + 2 + 3) = 12.  Default lean_zc: nh * items <= 256
    assert (lean(300, 21)["nblk"], lean(300, 21)["fused_items"]) == (5, 12)
    assert lean(300, 21)["zero_copy"] == 1                              # 252
    p = lean(300, 22)
    assert (p["zero_copy"], p["fused"]) == (0, 1)                       # 264
    assert lean(300, 22, lean_zc=1)["zero_copy"] == 1
    assert lean(300, 21, lean_zc=0)["zero_copy"] == 0
    for N, H in ((17, 1), (300, 21), (300, 22)):                        # per-launch events need the copy as a stream operation
        for zc in (-1, 1):
            p = lean(N, H, timing=1, lean_zc=zc)
            assert (p["zero_copy"], p["fused"], p["bracket"]) == (0, 1, 1)


# ---- residency ------------------------------------------------------------------------------------------------------------
@needs_cxx
def test_flow_residency():
    # N = 2048: nblk = 32, load = nh * 32 * sqrt(32) = 181.02 nh: 724 at 4 draws, 905 at 5; the threshold is 800
    assert (lean(2048, 4)["nblk"], lean(2048, 4)["flow_alone"]) == (32, 1)
    assert lean(2048, 5)["flow_alone"] == 0
    assert lean(2048, 5, lean_flow_cu=1)["flow_alone"] == 1
    assert lean(2048, 4, lean_flow_cu=0)["flow_alone"] == 0
    assert lean(2048, 4)["yield"] == 1 and lean(2048, 4, lean_flow_yield=0)["yield"] == 0


# ---- one launch per block column (lean_flow = 0) -----------------------------------------------------------------------------
@needs_cxx
def test_step_forms():
    # lazy by size: 4 nh Np^2 > 300e6.  N = 2048: 16.78e6 nh -> 285e6 at 17 draws, 302e6 at 18.  ps = rl and not lazy and
    # lean_ps != 0 and not flow
    assert flags_of(lean(2048, 17, lean_flow=0), "ps", "lazy", "flow", "rl") == (True, False, False, True)
    assert flags_of(lean(2048, 18, lean_flow=0), "ps", "lazy") == (False, True)
    # N = 4096: 67.1e6 nh -> 268e6 at 4 draws, 336e6 at 5
    assert lean(4096, 4, lean_flow=0)["lazy"] == 0 and lean(4096, 5, lean_flow=0)["lazy"] == 1
    assert lean(2048, 17, lean_flow=0, lean_ps=0)["ps"] == 0
    assert flags_of(lean(2048, 17, lean_flow=0, lean_lazy=1), "ps", "lazy") == (False, True)
    assert lean(2048, 17)["ps"] == 0                                    # (with the data-flow launch there is no step launch)


# ---- the EI path's factorisation -------------------------------------------------------------------------------------------
@needs_cxx
def test_ei_path_factorisation():
    p = eifac(130, 3)                                                   # the predict GEMM's 128-row tiles: 130 -> 256
    assert (p["Np"], p["nblk"], p["nm"], p["nh"]) == (256, 4, 1, 3)
    assert flags_of(p, "flow", "tiled", "cov_in_flow", "bracket") == (True,) * 4     # ei_flow default on
    assert flags_of(p, "rl", "fused", "merged_prologue", "zero_in_kernel", "step") == (False,) * 5
    assert flags_of(eifac(130, 3, ei_flow=0), "flow", "tiled") == (False, False)
    assert flags_of(eifac(130, 3, lean_flow=0), "flow", "tiled") == (False, False)
    p = eifac(130, 3, time=1)                                           # the log-duration GP's draws ride along
    assert (p["nm"], p["nh"]) == (2, 6)
    assert lean(130, 3, time=1)["nm"] == 1                              # ... but not through the log-likelihood call
    assert eifac(130, 3, defer=1)["step"] == 1


@needs_cxx
def test_flag_words_and_sizes():
    for N, H, Np, nblk in ((300, 3, 320, 5), (17, 32, 64, 1)):
        p = lean(N, H)
        assert (p["Np"], p["nblk"]) == (Np, nblk)
        assert p["nfl"] == H * (nblk + 1) * nblk + H * nblk + 2 + 4096
        assert p["nn_bytes"] == H * Np * Np * 8 and p["rhs_bytes"] == H * 64 * Np * 8
        assert p["hyp_doubles"] == H * (3 + 2) + H * 4 and p["xs_bytes"] == H * Np * 4 * 8


# ---- the EI pass -----------------------------------------------------------------------------------------------------------
def ei(N, M, H, D=2, **kw):
    return ph.plan("ei", N=N, M=M, H=H, D=D, **kw)


@needs_cxx
def test_ei_pass_small_n_is_fused():
    # Mp = 157 * 128 = 20 096; the 512 MiB staging buffer holds 524 288 candidates of a draw at Np = 128: one chunk; draws
    # per launch 2^29 / (8 * 128 * 20 096) = 26 -> capped at H = 10.  Np == 128, no fantasies -> k_ei_fused128, one stream
    p = ei(128, 20000, 10)
    assert (p["Mp"], p["Mc"], p["Hb"], p["nrb"]) == (20096, 20096, 10, 1)
    assert (p["fused"], p["ns"], p["gemm_path"], p["slots"], p["ring_items"]) == (1, 1, 0, 0, 0)
    assert ei(128, 20000, 10, streams=2)["ns"] == 1                     # (the fused path never uses more than one stream)
    p = ei(128, 20000, 10, ei_fused=0)
    assert (p["fused"], p["gemm_path"], p["slots"], p["ring_items"]) == (0, 1, 1, 1)
    assert ei(128, 20000, 10, S=2, fant_budget=1 << 31)["fused"] == 0   # fantasies: the three-stage path


@needs_cxx
def test_ei_pass_chunks():
    # Np = 256, Mp = 1024; a 1 MiB buffer holds 2^20 / (8 * 256) = 512 candidates of one draw: two chunks of 512 (a whole
    # number of tiles per XCD would be 1024 > budget, and 512 < 16 tiles: unchanged); 2^20 / (8 * 256 * 512) = 1 draw
    p = ei(130, 1000, 3, kstar_budget_bytes=1 << 20)
    assert (p["Mp"], p["Mc"], p["Hb"], p["nrb"], p["ns"], p["ringed"], p["R"]) == (1024, 512, 1, 2, 1, 0, 0)
    assert p["kst_bytes"] == 1 << 20 and (p["slots"], p["kst_bufs"]) == (1, 1)
    p2 = ei(130, 1000, 3, kstar_budget_bytes=1 << 20, streams=2)
    assert (p2["slots"], p2["kst_bufs"]) == (2, 2)                      # (kst_bufs: slots of a pass that is not ringed)
    # items = 2 chunks x 3 draw groups under every stream count
    for streams in (1, 2, 3):
        assert ei(130, 1000, 3, kstar_budget_bytes=1 << 20, streams=streams, ring_budget=10 << 30)["ring_items"] == 6
    # slots the pass does not use are given back by a pass that stages -- not by a fused or a time-only one (slots = 0:
    # they would free the staging buffer of the passes around them)
    for streams in (1, 2):
        assert ei(130, 1000, 3, kstar_budget_bytes=1 << 20, streams=streams)["trim_ring"] == 1
        assert (ei(128, 1000, 3, streams=streams)["fused"], ei(128, 1000, 3, streams=streams)["trim_ring"]) == (1, 0)
        p = ei(130, 1000, 3, streams=streams, nmodels=2, flags=PER_SEC | KEEP_MOMENTS | TIME_ONLY)
        assert (p["ns"], p["slots"], p["ring_items"], p["trim_ring"]) == (streams, 0, 0, 0)


@needs_cxx
def test_ei_pass_ring():
    base = dict(kstar_budget_bytes=1 << 20, streams=3)
    # one slot = Hb Np Mc 8 = 1 MiB; items = 2 chunks x 3 draw groups = 6; R = min(budget / slot, items) in [1, 4096]
    for budget, R in ((0, 1), ((7 << 20) // 2, 3), (6 << 20, 6), (10 << 30, 6)):
        p = ei(130, 1000, 3, ring_budget=budget, **base)
        assert (p["ns"], p["ringed"], p["slot_bytes"], p["ring_items"], p["R"], p["slots"], p["trim_ring"]) == (3, 1, 1 << 20, 6, R, R, 1)
        assert p["kst_bufs"] == 0
    assert ei(130, 1000, 3, ring_budget=10 << 30, kstar_ring=2, **base)["R"] == 2
    assert ei(130, 1000, 3, ring_budget=0, kstar_ring=9, **base)["R"] == 6          # never more slots than items
    for kw in (dict(timing=1), dict(flags=TIMING)):                     # per-launch events: in order on one stream
        p = ei(130, 1000, 3, ring_budget=10 << 30, **dict(base, **kw))
        assert (p["ns"], p["ringed"], p["R"], p["trim_ring"], p["timing_on"]) == (1, 0, 0, 0, 1)
        assert (p["slots"], p["ring_items"]) == (1, 6)                       # one slot of the ring it keeps
    p = ei(130, 1000, 3, ring_budget=10 << 30, nmodels=2, flags=PER_SEC | KEEP_MOMENTS | TIME_ONLY, **base)
    assert (p["ns"], p["ringed"], p["R"], p["gemm_path"], p["time_only"]) == (3, 0, 0, 0, 1)
    assert (p["slots"], p["ring_items"], p["trim_ring"]) == (0, 0, 0)
    assert ei(128, 1000, 3, ring_budget=10 << 30, **base)["trim_ring"] == 0         # fused on a streams = 3 handle: the ring stays
    assert ei(130, 1000, 3, ring_budget=10 << 30, **base)["corun"] == 1
    assert ei(130, 1000, 3, ring_budget=10 << 30, kstar_corun=0, **base)["corun"] == 0
    assert ei(130, 1000, 3, ring_budget=10 << 30, cov_flat=0, **base)["corun"] == 0
    assert ei(130, 1000, 3, kstar_budget_bytes=1 << 20, streams=2)["corun"] == 0


@needs_cxx
def test_ei_pass_fantasies_cap():
    # default staging budget: one chunk of 1024, all 3 draws.  Partial means [nrb = 2][2][S = 4][Mc] doubles = 128 Mc bytes:
    # a 64 KiB budget holds 512 candidates -> two chunks of 512, and 65 536 / (128 * 512) = 1 draw per launch
    free = ei(130, 1000, 3, S=4, fant_budget=1 << 31)
    assert (free["Mc"], free["Hb"]) == (1024, 3)
    p = ei(130, 1000, 3, S=4, fant_budget=1 << 16)
    assert (p["Mc"], p["Hb"], p["fused"]) == (512, 1, 0)
    assert p["bgS_bytes"] == 2 * 2 * 1 * 4 * 512 * 8 and p["scratch_bytes"] == 1 * 4 * 512 * 8


@needs_cxx
def test_ei_pass_overlap():
    for pending, streams, so, want in ((1, 1, -1, 1), (1, 1, 1, 1), (1, 1, 0, 0), (0, 1, -1, 0), (1, 2, -1, 0), (1, 3, -1, 0)):
        p = ei(300, 1000, 3, pending=pending, streams=streams, step_overlap=so, ring_budget=1 << 30)
        assert p["overlap"] == want, (pending, streams, so)
    assert ei(128, 1000, 3, pending=1, streams=3)["overlap"] == 1       # (fused: one stream whatever was asked)
    assert (ei(300, 1000, 3, pending=1, nmodels=2)["n_info"], ei(300, 1000, 3)["n_info"]) == (6, 0)


@needs_cxx
def test_ei_pass_padding_skip():
    # N = 129: Np = 256, two row blocks; 9 live 16-row tiles, one of them in the last block: saves 7 / 12 of it >= 0.12
    p = ei(129, 1000, 3)
    assert (p["gemm_nlive"], p["cov_live_rows"]) == (9, 144)
    assert ei(129, 1000, 3, gemm_partial=0)["gemm_nlive"] == 0
    assert ei(129, 1000, 3, gemm_waves=14)["gemm_nlive"] == 0           # (only the production GEMM has the short block)
    assert ei(128, 1000, 3, ei_fused=0)["gemm_nlive"] == 0              # all 8 tiles live
    # N = 20: two live tiles of eight -- but the fused kernel has no padding to skip
    assert ei(20, 1000, 3, ei_fused=0)["gemm_nlive"] == 2
    assert ei(20, 1000, 3)["gemm_nlive"] == 0


# ---- invariants over a lattice ------------------------------------------------------------------------------------------
TRI = ("lean_lazy", "ei_flow", "lean_flow_cov", "lean_flow_yield", "lean_flow_cu", "lean_flow", "lean_ps", "lean_merge",
       "lean_one", "lean_poll", "lean_zc", "step_overlap", "ei_fused", "stage_copies", "cov_flat", "gemm_partial", "kstar_corun")


@needs_cxx
def test_invariants_over_the_lattice():
    cases, keys = [], []
    for N, H, is_lean in itertools.product((1, 17, 64, 65, 128, 129, 130, 200, 300, 1025), (1, 2, 3, 21, 22, 32, 33), (0, 1)):
        for opt, v in [(None, 0)] + [(o, v) for o in TRI for v in (-1, 0, 1)] + [("timing", 1)]:
            kv = dict(N=N, H=H, D=2, lean=is_lean, defer=is_lean, dest=is_lean)
            if opt:
                kv[opt] = v
            cases.append(("factor", kv))
            keys.append((N, H, is_lean, opt, v))
    for key, p in zip(keys, ph.plans(cases)):
        N, H, is_lean, opt, v = key
        timing = opt == "timing"
        if p["ps"]:
            assert p["rl"] and not p["flow"] and not p["lazy"], key
        if p["fused"]:
            assert p["merged_prologue"], key
        if p["merged_prologue"]:
            assert p["flow"] and p["cov_in_flow"], key
        if p["zero_copy"]:
            assert p["fused"] and not timing, key
        if p["cov_in_flow"]:
            assert p["flow"], key
        assert bool(p["tiled"]) == bool(p["rl"] or p["flow"]), key
        assert p["Np"] % 64 == 0 and p["Np"] >= N and p["nblk"] * 64 == p["Np"], key
        if not (is_lean and p["nh"] <= 32):
            assert p["Np"] % 128 == 0, key
        assert p["Np"] - N < (64 if is_lean and p["nh"] <= 32 else 128), key


# ---- the option table, through the library ---------------------------------------------------------------------------------
ALL_OPTIONS = ("kstar_budget_bytes", "gemm_waves", "covar", "streams", "kstar_ring", "flow_rearm_after", "flow_spin_limit",
               "timing") + TRI


def _header_options():
    src = open(os.path.join(ROOT, "include", "spx.h")).read()
    block = src[src.index('/* options: "covar"'):src.index("int spx_set_option(")]
    return sorted(set(n for pre, n in re.findall(r'(spx_get_stat )?"([a-z_0-9]+)"', block) if not pre))


@pytest.fixture(scope="module")
def eng():
    if not os.path.exists(engine.default_lib_path()):
        import __graft_entry__ as g
        g.build()
    e = engine.Engine(0)
    yield e
    e.close()


def test_every_option_is_accepted(eng):
    names = _header_options()
    assert len(names) >= 19 and {"covar", "streams", "timing", "gemm_waves", "lean_flow", "kstar_ring", "cov_flat"} <= set(names)
    assert set(names) <= set(ALL_OPTIONS)
    for name in sorted(set(names) | set(ALL_OPTIONS)):
        for value in (0, 1, -1) if name not in ("gemm_waves", "covar") else (0,):
            eng.set_option(name, value)
    for name in ALL_OPTIONS:                                            # back to the defaults of a new handle
        eng.set_option(name, {"streams": 1, "timing": 0, "gemm_waves": 0, "covar": 0, "kstar_ring": 0, "kstar_budget_bytes": 0,
                              "flow_spin_limit": 0}.get(name, -1))


def test_option_errors(eng):
    with pytest.raises(ValueError, match=r"^spx_set_option: unknown option 'lean_flwo'$"):
        eng.set_option("lean_flwo", 1)
    with pytest.raises(ValueError, match=r"^spx_set_option: gemm_waves=5 is not a variant of this build$"):
        eng.set_option("gemm_waves", 5)
    for v in (-1, 4):
        with pytest.raises(ValueError, match=r"^spx_set_option: covar=%d is not one of SPX_COVAR_\*$" % v):
            eng.set_option("covar", v)
    eng.set_option("covar", 3)
    eng.set_option("covar", 0)
    eng.set_option("gemm_waves", 14)
    eng.set_option("gemm_waves", 0)


def test_option_values_reach_the_handle(eng):
    # what can be seen of a stored value without a device: flow_enabled follows lean_flow's tri-state
    eng.set_option("lean_flow", 0)
    assert eng.stat("flow_enabled") == 0
    eng.set_option("lean_flow", 7)
    assert eng.stat("flow_enabled") == 1
    eng.set_option("lean_flow", -1)
    assert eng.stat("flow_enabled") == 1
