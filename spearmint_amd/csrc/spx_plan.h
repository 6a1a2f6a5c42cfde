// What a call will run, decided before anything is reserved or queued: the options of a handle and two pure functions,
// plan_factor (do_factor) and plan_ei (ei_run_impl), of the options and the call's shape.  Host-only, plain C++17, no HIP and
// no handle: spx_api.hip executes a plan and keeps it for spx_get_stat & co.; tests/c/plan_client.cpp prints plans on a
// machine without a GPU.  A new path decision is a field of a plan, set here, read there.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/spx.h"   // SPX_FLAG_*
#include "spx_geom.h"

#ifndef SPX_DEFAULT_CORUN
#define SPX_DEFAULT_CORUN -1          // option "kstar_corun" of a new handle (make DEFAULT_CORUN=0: the attribution build, for
#endif                                // callers such as bench.py that set "streams" but not this option)

// every field spx_set_option writes (its table, spx_api.hip, has a description per name); tri-states: 1 / 0 / -1 = default
struct Options {
    int64_t kst_budget = 512ll << 20;   // "kstar_budget_bytes": K(X*,X) staging buffer per stream
    int gemm_variant = 0;               // "gemm_waves": predict-GEMM variant of THIS handle; 0 = production
    int cov_kind = 0;                   // "covar": SPX_COVAR_*; SE = ARDSE kernels on unit length scales
    int nstreams = 1;                   // "streams"
    int ring_opt = 0;                   // "kstar_ring": slots of the ring (0 = from the byte budget)
    int corun_opt = SPX_DEFAULT_CORUN;  // "kstar_corun"
    int flow_rearm_after = 16;          // (0 = never)
    int flow_spin_limit = 0;            // (0 = the kernel's default)
    int64_t effects_pass_rows = 0;      // "effects_pass_rows": rows per pass of spx_main_effects (0 = default)
    int mes_grid = 256;                 // "mes_grid": probe values J of a max-value entropy search pass (8 .. 4096)
    bool timing = false;
    int lean_lazy = -1, step_overlap = -1, ei_fused = -1, ei_flow = -1, lean_flow_cov = -1, lean_flow_yield = -1,
        lean_flow_cu = -1, lean_flow = -1, lean_ps = -1, lean_merge = -1, lean_one = -1, lean_poll = -1, lean_zc = -1,
        stage_copies = -1, cov_flat = -1, gemm_partial = -1;
};

// ---- the factorisation (do_factor) ----------------------------------------------------------------------------------
struct FactorShape {
    int64_t N = 0;
    int D = 0, H = 0;
    int Np = 0;                  // the handle's: N padded to the predict GEMM's 128-row tiles
    bool have_time = false;      // a time model is set
    bool lean = false;           // objective GP only, Cholesky + forward solve, no W = L^-1 (log-likelihood path)
    bool defer_sync = false;     // return with the work queued (spx_gp_logprob, spx_ei_step)
    bool have_dest = false;      // pinned destinations for the one-launch form's results were supplied
    bool flow_demoted = false;   // a hand-off time-out keeps the handle on one launch per block column
    bool rhs_rows_on = false;    // spx_gp_logprob_rhs: a right-hand side per draw
};

struct FactorPlan {
    bool lean = false;
    int nm = 1, nh = 0, Np = 0, nblk = 0, Dp = 0, hs = 0;
    // The factorisation, blocked with 64x64 tiles; three generations, the same factor bit for bit (every tile receives its
    // update steps in the order 0, 1, 2, ..., through the same MFMA chains, and the diagonal blocks share diag_block):
    //   flow  k_lean_flow: ONE data-flow launch for all block columns of all draws, tile-major storage (the default);
    //   rl    the log-likelihood path's one-step-deep launches per block column, tile-major (k_lean_step_ps, or
    //         k_lean_step [+ k_lean_step2] + k_lean_trsm), up to 32 draws -- the fallback of `flow` there;
    //   else  the batched left-looking launches of the EI path, row-major (k_chol_diag + k_chol_panel) -- the fallback of
    //         `flow` for spx_factor, and the log-likelihood path beyond 32 draws.
    bool rl = false, flow = false, tiled = false;
    bool flow_alone = false;        // k_lean_flow: one workgroup per CU
    bool yield = false;             // ... two per CU: a workgroup yields to a neighbour's diagonal block
    bool cov_in_flow = false;       // k_lean_flow builds the tiles of K(X,X) itself
    int lazy = 0, ps = 0;           // rl: trailing updates two steps at a time / panel solve inside the step launch
    bool merged_prologue = false;   // observation scaling and right-hand-side rows in one launch
    bool fused = false;             // ... and in no launch of their own: the log-likelihood call is ONE launch
    bool zero_copy = false;         // ... which reads the hyper rows out of the pinned upload buffer itself
    bool poll = false;              // ... and whose completion the host watches in its pinned flags
    bool zero_in_kernel = false;    // the right-hand-side kernel zeroes info (else k_scale_rows does)
    bool bracket = false;           // whole-stage events around the call
    bool step = false;              // spx_ei_step: events for the EI pass that is queued behind
    int fused_items = 0;
    int64_t vstride = 0;            // right-hand side: 0 = the shared values, N = a row per draw
    size_t nfl = 0;                 // k_lean_flow's flag words
    size_t hyp_doubles = 0, xs_bytes = 0, vec_bytes = 0, nn_bytes = 0, dinv_bytes = 0, info_bytes = 0, ps_bytes = 0,
           rhs_bytes = 0, diagL_bytes = 0;
};

inline FactorPlan plan_factor(const Options& o, const FactorShape& s)
{
    FactorPlan p;
    p.lean = s.lean;
    p.nm = (s.have_time && !s.lean) ? 2 : 1;
    p.nh = p.nm * s.H;
    p.Dp = padded_dim(s.D);
    p.hs = 3 + s.D;
    const int nh = p.nh;
    // the log-likelihood path's own forms hold up to 32 draws (beyond ~40 the one-step launches are work-bound and lose); it
    // then zeroes info (and the hand-off flags) in its right-hand-side kernel: two stream operations fewer per call
    p.rl = p.zero_in_kernel = s.lean && nh <= 32;
    // The EI path pads the observations to the predict GEMM's 128-row tiles.  The log-likelihood path (tile-major, up to
    // 32 draws) only needs whole 64 x 64 blocks: N <= 64 is ONE diagonal block instead of two, N = 129 .. 192 three
    // instead of four -- the padding block is an identity that costs a full link of the chain of diagonal blocks
    // (~17 us of a 64 us call at N <= 64).  Same bits: padding rows never touch the others.
    p.Np = p.rl ? (int)round_up(s.N, SPX_NB) : s.Np;
    p.nblk = p.Np / SPX_NB;
    const int nblk = p.nblk;
    // The EI path (spx_factor) takes the data-flow launch too (option ei_flow, default on; measured against the left-looking
    // launches: factor stage 0.28 -> 0.19 ms at N = 256 x 10 draws, 6.3 -> 3.8 ms at 2048 x 20, 2.3 -> 1.5 ms at
    // 1024 x 40, 0.85 -> 0.61 ms at 512 x 60): no right-hand-side rows, the diagonal blocks of L kept for spx_get_factor,
    // W = L^-1 from the tile-major factor (k_trinv<true>); every EI result stays what it was.
    const bool eflow = !s.lean && o.ei_flow != 0;
    // The whole factorisation as ONE data-flow launch (k_lean_flow; option lean_flow, default on): against one launch per
    // block column -27 ... -36 % per call at N = 2048 (1-32 draws), -25 ... -34 % at N = 1000, -20 % at N = 256, -6 ... -10 %
    // at N = 64 (profiles/r03_flow_ab.log); the same factor bit for bit
    p.flow = (p.rl || eflow) && o.lean_flow != 0 && !s.flow_demoted;
    p.tiled = p.rl || p.flow;
    // Residency (option lean_flow_cu: 1 / 0 / -1 = by size; scripts/dev/flow_modes.py).  A diagonal block's dependent MFMA
    // chain runs a third slower beside a neighbour whose products keep the matrix pipes busy, and the whole call follows
    // that chain.  Small launches (draws x block columns^1.5 <= 800: N = 2048 up to 4 draws, N = 1000 up to 12) get ONE
    // workgroup per CU (the launch asks for 96 KB of LDS).  Larger ones need the places: two per CU, and a workgroup yields
    // while its neighbour is the next link of a draw's chain -- from the end of its history through its diagonal block
    // (option lean_flow_yield; a word per CU, found by XCC_ID / HW_ID).  Against two per CU without yielding: N = 2048:
    // -11 % at 4 draws, -13 % at 6, -10 % at 8, -2 % at 12; N = 4096: -16 % at 2 draws; N = 1000: -7 % at 20 draws.
    const double flow_load = (double)nh * nblk * sqrt((double)nblk);
    p.flow_alone = o.lean_flow_cu >= 0 ? o.lean_flow_cu != 0 : flow_load <= 800.0;
    p.yield = o.lean_flow_yield != 0;
    // k_lean_flow builds the tiles of K(X,X) itself, where they are consumed: -1 ... -8 % per call at every size (no k_cov
    // launch, no round trip of the matrix through memory; option lean_flow_cov, scripts/dev/lean_option_ab.py)
    p.cov_in_flow = p.flow && o.lean_flow_cov != 0;
    // Trailing updates two block columns at a time (k_lean_step2) halve the traffic of the trailing matrices but
    // put a second MFMA step in front of every other diagonal block; that pays once the lower triangles of the
    // batch no longer fit the 256 MB Infinity Cache (measured: N=2048 from ~20 draws, N=4096 from 6; -3 ... -16 %),
    // and costs 5-10 % below that.  Same factor either way, bit for bit.
    p.lazy = o.lean_lazy >= 0 ? o.lean_lazy : ((double)nh * p.Np * p.Np * 4.0 > 300e6 ? 1 : 0);
    // Panel solve inside the step launch, pipelined behind the diagonal block's pivots (k_lean_step_ps): option lean_ps
    // (measured against a launch of its own per panel solve, scripts/dev/lean_option_ab.py: -1 ... -8 % per call from N = 256
    // up -- 2048: -6.5 % at 4-12 draws, -1 % at one; 1000: -3 ... -13 %; 4096: -4 ... -5 %)
    const int want_ps = o.lean_ps >= 0 ? o.lean_ps : 1;
    p.ps = (p.rl && !p.lazy && want_ps && !p.flow) ? 1 : 0;   // (only without the data-flow launch)
    // The log-likelihood call is a chain of small dependent launches (~4 us each whatever they do): when nothing between
    // them needs x / ls (k_lean_flow builds K(X,X) itself: the default), the scaling of the observations and the
    // right-hand-side rows are ONE launch, where the right-hand side used to be written (option lean_merge).
    p.merged_prologue = p.rl && p.cov_in_flow && o.lean_merge != 0;
    // ... and since round 6 NO launch of their own (option lean_one): k_lean_flow's items scale the rows they need into LDS,
    // generate the right-hand-side rows, and the last item of a draw reduces the log-likelihood into pinned host memory --
    // the call is the upload of the hyper rows and ONE launch.  (Dp <= 64: a block's scaled rows fit the kernel's LDS tile.)
    // (measured, profiles/r06_lean_one_ab.log: one launch instead of three is -11 us of 46 at N <= 64 with the polled
    // completion and the zero-copy rows, -12 of 91 at N = 256, -2 ... -4 % up to N = 1024; at N = 2048 with several draws the
    // items' own scaling costs more than the two launches did (+3 %), and with hundreds of items the reads of host memory do)
    p.fused = p.merged_prologue && o.lean_one != 0 && s.have_dest && p.Dp <= 64 && (o.lean_one > 0 || nblk <= 16 || nh <= 2);
    p.fused_items = (nblk + 1) / 2;
    for (int i = 0; i < nblk; ++i) p.fused_items += (i + 2) / 2;
    // (the fused launch reads the rows out of the pinned buffer itself -- option lean_zc: one stream operation fewer in front
    // of it)
    p.zero_copy = p.fused && o.lean_zc != 0 && !o.timing && (o.lean_zc > 0 || (int64_t)nh * p.fused_items <= 256);
    // The fused launch stores every draw's value, then -- released at system scope -- its flag into the pinned buffer: the
    // host watches the flags instead of waiting for the stream to drain (option lean_poll; the end-of-kernel release and the
    // completion signal are ~7 us of a 42 us call)
    p.poll = p.fused && o.lean_poll != 0 && !o.timing;
    p.bracket = o.timing || !s.lean;
    p.step = s.defer_sync && !s.lean;
    p.vstride = s.rhs_rows_on ? s.N : 0;
    p.nfl = (size_t)nh * (nblk + 1) * nblk + (size_t)nh * nblk + 2 + 4096;   // (+ one word per CU: cu_busy)
    // raw hyper rows and the table [mean, noise, amp2, amp2*(1+1e-6)] travel in ONE upload
    p.hyp_doubles = (size_t)nh * p.hs + (size_t)nh * SPX_HT;
    p.xs_bytes = (size_t)nh * p.Np * p.Dp * 8;
    p.vec_bytes = (size_t)nh * p.Np * 8;
    p.nn_bytes = (size_t)nh * p.Np * p.Np * 8;
    p.dinv_bytes = (size_t)nh * nblk * SPX_NB * SPX_NB * 8;
    p.info_bytes = (size_t)nh * sizeof(int);
    p.ps_bytes = (size_t)nh * nblk * sizeof(int);
    p.rhs_bytes = (size_t)nh * SPX_NB * p.Np * 8;
    p.diagL_bytes = p.vec_bytes;
    return p;
}

// ---- the EI pass (ei_run_impl) --------------------------------------------------------------------------------------
// what the production GEMM does with a padded observation count: 0 = nothing to skip (or not this variant), else
// nlive = ceil(N / 16): the last row block goes to k_predict_gemm_tail, K(X*,X) stops at row 16 nlive
inline int predict_gemm_padding_plan(int variant, int N, int Np)
{
    if (!(variant == 0 || variant == 32)) return 0;
    const int nlive = (N + 15) / 16;
    const int nrb = Np / SPX_BM;
    const int lt = nlive - 8 * (nrb - 1);          // live 16-row tiles of the last row block
    if (lt < 1 || lt > 6) return 0;
    // The short block is a launch of its own in front of the others (it cannot share k_predict_gemm_tri's registers), which
    // costs a launch boundary: about a tenth of the pass.  What it saves is (8 - lt) / 8 of the last block's (8 nrb)-step K
    // loop out of 4 nrb (nrb + 1) steps in all = (8 - lt) / (4 (nrb + 1)).  Measured (profiles/r05_padding_skip.log: EI step,
    // 20 000 x 10 / 100 000 x 10): N = 129 ... 160 -31 %, 257 -21 %, 300 -14 %, 400 -16 %, 900 -7 %, 1300 -5 %; but N = 600
    // +-0, 1500 +6 %, 2000 +3 % where the saving is under a tenth.  Taken from 0.12 up.
    return (25 * (8 - lt) >= 12 * (nrb + 1)) ? nlive : 0;
}

struct EiShape {
    int64_t N = 0, M = 0;
    int Np = 0, D = 0, H = 0;
    int S = 0;                      // fantasies per draw
    int nmodels = 1;
    int32_t flags = 0;              // SPX_FLAG_*
    bool factor_pending = false;    // spx_ei_step: the factorisation is queued on the stream but not yet checked
    int64_t kst_budget = 0;         // bytes of a K(X*,X) staging buffer (option kstar_budget_bytes)
    int64_t fant_budget = 0;        // bytes the per-fantasy partial means may take (read when S > 0)
    int64_t ring_budget = 0;        // bytes the streams = 3 ring may take (read when the plan is `ringed` without kstar_ring)
};

struct EiPlan {
    bool per_sec = false, keep_mom = false, time_only = false, constrained = false;
    int64_t Mp = 0, Mc = 0;
    int Hb = 0, nrb = 0, Dp = 0;
    bool fused = false;             // the whole pass of a chunk is k_ei_fused128
    bool gemm_path = false;         // K(X*,X) -> predict GEMM -> EI finalize
    bool timing_on = false;
    int ns = 1;                     // streams the pass runs on
    int64_t ring_items = 0;         // work items of the pass (chunks x draw groups; the GEMM path, ringed or not)
    int slots = 0;                  // staging slots the pass uses: item i goes through slot i % slots (0: it stages nothing)
    int kst_bufs = 0;               // `slots` of a pass that is not ringed: read by nothing here, printed for the plan clients of earlier trees
    bool ringed = false;            // streams = 3: the slots are a ring of R, sized by a byte budget
    int64_t slot_bytes = 0;         // one slot of that ring: K(X*,X) of a work item and its fantasy partials
    int R = 0;
    bool trim_ring = false;         // slots beyond `slots` go back to the device
    bool overlap = false;           // a step's first producer work runs beside the factorisation
    bool cov_flat = false, corun = false;   // K(X*,X) launches: equal shares / (behind the pass's first) the co-resident form
    int gemm_nlive = 0, cov_live_rows = 0;
    int n_info = 0;                 // not-PD flags that travel home with the winner
    size_t cs_bytes = 0, s2_bytes = 0, kst_bytes = 0, bgS_bytes = 0, part_bytes = 0, scratch_bytes = 0, draw_bytes = 0,
           mean_bytes = 0;
};

// With `ringed` and no kstar_ring option, R is read off s.ring_budget, which the caller finds when slot_bytes changes: it
// plans, compares slot_bytes with the slot its budget was found for, and plans again with the new budget if they differ.
inline EiPlan plan_ei(const Options& o, const EiShape& s)
{
    EiPlan p;
    p.per_sec = (s.flags & SPX_FLAG_PER_SEC) != 0;
    p.keep_mom = (s.flags & SPX_FLAG_KEEP_MOMENTS) != 0;
    p.time_only = (s.flags & SPX_FLAG_TIME_ONLY) != 0;
    p.constrained = (s.flags & SPX_FLAG_CONSTRAINED) != 0;
    const int H = s.H, Np = s.Np, S = s.S;
    const int64_t Mp = round_up(s.M, SPX_BN);
    p.Mp = Mp;
    p.Dp = padded_dim(s.D);
    p.nrb = Np / SPX_BM;
    const int nrb = p.nrb;
    // candidate-chunk / draw-group plan for the K(X*,X) staging buffer
    int64_t mc_budget = s.kst_budget / (8ll * Np) / SPX_BN * SPX_BN;   // what the staging buffer holds of one draw
    if (mc_budget < SPX_BN) mc_budget = SPX_BN;
    int64_t Mc = mc_budget < Mp ? mc_budget : Mp;
    {
        // equal-sized chunks (no tiny, inefficient last launch) ...
        const int64_t nchunks = (Mp + Mc - 1) / Mc;
        Mc = round_up((Mp + nchunks - 1) / nchunks, SPX_BN);
        // ... of a whole number of candidate tiles per XCD when there are several: the predict GEMM deals the
        // 128-candidate tiles of a launch round-robin to the 8 XCDs, and a launch with 245 tiles runs as long as one
        // with 248 (measured at C3: 7 chunks of 224 tiles 268 ms per step, 6 of 261 or 5 of 313 tiles 273 ms)
        if (nchunks > 1) {
            const int64_t up = round_up(Mc, 8 * SPX_BN);
            if (up <= mc_budget) Mc = up;
            else if (Mc >= 16 * SPX_BN) Mc = Mc / (8 * SPX_BN) * (8 * SPX_BN);
        }
    }
    int64_t Hb = s.kst_budget / (8ll * Np * Mc);
    if (Hb < 1) Hb = 1;
    if (Hb > H) Hb = H;
    if (S > 0) {
        // the per-fantasy partial means are [nrb][2][S][Mc]: keep them under the fantasies budget (2 GB of 288 -- at C3 size
        // with 100 fantasies the plan's own 28 672-candidate chunks fit; the 256 MB of earlier rounds cut them to 9 856: 420
        // launch pairs of a few dozen workgroups instead of 140 -- or less on a smaller or fuller GPU: smaller chunks instead
        // of an allocation failure)
        int64_t cap = s.fant_budget / ((int64_t)nrb * 2 * S * 8) / SPX_BN * SPX_BN;
        if (cap < SPX_BN) cap = SPX_BN;
        if (Mc > cap) {
            const int64_t nchunks = (Mp + cap - 1) / cap;
            Mc = round_up((Mp + nchunks - 1) / nchunks, SPX_BN);
        }
        // ... and as many draws per launch as that leaves room for (small problems: all of them -- ten launch pairs of a
        // 20 000-candidate pass become one)
        int64_t hb = s.fant_budget / ((int64_t)nrb * 2 * S * 8 * Mc);
        if (hb > 65535 / S) hb = 65535 / S;       // (grid.y of the per-fantasy EI kernel)
        if (hb < 1) hb = 1;
        if (hb < Hb) Hb = hb;
    }
    p.Mc = Mc;
    p.Hb = (int)Hb;
    // N <= 128 without fantasies: the whole EI pass of a chunk -- K(X,X*), beta = W K*, the moments, EI -- is one kernel
    // with K* and beta in registers (fused_kernels.hip; option ei_fused); same bits as the three-stage path
    p.fused = Np == SPX_PADN && S == 0 && o.ei_fused != 0;
    p.gemm_path = !p.fused && !p.time_only;
    // streams = 3 with per-launch timing: the pass runs in order on one stream, so that every stage's events bracket that
    // stage's kernels alone (the stage table, bench.py --full's roofline)
    p.timing_on = o.timing || (s.flags & SPX_FLAG_TIMING);
    p.ns = p.fused ? 1 : ((o.nstreams == 3 && p.timing_on) ? 1 : o.nstreams);
    // K(X*,X) of work item i goes to staging slot i % slots (each slot with its own fantasy partials): one slot on one
    // stream, two on two, and with streams = 3 a ring of R, so that the producer stream runs up to R items ahead of the GEMM.
    // R comes from a byte budget -- a sixteenth of what the device has free, at most 10 GiB (C3: one chunk's twenty draws,
    // 9.4 GB of 288) -- or from option "kstar_ring"; never more slots than the pass has items.
    p.ringed = p.ns == 3 && !p.time_only;
    p.kst_bytes = (size_t)p.Hb * Np * Mc * 8;
    p.bgS_bytes = S > 0 ? (size_t)nrb * 2 * p.Hb * S * Mc * 8 : 0;
    if (p.gemm_path) p.ring_items = ((Mp + Mc - 1) / Mc) * ((H + p.Hb - 1) / p.Hb);
    if (p.ringed) {
        p.slot_bytes = (int64_t)(p.kst_bytes + p.bgS_bytes);
        int64_t r = o.ring_opt > 0 ? o.ring_opt : s.ring_budget / p.slot_bytes;
        r = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(r, p.ring_items), 4096));
        p.R = (int)r;
    }
    p.slots = !p.gemm_path ? 0 : p.ringed ? p.R : p.ns;
    p.kst_bufs = p.ringed ? 0 : p.slots;
    // slots the pass does not use go back to the device.  A pass that stages nothing releases nothing (a chooser whose
    // proposal pass is staged and whose recommendation pass is fused keeps its staging buffer), and a streams = 3 handle that
    // runs ONE pass another way (per-launch timing) keeps its ring: the next pass would only allocate the same gigabytes again
    p.trim_ring = p.gemm_path && (p.ringed || o.nstreams != 3);
    // A step (factor_pending): the factorisation is still running on the main stream -- a chain of small launches that leaves
    // most of the chip idle -- and the first producer work of the pass (candidate scaling, K(X*,X) of the first group of
    // draws) depends only on what the factorisation's FIRST kernel wrote.  It goes to the second stream, beside the
    // factorisation (C2: K(X*,X) of all ten draws, 0.10 ms, hidden behind a 0.17 ms factorisation).
    p.overlap = s.factor_pending && p.ns == 1 && o.step_overlap != 0;
    p.cov_flat = o.cov_flat != 0;
    // (the pass's first K(X*,X) has the chip to itself -- or shares it with the factorisation's small launches: the stand-alone
    // kernel; every later one of a streams = 3 pass runs beside a GEMM: the form that fits there)
    p.corun = p.ns == 3 && o.corun_opt != 0 && p.cov_flat;
    // N is padded to the predict GEMM's 128-row tiles with an identity: the production GEMM skips what the padding would
    // multiply (K steps and row tiles from tile ceil(N / 16) on) and K(X*,X) then leaves those rows unwritten.  Same bits.
    p.gemm_nlive = (!p.fused && o.gemm_partial != 0) ? predict_gemm_padding_plan(o.gemm_variant, (int)s.N, Np) : 0;
    p.cov_live_rows = 16 * p.gemm_nlive;
    p.n_info = s.factor_pending ? s.nmodels * H : 0;
    p.cs_bytes = (size_t)H * Mc * p.Dp * 8;
    p.s2_bytes = (size_t)H * Mc * 8;
    p.part_bytes = (size_t)nrb * H * Mc * 8;
    p.scratch_bytes = (size_t)p.Hb * S * Mc * 8;
    p.draw_bytes = (size_t)H * Mp * 8;
    p.mean_bytes = (size_t)Mp * 8;
    return p;
}

// ---- Thompson sampling (spx_thompson) -------------------------------------------------------------------------------
// The call runs the EI pass's S > 0 GEMM branch (plan_ei with S = the paths per draw and no flags: chunks, draw groups, slots
// and the per-fantasy partial sums are that plan's) with right-hand sides of its own; what it holds beside that plan's buffers
// is decided here, next to the fantasy buffers' sizes.
#define SPX_TS_MAX_PATH_BYTES (4ll << 30)     // H S Mp 8 of one call; beyond it spx_thompson refuses
struct TsShape {
    int64_t N = 0, M = 0;
    int Np = 0, D = 0, H = 0, S = 0, F = 0;
    bool per_draw = false;
};
struct TsPlan {
    int64_t Mp = 0;
    int Dp = 0, sblocks = 0;                // blocks of 16 paths: k_ts_prior forms the features once per block
    size_t par_doubles = 0;                 // nu [H][F Dp] | phase [F] | scale [H] | sig [H], one upload
    size_t w_bytes = 0, eps_bytes = 0;      // the caller's normals as uploaded ([H or 1][S][F], [H or 1][S][N])
    size_t obs_bytes = 0;                   // the prior at the observations, and the right-hand sides: [H][S][N] each
    size_t gamma_bytes = 0;                 // Gamma [H][S][Np], the layout of launch_gamma_multi
    size_t path_bytes = 0;                  // the prior at the candidates, and the paths: [H][S][Mp] each
    bool fits = false;                      // path_bytes <= SPX_TS_MAX_PATH_BYTES and the per-path launches' grids (H S <= 65535)
};
inline TsPlan plan_ts(const TsShape& s)
{
    TsPlan p;
    p.Mp = round_up(s.M, SPX_BN);
    p.Dp = padded_dim(s.D);
    p.sblocks = (s.S + 15) / 16;
    const size_t nd = s.per_draw ? (size_t)s.H : 1;
    p.par_doubles = (size_t)s.H * s.F * p.Dp + (size_t)s.F + 2 * (size_t)s.H;
    p.w_bytes = nd * s.S * s.F * 8;
    p.eps_bytes = nd * s.S * (size_t)s.N * 8;
    p.obs_bytes = (size_t)s.H * s.S * (size_t)s.N * 8;
    p.gamma_bytes = (size_t)s.H * s.S * (size_t)s.Np * 8;
    p.path_bytes = (size_t)s.H * s.S * (size_t)p.Mp * 8;
    p.fits = (int64_t)s.H * s.S <= 65535 && (double)s.H * s.S * (double)p.Mp * 8.0 <= (double)SPX_TS_MAX_PATH_BYTES;
    return p;
}

// ---- the main-effects report (spx_main_effects) ---------------------------------------------------------------------
// (D T + 1) Q structured rows go through ordinary EI passes with the moments kept; the rows of a pass are formed on the
// device, the kept means are reduced on the device.  What is decided here: how many rows a pass takes (option
// "effects_pass_rows": the candidate buffer, the scaled rows and the per-draw result rows of a pass grow with it, so it bounds
// the memory of the call; blocks of Q may straddle a boundary -- the means of all passes are gathered into one [H][rows]
// array first, so every split gives the same bits) and how k_effects_mean reads a block of Q means.
#define SPX_EFFECTS_MAX_ROWS (1ll << 30)      // (D T + 1) Q of one call; beyond it spx_main_effects refuses
#define SPX_EFFECTS_PASS_ROWS (1ll << 20)     // default rows per pass
#define SPX_EFFECTS_LDS_BYTES (48 << 10)      // k_effects_mean's staging tile (three workgroups per CU)
#define SPX_EFFECTS_THREADS 256
struct EffectsShape {
    int D = 0, H = 0;
    int64_t Q = 0, T = 0;
    int64_t pass_rows_opt = 0;      // option "effects_pass_rows" (0 = default)
};

struct EffectsPlan {
    int64_t rows = 0;               // (D T + 1) Q
    int64_t nblocks = 0;            // D T blocks of Q rows that become one entry of `curves` each
    int64_t pass_rows = 0;
    int npass = 0;
    bool gather = false;            // several passes: their kept means are copied into one [H][rows] array
    // k_effects_mean: a workgroup stages `wg_blocks` whole blocks in LDS with coalesced loads (row stride Q | 1: odd, so the
    // lanes that then walk one block each start in different banks) and one lane per block walks numpy's pairwise tree;
    // a block too long for the tile is walked straight from memory, one lane each
    bool mean_lds = false;
    int wg_blocks = 0;
    int64_t mean_tiles = 0;         // workgroups of the reduction, per draw
    int64_t gather_tiles = 0;       // ... and of the base_mean gather behind them
    size_t lds_bytes = 0;
    size_t in_bytes = 0, out_bytes = 0, cand_bytes = 0, gather_bytes = 0;
};

inline EffectsPlan plan_effects(const EffectsShape& s)
{
    EffectsPlan p;
    p.nblocks = (int64_t)s.D * s.T;
    p.rows = (p.nblocks + 1) * s.Q;
    const int64_t want = s.pass_rows_opt > 0 ? s.pass_rows_opt : SPX_EFFECTS_PASS_ROWS;
    p.pass_rows = std::min<int64_t>(p.rows, want);
    p.npass = (int)((p.rows + p.pass_rows - 1) / p.pass_rows);
    p.gather = p.npass > 1;
    const int64_t ldq = s.Q | 1;
    const int64_t fit = SPX_EFFECTS_LDS_BYTES / (ldq * 8);
    p.mean_lds = fit >= 1;
    p.wg_blocks = p.mean_lds ? (int)std::min<int64_t>(fit, SPX_EFFECTS_THREADS) : SPX_EFFECTS_THREADS;
    p.mean_tiles = (p.nblocks + p.wg_blocks - 1) / p.wg_blocks;
    p.gather_tiles = (s.Q + SPX_EFFECTS_THREADS - 1) / SPX_EFFECTS_THREADS;
    p.lds_bytes = p.mean_lds ? (size_t)p.wg_blocks * ldq * 8 : 0;
    p.in_bytes = ((size_t)s.Q * s.D + (size_t)s.T) * 8;
    p.out_bytes = ((size_t)s.H * p.nblocks + (size_t)s.H * s.Q) * 8;
    p.cand_bytes = (size_t)p.pass_rows * s.D * 8;
    p.gather_bytes = p.gather ? (size_t)s.H * p.rows * 8 : 0;
    return p;
}
