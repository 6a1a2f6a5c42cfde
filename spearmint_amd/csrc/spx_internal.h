// Internal definitions shared by spx_api.hip (single-GPU engine + C ABI) and spx_multi.hip
// (several GPUs behind one handle).  Not installed; include/spx.h is the public surface.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/spx.h"
#include "common.h"
#include "spx_plan.h"
#include "spx_held.h"

std::string& spx_err_slot();            // thread-local last-error text
int spx_fail(int code, const char* fmt, ...);
#define fail spx_fail

#define HIPCHK(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (void)hipGetLastError(); /* reported now: the runtime's sticky copy is cleared */   \
            return fail(SPX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                  \
        }                                                                                     \
    } while (0)

// after a batch of launches: a noted hipFuncSetAttribute refusal first (common.h: SPX_LDS_ATTR), then the runtime's own error
std::string& spx_attr_err_slot();
#define LAUNCHCHK()                                                             \
    do {                                                                        \
        if (!spx_attr_err_slot().empty()) {                                     \
            std::string m_ = spx_attr_err_slot();                               \
            spx_attr_err_slot().clear();                                        \
            (void)hipGetLastError();                                            \
            return fail(SPX_ERR_HIP, "%s", m_.c_str());                         \
        }                                                                       \
        HIPCHK(hipGetLastError());                                              \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool owned = true;      // false: p points into another DevBuf (alias_of): never freed here
    void alias_of(void* q) { if (p && owned) (void)hipFree(p); p = q; cap = 0; owned = false; }
    int reserve(size_t bytes)
    {
        if (!owned) { p = nullptr; cap = 0; owned = true; }
        if (bytes <= cap) return SPX_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();   // reported here; do not leave it for the next call's launch check to find
            return fail(SPX_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        }
        cap = bytes;
        return SPX_OK;
    }
    void release() { if (p && owned) (void)hipFree(p); p = nullptr; cap = 0; owned = true; }
    double* d() const { return (double*)p; }
};

// pinned (page-locked, device-visible) host memory: uploads from it are true asynchronous DMA without a staging copy
// inside the runtime, and a kernel can write a handful of result words straight into it
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return SPX_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        if (bytes < 4096) bytes = 4096;
        // coherent (fine-grained) whatever HIP_HOST_COHERENT says: kernels read hyper rows out of these buffers and store results
        // and completion flags into them that the host watches while the launch is still running (spx_gp_logprob)
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocCoherent);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return fail(SPX_ERR_HIP, "hipHostMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        }
        cap = bytes;
        return SPX_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};


enum Stage {
    ST_SCALE = 0, ST_COV_SELF, ST_CHOL_DIAG, ST_CHOL_PANEL, ST_TRINV, ST_GAMMA_ALPHA,
    ST_COV_CROSS, ST_CROSS_MEAN, ST_PREDICT_GEMM, ST_EI_FINALIZE, ST_MEAN_ARGMAX,
    ST_MES,               // the four kernels of a max-value entropy search pass (launch_mes), as one stage
    ST_EHVI,              // k_ehvi of an expected-hypervolume-improvement pass (launch_ehvi)
    ST_TS_PRIOR,          // spx_thompson: k_ts_prior over the observations and over every candidate chunk (+ k_ts_rhs)
    ST_TS_FINISH,         // ... and k_ts_finish per work item + the two k_ts_argmin launches
    ST_KG,                // a knowledge-gradient pass: k_kg_lines + k_kg_value per work item (and k_kg_mu once)
    ST_FACTOR_TOTAL, ST_EI_RUN_TOTAL, ST_COUNT
};
struct spx_handle {
    int device = 0;
    Options opt;                     // everything spx_set_option writes (spx_plan.h)
    // What the last calls ran (spx_plan.h): decided by plan_factor / plan_ei before anything was queued, read back by
    // gp_logprob_once, spx_get_factor*, the time-out recovery and spx_get_stat.  A call that fails in a reservation or a
    // launch leaves the plan it failed with.
    FactorPlan lean_plan;            // the last log-likelihood factorisation (spx_gp_logprob)
    FactorPlan factor_plan;          // the last EI-path factorisation (spx_factor, spx_ei_step)
    const FactorPlan* last_factor = &factor_plan;   // ... and whichever of the two ran last
    EiPlan ei_plan;                  // the last EI pass
    bool inited = false;
    hipStream_t stream = nullptr;    // main stream (also the only one the factorization uses)
    hipStream_t stream2 = nullptr;   // optional producer stream (option "streams" = 2): K(X*,X) of the next
                                     // work item is generated (VALU) while the GEMM of the current one runs (MFMA)
    hipStream_t stream3 = nullptr;   // option "streams" = 3: K(X*,X) runs AHEAD of the predict GEMM on a low-priority stream, made on the first such pass
    // the staging slots of an EI pass under every stream count (ei_run_impl): K(X*,X) of a work item with its fantasy
    // partials, and the two events of the slot's hand-off; made as passes ask for them
    struct RingSlot { DevBuf Kst, part_bgS; hipEvent_t ready = nullptr, consumed = nullptr; };
    std::vector<RingSlot> ring;
    // a pass's buffers per candidate chunk, by chunk parity: scaled candidates and norms (objective / constraint model),
    // predicted durations, P(feasible); `consumed`: the chunk's last reader is queued on the main stream
    struct ChunkBufs { DevBuf Cs, s2, time_m, con_Cs, con_s2, con_p; hipEvent_t consumed = nullptr; } chunk[2];
    int64_t ring_budget = 0;            // bytes the ring may take (a share of free device memory) ...
    int64_t ring_budget_slot = -1;      // ... as found when the size of a slot last changed
    int corun_launches = 0;             // K(X*,X) launches of the last pass that took k_cov_corun (spx_get_stat "last_corun_launches")
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;   // whole-stage timers (factor / ei_run)
    hipEvent_t ev_fac = nullptr;                   // spx_ei_step: the whole factorisation (alpha included) is done (stream)
    hipEvent_t ev_obs = nullptr, ev_p0 = nullptr;  // spx_ei_step: observations scaled (stream) / a pass's producer work outside the slots done

    int64_t N = 0, M = 0, index_base = 0;
    int D = 0, Dp = 0, Np = 0, H = 0;
    Held held;        // what of all this is resident and valid (spx_held.h); taken away by spx_drop below alone
    int nmodels = 1;  // what FACTOR was built with: 1 = objective GP only, 2 = + log-duration GP
    double best = 0.0;
    int acq = 0;              // SPX_ACQ_*: what the EI pass and the refinement objective compute (spx_set_acquisition) ...
    double acq_par = 0.0;     // ... and its parameter: xi (PI) / kappa (LCB)
    int not_pd_draw = -1, not_pd_pivot = -1;
    int64_t fant_budget = 0;            // bytes the per-fantasy partial means may take (an eighth of free memory, <= 2 GB) ...
    int fant_budget_S = -1;             // ... as found when the number of fantasies last changed
    double* fused_lp = nullptr;         // (spx_gp_logprob -> do_factor: pinned destinations of the fused form's results)
    int* fused_info = nullptr;
    const void* info_clean_ptr = nullptr;   // the not-PD flags at this address ...
    size_t info_clean_bytes = 0;            // ... in a buffer of this size are all zero (left so by the fused launch)
    struct spx_multi* multi = nullptr;  // non-null: this handle fronts several per-GPU handles (spx_multi.hip)
    struct spx_comm* comm = nullptr;    // non-null: one-process-per-GPU communicator attached (spx_comm_attach)

    std::vector<double> hyp_host, thyp_host;
    std::vector<double> up_raw, up_tab;     // host staging of the per-call hyper upload (do_factor)

    DevBuf comp, vals, ldur, cand, hyp, htab;
    DevBuf Xs, X2s, s1, Lm, WT, Dinv, gamma, alpha, info, lp;
    DevBuf part_ss, part_bg, ei_draw, ei_mean, mom_m, mom_v, mom_t;
    DevBuf am_val, am_idx, am_out_val, am_out_idx, scratch;
    // pending-experiment fantasies (spx_set_fantasies): S right-hand sides per draw; S > 0 exactly when FANT is held
    int S = 0;
    DevBuf fantT, gammaS, bests;
    DevBuf alphaS;                 // [H][S][Np] = W^T Gamma_s, built on the first spx_ei_grad_batch after spx_set_fantasies (ALPHA_S)
    // spx_draw_fantasies: the resident fantasies were formed on the device from P trailing pending rows
    bool fant_device = false;
    int fant_P = 0;
    DevBuf fant_z, fant_post, fant_pend, fant_info;   // z as uploaded; C | T | pend_m | min per draw; pend_fant [H][P][S]; pivot flags [H]
    DevBuf pt_x, pt_k, pt_dk, pt_t, pt_z, pt_out, pt_kt, pt_dkt, pt_u;   // spx_ei_grad_batch work vectors
    DevBuf rec_send, rec_recv, rec_out;   // {best mean EI, global index} records of the multi-GPU all-gather
    // 2-D partition with a communicator attached (spx_set_partition): the M_total-vector of EI sums / means
    int part_ph = 1;
    int64_t part_M = 0;            // > 0: the collective is the all-reduce(SUM) of EI sums
    int part_H = 0;
    DevBuf ei_sum_full;
    DevBuf sobol_dirs, sobol_out;                                   // spx_sobol_grid
    // spx_main_effects: base | levels as uploaded; the kept means of several passes gathered [H][rows]; curves | base_mean
    DevBuf eff_in, eff_m, eff_out;
    EffectsPlan effects_plan;                                       // the last spx_main_effects (spx_plan.h)
    // max-value entropy search (SPX_ACQ_MES): partial minima, partial log-survival sums, G [H][J], y* [H][K], fit [H][8] of the
    // last MES pass and its sizes; part of RESULTS (held.results.mes)
    DevBuf mes_bpart, mes_part, mes_G, mes_ystar, mes_fit;
    int mes_K = 0, mes_J = 0;
    // two objectives (SPX_ACQ_EHVI): the front as spx_set_pareto_front received it (FRONT held: front_n >= 0) and as k_ehvi reads
    // it -- [2][front_n + 1]: the strips' upper edges a_1 .. a_n, r1, then their heights' levels r2, b_1 .. b_n; the second GP's
    // internal handle on the same device (SEC / SEC_CAND: what of the caller's data it holds), its moments are the pass's
    int front_n = -1;
    double front_r1 = 0.0, front_r2 = 0.0;
    std::vector<double> front_a, front_b;
    DevBuf front_dev;
    spx_handle* sec = nullptr;
    // Thompson sampling (spx_thompson): frequencies nu [H][F Dp] (operand order) | phase [F] | scale [H] | sig [H]; w and eps as uploaded; the
    // prior at the observations [H][S][N], the right-hand sides [H][S][N] and their Gamma [H][S][Np]; the prior at the candidates
    // and the paths, [H][S][Mp] each; the argmin's partials and results.  ts_S / ts_F: sizes of the held paths (RESULTS with
    // held.results.ts), 0 otherwise
    DevBuf ts_par, ts_w, ts_eps, ts_pobs, ts_rhs, ts_gammaS, ts_pcand, ts_path, ts_am_val, ts_am_idx, ts_out_val, ts_out_idx;
    // spx_thompson_grad_batch: alpha [H][S][Np] = W^T Gamma of every held path (held.results.ts_alpha); the points [P][D] | path_of
    // [P] as uploaded; prior [P] | its gradient [P][D] | dk/dr^2 [P][Np] between the two kernels; {value, prior, grad[D]} per point
    DevBuf ts_alpha, ts_gin, ts_gwork, ts_gout;
    int ts_S = 0, ts_F = 0;
    int64_t ts_fant_budget = 0;    // the per-path partial means' byte budget, as fant_budget / fant_budget_S are the fantasies'
    int ts_fant_budget_S = -1;
    size_t ts_w_stride = 0;        // doubles between the draws' blocks of w (0: shared)
    // knowledge gradient (SPX_ACQ_KG): the representer points as spx_set_kg_points received them (KGPTS held: kg_A >= 1) and on
    // the device; per pass: the points scaled per draw [H][Ap][Dp] and their norms [H][Ap], k(A, X) [H][Ap][Np], the columns
    // gamma | Gamma_a [H][A + 1][Np], mu_a [H][A]; per work item: k(A, c) [Hb][Ap][Mc] and mu_c [Hb][Mc] (the slopes take `scratch`);
    // with the moments kept C [H][A][Mp].  kg_last_A: A of the held KG results (held.results.kg)
    int kg_A = -1, kg_last_A = 0;
    std::vector<double> kg_pts_host;
    DevBuf kg_pts, kg_As, kg_sA, kg_kxa, kg_gammaS, kg_mua, kg_Kac, kg_muc, kg_cov;
    int64_t kg_fant_budget = 0;    // the per-column partial means' byte budget, as fant_budget / fant_budget_S are the fantasies'
    int kg_fant_budget_S = -1;
    DevBuf loo_out;                                                 // spx_loo: loo_mean | loo_var | kinv_diag, [3][H][N]; scratch of that call, not part of `held`
    // probit constraint model (spx_set_constraint_model): an internal handle on the same device factors
    // (amp2_c (K_c + 1e-6 I) + noise_c I) alpha_c = ff over its own Nc points; the EI pass reads its scaled rows and alpha_c
    spx_handle* con = nullptr;
    int64_t con_n = 0;                                              // Nc (0: all valid, P_d = Phi(gain_d))
    std::vector<double> con_tab_host;                               // [H][SPX_HT]: gain, noise_c, amp2_c, amp2_c
    DevBuf con_tab, mom_c;
    // spx_constrained_ei_grad_batch: the objective's hypers over the constraint model's points X_c (the variance of the
    // reference's no-pending refinement objective, GPConstrainedEIChooser.py:692-803) -- a third internal handle, factored
    // on the first call and kept until observations, hypers, the constraint points or option "covar" change
    spx_handle* full = nullptr;
    std::vector<double> con_comp_host;                              // X_c as spx_set_constraint_model received it
    // spx_gp_logprob_rhs: a right-hand side per hyper row, [H][N], read in place of the resident values while set
    DevBuf rhs_rows;
    bool rhs_rows_on = false;
    DevBuf rhs;                                                     // spx_gp_logprob: [H][64][Np] right-hand-side rows
    DevBuf diagL;                                                   // spx_gp_logprob (tile-major path): diag(L), [H][Np]
    DevBuf ps_flags;                                                // k_lean_step_ps: progress of every diagonal block, [H][nblk]
    int64_t flow_fallbacks = 0;                                     // k_lean_flow hand-off time-outs that sent this handle back to one launch per block column
    bool flow_demoted = false;                                      // ... and it is there now (until flow_rearm_after clean factorisations, or option lean_flow)
    int flow_clean = 0;                                             // clean factorisations since the last time-out
    int64_t flow_rearms = 0;                                        // times the handle went back to k_lean_flow
    int ranks_seen = 1;                                             // records in the last all-gather's table (spx_comm_exchange)
    int n_cu = 256;                                                 // compute units of the device (ensure_init)
    DevBuf flow_flags;                                              // k_lean_flow: [H][nblk + 1][nblk] tile flags + [H][nblk] diagonal progress + the ticket and done counters
    size_t flow_flags_n = 0;                                        // ints the flags were zeroed for
    int flow_gen = 0;                                               // generation of the last call (flags are compared, not cleared)
    PinBuf pin_stage;                                               // staging of the callers' small host buffers (stage_h2d / stage_d2h in spx_api.hip)
    size_t stage_off = 0;
    PinBuf pin_up, pin_res;                                         // hyper-parameter upload staging; log-likelihood results
    bool handoff_timeout = false;                                   // finish_factor saw info < 0

    double best_val = 0.0;
    int64_t best_idx = -1;

    struct Ev { hipEvent_t a, b; int stage; };
    std::vector<Ev> ev_pool;
    size_t ev_used = 0;
    double st_ms[ST_COUNT] = {0};
    int64_t st_n[ST_COUNT] = {0};
};

// Take x, and everything made from it, away from the handle: the bits, and the data that means nothing without them.  Every
// entry point calls this for what it is about to overwrite BEFORE its first mutation and sets it again after its last check.
inline void spx_drop(spx_handle* h, Held::Thing x)
{
    const Held was = h->held;
    h->held.drop(x);
    if (was.has(Held::FANT) && !h->held.has(Held::FANT)) { h->S = 0; h->fant_P = 0; h->fant_device = false; }
    if (was.has(Held::FACTOR) && !h->held.has(Held::FACTOR)) h->nmodels = 1;
}
// ... and give it back; a refusal means that an entry point set a product without what it is made from
inline int spx_hold(spx_handle* h, Held::Thing x, Held::Results r = Held::Results())
{
    return h->held.set(x, r) ? SPX_OK : spx_fail(SPX_ERR_ARG, "internal error: thing %d set without what it is made from", (int)x);
}

// ---- several GPUs behind one handle (spx_multi.hip) --------------------------------------------
struct spx_multi;
void spx_multi_destroy(spx_multi* m);
int spx_multi_set_option(spx_multi* m, const char* name, int64_t value);
int spx_multi_set_acquisition(spx_multi* m, int32_t kind, double par);
int spx_multi_get_acquisition(spx_multi* m, int32_t* kind, double* par);
int spx_multi_set_observations(spx_multi* m, const double* comp, const double* vals, int64_t N, int32_t D);
int spx_multi_set_candidates(spx_multi* m, const double* cand, int64_t M, int32_t D, int64_t index_base);
int spx_multi_set_hypers(spx_multi* m, const double* hypers, int32_t H);
int spx_multi_set_time_model(spx_multi* m, const double* log_durs, const double* time_hypers);
int spx_multi_factor(spx_multi* m);
int spx_multi_set_fantasies(spx_multi* m, const double* fant, const double* bests, int32_t S);
int spx_multi_draw_fantasies(spx_multi* m, int32_t P, const double* z, int32_t per_draw, int32_t S);
int spx_multi_get_pending_fantasies(spx_multi* m, int32_t draw, double* pend_fant, double* bests);
int spx_multi_ei_run(spx_multi* m, int32_t flags);
int spx_multi_get_best(spx_multi* m, int64_t* best_idx, double* best_val);
int spx_multi_get_ei_mean(spx_multi* m, double* out);
int spx_multi_get_ei_draws(spx_multi* m, double* out);
int spx_multi_get_moments(spx_multi* m, int32_t draw, double* func_m, double* func_v);
int spx_multi_get_time_mean(spx_multi* m, int32_t draw, double* out);
int spx_multi_get_factor(spx_multi* m, int32_t draw, double* K, double* L, double* alpha);
int spx_multi_get_factor_rows(spx_multi* m, int32_t draw, int64_t row0, int64_t nrows, double* L_rows, double* gamma);
int spx_multi_get_cross_cov(spx_multi* m, int32_t draw, int64_t c0, int64_t nc, double* out);
int spx_multi_gp_logprob(spx_multi* m, double* out);
int spx_multi_ei_grad_batch(spx_multi* m, const double* points, int32_t P, double* neg_ei, double* grad);
int spx_multi_sobol_grid(spx_multi* m, const uint32_t* dirs, int32_t dim_max, int32_t dim, int64_t n,
                         int64_t skip, double* grid_out, int32_t as_candidates, double* kernel_ms);
int spx_multi_not_pd_info(spx_multi* m, int32_t* draw, int32_t* pivot);
int spx_multi_get_timings(spx_multi* m, double* ms, int64_t* launches, int n);
int spx_multi_stat(spx_multi* m, const char* name, int64_t* value);
int spx_multi_info(spx_multi* m, int32_t* n_dev, int32_t* transport, int32_t* device_ids, int32_t cap);
// one process per GPU (spx_comm_attach): exchange this handle's record with the other ranks / drop the communicator
int spx_comm_exchange(spx_handle* h, bool* global_2d);
void spx_comm_release(spx_handle* h);
// single-GPU pieces the multi layer needs
int spx_ensure_init(spx_handle* h);
