// libspx host side: handle, device buffers, kernel orchestration, C ABI (include/spx.h).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include <chrono>

#include "spx_internal.h"
#include "np_sum.h"
#include "ts_device.h"   // SPX_TS_TWO_PI

#define SPX_VERSION 200

static const char* kStageNames[ST_COUNT] = {
    "scale_rows", "cov_self", "chol_diag", "chol_panel", "trinv", "gamma_alpha",
    "cov_cross", "cross_mean", "predict_gemm", "ei_finalize", "mean_argmax", "mes", "ehvi",
    "ts_prior", "ts_finish", "kg", "factor_total", "ei_run_total"};


std::string& spx_err_slot()
{
    static thread_local std::string g_err;
    return g_err;
}

std::string& spx_attr_err_slot()
{
    static thread_local std::string g_attr;
    return g_attr;
}

void spx_note_attr_error(const char* kernel, size_t lds_bytes, hipError_t e)
{
    char buf[384];
    snprintf(buf, sizeof buf, "hipFuncSetAttribute(%s, MaxDynamicSharedMemorySize = %zu) failed: %s", kernel, lds_bytes,
             hipGetErrorString(e));
    (void)hipGetLastError();
    if (spx_attr_err_slot().empty()) spx_attr_err_slot() = buf;   // the first one is the cause
}

int spx_fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    spx_err_slot() = buf;
    // a hipFuncSetAttribute refusal noted during THIS call (SPX_LDS_ATTR) and not yet reported by a LAUNCHCHK must not
    // outlive the call: the next launch check on this thread, for another handle, would name a kernel it never launched
    if (!spx_attr_err_slot().empty()) {
        spx_err_slot() += " [also: " + spx_attr_err_slot() + "]";
        spx_attr_err_slot().clear();
    }
    return code;
}

static int ensure_init(spx_handle* h)
{
    HIPCHK(hipSetDevice(h->device));
    if (!h->inited) {
        // the main stream (factorisation, predict GEMM, EI) at the device's highest priority, the K(X*,X) producer of option
        // streams = 3 (ensure_stream3) at its lowest: a place that comes free on a CU goes to a waiting GEMM workgroup first
        int prio_least = 0, prio_greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = prio_greatest = 0; }
        HIPCHK(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prio_greatest));
        HIPCHK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
        for (auto& cb : h->chunk) HIPCHK(hipEventCreateWithFlags(&cb.consumed, hipEventDisableTiming));
        HIPCHK(hipEventCreate(&h->ev_t0));
        HIPCHK(hipEventCreate(&h->ev_t1));
        HIPCHK(hipEventCreateWithFlags(&h->ev_obs, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_p0, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_fac, hipEventDisableTiming));
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && ncu > 0) h->n_cu = ncu;
        h->inited = true;
    }
    return SPX_OK;
}

// option streams = 3: the producer stream
static int ensure_stream3(spx_handle* h)
{
    if (h->stream3) return SPX_OK;
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = prio_greatest = 0; }
    HIPCHK(hipStreamCreateWithPriority(&h->stream3, hipStreamNonBlocking, prio_least));
    return SPX_OK;
}
// `n` staging slots (events only: the buffers are reserved by the pass)
static int ensure_slots(spx_handle* h, int n)
{
    while ((int)h->ring.size() < n) {
        spx_handle::RingSlot sl;
        HIPCHK(hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming));
        hipError_t e = hipEventCreateWithFlags(&sl.consumed, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipEventDestroy(sl.ready);
            (void)hipGetLastError();
            return fail(SPX_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        h->ring.push_back(sl);
    }
    return SPX_OK;
}
// record `ev` on `from` and make `to` wait for it: what `from` has queued so far is done before what `to` queues from here
// on; nothing when they are one stream
static int hand_off(hipStream_t from, hipStream_t to, hipEvent_t ev)
{
    if (from == to) return SPX_OK;
    HIPCHK(hipEventRecord(ev, from));
    HIPCHK(hipStreamWaitEvent(to, ev, 0));
    return SPX_OK;
}

static int ev_begin(spx_handle* h, int stage, hipStream_t strm)
{
    if (!h->opt.timing) return -1;
    if (h->ev_used == h->ev_pool.size()) {
        spx_handle::Ev e;
        if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return -1;
        h->ev_pool.push_back(e);
    }
    spx_handle::Ev& e = h->ev_pool[h->ev_used];
    e.stage = stage;
    (void)hipEventRecord(e.a, strm);
    return (int)h->ev_used++;
}
static void ev_end(spx_handle* h, int id, hipStream_t strm)
{
    if (id >= 0) (void)hipEventRecord(h->ev_pool[id].b, strm);
}
static void ev_collect(spx_handle* h)
{
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev_pool[i].a, h->ev_pool[i].b) == hipSuccess) {
            h->st_ms[h->ev_pool[i].stage] += ms;
            h->st_n[h->ev_pool[i].stage] += 1;
        }
    }
    h->ev_used = 0;
}
#define TIMED_S(stage, strm, stmt)              \
    do {                                        \
        int ev_ = ev_begin(h, stage, strm);     \
        stmt;                                   \
        ev_end(h, ev_, strm);                   \
    } while (0)
#define TIMED(stage, stmt) TIMED_S(stage, h->stream, stmt)

int spx_ensure_init(spx_handle* h) { return ensure_init(h); }

// kernel-level correlation kind of a handle: SE runs as ARDSE on unit length scales (do_factor substitutes them)
static inline int dev_kind(const spx_handle* h) { return h->opt.cov_kind == SPX_COVAR_SE ? SPX_COV_ARDSE : h->opt.cov_kind; }
// the EI path's factor is tile-major (k_lean_flow made it) -- false again once a log-likelihood call has overwritten it
static inline bool factor_tiled(const spx_handle* h) { return !h->last_factor->lean && h->last_factor->flow; }

// ---- options: one table.  The tri-state and clamped-integer kinds are served by it, the others by the handlers above it ----
static int opt_kstar_budget(spx_handle* h, int64_t value)
{
    h->opt.kst_budget = value > 0 ? value : (512ll << 20);
    return SPX_OK;
}
static int opt_effects_pass_rows(spx_handle* h, int64_t value)
{
    h->opt.effects_pass_rows = value > 0 ? value : 0;
    return SPX_OK;
}
static int opt_gemm_waves(spx_handle* h, int64_t value)
{
    if (!predict_gemm_variant_ok((int)value))
        return fail(SPX_ERR_ARG, "spx_set_option: gemm_waves=%lld is not a variant of this build", (long long)value);
    h->opt.gemm_variant = (int)value;
    return SPX_OK;
}
static int opt_covar(spx_handle* h, int64_t value)
{
    if (value < SPX_COVAR_MATERN52 || value > SPX_COVAR_SE)
        return fail(SPX_ERR_ARG, "spx_set_option: covar=%lld is not one of SPX_COVAR_*", (long long)value);
    if (h->opt.cov_kind == (int)value) return SPX_OK;
    h->opt.cov_kind = (int)value;
    spx_drop(h, Held::COVAR);         // the three factorisations and what was made from them
    // the internal handles follow at once: their factors, scaled rows and (SE) unit length scales belong to the old kernel
    if (h->con) opt_covar(h->con, value);
    if (h->full) opt_covar(h->full, value);
    return SPX_OK;
}
static int opt_lean_flow(spx_handle* h, int64_t value)
{
    h->opt.lean_flow = value < 0 ? -1 : (value != 0);
    h->flow_demoted = false;        // asking again re-arms a handle that a hand-off time-out had sent to the launches
    h->flow_clean = 0;
    return SPX_OK;
}
static int opt_streams(spx_handle* h, int64_t value)
{
    h->opt.nstreams = (value == 2 || value == 3) ? (int)value : 1;
    return SPX_OK;
}
// J of a max-value entropy search pass; the y* table of the last one was fitted on the old grid and goes with its results
static int opt_mes_grid(spx_handle* h, int64_t value)
{
    if (value < 8 || value > 4096)
        return fail(SPX_ERR_ARG, "spx_set_option: mes_grid=%lld probe values (allowed: 8 .. 4096)", (long long)value);
    spx_drop(h, Held::RESULTS);
    h->opt.mes_grid = (int)value;
    return SPX_OK;
}
static int opt_timing(spx_handle* h, int64_t value)
{
    h->opt.timing = value != 0;
    memset(h->st_ms, 0, sizeof h->st_ms);
    memset(h->st_n, 0, sizeof h->st_n);
    return SPX_OK;
}

struct OptRow {
    const char* name;
    int Options::* member;                  // tri-state: value < 0 ? -1 : (value != 0) ...
    int neg, max;                           // ... or, max > 0, a clamped integer: value < 0 ? neg : min(value, max)
    int (*call)(spx_handle*, int64_t);      // ... or a handler
};
#define OPT_TRI(name, member) {name, &Options::member, 0, 0, nullptr}
#define OPT_CLAMP(name, member, neg, max) {name, &Options::member, neg, max, nullptr}
#define OPT_CALL(name, fn) {name, nullptr, 0, 0, fn}
static const OptRow kOptions[] = {
    OPT_CALL("kstar_budget_bytes", opt_kstar_budget),   // K(X*,X) staging buffer per stream (0 = default, 512 MiB)
    OPT_CALL("effects_pass_rows", opt_effects_pass_rows),   // spx_main_effects: structured rows per grid pass (0 = default, 2^20); same bits for every value
    OPT_CALL("gemm_waves", opt_gemm_waves),             // predict-GEMM variant of this handle (predict_kernels.hip)
    OPT_CALL("covar", opt_covar),                       // SPX_COVAR_*: the reference's covar= (gp.py:87-132)
    OPT_TRI("lean_lazy", lean_lazy),                    // log-likelihood path: trailing updates two steps at a time (1), one (0), by size (-1, default)
    OPT_TRI("step_overlap", step_overlap),              // spx_ei_step: candidate scaling + first K(X*,X) on the second stream beside the factorisation (1, default) or behind it (0)
    OPT_TRI("ei_fused", ei_fused),                      // N <= 128, no fantasies: K* -> beta -> EI of a chunk in one kernel (1, default) or the general three-stage path (0)
    OPT_TRI("ei_flow", ei_flow),                        // spx_factor through k_lean_flow (1, default), the left-looking launches (0)
    OPT_TRI("lean_flow_cov", lean_flow_cov),            // k_lean_flow builds K(X,X) tile by tile itself (1, default) or reads k_cov's (0)
    OPT_TRI("lean_flow_yield", lean_flow_yield),        // k_lean_flow, two workgroups per CU: yield to a neighbour's diagonal block (1, default) or not (0)
    OPT_TRI("lean_flow_cu", lean_flow_cu),              // k_lean_flow: one workgroup per CU (1), two (0), by size (-1, default)
    OPT_CALL("lean_flow", opt_lean_flow),               // log-likelihood path: the whole factorisation as ONE data-flow launch (1, default), one launch per block column (0)
    OPT_CLAMP("flow_rearm_after", flow_rearm_after, 16, 1 << 30),   // clean factorisations after a hand-off time-out before k_lean_flow is tried again (default 16; 0 = never)
    OPT_CLAMP("flow_spin_limit", flow_spin_limit, 0, 1 << 30),      // polls a k_lean_flow workgroup waits for a hand-off before it gives up (0 = default, 2^20); tests set 1 to see a time-out
    OPT_TRI("lean_ps", lean_ps),                        // log-likelihood path: panel solve pipelined inside the step launch (1, default), separate launch (0)
    OPT_TRI("lean_merge", lean_merge),                  // log-likelihood path: observation scaling and the right-hand-side rows in one launch (1, default) or two (0)
    OPT_TRI("lean_one", lean_one),                      // spx_gp_logprob as one launch (1, default) or prologue + k_lean_flow + reduction (0): same bits
    OPT_TRI("lean_poll", lean_poll),                    // the one-launch call's results are awaited by polling their pinned flags (1, default) instead of hipStreamSynchronize (0)
    OPT_TRI("lean_zc", lean_zc),                        // the one-launch call reads the hyper rows from the pinned staging buffer itself (1, default) instead of behind a host-to-device copy (0)
    OPT_TRI("stage_copies", stage_copies),              // callers' small host buffers through the handle's page-locked staging buffer (1, default) or handed to the runtime as they are (0)
    OPT_TRI("cov_flat", cov_flat),                      // K(X*,X) launches of several residency rounds: equal contiguous shares (k_cov_flat; 1, default) or the 3-D grid (0)
    OPT_TRI("gemm_partial", gemm_partial),              // N not a multiple of 128: skip the padding's K steps / row tiles / K* rows (1, default) or compute them (0)
    OPT_CALL("streams", opt_streams),                   // 1 = everything on one stream (default), 2 = alternate EI work items, 3 = K(X*,X) ahead of the GEMM through a ring
    OPT_CLAMP("kstar_ring", ring_opt, 0, 4096),         // streams = 3: staging slots of the ring (0, default: as many as the byte budget holds)
    OPT_TRI("kstar_corun", corun_opt),                  // streams = 3: K(X*,X) launches beside a GEMM in the form that fits there (1, default) or as k_cov_flat (0); same bits
    OPT_CALL("mes_grid", opt_mes_grid),                 // SPX_ACQ_MES: probe values J of the log-survival grid (default 256, 8 .. 4096); drops the last pass's results
    OPT_CALL("timing", opt_timing),                     // per-launch HIP events on the handle's stream; (re)starts the accumulators
};

extern "C" {

int spx_version(void) { return SPX_VERSION; }
const char* spx_last_error(void) { return spx_err_slot().c_str(); }

int spx_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(SPX_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int spx_create(int device_id, spx_handle** out)
{
    if (!out || device_id < 0) return fail(SPX_ERR_ARG, "spx_create: bad arguments");
    spx_handle* h = new spx_handle();
    h->device = device_id;
    *out = h;
    return SPX_OK;
}

void spx_destroy(spx_handle* h)
{
    if (!h) return;
    if (h->multi) { spx_multi_destroy(h->multi); delete h; return; }
    spx_comm_release(h);
    if (h->con) { spx_destroy(h->con); h->con = nullptr; }
    if (h->full) { spx_destroy(h->full); h->full = nullptr; }
    if (h->sec) { spx_destroy(h->sec); h->sec = nullptr; }
    if (h->inited) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->stream2);
        if (h->stream3) (void)hipStreamSynchronize(h->stream3);
        for (auto& sl : h->ring) {
            sl.Kst.release();
            sl.part_bgS.release();
            (void)hipEventDestroy(sl.ready);
            (void)hipEventDestroy(sl.consumed);
        }
        h->ring.clear();
        if (h->stream3) (void)hipStreamDestroy(h->stream3);
        for (auto& cb : h->chunk) {
            for (DevBuf* b : {&cb.Cs, &cb.s2, &cb.time_m, &cb.con_Cs, &cb.con_s2, &cb.con_p}) b->release();
            (void)hipEventDestroy(cb.consumed);
        }
        DevBuf* bufs[] = {&h->comp, &h->vals, &h->ldur, &h->cand, &h->hyp, &h->htab, &h->Xs, &h->X2s,
                          &h->s1, &h->Lm, &h->WT, &h->Dinv, &h->gamma, &h->alpha, &h->info, &h->lp, &h->part_ss, &h->part_bg,
                          &h->fantT, &h->gammaS, &h->bests, &h->fant_z, &h->fant_post, &h->fant_pend, &h->fant_info,
                          &h->pt_x, &h->pt_k, &h->pt_dk, &h->pt_t, &h->pt_z, &h->pt_out, &h->pt_kt, &h->pt_dkt,
                          &h->ei_draw, &h->ei_mean, &h->mom_m, &h->mom_v, &h->mom_t, &h->am_val, &h->am_idx,
                          &h->am_out_val, &h->am_out_idx, &h->scratch, &h->sobol_dirs, &h->sobol_out, &h->rhs, &h->diagL, &h->ps_flags, &h->flow_flags,
                          &h->alphaS, &h->pt_u, &h->rec_send, &h->rec_recv, &h->rec_out, &h->ei_sum_full,
                          &h->con_tab, &h->mom_c, &h->rhs_rows, &h->eff_in, &h->eff_m, &h->eff_out, &h->loo_out,
                          &h->mes_bpart, &h->mes_part, &h->mes_G, &h->mes_ystar, &h->mes_fit, &h->front_dev,
                          &h->ts_par, &h->ts_w, &h->ts_eps, &h->ts_pobs, &h->ts_rhs, &h->ts_gammaS, &h->ts_pcand, &h->ts_path,
                          &h->ts_am_val, &h->ts_am_idx, &h->ts_out_val, &h->ts_out_idx,
                          &h->ts_alpha, &h->ts_gin, &h->ts_gwork, &h->ts_gout,
                          &h->kg_pts, &h->kg_As, &h->kg_sA, &h->kg_kxa, &h->kg_gammaS, &h->kg_mua, &h->kg_Kac, &h->kg_muc, &h->kg_cov};
        for (DevBuf* b : bufs) b->release();
        h->pin_up.release();
        h->pin_res.release();
        h->pin_stage.release();
        for (auto& e : h->ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
        (void)hipEventDestroy(h->ev_t0);
        (void)hipEventDestroy(h->ev_t1);
        (void)hipEventDestroy(h->ev_obs);
        (void)hipEventDestroy(h->ev_p0);
        (void)hipEventDestroy(h->ev_fac);
        (void)hipStreamDestroy(h->stream);
        (void)hipStreamDestroy(h->stream2);
    }
    delete h;
}

int spx_set_option(spx_handle* h, const char* name, int64_t value)
{
    if (!h || !name) return fail(SPX_ERR_ARG, "spx_set_option: null");
    if (h->multi) return spx_multi_set_option(h->multi, name, value);
    for (const OptRow& r : kOptions) {
        if (strcmp(name, r.name)) continue;
        if (r.call) {
            const int rc = r.call(h, value);
            if (rc) return rc;
        } else {
            h->opt.*r.member = r.max ? (value < 0 ? r.neg : (int)std::min<int64_t>(value, r.max)) : (value < 0 ? -1 : (value != 0));
        }
        // the second GP of an EHVI pass runs with the caller's options (its timers are not the caller's)
        if (h->sec && strcmp(name, "timing")) (void)spx_set_option(h->sec, name, value);
        return SPX_OK;
    }
    return fail(SPX_ERR_ARG, "spx_set_option: unknown option '%s'", name);
}

// The acquisition every later pass and refinement call computes in EI's place (spx.h).  Nothing but the results of the last
// pass depends on it: the factor, the fantasies and alpha_s stay.
static_assert(SPX_ACQ_EI == SPX_ACQ_DEV_EI && SPX_ACQ_PI == SPX_ACQ_DEV_PI && SPX_ACQ_LCB == SPX_ACQ_DEV_LCB
                  && SPX_ACQ_MES == SPX_ACQ_DEV_MES && SPX_ACQ_EHVI == SPX_ACQ_DEV_EHVI && SPX_ACQ_KG == SPX_ACQ_DEV_KG,
              "spx.h and common.h number the acquisitions alike");
int spx_set_acquisition(spx_handle* h, int32_t kind, double par)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_set_acquisition: null handle");
    if (kind != SPX_ACQ_EI && kind != SPX_ACQ_PI && kind != SPX_ACQ_LCB && kind != SPX_ACQ_MES && kind != SPX_ACQ_EHVI
        && kind != SPX_ACQ_KG)
        return fail(SPX_ERR_ARG, "spx_set_acquisition: unknown acquisition %d (SPX_ACQ_EI, SPX_ACQ_PI, SPX_ACQ_LCB, SPX_ACQ_MES, "
                                 "SPX_ACQ_EHVI, SPX_ACQ_KG are known)", (int)kind);
    if (!(par >= 0.0) || !std::isfinite(par))
        return fail(SPX_ERR_ARG, "spx_set_acquisition: the parameter must be finite and >= 0 (got %g)", par);
    if (kind == SPX_ACQ_EI && par != 0.0)
        return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_EI takes no parameter (par must be 0, got %g)", par);
    if (kind == SPX_ACQ_MES) {
        if (!(par >= 1.0 && par <= 1024.0) || par != std::floor(par))
            return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_MES takes par = K, the number of y* levels, an integer in "
                                     "1 .. 1024 (got %g)", par);
        // y* of a draw needs the moments of every candidate of the pass: one device holds them all, or it is refused
        if (h->multi) return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_MES is single-device only (multi-device handle)");
        if (h->comm) return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_MES is single-device only (communicator attached)");
        if (h->part_ph > 1 || h->part_M > 0)
            return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_MES is not available with a 2-D partition");
    }
    if (kind == SPX_ACQ_EHVI) {
        if (par != 0.0)
            return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_EHVI takes no parameter (par must be 0, got %g)", par);
        // the second GP's moments of every candidate live on an internal handle of the same device
        if (h->multi) return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_EHVI is single-device only (multi-device handle)");
        if (h->comm) return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_EHVI is single-device only (communicator attached)");
        if (h->part_ph > 1 || h->part_M > 0)
            return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_EHVI is not available with a 2-D partition");
    }
    if (kind == SPX_ACQ_KG) {
        if (par != 0.0)
            return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_KG takes no parameter (par must be 0, got %g)", par);
        // the representer points' columns and mu_a live on one device
        if (h->multi) return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_KG is single-device only (multi-device handle)");
        if (h->comm) return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_KG is single-device only (communicator attached)");
        if (h->part_ph > 1 || h->part_M > 0)
            return fail(SPX_ERR_ARG, "spx_set_acquisition: SPX_ACQ_KG is not available with a 2-D partition");
    }
    if (h->multi) return spx_multi_set_acquisition(h->multi, kind, par);
    spx_drop(h, Held::RESULTS);
    h->acq = kind;
    h->acq_par = par;
    return SPX_OK;
}

int spx_get_acquisition(spx_handle* h, int32_t* kind, double* par)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_get_acquisition: null handle");
    if (h->multi) return spx_multi_get_acquisition(h->multi, kind, par);
    if (kind) *kind = h->acq;
    if (par) *par = h->acq_par;
    return SPX_OK;
}

// Copies between a CALLER's host buffer and the device.  The runtime's own path for pageable host memory (a pool of staging
// chunks) stalls for 13-28 ms every few dozen small copies on this stack (profiles/r06_set_obs_spikes.log: one
// spx_set_observations in five, median 0.03 ms) -- at Spearmint's operating sizes that is a whole next().  Buffers up to
// SPX_STAGE_MAX go through the handle's own page-locked staging buffer instead (one host memcpy; larger ones are pinned in place by
// the runtime, which does not show the stall).  stage_begin() at the start of an entry point (the stream is idle: every entry
// point that copies synchronises before it returns); a host-to-device copy is queued on `s`, the caller synchronises as before.
#define SPX_STAGE_MAX (8u << 20)
static void stage_begin(spx_handle* h) { h->stage_off = 0; }
static int stage_h2d(spx_handle* h, void* dst, const void* src, size_t bytes, hipStream_t s)
{
    if (h->opt.stage_copies == 0 || bytes > SPX_STAGE_MAX || h->stage_off + bytes > 4 * (size_t)SPX_STAGE_MAX) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        return SPX_OK;
    }
    if (h->pin_stage.cap < h->stage_off + bytes) {
        if (h->stage_off) {           // (growing would move what earlier copies of this call still read)
            HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
            return SPX_OK;
        }
        int rc = h->pin_stage.reserve(bytes > (1u << 20) ? bytes : (1u << 20));
        if (rc) return rc;
    }
    char* st = (char*)h->pin_stage.p + h->stage_off;
    memcpy(st, src, bytes);
    h->stage_off += (bytes + 255) & ~(size_t)255;
    HIPCHK(hipMemcpyAsync(dst, st, bytes, hipMemcpyHostToDevice, s));
    return SPX_OK;
}
// device -> caller's buffer, complete on return (the stream is synchronised)
static int stage_d2h(spx_handle* h, void* dst, const void* src, size_t bytes, hipStream_t s)
{
    if (h->opt.stage_copies == 0 || bytes > SPX_STAGE_MAX) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return SPX_OK;
    }
    HIPCHK(hipStreamSynchronize(s));     // (nothing queued may still read the staging buffer)
    int rc = h->pin_stage.reserve(bytes > (1u << 20) ? bytes : (1u << 20));
    if (rc) return rc;
    h->stage_off = 0;
    HIPCHK(hipMemcpyAsync(h->pin_stage.p, src, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(dst, h->pin_stage.p, bytes);
    return SPX_OK;
}

int spx_set_observations(spx_handle* h, const double* comp, const double* vals, int64_t N, int32_t D)
{
    if (h && h->multi) return spx_multi_set_observations(h->multi, comp, vals, N, D);
    if (!h || !comp || !vals || N < 1 || D < 1 || N > (1 << 20))
        return fail(SPX_ERR_ARG, "spx_set_observations: bad arguments (N=%lld, D=%d)", (long long)N, D);
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::OBS);
    if (D != h->D) { spx_drop(h, Held::CAND); spx_drop(h, Held::HYP); }   // (candidates and hypers of another dimension)
    if (D != h->D && h->held.has(Held::KGPTS)) { spx_drop(h, Held::KGPTS); h->kg_A = -1; h->kg_pts_host.clear(); }   // (and representer points)
    h->N = N; h->D = D; h->Dp = padded_dim(D); h->Np = (int)round_up(N, SPX_PADN);
    if ((rc = h->comp.reserve((size_t)N * D * 8))) return rc;
    if ((rc = h->vals.reserve((size_t)N * 8))) return rc;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->comp.p, comp, (size_t)N * D * 8, h->stream))) return rc;
    if ((rc = stage_h2d(h, h->vals.p, vals, (size_t)N * 8, h->stream))) return rc;
    double b = vals[0];
    for (int64_t i = 1; i < N; ++i) {  // np.min semantics: NaN propagates
        if (vals[i] != vals[i]) { b = vals[i]; break; }
        if (vals[i] < b) b = vals[i];
    }
    h->best = b;
    HIPCHK(hipStreamSynchronize(h->stream));
    return spx_hold(h, Held::OBS);
}

int spx_set_candidates(spx_handle* h, const double* cand, int64_t M, int32_t D, int64_t index_base)
{
    if (h && h->multi) return spx_multi_set_candidates(h->multi, cand, M, D, index_base);
    if (!h || !cand || M < 1 || D < 1)
        return fail(SPX_ERR_ARG, "spx_set_candidates: bad arguments (M=%lld, D=%d)", (long long)M, D);
    if (h->held.has(Held::OBS) && D != h->D)
        return fail(SPX_ERR_ARG, "spx_set_candidates: D=%d but observations have D=%d", D, h->D);
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::CAND);
    if (!h->held.has(Held::OBS)) {
        if (D != h->D && h->held.has(Held::KGPTS)) { spx_drop(h, Held::KGPTS); h->kg_A = -1; h->kg_pts_host.clear(); }
        h->D = D; h->Dp = padded_dim(D);
    }
    h->M = M; h->index_base = index_base;
    if ((rc = h->cand.reserve((size_t)M * D * 8))) return rc;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->cand.p, cand, (size_t)M * D * 8, h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return spx_hold(h, Held::CAND);
}

int spx_set_hypers(spx_handle* h, const double* hypers, int32_t H)
{
    if (h && h->multi) return spx_multi_set_hypers(h->multi, hypers, H);
    if (!h || !hypers || H < 1) return fail(SPX_ERR_ARG, "spx_set_hypers: bad arguments (H=%d)", H);
    if (H > NP_PAIRWISE_MAX_N)   // the mean over draws walks numpy's pairwise tree with fixed-depth stacks (np_sum.h)
        return fail(SPX_ERR_ARG, "spx_set_hypers: at most %d hyper-parameter draws (got %d)", NP_PAIRWISE_MAX_N, H);
    if (!h->held.has(Held::OBS)) return fail(SPX_ERR_ARG, "spx_set_hypers: call spx_set_observations first");
    spx_drop(h, Held::HYP);
    h->H = H;
    h->hyp_host.assign(hypers, hypers + (size_t)H * (3 + h->D));
    return spx_hold(h, Held::HYP);
}

int spx_set_time_model(spx_handle* h, const double* log_durs, const double* time_hypers)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_set_time_model: null handle");
    if (h->multi) return spx_multi_set_time_model(h->multi, log_durs, time_hypers);
    if (!log_durs || !time_hypers) { spx_drop(h, Held::TIME); return SPX_OK; }
    if (!h->held.has(Held::OBS) || !h->held.has(Held::HYP))
        return fail(SPX_ERR_ARG, "spx_set_time_model: set observations and hypers first");
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::TIME);
    if ((rc = h->ldur.reserve((size_t)h->N * 8))) return rc;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->ldur.p, log_durs, (size_t)h->N * 8, h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->thyp_host.assign(time_hypers, time_hypers + (size_t)h->H * (3 + h->D));
    return spx_hold(h, Held::TIME);
}

// The Pareto front of an EHVI pass (spx.h): a setting of the handle.  Everything is checked before anything is touched; the
// device copy is in k_ehvi's form, n + 1 strips: their upper edges a_1 .. a_n, r1 and their levels r2, b_1 .. b_n.
int spx_set_pareto_front(spx_handle* h, const double* a, const double* b, int32_t n, double r1, double r2)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_set_pareto_front: null handle");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_set_pareto_front: SPX_ACQ_EHVI is single-device only (multi-device handle)");
    if (n < 0) { spx_drop(h, Held::FRONT); h->front_n = -1; h->front_a.clear(); h->front_b.clear(); return SPX_OK; }
    if (n > SPX_MAX_FRONT) return fail(SPX_ERR_ARG, "spx_set_pareto_front: n=%d front points (allowed: 0 .. %d)", (int)n, SPX_MAX_FRONT);
    if (n > 0 && (!a || !b)) return fail(SPX_ERR_ARG, "spx_set_pareto_front: null front with n=%d", (int)n);
    if (!std::isfinite(r1) || !std::isfinite(r2))
        return fail(SPX_ERR_ARG, "spx_set_pareto_front: the reference point must be finite (got %g, %g)", r1, r2);
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(a[i]) || !std::isfinite(b[i]))
            return fail(SPX_ERR_ARG, "spx_set_pareto_front: front point %d is not finite (%g, %g)", i, a[i], b[i]);
        if (i > 0 && !(a[i - 1] < a[i]))
            return fail(SPX_ERR_ARG, "spx_set_pareto_front: the first objective must be strictly increasing (point %d)", i);
        if (i > 0 && !(b[i - 1] > b[i]))
            return fail(SPX_ERR_ARG, "spx_set_pareto_front: the second objective must be strictly decreasing (point %d)", i);
    }
    if (n > 0 && (!(a[n - 1] < r1) || !(b[0] < r2)))
        return fail(SPX_ERR_ARG, "spx_set_pareto_front: the reference point (%g, %g) must lie beyond every front point", r1, r2);
    int rc = ensure_init(h);
    if (rc) return rc;
    std::vector<double> strips(2 * ((size_t)n + 1));
    for (int i = 0; i < n; ++i) { strips[i] = a[i]; strips[(size_t)n + 2 + i] = b[i]; }
    strips[n] = r1;
    strips[(size_t)n + 1] = r2;
    // (a reservation that fails has released the old buffer: the front it belonged to goes first)
    spx_drop(h, Held::FRONT);
    h->front_n = -1;
    if ((rc = h->front_dev.reserve(strips.size() * 8))) return rc;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->front_dev.p, strips.data(), strips.size() * 8, h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->front_a.assign(a, a + n);
    h->front_b.assign(b, b + n);
    h->front_r1 = r1; h->front_r2 = r2; h->front_n = n;
    return spx_hold(h, Held::FRONT);
}

int spx_get_pareto_front(spx_handle* h, double* a, double* b, int32_t* n, double* r1, double* r2)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_get_pareto_front: null handle");
    const bool have = !h->multi && h->held.has(Held::FRONT);
    if (n) *n = have ? h->front_n : -1;
    if (!have) return SPX_OK;
    if (a) std::copy(h->front_a.begin(), h->front_a.end(), a);
    if (b) std::copy(h->front_b.begin(), h->front_b.end(), b);
    if (r1) *r1 = h->front_r1;
    if (r2) *r2 = h->front_r2;
    return SPX_OK;
}

// The representer points of a knowledge-gradient pass (spx.h): a setting of the handle, as the front is.  Everything is
// checked before anything is touched; D is the handle's (observations or candidates set it).
int spx_set_kg_points(spx_handle* h, const double* pts, int32_t A)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_set_kg_points: null handle");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_set_kg_points: SPX_ACQ_KG is single-device only (multi-device handle)");
    if (A < 0) { spx_drop(h, Held::KGPTS); h->kg_A = -1; h->kg_pts_host.clear(); return SPX_OK; }
    if (A < 1 || A > SPX_KG_MAX_POINTS)
        return fail(SPX_ERR_ARG, "spx_set_kg_points: A=%d representer points (allowed: 1 .. %d)", (int)A, SPX_KG_MAX_POINTS);
    if (!pts) return fail(SPX_ERR_ARG, "spx_set_kg_points: null points with A=%d", (int)A);
    if (!h->held.has(Held::OBS) && !h->held.has(Held::CAND))
        return fail(SPX_ERR_ARG, "spx_set_kg_points: set observations or candidates first (they give the dimension)");
    const int D = h->D;
    for (size_t i = 0; i < (size_t)A * D; ++i)
        if (!std::isfinite(pts[i]))
            return fail(SPX_ERR_ARG, "spx_set_kg_points: coordinate %d of point %d is not finite (%g)", (int)(i % D), (int)(i / D), pts[i]);
    int rc = ensure_init(h);
    if (rc) return rc;
    // (a reservation that fails has released the old buffer: the points it belonged to go first)
    spx_drop(h, Held::KGPTS);
    h->kg_A = -1;
    h->kg_pts_host.clear();
    if ((rc = h->kg_pts.reserve((size_t)A * D * 8))) return rc;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->kg_pts.p, pts, (size_t)A * D * 8, h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->kg_pts_host.assign(pts, pts + (size_t)A * D);
    h->kg_A = A;
    return spx_hold(h, Held::KGPTS);
}

int spx_get_kg_points(spx_handle* h, double* pts, int32_t* A)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_get_kg_points: null handle");
    const bool have = !h->multi && h->held.has(Held::KGPTS);
    if (A) *A = have ? h->kg_A : -1;
    if (have && pts) std::copy(h->kg_pts_host.begin(), h->kg_pts_host.end(), pts);
    return SPX_OK;
}

// ---------------------------------------------------------------------------
static int finish_factor(spx_handle* h, const std::vector<int>& info, bool tolerate_not_pd, bool lean);

int spx_set_constraint_model(spx_handle* h, const double* comp_c, const double* ff, int64_t Nc, const double* c_hypers)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_set_constraint_model: null handle");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_set_constraint_model: the constraint model is single-device only "
                                           "(multi-device handles and hyper_shards > 1 are not supported)");
    if (!comp_c && !ff && !c_hypers) { spx_drop(h, Held::CON); return SPX_OK; }
    if (!h->held.has(Held::OBS) || !h->held.has(Held::HYP))
        return fail(SPX_ERR_ARG, "spx_set_constraint_model: set observations and hypers first");
    if (!c_hypers || Nc < 0 || Nc > (1 << 20) || (Nc > 0 && (!comp_c || !ff)))
        return fail(SPX_ERR_ARG, "spx_set_constraint_model: bad arguments (Nc=%lld)", (long long)Nc);
    int rc = ensure_init(h);
    if (rc) return rc;
    const int H = h->H, D = h->D, hs = 3 + D;
    spx_drop(h, Held::CON);
    if (Nc > 0) {
        if (!h->con) {
            if ((rc = spx_create(h->device, &h->con))) return rc;
            h->con->opt.stage_copies = h->opt.stage_copies;
            h->con->opt.cov_kind = h->opt.cov_kind;     // (from here on option "covar" reaches it: opt_covar)
        }
        // the factor's rows: [0, noise_c, amp2_c, ls_c...] -- alpha_c = K_c^-1 (ff - 0): no mean term (:819-842)
        std::vector<double> rows(c_hypers, c_hypers + (size_t)H * hs);
        for (int i = 0; i < H; ++i) rows[(size_t)i * hs] = 0.0;
        if ((rc = spx_set_observations(h->con, comp_c, ff, Nc, D))) return rc;
        if ((rc = spx_set_hypers(h->con, rows.data(), H))) return rc;
        h->con_comp_host.assign(comp_c, comp_c + (size_t)Nc * D);
    }
    h->con_tab_host.assign((size_t)H * SPX_HT, 0.0);
    for (int i = 0; i < H; ++i) {
        const double* r = c_hypers + (size_t)i * hs;
        double* t = &h->con_tab_host[(size_t)i * SPX_HT];
        t[0] = r[0]; t[1] = r[1]; t[2] = r[2]; t[3] = r[2];
    }
    if ((rc = h->con_tab.reserve(h->con_tab_host.size() * 8))) return rc;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->con_tab.p, h->con_tab_host.data(), h->con_tab_host.size() * 8, h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->con_n = Nc;
    return spx_hold(h, Held::CON);
}

// The constraint model's alpha_c, before the objective's factorisation (spx_factor / spx_ei_step).  Its own handle, its own
// synchronisation: a not-PD constraint covariance is reported as draw 2H + d.
static int factor_constraint(spx_handle* h)
{
    if (!h->held.has(Held::CON) || h->con_n == 0 || h->held.has(Held::CON_FACTOR)) return SPX_OK;
    spx_handle* c = h->con;
    if (c->H != h->H || c->D != h->D)
        return fail(SPX_ERR_ARG, "spx_factor: the constraint model has H=%d, D=%d but the objective H=%d, D=%d "
                                 "(call spx_set_constraint_model again)", c->H, c->D, h->H, h->D);
    int rc = spx_factor(c);
    if (rc == SPX_ERR_NOT_PD) {
        h->not_pd_draw = 2 * h->H + c->not_pd_draw;
        h->not_pd_pivot = c->not_pd_pivot;
        return fail(SPX_ERR_NOT_PD, "%d-th leading minor of the array is not positive definite (draw %d, constraint model)",
                    c->not_pd_pivot + 1, c->not_pd_draw);
    }
    if (rc) return rc;
    return spx_hold(h, Held::CON_FACTOR);
}

// A hand-off of k_lean_flow timed out (its polls are bounded: an error, never a hang; not seen on a healthy device -- a
// preempted or badly oversubscribed GPU could produce one).  The call is repeated with one launch per block column -- the
// same arithmetic, the same bits -- and the handle STAYS there for `flow_rearm_after` clean factorisations (default 16), then
// tries the data-flow launch again (finish_factor): one bad moment does not cost a long-lived chooser process 30 % of every
// later factorisation.  spx_set_option("lean_flow", 1) re-arms at once.  Counters: spx_get_stat("flow_fallbacks" /
// "flow_rearms" / "flow_enabled").
static void note_flow_timeout(spx_handle* h)
{
    h->flow_fallbacks += 1;
    h->flow_demoted = true;
    h->flow_clean = -1;             // (the repeat of THIS call is not one of the clean factorisations that are counted)
    h->handoff_timeout = false;
}
// ... and the repeated call succeeded: SPX_OK, with a WARNING left in spx_last_error() (text starts with "warning:")
static void warn_flow_fallback(spx_handle* h)
{
    char buf[320];
    snprintf(buf, sizeof buf, "warning: a hand-off inside the data-flow factorisation timed out (%lld so far on this handle); "
             "this call was repeated with one launch per block column (same results) and the handle stays there for %d "
             "clean factorisations", (long long)h->flow_fallbacks, h->opt.flow_rearm_after);
    spx_err_slot() = buf;
}

#define SPX_POLL_SENTINEL 0x7fffffff   // no not-PD flag has this value (pivots <= 2^20, time-outs < 0)
// defer_sync (log-likelihood path): return with the work queued -- the caller adds its own kernel, copies `info` back
// together with its result, synchronises ONCE and calls finish_factor (one host round trip per call instead of two)
static int do_factor(spx_handle* h, bool tolerate_not_pd, bool lean = false, bool defer_sync = false)
{
    if (!h->held.has(Held::OBS) || !h->held.has(Held::HYP))
        return fail(SPX_ERR_ARG, "spx_factor: observations and hypers must be set first");
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::FACTOR);      // both paths overwrite Xs, the hyper tables and L; finish_factor sets it again (not the lean path)
    FactorShape sh;
    sh.N = h->N; sh.D = h->D; sh.H = h->H; sh.Np = h->Np;
    // (under SPX_ACQ_EHVI the time model is the second objective's GP, factored on its own internal handle: ehvi_second)
    sh.have_time = h->held.has(Held::TIME) && h->acq != SPX_ACQ_EHVI; sh.lean = lean; sh.defer_sync = defer_sync; sh.have_dest = h->fused_lp != nullptr;
    sh.flow_demoted = h->flow_demoted; sh.rhs_rows_on = h->rhs_rows_on;
    FactorPlan& p = lean ? h->lean_plan : h->factor_plan;
    p = plan_factor(h->opt, sh);              // every decision of this call (spx_plan.h); below: reserve, upload, launch
    h->last_factor = &p;
    if (!lean) h->nmodels = p.nm;
    const int nm = p.nm, H = h->H, nh = p.nh, D = h->D, Dp = p.Dp, Np = p.Np, nblk = p.nblk, hs = p.hs;
    const int64_t N = h->N;

    // host-side hyper tables: raw rows (for ls) and [mean, noise, amp2, amp2*(1+1e-6)]
    // (members, not locals: the log-likelihood path returns before it synchronises, and the upload must not outlive its source)
    std::vector<double>& raw = h->up_raw;
    std::vector<double>& tab = h->up_tab;
    raw.assign((size_t)nh * hs, 0.0);
    tab.assign((size_t)nh * SPX_HT, 0.0);
    for (int m = 0; m < nm; ++m) {
        const std::vector<double>& src = m ? h->thyp_host : h->hyp_host;
        for (int i = 0; i < H; ++i) {
            const double* r = &src[(size_t)i * hs];
            memcpy(&raw[((size_t)m * H + i) * hs], r, sizeof(double) * hs);
            if (h->opt.cov_kind == SPX_COVAR_SE)   // gp.SE ignores its length scales (gp.py:88)
                for (int d = 0; d < D; ++d) raw[((size_t)m * H + i) * hs + 3 + d] = 1.0;
            double* t = &tab[((size_t)m * H + i) * SPX_HT];
            t[0] = r[0]; t[1] = r[1]; t[2] = r[2];
            t[3] = r[2] * (1 + 1e-6);  // self.amp2*(1+1e-6), GPEIChooser.py:199
        }
    }
    // raw rows and the table travel in ONE upload: htab is a view of the tail of the hyp buffer
    raw.insert(raw.end(), tab.begin(), tab.end());
    if ((rc = h->hyp.reserve(p.hyp_doubles * 8))) return rc;
    h->htab.alias_of(h->hyp.d() + (size_t)nh * hs);
    if ((rc = h->Xs.reserve(p.xs_bytes))) return rc;
    if ((rc = h->X2s.reserve(p.xs_bytes))) return rc;
    if ((rc = h->s1.reserve(p.vec_bytes))) return rc;
    if ((rc = h->Lm.reserve(p.nn_bytes))) return rc;
    if (!lean && (rc = h->WT.reserve(p.nn_bytes))) return rc;
    if ((rc = h->Dinv.reserve(p.dinv_bytes))) return rc;
    if ((rc = h->gamma.reserve(p.vec_bytes))) return rc;
    if ((rc = h->alpha.reserve(p.vec_bytes))) return rc;
    if ((rc = h->info.reserve(p.info_bytes))) return rc;

    hipStream_t s = h->stream;
    h->ev_used = 0;
    hipEvent_t t0 = h->ev_t0, t1 = h->ev_t1;
    // through pinned memory: a pageable source makes the runtime stage the copy and wait for it (the stream is idle here:
    // every entry point that queues work on it synchronises before it returns, so the staging buffer is free)
    if ((rc = h->pin_up.reserve(p.hyp_doubles * 8))) return rc;
    memcpy(h->pin_up.p, raw.data(), p.hyp_doubles * 8);
    if (p.poll) for (int k = 0; k < H; ++k) h->fused_info[k] = SPX_POLL_SENTINEL;   // (coherent pinned memory: in place before the launch is queued)
    if (!p.zero_copy) HIPCHK(hipMemcpyAsync(h->hyp.p, h->pin_up.p, p.hyp_doubles * 8, hipMemcpyHostToDevice, s));
    if (p.bracket) HIPCHK(hipEventRecord(t0, s));
    // (W^T's zeros above the diagonal blocks are written by k_trinv itself)

    const double* ls = h->hyp.d() + 3;
    // the not-PD flags: zeroed once per allocation; the fused launch leaves them zero.  (Address AND size: a buffer that grew may
    // come back at the address the smaller one had -- its new words are not the zeros the old ones were.)
    if (p.fused && (h->info_clean_ptr != h->info.p || h->info_clean_bytes != h->info.cap)) {
        HIPCHK(hipMemsetAsync(h->info.p, 0, h->info.cap, s));
        h->info_clean_ptr = h->info.p;
        h->info_clean_bytes = h->info.cap;
    }
    if (!p.fused) h->info_clean_ptr = nullptr;
    // x / ls and, in the same launch, the second operand pre-multiplied by 2 (gp.py:50; exact)
    if (!p.merged_prologue)
        TIMED(ST_SCALE, launch_scale_rows(s, h->comp.d(), N, Np, D, Dp, ls, hs, nh, 1.0, h->Xs.d(), h->s1.d(), h->X2s.d(),
                                          p.zero_in_kernel ? nullptr : (int*)h->info.p, nh));
    // (spx_ei_step: the candidate side of the EI pass needs x / ls and the hyper table, not the factor -- it starts here,
    // on the second stream, beside the factorisation)
    if (p.step) HIPCHK(hipEventRecord(h->ev_obs, s));
    if (!p.cov_in_flow)
        TIMED(ST_COV_SELF, launch_cov_self(s, h->Xs.d(), h->s1.d(), h->X2s.d(), h->htab.d(), h->Lm.d(), (int)N, Np, Dp, nh, p.tiled, dev_kind(h)));
    if (p.ps && (rc = h->ps_flags.reserve(p.ps_bytes))) return rc;   // zeroed by k_lean_rhs_init
    int* lflags = nullptr; int* dflags = nullptr; int* cu_busy = nullptr; unsigned* tickets = nullptr;
    if (p.flow) {
        if (p.nfl > h->flow_flags_n || h->flow_gen >= (1 << 27)) {
            if ((rc = h->flow_flags.reserve(p.nfl * sizeof(int)))) return rc;
            HIPCHK(hipMemsetAsync(h->flow_flags.p, 0, h->flow_flags.cap, h->stream));
            h->flow_flags_n = h->flow_flags.cap / sizeof(int);
            h->flow_gen = 0;
        }
        h->flow_gen += 1;
        tickets = (unsigned*)h->flow_flags.p;          // first (counter, done count): their place does not move with the batch size
        cu_busy = (int*)h->flow_flags.p + 2;           // [xcc][se, sh, cu]: workgroups inside a diagonal block, back to 0 after every launch
        lflags = cu_busy + 4096;
        dflags = lflags + (size_t)nh * (nblk + 1) * nblk;
    }
    // lean: the right-hand side vals - mean rides through the factorisation as an extra row block,
    // so y = L^-1 (vals - mean) is ready when the last column is
    double* rhs = nullptr;
    // (spx_gp_logprob_rhs: draw h's right-hand side is row h of rhs_rows instead of the shared values)
    const double* vsrc = h->rhs_rows_on ? h->rhs_rows.d() : h->vals.d();
    if (lean) {
        if ((rc = h->rhs.reserve(p.rhs_bytes))) return rc;
        rhs = h->rhs.d();
        if (p.rl) {
            if ((rc = h->diagL.reserve(p.diagL_bytes))) return rc;
            if (p.fused) {}            // (nothing to launch)
            else if (p.merged_prologue)     // (implies flow and cov_in_flow: nothing before this point read x / ls)
                TIMED(ST_SCALE, launch_lean_prologue(s, h->comp.d(), N, Np, D, Dp, ls, hs, nh, h->Xs.d(), h->s1.d(), h->X2s.d(),
                                                     vsrc, h->htab.d(), rhs, (int*)h->info.p, p.ps ? (int*)h->ps_flags.p : nullptr,
                                                     p.vstride));
            else
                TIMED(ST_GAMMA_ALPHA, launch_lean_rhs_init(s, vsrc, h->htab.d(), rhs, (int)N, Np, nh, (int*)h->info.p,
                                                           p.ps ? (int*)h->ps_flags.p : nullptr, p.vstride));
        } else {
            TIMED(ST_GAMMA_ALPHA, launch_rhs_init(s, vsrc, h->htab.d(), rhs, (int)N, Np, nh, p.vstride));
        }
    }
    FlowFused ff{h->comp.d(), p.zero_copy ? (const double*)h->pin_up.p : h->hyp.d(), vsrc, D, hs, h->fused_lp, h->fused_info,
                 lean ? p.vstride : 0};
    const double* htab_dev = p.zero_copy ? (const double*)h->pin_up.p + (size_t)nh * hs : h->htab.d();
    if (p.flow)
        TIMED(ST_CHOL_DIAG, launch_lean_flow(s, h->Lm.d(), h->Dinv.d(), (int*)h->info.p, rhs, lean ? h->diagL.d() : nullptr, lflags, dflags, tickets, Np, nh, h->flow_gen, p.flow_alone,
                                             p.cov_in_flow ? h->Xs.d() : nullptr, h->X2s.d(), h->s1.d(), htab_dev, (int)N, Dp, dev_kind(h),
                                             p.yield ? cu_busy : nullptr, h->opt.flow_spin_limit, p.fused ? &ff : nullptr));
    for (int k = 0; k < (p.flow ? 0 : nblk); ++k) {
        if (p.ps) {
            TIMED(ST_CHOL_DIAG, launch_lean_step_ps(s, h->Lm.d(), h->Dinv.d(), (int*)h->info.p, rhs, h->diagL.d(), (int*)h->ps_flags.p, Np, k, nh));
        } else if (p.rl) {
            TIMED(ST_CHOL_DIAG, launch_lean_step(s, h->Lm.d(), h->Dinv.d(), (int*)h->info.p, rhs, h->diagL.d(), Np, k, nh, p.lazy));
            TIMED(ST_CHOL_PANEL, launch_lean_trsm(s, h->Lm.d(), h->Dinv.d(), rhs, Np, k, nh));
        } else {
            TIMED(ST_CHOL_DIAG, launch_chol_diag(s, h->Lm.d(), h->Dinv.d(), (int*)h->info.p, Np, k, nh, 0));
            if (k + 1 < nblk || rhs) TIMED(ST_CHOL_PANEL, launch_chol_panel(s, h->Lm.d(), h->Dinv.d(), Np, k, nh, rhs));
        }
    }
    if (!lean) {
        TIMED(ST_TRINV, launch_trinv(s, h->Lm.d(), h->Dinv.d(), h->WT.d(), Np, nh, p.flow));
        TIMED(ST_GAMMA_ALPHA, launch_gamma(s, h->WT.d(), h->vals.d(), h->htab.d(), h->gamma.d(), (int)N, Np, H));
        if (nm == 2)
            TIMED(ST_GAMMA_ALPHA, launch_gamma(s, h->WT.d() + (size_t)H * Np * Np, h->ldur.d(),
                                                h->htab.d() + (size_t)H * SPX_HT,
                                                h->gamma.d() + (size_t)H * Np, (int)N, Np, H));
        TIMED(ST_GAMMA_ALPHA, launch_alpha(s, h->WT.d(), h->gamma.d(), h->alpha.d(), Np, nh));
    }
    if (p.bracket) HIPCHK(hipEventRecord(t1, s));
    if (p.step) HIPCHK(hipEventRecord(h->ev_fac, s));   // (spx_ei_step with two streams: alpha is ready)
    if (defer_sync) return SPX_OK;
    std::vector<int> info(nh);
    if ((rc = stage_d2h(h, info.data(), h->info.p, (size_t)nh * sizeof(int), s))) return rc;
    return finish_factor(h, info, tolerate_not_pd, lean);
}

static int finish_factor(spx_handle* h, const std::vector<int>& info, bool tolerate_not_pd, bool lean)
{
    const int nh = (int)info.size(), H = h->H;
    LAUNCHCHK();
    float ms = 0.f;
    if (h->opt.timing) {
        (void)hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1);
        ev_collect(h);
        h->st_ms[ST_FACTOR_TOTAL] += ms; h->st_n[ST_FACTOR_TOTAL] += 1;
    }
    h->not_pd_draw = h->not_pd_pivot = -1;
    for (int i = 0; i < nh; ++i)
        if (info[i] < 0) { // k_lean_flow / k_lean_step_ps: a workgroup gave up waiting for a tile or a diagonal block (bounded spin)
            h->handoff_timeout = true;
            return fail(SPX_ERR_HIP, "log-likelihood factorisation: in-launch hand-off timed out (draw %d)", i);
        }
    if (h->flow_demoted && h->opt.flow_rearm_after > 0 && ++h->flow_clean >= h->opt.flow_rearm_after) {
        h->flow_demoted = false;     // the next factorisation is the data-flow launch again
        h->flow_clean = 0;
        h->flow_rearms += 1;
    }
    for (int i = 0; i < nh; ++i)
        if (info[i]) { h->not_pd_draw = i; h->not_pd_pivot = info[i] - 1; break; }
    if (h->not_pd_draw >= 0 && !tolerate_not_pd)
        return fail(SPX_ERR_NOT_PD, "%d-th leading minor of the array is not positive definite (draw %d%s)",
                    h->not_pd_pivot + 1, h->not_pd_draw % H, h->not_pd_draw >= H ? ", time model" : "");
    return lean ? SPX_OK : spx_hold(h, Held::FACTOR);
}

int spx_factor(spx_handle* h)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_factor: null handle");
    if (h->multi) return spx_multi_factor(h->multi);
    int rc = factor_constraint(h);
    if (rc) return rc;
    h->handoff_timeout = false;
    rc = do_factor(h, false);
    if (rc == SPX_ERR_HIP && h->handoff_timeout && h->last_factor->flow) {   // as in spx_gp_logprob: never seen; bounded, then the launches
        note_flow_timeout(h);
        rc = do_factor(h, false);
        if (!rc) warn_flow_fallback(h);
    }
    return rc;
}

int spx_not_pd_info(spx_handle* h, int32_t* draw, int32_t* pivot)
{
    if (!h) return fail(SPX_ERR_ARG, "null handle");
    if (h->multi) return spx_multi_not_pd_info(h->multi, draw, pivot);
    if (draw) *draw = h->not_pd_draw;
    if (pivot) *pivot = h->not_pd_pivot;
    return SPX_OK;
}

// The clear forms of spx_set_fantasies / spx_draw_fantasies: the fantasies go; the results of the last pass, a record of what
// it computed with them, stay readable (as they always did -- the next pass runs without them)
static int clear_fantasies(spx_handle* h)
{
    const bool had = h->held.has(Held::RESULTS);
    const Held::Results r = h->held.results;
    spx_drop(h, Held::FANT);
    return had ? spx_hold(h, Held::RESULTS, r) : (int)SPX_OK;
}

int spx_set_fantasies(spx_handle* h, const double* fant, const double* bests, int32_t S)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_set_fantasies: null handle");
    if (h->multi) return spx_multi_set_fantasies(h->multi, fant, bests, S);
    if (!fant || !bests || S <= 0) return clear_fantasies(h);
    if (!h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_set_fantasies: call spx_factor first");
    if (S > 4096) return fail(SPX_ERR_ARG, "spx_set_fantasies: at most 4096 fantasies (got %d)", S);
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::FANT);
    const int H = h->H, Np = h->Np;
    const int64_t n = h->N;
    // host transpose to [H][S][n] so that every fantasy column is a contiguous right-hand side
    std::vector<double> ft((size_t)H * S * n);
    for (int d = 0; d < H; ++d)
        for (int64_t i = 0; i < n; ++i)
            for (int c = 0; c < S; ++c)
                ft[((size_t)d * S + c) * n + i] = fant[((size_t)d * n + i) * S + c];
    if ((rc = h->fantT.reserve(ft.size() * 8))) return rc;
    if ((rc = h->gammaS.reserve((size_t)H * S * Np * 8))) return rc;
    if ((rc = h->bests.reserve((size_t)H * S * 8))) return rc;
    hipStream_t s = h->stream;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->fantT.p, ft.data(), ft.size() * 8, s))) return rc;
    if ((rc = stage_h2d(h, h->bests.p, bests, (size_t)H * S * 8, s))) return rc;
    for (int d = 0; d < H; ++d)   // Gamma_d = W_d (F_d - mean_d), one launch per draw, S columns each
        launch_gamma_multi(s, h->WT.d() + (size_t)d * Np * Np, h->fantT.d() + (size_t)d * S * n,
                           h->htab.d() + (size_t)d * SPX_HT, h->gammaS.d() + (size_t)d * S * Np, (int)n, Np, S);
    HIPCHK(hipStreamSynchronize(s));
    LAUNCHCHK();
    h->S = S;
    return spx_hold(h, Held::FANT);
}

// The pending branch without the host (GPEIChooser.py:219-249): the posterior of the P trailing rows from the resident
// factor, the fantasies from the caller's normals, bests and Gamma -- two launches and one wait for the device; P S (or H P S)
// doubles go up, H flags come back.  Gamma's first N rows do not depend on the fantasy (L is lower triangular): they are
// copied from gamma, only the last P are solved for (fantasy_kernels.hip).
int spx_draw_fantasies(spx_handle* h, int32_t P, const double* z, int32_t per_draw, int32_t S)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_draw_fantasies: null handle");
    if (h->multi) return spx_multi_draw_fantasies(h->multi, P, z, per_draw, S);
    if (!z || S <= 0) return clear_fantasies(h);
    if (!h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_draw_fantasies: call spx_factor first");
    if (S > 4096) return fail(SPX_ERR_ARG, "spx_draw_fantasies: at most 4096 fantasies (got %d)", S);
    if (P < 1 || P > SPX_MAX_PENDING || P > h->N - 1)
        return fail(SPX_ERR_ARG, "spx_draw_fantasies: P = %d pending rows, need 1 .. min(%d, n - 1) with n = %lld", P,
                    SPX_MAX_PENDING, (long long)h->N);
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::FANT);
    const int H = h->H, Np = h->Np, Nc = (int)(h->N - P);
    const size_t zcount = (size_t)(per_draw ? H : 1) * P * S;
    if ((rc = h->fant_z.reserve(zcount * 8))) return rc;
    if ((rc = h->fant_post.reserve((size_t)H * fant_post_stride(P) * 8))) return rc;
    if ((rc = h->fant_pend.reserve((size_t)H * P * S * 8))) return rc;
    if ((rc = h->fant_info.reserve((size_t)H * sizeof(int)))) return rc;
    if ((rc = h->gammaS.reserve((size_t)H * S * Np * 8))) return rc;
    if ((rc = h->bests.reserve((size_t)H * S * 8))) return rc;
    hipStream_t s = h->stream;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->fant_z.p, z, zcount * 8, s))) return rc;
    launch_fant_posterior(s, h->Lm.d(), factor_tiled(h), h->gamma.d(), h->htab.d(), h->vals.d(), h->fant_post.d(),
                          (int*)h->fant_info.p, Nc, P, Np, H);
    launch_fant_fill(s, h->fant_post.d(), h->fant_z.d(), per_draw ? (size_t)P * S : 0, h->gamma.d(), h->gammaS.d(),
                     h->bests.d(), h->fant_pend.d(), Nc, P, Np, S, H);
    std::vector<int> info(H);
    if ((rc = stage_d2h(h, info.data(), h->fant_info.p, (size_t)H * sizeof(int), s))) return rc;
    LAUNCHCHK();
    for (int d = 0; d < H; ++d)     // (a clean call leaves spx_not_pd_info what the factorisation made it, as spx_set_fantasies does)
        if (info[d]) {
            h->not_pd_draw = 4 * H + d; h->not_pd_pivot = info[d] - 1;
            return fail(SPX_ERR_NOT_PD, "%d-th leading minor of the array is not positive definite (draw %d, posterior of "
                                        "the pending points)", info[d], d);
        }
    h->S = S; h->fant_P = P; h->fant_device = true;
    return spx_hold(h, Held::FANT);
}

int spx_get_pending_fantasies(spx_handle* h, int32_t draw, double* pend_fant, double* bests)
{
    if (h && h->multi) return spx_multi_get_pending_fantasies(h->multi, draw, pend_fant, bests);
    if (!h || !h->held.has(Held::FANT) || !h->fant_device)
        return fail(SPX_ERR_ARG, "spx_get_pending_fantasies: call spx_draw_fantasies first");
    if (draw < 0 || draw >= h->H) return fail(SPX_ERR_ARG, "spx_get_pending_fantasies: draw out of range");
    int rc = ensure_init(h);
    if (rc) return rc;
    const size_t ps = (size_t)h->fant_P * h->S;
    if (pend_fant && (rc = stage_d2h(h, pend_fant, h->fant_pend.d() + (size_t)draw * ps, ps * 8, h->stream))) return rc;
    if (bests && (rc = stage_d2h(h, bests, h->bests.d() + (size_t)draw * h->S, (size_t)h->S * 8, h->stream))) return rc;
    return SPX_OK;
}


// factor_pending (spx_ei_step): the factorisation is queued on the stream but not yet checked -- its not-PD flags travel
// home with the winner, and ONE synchronisation ends the step
// rhs: what the pass's S > 0 GEMM branch runs over when it is not the handle's fantasies (FANT, S = h->S):
//   TS (spx_thompson)  the rhs.S right-hand sides per draw in h->ts_gammaS, k_ts_prior per chunk, k_ts_finish in place of the
//                      acquisition, a per-path argmin in place of the mean and argmax
//   KG (decided inside, from the handle's acquisition: no caller passes it)  gamma | Gamma_a of the A representer points in
//                      h->kg_gammaS, S = A + 1; k(A, c) per work item and the two kg kernels in place of the acquisition
struct PassRhs { enum Kind { FANT, TS, KG } kind = FANT; int S = 0; };
static int ei_run_impl(spx_handle* h, int32_t flags, bool factor_pending, PassRhs rhs = PassRhs());
static int ehvi_second(spx_handle* h);

// what an EI pass refuses because of its flags alone (nmodels: 2 when a time model is / will be factored)
static const char* acq_name(int acq)
{
    return acq == SPX_ACQ_PI ? "PI" : acq == SPX_ACQ_LCB ? "LCB" : acq == SPX_ACQ_MES ? "MES" : acq == SPX_ACQ_EHVI ? "EHVI"
         : acq == SPX_ACQ_KG ? "KG" : "EI";
}

// what a pass under SPX_ACQ_KG refuses, decided from the host's record alone (who: the entry point's name)
static int check_kg(const spx_handle* h, int32_t flags, const char* who)
{
    if (h->acq != SPX_ACQ_KG) return SPX_OK;
    if (flags & (SPX_FLAG_PER_SEC | SPX_FLAG_CONSTRAINED | SPX_FLAG_TIME_ONLY))
        return fail(SPX_ERR_ARG, "%s: SPX_FLAG_PER_SEC / SPX_FLAG_CONSTRAINED / SPX_FLAG_TIME_ONLY are defined for "
                                 "SPX_ACQ_EI only (spx_set_acquisition chose KG)", who);
    if (h->comm || h->part_ph > 1 || h->part_M > 0)
        return fail(SPX_ERR_ARG, "%s: SPX_ACQ_KG is single-device only (communicator attached or 2-D partition set)", who);
    if (!h->held.has(Held::KGPTS))
        return fail(SPX_ERR_ARG, "%s: SPX_ACQ_KG needs representer points (spx_set_kg_points)", who);
    if (h->S > 0)
        return fail(SPX_ERR_ARG, "%s: SPX_ACQ_KG is not defined over fantasies (clear them, or score the call with SPX_ACQ_EI)", who);
    if ((flags & SPX_FLAG_KEEP_MOMENTS) && h->held.has(Held::CAND) && h->held.has(Held::HYP)
        && (double)h->H * h->kg_A * (double)round_up(h->M, SPX_BN) * 8.0 > (double)SPX_KG_MAX_LINE_BYTES)
        return fail(SPX_ERR_ARG, "%s: H A Mp 8 = %d x %d x %lld x 8 bytes of kept covariances (SPX_FLAG_KEEP_MOMENTS under SPX_ACQ_KG "
                                 "allows up to %lld bytes)", who, h->H, h->kg_A, (long long)round_up(h->M, SPX_BN),
                    (long long)SPX_KG_MAX_LINE_BYTES);
    return SPX_OK;
}

// what a pass under SPX_ACQ_EHVI refuses, decided from the host's record alone (who: the entry point's name)
static int check_ehvi(const spx_handle* h, int32_t flags, const char* who)
{
    if (h->acq != SPX_ACQ_EHVI) return SPX_OK;
    if (flags & (SPX_FLAG_PER_SEC | SPX_FLAG_CONSTRAINED | SPX_FLAG_TIME_ONLY))
        return fail(SPX_ERR_ARG, "%s: SPX_FLAG_PER_SEC / SPX_FLAG_CONSTRAINED / SPX_FLAG_TIME_ONLY are defined for "
                                 "SPX_ACQ_EI only (spx_set_acquisition chose EHVI)", who);
    if (h->comm || h->part_ph > 1 || h->part_M > 0)
        return fail(SPX_ERR_ARG, "%s: SPX_ACQ_EHVI is single-device only (communicator attached or 2-D partition set)", who);
    if (!h->held.has(Held::TIME))
        return fail(SPX_ERR_ARG, "%s: SPX_ACQ_EHVI needs the second objective's GP (spx_set_time_model)", who);
    if (!h->held.has(Held::FRONT))
        return fail(SPX_ERR_ARG, "%s: SPX_ACQ_EHVI needs a front (spx_set_pareto_front)", who);
    if (h->S > 0)
        return fail(SPX_ERR_ARG, "%s: SPX_ACQ_EHVI is not defined over fantasies (clear them first)", who);
    return SPX_OK;
}

static int check_run_flags(const spx_handle* h, int32_t flags, int nmodels)
{
    int rc_ehvi = check_ehvi(h, flags, "spx_ei_run");
    if (rc_ehvi) return rc_ehvi;
    if ((rc_ehvi = check_kg(h, flags, "spx_ei_run"))) return rc_ehvi;
    const bool per_sec = (flags & SPX_FLAG_PER_SEC) != 0;
    const bool keep_mom = (flags & SPX_FLAG_KEEP_MOMENTS) != 0;
    const bool time_only = (flags & SPX_FLAG_TIME_ONLY) != 0;
    if (h->acq != SPX_ACQ_EI && (flags & (SPX_FLAG_PER_SEC | SPX_FLAG_CONSTRAINED | SPX_FLAG_TIME_ONLY)))
        return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_PER_SEC / SPX_FLAG_CONSTRAINED / SPX_FLAG_TIME_ONLY are defined for "
                                 "SPX_ACQ_EI only (spx_set_acquisition chose %s)",
                    acq_name(h->acq));
    // (a communicator or a partition attached after spx_set_acquisition accepted MES)
    if (h->acq == SPX_ACQ_MES && (h->comm || h->part_ph > 1 || h->part_M > 0))
        return fail(SPX_ERR_ARG, "spx_ei_run: SPX_ACQ_MES is single-device only: y* of a draw needs every shard's moments "
                                 "(communicator attached or 2-D partition set)");
    if (time_only && !(per_sec && keep_mom))
        return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_TIME_ONLY needs SPX_FLAG_PER_SEC | SPX_FLAG_KEEP_MOMENTS");
    if (time_only && h->comm) return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_TIME_ONLY has no winner to exchange (communicator attached)");
    if (per_sec && nmodels != 2)
        return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_PER_SEC needs spx_set_time_model before spx_factor");
    if (flags & SPX_FLAG_CONSTRAINED) {
        if (per_sec) return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_CONSTRAINED cannot be combined with SPX_FLAG_PER_SEC");
        if (!h->held.has(Held::CON)) return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_CONSTRAINED needs spx_set_constraint_model");
        if (h->comm) return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_CONSTRAINED is single-device only (communicator attached)");
        if (h->con_n > 0 && (h->con->H != h->H || h->con->D != h->D))
            return fail(SPX_ERR_ARG, "spx_ei_run: the constraint model does not match the objective's H / D");
        if ((int64_t)h->con_tab_host.size() != (int64_t)h->H * SPX_HT)
            return fail(SPX_ERR_ARG, "spx_ei_run: the constraint model has a different number of draws");
    }
    return SPX_OK;
}

int spx_ei_run(spx_handle* h, int32_t flags)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_ei_run: null handle");
    if (h->multi && (flags & SPX_FLAG_CONSTRAINED))
        return fail(SPX_ERR_ARG, "spx_ei_run: SPX_FLAG_CONSTRAINED is single-device only (multi-device handle)");
    if (h->multi) return spx_multi_ei_run(h->multi, flags & ~SPX_FLAG_TIME_ONLY);   // (several GPUs: the full pass; the durations are a by-product)
    return ei_run_impl(h, flags, false);
}

// spx_factor + spx_ei_run as ONE call with ONE host round trip (what a chooser's next() and bench.py's step are): at small
// N the two synchronisations and the device-to-host copies behind them were a quarter of the step (N = 128, 20 000
// candidates, 10 draws: ~85 of 310 us).  Same kernels, same results; a covariance that is not positive definite is
// reported exactly as spx_factor reports it (SPX_ERR_NOT_PD, spx_not_pd_info), after the one synchronisation.
int spx_ei_step(spx_handle* h, int32_t flags)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_ei_step: null handle");
    if (h->multi && (flags & SPX_FLAG_CONSTRAINED))
        return fail(SPX_ERR_ARG, "spx_ei_step: SPX_FLAG_CONSTRAINED is single-device only (multi-device handle)");
    if (h->multi) {
        int rc = spx_multi_factor(h->multi);
        return rc ? rc : spx_multi_ei_run(h->multi, flags & ~SPX_FLAG_TIME_ONLY);
    }
    {   // EHVI's refusals come before the factorisation in either form below (which would drop the fantasies it refuses)
        int rc = check_ehvi(h, flags, "spx_ei_step");
        if (rc) return rc;
        if ((rc = check_kg(h, flags, "spx_ei_step"))) return rc;   // (likewise)
    }
    if (h->opt.timing || (flags & SPX_FLAG_TIMING) || !h->held.has(Held::CAND)) {   // stage timers bracket each call: keep the two-call form
        int rc = spx_factor(h);
        return rc ? rc : ei_run_impl(h, flags, false);
    }
    // the pass's argument checks BEFORE anything is queued (ei_run_impl repeats them for spx_ei_run)
    int rc = check_run_flags(h, flags, h->held.has(Held::TIME) ? 2 : 1);
    if (rc) return rc;
    if ((rc = factor_constraint(h))) return rc;
    // EHVI: the second GP's factorisation and pass run to their end first, as the constraint model's factorisation does -- one
    // data-flow factorisation on the device at a time, and nothing of this handle is queued when a failure returns
    if (h->acq == SPX_ACQ_EHVI && (rc = ensure_init(h))) return rc;
    if (h->acq == SPX_ACQ_EHVI && (rc = ehvi_second(h))) return rc;
    h->handoff_timeout = false;
    rc = do_factor(h, false, false, true);
    if (rc) return rc;
    rc = ei_run_impl(h, flags, true);
    if (rc == SPX_ERR_HIP && h->handoff_timeout && h->last_factor->flow) {   // as in spx_factor: bounded, then the launches
        note_flow_timeout(h);
        rc = do_factor(h, false);
        if (!rc) rc = ei_run_impl(h, flags, false);
        if (!rc) warn_flow_fallback(h);
        return rc;
    }
    if (rc) {
        // any other error exit of a pending step (argument checks that depend on the plan, a failed reservation, a launch
        // error): the factorisation may still be queued -- every entry point returns with the streams idle (the pinned
        // upload staging relies on it); the factor it did not check is not held (do_factor dropped it)
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->stream2);
        if (h->stream3) (void)hipStreamSynchronize(h->stream3);
        (void)hipGetLastError();
    }
    return rc;
}

// everything an EI pass writes on the device, reserved as its plan says before anything is queued
static int ei_reserve(spx_handle* h, const EiPlan& p, int S)
{
    int rc;
    const bool fant = S > 0, con_gp = p.constrained && h->con_n > 0;
    if (p.ns == 3 && (rc = ensure_stream3(h))) return rc;   // (a time-only pass too: it stages nothing, but produces there)
    // the staging slots: K(X*,X) of a work item and, with fantasies, its partial means; the buffers of slots that the pass
    // does not use go back to the device first
    if (p.trim_ring)
        for (size_t k = p.slots; k < h->ring.size(); ++k) { h->ring[k].Kst.release(); h->ring[k].part_bgS.release(); }
    if ((rc = ensure_slots(h, p.slots))) return rc;
    for (int k = 0; k < p.slots; ++k) {
        if ((rc = h->ring[k].Kst.reserve(p.kst_bytes))) return rc;
        if (fant && (rc = h->ring[k].part_bgS.reserve(p.bgS_bytes))) return rc;
    }
    // scaled candidates (all draws), predicted durations and P(feasible) are double-buffered by chunk parity
    for (auto& cb : h->chunk) {
        if ((rc = cb.Cs.reserve(p.cs_bytes))) return rc;
        if ((rc = cb.s2.reserve(p.s2_bytes))) return rc;
        if (p.per_sec && (rc = cb.time_m.reserve(p.s2_bytes))) return rc;
        if (p.constrained && (rc = cb.con_p.reserve(p.s2_bytes))) return rc;
        if (con_gp && (rc = cb.con_Cs.reserve(p.cs_bytes))) return rc;
        if (con_gp && (rc = cb.con_s2.reserve(p.s2_bytes))) return rc;
    }
    // column sums of beta^2 and beta*gamma per row block for ALL draws of a chunk: written by the
    // GEMM launches and read by one EI-finalize launch per chunk, all on the consumer stream
    if (p.gemm_path && (rc = h->part_ss.reserve(p.part_bytes))) return rc;
    if (p.gemm_path && (rc = h->part_bg.reserve(p.part_bytes))) return rc;
    if (fant && (rc = h->scratch.reserve(p.scratch_bytes))) return rc;   // EI per (draw of the group, fantasy, candidate)
    if ((rc = h->ei_draw.reserve(p.draw_bytes))) return rc;
    if ((rc = h->ei_mean.reserve(p.mean_bytes))) return rc;
    if (p.keep_mom) {
        if ((rc = h->mom_m.reserve(p.draw_bytes))) return rc;
        if ((rc = h->mom_v.reserve(p.draw_bytes))) return rc;
        if (p.per_sec && (rc = h->mom_t.reserve(p.draw_bytes))) return rc;
        if (p.constrained && (rc = h->mom_c.reserve(p.draw_bytes))) return rc;
    }
    const int nab = argmax_blocks(h->M);
    if ((rc = h->am_val.reserve((size_t)nab * 8))) return rc;
    if ((rc = h->am_idx.reserve((size_t)nab * 8))) return rc;
    if ((rc = h->am_out_val.reserve(8))) return rc;
    return h->am_out_idx.reserve(8);
}

// The second GP of an EHVI pass (spx.h): an internal handle on the same device holds (comp, second values, second hypers) and
// the candidates -- copied over from the resident ones when what they were made from changed (SEC / SEC_CAND) -- and runs the
// ordinary factorisation and pass with the moments kept, so func_m / func_v are those of a plain handle to the bit.  Its own
// handle, its own synchronisation, as the constraint model's factorisation; not positive definite: draw 5H + d.
static int ehvi_second(spx_handle* h)
{
    int rc;
    if (!h->sec) {
        if ((rc = spx_create(h->device, &h->sec))) return rc;
        h->sec->opt = h->opt;               // (from here on spx_set_option reaches it)
        h->sec->opt.timing = false;
    }
    spx_handle* c = h->sec;
    const int64_t N = h->N, M = h->M;
    const int D = h->D, H = h->H;
    if ((int64_t)h->thyp_host.size() != (int64_t)H * (3 + D))
        return fail(SPX_ERR_ARG, "spx_ei_run: the second objective's hypers do not match H / D (spx_set_time_model again)");
    if ((rc = ensure_init(c))) return rc;
    // What spx_set_observations / spx_set_candidates do with a caller's host buffer, from the resident copies: device to device on
    // the internal handle's stream (the caller's streams are idle: every entry point returns so).  `best` of the internal
    // handle is not read by anything kept -- its EI values are never served -- and stays 0.
    if (!h->held.has(Held::SEC)) {
        spx_drop(c, Held::OBS);
        if (D != c->D) { spx_drop(c, Held::CAND); spx_drop(c, Held::HYP); }
        c->N = N; c->D = D; c->Dp = padded_dim(D); c->Np = (int)round_up(N, SPX_PADN);
        c->best = 0.0;
        if ((rc = c->comp.reserve((size_t)N * D * 8))) return rc;
        if ((rc = c->vals.reserve((size_t)N * 8))) return rc;
        HIPCHK(hipMemcpyAsync(c->comp.p, h->comp.p, (size_t)N * D * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->vals.p, h->ldur.p, (size_t)N * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if ((rc = spx_hold(c, Held::OBS))) return rc;
        if ((rc = spx_set_hypers(c, h->thyp_host.data(), H))) return rc;
        if ((rc = spx_hold(h, Held::SEC))) return rc;
    }
    if (!h->held.has(Held::SEC_CAND)) {
        spx_drop(c, Held::CAND);
        c->M = M; c->index_base = 0;
        if ((rc = c->cand.reserve((size_t)M * D * 8))) return rc;
        HIPCHK(hipMemcpyAsync(c->cand.p, h->cand.p, (size_t)M * D * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if ((rc = spx_hold(c, Held::CAND))) return rc;
        if ((rc = spx_hold(h, Held::SEC_CAND))) return rc;
    }
    rc = c->held.has(Held::FACTOR) ? spx_ei_run(c, SPX_FLAG_KEEP_MOMENTS) : spx_ei_step(c, SPX_FLAG_KEEP_MOMENTS);
    if (rc == SPX_ERR_NOT_PD) {
        h->not_pd_draw = 5 * H + c->not_pd_draw;
        h->not_pd_pivot = c->not_pd_pivot;
        return fail(SPX_ERR_NOT_PD, "%d-th leading minor of the array is not positive definite (draw %d, second objective)",
                    c->not_pd_pivot + 1, c->not_pd_draw);
    }
    return rc;
}

static int ei_run_impl(spx_handle* h, int32_t flags, bool factor_pending, PassRhs rhs)
{
    if (!h->held.has(Held::FACTOR) && !factor_pending) return fail(SPX_ERR_ARG, "spx_ei_run: call spx_factor first");
    if (!h->held.has(Held::CAND)) return fail(SPX_ERR_ARG, "spx_ei_run: no candidates set");
    const bool ts = rhs.kind == PassRhs::TS;       // (spx_thompson made every check of its own; the acquisition setting is not read)
    int rc = ts ? (int)SPX_OK : check_run_flags(h, flags, h->nmodels);
    if (rc) return rc;
    // Max-value entropy search: the ordinary pass as EI with the moments kept (the way spx_main_effects runs it; the handle's
    // setting is not touched: the pass's kernels are handed pass_acq), then the MES stages on the same stream, which
    // overwrite the per-draw values before the mean and the argmax -- still ONE synchronisation.
    const bool mes = !ts && h->acq == SPX_ACQ_MES;
    if (mes && h->S > 0)
        return fail(SPX_ERR_ARG, "spx_ei_run: SPX_ACQ_MES is not defined over fantasies (clear them, or score the call with "
                                 "SPX_ACQ_EI)");
    // Expected hypervolume improvement: the same shape -- the pass as EI with the moments kept, k_ehvi behind it on the same
    // stream -- after the second GP's pass over the same candidates (ehvi_second, below)
    const bool ehvi = !ts && h->acq == SPX_ACQ_EHVI;
    if (mes || ehvi) flags |= SPX_FLAG_KEEP_MOMENTS;
    // Knowledge gradient: the S > 0 branch over gamma | Gamma_a (column 0 gives func_m, the others q(c, a)), the lines and the
    // values per work item in place of the acquisition; then the mean and the argmax of every pass (check_kg passed above)
    const bool kg = !ts && h->acq == SPX_ACQ_KG;
    if (kg) rhs = PassRhs{PassRhs::KG, h->kg_A + 1};
    const int pass_acq = (mes || ehvi || kg) ? SPX_ACQ_EI : h->acq;
    const double pass_par = (mes || ehvi || kg) ? 0.0 : h->acq_par;
    if ((rc = ensure_init(h))) return rc;
    if ((flags & SPX_FLAG_CONSTRAINED) && h->con_n > 0 && !h->held.has(Held::CON_FACTOR))
        return fail(SPX_ERR_ARG, "spx_ei_run: the constraint model is not factored (spx_factor after spx_set_constraint_model)");
    spx_drop(h, Held::RESULTS);     // the pass overwrites them; a failed one keeps the factor and the fantasies
    if (ehvi && !factor_pending && (rc = ehvi_second(h))) return rc;     // (a pending step ran it before its own factorisation)
    EiShape sh;
    sh.N = h->N; sh.M = h->M; sh.Np = h->Np; sh.D = h->D; sh.H = h->H; sh.S = (ts || kg) ? rhs.S : h->S; sh.nmodels = h->nmodels;
    sh.flags = flags; sh.factor_pending = factor_pending; sh.kst_budget = h->opt.kst_budget;
    // The byte budgets of the plan are shares of what the device has free (a smaller or fuller GPU takes smaller chunks
    // instead of an allocation failure).  They are queried when the number of fantasies / the size of a ring slot changes, not
    // per pass: the plan -- buffer sizes, launch counts -- then stays what it was from pass to pass and across ranks that
    // share a device.  Fantasies: an eighth of free memory, at most 2 GB.
    // (spx_thompson's paths keep a budget of their own: the one cached for the fantasies, and with it the chunking of a later
    // fantasy pass, is what it is on a handle that never drew a path)
    int64_t& fant_budget = ts ? h->ts_fant_budget : kg ? h->kg_fant_budget : h->fant_budget;
    int& fant_budget_S = ts ? h->ts_fant_budget_S : kg ? h->kg_fant_budget_S : h->fant_budget_S;
    if (sh.S > 0 && fant_budget_S != sh.S) {
        size_t mem_free = 0, mem_total = 0;
        int64_t b = 2048ll << 20;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) {
            size_t held = h->scratch.cap;
            for (auto& sl : h->ring) held += sl.part_bgS.cap;
            b = std::max<int64_t>(64ll << 20, std::min<int64_t>(b, (int64_t)(mem_free / 8) + (int64_t)held / 2));
        } else (void)hipGetLastError();
        fant_budget = b;
        fant_budget_S = sh.S;
    }
    sh.fant_budget = fant_budget;
    sh.ring_budget = h->ring_budget;
    EiPlan& p = h->ei_plan;
    p = plan_ei(h->opt, sh);                  // every decision of this pass (spx_plan.h); below: reserve and launch
    // The ring: a sixteenth of free memory, at most 10 GiB.  Its slot size comes out of the plan, so a new size means a new
    // budget and the plan again.
    if (p.ringed && h->ring_budget_slot != p.slot_bytes) {
        size_t mem_free = 0, mem_total = 0;
        int64_t b = 10ll << 30;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) {
            int64_t held = 0;
            for (auto& sl : h->ring) held += (int64_t)(sl.Kst.cap + sl.part_bgS.cap);
            b = std::min<int64_t>(b, (int64_t)(mem_free / 16) + held);
        } else (void)hipGetLastError();
        h->ring_budget = b;
        h->ring_budget_slot = p.slot_bytes;
        sh.ring_budget = b;
        p = plan_ei(h->opt, sh);
    }
    const bool per_sec = p.per_sec, keep_mom = p.keep_mom, time_only = p.time_only, constrained = p.constrained, fused = p.fused;
    const int H = h->H, D = h->D, Dp = p.Dp, Np = h->Np, hs = 3 + D, nrb = p.nrb, Hb = p.Hb, S = sh.S, ns = p.ns;
    const int64_t N = h->N, M = h->M, Mp = p.Mp, Mc = p.Mc;
    if ((rc = ei_reserve(h, p, S))) return rc;
    const int kgA = kg ? h->kg_A : 0, kgAp = (int)round_up(kgA, SPX_PADN);     // (rows of a K(A, .) launch: padded as N is)
    if (kg) {
        if ((rc = h->kg_As.reserve((size_t)H * kgAp * Dp * 8))) return rc;
        if ((rc = h->kg_sA.reserve((size_t)H * kgAp * 8))) return rc;
        if ((rc = h->kg_kxa.reserve((size_t)H * kgAp * Np * 8))) return rc;
        if ((rc = h->kg_gammaS.reserve((size_t)H * S * Np * 8))) return rc;
        if ((rc = h->kg_mua.reserve((size_t)H * kgA * 8))) return rc;
        if ((rc = h->kg_Kac.reserve((size_t)Hb * kgAp * Mc * 8))) return rc;
        if ((rc = h->kg_muc.reserve((size_t)Hb * Mc * 8))) return rc;
        if (keep_mom && (rc = h->kg_cov.reserve((size_t)H * kgA * Mp * 8))) return rc;
    }
    // (read AFTER the reservations above: a buffer that grows moves)
    const double* gammaS_all = ts ? h->ts_gammaS.d() : kg ? h->kg_gammaS.d() : h->gammaS.d();
    const int mesK = mes ? (int)h->acq_par : 0, mesJ = h->opt.mes_grid;
    if (mes) {
        if ((rc = h->mes_bpart.reserve((size_t)H * mes_bound_blocks(M) * 3 * 8))) return rc;
        if ((rc = h->mes_part.reserve((size_t)H * mes_sum_blocks(M) * mesJ * 8))) return rc;
        if ((rc = h->mes_G.reserve((size_t)H * mesJ * 8))) return rc;
        if ((rc = h->mes_ystar.reserve((size_t)H * mesK * 8))) return rc;
        if ((rc = h->mes_fit.reserve((size_t)H * 8 * 8))) return rc;
    }
    h->corun_launches = 0;

    hipStream_t s = h->stream;
    if (flags & SPX_FLAG_TIMING) h->opt.timing = true;
    if (!ts) h->ev_used = 0;         // (spx_thompson's own stages in front of the pass are in the pool already)
    hipEvent_t t0 = h->ev_t0, t1 = h->ev_t1;
    HIPCHK(hipEventRecord(t0, s));
    const int gemm_nlive = p.gemm_nlive;
    const double* ls = h->hyp.d() + 3;
    const size_t nn = (size_t)Np * Np;
    // Streams: G (consumer: predict GEMM + EI finalize) and P (producer: candidate scaling and
    // K(X*,X)): the main stream with one stream, the second with two, with three a stream of the device's lowest priority.
    // K(X*,X) of item i goes through staging slot i % slots (the plan: one slot, two, or the ring's R), by one rule: the
    // producer of item i waits for the slot's `consumed` of item i - slots, G waits for the slot's `ready` before the item's
    // GEMM, and records `consumed` behind the item's last launch where a later item will wait for it.  An event between a
    // stream and itself is left out, so with P == G everything is in order without any; with more slots the producer runs
    // that many items ahead, beside the GEMMs and, in a step, beside the factorisation (whether the two share a SIMD depends
    // on the kernels' registers: two GEMM waves of 176 VGPRs leave room for a producer wave of at most 152 -- k_cov_corun,
    // used by streams = 3 only; k_cov_flat at D = 32 takes 184).  The chunk-level buffers go by chunk parity the same way.
    hipStream_t G = h->stream, P = (ns == 3) ? h->stream3 : (ns == 2) ? h->stream2 : h->stream;
    // A step (factor_pending): the factorisation is still running on G -- a chain of small launches that leaves most of the
    // chip idle -- and the first producer work of the pass (candidate scaling, K(X*,X) of the first group of draws) depends
    // only on what the factorisation's FIRST kernel wrote.  It goes to the second stream, beside the factorisation
    // (C2: K(X*,X) of all ten draws, 0.10 ms, hidden behind a 0.17 ms factorisation).  A time model's predicted durations
    // need alpha: they stay behind the factorisation on G, with the chunk's other-parity scaling buffers to themselves.
    const bool overlap = p.overlap;
    hipStream_t P0 = overlap ? h->stream2 : P;
    if (overlap) HIPCHK(hipStreamWaitEvent(P0, h->ev_obs, 0));
    // Two streams (option streams = 2) in a step: the producer stream has no other order against the factorisation that is
    // still queued on G.  Its scaling and K(X*,X) launches read x / ls, the row norms and the hyper table (written by the
    // factorisation's first kernel: ev_obs); a time model's predicted durations read alpha of the duration GP -- the END of
    // the factorisation (ev_fac).
    if (factor_pending && ns >= 2) HIPCHK(hipStreamWaitEvent(P, per_sec ? h->ev_fac : h->ev_obs, 0));
    if (kg) {
        // Once per pass, on the consumer stream (in a step: behind the factorisation queued there): the points scaled per draw;
        // k(A, X) with the points as the rows and the observations -- the factorisation's pre-doubled rows -- as the columns of
        // the library's own cross-covariance launch, [H][Ap][Np]; Gamma_a = W k(X, a), no mean subtracted, behind column 0 =
        // the ordinary gamma; mu_a
        TIMED_S(ST_SCALE, G, launch_scale_rows(G, h->kg_pts.d(), kgA, kgAp, D, Dp, ls, hs, H, 1.0, h->kg_As.d(), h->kg_sA.d()));
        TIMED_S(ST_COV_CROSS, G, launch_cov_cross(G, h->kg_As.d(), h->kg_sA.d(), h->X2s.d(), h->s1.d(), h->htab.d(), h->kg_kxa.d(), kgA,
                                                  kgAp, Np, Dp, H, dev_kind(h)));
        HIPCHK(hipMemcpy2DAsync(h->kg_gammaS.d(), (size_t)S * Np * 8, h->gamma.d(), (size_t)Np * 8, (size_t)Np * 8, (size_t)H,
                                hipMemcpyDeviceToDevice, G));
        for (int d = 0; d < H; ++d)
            TIMED_S(ST_GAMMA_ALPHA, G, launch_gamma_cols(G, h->WT.d() + (size_t)d * nn, h->kg_kxa.d() + (size_t)d * kgAp * Np, (size_t)Np,
                                                         h->kg_gammaS.d() + ((size_t)d * S + 1) * Np, (int)N, Np, kgA));
        TIMED_S(ST_KG, G, launch_kg_mu(G, h->kg_gammaS.d(), h->htab.d(), Np, S, H, h->kg_mua.d()));
    }
    int item = 0, chunk = 0;
    for (int64_t c0 = 0; c0 < Mp; c0 += Mc, ++chunk) {
        const int mc = (int)std::min<int64_t>(Mc, Mp - c0);       // multiple of 128
        const int64_t nreal = std::min<int64_t>(mc, M - c0);      // real candidates in the chunk
        const double* xc = h->cand.d() + (size_t)c0 * D;
        spx_handle::ChunkBufs& cb = h->chunk[chunk & 1];
        double *Cs = cb.Cs.d(), *s2 = cb.s2.d();
        double* tm = per_sec ? cb.time_m.d() : nullptr;
        // the chunk-level buffers of this parity were last read (by EI finalize on G) two chunks ago
        if (P != G && chunk >= 2) HIPCHK(hipStreamWaitEvent(P, cb.consumed, 0));
        if (per_sec) {
            // log-duration GP: predicted duration of every candidate of the chunk, all draws in one launch
            const bool side = overlap && chunk == 0;         // (a step's first chunk: the objective's scaling runs on P0 meanwhile)
            hipStream_t T = side ? G : P;
            double* CsT = side ? h->chunk[1].Cs.d() : Cs;
            double* s2T = side ? h->chunk[1].s2.d() : s2;
            TIMED_S(ST_SCALE, T, launch_scale_rows(T, xc, nreal, mc, D, Dp, ls + (size_t)H * hs, hs, H, 2.0, CsT, s2T));
            TIMED_S(ST_CROSS_MEAN, T, launch_cross_mean(T, h->Xs.d() + (size_t)H * Np * Dp, h->s1.d() + (size_t)H * Np, CsT, s2T,
                                                        h->htab.d() + (size_t)H * SPX_HT, h->alpha.d() + (size_t)H * Np, tm,
                                                        (int)N, Np, mc, Dp, H, dev_kind(h)));
            if (keep_mom)   // predicted durations [H][mc] -> [H][Mp] for spx_get_time_mean
                HIPCHK(hipMemcpy2DAsync(h->mom_t.d() + c0, (size_t)Mp * 8, tm, (size_t)mc * 8,
                                        (size_t)std::min<int64_t>(mc, Mp - c0) * 8, (size_t)H, hipMemcpyDeviceToDevice, T));
        }
        if (time_only) continue;      // (the predicted durations of the chunk are in mom_t: nothing else was asked for)
        double* cp = constrained ? cb.con_p.d() : nullptr;
        if (constrained) {
            // P_d(x) of the chunk, all draws, on the producer stream ahead of the objective's work there: with one stream P is G,
            // with two the EI epilogues on G wait for K(X*,X) recorded on P after it.  alpha_c was made (and synchronised) by
            // factor_constraint.
            if (h->con_n > 0) {
                spx_handle* c = h->con;
                TIMED_S(ST_SCALE, P, launch_scale_rows(P, xc, nreal, mc, D, Dp, c->hyp.d() + 3, hs, H, 2.0, cb.con_Cs.d(),
                                                       cb.con_s2.d()));
                TIMED_S(ST_CROSS_MEAN, P, launch_constraint_prob(P, c->Xs.d(), c->s1.d(), cb.con_Cs.d(), cb.con_s2.d(),
                                                                 h->con_tab.d(), c->alpha.d(), cp, (int)c->N, c->Np, mc, Dp, H,
                                                                 dev_kind(h)));
            } else {
                TIMED_S(ST_CROSS_MEAN, P, launch_constraint_const(P, h->con_tab.d(), cp, mc, H));
            }
            if (keep_mom)   // P_d [H][mc] -> [H][Mp] for spx_get_constraint_prob
                HIPCHK(hipMemcpy2DAsync(h->mom_c.d() + c0, (size_t)Mp * 8, cp, (size_t)mc * 8,
                                        (size_t)std::min<int64_t>(mc, Mp - c0) * 8, (size_t)H, hipMemcpyDeviceToDevice, P));
        }
        // 2 * cand / ls and |cand / ls|^2 for every draw (one launch per chunk)
        hipStream_t Pc = (chunk == 0) ? P0 : P;       // (the first chunk's producer work of a step: beside the factorisation)
        TIMED_S(ST_SCALE, Pc, launch_scale_rows(Pc, xc, nreal, mc, D, Dp, ls, hs, H, 2.0, Cs, s2));
        if (ts) {   // the prior of the chunk's rows under every draw and path, on the consumer stream in front of the finishes that read it
            const double* par = h->ts_par.d();
            const size_t nnu = (size_t)H * h->ts_F * Dp;
            TIMED_S(ST_TS_PRIOR, G, launch_ts_prior(G, xc, nreal, D, Dp, par, par + nnu, h->ts_w.d(), h->ts_w_stride, par + nnu + h->ts_F,
                                                    h->ts_F, S, H, h->ts_pcand.d(), Mp, c0));
        }
        if (fused && (rc = hand_off(Pc, G, h->ev_p0))) return rc;
        if (fused)
            TIMED_S(ST_PREDICT_GEMM, G, launch_ei_fused128(G, dev_kind(h), h->WT.d(), h->gamma.d(), h->Xs.d(), h->s1.d(), Cs, s2,
                                                           h->htab.d(), tm, cp, h->best, h->ei_draw.d(), keep_mom ? h->mom_m.d() : nullptr,
                                                           keep_mom ? h->mom_v.d() : nullptr, (int)N, mc, Dp, H, c0, M, Mp, h->n_cu,
                                                           pass_acq, pass_par));
        for (int h0 = 0; h0 < (fused ? 0 : H); h0 += Hb, ++item) {
            const int nhb = std::min(Hb, H - h0);
            spx_handle::RingSlot& sl = h->ring[item % p.slots];
            if (P != G && item >= p.slots) HIPCHK(hipStreamWaitEvent(P, sl.consumed, 0));   // (by item - slots)
            hipStream_t Pi = (item == 0) ? Pc : P;
            double *Kst_k = sl.Kst.d(), *bgS_k = S > 0 ? sl.part_bgS.d() : nullptr;
            const bool corun = p.corun && item > 0;
            h->corun_launches += corun ? 1 : 0;
            TIMED_S(ST_COV_CROSS, Pi, launch_cov_cross(Pi, h->Xs.d() + (size_t)h0 * Np * Dp, h->s1.d() + (size_t)h0 * Np,
                                                      Cs + (size_t)h0 * mc * Dp, s2 + (size_t)h0 * mc,
                                                      h->htab.d() + (size_t)h0 * SPX_HT, Kst_k, (int)N, Np, mc, Dp, nhb, dev_kind(h),
                                                      p.cov_live_rows, p.cov_flat, corun));
            if ((rc = hand_off(Pi, G, sl.ready))) return rc;
            // with fantasies the launch's partial sums are consumed right away and sit at draws 0 .. nhb-1
            TIMED_S(ST_PREDICT_GEMM, G, launch_predict_gemm(G, h->opt.gemm_variant, h->WT.d() + (size_t)h0 * nn, Kst_k,
                                                            h->gamma.d() + (size_t)h0 * Np, h->part_ss.d(),
                                                            h->part_bg.d(), Np, mc, nhb, S > 0 ? nhb : H, S > 0 ? 0 : h0,
                                                            S > 0 ? gammaS_all + (size_t)h0 * S * Np : nullptr, S,
                                                            bgS_k, gemm_nlive));
            if (kg) {   // k(A, c) of the work item (the points as rows: the pass's own K(X*,X) launch over A rows), its lines, its values
                TIMED_S(ST_COV_CROSS, G, launch_cov_cross(G, h->kg_As.d() + (size_t)h0 * kgAp * Dp, h->kg_sA.d() + (size_t)h0 * kgAp,
                                                          Cs + (size_t)h0 * mc * Dp, s2 + (size_t)h0 * mc,
                                                          h->htab.d() + (size_t)h0 * SPX_HT, h->kg_Kac.d(), kgA, kgAp, mc, Dp, nhb,
                                                          dev_kind(h)));
                TIMED_S(ST_KG, G, {
                    launch_kg_lines(G, h->part_ss.d(), bgS_k, h->htab.d() + (size_t)h0 * SPX_HT, h->kg_Kac.d(), nrb, mc, nhb, S, kgAp, c0, M,
                                    Mp, h0, h->scratch.d(), h->kg_muc.d(), keep_mom ? h->mom_m.d() : nullptr,
                                    keep_mom ? h->mom_v.d() : nullptr, keep_mom ? h->kg_cov.d() : nullptr);
                    launch_kg_value(G, h->scratch.d(), h->kg_muc.d(), h->kg_mua.d() + (size_t)h0 * kgA, mc, nhb, S, c0, M, Mp, h0,
                                    h->ei_draw.d());
                });
            } else if (ts)
                TIMED_S(ST_TS_FINISH, G, launch_ts_finish(G, bgS_k, h->htab.d() + (size_t)h0 * SPX_HT, h->ts_pcand.d(), nrb, mc, nhb, S,
                                                          c0, M, Mp, h0, h->ts_path.d()));
            else if (S > 0)
                TIMED_S(ST_EI_FINALIZE, G, launch_ei_finalize_fant(G, h->part_ss.d(), bgS_k,
                                                                   h->htab.d() + (size_t)h0 * SPX_HT,
                                                                   h->bests.d() + (size_t)h0 * S,
                                                                   per_sec ? tm + (size_t)h0 * mc : nullptr,
                                                                   constrained ? cp + (size_t)h0 * mc : nullptr,
                                                                   h->ei_draw.d(), nrb, mc, nhb, S, c0, M, Mp, h0,
                                                                   h->scratch.d(), pass_acq, pass_par));
            if (P != G && (int64_t)item + p.slots < p.ring_items) HIPCHK(hipEventRecord(sl.consumed, G));   // (only where an item waits for it)
        }
        if (S == 0 && !fused)   // every draw of the chunk in one launch
            TIMED_S(ST_EI_FINALIZE, G, launch_ei_finalize(G, h->part_ss.d(), h->part_bg.d(), h->htab.d(), tm, cp, h->best,
                                                          h->ei_draw.d(), keep_mom ? h->mom_m.d() : nullptr,
                                                          keep_mom ? h->mom_v.d() : nullptr, nrb, mc, H, c0, M, Mp, 0, pass_acq,
                                                          pass_par));
        if (P != G) HIPCHK(hipEventRecord(cb.consumed, G));
    }
    // the duration / probability copies ran on P
    if ((per_sec || constrained) && keep_mom && (rc = hand_off(P, G, h->ev_p0))) return rc;
    // the winner (and, in a step, the factorisation's flags) go home through pinned memory with the last kernel's own stores
    const int n_info = p.n_info;
    if ((rc = h->pin_res.reserve(16 + (size_t)n_info * sizeof(int)))) return rc;
    double* mirror = (double*)h->pin_res.p;
    if (mes)   // behind the last finalize on the main stream: every draw's moments are complete
        TIMED(ST_MES, launch_mes(s, h->mom_m.d(), h->mom_v.d(), h->htab.d(), SPX_HT, h->best, M, Mp, H, mesJ, mesK, h->mes_bpart.d(),
                                 h->mes_part.d(), h->mes_G.d(), h->mes_ystar.d(), h->mes_fit.d(), h->ei_draw.d()));
    if (ehvi) {   // likewise; the second GP's moments were complete (and synchronised) before this pass began
        const spx_handle* c = h->sec;
        if (c->M != M || c->H != H || c->ei_plan.Mp != Mp)
            return fail(SPX_ERR_ARG, "internal error: the second GP's pass does not match the objective's (M, H, Mp)");
        const int nstrips = h->front_n + 1;
        TIMED(ST_EHVI, launch_ehvi(s, h->mom_m.d(), h->mom_v.d(), c->mom_m.d(), c->mom_v.d(), h->front_dev.d(),
                                   h->front_dev.d() + nstrips, nstrips, M, Mp, H, h->ei_draw.d()));
    }
    if (ts)
        TIMED(ST_TS_FINISH, launch_ts_argmin(s, h->ts_path.d(), M, Mp, H * S, h->ts_am_val.d(), (int64_t*)h->ts_am_idx.p,
                                             h->ts_out_val.d(), (int64_t*)h->ts_out_idx.p, h->index_base));
    else TIMED(ST_MEAN_ARGMAX, {
        launch_mean_argmax(s, h->ei_draw.d(), h->ei_mean.d(), M, Mp, H, h->am_val.d(), (int64_t*)h->am_idx.p, h->am_out_val.d(),
                           (int64_t*)h->am_out_idx.p, mirror, (const int*)h->info.p, n_info);
    });
    HIPCHK(hipEventRecord(t1, s));
    HIPCHK(hipStreamSynchronize(s));
    LAUNCHCHK();
    if (!ts) {
        h->best_val = mirror[0];
        h->best_idx = ((const int64_t*)mirror)[1];
    }
    if (factor_pending) {
        std::vector<int> info((const int*)(mirror + 2), (const int*)(mirror + 2) + n_info);
        if ((rc = finish_factor(h, info, false, false))) return rc;
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, t0, t1);
    if (h->opt.timing) {
        ev_collect(h);
        h->st_ms[ST_EI_RUN_TOTAL] += ms; h->st_n[ST_EI_RUN_TOTAL] += 1;
    }
    Held::Results r;
    r.time_only = time_only;         // (a time-only pass has no EI results: spx_get_best & co. refuse)
    r.ts = ts;                       // (paths and priors, nothing else: every EI getter refuses)
    r.moments = keep_mom && (S == 0 || kg) && !time_only;   // (KG: k_kg_lines wrote func_m / func_v from column 0)
    r.kg = kg;
    r.kg_lines = kg && keep_mom;
    if (kg) h->kg_last_A = kgA;
    r.tmean = keep_mom && per_sec;   // (with fantasies the pass keeps no func_m / func_v, but mom_t is written all the same)
    r.con = constrained && keep_mom && !time_only;
    r.ehvi = ehvi;
    r.mes = mes;
    if (mes) { h->mes_K = mesK; h->mes_J = mesJ; }
    if (h->comm && (rc = spx_comm_exchange(h, &r.global2d))) return rc;   // one process per GPU: the winner over all ranks
    return spx_hold(h, Held::RESULTS, r);
}

int spx_get_best(spx_handle* h, int64_t* best_idx, double* best_val)
{
    if (h && h->multi) return spx_multi_get_best(h->multi, best_idx, best_val);
    if (!h || !h->held.ei()) return fail(SPX_ERR_ARG, "spx_get_best: no results (call spx_ei_run)");
    if (best_idx) *best_idx = h->best_idx + h->index_base;
    if (best_val) *best_val = h->best_val;
    return SPX_OK;
}

int spx_get_ei_mean(spx_handle* h, double* out)
{
    if (h && h->multi) return spx_multi_get_ei_mean(h->multi, out);
    if (!h || !out || !h->held.ei()) return fail(SPX_ERR_ARG, "spx_get_ei_mean: no results / null output");
    int rc = ensure_init(h);
    if (rc) return rc;
    // after the all-reduce of a partitioned run: the GLOBAL mean (all draws of all ranks) of this handle's candidates
    const double* src = h->held.results.global2d ? h->ei_sum_full.d() + h->index_base : h->ei_mean.d();
    return stage_d2h(h, out, src, (size_t)h->M * 8, h->stream);
}

int spx_get_ei_draws(spx_handle* h, double* out)
{
    if (h && h->multi) return spx_multi_get_ei_draws(h->multi, out);
    if (!h || !out || !h->held.ei()) return fail(SPX_ERR_ARG, "spx_get_ei_draws: no results / null output");
    int rc = ensure_init(h);
    if (rc) return rc;
    const int64_t M = h->M, Mp = round_up(M, SPX_BN);
    const int H = h->H;
    std::vector<double> tmp((size_t)H * Mp);
    if ((rc = stage_d2h(h, tmp.data(), h->ei_draw.p, tmp.size() * 8, h->stream))) return rc;
    for (int64_t c = 0; c < M; ++c)
        for (int d = 0; d < H; ++d) out[(size_t)c * H + d] = tmp[(size_t)d * Mp + c];
    return SPX_OK;
}

// one [Mp]-strided row per draw of up to two results of the last pass, into the caller's M doubles each
static int get_draw_rows(spx_handle* h, const char* who, int32_t draw, const DevBuf& a, double* out_a,
                         const DevBuf* b = nullptr, double* out_b = nullptr)
{
    if (draw < 0 || draw >= h->H) return fail(SPX_ERR_ARG, "%s: draw out of range", who);
    int rc = ensure_init(h);
    if (rc) return rc;
    const int64_t Mp = round_up(h->M, SPX_BN);
    if (out_a) HIPCHK(hipMemcpy(out_a, a.d() + (size_t)draw * Mp, (size_t)h->M * 8, hipMemcpyDeviceToHost));
    if (b && out_b) HIPCHK(hipMemcpy(out_b, b->d() + (size_t)draw * Mp, (size_t)h->M * 8, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_get_moments(spx_handle* h, int32_t draw, double* func_m, double* func_v)
{
    if (h && h->multi) return spx_multi_get_moments(h->multi, draw, func_m, func_v);
    if (!h || !h->held.results.moments)
        return fail(SPX_ERR_ARG, "spx_get_moments: run spx_ei_run with SPX_FLAG_KEEP_MOMENTS first");
    if (h->held.results.ehvi && draw >= h->H && draw < 2 * h->H)    // the second GP's moments of an EHVI pass
        return spx_get_moments(h->sec, draw - h->H, func_m, func_v);
    return get_draw_rows(h, "spx_get_moments", draw, h->mom_m, func_m, &h->mom_v, func_v);
}

int spx_get_mes(spx_handle* h, int32_t draw, double* ystar, double* fit, double* G)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_get_mes: null handle");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_get_mes: SPX_ACQ_MES is single-device only (multi-device handle)");
    if (!h->held.results.mes) return fail(SPX_ERR_ARG, "spx_get_mes: no max-value entropy search results (run a pass with SPX_ACQ_MES set)");
    if (draw < 0 || draw >= h->H) return fail(SPX_ERR_ARG, "spx_get_mes: draw out of range");
    int rc = ensure_init(h);
    if (rc) return rc;
    const size_t K = (size_t)h->mes_K, J = (size_t)h->mes_J;
    if (ystar) HIPCHK(hipMemcpy(ystar, h->mes_ystar.d() + (size_t)draw * K, K * 8, hipMemcpyDeviceToHost));
    if (fit) HIPCHK(hipMemcpy(fit, h->mes_fit.d() + (size_t)draw * 8, 8 * 8, hipMemcpyDeviceToHost));
    if (G) HIPCHK(hipMemcpy(G, h->mes_G.d() + (size_t)draw * J, J * 8, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_get_kg_lines(spx_handle* h, int32_t draw, double* mu_a, double* cov)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_get_kg_lines: null handle");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_get_kg_lines: SPX_ACQ_KG is single-device only (multi-device handle)");
    if (!h->held.results.kg) return fail(SPX_ERR_ARG, "spx_get_kg_lines: no knowledge-gradient results (run a pass with SPX_ACQ_KG set)");
    if (draw < 0 || draw >= h->H) return fail(SPX_ERR_ARG, "spx_get_kg_lines: draw out of range");
    if (cov && !h->held.results.kg_lines)
        return fail(SPX_ERR_ARG, "spx_get_kg_lines: the covariances are kept by a pass with SPX_FLAG_KEEP_MOMENTS");
    int rc = ensure_init(h);
    if (rc) return rc;
    const size_t A = (size_t)h->kg_last_A;
    const int64_t Mp = round_up(h->M, SPX_BN);
    if (mu_a) HIPCHK(hipMemcpy(mu_a, h->kg_mua.d() + (size_t)draw * A, A * 8, hipMemcpyDeviceToHost));
    if (cov)
        HIPCHK(hipMemcpy2D(cov, (size_t)h->M * 8, h->kg_cov.d() + (size_t)draw * A * Mp, (size_t)Mp * 8, (size_t)h->M * 8, A,
                           hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_get_time_mean(spx_handle* h, int32_t draw, double* out)
{
    if (h && h->multi) return spx_multi_get_time_mean(h->multi, draw, out);
    if (!h || !out || !(h->held.results.moments || h->held.results.tmean) || h->nmodels != 2)
        return fail(SPX_ERR_ARG, "spx_get_time_mean: run spx_ei_run with SPX_FLAG_PER_SEC | SPX_FLAG_KEEP_MOMENTS first");
    return get_draw_rows(h, "spx_get_time_mean", draw, h->mom_t, out);
}

int spx_get_constraint_prob(spx_handle* h, int32_t draw, double* out)
{
    if (h && h->multi) return fail(SPX_ERR_ARG, "spx_get_constraint_prob: the constraint model is single-device only");
    if (!h || !out || !h->held.results.con)
        return fail(SPX_ERR_ARG, "spx_get_constraint_prob: run spx_ei_run with SPX_FLAG_CONSTRAINED | SPX_FLAG_KEEP_MOMENTS first");
    return get_draw_rows(h, "spx_get_constraint_prob", draw, h->mom_c, out);
}

// Element (ri, cj) of a 64 x 64 tile of the tile-major factor (k_lean_flow): tile (I, J) at (I nblk + J) * 4096 doubles; below
// the diagonal in accumulator order -- value q = 4 nt + r of thread t at ((q >> 1) * 256 + t) * 2 + (q & 1) is the element
// (16 (t >> 6) + ((t & 63) >> 4) + 4 r, 16 nt + (t & 15)) -- the diagonal tiles row-major (diag_block's Lkk)
static inline double tile_elem(const double* tile, bool diagonal, int ri, int cj)
{
    if (diagonal) return tile[ri * 64 + cj];
    const int t = (ri >> 4) * 64 + (ri & 3) * 16 + (cj & 15), q = (cj >> 4) * 4 + ((ri & 15) >> 2);
    return tile[((q >> 1) * 256 + t) * 2 + (q & 1)];
}

int spx_get_factor(spx_handle* h, int32_t draw, double* K, double* L, double* alpha)
{
    if (h && h->multi) return spx_multi_get_factor(h->multi, draw, K, L, alpha);
    if (!h || !h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_get_factor: call spx_factor first");
    const int nh = h->nmodels * h->H;
    if (draw < 0 || draw >= nh) return fail(SPX_ERR_ARG, "spx_get_factor: draw out of range");
    int rc = ensure_init(h);
    if (rc) return rc;
    const int Np = h->Np, Dp = h->Dp;
    const int64_t N = h->N;
    const size_t nn = (size_t)Np * Np;
    if (K) {
        if ((rc = h->scratch.reserve(nn * 8))) return rc;
        launch_cov_self(h->stream, h->Xs.d() + (size_t)draw * Np * Dp, h->s1.d() + (size_t)draw * Np,
                        h->X2s.d() + (size_t)draw * Np * Dp, h->htab.d() + (size_t)draw * SPX_HT,
                        h->scratch.d(), (int)N, Np, Dp, 1, false, dev_kind(h));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy2D(K, (size_t)N * 8, h->scratch.p, (size_t)Np * 8, (size_t)N * 8, (size_t)N, hipMemcpyDeviceToHost));
    }
    if (L && factor_tiled(h)) {
        std::vector<double> T(nn);
        HIPCHK(hipMemcpy(T.data(), h->Lm.d() + (size_t)draw * nn, nn * 8, hipMemcpyDeviceToHost));
        const int nblk = Np / SPX_NB;
        for (int64_t i = 0; i < N; ++i)
            for (int64_t j = 0; j < N; ++j) {
                const int I = (int)(i >> 6), J = (int)(j >> 6);
                L[i * N + j] = j <= i ? tile_elem(T.data() + ((size_t)I * nblk + J) * 4096, I == J, (int)(i & 63), (int)(j & 63)) : 0.0;
            }
    } else if (L) {
        HIPCHK(hipMemcpy2D(L, (size_t)N * 8, h->Lm.d() + (size_t)draw * nn, (size_t)Np * 8, (size_t)N * 8, (size_t)N,
                           hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < N; ++i)
            for (int64_t j = i + 1; j < N; ++j) L[i * N + j] = 0.0;
    }
    if (alpha) HIPCHK(hipMemcpy(alpha, h->alpha.d() + (size_t)draw * Np, (size_t)N * 8, hipMemcpyDeviceToHost));
    return SPX_OK;
}

// Rows [row0, row0 + nrows) of L (each N long, zeros above the diagonal) and gamma = L^-1 (vals - mean) of one draw.  What
// the pending branch needs of the factorisation of cov([comp; pend]) (GPEIChooser.py:219-249): with the P pending points
// last, the bottom P rows are [ (L_A^-1 B)^T | L_S ] -- B = cov(comp, pend), L_S the factor of the Schur complement -- so the
// posterior of the pending points is pend_m = L21 gamma[:N] + mean, pend_K = L_S L_S^T - noise I: a P x (N + P) block and one
// vector per draw instead of the whole N x N factor (1.6 MB instead of 671 MB at N = 2048, 20 draws, P = 4).
int spx_get_factor_rows(spx_handle* h, int32_t draw, int64_t row0, int64_t nrows, double* L_rows, double* gamma)
{
    if (h && h->multi) return spx_multi_get_factor_rows(h->multi, draw, row0, nrows, L_rows, gamma);
    if (!h || !h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_get_factor_rows: call spx_factor first");
    const int nh = h->nmodels * h->H;
    const int64_t N = h->N;
    if (draw < 0 || draw >= nh) return fail(SPX_ERR_ARG, "spx_get_factor_rows: draw out of range");
    if (row0 < 0 || nrows < 0 || row0 + nrows > N) return fail(SPX_ERR_ARG, "spx_get_factor_rows: rows out of range");
    int rc = ensure_init(h);
    if (rc) return rc;
    const int Np = h->Np;
    const size_t nn = (size_t)Np * Np;
    if (L_rows && nrows > 0 && factor_tiled(h)) {
        // (tile-major factor: the tiles (I, 0 .. I) of a block row are contiguous)
        const int nblk = Np / SPX_NB;
        std::vector<double> T;
        for (int I = (int)(row0 >> 6); I <= (int)((row0 + nrows - 1) >> 6); ++I) {
            T.resize((size_t)(I + 1) * 4096);
            HIPCHK(hipMemcpy(T.data(), h->Lm.d() + (size_t)draw * nn + (size_t)I * nblk * 4096, T.size() * 8, hipMemcpyDeviceToHost));
            for (int64_t i = std::max<int64_t>(row0, (int64_t)I * 64); i < std::min<int64_t>(row0 + nrows, (int64_t)(I + 1) * 64); ++i) {
                double* out = L_rows + (size_t)(i - row0) * N;
                const int ri = (int)(i & 63);
                for (int64_t j = 0; j < N; ++j)
                    out[j] = j <= i ? tile_elem(T.data() + (size_t)(j >> 6) * 4096, I == (int)(j >> 6), ri, (int)(j & 63)) : 0.0;
            }
        }
    } else if (L_rows && nrows > 0) {
        HIPCHK(hipMemcpy2D(L_rows, (size_t)N * 8, h->Lm.d() + (size_t)draw * nn + (size_t)row0 * Np, (size_t)Np * 8, (size_t)N * 8,
                           (size_t)nrows, hipMemcpyDeviceToHost));
        for (int64_t i = row0; i < row0 + nrows; ++i)
            for (int64_t j = i + 1; j < N; ++j) L_rows[(size_t)(i - row0) * N + j] = 0.0;
    }
    if (gamma) HIPCHK(hipMemcpy(gamma, h->gamma.d() + (size_t)draw * Np, (size_t)N * 8, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_get_cross_cov(spx_handle* h, int32_t draw, int64_t c0, int64_t nc, double* out)
{
    if (h && h->multi) return spx_multi_get_cross_cov(h->multi, draw, c0, nc, out);
    if (!h || !out || !h->held.has(Held::FACTOR) || !h->held.has(Held::CAND))
        return fail(SPX_ERR_ARG, "spx_get_cross_cov: need spx_factor and candidates");
    const int nh = h->nmodels * h->H;
    if (draw < 0 || draw >= nh || c0 < 0 || nc < 1 || c0 + nc > h->M)
        return fail(SPX_ERR_ARG, "spx_get_cross_cov: range error");
    int rc = ensure_init(h);
    if (rc) return rc;
    const int Np = h->Np, Dp = h->Dp, D = h->D, hs = 3 + D;
    const int mc = (int)round_up(nc, SPX_BN);
    DevBuf cs, s2, kst;
    if ((rc = cs.reserve((size_t)mc * Dp * 8)) || (rc = s2.reserve((size_t)mc * 8)) ||
        (rc = kst.reserve((size_t)Np * mc * 8))) {
        cs.release(); s2.release(); kst.release();
        return rc;
    }
    hipStream_t s = h->stream;
    launch_scale_rows(s, h->cand.d() + (size_t)c0 * D, nc, mc, D, Dp, h->hyp.d() + 3 + (size_t)draw * hs, hs, 1, 2.0,
                      cs.d(), s2.d());
    launch_cov_cross(s, h->Xs.d() + (size_t)draw * Np * Dp, h->s1.d() + (size_t)draw * Np, cs.d(), s2.d(),
                     h->htab.d() + (size_t)draw * SPX_HT, kst.d(), (int)h->N, Np, mc, Dp, 1, dev_kind(h), 0,
                     h->opt.cov_flat != 0);   // (option cov_flat holds here as in the EI pass: the two forms can be compared element by element)
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess)
        e = hipMemcpy2D(out, (size_t)nc * 8, kst.p, (size_t)mc * 8, (size_t)nc * 8, (size_t)h->N, hipMemcpyDeviceToHost);
    cs.release(); s2.release(); kst.release();
    if (e != hipSuccess) return fail(SPX_ERR_HIP, "spx_get_cross_cov: %s", hipGetErrorString(e));
    return SPX_OK;
}

static int gp_logprob_once(spx_handle* h, double* out);

int spx_gp_logprob(spx_handle* h, double* out)
{
    if (!h || !out) return fail(SPX_ERR_ARG, "spx_gp_logprob: null");
    if (h->multi) return spx_multi_gp_logprob(h->multi, out);
    h->handoff_timeout = false;
    int rc = gp_logprob_once(h, out);
    if (rc == SPX_ERR_HIP && h->handoff_timeout && h->last_factor->flow) {
        // never seen on a healthy device; if the one-launch data flow ever stalls (its spins are bounded), the call is
        // repeated with one launch per block column -- same kernels' arithmetic, same bits -- and the handle stays there
        note_flow_timeout(h);
        rc = gp_logprob_once(h, out);
        if (!rc) warn_flow_fallback(h);
    }
    return rc;
}

int spx_gp_logprob_rhs(spx_handle* h, const double* rows, const double* rhs, int32_t n_rows, double* lp_out)
{
    if (!h || !rows || !rhs || !lp_out) return fail(SPX_ERR_ARG, "spx_gp_logprob_rhs: null argument");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_gp_logprob_rhs: single-device only (multi-device handle)");
    if (n_rows < 1 || n_rows > 32) return fail(SPX_ERR_ARG, "spx_gp_logprob_rhs: 1 .. 32 rows per call (got %d)", n_rows);
    if (!h->held.has(Held::OBS)) return fail(SPX_ERR_ARG, "spx_gp_logprob_rhs: call spx_set_observations first (the points)");
    int rc = spx_set_hypers(h, rows, n_rows);
    if (rc) return rc;
    const size_t bytes = (size_t)n_rows * h->N * 8;
    if ((rc = h->rhs_rows.reserve(bytes))) return rc;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->rhs_rows.p, rhs, bytes, h->stream))) return rc;
    // (the copy is ordered in front of the factorisation on the same stream; the staging buffer is the caller's until the
    // stream has drained, which spx_gp_logprob waits for before it returns)
    h->rhs_rows_on = true;
    rc = spx_gp_logprob(h, lp_out);
    h->rhs_rows_on = false;
    (void)hipStreamSynchronize(h->stream);
    return rc;
}

static int gp_logprob_once(spx_handle* h, double* out)
{
    // the kernels write the H values and the H not-PD flags straight into pinned host memory: no device-to-host copies
    // (two of them, to pageable memory, were 40 us of a 95 us call at N = 64)
    int rc;
    if ((rc = ensure_init(h))) return rc;
    if ((rc = h->pin_res.reserve((size_t)h->H * 12))) return rc;
    double* lp_host = (double*)h->pin_res.p;
    int* info_host = (int*)(lp_host + h->H);
    h->fused_lp = lp_host; h->fused_info = info_host;
    rc = do_factor(h, true, true, true);   // K(X,X), Cholesky, forward solve -- no inverse; queued, not yet synchronised
    h->fused_lp = nullptr; h->fused_info = nullptr;
    if (rc) { h->info_clean_ptr = nullptr; return rc; }
    if ((rc = h->lp.reserve((size_t)h->H * 8))) return rc;
    std::vector<int> info(h->H);
    const FactorPlan& lp = h->lean_plan;    // (what do_factor just ran)
    const bool polled = lp.poll;
    if (lp.rl) {
        if (!lp.fused)   // (the fused launch has reduced the log-likelihood itself)
            launch_lean_logprob(h->stream, h->diagL.d(), h->rhs.d(), (const int*)h->info.p, lp_host, info_host, (int)h->N, lp.Np, h->H);
        // polled: the host watches the pinned flags of the fused launch.  What is still running when they have all arrived --
        // other workgroups' last instructions, the ticket reset -- is ordered in front of whatever this stream is given next.
        // Bounded: after 20 ms (a long call at N = 8192 takes 10) the stream is synchronised the ordinary way.
        // (the device-side flags count as clean again only once this call is known to have ended well)
        const void* const clean_ptr = h->info_clean_ptr;
        if (lp.fused) h->info_clean_ptr = nullptr;
        bool seen = false;
        if (polled) {
            volatile int* fl = (volatile int*)info_host;
            const auto t0 = std::chrono::steady_clock::now();
            for (unsigned spin = 0;; ++spin) {
                int k = 0;
                while (k < h->H && __atomic_load_n(&fl[k], __ATOMIC_ACQUIRE) != SPX_POLL_SENTINEL) ++k;
                if (k == h->H) { seen = true; break; }
                if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
            }
        }
        if (!seen) HIPCHK(hipStreamSynchronize(h->stream));
        LAUNCHCHK();
        if (polled)      // (a launch that never ran -- refused, or a device error -- leaves its flags untouched)
            for (int k = 0; k < h->H; ++k)
                if (info_host[k] == SPX_POLL_SENTINEL)
                    return fail(SPX_ERR_HIP, "spx_gp_logprob: the launch finished without delivering draw %d", k);
        // a hand-off that timed out: a workgroup that gives up later than the draw's reducing item leaves -1 behind it -- the
        // device-side flags are then zeroed again before the next one-launch call
        if (lp.fused) {
            bool timed_out = false;
            for (int k = 0; k < h->H; ++k) timed_out |= info_host[k] < 0;
            if (!timed_out) h->info_clean_ptr = clean_ptr;
        }
        memcpy(out, lp_host, (size_t)h->H * 8);
        memcpy(info.data(), info_host, (size_t)h->H * sizeof(int));
    } else {
        launch_logprob(h->stream, h->Lm.d(), h->rhs.d(), (size_t)SPX_NB * lp.Np, (const int*)h->info.p, h->lp.d(), lp.Np, h->H);
        HIPCHK(hipMemcpyAsync(out, h->lp.p, (size_t)h->H * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(info.data(), h->info.p, (size_t)h->H * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return finish_factor(h, info, true, true);
}

static int run_grid(spx_handle* h, const double* comp, const double* vals, const double* log_durs,
                    int64_t N, int32_t D, const double* cand, int64_t M, const double* hypers,
                    const double* time_hypers, int32_t H, int32_t flags, double* ei_mean_out,
                    double* ei_draw_out, int64_t* best_idx, double* best_val)
{
    int rc;
    if ((rc = spx_set_observations(h, comp, vals, N, D))) return rc;
    if ((rc = spx_set_candidates(h, cand, M, D, 0))) return rc;
    if ((rc = spx_set_hypers(h, hypers, H))) return rc;
    if (log_durs && (rc = spx_set_time_model(h, log_durs, time_hypers))) return rc;
    if ((rc = spx_ei_step(h, flags))) return rc;
    if ((rc = spx_get_best(h, best_idx, best_val))) return rc;
    if (ei_mean_out && (rc = spx_get_ei_mean(h, ei_mean_out))) return rc;
    if (ei_draw_out && (rc = spx_get_ei_draws(h, ei_draw_out))) return rc;
    return SPX_OK;
}

int spx_ei_grid(spx_handle* h, const double* comp, const double* vals, int64_t N, int32_t D,
                const double* cand, int64_t M, const double* hypers, int32_t H, int32_t flags,
                double* ei_mean_out, double* ei_draw_out, int64_t* best_idx, double* best_val)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_ei_grid: null handle");
    return run_grid(h, comp, vals, nullptr, N, D, cand, M, hypers, nullptr, H, flags & ~SPX_FLAG_PER_SEC,
                    ei_mean_out, ei_draw_out, best_idx, best_val);
}

int spx_ei_per_sec_grid(spx_handle* h, const double* comp, const double* vals, const double* log_durs,
                        int64_t N, int32_t D, const double* cand, int64_t M, const double* hypers,
                        const double* time_hypers, int32_t H, int32_t flags, double* ei_mean_out,
                        double* ei_draw_out, int64_t* best_idx, double* best_val)
{
    if (!h || !log_durs || !time_hypers) return fail(SPX_ERR_ARG, "spx_ei_per_sec_grid: null argument");
    // (under SPX_ACQ_EHVI log_durs / time_hypers are the second objective's values and draws, and nothing is per second)
    const bool ehvi = !h->multi && h->acq == SPX_ACQ_EHVI;
    return run_grid(h, comp, vals, log_durs, N, D, cand, M, hypers, time_hypers, H,
                    ehvi ? (flags & ~SPX_FLAG_PER_SEC) : (flags | SPX_FLAG_PER_SEC),
                    ei_mean_out, ei_draw_out, best_idx, best_val);
}

int spx_sobol_grid(spx_handle* h, const uint32_t* dirs, int32_t dim_max, int32_t dim, int64_t n,
                   int64_t skip, double* grid_out, int32_t as_candidates, double* kernel_ms)
{
    if (h && h->multi) return spx_multi_sobol_grid(h->multi, dirs, dim_max, dim, n, skip, grid_out, as_candidates, kernel_ms);
    if (!h || !dirs || dim < 1 || dim > dim_max || n < 1)
        return fail(SPX_ERR_ARG, "spx_sobol_grid: bad arguments (dim=%d of %d, n=%lld)", dim, dim_max, (long long)n);
    if (skip + n - 2 >= (1ll << 30) || skip < -(1ll << 40))
        return fail(SPX_ERR_ARG, "spx_sobol_grid: skip + n - 2 = %lld does not fit 30 direction columns "
                    "(the reference stops with 'Too many calls')", (long long)(skip + n - 2));
    if (as_candidates && h->held.has(Held::OBS) && dim != h->D)
        return fail(SPX_ERR_ARG, "spx_sobol_grid: dim=%d but observations have D=%d", dim, h->D);
    int rc = ensure_init(h);
    if (rc) return rc;
    hipStream_t s = h->stream;
    const size_t tbytes = (size_t)dim * 30 * sizeof(uint32_t);
    if ((rc = h->sobol_dirs.reserve(tbytes))) return rc;
    if (as_candidates) spx_drop(h, Held::CAND);
    DevBuf& dst = as_candidates ? h->cand : h->sobol_out;
    if ((rc = dst.reserve((size_t)n * dim * 8))) return rc;
    HIPCHK(hipMemcpyAsync(h->sobol_dirs.p, dirs, tbytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->ev_t0, s));
    launch_sobol_grid(s, (const uint32_t*)h->sobol_dirs.p, dim, n, skip, dst.d());
    HIPCHK(hipEventRecord(h->ev_t1, s));
    if (grid_out) HIPCHK(hipMemcpyAsync(grid_out, dst.p, (size_t)n * dim * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    LAUNCHCHK();
    if (kernel_ms) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
        *kernel_ms = ms;
    }
    if (as_candidates) {
        if (!h->held.has(Held::OBS)) { h->D = dim; h->Dp = padded_dim(dim); }
        h->M = n; h->index_base = 0;
        return spx_hold(h, Held::CAND);
    }
    return SPX_OK;
}

// ---- the refinement objective: both entry points are these helpers plus their own checks and choice of sides --------

// One set of rows a call solves against: model `model` of r's tables (1: the time model's rows H..2H-1, into pt_kt /
// pt_dkt), and with `solve` t = W k, z = W^T t = K^-1 k in r's pt_t / pt_z.  r is the calling handle itself, its internal
// full handle or its constraint handle.
struct RefineRows { spx_handle* r; int model; bool solve; };

static int refine_rows_reserve(const spx_handle* h, const RefineRows& rr, int P)
{
    int rc;
    spx_handle* r = rr.r;
    const size_t vec = (size_t)h->H * P * r->Np * 8;
    if ((rc = (rr.model ? r->pt_kt : r->pt_k).reserve(vec))) return rc;
    if ((rc = (rr.model ? r->pt_dkt : r->pt_dk).reserve(vec))) return rc;
    if (rr.solve) {
        if ((rc = r->pt_t.reserve(vec))) return rc;
        if ((rc = r->pt_z.reserve(vec))) return rc;
    }
    return SPX_OK;
}

// k and dk/dr2 at the staged points, then the two solves; every launch goes on the calling handle's stream
static void refine_rows_launch(spx_handle* h, const RefineRows& rr, int P)
{
    spx_handle* r = rr.r;
    const int H = h->H, D = h->D, Dp = h->Dp, Np = r->Np;
    double* k = (rr.model ? r->pt_kt : r->pt_k).d();
    double* dk = (rr.model ? r->pt_dkt : r->pt_dk).d();
    hipStream_t s = h->stream;
    const size_t m = (size_t)rr.model * H;
    launch_point_cov(s, r->Xs.d() + m * Np * Dp, r->s1.d() + m * Np, r->hyp.d() + m * (3 + D), r->htab.d() + m * SPX_HT,
                     h->pt_x.d(), k, dk, (int)r->N, Np, D, Dp, H, P, dev_kind(h));
    if (rr.solve) {
        launch_trimv_multi(s, r->WT.d(), k, r->pt_t.d(), Np, H, P);                // t = W k
        launch_trimvT_multi(s, r->WT.d(), r->pt_t.d(), r->pt_z.d(), Np, H, P);     // z = W^T t = K^-1 k
    }
}

// model `model` of r's tables as one side of the finish, with gradient weights w
static FinishSide refine_side(const spx_handle* h, const spx_handle* r, int model, const double* w)
{
    const size_t m = (size_t)model * h->H;
    return FinishSide{r->Xs.d() + m * r->Np * h->Dp, r->hyp.d() + m * (3 + h->D), model ? r->pt_dkt.d() : r->pt_dk.d(), w,
                      (int)r->N, r->Np};
}

// Reserve everything the call needs before anything is queued, build alpha_s = W^T Gamma_s = K^-1 (fant_s - mean) for
// every fantasy column once per set of fantasies (:501-502), stage the points and solve against every set of rows.
static int refine_solve(spx_handle* h, const double* points, int P, const RefineRows* rows, int n_rows)
{
    int rc;
    const int H = h->H, D = h->D, Np = h->Np, S = h->S;
    if ((rc = h->pt_x.reserve((size_t)P * D * 8))) return rc;
    if ((rc = h->pt_out.reserve((size_t)H * P * (1 + D) * 8))) return rc;
    for (int i = 0; i < n_rows; ++i)
        if ((rc = refine_rows_reserve(h, rows[i], P))) return rc;
    if (S > 0) {
        if ((rc = h->pt_u.reserve((size_t)H * P * Np * 8))) return rc;
        if (!h->held.has(Held::ALPHA_S)) {
            if ((rc = h->alphaS.reserve((size_t)H * S * Np * 8))) return rc;
            launch_trimvT_multi(h->stream, h->WT.d(), h->gammaS.d(), h->alphaS.d(), Np, H, S);
            if ((rc = spx_hold(h, Held::ALPHA_S))) return rc;
        }
    }
    stage_begin(h);
    if ((rc = stage_h2d(h, h->pt_x.p, points, (size_t)P * D * 8, h->stream))) return rc;
    for (int i = 0; i < n_rows; ++i) refine_rows_launch(h, rows[i], P);
    return SPX_OK;
}

// the finish over the mean side (the handle's own rows), the variance side v and the third side c3 (n = 0: none), then the
// read-back and the sum over draws in draw order, as grad_optimize_ei_over_hypers does (GPEIOptChooser.py:368-380,
// GPConstrainedEIChooser.py:471-501)
static int refine_finish(spx_handle* h, const spx_handle* v, const FinishSide& c3, const double* k3, const double* tab3,
                         bool constrained, double best, int P, double* neg, double* grad)
{
    int rc;
    const int H = h->H, D = h->D, S = h->S;
    FinishArgs a{};
    a.m = refine_side(h, h, 0, h->alpha.d());
    a.v = refine_side(h, v, 0, v->pt_z.d());
    a.c = c3;
    a.htab = h->htab.d(); a.k = h->pt_k.d(); a.t = v->pt_t.d(); a.k3 = k3; a.tab3 = tab3;
    a.x = h->pt_x.d(); a.best = best; a.out = h->pt_out.d();
    a.D = D; a.Dp = h->Dp; a.nh = H; a.P = P; a.S = S;
    a.acq = constrained ? SPX_ACQ_EI : h->acq; a.par = constrained ? 0.0 : h->acq_par;
    if (a.acq == SPX_ACQ_MES) { a.ystar = h->mes_ystar.d(); a.par = (double)h->mes_K; }
    if (S > 0) {
        a.gammaS = h->gammaS.d(); a.alphaS = h->alphaS.d(); a.uvec = h->pt_u.d();
        if (!constrained) a.bests = h->bests.d();
    }
    launch_point_finish(h->stream, a, constrained);
    std::vector<double> out((size_t)H * P * (1 + D));
    if ((rc = stage_d2h(h, out.data(), h->pt_out.p, out.size() * 8, h->stream))) return rc;
    LAUNCHCHK();
    for (int p = 0; p < P; ++p) {
        double f = 0.0;
        double* g = grad + (size_t)p * D;
        for (int d = 0; d < D; ++d) g[d] = 0.0;
        for (int i = 0; i < H; ++i) {
            const double* o = &out[((size_t)i * P + p) * (1 + D)];
            f += -o[0];
            for (int d = 0; d < D; ++d) g[d] = g[d] + o[1 + d];
        }
        neg[p] = f;
    }
    return SPX_OK;
}

int spx_ei_grad_batch(spx_handle* h, const double* points, int32_t P, double* neg_ei, double* grad)
{
    if (!h || !points || !neg_ei || !grad || P < 1) return fail(SPX_ERR_ARG, "spx_ei_grad_batch: bad argument");
    if (h->multi) return spx_multi_ei_grad_batch(h->multi, points, P, neg_ei, grad);
    if (h->acq == SPX_ACQ_EHVI)
        return fail(SPX_ERR_ARG, "spx_ei_grad_batch: not defined under SPX_ACQ_EHVI (its refinement needs the second GP's variance "
                                 "gradient; the grid pass is the whole of it)");
    if (h->acq == SPX_ACQ_KG)
        return fail(SPX_ERR_ARG, "spx_ei_grad_batch: not defined under SPX_ACQ_KG (its refinement needs the gradient of the "
                                 "envelope; the grid pass is the whole of it)");
    if (!h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_ei_grad_batch: call spx_factor (or spx_ei_grid) first");
    const bool per_sec = (h->nmodels == 2);   // a time model was factored: EI per second (GPEIperSecChooser.py:349-434)
    if (per_sec && h->acq != SPX_ACQ_EI)
        return fail(SPX_ERR_ARG, "spx_ei_grad_batch: a time model is factored, and per second is defined for SPX_ACQ_EI only "
                                 "(spx_set_acquisition)");
    if (h->S > 0 && per_sec)
        return fail(SPX_ERR_ARG, "spx_ei_grad_batch: fantasies with a time model are not defined "
                    "(the reference's per-second refinement ignores pending jobs)");
    // MES: against the y* table of the last MES pass, held fixed (a reader of it: nothing is dropped)
    if (h->acq == SPX_ACQ_MES && !h->held.results.mes)
        return fail(SPX_ERR_ARG, "spx_ei_grad_batch: SPX_ACQ_MES needs the y* table of a max-value entropy search pass "
                                 "(spx_ei_run / spx_ei_step / spx_ei_grid with SPX_ACQ_MES set)");
    int rc = ensure_init(h);
    if (rc) return rc;
    // the handle's own rows, and k and dk/dr2 of the log-duration GP (table rows H..2H-1)
    const RefineRows rows[2] = {{h, 0, true}, {h, 1, false}};
    if ((rc = refine_solve(h, points, P, rows, per_sec ? 2 : 1))) return rc;
    FinishSide tm{};
    if (per_sec) tm = refine_side(h, h, 1, h->alpha.d() + (size_t)h->H * h->Np);
    return refine_finish(h, h, tm, per_sec ? h->pt_kt.d() : nullptr,
                         per_sec ? h->htab.d() + (size_t)h->H * SPX_HT : nullptr, false, h->best, P, neg_ei, grad);
}

int spx_ei_grad(spx_handle* h, const double* point, double* neg_ei_sum, double* grad)
{
    return spx_ei_grad_batch(h, point, 1, neg_ei_sum, grad);
}

// W_f = L_f^-1, L_f L_f^T = amp2 (corr(ls; X_c, X_c) + 1e-6 I) + noise I: the objective's draws over the constraint model's
// points, through the ordinary factorisation path on an internal handle.  Not positive definite: draw 3H + d.
static int ensure_full_factor(spx_handle* h)
{
    if (h->held.has(Held::FULL_FACTOR)) return SPX_OK;
    int rc;
    if (!h->full) {
        if ((rc = spx_create(h->device, &h->full))) return rc;
        h->full->opt.stage_copies = h->opt.stage_copies;
        h->full->opt.cov_kind = h->opt.cov_kind;     // (from here on option "covar" reaches it: opt_covar)
    }
    spx_handle* f = h->full;
    const std::vector<double> zeros((size_t)h->con_n, 0.0);   // (the values are not read: only W_f and the scaled rows are)
    if ((rc = spx_set_observations(f, h->con_comp_host.data(), zeros.data(), h->con_n, h->D))) return rc;
    if ((rc = spx_set_hypers(f, h->hyp_host.data(), h->H))) return rc;
    rc = spx_factor(f);
    if (rc == SPX_ERR_NOT_PD) {
        h->not_pd_draw = 3 * h->H + f->not_pd_draw;
        h->not_pd_pivot = f->not_pd_pivot;
        return fail(SPX_ERR_NOT_PD, "%d-th leading minor of the array is not positive definite (draw %d, objective over the "
                                    "constraint model's points)", f->not_pd_pivot + 1, f->not_pd_draw);
    }
    if (rc) return rc;
    return spx_hold(h, Held::FULL_FACTOR);
}

int spx_constrained_ei_grad_batch(spx_handle* h, const double* points, int32_t P, double best, double* neg_cei, double* grad)
{
    if (!h || !points || !neg_cei || !grad || P < 1) return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: bad argument");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: the constraint model is single-device only "
                                           "(multi-device handle)");
    if (h->acq != SPX_ACQ_EI)
        return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: the constrained objective is defined for SPX_ACQ_EI only "
                                 "(spx_set_acquisition)");
    if (!h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: call spx_factor (or spx_ei_step) first");
    if (!h->held.has(Held::CON)) return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: needs spx_set_constraint_model");
    if (h->nmodels == 2) return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: not defined with a time model");
    if ((int64_t)h->con_tab_host.size() != (int64_t)h->H * SPX_HT)
        return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: the constraint model has a different number of draws");
    const int64_t Nc = h->con_n;
    spx_handle* c = Nc > 0 ? h->con : nullptr;
    if (c && (c->H != h->H || c->D != h->D))
        return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: the constraint model does not match the objective's H / D");
    if (c && !h->held.has(Held::CON_FACTOR))
        return fail(SPX_ERR_ARG, "spx_constrained_ei_grad_batch: the constraint model is not factored (spx_factor after "
                                 "spx_set_constraint_model)");
    int rc = ensure_init(h);
    if (rc) return rc;
    const bool two_factor = (h->S == 0 && c);        // variance over X_c (the quirk of :692-803)
    if (two_factor && (rc = ensure_full_factor(h))) return rc;
    RefineRows rows[3] = {{h, 0, !two_factor}};
    int n_rows = 1;
    // k_f, dk_f: the objective's length scales against X_c; t_f = W_f k_f, z_f = W_f^T t_f
    if (two_factor) rows[n_rows++] = {h->full, 0, true};
    // k_c, dk_c: the constraint GP's own length scales and amplitude
    if (c) rows[n_rows++] = {c, 0, false};
    if ((rc = refine_solve(h, points, P, rows, n_rows))) return rc;
    FinishSide cm{};
    if (c) cm = refine_side(h, c, 0, c->alpha.d());
    // no violation seen, no pending job: comp == compfull and P = 1 -- spx_ei_grad_batch's own arithmetic
    return refine_finish(h, two_factor ? h->full : h, cm, c ? c->pt_k.d() : nullptr, h->con_tab.d(), h->S > 0 || c, best, P,
                         neg_cei, grad);
}

// Main effects of the posterior mean (spx.h).  The (D T + 1) Q structured rows are formed on the device (k_effects_rows) and
// scored by the ordinary pass with the moments kept -- ei_run_impl, one call per plan_effects pass, so a row's func_m is the
// bits spx_ei_run + spx_get_moments give for it -- and the kept means are reduced on the device (k_effects_mean).  The pass
// runs as SPX_ACQ_EI whatever the handle is set to (the moments do not depend on it; the setting is put back), and its own
// results (the winner, the EI values) are not kept: the call drops CAND, and with it RESULTS, before its first mutation and
// leaves them dropped.
int spx_main_effects(spx_handle* h, const double* base, int32_t Q, const double* levels, int32_t T, double* curves,
                     double* base_mean)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_main_effects: null handle");
    if (!base || !levels || !curves) return fail(SPX_ERR_ARG, "spx_main_effects: base, levels and curves must not be NULL");
    if (Q < 1 || Q > NP_PAIRWISE_MAX_N)
        return fail(SPX_ERR_ARG, "spx_main_effects: Q=%d base points (allowed: 1 .. %d)", (int)Q, NP_PAIRWISE_MAX_N);
    if (T < 1) return fail(SPX_ERR_ARG, "spx_main_effects: T=%d levels (allowed: >= 1)", (int)T);
    if (h->multi) return fail(SPX_ERR_ARG, "spx_main_effects: single-GPU handles only (multi-device handle)");
    if (h->comm) return fail(SPX_ERR_ARG, "spx_main_effects: single-GPU handles only (communicator attached)");
    if (h->part_ph > 1 || h->part_M > 0) return fail(SPX_ERR_ARG, "spx_main_effects: not available with a 2-D partition");
    if (!h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_main_effects: call spx_factor first");
    if (h->held.has(Held::FANT))
        return fail(SPX_ERR_ARG, "spx_main_effects: fantasies are held (the resident rows include pending points); clear them first");
    EffectsShape sh;
    sh.D = h->D; sh.H = h->H; sh.Q = Q; sh.T = T; sh.pass_rows_opt = h->opt.effects_pass_rows;
    if (((int64_t)h->D * T + 1) > SPX_EFFECTS_MAX_ROWS / Q)
        return fail(SPX_ERR_ARG, "spx_main_effects: (D T + 1) Q = (%d x %d + 1) x %d rows (allowed: up to %lld)", h->D, (int)T, (int)Q,
                    (long long)SPX_EFFECTS_MAX_ROWS);
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::CAND);          // and RESULTS, which are made from them
    EffectsPlan& p = h->effects_plan;
    p = plan_effects(sh);
    const int D = h->D, H = h->H;
    if ((rc = h->eff_in.reserve(p.in_bytes))) return rc;
    if ((rc = h->eff_out.reserve(p.out_bytes))) return rc;
    if ((rc = h->cand.reserve(p.cand_bytes))) return rc;
    if (p.gather && (rc = h->eff_m.reserve(p.gather_bytes))) return rc;
    double* d_base = h->eff_in.d();
    double* d_levels = d_base + (size_t)Q * D;
    double* d_curves = h->eff_out.d();
    double* d_bmean = d_curves + (size_t)H * p.nblocks;
    stage_begin(h);
    if ((rc = stage_h2d(h, d_base, base, (size_t)Q * D * 8, h->stream))) return rc;
    if ((rc = stage_h2d(h, d_levels, levels, (size_t)T * 8, h->stream))) return rc;
    const int acq = h->acq;
    const double acq_par = h->acq_par;
    h->acq = SPX_ACQ_EI; h->acq_par = 0.0;
    h->index_base = 0;
    for (int64_t r0 = 0; r0 < p.rows && !rc; r0 += p.pass_rows) {
        const int64_t m = std::min<int64_t>(p.pass_rows, p.rows - r0);
        launch_effects_rows(h->stream, d_base, d_levels, D, T, Q, r0, m, h->cand.d());
        // (the pass may read the rows on a producer stream of its own: they are complete before it is queued)
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) { rc = fail(SPX_ERR_HIP, "spx_main_effects: k_effects_rows failed: %s", hipGetErrorString(e)); break; }
        h->M = m;
        if ((rc = spx_hold(h, Held::CAND))) break;
        if ((rc = ei_run_impl(h, SPX_FLAG_KEEP_MOMENTS, false))) break;
        if (p.gather) {
            const int64_t Mp = h->ei_plan.Mp;
            e = hipMemcpy2DAsync(h->eff_m.d() + r0, (size_t)p.rows * 8, h->mom_m.d(), (size_t)Mp * 8, (size_t)m * 8, (size_t)H,
                                 hipMemcpyDeviceToDevice, h->stream);
            if (e != hipSuccess) { (void)hipGetLastError(); rc = fail(SPX_ERR_HIP, "spx_main_effects: hipMemcpy2DAsync failed: %s", hipGetErrorString(e)); }
        }
    }
    h->acq = acq; h->acq_par = acq_par;
    if (!rc) {
        launch_effects_mean(h->stream, p, p.gather ? h->eff_m.d() : h->mom_m.d(), p.gather ? p.rows : h->ei_plan.Mp, Q, H, d_curves,
                            d_bmean);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(SPX_ERR_HIP, "spx_main_effects: k_effects_mean failed: %s", hipGetErrorString(e));
    }
    if (!rc) rc = stage_d2h(h, curves, d_curves, (size_t)H * p.nblocks * 8, h->stream);
    if (!rc && base_mean) rc = stage_d2h(h, base_mean, d_bmean, (size_t)H * Q * 8, h->stream);
    if (rc) { (void)hipStreamSynchronize(h->stream); (void)hipGetLastError(); }
    spx_drop(h, Held::CAND);          // the rows of the last pass are nobody's candidates
    h->M = 0;
    return rc;
}

// Leave-one-out cross-validation of the resident factorisation (spx.h).  A reader, as spx_get_factor is: every refusal is
// decided before a device is touched, nothing of `held` is set or dropped, and the only thing written on the device is the
// call's own output buffer.  K^-1 = W^T W, so diag(K^-1) is the squared row norms of the resident WT (k_loo_diag).
int spx_loo(spx_handle* h, int32_t model, double* loo_mean, double* loo_var, double* kinv_diag)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_loo: null handle");
    if (!loo_mean || !loo_var) return fail(SPX_ERR_ARG, "spx_loo: loo_mean and loo_var must not be NULL");
    if (model != SPX_LOO_OBJECTIVE && model != SPX_LOO_TIME)
        return fail(SPX_ERR_ARG, "spx_loo: model=%d (allowed: SPX_LOO_OBJECTIVE, SPX_LOO_TIME)", (int)model);
    if (h->multi) return fail(SPX_ERR_ARG, "spx_loo: single-GPU handles only (multi-device handle)");
    if (h->comm) return fail(SPX_ERR_ARG, "spx_loo: single-GPU handles only (communicator attached)");
    if (h->part_ph > 1 || h->part_M > 0) return fail(SPX_ERR_ARG, "spx_loo: not available with a 2-D partition");
    if (!h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_loo: call spx_factor first");
    if (h->held.has(Held::FANT))
        return fail(SPX_ERR_ARG, "spx_loo: fantasies are held (the resident rows include pending points); clear them first");
    if (model == SPX_LOO_TIME && h->nmodels < 2)
        return fail(SPX_ERR_ARG, "spx_loo: SPX_LOO_TIME needs a factorisation made with a time model (spx_set_time_model, then spx_factor)");
    int rc = ensure_init(h);
    if (rc) return rc;
    const int H = h->H, Np = h->Np, N = (int)h->N;
    const size_t hn = (size_t)H * N;
    if ((rc = h->loo_out.reserve(3 * hn * 8))) return rc;
    double* out = h->loo_out.d();
    const size_t m0 = (size_t)model * H;              // the time model's draws follow the objective's in WT and alpha
    launch_loo_diag(h->stream, h->WT.d() + m0 * Np * Np, h->alpha.d() + m0 * Np, model ? h->ldur.d() : h->vals.d(), N, Np, H,
                    out, out + hn, out + 2 * hn);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream); (void)hipGetLastError();
        return fail(SPX_ERR_HIP, "spx_loo: k_loo_diag failed: %s", hipGetErrorString(e));
    }
    rc = stage_d2h(h, loo_mean, out, hn * 8, h->stream);
    if (!rc) rc = stage_d2h(h, loo_var, out + hn, hn * 8, h->stream);
    if (!rc && kinv_diag) rc = stage_d2h(h, kinv_diag, out + 2 * hn, hn * 8, h->stream);
    if (rc) { (void)hipStreamSynchronize(h->stream); (void)hipGetLastError(); }
    return rc;
}

// Thompson sampling by pathwise conditioning (spx.h).  Every refusal is decided from the host's record and the caller's arrays
// before a device is touched.  Then: the frequencies on the host (one IEEE operation each), one upload, the prior at the
// observations (k_ts_prior), the right-hand sides (k_ts_rhs), Gamma through launch_gamma_multi, and the candidates through
// ei_run_impl's S > 0 GEMM branch -- every chunk, draw group, stream count and the padding skip are that pass's -- with
// k_ts_prior per chunk, k_ts_finish per work item and the per-path argmin behind the last one; ONE synchronisation.
int spx_thompson(spx_handle* h, int32_t F, int32_t S, const double* omega_z, const double* chi, const double* phase,
                 const double* w, const double* eps, int32_t per_draw, int64_t* idx_out, double* min_out)
{
#pragma clang fp contract(off)
    if (!h) return fail(SPX_ERR_ARG, "spx_thompson: null handle");
    if (h->multi) return fail(SPX_ERR_ARG, "spx_thompson: single-GPU handles only (multi-device handle)");
    if (h->comm) return fail(SPX_ERR_ARG, "spx_thompson: single-GPU handles only (communicator attached)");
    if (h->part_ph > 1 || h->part_M > 0) return fail(SPX_ERR_ARG, "spx_thompson: not available with a 2-D partition");
    if (!h->held.has(Held::FACTOR)) return fail(SPX_ERR_ARG, "spx_thompson: call spx_factor first");
    if (!h->held.has(Held::CAND)) return fail(SPX_ERR_ARG, "spx_thompson: no candidates set");
    if (h->held.has(Held::FANT))
        return fail(SPX_ERR_ARG, "spx_thompson: fantasies are held (the resident rows include pending points); clear them first");
    if (F < 16 || F > SPX_TS_MAX_FEATURES || F % 16)
        return fail(SPX_ERR_ARG, "spx_thompson: F=%d features (allowed: a multiple of 16 in 16 .. %d)", (int)F, SPX_TS_MAX_FEATURES);
    if (S < 1 || S > SPX_TS_MAX_PATHS) return fail(SPX_ERR_ARG, "spx_thompson: S=%d paths (allowed: 1 .. %d)", (int)S, SPX_TS_MAX_PATHS);
    const int kind = h->opt.cov_kind;
    const bool matern = kind == SPX_COVAR_MATERN52 || kind == SPX_COVAR_MATERN32;
    if (!omega_z || !phase || !w || !eps || !idx_out || !min_out || (matern && !chi))
        return fail(SPX_ERR_ARG, "spx_thompson: omega_z, phase, w, eps, idx_out and min_out must not be NULL%s",
                    matern ? " (nor chi under a Matern covariance)" : "");
    for (int f = 0; f < F; ++f) {
        if (matern && !(chi[f] > 0.0 && chi[f] <= 1.79769313486231570815e308))
            return fail(SPX_ERR_ARG, "spx_thompson: chi[%d] = %g (must be finite and > 0)", f, chi[f]);
        if (!(phase[f] >= 0.0 && phase[f] < 1.0))
            return fail(SPX_ERR_ARG, "spx_thompson: phase[%d] = %g (must lie in [0, 1): the phase in turns)", f, phase[f]);
    }
    TsShape tsh;
    tsh.N = h->N; tsh.M = h->M; tsh.Np = h->Np; tsh.D = h->D; tsh.H = h->H; tsh.S = S; tsh.F = F; tsh.per_draw = per_draw != 0;
    const TsPlan tp = plan_ts(tsh);
    if (!tp.fits)
        return fail(SPX_ERR_ARG, "spx_thompson: H S Mp 8 = %d x %d x %lld x 8 bytes of paths (allowed: up to %lld bytes, H S <= 65535)",
                    h->H, (int)S, (long long)tp.Mp, (long long)SPX_TS_MAX_PATH_BYTES);
    if ((int64_t)h->hyp_host.size() != (int64_t)h->H * (3 + h->D))
        return fail(SPX_ERR_ARG, "spx_thompson: internal error: the resident hypers do not match H / D");
    int rc = ensure_init(h);
    if (rc) return rc;
    spx_drop(h, Held::RESULTS);      // the call overwrites them; the factor, the candidates and every setting stay
    const int H = h->H, D = h->D, Dp = tp.Dp, Np = h->Np, hs = 3 + D;
    const int64_t N = h->N, M = h->M;
    // frequencies in turns, nu[d][f][j] = (omega_z[f][j] t_f) / (TWO_PI ls[d][j]) with t_f = sqrt(2 nu / chi_f) (1 for ARDSE / SE;
    // SE: unit length scales), zero in the pad dimensions; scale_d = sqrt(2 amp2_d / F); sig_d = sqrt(noise_d + 1e-6 amp2_d)
    std::vector<double> par(tp.par_doubles, 0.0);
    double* nu = par.data();
    double* ph = nu + (size_t)H * F * Dp;
    double* scale = ph + F;
    double* sig = scale + H;
    const double two_nu = kind == SPX_COVAR_MATERN52 ? 5.0 : 3.0;
    for (int f = 0; f < F; ++f) {
        const double t = matern ? sqrt(two_nu / chi[f]) : 1.0;
        for (int j = 0; j < D; ++j) {
            const double num = omega_z[(size_t)f * D + j] * t;
            for (int d = 0; d < H; ++d) {
                const double ls = kind == SPX_COVAR_SE ? 1.0 : h->hyp_host[(size_t)d * hs + 3 + j];
                nu[(size_t)d * F * Dp + ts_nu_index(f, j, Dp)] = num / (SPX_TS_TWO_PI * ls);
            }
        }
        ph[f] = phase[f];
    }
    for (int d = 0; d < H; ++d) {
        const double noise = h->hyp_host[(size_t)d * hs + 1], amp2 = h->hyp_host[(size_t)d * hs + 2];
        const double two_amp2 = 2.0 * amp2, jit = 1e-6 * amp2;
        scale[d] = sqrt(two_amp2 / (double)F);
        sig[d] = sqrt(noise + jit);
    }
    if ((rc = h->ts_par.reserve(tp.par_doubles * 8))) return rc;
    if ((rc = h->ts_w.reserve(tp.w_bytes))) return rc;
    if ((rc = h->ts_eps.reserve(tp.eps_bytes))) return rc;
    if ((rc = h->ts_pobs.reserve(tp.obs_bytes))) return rc;
    if ((rc = h->ts_rhs.reserve(tp.obs_bytes))) return rc;
    if ((rc = h->ts_gammaS.reserve(tp.gamma_bytes))) return rc;
    if ((rc = h->ts_pcand.reserve(tp.path_bytes))) return rc;
    if ((rc = h->ts_path.reserve(tp.path_bytes))) return rc;
    const size_t nab = (size_t)H * S * ts_argmin_blocks(M);
    if ((rc = h->ts_am_val.reserve(nab * 8))) return rc;
    if ((rc = h->ts_am_idx.reserve(nab * 8))) return rc;
    if ((rc = h->ts_out_val.reserve((size_t)H * S * 8))) return rc;
    if ((rc = h->ts_out_idx.reserve((size_t)H * S * 8))) return rc;
    h->ts_S = S; h->ts_F = F;
    h->ts_w_stride = per_draw ? (size_t)S * F : 0;
    hipStream_t s = h->stream;
    stage_begin(h);
    if ((rc = stage_h2d(h, h->ts_par.p, par.data(), tp.par_doubles * 8, s))) return rc;
    if ((rc = stage_h2d(h, h->ts_w.p, w, tp.w_bytes, s))) return rc;
    if ((rc = stage_h2d(h, h->ts_eps.p, eps, tp.eps_bytes, s))) return rc;
    h->ev_used = 0;
    const double* dpar = h->ts_par.d();
    const size_t nnu = (size_t)H * F * Dp;
    TIMED(ST_TS_PRIOR, {
        launch_ts_prior(s, h->comp.d(), N, D, Dp, dpar, dpar + nnu, h->ts_w.d(), h->ts_w_stride, dpar + nnu + F, F, S, H, h->ts_pobs.d(), N, 0);
        launch_ts_rhs(s, h->vals.d(), h->ts_pobs.d(), h->ts_eps.d(), per_draw ? (size_t)S * N : 0, dpar + nnu + F + H, N, S, H,
                      h->ts_rhs.d());
    });
    for (int d = 0; d < H; ++d)      // Gamma_d = W_d (rhs_d - mean_d): what spx_set_fantasies does with its fantasy columns
        TIMED(ST_GAMMA_ALPHA, launch_gamma_multi(s, h->WT.d() + (size_t)d * Np * Np, h->ts_rhs.d() + (size_t)d * S * N,
                                                 h->htab.d() + (size_t)d * SPX_HT, h->ts_gammaS.d() + (size_t)d * S * Np, (int)N, Np, S));
    if ((rc = ei_run_impl(h, 0, false, PassRhs{PassRhs::TS, S}))) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->stream2);
        if (h->stream3) (void)hipStreamSynchronize(h->stream3);
        (void)hipGetLastError();
        return rc;
    }
    if ((rc = stage_d2h(h, idx_out, h->ts_out_idx.p, (size_t)H * S * 8, s))) return rc;
    return stage_d2h(h, min_out, h->ts_out_val.p, (size_t)H * S * 8, s);
}

static int ts_getter_checks(spx_handle* h, const char* who, int32_t draw, int32_t sidx)
{
    if (!h) return fail(SPX_ERR_ARG, "%s: null handle", who);
    if (h->multi) return fail(SPX_ERR_ARG, "%s: single-GPU handles only (multi-device handle)", who);
    if (!h->held.results.ts) return fail(SPX_ERR_ARG, "%s: no sample paths are held (call spx_thompson first)", who);
    if (draw < 0 || draw >= h->H) return fail(SPX_ERR_ARG, "%s: draw out of range", who);
    if (sidx < 0 || sidx >= h->ts_S) return fail(SPX_ERR_ARG, "%s: path out of range", who);
    return ensure_init(h);
}

int spx_get_thompson_path(spx_handle* h, int32_t draw, int32_t sidx, double* path)
{
    int rc = ts_getter_checks(h, "spx_get_thompson_path", draw, sidx);
    if (rc) return rc;
    if (!path) return fail(SPX_ERR_ARG, "spx_get_thompson_path: null output");
    const int64_t Mp = round_up(h->M, SPX_BN);
    HIPCHK(hipMemcpy(path, h->ts_path.d() + ((size_t)draw * h->ts_S + sidx) * Mp, (size_t)h->M * 8, hipMemcpyDeviceToHost));
    return SPX_OK;
}

int spx_get_thompson_prior(spx_handle* h, int32_t draw, int32_t sidx, double* prior_cand, double* prior_obs)
{
    int rc = ts_getter_checks(h, "spx_get_thompson_prior", draw, sidx);
    if (rc) return rc;
    const int64_t Mp = round_up(h->M, SPX_BN);
    const size_t p = (size_t)draw * h->ts_S + sidx;
    if (prior_cand) HIPCHK(hipMemcpy(prior_cand, h->ts_pcand.d() + p * Mp, (size_t)h->M * 8, hipMemcpyDeviceToHost));
    if (prior_obs) HIPCHK(hipMemcpy(prior_obs, h->ts_pobs.d() + p * h->N, (size_t)h->N * 8, hipMemcpyDeviceToHost));
    return SPX_OK;
}

// Value and gradient of held sample paths at a batch of points (spx.h).  A reader: every refusal comes from the host's record
// and the caller's arrays; alpha = W^T Gamma of every held path is built once per spx_thompson (launch_trimvT_multi over
// ts_gammaS) and kept with the results.  After that a call is one staged upload, k_ts_grad_prior, k_ts_grad_update, one
// download and ONE synchronisation.
int spx_thompson_grad_batch(spx_handle* h, const double* points, const int32_t* path_of, int32_t P, double* value, double* grad,
                            double* prior)
{
    if (!h) return fail(SPX_ERR_ARG, "spx_thompson_grad_batch: null handle");
    if (h->multi || !h->held.results.ts)
        return fail(SPX_ERR_ARG, "spx_thompson_grad_batch: no sample paths are held (call spx_thompson first)");
    if (!points || !value || !grad) return fail(SPX_ERR_ARG, "spx_thompson_grad_batch: points, value and grad must not be NULL");
    if (P < 1 || P > SPX_TS_GRAD_MAX_POINTS)
        return fail(SPX_ERR_ARG, "spx_thompson_grad_batch: P=%d points (allowed: 1 .. %d)", (int)P, SPX_TS_GRAD_MAX_POINTS);
    const int H = h->H, D = h->D, Dp = h->Dp, Np = h->Np, S = h->ts_S, F = h->ts_F;
    if (path_of)
        for (int p = 0; p < P; ++p)
            if (path_of[p] < 0 || path_of[p] >= H * S)
                return fail(SPX_ERR_ARG, "spx_thompson_grad_batch: path_of[%d] = %d (allowed: 0 .. H S - 1 = %d)", p, (int)path_of[p],
                            H * S - 1);
    int rc = ensure_init(h);
    if (rc) return rc;
    hipStream_t s = h->stream;
    const size_t x_bytes = (size_t)P * D * 8, in_bytes = x_bytes + (path_of ? (size_t)P * 4 : 0);
    const size_t out_doubles = (size_t)P * (2 + D);
    if ((rc = h->ts_gin.reserve(in_bytes))) return rc;
    if ((rc = h->ts_gwork.reserve(((size_t)P * (1 + D) + (size_t)P * Np) * 8))) return rc;
    if ((rc = h->ts_gout.reserve(out_doubles * 8))) return rc;
    // inputs and outputs share the pinned staging buffer, the outputs behind the inputs: nothing waits for the upload alone
    const size_t stage_in = ((x_bytes + 255) & ~(size_t)255) + (((size_t)P * 4 + 255) & ~(size_t)255);
    const bool one_stage = h->opt.stage_copies != 0 && stage_in + out_doubles * 8 <= SPX_STAGE_MAX;
    if (one_stage && (rc = h->pin_stage.reserve(std::max<size_t>(stage_in + out_doubles * 8, 1u << 20)))) return rc;
    const bool build_alpha = !h->held.results.ts_alpha;
    if (build_alpha) {
        if ((rc = h->ts_alpha.reserve((size_t)H * S * Np * 8))) return rc;
        launch_trimvT_multi(s, h->WT.d(), h->ts_gammaS.d(), h->ts_alpha.d(), Np, H, S);
    }
    stage_begin(h);
    double* dx = h->ts_gin.d();
    const int32_t* dpath = path_of ? (const int32_t*)((const char*)h->ts_gin.p + x_bytes) : nullptr;
    if ((rc = stage_h2d(h, dx, points, x_bytes, s))) return rc;
    if (path_of && (rc = stage_h2d(h, (void*)dpath, path_of, (size_t)P * 4, s))) return rc;
    const double* par = h->ts_par.d();
    const size_t nnu = (size_t)H * F * Dp;
    double* d_prior = h->ts_gwork.d();
    double* d_gp = d_prior + P;
    double* d_dk = d_gp + (size_t)P * D;
    launch_ts_grad_prior(s, dx, dpath, P, D, Dp, par, par + nnu, h->ts_w.d(), h->ts_w_stride, par + nnu + F, F, S, H, d_prior, d_gp);
    launch_ts_grad_update(s, h->Xs.d(), h->s1.d(), h->hyp.d(), h->htab.d(), h->ts_alpha.d(), dx, dpath, d_prior, d_gp, d_dk,
                          h->ts_gout.d(), (int)h->N, Np, D, Dp, S, P, dev_kind(h));
    std::vector<double> pageable;
    const double* out;
    if (one_stage) {
        double* st = (double*)((char*)h->pin_stage.p + stage_in);
        HIPCHK(hipMemcpyAsync(st, h->ts_gout.p, out_doubles * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        out = st;
    } else {
        pageable.resize(out_doubles);
        if ((rc = stage_d2h(h, pageable.data(), h->ts_gout.p, out_doubles * 8, s))) return rc;
        out = pageable.data();
    }
    LAUNCHCHK();
    if (build_alpha) h->held.results.ts_alpha = true;      // (a flag of the held results: whatever drops them drops it)
    for (int p = 0; p < P; ++p) {
        const double* o = out + (size_t)p * (2 + D);
        value[p] = o[0];
        if (prior) prior[p] = o[1];
        memcpy(grad + (size_t)p * D, o + 2, (size_t)D * 8);
    }
    return SPX_OK;
}

int spx_get_stat(spx_handle* h, const char* name, int64_t* value)
{
    if (!h || !name || !value) return fail(SPX_ERR_ARG, "spx_get_stat: null");
    if (h->multi) {
        if (!strcmp(name, "ranks_seen") || !strcmp(name, "flow_fallbacks") || !strcmp(name, "flow_rearms") || !strcmp(name, "obs_dims")
            || !strcmp(name, "last_fantasies_device") || !strcmp(name, "fantasies_pending_rows") || !strcmp(name, "fantasies_count"))
            return spx_multi_stat(h->multi, name, value);
        return fail(SPX_ERR_ARG, "spx_get_stat: ask the per-device handles (single-GPU handles only)");
    }
    if (!strcmp(name, "flow_fallbacks")) *value = h->flow_fallbacks;          // hand-off time-outs of k_lean_flow so far
    else if (!strcmp(name, "flow_enabled")) *value = (h->opt.lean_flow != 0 && !h->flow_demoted);   // 0 while a time-out keeps the handle on one launch per block column
    else if (!strcmp(name, "flow_rearms")) *value = h->flow_rearms;           // times the handle went back to k_lean_flow after a fallback
    else if (!strcmp(name, "ranks_seen")) *value = h->comm ? h->ranks_seen : 1;   // size of the communicator the last exchange ran on (its table has one record per rank)
    else if (!strcmp(name, "n_cu")) *value = h->n_cu;
    else if (!strcmp(name, "obs_dims")) *value = h->held.has(Held::OBS) ? h->D : 0;   // D of the resident observations (0: none)
    else if (!strcmp(name, "last_step_fused")) *value = h->ei_plan.fused ? 1 : 0; // the last EI pass ran k_ei_fused128
    else if (!strcmp(name, "last_factor_flow")) *value = h->last_factor->flow ? 1 : 0;             // the last factorisation ran k_lean_flow
    else if (!strcmp(name, "last_factor_cov_in_flow")) *value = h->last_factor->cov_in_flow ? 1 : 0;   // ... which built K(X,X) tile by tile itself
    else if (!strcmp(name, "last_logprob_one_launch")) *value = h->last_factor->fused ? 1 : 0;      // the last do_factor was the one-launch log-likelihood
    else if (!strcmp(name, "last_step_skipped_padding")) *value = h->ei_plan.gemm_nlive > 0 ? 1 : 0;   // ... skipped the padding of N (k_predict_gemm_tail)
    else if (!strcmp(name, "last_corun_launches")) *value = h->corun_launches;   // K(X*,X) launches of the last EI pass in the co-resident form (k_cov_corun)
    else if (!strcmp(name, "last_fantasies_device")) *value = (h->S > 0 && h->fant_device) ? 1 : 0;   // the resident fantasies came from spx_draw_fantasies
    else if (!strcmp(name, "fantasies_pending_rows")) *value = (h->S > 0 && h->fant_device) ? h->fant_P : 0;   // ... P and
    else if (!strcmp(name, "fantasies_count")) *value = (h->S > 0 && h->fant_device) ? h->S : 0;               // ... S of them
    else if (!strcmp(name, "last_kstar_ring")) *value = h->ei_plan.R;   // slots of the K(X*,X) ring the last EI pass ran with (0: not a streams = 3 pass)
    else if (!strcmp(name, "last_effects_passes")) *value = h->effects_plan.npass;   // grid passes the last spx_main_effects ran its rows in
    else if (!strcmp(name, "last_effects_rows")) *value = h->effects_plan.rows;      // ... and how many rows that were
    else if (!strcmp(name, "last_mes_samples")) *value = h->held.results.mes ? h->mes_K : 0;   // K and
    else if (!strcmp(name, "last_mes_grid")) *value = h->held.results.mes ? h->mes_J : 0;      // ... J of the held MES results (0: none)
    else if (!strcmp(name, "last_ts_paths")) *value = h->held.results.ts ? h->ts_S : 0;        // S and
    else if (!strcmp(name, "last_ts_features")) *value = h->held.results.ts ? h->ts_F : 0;     // ... F of the held sample paths (0: none)
    else if (!strcmp(name, "kg_points")) *value = h->held.has(Held::KGPTS) ? h->kg_A : 0;       // A of the held representer points (0: none)
    else if (!strcmp(name, "last_kg_points")) *value = h->held.results.kg ? h->kg_last_A : 0;  // ... and of the held KG results
    else if (!strcmp(name, "last_kg_lines")) *value = h->held.results.kg_lines ? 1 : 0;        // ... whose covariances are kept
    else if (!strcmp(name, "gemm_lds_bytes")) *value = (int64_t)predict_gemm_lds_bytes();   // dynamic LDS of a predict-GEMM workgroup (two are resident per CU)
    else if (!strcmp(name, "hip_runtime_version") || !strcmp(name, "hip_driver_version")) {
        // what the process runs on: a measurement names it (bench.py's line), two boxes of one pool differed in round 5
        int v = 0;
        HIPCHK(name[4] == 'r' ? hipRuntimeGetVersion(&v) : hipDriverGetVersion(&v));
        *value = v;
    } else if (!strcmp(name, "clock_khz") || !strcmp(name, "mem_clock_khz") || !strcmp(name, "wall_clock_khz")
               || !strcmp(name, "l2_bytes") || !strcmp(name, "mem_bus_bits")) {
        int rc = ensure_init(h);
        if (rc) return rc;
        int v = 0;
        const hipDeviceAttribute_t a = !strcmp(name, "clock_khz") ? hipDeviceAttributeClockRate
            : !strcmp(name, "mem_clock_khz") ? hipDeviceAttributeMemoryClockRate
            : !strcmp(name, "wall_clock_khz") ? hipDeviceAttributeWallClockRate
            : !strcmp(name, "l2_bytes") ? hipDeviceAttributeL2CacheSize : hipDeviceAttributeMemoryBusWidth;
        HIPCHK(hipDeviceGetAttribute(&v, a, h->device));
        *value = v;
    }
    else return fail(SPX_ERR_ARG, "spx_get_stat: unknown statistic '%s'", name);
    return SPX_OK;
}

int spx_get_timings(spx_handle* h, double* ms, int64_t* launches, int n)
{
    if (!h) return fail(SPX_ERR_ARG, "null handle");
    if (h->multi) return spx_multi_get_timings(h->multi, ms, launches, n);
    for (int i = 0; i < n && i < ST_COUNT; ++i) {
        if (ms) ms[i] = h->st_ms[i];
        if (launches) launches[i] = h->st_n[i];
    }
    return ST_COUNT;
}

const char* spx_timing_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

}  // extern "C"