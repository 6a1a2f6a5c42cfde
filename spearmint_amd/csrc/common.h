// Shared device/host definitions for libspx (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

// v_mfma_f64_16x16x4_f64: D(16x16) = A(16x4) * B(4x16) + C.
//   A: lane l supplies A[i = l & 15][k = l >> 4]
//   B: lane l supplies B[k = l >> 4][n = l & 15]
//   C/D: reg r of lane l is element [row = (l >> 4) + 4 r][col = l & 15]
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#include "spx_geom.h"   // SPX_NB, SPX_BM, SPX_BN, SPX_BK, SPX_PADN, SPX_HT, round_up, padded_dim

// correlation function of the GP (gp.py:87-132; spx.h SPX_COVAR_*).  SE is ARDSE with unit length scales
// (gp.py:88): the API layer substitutes the length scales, the kernels see ARDSE.
#define SPX_COV_MATERN52 0
#define SPX_COV_MATERN32 1
#define SPX_COV_ARDSE 2

// acquisition function (spx.h SPX_ACQ_*, the same numbers: spx_api.hip asserts it): a template parameter of every kernel
// that ends in an acquisition value (ei_device.h: acq_dev; refine_kernels.hip: acq_terms)
#define SPX_ACQ_DEV_EI 0
#define SPX_ACQ_DEV_PI 1
#define SPX_ACQ_DEV_LCB 2
#define SPX_ACQ_DEV_EHVI 4  // expected hypervolume improvement over two GPs: likewise a stage behind the pass (ehvi_kernels.hip)
#define SPX_ACQ_DEV_KG 5    // knowledge gradient: a stage behind the pass's S > 0 branch over the representer points' columns (kg_kernels.hip)
#define SPX_ACQ_DEV_MES 3   // max-value entropy search: a second stage behind the pass (mes_kernels.hip), never a template argument of the pass's own kernels

// The launchers below return nothing: a kernel that needs more dynamic LDS than the default asks for it right before its
// launch, and a refusal is NOTED (per host thread, spx_api.hip) and reported by the API's next launch check (LAUNCHCHK) as
// SPX_ERR_HIP naming the kernel -- not left to surface as an opaque launch failure.
void spx_note_attr_error(const char* kernel, size_t lds_bytes, hipError_t e);
#define SPX_LDS_ATTR(fn, bytes)                                                                                            \
    do {                                                                                                                   \
        hipError_t ae_ = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                             (int)(bytes));                                                                \
        if (ae_ != hipSuccess) spx_note_attr_error(#fn, (size_t)(bytes), ae_);                                             \
    } while (0)

// ---- launchers (defined in the *.hip translation units) ---------------------
// cov_kernels.hip
void launch_scale_rows(hipStream_t s, const double* x, int64_t n, int64_t n_pad, int D, int Dp,
                       const double* ls /*[nh][ls_stride]*/, int ls_stride, int nh, double factor,
                       double* xs /*[nh][n_pad][Dp]*/, double* sumsq /*[nh][n_pad]*/,
                       double* xs2 = nullptr /*optional: 2 * xs, same launch*/,
                       int* zero_ints = nullptr /*optional: n_zero ints cleared by the same launch*/, int n_zero = 0);
// the log-likelihood path's prologue in ONE launch: launch_scale_rows (factor 1, with the doubled copy) + launch_lean_rhs_init
void launch_lean_prologue(hipStream_t s, const double* x, int64_t n, int64_t n_pad, int D, int Dp, const double* ls,
                          int ls_stride, int nh, double* xs, double* sumsq, double* xs2, const double* vals,
                          const double* htab, double* rhs, int* info, int* flags, int64_t vals_stride = 0);
void launch_cov_self(hipStream_t s, const double* Xs, const double* s1, const double* X2s,
                     const double* htab, double* K, int N, int Np, int Dp, int nh, bool tiled = false,
                     int kind = SPX_COV_MATERN52);
void launch_cov_cross(hipStream_t s, const double* Xs, const double* s1, const double* Cs,
                      const double* s2, const double* htab, double* Kst, int N, int Np, int Mc,
                      int Dp, int nh, int kind = SPX_COV_MATERN52, int live_rows = 0 /*> 0: rows from here on are NOT written*/,
                      bool allow_flat = true /*false: always the 3-D grid (option cov_flat)*/,
                      bool corun = false /*true: the form that fits beside two predict-GEMM workgroups (k_cov_corun)*/);
void launch_cross_mean(hipStream_t s, const double* Xs, const double* s1, const double* Cs,
                       const double* s2, const double* htab, const double* alpha, double* out,
                       int N, int Np, int Mc, int Dp, int nh, int kind = SPX_COV_MATERN52);
void launch_constraint_prob(hipStream_t s, const double* Xs, const double* s1, const double* Cs,
                            const double* s2, const double* htab, const double* alpha, double* out,
                            int N, int Np, int Mc, int Dp, int nh, int kind);
void launch_constraint_const(hipStream_t s, const double* htab, double* out, int Mc, int nh);

// chol_kernels.hip
void launch_chol_diag(hipStream_t s, double* L, double* Dinv, int* info, int Np, int k, int nh, int updated = 0);
void launch_chol_panel(hipStream_t s, double* L, const double* Dinv, int Np, int k, int nh, double* rhs = nullptr);
// log-likelihood path, tile-major storage (chol_kernels.hip)
void launch_lean_step(hipStream_t s, double* Lt, double* Dinv, int* info, double* rhs, double* diagL, int Np, int k,
                      int nh, int lazy);
void launch_lean_trsm(hipStream_t s, double* Lt, const double* Dinv, double* rhs, int Np, int k, int nh);
void launch_lean_step_ps(hipStream_t s, double* Lt, double* Dinv, int* info, double* rhs, double* diagL, int* flags,
                         int Np, int k, int nh);
// (k_lean_flow's `fused` form -- the log-likelihood call as one launch: where the raw inputs and the pinned outputs are)
struct FlowFused {
    const double* comp; const double* hyp; const double* vals; int D, hs;
    double* lp_out; int* info_out;
    int64_t vals_stride;   // 0: vals shared by every draw; N: a right-hand side per draw (spx_gp_logprob_rhs)
};
void launch_lean_flow(hipStream_t s, double* Lt, double* Dinv, int* info, double* rhs, double* diagL, int* lflags,
                      int* dflags, unsigned* tickets, int Np, int nh, int gen, bool alone,
                      const double* Xs, const double* X2s, const double* s1, const double* htab, int N, int Dp, int kind,
                      int* cu_busy, int spin_limit = 0, const FlowFused* fused = nullptr);
void launch_lean_rhs_init(hipStream_t s, const double* vals, const double* htab, double* rhs, int N, int Np, int nh,
                          int* info, int* flags, int64_t vals_stride = 0);
void launch_lean_logprob(hipStream_t s, const double* diagL, const double* rhs, const int* info, double* out, int* info_out,
                         int N, int Np, int nh);
void launch_trinv(hipStream_t s, const double* L, const double* Dinv, double* WT, int Np, int nh, bool tiled = false);
void launch_gamma(hipStream_t s, const double* WT, const double* vals, const double* htab,
                  double* gamma, int N, int Np, int nh);
void launch_gamma_multi(hipStream_t s, const double* WT_h, const double* rhs, const double* htab_h,
                        double* gamma, int N, int Np, int S);
void launch_gamma_cols(hipStream_t s, const double* WT_h, const double* rhs, size_t rhs_stride, double* gamma, int N, int Np,
                       int S);
void launch_gemv_lower(hipStream_t s, const double* WT, const double* rhs, double* out, int Np, int nh);
void launch_alpha(hipStream_t s, const double* WT, const double* gamma, double* alpha, int Np, int nh);
void launch_rhs_init(hipStream_t s, const double* vals, const double* htab, double* rhs, int N, int Np, int nh,
                     int64_t vals_stride = 0);
void launch_logprob(hipStream_t s, const double* L, const double* gamma, size_t gstride, const int* info,
                    double* out, int Np, int nh);

// refine_kernels.hip
#define SPX_REFINE_PB 8   // points (right-hand sides) that share one pass over W in the refinement kernels
void launch_point_cov(hipStream_t s, const double* Xs, const double* s1, const double* hyp,
                      const double* htab, const double* x, double* kvec, double* dkdr2, int N, int Np,
                      int D, int Dp, int nh, int P, int kind = SPX_COV_MATERN52);
void launch_trimv_multi(hipStream_t s, const double* WT, const double* rhs, double* out, int Np, int nh, int P);
void launch_trimvT_multi(hipStream_t s, const double* WT, const double* rhs, double* out, int Np, int nh, int P);
// The finish of the refinement objective (k_point_finish): EI and its gradient per (draw, point) from up to three sets of
// rows, each with its own count and padding.
struct FinishSide {
    const double* Xs;    // [nh][Np][Dp] rows scaled by this side's length scales
    const double* hyp;   // [nh][3 + D]  this side's hyper rows (length scales at +3)
    const double* dk;    // [nh][P][Np]  dk/dr2 at the points (launch_point_cov)
    const double* w;     // weights of the gradient sum: alpha [nh][Np] (mean and third side), z = W^T t [nh][P][Np] (variance)
    int n, Np;
};
struct FinishArgs {
    FinishSide m;          // mean side: func_m = k . alpha + mean
    FinishSide v;          // variance side: func_v = amp2 (1 + 1e-6) - |t|^2 with the mean side's length scales and amplitude;
                           // the mean side's rows again (v.Xs == m.Xs) unless the constrained objective's variance runs over X_c
    FinishSide c;          // third side, n = 0: none.  Plain: the time model (EI per second).  Constrained: the constraint model
    const double* htab;    // [nh][SPX_HT] the mean side's table rows
    const double* k;       // [nh][P][m.Np] k at the points, mean side
    const double* t;       // [nh][P][v.Np] t = W k, variance side
    const double* k3;      // [nh][P][c.Np] k at the points, third side
    const double* tab3;    // [nh][SPX_HT] third side: the time model's table rows / [gain, noise_c, amp2_c, amp2_c]
    const double* x;       // [P][D]
    double best;           // (with fantasies the plain objective reads bests[h][s] instead)
    double* out;           // [nh][P][1 + D]
    int D, Dp, nh, P;
    int S;                 // fantasies per draw (0: none); then mean side == variance side
    const double* gammaS;  // [nh][S][Np]
    const double* alphaS;  // [nh][S][Np]
    const double* bests;   // [nh][S], plain objective only
    double* uvec;          // [nh][P][Np] work vector
    int acq;               // SPX_ACQ_* (plain objective only; 0 = EI) and its parameter: xi / kappa / K (MES)
    double par;
    const double* ystar;   // [nh][K] MES only: the resident y* table of the last MES pass (it travels in the kernel's `bests` slot: S = 0 then)
};
// constrained = false: EI, averaged over the fantasies; true: EI x P(feasible), summed over them (refine_kernels.hip)
void launch_point_finish(hipStream_t s, const FinishArgs& a, bool constrained);

// fused_kernels.hip: the whole EI pass of a chunk for N <= 128 in one launch (no K* / beta in memory)
void launch_ei_fused128(hipStream_t s, int kind, const double* WT, const double* gamma, const double* Xs, const double* s1,
                        const double* Cs, const double* s2, const double* htab, const double* time_m, const double* cprob, double best,
                        double* ei_draw, double* mom_m, double* mom_v, int N, int Mc, int Dp, int nh, int64_t c0,
                        int64_t M, int64_t Mp, int n_cu, int acq = 0 /*SPX_ACQ_*: ei_device.h*/, double par = 0.0);

// fantasy_kernels.hip: the pending posterior and the fantasies of spx_draw_fantasies
size_t fant_post_stride(int P);   // doubles per draw of `post`: C [P][P] | T = L_S^-1 C [P][P] | pend_m [P] | np.min(vals[:N])
void launch_fant_posterior(hipStream_t s, const double* Lm, bool tiled, const double* gamma, const double* htab,
                           const double* vals, double* post, int* info, int N, int P, int Np, int H);
void launch_fant_fill(hipStream_t s, const double* post, const double* z, size_t z_stride, const double* gamma,
                      double* gammaS, double* bests, double* pend_fant, int N, int P, int Np, int S, int H);

// sobol_kernels.hip
void launch_sobol_grid(hipStream_t s, const uint32_t* dirs, int dim, int64_t n, int64_t skip, double* out);

// effects_kernels.hip: the structured rows of spx_main_effects for rows [r0, r0 + m), and the reduction of the kept means
// ([H] rows of `mstride` doubles) into curves [H][D T] and base_mean [H][Q] (spx_plan.h: plan_effects)
struct EffectsPlan;
void launch_effects_rows(hipStream_t s, const double* base, const double* levels, int D, int T, int Q, int64_t r0, int64_t m,
                         double* out);
void launch_effects_mean(hipStream_t s, const EffectsPlan& p, const double* mean, int64_t mstride, int Q, int H, double* curves,
                         double* base_mean);

// loo_kernels.hip: c = diag(K^-1) = the squared row norms of WT, 1 / c and y - alpha / c for rows j < N of nh draws of one model
// (WT, alpha: that model's first draw; outputs [nh][N])
void launch_loo_diag(hipStream_t s, const double* WT, const double* alpha, const double* y, int N, int Np, int nh,
                     double* loo_mean, double* loo_var, double* kinv_diag);

// mes_kernels.hip: max-value entropy search behind a pass that kept its moments ([H][Mp]) -- bounds, log-survival sums for J probe
// values, quartiles + Gumbel fit + the y* table [H][K], and the values into ei_draw.  bpart: [H][mes_bound_blocks(M)][3],
// part: [H][mes_sum_blocks(M)][J], G: [H][J], fit: [H][8]; hyp: a row per draw with the noise at +1, hs doubles apart (htab)
int mes_sum_blocks(int64_t M);
int mes_bound_blocks(int64_t M);
void launch_mes(hipStream_t s, const double* mom_m, const double* mom_v, const double* hyp, int hs, double best, int64_t M,
                int64_t Mp, int H, int J, int K, double* bpart, double* part, double* G, double* ystar, double* fit,
                double* ei_draw);

// ehvi_kernels.hip: expected hypervolume improvement of every (draw, candidate) from the kept moments of the two GPs ([H][Mp]
// each) against the front in k_ehvi's form (edges: a_1 .. a_n, r1; levels: r2, b_1 .. b_n; nstrips = n + 1), into ei_draw
void launch_ehvi(hipStream_t s, const double* m1, const double* v1, const double* m2, const double* v2, const double* edges,
                 const double* levels, int nstrips, int64_t M, int64_t Mp, int H, double* ei_draw);

// ts_kernels.hip: Thompson sampling by pathwise conditioning (spx.h: spx_thompson).  The prior p_{d,s} of rows x [n][D] under
// nu [H][F Dp] in operand order (ts_nu_index within a draw), phase [F], w [H or 1][S][F] (w_stride doubles between draws, 0: shared) and scale [H], into
// out[(d S + s) ldo + col0 + row];  the right-hand sides rhs [H][S][N] = (vals - prior) - sig eps;  the finish of a work item of
// the S > 0 GEMM branch, path = (bg + mean) + prior, both [H][S][Mp];  numpy's argmin of every path, index_base added
void launch_ts_prior(hipStream_t s, const double* x, int64_t n, int D, int Dp, const double* nu, const double* phase,
                     const double* w, size_t w_stride, const double* scale, int F, int S, int H, double* out, int64_t ldo,
                     int64_t col0);
void launch_ts_rhs(hipStream_t s, const double* vals, const double* prior, const double* eps, size_t eps_stride,
                   const double* sig, int64_t N, int S, int H, double* rhs);
void launch_ts_finish(hipStream_t s, const double* part_bgS, const double* htab, const double* prior, int nrb, int Mc, int nh,
                      int S, int64_t c0, int64_t M, int64_t Mp, int h0, double* path);
size_t ts_nu_index(int f, int j, int Dp);
int ts_argmin_blocks(int64_t M);
void launch_ts_argmin(hipStream_t s, const double* path, int64_t M, int64_t Mp, int npaths, double* blk_val, int64_t* blk_idx,
                      double* out_val, int64_t* out_idx, int64_t index_base);

// ts_grad_kernels.hip: value and gradient of sample paths at points x [P][D], point p under path path_of[p] = draw S + s (null:
// path 0 of draw 0) (spx.h: spx_thompson_grad_batch).  The prior and its gradient into prior [P] and gp [P][D]; then, one
// workgroup per point, the update term against alpha [H S][Np] and the combine into out [P][2 + D] = {value, prior, grad};
// dkw [P][Np]: work vector
void launch_ts_grad_prior(hipStream_t s, const double* x, const int32_t* path_of, int P, int D, int Dp, const double* nu,
                          const double* phase, const double* w, size_t w_stride, const double* scale, int F, int S, int H,
                          double* prior, double* gp);
void launch_ts_grad_update(hipStream_t s, const double* Xs, const double* s1, const double* hyp, const double* htab,
                           const double* alpha, const double* x, const int32_t* path_of, const double* prior, const double* gp,
                           double* dkw, double* out, int N, int Np, int D, int Dp, int S, int P, int kind);

// kg_kernels.hip: the knowledge gradient behind the S > 0 GEMM branch with S = A + 1 columns per draw (spx.h SPX_ACQ_KG).
// mu_a [H][A] from gammaS [H][S][Np] (column 0: gamma);  the lines of a work item -- slopes [nh][S][Mc], mu_c [nh][Mc], and with
// mom_m / cov given func_m, func_v [H][Mp] and C [H][A][Mp] -- from its partial sums and Kac [nh][Ap][Mc] = amp2 k(a, c);  the
// values of the work item into ei_draw (mua: the group's first draw)
void launch_kg_mu(hipStream_t s, const double* gammaS, const double* htab, int Np, int S, int H, double* mua);
void launch_kg_lines(hipStream_t s, const double* part_ss, const double* part_bgS, const double* htab, const double* Kac, int nrb,
                     int Mc, int nh, int S, int Ap, int64_t c0, int64_t M, int64_t Mp, int h0, double* slope, double* muc,
                     double* mom_m, double* mom_v, double* cov);
void launch_kg_value(hipStream_t s, const double* slope, const double* muc, const double* mua, int Mc, int nh, int n, int64_t c0,
                     int64_t M, int64_t Mp, int h0, double* ei_draw);
int kg_tile_candidates(int n);

// predict_kernels.hip
void launch_predict_gemm(hipStream_t s, int variant, const double* WT, const double* Kst, const double* gamma,
                         double* part_ss, double* part_bg, int Np, int Mc, int nh, int part_nh, int part_h0,
                         const double* gammaS = nullptr, int S = 0, double* part_bgS = nullptr, int nlive = 0);
bool predict_gemm_variant_ok(int v);
size_t predict_gemm_lds_bytes();        // dynamic LDS of one predict-GEMM workgroup
void launch_ei_finalize_fant(hipStream_t s, const double* part_ss, const double* part_bgS,
                             const double* htab, const double* bests, const double* time_m, const double* cprob,
                             double* ei_draw, int nrb, int Mc, int nh, int S, int64_t c0, int64_t M,
                             int64_t Mp, int h0, double* ei_s, int acq = 0, double par = 0.0);
void launch_ei_finalize(hipStream_t s, const double* part_ss, const double* part_bg,
                        const double* htab, const double* time_m, const double* cprob, double best, double* ei_draw,
                        double* mom_m, double* mom_v, int nrb, int Mc, int nh, int64_t c0,
                        int64_t M, int64_t Mp, int h0, int acq = 0, double par = 0.0);
void launch_mean_over_draws(hipStream_t s, const double* ei_draw, double* ei_mean, int64_t M,
                            int64_t Mp, int H);
void launch_sum_over_draws(hipStream_t s, const double* ei_draw, double* out, int64_t M, int64_t Mp, int H);
void launch_div_scalar(hipStream_t s, double* v, int64_t n, double denom);
void launch_argmax(hipStream_t s, const double* v, int64_t M, double* blk_val, int64_t* blk_idx,
                   double* out_val, int64_t* out_idx, double* host_mirror = nullptr, const int* info = nullptr, int n_info = 0);
void launch_mean_argmax(hipStream_t s, const double* ei_draw, double* ei_mean, int64_t M, int64_t Mp, int H, double* blk_val,
                        int64_t* blk_idx, double* out_val, int64_t* out_idx, double* host_mirror = nullptr,
                        const int* info = nullptr, int n_info = 0);
int argmax_blocks(int64_t M);
