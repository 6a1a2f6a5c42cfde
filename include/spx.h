/*
 * spx.h -- C ABI of libspx.so, the MI355X (gfx950) GP-EI engine behind the
 * Spearmint chooser plugin API.
 *
 * Boundary.  The reference has no FFI: its choosers
 * call numpy/scipy in-process.  This library replaces exactly the block
 *
 *     for mcmc_iter in range(mcmc_iters): overall_ei[:, i] = compute_ei(...)
 *     best_cand = argmax(mean(overall_ei, axis=1))
 *
 * of  spearmint/spearmint/chooser/GPEIChooser.py:143-153,
 *     GPEIOptChooser.py:331-341 (+ :269-271, :293-294),
 *     GPEIperSecChooser.py:284-302,
 * i.e. per hyper-parameter draw:  gp.Matern52/dist2 (gp.py:34-54,120-127),
 * chooser cov (GPEIChooser.py:117-122), spla.cholesky (:191), cho_solve (:194),
 * solve_triangular (:195), predictive mean/variance (:198-199), EI (:202-206).
 * and, for the local refinement that follows that block, the L-BFGS-B objectives
 * grad_optimize_ei_over_hypers of GPEIOptChooser.py:360-525 / GPEIperSecChooser.py:322-434
 * (spx_ei_grad_batch) and of GPConstrainedEIChooser.py:471-803, EI times the probability of
 * feasibility (spx_constrained_ei_grad_batch), at a batch of points per call.
 * The Python choosers in spearmint_amd/chooser/ bind it with ctypes
 * (see INTEGRATION.md for the stub a maintainer would add to the reference).
 *
 * Conventions: plain C, caller-owned buffers, row-major float64, int64 sizes.
 * No torch types.  Every function returns an int status: 0 = ok, <0 = error
 * (spx_last_error() gives the text; after a SUCCESSFUL call it may hold a text that
 * starts with "warning:" -- see spx_get_stat).  No exceptions or exit() cross the ABI.
 * One handle = one GPU = one HIP stream; calls on a handle are serialized by
 * the caller.  All calls are synchronous unless stated.
 *
 * Hyper-parameter row layout, everywhere: [mean, noise, amp2, ls[0..D)]
 * (the tuple order of GPEIOptChooser.py:628), H rows of (3 + D) doubles.
 */
#ifndef SPX_H
#define SPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spx_handle spx_handle;

/* status codes */
#define SPX_OK            0
#define SPX_ERR_ARG      -1   /* bad argument / call order                     */
#define SPX_ERR_HIP      -2   /* HIP runtime error (no device, OOM, ...)        */
#define SPX_ERR_NOT_PD   -3   /* covariance not positive definite == the
                                 numpy.linalg.LinAlgError spla.cholesky raises
                                 (GPEIChooser.py:191); see spx_not_pd_info()     */

/* flags for spx_ei_run / spx_ei_grid */
#define SPX_FLAG_PER_SEC     1   /* divide EI by exp(predicted log duration)
                                    (GPEIperSecChooser.py:437-491); needs
                                    spx_set_time_model()                         */
#define SPX_FLAG_KEEP_MOMENTS 2  /* keep func_m / func_v per (draw, candidate)
                                    for spx_get_moments() (test / debug)          */
#define SPX_FLAG_TIMING      4   /* bracket every kernel launch with HIP events
                                    on the handle's stream (spx_get_timings)      */
#define SPX_FLAG_TIME_ONLY   8   /* with PER_SEC | KEEP_MOMENTS: only the log-duration GP's predicted durations are
                                    computed (spx_get_time_mean); no EI, no winner.  The per-second chooser's pending
                                    branch needs exactly that from its first pass (GPEIperSecChooser.py:492-548: the two
                                    GPs have different observation sets there)                                      */
#define SPX_FLAG_CONSTRAINED 16  /* multiply every draw's EI by the constraint model's P_d(x) = Phi(gain_d k_c(x,X_c)' alpha_c)
                                    (GPConstrainedEIChooser.py:816-842, :931-940) before the mean over draws; needs
                                    spx_set_constraint_model().  SPX_ERR_ARG with SPX_FLAG_PER_SEC, on a multi-device
                                    handle and with a communicator attached                                          */

/* ---- lifetime ---------------------------------------------------------- */
/* Create an engine on HIP device `device_id` (lazy: the first call that needs
 * the GPU initialises it, so the handle can be created before a fork).       */
int  spx_create(int device_id, spx_handle** out);
/* One handle over n_dev GPUs of this node, for the single-process driver:
 * every call below works on it unchanged.  Candidate rows are sharded contiguously over the
 * devices, observations / hyper draws are replicated, each device is driven by its own host
 * thread, and spx_ei_run ends with the path's single collective -- one ncclAllGather (RCCL over
 * xGMI, communicator from ncclCommInitAll) of a 16-byte {best mean EI, global index} record per
 * device, followed by the same numpy-argmax reduction on every device.  Results are bit-identical
 * to a one-GPU handle (np.argmax(np.mean(overall_ei, axis=1)), GPEIChooser.py:153).
 * spx_gp_logprob shards its draws and spx_ei_grad_batch its points over the devices.
 * Repeated device ids (several engines on one GPU: test configuration) cannot form an RCCL
 * communicator; the records then go through host memory (SPX_TRANSPORT_HOST).  librccl is
 * loaded when this is first called, not when libspx is.                                        */
int  spx_create_multi(const int* device_ids, int32_t n_dev, spx_handle** out);
/* The same with the transport of the records chosen by the caller instead of by the device list: SPX_TRANSPORT_NONE =
 * as spx_create_multi decides (RCCL for distinct devices, host memory for repeated ids); SPX_TRANSPORT_HOST = host memory
 * even between distinct GPUs; SPX_TRANSPORT_RCCL = the RCCL code path even for repeated ids (a real librccl refuses such
 * a communicator -- for a stand-in library named by SPX_RCCL_LIB, tests/test_gpu_d2_fake_rccl.py).
 * Environment read by the library (deployment hooks, nothing else): SPX_RCCL_LIB = the librccl to dlopen;
 * SPX_RCCL_ANY_VERSION=1 waives the ncclGetVersion range check of the hand-declared binding.                        */
int  spx_create_multi_transport(const int* device_ids, int32_t n_dev, int32_t transport, spx_handle** out);
#define SPX_TRANSPORT_NONE 0   /* single-GPU handle: no collective                */
#define SPX_TRANSPORT_RCCL 1   /* ncclAllGather over the devices' streams          */
#define SPX_TRANSPORT_HOST 2   /* records staged through host memory               */
/* n_dev, transport and (up to cap) device ids of a handle; any pointer may be NULL */
int  spx_multi_query(spx_handle* h, int32_t* n_dev, int32_t* transport, int32_t* device_ids, int32_t cap);
/* One process per GPU (a launcher-based run, bench.py --gpus N): attach an RCCL communicator to a
 * single-GPU handle.  Rank 0 obtains an id (ncclGetUniqueId), the launcher's own channel carries its
 * SPX_COMM_ID_BYTES bytes to the other ranks, every rank attaches (ncclCommInitRank).  From then on
 * spx_ei_run ends with the path's collective -- one ncclAllGather of the ranks' 16-byte {best mean EI,
 * global index} records on the handle's stream and the same numpy-argmax reduction on every rank -- and
 * spx_get_best returns the global winner.  Candidates are sharded by the caller (spx_set_candidates'
 * index_base).                                                                                     */
#define SPX_COMM_ID_BYTES 128
int  spx_comm_unique_id(char* id_out /* SPX_COMM_ID_BYTES */);
/* librccl is bound at run time (dlopen; SPX_RCCL_LIB overrides the name) through hand-declared types, so the loaded
 * library's ncclGetVersion is checked before anything else of it is called: NCCL API 2.10 <= version < 3.0 (tested
 * with RCCL 2.27.7); anything else, or a library without ncclGetVersion, is refused with SPX_ERR_HIP and a message
 * naming the version (SPX_RCCL_ANY_VERSION=1 waives the range).  Returns the loaded library's version code
 * (22707 = 2.27.7) in *version_code; loads the library if it is not loaded yet.                                */
int  spx_rccl_version(int32_t* version_code);
int  spx_comm_attach(spx_handle* h, const char* id, int32_t nranks, int32_t rank);
/* Optional 2-D partition, "hypers x candidates" (SURVEY.md 8(e)): P = hyper_shards x P_c devices / ranks, device
 * r = rc * hyper_shards + rh evaluates the draws of hyper shard rh for the candidates of shard rc, and the path's
 * single collective becomes ONE ncclAllReduce(SUM) of the zero-padded M-vector of per-candidate EI sums on the
 * handle's stream (8 M bytes; the sums over a device's own draws are formed on the device in numpy's order), after
 * which every device divides by the number of draws and takes numpy's argmax over ALL candidates: no per-draw EI
 * leaves the device, no host-side reduction.  Each device then factors H / hyper_shards covariances instead of H.
 * The sum over draws is "local sums, then the reduction tree", so means agree with the candidates-only scheme to
 * ~1e-16 relative (near-ties may resolve differently): that scheme stays the default.
 *   multi-device handle: spx_set_partition(h, hyper_shards, 0, 0) -- hyper_shards must divide n_dev; the library
 *     shards draws and candidates itself on the following spx_set_hypers / spx_set_candidates (call it first).
 *     spx_set_fantasies and spx_ei_grad_batch are not available with hyper_shards > 1.
 *   one process per GPU (spx_comm_attach): the caller sets ITS draw shard (spx_set_hypers) and candidate shard
 *     (spx_set_candidates with index_base) and passes the totals; M_total > 0 switches the collective of spx_ei_run
 *     from the all-gather of records to the all-reduce of sums (hyper_shards = 1 is allowed: candidates only, but
 *     every rank ends up with the whole mean vector); spx_get_ei_mean then returns the global means of the handle's
 *     own candidates.  M_total = 0 switches back.                                                              */
int  spx_set_partition(spx_handle* h, int32_t hyper_shards, int64_t M_total, int32_t H_total);
void spx_destroy(spx_handle* h);
const char* spx_last_error(void);
int  spx_version(void);
/* number of visible HIP devices, or <0 */
int  spx_device_count(void);

/* ---- resident-data API (what bench.py times: inputs already in HBM) ----- */
/* comp = grid[complete,:] (N x D), vals = values[complete] (N)
 * -- GPEIChooser.py:135-138.                                                  */
int spx_set_observations(spx_handle* h, const double* comp, const double* vals,
                         int64_t N, int32_t D);
/* cand = grid[candidates,:] (M x D) -- GPEIChooser.py:136.  `index_base` is
 * added to local candidate indices in results (a rank that owns candidate
 * rows [base, base+M) of a sharded grid passes base).                         */
int spx_set_candidates(spx_handle* h, const double* cand, int64_t M, int32_t D,
                       int64_t index_base);
/* H hyper-parameter draws, rows [mean, noise, amp2, ls...] */
int spx_set_hypers(spx_handle* h, const double* hypers, int32_t H);
/* second GP on log durations (GPEIperSecChooser.py:176, :437-458):
 * log_durs (N), time_hypers H x (3+D).  Pass NULLs to clear.  Either form
 * drops the factorisation and everything made from it (fantasies, results).
 * log_durs is not checked (the reference cannot get there: scipy's check_finite
 * raises).  A NaN in it propagates by IEEE rules: alpha_t of every draw is NaN
 * throughout, so every predicted duration of every draw and every per-second
 * value is NaN and spx_get_best returns index 0 (numpy's first NaN); func_m /
 * func_v of the objective are what they are without it, and the handle is as
 * good as new after the next spx_set_time_model with finite durations.         */
int spx_set_time_model(spx_handle* h, const double* log_durs,
                       const double* time_hypers);
/* Probit constraint GP (GPConstrainedEIChooser.py:816-842): Nc points comp_c (Nc x D, all completed jobs, Nc independent
 * of the objective's N), their latent values ff (Nc) and H rows c_hypers [gain, noise_c, amp2_c, ls_c...] (H and D as
 * spx_set_hypers set them).  alpha_c = (amp2_c (k(X_c,X_c) + 1e-6 I) + noise_c I)^-1 ff -- no mean term -- is factored
 * by the next spx_factor / spx_ei_step, before the objective draws, on an internal handle of the same device (same
 * factorisation path, SPX_ERR_NOT_PD as for the objective; spx_not_pd_info reports draw 2H + d; 3H + d is the objective's
 * draw d over these Nc points, factored by spx_constrained_ei_grad_batch).  Nc = 0 is the
 * all-valid case (comp_c / ff may be NULL): P_d = Phi(gain_d).  All three pointers NULL clears the model.  Either form
 * drops the results of the last pass and the two factorisations over X_c; the objective's own factor stays.
 * SPX_ERR_ARG on a multi-device handle.                                                                            */
int spx_set_constraint_model(spx_handle* h, const double* comp_c, const double* ff, int64_t Nc,
                             const double* c_hypers);

/* Hot path, stage 1: for every draw build K(X,X)+noise (gp.py:34-54,120-127;
 * GPEIChooser.py:186,190), factor it (:191), and form what the solves need
 * (:194).  Returns SPX_ERR_NOT_PD like spla.cholesky raising LinAlgError.     */
int spx_factor(spx_handle* h);
/* Pending-experiment fantasies (GPEIChooser.py:209-266; "next" row 2 of SURVEY 8(f)).
 * Call after spx_set_observations was given comp_pend = [comp; pend] (n = N + P rows; the
 * vals argument is then only a placeholder) and spx_factor has run:
 *   fant  H x n x S, per draw row-major [i][s]: fant_vals of :245-246 (tile(vals) on top of
 *         pend_fant);   bests H x S: np.min(fant_vals, axis=0) (:249).   1 <= S <= 4096.
 * The next spx_ei_run scores every candidate against every fantasy (:253-263) and averages
 * over S in numpy's summation order (:265).  NULL / S = 0 clears; so does any call that
 * invalidates the factorisation.  SPX_FLAG_PER_SEC with fantasies set is defined: the mean over S
 * of every draw is divided by the predicted duration of a time model over the SAME n resident rows
 * (log_durs of length n); no chooser of the reference forms it.  SPX_FLAG_KEEP_MOMENTS then keeps
 * the predicted durations (spx_get_time_mean) but no func_m / func_v: spx_get_moments refuses. */
int spx_set_fantasies(spx_handle* h, const double* fant, const double* bests, int32_t S);

#define SPX_MAX_PENDING 64
/* Pending-experiment fantasies formed by the library (GPEIChooser.py:219-249).  Call after spx_set_observations was
 * given [comp; pend] (n = N + P rows; vals[N..n) placeholders, not read) and spx_factor / spx_ei_step has run.
 *   P        trailing resident rows that are pending, 1 <= P <= min(SPX_MAX_PENDING, n - 1)
 *   z        standard normals, drawn by the caller where the reference consumes its RNG:
 *            per_draw != 0: H x P x S (draw d uses z[d]);  per_draw == 0: P x S, shared by all draws
 *   S        1 .. 4096.   z == NULL or S == 0 clears, as spx_set_fantasies(NULL) does.
 * Per draw: pend_m = L21 gamma[:N] + mean;  pend_K = L_S L_S^T - noise I (the product rounded, then the subtraction:
 * no contraction);  C = lower Cholesky of pend_K;  pend_fant = C z + pend_m;
 * bests[s] = min(np.min(vals[:N]), min_p pend_fant[p][s]) with np.min's NaN rule.
 * Leaves the handle in the state spx_set_fantasies(fant = [tile(vals[:N]); pend_fant], bests, S) leaves it in; every
 * later call (spx_ei_run with any flag, spx_ei_grad_batch, spx_constrained_ei_grad_batch, what drops or keeps the
 * fantasies) behaves as after that call.  Gamma is written in its factored form: rows < N of every column are gamma[:N],
 * rows N..n are L_S^-1 C z_s, pad rows are zero.  Nothing of the factor travels to the host,
 * and no H x n x S array is formed anywhere.
 * SPX_ERR_NOT_PD when a pivot of some draw's pend_K is not > 0 (spla.cholesky raising at :239); spx_not_pd_info then
 * reports draw 4H + d and the 0-based pivot inside the P x P block; the handle then holds no fantasies.
 * SPX_ERR_ARG: not factored, P or S out of range, the 2-D partition.  (A time model over other rows than these n cannot
 * be resident: spx_set_time_model takes the durations of the resident rows, and new observations drop it.) */
int spx_draw_fantasies(spx_handle* h, int32_t P, const double* z, int32_t per_draw, int32_t S);
/* pend_fant (P x S, row-major) and bests (S) of draw `draw`, as the last spx_draw_fantasies formed them; either may be NULL */
int spx_get_pending_fantasies(spx_handle* h, int32_t draw, double* pend_fant, double* bests);

/* ---- the acquisition function ------------------------------------------------------------------------------------
 * What an EI pass scores candidates with, from the same predictive moments func_m / func_v of every (candidate, draw)
 * (func_s = sqrt(func_v): NaN for func_v < 0, as np.sqrt gives, and then so is every acquisition):
 *   SPX_ACQ_EI   expected improvement, the reference's and the default; par must be 0
 *   SPX_ACQ_PI   probability of improvement  Phi((best - par - func_m) / func_s),  par = xi >= 0
 *   SPX_ACQ_LCB  the negated lower confidence bound  par * func_s - func_m,        par = kappa >= 0
 *                (larger is better, as for EI and PI; kappa = 0: minus the posterior mean -- its argmax is where the
 *                model's mean is lowest)
 * `best` is what EI uses: the minimum of the resident values, or bests[s] per fantasy.  With fantasies the value of
 * every fantasy is averaged over S in numpy's order exactly as EI's is (LCB: par * func_s - func_m_s).  Over the draws:
 * the numpy-order mean, then the argmax with numpy's rule -- everything but the formula is the EI pass.
 * The setting belongs to the handle (a multi-device handle replicates it to every device; with a communicator attached
 * every rank sets it on its own handle).  spx_ei_run, spx_ei_step, spx_ei_grid, spx_ei_grad_batch and spx_ei_grad follow
 * it; spx_get_best, spx_get_ei_mean and spx_get_ei_draws keep their names and return the chosen acquisition's values.
 * spx_ei_grad_batch returns MINUS the acquisition summed over the draws, and the gradient of that in the scaling it has
 * for EI (the reference's factor one half included), so the same L-BFGS-B driver minimises it.
 * spx_set_acquisition takes away the results of the last pass (the result getters refuse until the next one) and nothing
 * else: the factorisation, the fantasies and what the refinement built from them stay.
 * OUT OF SCOPE, refused with SPX_ERR_ARG: an unknown kind; par negative or not finite, or non-zero for SPX_ACQ_EI; any
 * acquisition but SPX_ACQ_EI in a pass with SPX_FLAG_PER_SEC, SPX_FLAG_CONSTRAINED or SPX_FLAG_TIME_ONLY, in
 * spx_ei_grad_batch while a time model is factored, and in spx_constrained_ei_grad_batch.  The handle stays usable. */
#define SPX_ACQ_EI  0
#define SPX_ACQ_PI  1
#define SPX_ACQ_LCB 2
#define SPX_ACQ_MES 3   /* max-value entropy search, below; par = K */
                        /* (4: SPX_ACQ_EHVI, 5: SPX_ACQ_KG, both below) */
int spx_set_acquisition(spx_handle* h, int32_t kind, double par);
int spx_get_acquisition(spx_handle* h, int32_t* kind, double* par);   /* either may be NULL */

/* ---- max-value entropy search (SPX_ACQ_MES) ------------------------------------------------------------------------
 * Wang & Jegelka (2017), restated for a minimisation: the value of a candidate depends on the posterior over the WHOLE candidate
 * set of the pass, through the distribution of the minimum y*, fitted per hyper draw d by a Gumbel distribution to the quartiles
 * of the minimum under the independence approximation.  spx_set_acquisition(h, SPX_ACQ_MES, K): K = number of y* levels, an
 * integer-valued double in 1 .. 1024 (anything else, 0 included, is SPX_ERR_ARG).  With it set, spx_ei_run / spx_ei_step /
 * spx_ei_grid run the ordinary pass as EI with the moments kept (SPX_FLAG_KEEP_MOMENTS is implied; spx_get_moments works
 * afterwards), then, on the device and behind the same single synchronisation, per draw over the M candidates of the pass
 * (mu = func_m, v = func_v, sigma = sqrt(v), no fused multiply-add anywhere; a candidate is VALID when mu is finite and v > 0
 * and finite, invalid ones are left out of 1-3):
 *   1  lo = min_c(mu - 8 sigma),  hi = min_c(mu + 5 sigma)
 *   2  step = (hi - lo) / (J - 1),  y_j = lo + j step,  j < J = option "mes_grid" (default 256, allowed 8 .. 4096)
 *   3  G_j = sum over the valid c of log Phi((mu_c - y_j) / sigma_c): the log-probability that every candidate exceeds y_j.
 *      Partial sums over 512 consecutive candidates, then over the partials in order, both compensated: G of a draw depends on
 *      that draw's moments, M and J alone.  G_0 >= -M 6.3e-16 and G_{J-1} <= log Phi(-5), so the targets of 4 are bracketed
 *   4  for p = 0.25, 0.5, 0.75: t_p = log(1 - p), j = the first index with G_j <= t_p,
 *      y_p = y_{j-1} + (y_j - y_{j-1}) (G_{j-1} - t_p) / (G_{j-1} - G_j);   b = (y_75 - y_25) / (log log 4 - log log(4/3)),
 *      a = y_50 - b log log 2   (the reflected Gumbel P(y* < y) = 1 - exp(-exp((y - a) / b)));   K levels without random
 *      numbers w_k = log(-log1p(-(k + 0.5) / K)),  y*_k = min(a + b w_k, cap),  cap = best - 5 sqrt(noise_d)  (best: what EI uses)
 *   5  MES_d(c) = (sum_k h(gamma_k)) / K,  gamma_k = (mu_c - y*_k) / sigma_c,  h(g) = g phi(g) / (2 Phi(g)) - log Phi(g),
 *      summed sequentially in k, then one division.  h keeps its accuracy in both tails (an asymptotic series below g = -12;
 *      +0.0, never negative, beyond g = 38.6).  func_v < 0: NaN, as for every acquisition.
 * then the numpy-order mean over the draws, the argmax rule and the result getters of every pass.  A draw without a valid
 * candidate has NaN y* and NaN values throughout; no error is returned.
 * The y* table, the fit and G are part of the pass's results: whatever drops those drops them, spx_set_acquisition and
 * spx_set_option("mes_grid") included.  spx_ei_grad_batch / spx_ei_grad under SPX_ACQ_MES evaluate -sum_d MES_d and its gradient
 * against that resident table, held fixed; they refuse (SPX_ERR_ARG) when no MES pass's results are held and do not drop it.
 * (spx_set_option("mes_grid") drops the results of the last pass whenever it is accepted, an unchanged value included, as
 * spx_set_acquisition does; a refused value drops nothing.)  With option "timing" the four kernels are the stage "mes".
 * spx_get_stat "last_mes_samples" / "last_mes_grid": K and J of the held MES results (0: none).
 * REFUSED with SPX_ERR_ARG, before any device is touched, the handle as it was: MES in a pass with SPX_FLAG_PER_SEC,
 * SPX_FLAG_CONSTRAINED or SPX_FLAG_TIME_ONLY; with fantasies held; on a multi-device handle, with a communicator attached or
 * with a 2-D partition (y* needs every shard's moments); in spx_constrained_ei_grad_batch.
 * spx_get_mes: of draw `draw` of the held MES results, ystar (K), fit (8: lo, hi, y25, y50, y75, a, b, cap) and G (J); any
 * pointer may be NULL.                                                                                                    */
int spx_get_mes(spx_handle* h, int32_t draw, double* ystar /* K */, double* fit /* 8 */, double* G /* J */);

/* ---- two objectives: expected hypervolume improvement (SPX_ACQ_EHVI) -----------------------------------------------------
 * Both objectives are minimised.  The first is the handle's own GP; the SECOND objective's GP is the model that
 * spx_set_time_model holds: its `log_durs` argument is "the second objective's values" of the resident rows (the chooser passes
 * log durations; the engine takes any vector) and `time_hypers` its draws.  The two predictions are taken as independent
 * Gaussians per draw d: (m1, v1) = func_m / func_v of the objective, (m2, v2) = func_m / func_v of the second GP -- its FULL
 * predictive moments, the ones a separate plain handle given (comp, second values, second hypers) and the same candidates
 * returns from spx_ei_run(SPX_FLAG_KEEP_MOMENTS) + spx_get_moments(d), bit for bit.
 * The front (spx_set_pareto_front): n mutually non-dominated points with a_1 < ... < a_n (first objective) and
 * b_1 > ... > b_n (second), and a reference point (r1, r2) with a_n < r1 and b_1 < r2.  With a_0 = -inf, a_{n+1} = r1, b_0 = r2
 * a new point (u, v) adds the area  I(u, v) = sum_{i=0..n} (a_{i+1} - max(u, a_i))+ (b_i - v)+,  and because
 * (A - max(u, a))+ = (A - u)+ - (a - u)+ for a <= A its expectation is
 *     EHVI = sum_{i=0..n} [G1(a_{i+1}) - G1(a_i)] G2(b_i),    G_k(y) = E[(y - f_k)+] = EI of (m_k, v_k) with best = y,
 *     G1(a_0) := +0.0
 * evaluated per (draw, candidate) sequentially in i = 0 .. n, every G1(a_i) once, every strip evaluated, nothing contracted
 * into a fused multiply-add; G is the EI formula of every pass itself, so v1 < 0 or v2 < 0 gives NaN.  n = 0: G1(r1) G2(r2).
 * spx_set_acquisition(h, SPX_ACQ_EHVI, 0) (a non-zero parameter is SPX_ERR_ARG).  With it set, spx_ei_run / spx_ei_step /
 * spx_ei_grid / spx_ei_per_sec_grid (which pass the second values on; their SPX_FLAG_PER_SEC is left out under EHVI) run
 *   1  the second GP's factorisation (when what it was made from changed) and its pass over the same candidates, on an internal
 *      handle of the same device with the caller's options, which takes the resident rows and candidates by device-to-device
 *      copies and synchronises on its own, as the constraint model's factorisation does, before anything else is queued;
 *   2  the ordinary pass over the objective as EI with the moments kept (SPX_FLAG_KEEP_MOMENTS is implied);
 *   3  the EHVI kernel over (draw, candidate) into the per-draw values, behind the pass on the same stream (with option
 *      "timing": stage "ehvi");
 *   4  the numpy-order mean over the draws, the argmax rule and the result getters of every pass.
 * Afterwards spx_get_moments(h, d, ...) serves the objective's moments for d < H and the second GP's for draw H + d.
 * Under EHVI spx_factor / spx_ei_step factor the objective's covariance alone (the time model is not factored a second time
 * inside the handle: a factorisation made under EHVI serves no per-second pass, and one made under another acquisition is
 * made again by the next step).  A covariance of the second GP that is not positive definite is SPX_ERR_NOT_PD with
 * spx_not_pd_info reporting draw 5H + d.  Which report comes first when both GPs fail: spx_ei_step runs the second GP before
 * the objective's factorisation, so 5H + d; spx_factor + spx_ei_run (and a step with option "timing") factor the objective
 * first, so d.
 * The front is a setting of the handle, as the acquisition is: it stays until replaced or cleared, and setting or clearing it
 * takes away the results of the last pass and nothing else.
 * REFUSED with SPX_ERR_ARG before any device is touched, the handle as it was: EHVI without a time model or without a front;
 * with SPX_FLAG_PER_SEC (spx_ei_run / spx_ei_step), SPX_FLAG_CONSTRAINED or SPX_FLAG_TIME_ONLY; with fantasies held; on a
 * multi-device handle, with a communicator attached or with a 2-D partition; spx_ei_grad_batch / spx_ei_grad /
 * spx_constrained_ei_grad_batch under EHVI (refinement needs the second GP's variance gradient: out of scope).
 * spx_set_pareto_front: n in 0 .. SPX_MAX_FRONT (a / b may be NULL when n = 0); n < 0 clears the front.  SPX_ERR_ARG, the
 * handle as it was: a non-finite number, a not strictly increasing, b not strictly decreasing, a_n >= r1 or b_1 >= r2, n out
 * of range.  spx_get_pareto_front: *n = -1 when no front is set; a / b receive n doubles each; any pointer may be NULL.   */
#define SPX_ACQ_EHVI 4
#define SPX_MAX_FRONT 4096
int spx_set_pareto_front(spx_handle* h, const double* a, const double* b, int32_t n, double r1, double r2);
int spx_get_pareto_front(spx_handle* h, double* a, double* b, int32_t* n, double* r1, double* r2);

/* ---- the knowledge gradient (SPX_ACQ_KG): the acquisition for noisy objectives ---------------------------------------------
 * Frazier, Powell & Dayanik (2009); Scott, Frazier & Powell (2011), the discrete form: a candidate c is valued by the expected
 * drop of the minimum of the posterior MEAN -- over c itself and A representer points -- after one more noisy evaluation at c.
 * (EI, PI and MES measure against `best`, the minimum OBSERVED value: on a noisy objective the luckiest draw.)
 * Everything is per hyper draw d.  A = number of representer points, 1 .. SPX_KG_MAX_POINTS; a contract:
 *   mu_c      = func_m(c) of the pass;   func_v(c) its variance;   s_c = sqrt(func_v(c) + noise_d), the standard deviation of a
 *               new OBSERVATION at c
 *   Gamma_a   = L^-1 k(X, a), no mean subtracted; k(X, a) from the library's own cross-covariance launch with the points as rows
 *   mu_a      = mean_d + sum_i Gamma_a[i] gamma[i]: the posterior mean at a -- what a kept-moments pass over a as a candidate
 *               returns for func_m, summed here per point (lane i mod 64 takes row i, then a butterfly over the 64 lanes) and
 *               not by the predict GEMM, so the two may differ in their last bits
 *   q(c, a)   = sum_i beta_c[i] Gamma_a[i], summed exactly as the pass sums bg for a fantasy column (the S > 0 GEMM branch with
 *               S = A + 1: column 0 is the ordinary gamma and gives func_m, column a + 1 is Gamma_a)
 *   C(c, a)   = amp2_d k(c, a) - q(c, a): the posterior covariance of c and a; amp2_d k(c, a) from the same launch over the
 *               chunk's candidates (a coincident pair gives what that kernel gives for r2 = 0: amp2_d)
 *   the A + 1 lines in Z ~ N(0, 1):  line 0 = (mu_c, func_v(c) / s_c),  line a = (mu_a, C(c, a) / s_c)
 *   KG_d(c)   = min_i mu_i - E_Z[min_i (mu_i + b_i Z)] = sum_k (b_k - b_{k+1}) f(-|z_k|),   f(z) = phi(z) + z Phi(z),
 *               over the lines ON the lower envelope in order of falling slope, z_k their breakpoints; f(-|z|) is the EI
 *               formula of every pass at unit sigma, func_m = 0 and best = -|z|, clamped at +0.0 from below.
 * The envelope is found without a sort, every line on its own (csrc/kg_device.h states it operation for operation): z_ij =
 * (mu_j - mu_i) / (b_i - b_j) for b_j < b_i, one expression per pair; line i is on the envelope when max over the steeper lines
 * of z_ji < min over the flatter lines of z_ij (strictly) and no line of its slope has a lower intercept -- the TIE RULE: among
 * lines of equal slope the lowest intercept stays, among equal lines the lowest index; the successor of an envelope line is the
 * envelope line of the largest slope below its own.  The terms are added in the order of the lines from +0.0.
 * EXACT cases: all slopes equal (duplicated points included): +0.0;  the value is never negative;  func_v(c) + noise_d not > 0,
 * or a non-finite mu or slope among the lines of (d, c): NaN for that (d, c) alone.
 * The value of (d, c) depends on its own lines and on the order of the points only: not on M, the chunking, the draw groups,
 * options "streams" / "gemm_partial", the position of c or the other draws.
 * spx_set_acquisition(h, SPX_ACQ_KG, 0) (a non-zero parameter is SPX_ERR_ARG).  With it set spx_ei_run / spx_ei_step /
 * spx_ei_grid form k(X, A), Gamma_a and mu_a per draw, run the pass's S > 0 branch over the A + 1 columns, form k(A, c) per work
 * item and run the KG kernels in place of the acquisition (option "timing": stage "kg"), then the numpy-order mean over the
 * draws, the argmax rule and the result getters of every pass behind one synchronisation.  SPX_FLAG_KEEP_MOMENTS keeps func_m /
 * func_v (spx_get_moments) and the covariances C[d][a][c]; refused when H A Mp 8 bytes exceed SPX_KG_MAX_LINE_BYTES.
 * spx_set_kg_points(h, pts, A): pts A x D row-major, D the handle's; a setting of the handle, as the front is: it stays until
 * replaced or cleared (A < 0) or until observations / candidates of another D arrive, and setting it takes away the results of the
 * last pass and nothing else.  spx_get_kg_points: *A = -1 when none are set; pts receives A x D doubles; either may be NULL.
 * spx_get_kg_lines: of draw `draw` of the held KG results, mu_a (A) and cov (A x M row-major; needs SPX_FLAG_KEEP_MOMENTS);
 * either may be NULL.  spx_get_stat "kg_points" / "last_kg_points" / "last_kg_lines": A of the held points, A of the held KG
 * results, and whether their covariances are kept (0: none).
 * REFUSED with SPX_ERR_ARG before any device is touched, the handle as it was: KG without points; with SPX_FLAG_PER_SEC,
 * SPX_FLAG_CONSTRAINED or SPX_FLAG_TIME_ONLY; with fantasies held; on a multi-device handle, with a communicator attached or
 * with a 2-D partition; spx_ei_grad_batch / spx_ei_grad / spx_constrained_ei_grad_batch under KG (refinement needs the gradient
 * of the envelope: out of scope); a non-finite coordinate in the points, A out of range.                                    */
#define SPX_ACQ_KG 5
#define SPX_KG_MAX_POINTS 255
#define SPX_KG_MAX_LINE_BYTES (4ll << 30)
int spx_set_kg_points(spx_handle* h, const double* pts /* A x D */, int32_t A);
int spx_get_kg_points(spx_handle* h, double* pts /* A x D */, int32_t* A);
int spx_get_kg_lines(spx_handle* h, int32_t draw, double* mu_a /* A */, double* cov /* A x M */);

/* ---- Thompson sampling: posterior sample paths over the candidates (pathwise conditioning) ---------------------------------
 * Wilson et al. (2020): a draw from the GP posterior is a draw from the prior plus a data-dependent update,
 *     f_s(x) = mean + p_s(x) + k(x, X)' (K + sig^2 I)^-1 (y - mean - p_s(X) - sig eps_s),      sig^2 = noise + 1e-6 amp2
 * (sig^2 is the diagonal term of the chooser covariance amp2 (k + 1e-6 I) + noise I).  The prior sample p_s comes from F random
 * Fourier features of the covariance's spectral density (Rahimi & Recht 2007); everything behind p_s(x) is a predictive mean
 * with another right-hand side, computed with the exact K(X*,X) and the resident factor by the pass's S > 0 GEMM branch (the
 * one the pending fantasies use) -- the feature approximation touches the prior alone.  The library draws no random numbers:
 * as with spx_draw_fantasies the caller supplies the base randoms.
 * D = dimension of the resident observations, H = resident draws, N = resident rows, M = resident candidates, nu_s = the
 * smoothness 5/2 (Matern52) or 3/2 (Matern32).  The arithmetic, a contract: every operation below is ONE IEEE rounding and
 * nothing is contracted into a fused multiply-add except where fma is written.
 *   frequencies, in TURNS (formed on the host)
 *              t_f = sqrt(2 nu_s / chi_f)  (ARDSE / SE: t_f = 1);   nu[d][f][j] = (omega_z[f][j] * t_f) / (TWO_PI * ls[d][j]),
 *              TWO_PI = 6.283185307179586 (2 * np.pi), ls = 1 for SE; the pad dimensions are zero
 *   feature    u = sum_j nu_j x_j + phase_f: the dot product on v_mfma_f64_16x16x4_f64 (its summation order is the kernel's
 *              own), then ONE addition of the phase;  r = u - rint(u), exact, so no argument reduction of a large angle is ever
 *              needed;  c = cos2pi(r), the polynomial of csrc/ts_device.h (SPX_TS_COS_ULPS = 4 ulp of the result; the text there
 *              is the definition).  A NaN or infinite coordinate gives NaN; |u| >= 2^52 gives r = 0
 *   prior      p_{d,s}(x) = scale_d * (sum_f w[s][f] c_f),   scale_d = sqrt((2 * amp2_d) / F).  The sum runs over f in a fixed
 *              order (16 features at a time, on the MFMA), so a row's value depends on its coordinates, the draw, s, F and the
 *              randoms alone -- not on M, the chunking, the row's position, the other paths of the call or any option
 *   conditioning
 *              rhs[d][s][i] = (y_i - p_{d,s}(x_i)) - sig_d * eps[s][i],   sig_d = sqrt(noise_d + 1e-6 * amp2_d);
 *              Gamma = L^-1 (rhs - mean_d) as spx_set_fantasies forms it from its fantasy columns; the pass over the candidates is
 *              spx_ei_run's over S fantasies: every chunk, draw group, "streams" 1 / 2 / 3 and "gemm_partial"
 *   finish     path = (bg + mean_d) + p_{d,s}(c), bg summed as the pass sums it for a fantasy; the paths are kept, [H S][M];
 *              then per (d, s) numpy's argmin -- the first NaN wins, else the first minimum -- and index_base is added.
 * State: takes the results of the last pass away (spx_get_best and the other result getters refuse afterwards) and holds the
 * paths and their priors as a results kind of their own: whatever drops a pass's results drops them.  The factorisation, the
 * candidates, the options and the acquisition setting stay (the call does not read that setting): an EI pass afterwards gives
 * the bits it gave before.  spx_get_stat "last_ts_paths" / "last_ts_features": S and F of the held paths (0: none).  With option
 * "timing" the stages are "ts_prior" (k_ts_prior over observations and candidates, k_ts_rhs) and "ts_finish" (k_ts_finish,
 * k_ts_argmin).  S > 16: every block of 16 paths forms the features again.
 * REFUSED with SPX_ERR_ARG before any device is touched, the handle as it was: no held factorisation or no candidates; fantasies
 * held; a multi-device handle, a communicator or a 2-D partition; F or S out of range; a NULL pointer where one is read; a chi
 * that is not finite and > 0; a phase outside [0, 1); H S Mp 8 bytes (Mp = M rounded up to 128) above 4 GiB, or H S > 65535.
 *
 * spx_thompson_grad_batch: value and gradient of held paths OFF the grid.  A path is a closed-form function of x,
 *     f_{d,s}(x) = mean_d + p_{d,s}(x) + k_d(x, X)' alpha_{d,s},      alpha_{d,s} = W_d^T Gamma_{d,s} = (K + sig^2 I)^-1 (rhs - mean),
 * and everything it needs is resident after spx_thompson.  Point p is evaluated under path path_of[p] = draw * S + s (NULL: path 0 of
 * draw 0 for every point).  The arithmetic, a contract in the same sense as above:
 *   prior      spx_thompson's own arithmetic -- the dot product on v_mfma_f64_16x16x4_f64 in k_ts_prior's order, ONE addition of the
 *              phase, r = u - rint(u), cos2pi, the contraction with the path's weights 16 features at a time on the MFMA, ONE
 *              multiplication by scale_d -- so at a point whose coordinates equal a resident candidate row (or observation row)
 *              `prior` equals spx_get_thompson_prior's entry BIT FOR BIT
 *   its gradient
 *              gp[j] = -(scale_d * TWO_PI) * sum_f nu[d][f][j] * (w[s][f] * sin2pi(r_f)),  sin2pi the polynomial of csrc/ts_device.h
 *              (SPX_TS_SIN_ULPS = 4 ulp of the result); the sum over f in a fixed order of the kernel's own (on the MFMA)
 *   update     m = sum_j k_j alpha_j with k and dk/dr^2 exactly as spx_ei_grad_batch forms them (the expanded r^2, the clamp at 0,
 *              the three correlation kinds, SE = ARDSE on unit length scales);  gu[j'] = sum_j (dk_j / dx_j') alpha_j, the TRUE
 *              partial derivative: no factor one half (a path is not an acquisition of the reference and inherits no scaling).
 *              alpha is built for all H S held paths by the first call after a spx_thompson and kept with the paths
 *   result     value = (m + mean_d) + prior,  grad[j] = gu[j] + gp[j], one rounding each.  grad is d value / d x: a minimiser of the
 *              path takes (value, grad) as they are.  Every point is computed by its own threads in a fixed order: its numbers do
 *              not depend on P, on its position in the batch, on the other points' paths or on how many paths and draws are
 *              resident.  A NaN or infinite coordinate gives NaN value and gradient for that point alone.
 * State: a reader.  Paths, priors, factorisation, candidates, options and the acquisition setting stay bit for bit (an EI pass
 * afterwards gives the bits it gave before); the cached alpha lives with the paths -- whatever drops a pass's results drops it.
 * After the first call: two kernel launches and one host synchronisation per call, no allocation once the buffers have grown.
 * REFUSED with SPX_ERR_ARG before any device is touched, the handle as it was: no sample paths held (a multi-device handle, a
 * communicator or a 2-D partition cannot hold any); points, value or grad NULL; P < 1 or P > SPX_TS_GRAD_MAX_POINTS (the most a
 * launch grid of spx_ei_grad_batch takes); a path_of entry outside 0 .. H S - 1.                                              */
#define SPX_TS_MAX_FEATURES 8192
#define SPX_TS_MAX_PATHS    256
int spx_thompson(spx_handle* h,
                 int32_t F,               /* features: a multiple of 16 in 16 .. SPX_TS_MAX_FEATURES  */
                 int32_t S,               /* paths per resident draw, 1 .. SPX_TS_MAX_PATHS           */
                 const double* omega_z,   /* F x D standard normals (shared by the draws)             */
                 const double* chi,       /* F chi-square(2 nu) draws: 5 dof Matern52, 3 Matern32;
                                             not read (may be NULL) for ARDSE / SE                    */
                 const double* phase,     /* F uniforms in [0, 1): the phase in TURNS                 */
                 const double* w,         /* per_draw ? H x S x F : S x F standard normals            */
                 const double* eps,       /* per_draw ? H x S x N : S x N standard normals            */
                 int32_t per_draw,
                 int64_t* idx_out,        /* H x S: index_base + argmin_c f_{d,s}(c), numpy's rule    */
                 double*  min_out);       /* H x S: that minimum                                      */
int spx_get_thompson_path (spx_handle* h, int32_t draw, int32_t s, double* path /* M */);
int spx_get_thompson_prior(spx_handle* h, int32_t draw, int32_t s,
                           double* prior_cand /* M */, double* prior_obs /* N */);  /* either may be NULL */
#define SPX_TS_GRAD_MAX_POINTS 65535
int spx_thompson_grad_batch(spx_handle* h, const double* points /* P x D */,
                            const int32_t* path_of /* P: draw * S + s of each point; NULL: path 0 of draw 0 for all */,
                            int32_t P, double* value /* P */, double* grad /* P x D */,
                            double* prior /* P, may be NULL: p_{d,s}(x) alone */);

/* Hot path, stage 2: K(X*,X) (:187), triangular solve (:195), predictive
 * mean/variance (:198-199), EI (:202-206) for every (candidate, draw); then the
 * MCMC mean and the argmax (:153).  Results stay on the device.               */
int spx_ei_run(spx_handle* h, int32_t flags);
/* spx_factor followed by spx_ei_run as ONE call with ONE host synchronisation: the body of a chooser's next() for fixed
 * hyper-parameter draws (GPEIChooser.py:143-153: compute_ei per draw, argmax of the mean) and bench.py's timed step.
 * Same kernels and results as the two calls; a covariance that is not positive definite is reported as spx_factor
 * reports it (SPX_ERR_NOT_PD + spx_not_pd_info) once the step's single synchronisation has passed.  Fantasies set
 * before the call are dropped, as by spx_factor.  What it saves matters at small N (N = 128, 20 000 candidates, 10
 * draws: two synchronisations + three device-to-host copies were ~85 us of a 310 us step).                        */
int spx_ei_step(spx_handle* h, int32_t flags);

/* results of the last spx_ei_run / spx_ei_step */
/* best_idx = index_base + argmax_c mean_h EI[c,h]  with numpy's rule (first NaN
 * wins, else first maximum); best_val = that mean EI.                         */
int spx_get_best(spx_handle* h, int64_t* best_idx, double* best_val);
int spx_get_ei_mean(spx_handle* h, double* out /* M */);
/* overall_ei exactly as the reference lays it out: M x H, row-major           */
int spx_get_ei_draws(spx_handle* h, double* out /* M*H */);

/* ---- parameter sensitivity: main effects of the posterior mean ---------------------------------------------------
 * The functional-ANOVA main effect of every input dimension under every resident hyper draw, from ONE structured grid of
 * (D T + 1) Q rows that is formed, scored and reduced on the device.  D = dimension of the resident observations, H = resident
 * draws; base = Q points of the unit cube (Q x D, row-major), levels = T values substituted into one coordinate at a time.
 *   rows     r = (j T + k) Q + q  is base[q] with coordinate j replaced by levels[k]   (j < D, k < T, q < Q);
 *            the last Q rows, r = D T Q + q, are base[q] itself.
 *   values   func_m_d(r) = the predictive mean of draw d at row r, exactly what spx_get_moments returns after a pass:
 *            curves[d][j][k] = np.mean of the Q values of block (j, k) in numpy's order (its pairwise sum, then ONE true
 *            division by Q);   base_mean[d][q] = func_m_d(D T Q + q)   (H x Q; may be NULL).
 * Bit-for-bit contract: the values equal those of the same rows built on the host, spx_set_candidates,
 * spx_ei_run(SPX_FLAG_KEEP_MOMENTS), spx_get_moments and np.mean(func_m.reshape(H, D, T, Q), axis=-1).  The means go through
 * the pass's own K(X*,X) + predict-GEMM (or fused N <= 128) path; a candidate's moments do not depend on which other candidates
 * share a pass, so the rows may be scored in several passes -- spx_set_option "effects_pass_rows" (rows per pass; 0 = the
 * default, 2^20) bounds what a pass allocates, blocks of Q may straddle a boundary, and every split gives the same bits.
 * Needs (SPX_ERR_ARG otherwise, decided before any device is touched, the handle exactly as it was, the last pass's results
 * included): a held factorisation (spx_factor, spx_ei_step or spx_ei_grid has run); no fantasies held (the resident rows would
 * include pending points, and such a pass keeps no func_m); a single-GPU handle without a communicator and without a 2-D
 * partition; base, levels, curves non-NULL; 1 <= Q <= 524 288 (the depth of the pairwise walk); 1 <= T;
 * (D T + 1) Q <= 2^30 rows.
 * State: the call takes the candidates and the results of the last pass away before its first mutation and leaves them away
 * (spx_get_best, spx_get_ei_mean, spx_get_moments and spx_ei_run refuse until spx_set_candidates / a new pass); the
 * factorisation, the time and constraint models, the options and the acquisition setting stay, and the values do not depend
 * on that setting.  spx_get_stat "last_effects_passes" / "last_effects_rows": passes and rows of the last call.           */
int spx_main_effects(spx_handle* h,
                     const double* base,   /* Q x D, row-major: points of the unit cube        */
                     int32_t Q,
                     const double* levels, /* T values substituted into one coordinate         */
                     int32_t T,
                     double* curves,       /* H x D x T                                         */
                     double* base_mean);   /* H x Q; may be NULL                                */

/* ---- model check: leave-one-out cross-validation of the resident factorisation ------------------------------------------
 * For every observation i and every resident hyper draw, the predictive mean and variance at x_i of the GP trained on all the
 * OTHER observations under that draw's hyper-parameters -- no refit (Rasmussen & Williams, 5.4.2): with K the draw's
 * amp2 (k + 1e-6 I) + noise I, c_i = (K^-1)_ii and alpha = K^-1 (y - mean),
 *     kinv_diag[d][i] = c_i        loo_var[d][i] = 1 / c_i        loo_mean[d][i] = y_i - alpha_i / c_i
 * (loo_var includes the noise: it is the variance of the left-out OBSERVATION).  c_i is the squared norm of row i of the
 * resident L^-T, summed on the device in an order that depends on i and on N rounded up to 128 alone: the values of a draw
 * do not depend on how many other draws are resident, on options, on candidates or on earlier passes.  1 / c and alpha / c are
 * IEEE divisions, the subtraction is one IEEE subtraction.  model = SPX_LOO_OBJECTIVE: y = the observed values;
 * SPX_LOO_TIME: y = log_durs, K and alpha those of the log-duration GP of spx_set_time_model.
 * NaN or inf in y propagates by IEEE rules (alpha is NaN throughout, so loo_mean is; loo_var and kinv_diag do not depend on y);
 * nothing is clamped and no error is returned.  N = 1: loo_mean = the draw's prior mean (up to the rounding of
 * alpha_0 = K_00^-1 (y_0 - mean)), loo_var = K_00.
 * Needs (SPX_ERR_ARG otherwise, decided before any device is touched, the handle exactly as it was): a held factorisation
 * (spx_factor, spx_ei_step or spx_ei_grid has run) -- for SPX_LOO_TIME one made while a time model was held; no fantasies held
 * (the resident rows would include pending points whose values are placeholders); a single-GPU handle without a communicator
 * and without a 2-D partition; loo_mean, loo_var non-NULL.
 * State: a reader, as spx_get_factor is.  Nothing is dropped or set: candidates, the results of the last pass, options and the
 * acquisition setting are bit for bit what they were.                                                                        */
#define SPX_LOO_OBJECTIVE 0
#define SPX_LOO_TIME      1   /* the log-duration GP of spx_set_time_model */
int spx_loo(spx_handle* h, int32_t model,
            double* loo_mean,   /* H x N */
            double* loo_var,    /* H x N */
            double* kinv_diag); /* H x N; may be NULL */

/* ---- one-shot convenience: host buffers in, results out ------------------ */
/* == ei_over_hypers + argmax(mean) (GPEIOptChooser.py:331-341, :294).
 * ei_mean_out (M) and ei_draw_out (M x H) may be NULL.                         */
int spx_ei_grid(spx_handle* h,
                const double* comp, const double* vals, int64_t N, int32_t D,
                const double* cand, int64_t M,
                const double* hypers, int32_t H, int32_t flags,
                double* ei_mean_out, double* ei_draw_out,
                int64_t* best_idx, double* best_val);
/* == GPEIperSecChooser.ei_over_hypers with all draws evaluated (:284-302) */
int spx_ei_per_sec_grid(spx_handle* h,
                const double* comp, const double* vals, const double* log_durs,
                int64_t N, int32_t D, const double* cand, int64_t M,
                const double* hypers, const double* time_hypers, int32_t H,
                int32_t flags, double* ei_mean_out, double* ei_draw_out,
                int64_t* best_idx, double* best_val);

/* ---- hyper-parameter slice sampling (the caller of spx_gp_logprob) -----------------------
 * The reference's sample_hypers (spearmint/spearmint/chooser/GPEIChooser.py:268-346; GPEIOptChooser.py:621-706;
 * GPEIperSecChooser.py:558-700) on util.slice_sample (spearmint/spearmint/util.py:34-93): per iteration ONE joint
 * random-direction move over [mean, amp2, noise] and ONE component-wise sweep over the length scales, every
 * log-probability a covariance build + Cholesky + solve.  spx_sample_hypers runs `n_iter` such iterations for the
 * resident observations (spx_set_observations) inside the library: the control flow of the sampler, the priors, the
 * speculative batching of its evaluations (each batch = one spx_gp_logprob call) and numpy's legacy random stream
 * (MT19937: rand / randn / shuffle as numpy.random.RandomState produces them) are host C++ -- no interpreter between
 * two GPU calls.  It is the SAME Markov chain as the reference's: the same points are accepted and the generator is
 * left in the same state, draw for draw (tests/test_sampler_native.py pins it to the reference's golden trace).
 *
 *   cfg        which model is sampled and how deep the speculation goes (below)
 *   rng        numpy.random.get_state() in, the state to numpy.random.set_state() out
 *   hyper_io   [mean, noise, amp2, ls[0..D)] -- the chain's current point in, its last point out
 *   rows_out   n_iter rows [mean, noise, amp2, ls...]: the point after every iteration (NULL: not wanted)
 *   hist_io    12 doubles of bracket statistics the speculation learns from (zeros to start; keep between calls)
 *   stats_out  SPX_SAMPLER_NSTATS values: {spx_gp_logprob calls, hyper rows evaluated, slice moves, moves that needed no
 *              call, iterations completed, then calls by number of hyper rows: [5 + r] for r = 0 .. 32, [38] beyond, [39] nanoseconds
 *              inside the log-likelihood calls, [40] nanoseconds in all} (NULL ok)
 *
 * Errors (the iteration that failed is left as the reference leaves it: a finished joint move is applied, an
 * unfinished sweep is not; `rng` is where the reference's generator would be; rows_out holds the iterations done;
 * stats_out[4] = iterations completed):
 *   SPX_ERR_NOT_PD      a covariance the sampler really evaluated was not positive definite (spla.cholesky raises)
 *   SPX_ERR_SLICE_NAN   "Slice sampler got a NaN"          (util.py:59-61)
 *   SPX_ERR_SLICE_ZERO  "Slice sampler shrank to zero!"    (util.py:68-69)                                            */
#define SPX_SAMPLER_NSTATS 41
#define SPX_ERR_SLICE_NAN  -4
#define SPX_ERR_SLICE_ZERO -5
typedef struct spx_rng_state {      /* numpy.random.get_state(): ('MT19937', key, pos, has_gauss, cached_gaussian)     */
    uint32_t key[624];
    int32_t  pos;
    int32_t  has_gauss;
    double   gauss;
} spx_rng_state;
typedef struct spx_sampler_cfg {
    int32_t D;                    /* input dimensions = number of length scales                                        */
    int32_t n_iter;               /* iterations: (joint move, length-scale sweep) each                                   */
    int32_t noiseless;            /* 1: noise pinned to 1e-3 (GPEIChooser.py:270,326)                                    */
    int32_t check_mean;           /* 1: -inf for a mean outside [vals_min, vals_max] (GPEIChooser.py:289-290)            */
    int32_t amp2_prior_on_sqrt;   /* log-normal prior on sqrt(amp2) (GPEIOptChooser.py:668) instead of amp2 (:312)       */
    int32_t lookahead;            /* step-out points per side and shrink proposals evaluated per call (>= 1)             */
    int32_t follow_props;         /* cross-move speculation: proposals planned for the NEXT coordinate's move ...        */
    int32_t follow_hyps;          /* ... under the hypotheses "this move accepts its 1st .. follow_hyps-th proposal"     */
    int32_t max_rows;             /* hyper rows per spx_gp_logprob call the speculation may fill (<= 32 stays one launch) */
    double  noise_scale;          /* horseshoe prior on the noise   (GPEIChooser.py:309)                                 */
    double  amp2_scale;           /* log-normal prior on the amplitude                                                  */
    double  max_ls;               /* top-hat prior on the length scales (GPEIChooser.py:279)                             */
    double  vals_min, vals_max;   /* min / max of the observed values (the mean's support)                               */
} spx_sampler_cfg;
int spx_sample_hypers(spx_handle* h, const spx_sampler_cfg* cfg, spx_rng_state* rng, double* hyper_io,
                      double* rows_out, double* hist_io /* 12 */, int64_t* stats_out /* SPX_SAMPLER_NSTATS */);
/* The same sampler on a caller-supplied log-likelihood: fn(ctx, rows[n_rows][3 + D], n_rows, lp_out[n_rows]) returns
 * 0 and the data term -sum log diag L - 0.5 r'K^-1 r per row (-inf = not positive definite).  No handle, no GPU:
 * how the CPU tests hold the sampler to the reference's chain, and how a host evaluator can be plugged in.  The
 * choosers never use it -- their sampler is spx_sample_hypers on the GPU.                                              */
typedef int (*spx_logprob_fn)(void* ctx, const double* rows, int32_t n_rows, double* lp_out);
int spx_sample_hypers_with(spx_logprob_fn fn, void* ctx, const spx_sampler_cfg* cfg, spx_rng_state* rng,
                           double* hyper_io, double* rows_out, double* hist_io, int64_t* stats_out);
/* numpy's legacy generator, for tests: n_rand x rand(), then n_randn x randn(), then a shuffle of range(n_shuffle)
 * (outputs may be NULL when their count is 0).                                                                         */
int spx_rng_draw(spx_rng_state* rng, int32_t n_rand, double* rand_out, int32_t n_randn, double* randn_out,
                 int32_t n_shuffle, int32_t* shuffle_out);


/* ---- building blocks (per-stage parity tests, "next" rows) --------------- */
/* After spx_factor: K + noise I (N x N, full symmetric), its lower Cholesky
 * factor L (N x N, strict upper = 0) and alpha = K^-1 (vals - mean) (N) of
 * draw `draw` (time model: draw + H).  Any pointer may be NULL.               */
int spx_get_factor(spx_handle* h, int32_t draw, double* K, double* L, double* alpha);
/* Rows [row0, row0 + nrows) of L (nrows x N, row-major, zeros above the diagonal) and gamma = L^-1 (vals - mean) (N) of one
 * draw; either pointer may be NULL.  The pending branch (GPEIChooser.py:219-249) needs only the bottom P rows of the factor
 * of cov([comp; pend]) and gamma: pend_m = L21 gamma[:N] + mean, pend_K = L_S L_S^T - noise I (L21 = rows N.., columns < N;
 * L_S the trailing P x P block) -- a P x (N + P) block per draw instead of the whole factor.                          */
int spx_get_factor_rows(spx_handle* h, int32_t draw, int64_t row0, int64_t nrows, double* L_rows, double* gamma);
/* K(X*,X) of draw `draw` for candidates [c0, c0+nc): N x nc row-major.         */
int spx_get_cross_cov(spx_handle* h, int32_t draw, int64_t c0, int64_t nc, double* out);
/* func_m, func_v (M each) of draw `draw`; needs SPX_FLAG_KEEP_MOMENTS.          */
int spx_get_moments(spx_handle* h, int32_t draw, double* func_m, double* func_v);
/* exp(predicted log duration) of every candidate under time draw `draw`
 * (func_time_m, GPEIperSecChooser.py:452-458); needs SPX_FLAG_PER_SEC | SPX_FLAG_KEEP_MOMENTS. */
int spx_get_time_mean(spx_handle* h, int32_t draw, double* out /* M */);
/* P_d(x) of every candidate under draw `draw` of the constraint model; needs SPX_FLAG_CONSTRAINED | SPX_FLAG_KEEP_MOMENTS
 * on the last pass (spx_get_ei_draws then holds EI_d * P_d).                                                          */
int spx_get_constraint_prob(spx_handle* h, int32_t draw, double* out /* M */);
/* GP marginal log-likelihood data term  -sum(log diag L) - 0.5 r' K^-1 r  for
 * each resident draw (GPEIChooser.py:281-285): out has H entries, -inf where
 * the covariance is not PD.  Needs spx_set_observations + spx_set_hypers.      */
int spx_gp_logprob(spx_handle* h, double* out);
/* The same data term with a right-hand side of its own per hyper row (the probit constraint GP's [amp2_c, ff] slice move,
 * GPConstrainedEIChooser.py:1159-1201, where every proposal carries its own ff): n_rows (1 .. 32, one launch) rows
 * [mean, noise, amp2, ls...] -- [0, noise_c, amp2_c, ls_c...] for that move -- and rhs (n_rows x N, row-major); row k's
 * residual is rhs[k] - mean_k.  The points are THIS handle's resident observations (spx_set_observations; their values
 * are not read): the constrained chooser keeps a handle of its own holding the completed points.  Replaces the
 * resident hypers as spx_set_hypers does.  With rhs[k] = vals - mean_k for every row the result equals spx_gp_logprob
 * bit for bit.  lp_out: n_rows values, -inf where not PD.  SPX_ERR_ARG on a multi-device handle.                 */
int spx_gp_logprob_rhs(spx_handle* h, const double* rows, const double* rhs /* n_rows x N */, int32_t n_rows,
                       double* lp_out);
/* Objective of the local refinement (GPEIOptChooser.py:360-525 grad_optimize_ei_over_hypers;
 * "next" row 3) at P points in ONE call -- the reference runs grid_subset (20) L-BFGS-B problems,
 * one objective evaluation at a time (:265-291): points (P x D) -> neg_ei[p] = the summed
 * negative EI over the resident draws, grad (P x D) its gradient, in the reference's scaling (its
 * grad_xp carries a factor one half).  A point's result does not depend on the other points of
 * the call.  Needs spx_factor or a previous spx_ei_grid.  With fantasies set (spx_set_fantasies;
 * the pending branch :441-525) EI and gradient are averaged over the S fantasies per draw; with
 * a factored time model (spx_set_time_model / spx_ei_per_sec_grid) the objective is EI per second
 * (GPEIperSecChooser.py:349-434; not combinable with fantasies, as in the reference).          */
int spx_ei_grad_batch(spx_handle* h, const double* points, int32_t P, double* neg_ei /* P */,
                      double* grad /* P x D */);
/* == spx_ei_grad_batch with P = 1 */
int spx_ei_grad(spx_handle* h, const double* point, double* neg_ei_sum, double* grad /* D */);
/* Objective of the CONSTRAINED chooser's local refinement (GPConstrainedEIChooser.py:471-501 grad_optimize_ei_over_hypers
 * over :529-690 / :692-803) at P points in one call: neg_cei[p] = -(sum over the resident draws of EI_d x P_d), grad (P x D)
 * its gradient in the reference's scaling (factor one half, as spx_ei_grad_batch).  Needs spx_factor / spx_ei_step and a
 * factored constraint model (spx_set_constraint_model before that spx_factor); SPX_ERR_ARG otherwise, with a time model,
 * and on a multi-device handle.  `best` is the caller's np.min of the VALID values (:655): neither the values the handle
 * holds nor the `bests` of spx_set_fantasies are read.  The reference's arithmetic, quirks included:
 *   no fantasies, Nc > 0   the predictive mean comes from the handle's own factor (the valid points), the variance and its
 *                          part of the gradient from the SAME hypers over ALL completed points X_c:
 *                          amp2 (k(X_c,X_c) + 1e-6 I) + noise I is factored on an internal handle on the first call (the
 *                          ordinary factorisation path; SPX_ERR_NOT_PD, spx_not_pd_info reporting draw 3H + d) and kept
 *                          until observations, hypers, the constraint model or option "covar" change.
 *                          value_d = -EI_d P_d, grad_d = P_d grad(-EI_d) + EI_d gcm_d with
 *                          gcm_d = 0.5 amp2_c gain phi(gain m_c) (alpha_c . dk_c/dx)   (the reference's sign)
 *   no fantasies, Nc = 0   P = 1: equal to spx_ei_grad_batch bit for bit (given best = the handle's own minimum)
 *   fantasies set          observations = [valid; pend]: every fantasy is scored against `best`, and EI and its gradient
 *                          are SUMMED over the S fantasies (spx_ei_grad_batch averages): -(sum_s EI_s) P,
 *                          P sum_s grad(-EI_s) + (sum_s EI_s) gcm.
 * A point's result does not depend on the other points of the call.                                                  */
int spx_constrained_ei_grad_batch(spx_handle* h, const double* points, int32_t P, double best,
                                  double* neg_cei /* P */, double* grad /* P x D */);
/* Sobol candidate grid on the device (ExperimentGrid.py:192-196 -> sobol_lib.py:125-157
 * i4_sobol_generate; "next" row 4): grid (n x dim, row-major) = transpose(i4_sobol_generate(dim,
 * n, skip)), bit-identical to the reference.  dirs = its scaled direction integers V[d][b]
 * (dim_max x 30 uint32, host; spearmint_amd/data/sobol_dirs_*.npy), dim <= dim_max,
 * skip + n - 2 < 2^30.  grid_out (host) may be NULL.  as_candidates != 0 also leaves the grid
 * resident as the candidate set (== spx_set_candidates(grid, n, dim, 0) without the host copy).
 * kernel_ms (may be NULL) receives the HIP-event duration of the generating kernel.          */
int spx_sobol_grid(spx_handle* h, const uint32_t* dirs, int32_t dim_max, int32_t dim, int64_t n,
                   int64_t skip, double* grid_out, int32_t as_candidates, double* kernel_ms);
/* which draw / pivot failed in the last SPX_ERR_NOT_PD                         */
int spx_not_pd_info(spx_handle* h, int32_t* draw, int32_t* pivot);

/* ---- measurement ---------------------------------------------------------- */
/* Per-kernel accumulated HIP-event time of the last spx_factor + spx_ei_run
 * executed with SPX_FLAG_TIMING.  Fills up to n entries of ms[] / launches[]
 * in the order of spx_timing_name(i); returns the number of stages.            */
int spx_get_timings(spx_handle* h, double* ms, int64_t* launches, int n);
/* Counters a caller can poll (single-GPU handles; "ranks_seen" also on a multi-device handle):
 *   "flow_fallbacks"   in-launch hand-off time-outs of the one-launch factorisation (k_lean_flow) so far.  The call
 *                      that saw one is repeated with one launch per block column (same bits) and returns SPX_OK with
 *                      a WARNING left in spx_last_error() (text starts with "warning:"); the handle then keeps that
 *                      form for "flow_rearm_after" clean factorisations (option, default 16; 0 = for good) and goes
 *                      back to the one-launch form by itself -- or at once on spx_set_option("lean_flow", 1).  Never
 *                      seen on a healthy device; bounded polls make it an error path instead of a hang;
 *   "flow_rearms"      times the handle went back to the one-launch form after a fallback;
 *   "flow_enabled"     1 while the one-launch factorisation is in use;   "n_cu"  compute units of the device;
 *   "last_step_fused"  1 if the last EI pass ran as a one-kernel form (no K* / beta in memory; no fantasies);
 *   "last_factor_flow" 1 if the last factorisation (spx_factor, spx_ei_step, spx_gp_logprob) was the one data-flow launch;
 *   "last_factor_cov_in_flow"  1 if that launch built the tiles of K(X,X) itself (option "lean_flow_cov"), 0 if k_cov wrote them;
 *   "last_logprob_one_launch"  1 if the last spx_gp_logprob ran as ONE launch (option "lean_one");
 *   "last_step_skipped_padding"  1 if the last EI pass left the padding of N (to the GEMM's 128-row tiles) uncomputed
 *                      (option "gemm_partial", default on: same bits, up to -31 % per pass just above a multiple of 128);
 *   "last_fantasies_device"  1 while the resident fantasies came from spx_draw_fantasies; 0 after spx_set_fantasies or when there are none
 *                      (on a multi-device handle: device slot 0's);   "fantasies_pending_rows", "fantasies_count": P and S of those
 *                      fantasies (the sizes spx_get_pending_fantasies writes), 0 while last_fantasies_device is 0;
 *   "last_kstar_ring"  staging slots of the K(X*,X) ring the last EI pass ran with (option "streams" = 3; 0: it ran another way);
 *   "last_corun_launches"  K(X*,X) launches of that pass in the form that fits beside two GEMM workgroups (k_cov_corun);
 *   "gemm_lds_bytes"   dynamic LDS of one predict-GEMM workgroup (two are resident per CU; the co-resident K(X*,X) form uses none);
 *   "obs_dims"         D of the resident observations (0: none set);   "hip_runtime_version", "hip_driver_version", "clock_khz",
 *                      "mem_clock_khz", "wall_clock_khz", "l2_bytes", "mem_bus_bits": what the process runs on (bench.py: platform);
 *   "ranks_seen"       size of the communicator the last exchange ran on (one record per rank in its table): the ranks of the attached communicator
 *                      (spx_comm_attach), the device slots of a multi-device handle, 1 otherwise.                  */
int spx_get_stat(spx_handle* h, const char* name, int64_t* value);
const char* spx_timing_name(int i);
/* The correlation function of the GP -- the choosers' covar= argument, a function of
 * spearmint/spearmint/gp.py selected by name (GPEIChooser.py:52): option "covar" of a handle.
 * Every entry point (K, K*, log-likelihood, EI grid, EI gradient) follows it; changing it
 * invalidates the factorisation.                                                             */
#define SPX_COVAR_MATERN52 0   /* gp.Matern52 (gp.py:120-127), the default                     */
#define SPX_COVAR_MATERN32 1   /* gp.Matern32 (gp.py:107-113)                                   */
#define SPX_COVAR_ARDSE    2   /* gp.ARDSE    (gp.py:95-100)                                    */
#define SPX_COVAR_SE       3   /* gp.SE       (gp.py:87-93): ARDSE with the length scales ignored */
/* options: "covar" (SPX_COVAR_*); tuning knobs "kstar_budget_bytes" (K(X*,X) staging buffer;
 * 0 = default), "streams" (1|2|3, below), "timing" (0|1), "gemm_waves" (predict-GEMM variant of THIS
 * handle; values the build does not contain are rejected with SPX_ERR_ARG), and the forms of the
 * factorisation, all bit-identical, -1 = the default / chosen from the sizes:
 *   "lean_flow"     1 (default): the whole factorisation of spx_gp_logprob is ONE data-flow launch
 *                   (k_lean_flow: every dependency a hand-off inside the launch); 0: one launch per
 *                   block column, in the forms selected by "lean_ps" / "lean_lazy";
 *   "ei_flow"       the same choice for spx_factor (default 1);
 *   "lean_flow_cu"  k_lean_flow with one workgroup per CU (1) or two (0); -1: by size;
 *   "lean_flow_yield" with two per CU: a workgroup yields while its neighbour on the CU factors a
 *                   diagonal block (1, default) or does not (0);
 *   "lean_flow_cov" k_lean_flow builds the tiles of K(X,X) itself (1, default) or reads k_cov's (0);
 *   "lean_lazy"     trailing updates one (0) or two (1) block columns at a time;
 *   "lean_merge"    spx_gp_logprob: observation scaling and the right-hand-side rows in one launch (1, default) or two (0);
 *   "lean_ps"       1: the panel solve of a block column runs inside the update launch, handed the
 *                   inverse of the diagonal block behind its pivots; 0: a launch of its own.
 * If an in-launch hand-off ever times out (its polls are bounded; never observed), the call is
 * repeated with one launch per block column, a warning is left in spx_last_error(), and the handle
 * stays in that form for "flow_rearm_after" clean factorisations (see spx_get_stat).
 *   "streams"           how K(X*,X) of an EI pass is scheduled against the predict GEMM that reads it; the same bits in all:
 *                       1 (default) one stream, each K(X*,X) launch in front of its GEMM; 2 a second stream and two staging
 *                       buffers (the next item is produced while this one is consumed); 3 a stream of the device's lowest
 *                       priority and a ring of staging slots: K(X*,X) runs up to a ring ahead, beside the GEMMs (and, in
 *                       spx_ei_step, beside the factorisation), in a kernel form that fits into what two resident GEMM
 *                       workgroups leave of a CU.  With "timing" = 1 a streams = 3 pass runs as streams = 1, so that every
 *                       stage's events bracket its own kernels; the fused N <= 128 path never uses more than one stream;
 *   "kstar_ring"        streams = 3: staging slots of the ring; 0 (default) as many as a sixteenth of the free device memory
 *                       holds, at most 10 GiB, never more than the pass has work items (spx_get_stat "last_kstar_ring");
 *   "kstar_corun"       streams = 3: K(X*,X) launches behind a pass's first use the co-resident kernel form (1, default) or
 *                       the stand-alone one (0);
 *   "gemm_partial"      N not a multiple of 128: the last 128-row block of the predict GEMM computes only the 16-row tiles
 *                       that hold observations (k_predict_gemm_tail) and K(X*,X) does not write the pad rows (1, default,
 *                       where it saves at least 12 % of the pass), or everything is computed on the padded size (0);
 *   "cov_flat"          K(X*,X) launches of several residency rounds deal their work out in equal contiguous shares
 *                       (k_cov_flat; 1, default) or run as the 3-D grid (0); the same bits.  Holds for the launches of an EI
 *                       pass and for spx_get_cross_cov, so that the two forms can be compared element by element;
 *   "flow_rearm_after"  clean factorisations before the one-launch form is tried again (default 16, 0 = never);
 *   "flow_spin_limit"   polls a waiting workgroup makes before it gives up (0 = default, 2^20); tests set 1.
 * A kernel that is refused the dynamic LDS it asks for (hipFuncSetAttribute) makes the call fail with
 * SPX_ERR_HIP and a message naming the kernel and the size.                                       */
int spx_set_option(spx_handle* h, const char* name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* SPX_H */
