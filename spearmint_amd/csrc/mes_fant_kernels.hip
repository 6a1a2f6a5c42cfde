// Max-value entropy search over the fantasies of pending jobs (spx.h: option "mes_fantasies"): the plain rule of mes_kernels.hip
// per (draw d, fantasy s), then the mean over s.  Conditioned on the pending inputs a candidate's variance does not depend on
// the fantasy -- only its mean does -- so sigma is formed once per (d, c) and shared by the S fantasies in every stage:
//   k_mes_fant_means     per chunk, where k_ei_fant_values runs in an EI pass: one thread per (candidate, draw of the group,
//                        column) sums part_bgS over the row blocks in k_ei_fant_values' order into the resident mu [H][S][Mp];
//                        column 0 also sums part_ss into v [H][Mp]
//   k_mes_fant_bounds    a workgroup stages sigma of MESF_BT candidates once; each of its four waves walks fantasies against it
//                        (mu streamed from memory, coalesced) and writes {min(mu - 8 sigma), min(mu + 5 sigma), any} per
//                        (d, s, tile) -- no barrier inside the walk
//   k_mes_fant_bounds2   one thread per (d, s): the tiles' minima in tile order (a min is exact in any order); NaN without a
//                        valid candidate
//   k_mes_fant_logsurv   the hot one, M H S J evaluations of log Phi: see below
//   k_mes_fant_fit       one workgroup per (d, s): mes_fit_record of mes_device.h, the arithmetic of k_mes_fit, against
//                        best[d][s] and noise_d
//   k_mes_fant_values    one thread per (d, c): sigma once, the levels of a block of fantasies through LDS, h over k inside s,
//                        the mean over s in numpy's pairwise order (np_sum.h's tree, streamed: MES_ds(c) is never stored)
// k_mes_fant_logsurv.  A workgroup of 256 threads owns MESF_CT = 512 candidates of one draw and a run of fantasies.  It stages
// sigma of its tile ONCE (0 marks func_v not > 0), then walks its fantasies in blocks of MESF_SB = 8, staging mu[s][tile] per
// block; a thread owns one probe value j of one fantasy of the block and walks the tile in index order with a compensated
// accumulator.  With J >= 64 every lane of a wave has the same fantasy, so both LDS reads of a step are broadcasts; with a
// smaller J a wave spans several rows of mu, which are MESF_CT + 1 doubles apart (two banks per row: no conflict up to 32
// rows).  sigma is what is shared, not 1 / sigma: (mu - y) / sigma is the plain pass's and the oracle's operation, and a
// reciprocal multiply moves the argument by an ulp, which at a = 8 is 64 ulp of log Phi -- the division is 17 of the ~250
// instructions, the square root and the validity tests of func_v are what the S fantasies save.
// Sizes: LDS = 512 x 8 + 8 x 513 x 8 = 36.9 KB per workgroup, four workgroups (16 waves) on a CU's 160 KB; the tile is the plain
// kernel's, so G of (d, s) is bit for bit what k_mes_logsurv + k_mes_fit give for the same moments.  A larger SB only lowers
// the number of barriers (two per 8 x 512 x J evaluations as it is); a larger tile lowers the partial sums' footprint
// (H S ceil(M / 512) J doubles) at the price of residency.  The launcher splits the fantasies of a (draw, tile) over several
// workgroups until the grid has 2048 of them; a partial sum is one thread's, whatever the split: no atomics, same bits.
// fp64-VALU bound.  One log Phi as built (profiles/mes_pending_kernel_regs.txt; the candidate loop of the kernel, disassembled):
// 17 VALU instructions up to the quotient, 111 for the argument reduction and the head of erfc, 125 or 89 for the interval its
// argument falls in, 10 for the compensated addition -- about 250 on one path (350 when the lanes of a wave fall in both
// intervals), nearly all fp64, at 4 cycles per wave instruction of 64 lanes:
//     M H S J x 250 x 4 / 64 cycles over 1024 SIMDs at 2.4 GHz = M H S J / 1.57e11 s:
// C2 (20 000 x 10) at S = 100, J = 256: 33 ms; C3 (200 000 x 20) at S = 100: 650 ms.  What the count leaves out: the two LDS
// reads per step, the waves whose lanes sit in both of erfc's intervals (a runs over 13 sigma along j), the quarter-rate seeds
// of the division, exp and log, and the tail of a grid that is not a multiple of the device.  Measured: README, "MES while
// jobs are pending".
#include "mes_device.h"
#include "np_sum.h"

// (MESF_CT / MESF_BT, candidates per partial sum / minimum, and mes_fant_sum_blocks / mes_fant_bound_blocks: spx_geom.h)
#define MESF_SB 8          // fantasies whose means a workgroup of k_mes_fant_logsurv holds in LDS at a time
#define MESF_JW 256        // probe values per workgroup of k_mes_fant_logsurv
#define MESF_LV 2048       // y* levels a workgroup of k_mes_fant_values holds in LDS at a time (K <= 1024: at least two fantasies)
#define MESF_DBL_MAX 1.79769313486231570815e308

__global__ __launch_bounds__(256) void k_mes_fant_means(const double* __restrict__ part_ss, const double* __restrict__ part_bgS,
                                                        const double* __restrict__ htab, int nrb, int Mc, int nh, int S, int64_t c0,
                                                        int64_t M, int64_t Mp, int h0, double* __restrict__ mu /*[H][S][Mp]*/,
                                                        double* __restrict__ v /*[H][Mp]*/)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y / S, sidx = blockIdx.y - h * S;
    if (c >= Mc || c0 + c >= M) return;
    double bg = 0.0;
    for (int ib = 0; ib < nrb; ++ib) {
        const size_t o0 = ((((size_t)ib * 2 + 0) * nh + h) * S + sidx) * Mc + c;
        const size_t o1 = ((((size_t)ib * 2 + 1) * nh + h) * S + sidx) * Mc + c;
        bg += part_bgS[o0] + part_bgS[o1];
    }
    mu[((size_t)(h0 + h) * S + sidx) * Mp + c0 + c] = bg + htab[h * SPX_HT + 0];
    if (sidx == 0) {
        double ss = 0.0;
        for (int ib = 0; ib < nrb; ++ib) ss += part_ss[((size_t)ib * nh + h) * Mc + c];
        v[(size_t)(h0 + h) * Mp + c0 + c] = htab[h * SPX_HT + 3] - ss;
    }
}

void launch_mes_fant_means(hipStream_t s, const double* part_ss, const double* part_bgS, const double* htab, int nrb, int Mc, int nh,
                           int S, int64_t c0, int64_t M, int64_t Mp, int h0, double* mu, double* v)
{
    hipLaunchKernelGGL(k_mes_fant_means, dim3((Mc + 255) / 256, nh * S), dim3(256), 0, s, part_ss, part_bgS, htab, nrb, Mc, nh, S, c0,
                       M, Mp, h0, mu, v);
}

// sigma of candidates [c0, c0 + n) of draw h into LDS, 0 where func_v is not > 0 or not finite; slots i >= n: 0
__device__ __forceinline__ void mesf_stage_sigma(const double* __restrict__ v, double* s_sg, int64_t o, int n, int tile)
{
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < tile; i += 256) {
        double sg = 0.0;
        if (i < n) {
            const double vv = v[o + i];
            if (vv > 0.0 && isfinite(vv)) sg = sqrt(vv);
        }
        s_sg[i] = sg;
    }
}

// bpart[d][s][b] = {min(mu - 8 sigma), min(mu + 5 sigma), 1 if any candidate was valid} over candidates [b MESF_BT, (b + 1) MESF_BT)
__global__ __launch_bounds__(256) void k_mes_fant_bounds(const double* __restrict__ mu, const double* __restrict__ v,
                                                         double* __restrict__ bpart, int64_t M, int64_t Mp, int S, int nbb)
{
#pragma clang fp contract(off)
    __shared__ double s_sg[MESF_BT];
    const int b = blockIdx.x, h = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c0 = (int64_t)b * MESF_BT;
    const int n = (int)(M - c0 < MESF_BT ? M - c0 : MESF_BT);
    mesf_stage_sigma(v, s_sg, (int64_t)h * Mp + c0, n, MESF_BT);
    __syncthreads();
    const double inf = __builtin_huge_val();
    for (int s = blockIdx.y * 4 + wave; s < S; s += 4 * gridDim.y) {
        const double* m_ = mu + ((size_t)h * S + s) * Mp + c0;
        double lo = inf, hi = inf, any = 0.0;
        for (int i = lane; i < n; i += 64) {
            const double sg = s_sg[i], m = m_[i];
            if (!(sg > 0.0) || !(fabs(m) <= MESF_DBL_MAX)) continue;
            const double a8 = 8.0 * sg, a5 = 5.0 * sg;
            lo = fmin(lo, m - a8);
            hi = fmin(hi, m + a5);
            any = 1.0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, off));
            hi = fmin(hi, __shfl_xor(hi, off));
            any = fmax(any, __shfl_xor(any, off));
        }
        if (lane == 0) {
            double* o = bpart + (((size_t)h * S + s) * nbb + b) * 3;
            o[0] = lo; o[1] = hi; o[2] = any;
        }
    }
}

// bnd[d][s] = {lo, hi, any}: one thread per record, the tiles in order
__global__ __launch_bounds__(256) void k_mes_fant_bounds2(const double* __restrict__ bpart, double* __restrict__ bnd, int nrec, int nbb)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    const double inf = __builtin_huge_val();
    double lo = inf, hi = inf, any = 0.0;
    for (int b = 0; b < nbb; ++b) {
        const double* o = bpart + ((size_t)r * nbb + b) * 3;
        lo = fmin(lo, o[0]);
        hi = fmin(hi, o[1]);
        any = fmax(any, o[2]);
    }
    if (!(any > 0.0)) { lo = __builtin_nan(""); hi = __builtin_nan(""); }
    double* o = bnd + (size_t)r * 3;
    o[0] = lo; o[1] = hi; o[2] = any;
}

// part[d][s][b][j] = sum over the valid candidates c of tile b of log Phi((mu[d][s][c] - y_j) / sigma[d][c]), y_j = lo_ds + j step_ds.
// grid: (tiles, J chunks x fantasy runs of `sper`, draws)
__global__ __launch_bounds__(256) void k_mes_fant_logsurv(const double* __restrict__ mu, const double* __restrict__ v,
                                                          const double* __restrict__ bnd, double* __restrict__ part, int64_t M,
                                                          int64_t Mp, int S, int J, int nb, int sper)
{
#pragma clang fp contract(off)
    __shared__ double s_sg[MESF_CT];
    __shared__ double s_mu[MESF_SB][MESF_CT + 1];
    const int b = blockIdx.x, h = blockIdx.z, tid = threadIdx.x;
    const int njc = (J + MESF_JW - 1) / MESF_JW;
    const int run = blockIdx.y / njc, j0 = (blockIdx.y - run * njc) * MESF_JW;
    const int jn = J - j0 < MESF_JW ? J - j0 : MESF_JW;
    const int s_begin = run * sper, s_end = s_begin + sper < S ? s_begin + sper : S;
    const int64_t c0 = (int64_t)b * MESF_CT;
    const int n = (int)(M - c0 < MESF_CT ? M - c0 : MESF_CT);
    mesf_stage_sigma(v, s_sg, (int64_t)h * Mp + c0, n, MESF_CT);
    for (int s0 = s_begin; s0 < s_end; s0 += MESF_SB) {
        const int sn = s_end - s0 < MESF_SB ? s_end - s0 : MESF_SB;
        __syncthreads();       // the block before this one has been read
        for (int idx = tid; idx < sn * MESF_CT; idx += 256) {
            const int sl = idx / MESF_CT, i = idx - sl * MESF_CT;
            s_mu[sl][i] = i < n ? mu[((size_t)h * S + s0 + sl) * Mp + c0 + i] : 0.0;
        }
        __syncthreads();
        for (int p = tid; p < sn * jn; p += 256) {
            const int sl = p / jn, j = j0 + (p - sl * jn);
            const double* bd = bnd + ((size_t)h * S + s0 + sl) * 3;
            const double lo = bd[0], hi = bd[1];
            const double step = (hi - lo) / (double)(J - 1);
            const double jy = (double)j * step;
            const double y = lo + jy;
            const double* m_ = s_mu[sl];
            double acc = 0.0, comp = 0.0;
            for (int i = 0; i < n; ++i) {
                const double sg = s_sg[i], m = m_[i];
                if (sg > 0.0 && fabs(m) <= MESF_DBL_MAX) mes_add(acc, comp, mes_log_ndtr((m - y) / sg));
            }
            part[(((size_t)h * S + s0 + sl) * nb + b) * J + j] = acc + comp;
        }
    }
}

// one workgroup per (d, s) record
__global__ __launch_bounds__(256) void k_mes_fant_fit(const double* __restrict__ bnd, const double* __restrict__ part, int nb, int J,
                                                      int K, int S, const double* __restrict__ hyp, int hs,
                                                      const double* __restrict__ bests, double* __restrict__ G,
                                                      double* __restrict__ ystar, double* __restrict__ fit)
{
#pragma clang fp contract(off)
    extern __shared__ double sg[];     // [J]
    __shared__ double sh_q[3], sh_ab[3];
    const size_t r = blockIdx.x;
    const int h = (int)(r / S);
    const double* bd = bnd + r * 3;
    mes_fit_record(bd[0], bd[1], bd[2] > 0.0, part + r * nb * J, nb, J, K, hyp[(size_t)h * hs + 1], bests[r], G + r * J, ystar + r * K,
                   fit + r * 8, sg, sh_q, sh_ab);
}

// np_sum.h's np_pairwise over f(0) .. f(n - 1), each formed when it is consumed: the tree is walked left to right, so f is asked
// in index order, once per index.  The eight accumulators of a leaf rotate through one slot, so f has one call site per loop.
template <class F>
__device__ __forceinline__ double mesf_pairwise_leaf(F& f, int st, int n)
{
#pragma clang fp contract(off)
    double res = -0.0;
    int i = 0;
    if (n >= 8) {
        double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0, r5 = 0.0, r6 = 0.0, r7 = 0.0;
        for (; i < n - (n % 8); ++i) {
            const double x = f(st + i);
            const double t = i < 8 ? x : r0 + x;
            r0 = r1; r1 = r2; r2 = r3; r3 = r4; r4 = r5; r5 = r6; r6 = r7; r7 = t;
        }
        res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    }
    for (; i < n; ++i) res += f(st + i);
    return res;
}

template <class F>
__device__ __forceinline__ double mesf_pairwise(F& f, int n)
{
#pragma clang fp contract(off)
    int ws[2 * PW_DEPTH + 2], wn[2 * PW_DEPTH + 2];   // wn < 0: the add marker (np_pairwise's walk)
    double vs[PW_DEPTH + 2];
#pragma unroll
    for (int q = 0; q < 2 * PW_DEPTH + 2; ++q) { ws[q] = 0; wn[q] = 0; }
#pragma unroll
    for (int q = 0; q < PW_DEPTH + 2; ++q) vs[q] = 0.0;
    ws[0] = 0; wn[0] = n;
    int depth = 1;
    while (depth > 0) {
        const int st = ws[0], len = wn[0];
#pragma unroll
        for (int q = 0; q < 2 * PW_DEPTH + 1; ++q) { ws[q] = ws[q + 1]; wn[q] = wn[q + 1]; }
        --depth;
        if (len < 0) {
            const double s = vs[1] + vs[0];
#pragma unroll
            for (int q = 1; q < PW_DEPTH + 1; ++q) vs[q] = vs[q + 1];
            vs[0] = s;
        } else if (len <= 128) {
            const double s = mesf_pairwise_leaf(f, st, len);
#pragma unroll
            for (int q = PW_DEPTH + 1; q > 0; --q) vs[q] = vs[q - 1];
            vs[0] = s;
        } else {
            int n2 = len / 2;
            n2 -= n2 % 8;
#pragma unroll
            for (int q = 2 * PW_DEPTH + 1; q > 2; --q) { ws[q] = ws[q - 3]; wn[q] = wn[q - 3]; }
            ws[0] = st;      wn[0] = n2;
            ws[1] = st + n2; wn[1] = len - n2;
            ws[2] = 0;       wn[2] = -1;
            depth += 3;
        }
    }
    return vs[0];
}

// MES_ds(c) for the thread's candidate, s in index order; the levels of `sblk` fantasies at a time through LDS.  Every thread
// of the workgroup asks for the same s at the same time (S is uniform), the ones without a candidate included.
struct MesfTerm {
    const double* __restrict__ mu_c;    // mu[d][0][c]
    const double* __restrict__ ys_d;    // ystar[d][0][0]
    double* s_y;
    int64_t Mp;
    int S, K, sblk;
    double sg;
    bool live;
    __device__ __forceinline__ double operator()(int s)
    {
#pragma clang fp contract(off)
        const int sl = s % sblk;
        if (sl == 0) {
            const int cnt = (S - s < sblk ? S - s : sblk) * K;
            __syncthreads();
            for (int i = threadIdx.x; i < cnt; i += 256) s_y[i] = ys_d[(size_t)s * K + i];
            __syncthreads();
        }
        const double m = live ? mu_c[(size_t)s * Mp] : 0.0;
        const double* ys = s_y + sl * K;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
            double hh, unused;
            mes_h_terms<false>((m - ys[k]) / sg, hh, unused);
            acc = acc + hh;
        }
        return acc / (double)K;
    }
};

// one thread per (candidate, draw); pad columns c >= M are not written
__global__ __launch_bounds__(256) void k_mes_fant_values(const double* __restrict__ mu, const double* __restrict__ v,
                                                         const double* __restrict__ ystar, int S, int K,
                                                         double* __restrict__ ei_draw, int64_t M, int64_t Mp)
{
#pragma clang fp contract(off)
    __shared__ double s_y[MESF_LV];
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y;
    MesfTerm f;
    f.live = c < M;
    f.mu_c = mu + (size_t)h * S * Mp + (f.live ? c : 0);
    f.ys_d = ystar + (size_t)h * S * K;
    f.s_y = s_y;
    f.Mp = Mp; f.S = S; f.K = K;
    f.sblk = MESF_LV / K;
    f.sg = f.live ? sqrt(v[(size_t)h * Mp + c]) : 1.0;      // NaN for func_v < 0, as np.sqrt
    const double res = S <= 128 ? mesf_pairwise_leaf(f, 0, S) : mesf_pairwise(f, S);
    if (f.live) ei_draw[(size_t)h * Mp + c] = (0.0 + res) / (double)S;
}

void launch_mes_fant(hipStream_t s, const double* mu, const double* v, const double* hyp, int hs, const double* bests, int64_t M,
                     int64_t Mp, int H, int S, int J, int K, double* bpart, double* bnd, double* part, double* G, double* ystar,
                     double* fit, double* ei_draw)
{
    const int nb = mes_fant_sum_blocks(M), nbb = mes_fant_bound_blocks(M);
    const int njc = (J + MESF_JW - 1) / MESF_JW;
    int by = (S + 3) / 4;                               // k_mes_fant_bounds: at most 16 workgroups share a tile's fantasies
    if (by > 16) by = 16;
    hipLaunchKernelGGL(k_mes_fant_bounds, dim3(nbb, by, H), dim3(256), 0, s, mu, v, bpart, M, Mp, S, nbb);
    hipLaunchKernelGGL(k_mes_fant_bounds2, dim3((H * S + 255) / 256), dim3(256), 0, s, bpart, bnd, H * S, nbb);
    // fantasies per workgroup: whole blocks of MESF_SB, as few workgroups per (draw, tile, J chunk) as fill the grid to 2048
    const int nsb = (S + MESF_SB - 1) / MESF_SB;
    int64_t want = (2048 + (int64_t)nb * njc * H - 1) / ((int64_t)nb * njc * H);
    int runs = (int)(want < 1 ? 1 : want > nsb ? nsb : want);
    const int sper = (nsb + runs - 1) / runs * MESF_SB;
    runs = (S + sper - 1) / sper;
    hipLaunchKernelGGL(k_mes_fant_logsurv, dim3(nb, njc * runs, H), dim3(256), 0, s, mu, v, bnd, part, M, Mp, S, J, nb, sper);
    hipLaunchKernelGGL(k_mes_fant_fit, dim3(H * S), dim3(256), (size_t)J * sizeof(double), s, bnd, part, nb, J, K, S, hyp, hs, bests,
                       G, ystar, fit);
    hipLaunchKernelGGL(k_mes_fant_values, dim3((unsigned)((M + 255) / 256), H), dim3(256), 0, s, mu, v, ystar, S, K, ei_draw, M, Mp);
}
