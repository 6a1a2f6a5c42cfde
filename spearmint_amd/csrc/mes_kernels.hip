// Max-value entropy search (spx.h SPX_ACQ_MES): the second stage behind an ordinary grid pass that kept its moments.
// Per hyper draw, from mom_m / mom_v ([H][Mp], real candidates c < M only):
//   k_mes_bounds    partial minima of mu - 8 sigma and mu + 5 sigma over the valid candidates (a min is exact in any order)
//   k_mes_logsurv   G_j = sum over the valid candidates of log Phi((mu - y_j) / sigma) for the J probe values -- the hot one:
//                   M H J evaluations of log Phi; a workgroup stages MES_CT candidates once and every thread owns one probe
//   k_mes_fit       the second stage of both reductions, the three quartiles, the Gumbel fit, the y* table and the fit record
//   k_mes_values    MES_d(c) = (sum_k h(gamma_k)) / K into the per-draw value buffer launch_mean_argmax reads
// Deterministic: no atomics; a partial sum covers candidates [b MES_CT, (b + 1) MES_CT) in index order and the second stage
// adds the partials in block order, both with a compensated (Neumaier) accumulator, so G of a draw is a function of that
// draw's moments, M and J alone and its summation error stays under two ulp whatever M is.
#include "mes_device.h"

// (MES_CT / MES_BT, candidates per partial sum / minimum, and mes_sum_blocks / mes_bound_blocks: spx_geom.h)

// min over the block of two values and the "or" of a flag; every thread returns with the results
__device__ __forceinline__ void mes_block_min2(double& lo, double& hi, double& any, double (*red)[4])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, off));
        hi = fmin(hi, __shfl_xor(hi, off));
        any = fmax(any, __shfl_xor(any, off));
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
        red[2][threadIdx.x >> 6] = any;
    }
    __syncthreads();
    lo = fmin(fmin(red[0][0], red[0][1]), fmin(red[0][2], red[0][3]));
    hi = fmin(fmin(red[1][0], red[1][1]), fmin(red[1][2], red[1][3]));
    any = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
}

// bpart[h][b] = {min(mu - 8 sigma), min(mu + 5 sigma), 1 if any candidate was valid} over candidates [b MES_BT, (b + 1) MES_BT)
__global__ __launch_bounds__(256) void k_mes_bounds(const double* __restrict__ mom_m, const double* __restrict__ mom_v,
                                                    double* __restrict__ bpart, int64_t M, int64_t Mp, int nbb)
{
#pragma clang fp contract(off)
    __shared__ double red[3][4];
    const int h = blockIdx.y, b = blockIdx.x;
    const double inf = __builtin_huge_val();
    double lo = inf, hi = inf, any = 0.0;
    for (int i = threadIdx.x; i < MES_BT; i += 256) {
        const int64_t c = (int64_t)b * MES_BT + i;
        if (c >= M) break;
        const double mu = mom_m[(size_t)h * Mp + c], v = mom_v[(size_t)h * Mp + c];
        if (!mes_valid(mu, v)) continue;
        const double sg = sqrt(v);
        const double a8 = 8.0 * sg, a5 = 5.0 * sg;
        lo = fmin(lo, mu - a8);
        hi = fmin(hi, mu + a5);
        any = 1.0;
    }
    mes_block_min2(lo, hi, any, red);
    if (threadIdx.x == 0) {
        double* o = bpart + ((size_t)h * nbb + b) * 3;
        o[0] = lo; o[1] = hi; o[2] = any;
    }
}

// the second stage of the bounds for draw h: lo, hi (NaN without a valid candidate) in every thread
__device__ __forceinline__ void mes_draw_bounds(const double* __restrict__ bpart, int h, int nbb, double (*red)[4], double& lo,
                                                double& hi, bool& any_valid)
{
    const double inf = __builtin_huge_val();
    double any = 0.0;
    lo = inf; hi = inf;
    for (int b = threadIdx.x; b < nbb; b += 256) {
        const double* o = bpart + ((size_t)h * nbb + b) * 3;
        lo = fmin(lo, o[0]);
        hi = fmin(hi, o[1]);
        any = fmax(any, o[2]);
    }
    mes_block_min2(lo, hi, any, red);
    any_valid = any > 0.0;
    if (!any_valid) { lo = __builtin_nan(""); hi = __builtin_nan(""); }
}

// part[h][b][j] = sum over the valid candidates c of block b of log Phi((mu_c - y_j) / sigma_c), y_j = lo + j step
__global__ __launch_bounds__(256) void k_mes_logsurv(const double* __restrict__ mom_m, const double* __restrict__ mom_v,
                                                     const double* __restrict__ bpart, int nbb, double* __restrict__ part,
                                                     int64_t M, int64_t Mp, int J, int nb)
{
#pragma clang fp contract(off)
    __shared__ double red[3][4];
    __shared__ double sm[MES_CT], ss[MES_CT];
    const int h = blockIdx.z, b = blockIdx.x, tid = threadIdx.x;
    double lo, hi;
    bool any_valid;
    mes_draw_bounds(bpart, h, nbb, red, lo, hi, any_valid);
    const int64_t c0 = (int64_t)b * MES_CT;
    const int n = (int)(M - c0 < MES_CT ? M - c0 : MES_CT);
    for (int i = tid; i < MES_CT; i += 256) {
        double mu = 0.0, sg = 0.0;               // sigma = 0 marks a candidate that is left out
        if (i < n) {
            const double m_ = mom_m[(size_t)h * Mp + c0 + i], v = mom_v[(size_t)h * Mp + c0 + i];
            if (mes_valid(m_, v)) { mu = m_; sg = sqrt(v); }
        }
        sm[i] = mu; ss[i] = sg;
    }
    __syncthreads();
    const int j = blockIdx.y * 256 + tid;
    if (j >= J) return;
    const double step = (hi - lo) / (double)(J - 1);
    const double jy = (double)j * step;
    const double y = lo + jy;
    double s = 0.0, comp = 0.0;
    for (int i = 0; i < n; ++i) {
        const double sg = ss[i];
        if (sg > 0.0) mes_add(s, comp, mes_log_ndtr((sm[i] - y) / sg));
    }
    part[((size_t)h * nb + b) * J + j] = s + comp;
}

// One workgroup per draw: G_j = the partial sums in block order, the quartiles of the minimum by linear interpolation of G on
// the probe grid, the reflected-Gumbel fit, K levels y*_k = min(a + b w_k, cap).  fit[h] = {lo, hi, y25, y50, y75, a, b, cap}.
__global__ __launch_bounds__(256) void k_mes_fit(const double* __restrict__ bpart, int nbb, const double* __restrict__ part,
                                                 int nb, int J, int K, const double* __restrict__ hyp, int hs, double best,
                                                 double* __restrict__ G, double* __restrict__ ystar, double* __restrict__ fit)
{
#pragma clang fp contract(off)
    extern __shared__ double sg[];     // [J]
    __shared__ double red[3][4];
    __shared__ double sh_q[3], sh_ab[3];
    const int h = blockIdx.x;
    double lo, hi;
    bool any_valid;
    mes_draw_bounds(bpart, h, nbb, red, lo, hi, any_valid);
    mes_fit_record(lo, hi, any_valid, part + (size_t)h * nb * J, nb, J, K, hyp[(size_t)h * hs + 1], best, G + (size_t)h * J,
                   ystar + (size_t)h * K, fit + (size_t)h * 8, sg, sh_q, sh_ab);
}

// one thread per (candidate, draw); pad columns c >= M are not written, as k_ei_finalize leaves them
__global__ __launch_bounds__(256) void k_mes_values(const double* __restrict__ mom_m, const double* __restrict__ mom_v,
                                                    const double* __restrict__ ystar, int K, double* __restrict__ ei_draw,
                                                    int64_t M, int64_t Mp)
{
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y;
    if (c >= M) return;
    const size_t o = (size_t)h * Mp + c;
    const double mu = mom_m[o];
    const double sg = sqrt(mom_v[o]);               // NaN for func_v < 0, as np.sqrt
    const double* ys = ystar + (size_t)h * K;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
        double hh, unused;
        mes_h_terms<false>((mu - ys[k]) / sg, hh, unused);
        acc = acc + hh;
    }
    ei_draw[o] = acc / (double)K;
}

void launch_mes(hipStream_t s, const double* mom_m, const double* mom_v, const double* hyp, int hs, double best, int64_t M,
                int64_t Mp, int H, int J, int K, double* bpart, double* part, double* G, double* ystar, double* fit,
                double* ei_draw)
{
    const int nb = mes_sum_blocks(M), nbb = mes_bound_blocks(M);
    hipLaunchKernelGGL(k_mes_bounds, dim3(nbb, H), dim3(256), 0, s, mom_m, mom_v, bpart, M, Mp, nbb);
    hipLaunchKernelGGL(k_mes_logsurv, dim3(nb, (J + 255) / 256, H), dim3(256), 0, s, mom_m, mom_v, bpart, nbb, part, M, Mp, J, nb);
    hipLaunchKernelGGL(k_mes_fit, dim3(H), dim3(256), (size_t)J * sizeof(double), s, bpart, nbb, part, nb, J, K, hyp, hs, best, G,
                       ystar, fit);
    hipLaunchKernelGGL(k_mes_values, dim3((unsigned)((M + 255) / 256), H), dim3(256), 0, s, mom_m, mom_v, ystar, K, ei_draw, M, Mp);
}
