// Thompson sampling by pathwise conditioning (spx.h: spx_thompson).  What is new on the device:
//   k_ts_prior    p_{d,s}(x) = scale_d sum_f w[s][f] cos2pi(nu_f . x + phase_f) for a block of rows (observations once,
//                 candidates per chunk): rows x features over K = Dp on the fp64 MFMA, phase + reduction + cos2pi on the
//                 accumulator registers, which are then the B operand of a second MFMA against W -- no feature reaches memory
//   k_ts_rhs      rhs[d][s][i] = (y_i - p_{d,s}(x_i)) - sig_d eps[s][i]: the right-hand sides launch_gamma_multi solves for
//   k_ts_finish   path = (bg + mean_d) + p_{d,s}(c) from the predict GEMM's per-fantasy partial sums (the S > 0 branch)
//   k_ts_argmin   per (d, s): numpy's argmin over the candidates -- the first NaN wins, else the first minimum -- in two stages
//
// k_ts_prior's bound.  A wave owns TS_RT tiles of 16 rows and walks the features 16 at a time.  Per tile of 16 rows x 16
// features (256 values, four per lane) the loop issues Dp / 4 MFMAs for the dot products, 4 for the contraction with up to 16
// columns of W, and 64 fp64 VALU instructions (the gfx950 listing: 40 v_fma, 8 v_mul, 12 v_add, 4 v_rndne): per value 3 (phase,
// rint, difference) + 13 (cos2pi, ts_device.h).  By
// cov_device.h's finding the fp64 VALU and the fp64 MFMA share the FMA units, 16 lanes a cycle per SIMD: a
// v_mfma_f64_16x16x4 holds the unit for 64 cycles, a 64-lane fp64 VALU instruction for 4.  So a tile costs
// 64 (Dp / 4 + 4) + 4 * 64 = 16 Dp + 512 cycles of one SIMD, (Dp + 32) / 16 per feature value: 2.5 cycles at Dp = 8, 4 at
// Dp = 32.  With 1024 SIMDs at 2.4 GHz the prior over M rows, H draws and F features is bounded by
//     M H F (Dp + 32) / 16 / 2.46e12 s     per block of 16 paths:
// 0.21 ms for 20 000 x 10 x 1024 at Dp = 8, 6.7 ms for 200 000 x 20 x 1024 at Dp = 32.  Measured (profiles/ts_time.jsonl, stage
// "ts_prior", which also brackets the observation-side launches): 1.6 x and 1.2 x that.  What is left in the loop beside the
// FMA-unit work: 24 accumulator-register moves and 10 loads per tile.  Memory is far below the bound: the rows are read once,
// and the frequencies arrive in operand order (ts_nu_index), 512 contiguous bytes per load of a wave -- with nu as a plain
// [F][Dp] array every operand load touched 16 cache lines and the Dp = 32 stage ran at 2.5 x its bound.
// (S > 16: every block of 16 paths forms the features again -- blockIdx.z; the bound is per block.)
#include "common.h"
#include "ts_device.h"

#define TS_RT 1            // row tiles of 16 per wave (one: 20 000 rows are 313 workgroups, enough for every CU)
#define TS_ROWS_WG (4 * 16 * TS_RT)

// KQ = Dp / 4 K steps with the rows' operand held in registers (Dp <= 32); KQ = 0: any Dp, the operand re-read per feature tile
template <int KQ>
__global__ __launch_bounds__(256) void k_ts_prior(const double* __restrict__ x /*[n][D]*/, int64_t n, int D, int Dp,
                                                  const double* __restrict__ nu /*[H][F / 16][Dp / 4][64]*/, const double* __restrict__ phase /*[F]*/,
                                                  const double* __restrict__ w /*[H or 1][S][F]*/, size_t w_stride,
                                                  const double* __restrict__ scale /*[H]*/, int F, int S,
                                                  double* __restrict__ out /*[H][S][ldo]*/, int64_t ldo, int64_t col0)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int d = blockIdx.y, sb = blockIdx.z;
    const int64_t rbase = ((int64_t)blockIdx.x * 4 + wave) * (16 * TS_RT);
    if (rbase >= n) return;                       // (whole wave: no barrier in this kernel)
    const double* nud = nu + (size_t)d * F * Dp;
    const double* wd = w + (size_t)d * w_stride;
    const int scol = sb * 16 + li;                // the path whose weights this lane supplies to the second MFMA
    // (lanes beyond S read path 0's weights: rows of the A operand beyond S feed accumulator rows that are never stored)
    const double* wrow = wd + (size_t)(scol < S ? scol : 0) * F;
    constexpr int NQ = KQ > 0 ? KQ : 1;
    const int nq = KQ > 0 ? KQ : Dp / 4;

    // B operand of the dot products: lane (li, g) supplies x[row li of the tile][dimension 4 q + g]; zeros beyond n and D
    double xb[TS_RT][NQ];
    if (KQ > 0) {
#pragma unroll
        for (int t = 0; t < TS_RT; ++t) {
            const int64_t row = rbase + 16 * t + li;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int k = 4 * q + g;
                xb[t][q] = (row < n && k < D) ? x[(size_t)row * D + k] : 0.0;
            }
        }
    }
    d4 acc[TS_RT];
#pragma unroll
    for (int t = 0; t < TS_RT; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};

    for (int f0 = 0; f0 < F; f0 += 16) {
        // The frequencies arrive in operand order (ts_nu_index): row i of the A tile is feature f0 + 4 (i % 4) + i / 4, so that
        // accumulator register r of lane (li, g) -- tile row g + 4 r -- is feature f0 + 4 g + r of row li: a lane's four phases
        // and its four weights are contiguous, and every operand load of the wave is one contiguous 512 bytes
        double ph[4], wa[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ph[r] = phase[f0 + 4 * g + r];
        // A operand of the contraction, K step r: W[path li][feature f0 + 4 g + r]
#pragma unroll
        for (int r = 0; r < 4; ++r) wa[r] = wrow[f0 + 4 * g + r];
        const double* pa = nud + (size_t)(f0 / 16) * nq * 64 + lane;      // A operand of the dot products, K step q at pa[64 q]
        d4 u[TS_RT];
#pragma unroll
        for (int t = 0; t < TS_RT; ++t) u[t] = (d4){0.0, 0.0, 0.0, 0.0};
        if (KQ > 0) {
            double af[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) af[q] = pa[64 * q];
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int t = 0; t < TS_RT; ++t) u[t] = MFMA_F64(af[q], xb[t][q], u[t]);
        } else {
            for (int q = 0; q < nq; ++q) {
                const double af = pa[64 * q];
                const int k = 4 * q + g;
#pragma unroll
                for (int t = 0; t < TS_RT; ++t) {
                    const int64_t row = rbase + 16 * t + li;
                    const double xv = (row < n && k < D) ? x[(size_t)row * D + k] : 0.0;
                    u[t] = MFMA_F64(af, xv, u[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < TS_RT; ++t) {
            double rr[4], c[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double uu = u[t][r] + ph[r];
                rr[r] = uu - __builtin_rint(uu);
            }
            cos2pi<4>(rr, c);
            // the tile of cosines is the B operand of K step r: p^T[path][row] += W[path][f0 + 4 r ..] c[f0 + 4 r ..][row]
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t] = MFMA_F64(wa[r], c[r], acc[t]);
        }
    }
    // accumulator register r of lane (li, g): path sb 16 + g + 4 r of row li
    const double sc = scale[d];
#pragma unroll
    for (int t = 0; t < TS_RT; ++t) {
        const int64_t row = rbase + 16 * t + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sidx = sb * 16 + g + 4 * r;
            if (row < n && sidx < S) out[((size_t)d * S + sidx) * ldo + col0 + row] = sc * acc[t][r];
        }
    }
}

// where nu[f][j] of one draw goes in the operand order k_ts_prior reads (F a multiple of 16, j < Dp): feature tile f / 16, K step
// j / 4, lane (j % 4) 16 + i with i the tile row of the feature, f % 16 = 4 (i % 4) + i / 4
size_t ts_nu_index(int f, int j, int Dp)
{
    const int e = f % 16, i = (e % 4) * 4 + e / 4;
    return ((size_t)(f / 16) * (Dp / 4) + j / 4) * 64 + (size_t)(j % 4) * 16 + i;
}

void launch_ts_prior(hipStream_t s, const double* x, int64_t n, int D, int Dp, const double* nu, const double* phase,
                     const double* w, size_t w_stride, const double* scale, int F, int S, int H, double* out, int64_t ldo,
                     int64_t col0)
{
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + TS_ROWS_WG - 1) / TS_ROWS_WG), H, (S + 15) / 16);
#define SPX_TSP(KQ_)                                                                                                       \
    hipLaunchKernelGGL(k_ts_prior<KQ_>, grid, dim3(256), 0, s, x, n, D, Dp, nu, phase, w, w_stride, scale, F, S, out, ldo, col0)
    if (Dp == 4) SPX_TSP(1);
    else if (Dp == 8) SPX_TSP(2);
    else if (Dp == 16) SPX_TSP(4);
    else if (Dp == 32) SPX_TSP(8);
    else SPX_TSP(0);
#undef SPX_TSP
}

__global__ __launch_bounds__(256) void k_ts_rhs(const double* __restrict__ vals /*[N]*/, const double* __restrict__ prior /*[H][S][N]*/,
                                                const double* __restrict__ eps /*[H or 1][S][N]*/, size_t eps_stride,
                                                const double* __restrict__ sig /*[H]*/, int64_t N, int S,
                                                double* __restrict__ rhs /*[H][S][N]*/)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int d = blockIdx.y / S, sidx = blockIdx.y - d * S;
    if (i >= N) return;
    const size_t o = ((size_t)d * S + sidx) * N + i;
    const double se = sig[d] * eps[(size_t)d * eps_stride + (size_t)sidx * N + i];
    rhs[o] = (vals[i] - prior[o]) - se;
}

void launch_ts_rhs(hipStream_t s, const double* vals, const double* prior, const double* eps, size_t eps_stride,
                   const double* sig, int64_t N, int S, int H, double* rhs)
{
    hipLaunchKernelGGL(k_ts_rhs, dim3((unsigned)((N + 255) / 256), H * S), dim3(256), 0, s, vals, prior, eps, eps_stride, sig, N,
                       S, rhs);
}

// The sum over the row blocks keeps k_ei_fant_values' order and its association (bg + mean); then one addition.
__global__ __launch_bounds__(256) void k_ts_finish(const double* __restrict__ part_bgS, const double* __restrict__ htab,
                                                   const double* __restrict__ prior /*[H][S][Mp]*/, int nrb, int Mc, int nh, int S,
                                                   int64_t c0, int64_t M, int64_t Mp, int h0, double* __restrict__ path /*[H][S][Mp]*/)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y / S, sidx = blockIdx.y - h * S;
    if (c >= Mc || c0 + c >= M) return;
    const double mean = htab[h * SPX_HT + 0];
    double bg = 0.0;
    for (int ib = 0; ib < nrb; ++ib) {
        const size_t o0 = ((((size_t)ib * 2 + 0) * nh + h) * S + sidx) * Mc + c;
        const size_t o1 = ((((size_t)ib * 2 + 1) * nh + h) * S + sidx) * Mc + c;
        bg += part_bgS[o0] + part_bgS[o1];
    }
    const size_t o = ((size_t)(h0 + h) * S + sidx) * Mp + c0 + c;
    path[o] = (bg + mean) + prior[o];
}

void launch_ts_finish(hipStream_t s, const double* part_bgS, const double* htab, const double* prior, int nrb, int Mc, int nh,
                      int S, int64_t c0, int64_t M, int64_t Mp, int h0, double* path)
{
    hipLaunchKernelGGL(k_ts_finish, dim3((Mc + 255) / 256, nh * S), dim3(256), 0, s, part_bgS, htab, prior, nrb, Mc, nh, S, c0, M,
                       Mp, h0, path);
}

// numpy's argmin: the first NaN wins; otherwise the first minimum (an index < 0: nothing yet)
__device__ __forceinline__ bool ts_better(double av, int64_t ai, double bv, int64_t bi)
{
    if (bi < 0) return ai >= 0;
    if (ai < 0) return false;
    const bool an = (av != av), bn = (bv != bv);
    if (an || bn) {
        if (an && bn) return ai < bi;
        return an;
    }
    if (av < bv) return true;
    if (av > bv) return false;
    return ai < bi;
}

__device__ __forceinline__ void ts_block_argmin(double& v, int64_t& idx)
{
    __shared__ double sv[256];
    __shared__ int64_t si[256];
    sv[threadIdx.x] = v;
    si[threadIdx.x] = idx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            if (ts_better(sv[threadIdx.x + s], si[threadIdx.x + s], sv[threadIdx.x], si[threadIdx.x])) {
                sv[threadIdx.x] = sv[threadIdx.x + s];
                si[threadIdx.x] = si[threadIdx.x + s];
            }
        }
        __syncthreads();
    }
    v = sv[0];
    idx = si[0];
}

#define TS_ARGMIN_BLOCKS 64
int ts_argmin_blocks(int64_t M)
{
    const int64_t b = (M + 255) / 256;
    return (int)(b < TS_ARGMIN_BLOCKS ? b : TS_ARGMIN_BLOCKS);
}

// stage 1 (nb = gridDim.x > 1 blocks per path): partial winners into bv / bi [paths][nb];  stage 2 (`bv` given as input,
// one block per path): the winner over them into out_val / out_idx [paths], index_base added
__global__ __launch_bounds__(256) void k_ts_argmin(const double* __restrict__ path, int64_t M, int64_t Mp, const double* __restrict__ bv_in,
                                                   const int64_t* __restrict__ bi_in, int nb_in, double* __restrict__ bv,
                                                   int64_t* __restrict__ bi, int64_t index_base)
{
    const int p = blockIdx.y;
    double best = 0.0;
    int64_t besti = -1;
    if (bv_in) {
        for (int i = threadIdx.x; i < nb_in; i += 256) {
            const double v = bv_in[(size_t)p * nb_in + i];
            const int64_t j = bi_in[(size_t)p * nb_in + i];
            if (ts_better(v, j, best, besti)) { best = v; besti = j; }
        }
    } else {
        const double* row = path + (size_t)p * Mp;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
            const double v = row[i];
            if (ts_better(v, i, best, besti)) { best = v; besti = i; }
        }
    }
    ts_block_argmin(best, besti);
    if (threadIdx.x == 0) {
        bv[(size_t)p * gridDim.x + blockIdx.x] = best;
        bi[(size_t)p * gridDim.x + blockIdx.x] = bv_in ? besti + index_base : besti;
    }
}

void launch_ts_argmin(hipStream_t s, const double* path, int64_t M, int64_t Mp, int npaths, double* blk_val, int64_t* blk_idx,
                      double* out_val, int64_t* out_idx, int64_t index_base)
{
    const int nb = ts_argmin_blocks(M);
    hipLaunchKernelGGL(k_ts_argmin, dim3(nb, npaths), dim3(256), 0, s, path, M, Mp, (const double*)nullptr, (const int64_t*)nullptr, 0,
                       blk_val, blk_idx, (int64_t)0);
    hipLaunchKernelGGL(k_ts_argmin, dim3(1, npaths), dim3(256), 0, s, path, M, Mp, (const double*)blk_val, (const int64_t*)blk_idx, nb,
                       out_val, out_idx, index_base);
}
