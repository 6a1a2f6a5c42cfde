// Value and gradient of posterior sample paths at arbitrary points (spx.h: spx_thompson_grad_batch).  A path is a closed-form
// function, f(x) = mean + p(x) + k(x, X)' alpha with alpha = W^T Gamma cached per path, so a point costs no pass over W:
//   k_ts_grad_prior    p_{d,s}(x) and its gradient for a tile of 16 points per wave, every point under a path of its own.  The
//                      features are k_ts_prior's, operation for operation: the dot products over K = Dp on the fp64 MFMA, the
//                      phase, r = u - rint(u), cos2pi.  The contraction with the weights feeds "row i = weights of point i's
//                      path" as the A operand and reads the DIAGONAL of the 16 x 16 result: an MFMA output element depends on
//                      its A row and its B column alone, so point i's number is the one k_ts_prior gives a row with these
//                      coordinates under that path, bit for bit.  The gradient is a second contraction, over the features:
//                      gp[j] = -(scale_d TWO_PI) sum_f nu[d][f][j] (w[s][f] sin2pi(r_f)), the (w sin) tile as the B operand
//                      against the frequency tile, which is in operand order already (read transposed: ts_nu_index).  The
//                      frequencies belong to a draw, so a wave walks the draws its 16 points name, one after the other (one
//                      draw: one walk), and every point keeps the columns of its own draw.
//   k_ts_grad_update   one workgroup per point: k_j and dk/dr^2 as k_point_cov forms them (refine_kernels.hip: the expanded r^2,
//                      the clamp, the three correlation kinds), m = sum_j k_j alpha_j, the TRUE partial derivatives
//                      gu[j'] = amp2 sum_j alpha_j dk_j/dr^2 2 (x_j'/ls_j' - X_jj'/ls_j') / ls_j' -- no factor one half: a path
//                      is not an acquisition of the reference and inherits no scaling -- and the combine
//                      value = (m + mean_d) + prior, grad[j] = gu[j] + gp[j], one rounding each.
// Sign convention: grad is d value / d x, the direction in which the path RISES; a minimiser of the path (L-BFGS-B) takes
// (value, grad) as they are.  tests/test_gpu_zu_thompson_grad.py holds it to central differences of the value.
// Every point is computed by its own lanes (prior) and its own workgroup (update) in a fixed order: its numbers do not depend
// on P, on its position, on the other points' paths or on how many paths and draws are resident.
//
// Operation counts.  Prior, per tile of 16 points x 16 features and per draw walked: Dp / 4 MFMAs (dot products) + 4 (weights)
// + 4 per 16 dimensions (gradient), and per value 3 (phase, rint, difference) + 13 (cos2pi) + 14 (sin2pi, which shares
// nothing with the cosine but its argument) + 1 (w sin) = 31 fp64 VALU operations.  By ts_kernels.hip's FMA-unit argument (an
// MFMA holds the unit 64 cycles, a VALU instruction 4) a tile costs 64 (Dp / 4 + 4 + 4 ceil(Dp / 16)) + 4 * 4 * 31 cycles of one
// SIMD: 1136 at Dp = 8, so 16 points x F = 1024 features are 73 000 cycles, 30 us at 2.4 GHz -- per WAVE, and 20 points are two
// waves: the kernel is latency, not throughput (README.md has the measurement).  Update, per point: N rows of Dp doubles read
// once per 8 dimensions, N (2 D + 12) flops and one exp per row.
// No kernel here uses scratch: every register array is indexed by unrolled loops (profiles/ts_grad_kernel_regs.txt).
#include "common.h"
#include "ts_device.h"

#define TSG_SQRT5 2.23606797749978969641
#define TSG_SQRT3 1.73205080756887719318
#define TSG_GD 8      // dimensions per gradient pass of the update kernel

// KQ = Dp / 4 K steps with the points' operand held in registers (Dp <= 32); KQ = 0: any Dp, the operand re-read per feature
// tile -- k_ts_prior's two forms, with the same summation order.  GT: tiles of 16 dimensions of the gradient per walk over
// the features (Dp > 16 GT: the walk is repeated for the next 16 GT dimensions)
template <int KQ, int GT>
__global__ __launch_bounds__(256) void k_ts_grad_prior(const double* __restrict__ x /*[P][D]*/, const int32_t* __restrict__ path_of /*[P] or null*/,
                                                       int P, int D, int Dp, const double* __restrict__ nu /*[H][F / 16][Dp / 4][64]*/,
                                                       const double* __restrict__ phase /*[F]*/, const double* __restrict__ w /*[H or 1][S][F]*/,
                                                       size_t w_stride, const double* __restrict__ scale /*[H]*/, int F, int S, int H,
                                                       double* __restrict__ prior /*[P]*/, double* __restrict__ gp /*[P][D]*/)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int pbase = (blockIdx.x * 4 + wave) * 16;
    if (pbase >= P) return;                       // (whole wave: no barrier in this kernel)
    const int pt = pbase + li;                    // this lane's point: B column li of every MFMA
    const bool live = pt < P;
    const int path = (live && path_of) ? path_of[pt] : 0;
    const int pd = path / S, ps = path - pd * S;  // its draw and its path under that draw
    constexpr int NQ = KQ > 0 ? KQ : 1;
    const int nq = KQ > 0 ? KQ : Dp / 4;

    // B operand of the dot products: lane (li, g) supplies x[point li of the tile][dimension 4 q + g]; zeros beyond P and D
    double xb[NQ];
    if (KQ > 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int k = 4 * q + g;
            xb[q] = (live && k < D) ? x[(size_t)pt * D + k] : 0.0;
        }
    }
    for (int d = 0; d < H; ++d) {
        if (__ballot(live && pd == d) == 0) continue;          // no point of this tile lives under draw d (wave-uniform)
        const double* nud = nu + (size_t)d * F * Dp;
        // the weights this lane supplies: those of ITS point's path if the point lives under draw d, else path 0 of draw d (a
        // row and a column that are never read)
        const bool mine = live && pd == d;
        const double* wrow = w + (size_t)d * w_stride + (size_t)(mine ? ps : 0) * F;
        const double sc = scale[d];
        const double gsc = sc * SPX_TS_TWO_PI;
        for (int j0 = 0; j0 < Dp; j0 += 16 * GT) {
            d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
            d4 gacc[GT];
#pragma unroll
            for (int t = 0; t < GT; ++t) gacc[t] = (d4){0.0, 0.0, 0.0, 0.0};
            for (int f0 = 0; f0 < F; f0 += 16) {
                // accumulator register r of lane (li, g) is feature f0 + 4 g + r of point li (ts_kernels.hip)
                double ph[4], wa[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) ph[r] = phase[f0 + 4 * g + r];
#pragma unroll
                for (int r = 0; r < 4; ++r) wa[r] = wrow[f0 + 4 * g + r];
                const double* tile = nud + (size_t)(f0 / 16) * nq * 64;
                const double* pa = tile + lane;                    // A operand of the dot products, K step q at pa[64 q]
                d4 u = (d4){0.0, 0.0, 0.0, 0.0};
                if (KQ > 0) {
                    double af[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) af[q] = pa[64 * q];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) u = MFMA_F64(af[q], xb[q], u);
                } else {
                    for (int q = 0; q < nq; ++q) {
                        const double af = pa[64 * q];
                        const int k = 4 * q + g;
                        const double xv = (live && k < D) ? x[(size_t)pt * D + k] : 0.0;
                        u = MFMA_F64(af, xv, u);
                    }
                }
                double rr[4], c[4], sn[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double uu = u[r] + ph[r];
                    rr[r] = uu - __builtin_rint(uu);
                }
                cos2pi<4>(rr, c);
                sin2pi<4>(rr, sn);
                // A row li = the weights of point li's path, B column li = point li's cosines: the diagonal is the prior
#pragma unroll
                for (int r = 0; r < 4; ++r) acc = MFMA_F64(wa[r], c[r], acc);
                // gradient: A[dimension j0 + 16 t + li][K step r: feature f0 + 4 g + r] = nu of that feature and dimension, read
                // out of the operand-order tile (ts_nu_index: tile row of feature 4 g + r is 4 r + g); B = w sin of point li
                double ws[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) ws[r] = wa[r] * sn[r];
#pragma unroll
                for (int t = 0; t < GT; ++t) {
                    const int j = j0 + 16 * t + li;
                    const double* pt_nu = tile + (size_t)(j / 4) * 64 + (size_t)(j % 4) * 16 + g;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double an = j < Dp ? pt_nu[4 * r] : 0.0;
                        gacc[t] = MFMA_F64(an, ws[r], gacc[t]);
                    }
                }
            }
            // prior: element (row li, column li) sits in register li / 4 of lane (li, g = li % 4)
            if (j0 == 0 && mine && g == (li & 3)) {
                double v = acc[0];
#pragma unroll
                for (int r = 1; r < 4; ++r)
                    if ((li >> 2) == r) v = acc[r];
                prior[pt] = sc * v;
            }
            // gradient: register r of lane (li, g) is dimension j0 + 16 t + g + 4 r of point li
            if (mine) {
#pragma unroll
                for (int t = 0; t < GT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = j0 + 16 * t + g + 4 * r;
                        if (j < D) gp[(size_t)pt * D + j] = -gsc * gacc[t][r];
                    }
            }
        }
    }
}

void launch_ts_grad_prior(hipStream_t s, const double* x, const int32_t* path_of, int P, int D, int Dp, const double* nu,
                          const double* phase, const double* w, size_t w_stride, const double* scale, int F, int S, int H,
                          double* prior, double* gp)
{
    const dim3 grid((unsigned)((P + 63) / 64));
#define SPX_TSG(KQ_, GT_)                                                                                                  \
    hipLaunchKernelGGL((k_ts_grad_prior<KQ_, GT_>), grid, dim3(256), 0, s, x, path_of, P, D, Dp, nu, phase, w, w_stride, scale, F, \
                       S, H, prior, gp)
    if (Dp == 4) SPX_TSG(1, 1);
    else if (Dp == 8) SPX_TSG(2, 1);
    else if (Dp == 16) SPX_TSG(4, 1);
    else if (Dp == 32) SPX_TSG(8, 2);
    else SPX_TSG(0, 2);
#undef SPX_TSG
}

// sum over the 256 threads of a workgroup in the fixed order of refine_kernels.hip's block_sum; every thread gets the result
__device__ __forceinline__ double tsg_block_sum(double v, double* red /*[4]*/)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// out[p] = {value, prior, grad[D]}.  Xs, s1: the factor's scaled rows and their squared norms; hyp: the length scales the
// points are scaled by (unit ones under SE, as everywhere); dkw [P][Np]: each thread's own dk/dr^2 between its two passes
__global__ __launch_bounds__(256) void k_ts_grad_update(const double* __restrict__ Xs /*[H][Np][Dp]*/, const double* __restrict__ s1 /*[H][Np]*/,
                                                        const double* __restrict__ hyp /*[H][3 + D]*/, const double* __restrict__ htab,
                                                        const double* __restrict__ alpha /*[H S][Np]*/, const double* __restrict__ x /*[P][D]*/,
                                                        const int32_t* __restrict__ path_of, const double* __restrict__ prior /*[P]*/,
                                                        const double* __restrict__ gp /*[P][D]*/, double* __restrict__ dkw,
                                                        double* __restrict__ out /*[P][2 + D]*/, int N, int Np, int D, int Dp, int S,
                                                        int kind)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    __shared__ double redv[4][TSG_GD];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int path = path_of ? path_of[p] : 0;
    const int h = path / S;
    const double* ls = hyp + (size_t)h * (3 + D) + 3;
    const double* xp = x + (size_t)p * D;
    const double* Xh = Xs + (size_t)h * Np * Dp;
    const double* s1h = s1 + (size_t)h * Np;
    const double* ap = alpha + (size_t)path * Np;
    double* dk = dkw + (size_t)p * Np;
    const double mean = htab[h * SPX_HT + 0], amp2 = htab[h * SPX_HT + 2];
    double* o = out + (size_t)p * (2 + D);

    // m = sum_j k_j alpha_j: k as k_point_cov forms it
    double mv = 0.0;
    for (int j = tid; j < N; j += 256) {
        const double* xj = Xh + (size_t)j * Dp;
        double gg = 0.0, s2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double xc = xp[d] / ls[d];
            gg = gg + xj[d] * (2.0 * xc);
            s2 = s2 + xc * xc;
        }
        const double t = (gg - s1h[j]) - s2;
        const double nt = -t;
        double r2 = (nt < 0.0) ? 0.0 : nt;
        r2 = fabs(r2);
        const double r = sqrt(r2);
        double kv, dv;
        if (kind == SPX_COV_MATERN52) {
            const double e = exp(-TSG_SQRT5 * r);
            kv = amp2 * (((1.0 + TSG_SQRT5 * r) + (5.0 / 3.0) * r2) * e);
            dv = -(5.0 / 6.0) * e * (1.0 + TSG_SQRT5 * r);
        } else if (kind == SPX_COV_MATERN32) {
            const double e = exp(-TSG_SQRT3 * r);
            kv = amp2 * ((1.0 + TSG_SQRT3 * r) * e);
            dv = -1.5 * e;
        } else {
            const double e = exp(-0.5 * r2);
            kv = amp2 * e;
            dv = -0.5 * e;
        }
        dk[j] = dv;
        mv += kv * ap[j];
    }
    const double m = tsg_block_sum(mv, red);
    const double pr = prior[p];
    if (tid == 0) {
        o[0] = (m + mean) + pr;
        o[1] = pr;
    }
    // gu[j'] = amp2 sum_j alpha_j (dk_j 2 (x_j' / ls_j' - Xs_jj') / ls_j'), TSG_GD dimensions per pass over the rows
    for (int d0 = 0; d0 < D; d0 += TSG_GD) {
        const int nd = min(TSG_GD, D - d0);
        double xc[TSG_GD], il[TSG_GD], acc[TSG_GD];
#pragma unroll
        for (int q = 0; q < TSG_GD; ++q) {
            const int d = d0 + (q < nd ? q : 0);
            acc[q] = 0.0;
            xc[q] = xp[d] / ls[d];
            il[q] = 1.0 / ls[d];
        }
        for (int j = tid; j < N; j += 256) {
            const double* xr = Xh + (size_t)j * Dp + d0;
            const double dj = dk[j], aj = ap[j];
#pragma unroll
            for (int q = 0; q < TSG_GD; ++q)
                if (q < nd) {
                    const double gj = dj * (2.0 * (xc[q] - xr[q]) * il[q]);
                    acc[q] += aj * gj;
                }
        }
#pragma unroll
        for (int q = 0; q < TSG_GD; ++q) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_xor(acc[q], off);
        }
        __syncthreads();
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < TSG_GD; ++q) redv[tid >> 6][q] = acc[q];
        }
        __syncthreads();
        if (tid < nd) {
            const double sv = ((redv[0][tid] + redv[1][tid]) + redv[2][tid]) + redv[3][tid];
            const double gu = amp2 * sv;
            o[2 + d0 + tid] = gu + gp[(size_t)p * D + d0 + tid];
        }
    }
}

void launch_ts_grad_update(hipStream_t s, const double* Xs, const double* s1, const double* hyp, const double* htab,
                           const double* alpha, const double* x, const int32_t* path_of, const double* prior, const double* gp,
                           double* dkw, double* out, int N, int Np, int D, int Dp, int S, int P, int kind)
{
    hipLaunchKernelGGL(k_ts_grad_update, dim3(P), dim3(256), 0, s, Xs, s1, hyp, htab, alpha, x, path_of, prior, gp, dkw, out, N, Np, D,
                       Dp, S, kind);
}
