// Pending-experiment fantasies formed on the device (spx_draw_fantasies; GPEIChooser.py:219-249).
//
// With the P pending points last, the factor of cov([comp; pend]) + noise I is L = [[L_A, 0], [L21, L_S]], and
//   pend_m = L21 gamma[:N] + mean,   pend_K = L_S L_S^T - noise I,   C = chol(pend_K),   pend_fant_s = C z_s + pend_m.
// Gamma_s = L^-1 (F_s - mean) with F_s = [vals; pend_fant_s]: L is lower triangular, so rows < N are gamma[:N] whatever
// the fantasy, and rows N..n are L_S^-1 (pend_fant_s - mean - L21 gamma[:N]) = (L_S^-1 C) z_s = T z_s.
//
//   k_fant_posterior  one workgroup per draw: pend_m, np.min(vals[:N]), pend_K and C in LDS, T = L_S^-1 C
//   k_fant_fill       (16 fantasy columns, draw) per workgroup: pend_fant, bests, Gamma in the layout of launch_gamma_multi
//
// No contraction in this file: a rounding happens where it is written (fma() where one fused step is meant).
#include "common.h"
#pragma clang fp contract(off)

// offset of element (i, j), j <= i, of one draw's factor: tile-major (k_lean_flow; spx_api.hip: tile_elem) or row-major
template <bool TILED>
__device__ __forceinline__ size_t fant_l_off(int Np, int i, int j)
{
    if (!TILED) return (size_t)i * Np + j;
    const int I = i >> 6, J = j >> 6, ri = i & 63, cj = j & 63;
    const size_t base = ((size_t)I * (Np >> 6) + J) * 4096;
    if (I == J) return base + ri * 64 + cj;
    const int t = (ri >> 4) * 64 + (ri & 3) * 16 + (cj & 15), q = (cj >> 4) * 4 + ((ri & 15) >> 2);
    return base + ((size_t)((q >> 1) * 256 + t)) * 2 + (q & 1);
}

// np.min's rule for two partial results: a NaN wins
__device__ __forceinline__ double fant_npmin(double a, double b)
{
    return (a != a) ? a : ((b != b) ? b : (b < a ? b : a));
}

// post (per draw, stride 2 P^2 + P + 1): C [P][P] | T [P][P] | pend_m [P] | np.min(vals[:N]);  info[d] = 1 + first failing pivot, or 0
template <bool TILED>
__global__ __launch_bounds__(256) void k_fant_posterior(const double* __restrict__ Lm, const double* __restrict__ gamma,
                                                        const double* __restrict__ htab, const double* __restrict__ vals,
                                                        double* __restrict__ post, int* __restrict__ info, int N, int P, int Np)
{
    extern __shared__ double fant_sm[];
    __shared__ double red[256];
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = P | 1, PP = P * P;
    double* LS = fant_sm;               // [P][ld]  trailing P x P block of the factor
    double* C = fant_sm + P * ld;       // [P][ld]  pend_K, then its factor, then T (lower triangles)
    const double* L = Lm + (size_t)d * Np * Np;
    const double* g = gamma + (size_t)d * Np;
    const double mean = htab[d * SPX_HT + 0], noise = htab[d * SPX_HT + 1];
    double* pd = post + (size_t)d * (2 * PP + P + 1);

    // pend_m[p] = sum_j L21[p][j] gamma[j] + mean: one wavefront per row, 64 partial sums, a butterfly
    for (int p = wave; p < P; p += 4) {
        double acc = 0.0;
        for (int j = lane; j < N; j += 64) acc = fma(L[fant_l_off<TILED>(Np, N + p, j)], g[j], acc);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) pd[2 * PP + p] = acc + mean;
    }
    for (int idx = tid; idx < PP; idx += 256) {
        const int p = idx / P, q = idx - p * P;
        LS[p * ld + q] = q <= p ? L[fant_l_off<TILED>(Np, N + p, N + q)] : 0.0;
    }
    // np.min(vals[:N])
    double m = __builtin_inf();
    for (int i = tid; i < N; i += 256) m = fant_npmin(m, vals[i]);
    red[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fant_npmin(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) pd[2 * PP + P] = red[0];
    // pend_K = L_S L_S^T - noise I: the product rounded, then the subtraction
    for (int idx = tid; idx < PP; idx += 256) {
        const int p = idx / P, q = idx - p * P;
        if (q > p) continue;
        double acc = 0.0;
        for (int k = 0; k <= q; ++k) acc = fma(LS[p * ld + k], LS[q * ld + k], acc);
        C[p * ld + q] = p == q ? acc - noise : acc;
    }
    __syncthreads();
    // left-looking Cholesky; every thread forms the pivot itself, so the verdict needs no broadcast
    int bad = 0;
    for (int j = 0; j < P; ++j) {
        double piv = C[j * ld + j];
        for (int k = 0; k < j; ++k) piv = fma(-C[j * ld + k], C[j * ld + k], piv);
        if (!(piv > 0.0)) { bad = j + 1; break; }
        const double r = sqrt(piv);
        __syncthreads();                 // (everyone has read C[j][j])
        if (tid == 0) C[j * ld + j] = r;
        for (int i = j + 1 + tid; i < P; i += 256) {
            double s = C[i * ld + j];
            for (int k = 0; k < j; ++k) s = fma(-C[i * ld + k], C[j * ld + k], s);
            C[i * ld + j] = s / r;
        }
        __syncthreads();
    }
    if (tid == 0) info[d] = bad;
    if (bad) return;
    for (int idx = tid; idx < PP; idx += 256) {
        const int p = idx / P, q = idx - p * P;
        pd[idx] = q <= p ? C[p * ld + q] : 0.0;
    }
    __syncthreads();
    // T = L_S^-1 C, column j in place by thread j
    if (tid < P) {
        const int j = tid;
        for (int i = j; i < P; ++i) {
            double s = C[i * ld + j];
            for (int k = j; k < i; ++k) s = fma(-LS[i * ld + k], C[k * ld + j], s);
            C[i * ld + j] = s / LS[i * ld + i];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < PP; idx += 256) {
        const int p = idx / P, q = idx - p * P;
        pd[PP + idx] = q <= p ? C[p * ld + q] : 0.0;
    }
}

#define FANT_COLS 16   // fantasy columns per workgroup of k_fant_fill
// z: [P][S] of this draw at z + d * z_stride (z_stride = 0: one array for every draw).  A column's values depend on
// nothing but that column of z: one thread forms it, in the order q = 0, 1, ...
__global__ __launch_bounds__(256) void k_fant_fill(const double* __restrict__ post, const double* __restrict__ z, size_t z_stride,
                                                   const double* __restrict__ gamma, double* __restrict__ gammaS,
                                                   double* __restrict__ bests, double* __restrict__ pend_fant,
                                                   int N, int P, int Np, int S)
{
    const int d = blockIdx.y, tid = threadIdx.x, s0 = blockIdx.x * FANT_COLS;
    const int PP = P * P;
    const double* pd = post + (size_t)d * (2 * PP + P + 1);
    if (tid < FANT_COLS && s0 + tid < S) {
        const int s = s0 + tid;
        const double* zd = z + (size_t)d * z_stride + s;
        double* gs = gammaS + ((size_t)d * S + s) * Np + N;
        double b = pd[2 * PP + P];
        for (int p = 0; p < P; ++p) {
            double a = 0.0, t = 0.0;
            for (int q = 0; q <= p; ++q) {
                const double zq = zd[(size_t)q * S];
                a = fma(pd[p * P + q], zq, a);
                t = fma(pd[PP + p * P + q], zq, t);
            }
            const double f = a + pd[2 * PP + p];
            pend_fant[((size_t)d * P + p) * S + s] = f;
            gs[p] = t;
            b = fant_npmin(b, f);
        }
        bests[(size_t)d * S + s] = b;
    }
    // rows < N of every column are gamma[:N]; pad rows are zero (what k_gamma computes there for finite values)
    const double* g = gamma + (size_t)d * Np;
    const int ncol = min(FANT_COLS, S - s0);
    for (int c = 0; c < ncol; ++c) {
        double* dst = gammaS + ((size_t)d * S + s0 + c) * Np;
        for (int i = tid; i < N; i += 256) dst[i] = g[i];
        for (int i = N + P + tid; i < Np; i += 256) dst[i] = 0.0;
    }
}

size_t fant_post_stride(int P) { return (size_t)2 * P * P + P + 1; }

void launch_fant_posterior(hipStream_t s, const double* Lm, bool tiled, const double* gamma, const double* htab,
                           const double* vals, double* post, int* info, int N, int P, int Np, int H)
{
    const size_t lds = (size_t)2 * P * (P | 1) * sizeof(double);
    if (tiled) {
        SPX_LDS_ATTR((k_fant_posterior<true>), lds);
        hipLaunchKernelGGL(k_fant_posterior<true>, dim3(H), dim3(256), lds, s, Lm, gamma, htab, vals, post, info, N, P, Np);
    } else {
        SPX_LDS_ATTR((k_fant_posterior<false>), lds);
        hipLaunchKernelGGL(k_fant_posterior<false>, dim3(H), dim3(256), lds, s, Lm, gamma, htab, vals, post, info, N, P, Np);
    }
}

void launch_fant_fill(hipStream_t s, const double* post, const double* z, size_t z_stride, const double* gamma,
                      double* gammaS, double* bests, double* pend_fant, int N, int P, int Np, int S, int H)
{
    hipLaunchKernelGGL(k_fant_fill, dim3((S + FANT_COLS - 1) / FANT_COLS, H), dim3(256), 0, s, post, z, z_stride, gamma,
                       gammaS, bests, pend_fant, N, P, Np, S);
}
