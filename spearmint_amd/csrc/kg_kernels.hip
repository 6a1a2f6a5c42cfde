// Knowledge gradient (spx.h SPX_ACQ_KG) behind the pass's S > 0 GEMM branch with S = A + 1 right-hand sides per draw: column 0 the
// ordinary gamma, column a + 1 Gamma_a = L^-1 k(X, a) of representer point a.
//   k_kg_mu      mu_a = mean + sum_i Gamma_a[i] gamma[i] per (draw, point), once per pass
//   k_kg_lines   one thread per (candidate of the chunk, draw of the group, column): func_m / func_v and the slope func_v / s_c of
//                line 0, C(c, a) = amp2 k(c, a) - q(c, a) and the slope C / s_c of line a, s_c = sqrt(func_v + noise); the sums
//                over the row blocks keep k_ei_fant_values' order.  func_v + noise not > 0: every slope of (d, c) is NaN
//   k_kg_value   a workgroup takes TC candidates of one draw, TC the largest power of two with n TC <= KG_SLOTS (at most 256): the
//                slopes go through LDS as [line][candidate], the intercepts of the representer points once per workgroup, and
//                every (line, candidate) is a work item of its own in both sweeps of kg_device.h -- each walks the n lines of its
//                candidate in LDS, lanes of one wave reading consecutive candidates (no bank conflict) or the same word
//                (broadcast).  The terms go back through LDS and one thread per candidate adds them in the order of the lines.
// Operations per (draw, candidate) as built: n^2 fp64 divisions (sweep 1: one per ordered pair of lines of different slope, each
// with two subtractions and two compare-selects), n^2 compare-selects (sweep 2), one division and one f -- erfc, exp, about 120
// fp64 instructions -- per envelope line, n additions.  A division is the expensive part: v_div_scale x 2, v_rcp, 5 x v_fma,
// v_div_fmas, v_div_fixup, about 11 issue slots of the fp64 VALU (4 cycles per wave each).  So sweep 1 bounds the kernel at
//     n^2 x 16 instructions x 4 cycles / 64 lanes = n^2 cycles of one SIMD per (draw, candidate),
// 1024 SIMDs at 2.4 GHz: M H n^2 / 2.46e12 s -- 0.34 ms for 20 000 x 10 at A = 64, 6.9 ms for 200 000 x 20.
// Measured (profiles/kg_time.jsonl, stage "kg"): 3.8 x that at C2, 6.0 x at C3 -- the count leaves out the two LDS reads per pair,
// the select chains, sweep 2, the divergence around f, the strided staging of the slopes, and the last round of a tile that is
// not a multiple of 256 work items (n = 65: 1040 = 4.06 rounds, the fifth with 16 threads).
// No atomics, no scratch (profiles/kg_kernel_regs.txt), 39 KB of static LDS: four workgroups per CU.
#include "common.h"
#include "kg_device.h"

#define KG_SLOTS 2048      // (line, candidate) pairs of a workgroup's tile: 2 x 16 KiB of LDS for slopes and terms

// one wave per (point a, draw d): partial sums over i = lane, lane + 64, ... in that order, then the butterfly over the lanes
__global__ __launch_bounds__(64) void k_kg_mu(const double* __restrict__ gammaS /*[H][S][Np]*/, const double* __restrict__ htab, int Np, int S,
                                              double* __restrict__ mua /*[H][S - 1]*/)
{
#pragma clang fp contract(off)
    const int a = blockIdx.x, d = blockIdx.y, lane = threadIdx.x;
    const double* g0 = gammaS + (size_t)d * S * Np;
    const double* ga = g0 + (size_t)(a + 1) * Np;
    double acc = 0.0;
    for (int i = lane; i < Np; i += 64) acc = acc + ga[i] * g0[i];
    for (int m = 32; m > 0; m >>= 1) acc = acc + __shfl_xor(acc, m);
    if (lane == 0) mua[(size_t)d * (S - 1) + a] = acc + htab[d * SPX_HT + 0];
}

void launch_kg_mu(hipStream_t s, const double* gammaS, const double* htab, int Np, int S, int H, double* mua)
{
    hipLaunchKernelGGL(k_kg_mu, dim3(S - 1, H), dim3(64), 0, s, gammaS, htab, Np, S, mua);
}

__global__ __launch_bounds__(256) void k_kg_lines(const double* __restrict__ part_ss, const double* __restrict__ part_bgS,
                                                  const double* __restrict__ htab, const double* __restrict__ Kac /*[nh][Ap][Mc]*/,
                                                  int nrb, int Mc, int nh, int S, int Ap, int64_t c0, int64_t M, int64_t Mp, int h0,
                                                  double* __restrict__ slope /*[nh][S][Mc]*/, double* __restrict__ muc /*[nh][Mc]*/,
                                                  double* __restrict__ mom_m, double* __restrict__ mom_v,
                                                  double* __restrict__ cov /*[H][S - 1][Mp] or null*/)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y / S, sidx = blockIdx.y - h * S;
    if (c >= Mc || c0 + c >= M) return;
    double ss = 0.0;
    for (int ib = 0; ib < nrb; ++ib) ss += part_ss[((size_t)ib * nh + h) * Mc + c];
    const double func_v = htab[h * SPX_HT + 3] - ss;
    double bg = 0.0;
    for (int ib = 0; ib < nrb; ++ib) {
        const size_t o0 = ((((size_t)ib * 2 + 0) * nh + h) * S + sidx) * Mc + c;
        const size_t o1 = ((((size_t)ib * 2 + 1) * nh + h) * S + sidx) * Mc + c;
        bg += part_bgS[o0] + part_bgS[o1];
    }
    const double vs = func_v + htab[h * SPX_HT + 1];      // the variance of a new observation at c
    const double sc = sqrt(vs);
    double sl;
    if (sidx == 0) {
        const double func_m = bg + htab[h * SPX_HT + 0];
        muc[(size_t)h * Mc + c] = func_m;
        sl = func_v / sc;
        if (mom_m) {
            const size_t o = (size_t)(h0 + h) * Mp + c0 + c;
            mom_m[o] = func_m;
            mom_v[o] = func_v;
        }
    } else {
        const double C = Kac[((size_t)h * Ap + (sidx - 1)) * Mc + c] - bg;
        sl = C / sc;
        if (cov) cov[((size_t)(h0 + h) * (S - 1) + (sidx - 1)) * Mp + c0 + c] = C;
    }
    slope[((size_t)h * S + sidx) * Mc + c] = (vs > 0.0) ? sl : __builtin_nan("");
}

void launch_kg_lines(hipStream_t s, const double* part_ss, const double* part_bgS, const double* htab, const double* Kac, int nrb,
                     int Mc, int nh, int S, int Ap, int64_t c0, int64_t M, int64_t Mp, int h0, double* slope, double* muc,
                     double* mom_m, double* mom_v, double* cov)
{
    hipLaunchKernelGGL(k_kg_lines, dim3((Mc + 255) / 256, nh * S), dim3(256), 0, s, part_ss, part_bgS, htab, Kac, nrb, Mc, nh, S, Ap,
                       c0, M, Mp, h0, slope, muc, mom_m, mom_v, cov);
}

__global__ __launch_bounds__(256) void k_kg_value(const double* __restrict__ slope /*[nh][n][Mc]*/, const double* __restrict__ muc /*[nh][Mc]*/,
                                                  const double* __restrict__ mua /*[nh][n - 1]*/, int Mc, int n, int TC, int64_t c0,
                                                  int64_t M, int64_t Mp, int h0, double* __restrict__ ei_draw)
{
#pragma clang fp contract(off)
    __shared__ double s_b[KG_SLOTS], s_t[KG_SLOTS], s_a[256], s_a0[256];
    __shared__ unsigned char s_on[KG_SLOTS];
    __shared__ int s_bad[256];
    const int tid = threadIdx.x, h = blockIdx.y;
    const int cbase = blockIdx.x * TC;
    if (cbase >= Mc || c0 + cbase >= M) return;            // (the whole workgroup: before any barrier)
    const int nslots = n * TC;                             // <= KG_SLOTS
    const int tsh = 31 - __builtin_clz(TC);                // (TC is a power of two)
    // a candidate of the tile beyond the chunk or beyond M: zero lines, computed like the others, never stored
    for (int idx = tid; idx < nslots; idx += 256) {
        const int i = idx >> tsh, ct = idx & (TC - 1), c = cbase + ct;
        s_b[idx] = (c < Mc && c0 + c < M) ? slope[((size_t)h * n + i) * Mc + c] : 0.0;
    }
    for (int i = tid; i < n; i += 256) s_a[i] = i ? mua[(size_t)h * (n - 1) + (i - 1)] : 0.0;
    if (tid < TC) {
        const int c = cbase + tid;
        s_a0[tid] = (c < Mc && c0 + c < M) ? muc[(size_t)h * Mc + c] : 0.0;
        s_bad[tid] = 0;
    }
    __syncthreads();
    for (int idx = tid; idx < nslots; idx += 256) {
        const int i = idx >> tsh, ct = idx & (TC - 1);
        const double ai = i ? s_a[i] : s_a0[ct], bi = s_b[idx];
        if (!(fabs(ai) <= 1.79769313486231570815e308) || !(fabs(bi) <= 1.79769313486231570815e308)) s_bad[ct] = 1;
        s_on[idx] = kg_on_envelope(s_a0[ct], s_a, s_b + ct, TC, n, i) ? 1 : 0;
    }
    __syncthreads();
    for (int idx = tid; idx < nslots; idx += 256) {
        const int i = idx >> tsh, ct = idx & (TC - 1);
        s_t[idx] = s_on[idx] ? kg_term(s_a0[ct], s_a, s_b + ct, TC, s_on + ct, TC, n, i) : 0.0;
    }
    __syncthreads();
    if (tid < TC) {
        const int c = cbase + tid;
        if (c < Mc && c0 + c < M) {
            double acc = 0.0;
            for (int i = 0; i < n; ++i) acc = acc + s_t[i * TC + tid];
            ei_draw[(size_t)(h0 + h) * Mp + c0 + c] = s_bad[tid] ? __builtin_nan("") : acc;
        }
    }
}

// the candidates of a workgroup's tile: the largest power of two with n TC <= KG_SLOTS, at most 256
int kg_tile_candidates(int n)
{
    int tc = 256;
    while (tc > 1 && n * tc > KG_SLOTS) tc >>= 1;
    return tc;
}

void launch_kg_value(hipStream_t s, const double* slope, const double* muc, const double* mua, int Mc, int nh, int n, int64_t c0,
                     int64_t M, int64_t Mp, int h0, double* ei_draw)
{
    const int TC = kg_tile_candidates(n);
    hipLaunchKernelGGL(k_kg_value, dim3((Mc + TC - 1) / TC, nh), dim3(256), 0, s, slope, muc, mua, Mc, n, TC, c0, M, Mp, h0, ei_draw);
}
