// Knowledge gradient by slope order and one scan (spx.h: option "kg_scan"): the plain pass of kg_kernels.hip up to and including
// its lines -- k_kg_mu, the S = A + 1 GEMM branch, k_kg_lines, nothing of them changed -- and then, in place of k_kg_value's
// all-pairs sweeps, the envelope rule of kg_fant_device.h with ONE line set per (draw, candidate), n = A + 1 up to 1024:
//   k_kgs_order   the slope order of every (d, c) of the work item.  A workgroup stages the slopes of TC candidates through LDS
//                 once, as [line][candidate] keys of 8 bytes beside the line index in 16 bits, padded to P = the next power of two
//                 with keys of -inf that follow every line, and sorts the TC sets side by side with a bitonic network under the
//                 header's order: slope falling, ties by rising index.  The order is total, so the network -- not stable by itself
//                 -- ends in the one permutation kgf_rank would count.  The sorted slopes and indices go to [d][rank][c] tables of
//                 the work item, 8 + 2 bytes per line.
//   k_kgs_value   one thread per (d, c), 256 per workgroup, lane = candidate: it walks its lines through kgf_value of
//                 kg_fant_device.h -- the scan, the stack a bit set over the ranks in LDS as [word][thread], the top of the stack
//                 in registers, then the walk over the stack for the terms.  A visit reads slope and index at [rank][c]: the
//                 lanes of a wave read consecutive addresses while they visit the same rank, which they do except inside a pop.
//                 The intercepts of the representer points are staged once per workgroup (8 A bytes) and read by index.
// Why a network and not rank counting (k_kgf_order's way).  Per (d, c), rank counting is n^2 compare-selects, each one LDS read
// of 8 bytes, two fp64 compares, a select and an add: about 5 instructions.  The network is P/2 log2 P (log2 P + 1) / 2
// compare-exchanges, each two LDS reads of 10 bytes, two fp64 compares, an index compare and two conditional writes of 10 bytes:
// about 14 instructions.
//     n = 65 (P = 128):     4 225 x 5 = 21 k     against      1 792 x 14 = 25 k     -- even
//     n = 256:             65 536 x 5 = 328 k    against      4 608 x 14 = 65 k     -- a fifth
//     n = 1024:         1 048 576 x 5 = 5.2 M    against     28 160 x 14 = 394 k    -- a thirteenth
// At n = 1024 rank counting would cost more than the all-pairs divisions it was meant to replace do at n = 256; the network is
// even where n is small and far ahead where the option is needed.  One path for every n.
// LDS.  k_kgs_order: 10 P TC + 4 TC bytes with P TC <= 4096 slots: at most 41 KB, three workgroups per CU.  k_kgs_value:
// 4 ceil(n / 32) 256 bytes of stacks + 8 A of intercepts: 1.3 KB + 0.5 KB at n = 65, 32 KB + 8 KB at n = 1024.
// fp64-VALU bound, from the kernels as built (profiles/kg_scan_kernel_regs.txt; a wave instruction of 64 lanes is 4 cycles of
// one SIMD, a division about 16 fp64 issue slots, f about 120 -- kg_kernels.hip's prices).  Per (d, c) with E lines on the
// envelope, P_ popped and d_ dropped for an equal slope the scan makes n + 2 P_ + E - 2 - d_ <= 3 n - 4 divisions and E - 1
// evaluations of f (kg_fant_kernels.hip derives it), and the network P/2 log2 P (log2 P + 1) / 2 compare-exchanges with two
// v_cmp_*_f64 each.  At n = 65, E = 8:  (65 + 114 + 8) x 16 + 7 x 120 = 3 832 slots for the scan, 1 792 x 2 = 3 584 for the
// order: 7 416 x 4 / 64 = 464 cycles of one SIMD per (d, c), so
//     M H x 464 / (1024 SIMDs x 2.4 GHz) = M H / 5.3e9 s:   C2 (20 000 x 10): 0.038 ms,   C3 (200 000 x 20): 0.76 ms
// against M H n^2 / 2.46e12 = 0.34 ms and 6.9 ms of the all-pairs rule.  At n = 1024, E = 8: 3 064 x 16 + 840 + 56 320 = 106 k
// slots = 6.6 k cycles: C2 0.54 ms.  What the count leaves out: the network's LDS traffic (20 bytes read and up to 20 written
// per compare-exchange, the fp64 compares are a seventh of its instructions) and its log2 P (log2 P + 1) / 2 barriers; the
// scan's memory reads in a dependent chain (a visit waits for its slope and index; a pop for the two lines under the top), the
// divergence of the pop loop between the candidates of a wave and around f.  Measured (profiles/kg_scan_time.jsonl, stage "kg"):
// 25 x the bound at C2 and 83 x at C3 for A = 64, 71 x at C2 for A = 1023 -- the stage waits for memory and LDS, not for the fp64
// VALU; at C3 its per-work-item launches of 112 workgroups are too few to hide a scan's chain of dependent loads (README, "KG by
// slope order and one scan").
// No atomics, no scratch.
#include "common.h"
#include "kg_fant_device.h"

#define KGS_SLOTS 4096         // (padded line, candidate) pairs of a k_kgs_order tile: 40 KB of keys and indices
#define KGS_DBL_MAX 1.79769313486231570815e308

// candidates of a k_kgs_order tile: KGS_SLOTS / P, at most 256 (P = n rounded up to a power of two, at least 2)
static int kgs_pow2(int n)
{
    int P = 2;
    while (P < n) P <<= 1;
    return P;
}
static int kgs_tile_candidates(int P) { return KGS_SLOTS / P < 256 ? KGS_SLOTS / P : 256; }

// line (bi, i) comes before line (bj, j): slope falling, ties by rising index (kgf_rank's order; a pad, -inf, follows every line)
__device__ __forceinline__ bool kgs_before(double bi, unsigned i, double bj, unsigned j) { return bi > bj || (bi == bj && i < j); }

__global__ __launch_bounds__(256) void k_kgs_order(const double* __restrict__ slope /*[nh][n][Mc]*/, int Mc, int n, int P, int TC,
                                                   int64_t c0, int64_t M, size_t orow, int64_t oc0, int oh0,
                                                   double* __restrict__ bsort /*[.][n][orow]*/,
                                                   unsigned short* __restrict__ perm /*[.][n][orow]*/)
{
    extern __shared__ double kgs_lds[];
    double* s_b = kgs_lds;                                         // [P][TC]
    int* s_bad = (int*)(s_b + (size_t)P * TC);                     // [TC]: a slope of the candidate is not finite
    unsigned short* s_i = (unsigned short*)(s_bad + TC);           // [P][TC]
    const int tid = threadIdx.x, h = blockIdx.y;
    const int cbase = blockIdx.x * TC;
    if (cbase >= Mc || c0 + cbase >= M) return;                    // (the whole workgroup: before any barrier)
    const int tsh = 31 - __builtin_clz(TC);                        // (TC is a power of two)
    const int nslots = P * TC;
    for (int t = tid; t < TC; t += 256) s_bad[t] = 0;
    __syncthreads();
    // a candidate of the tile beyond the chunk or beyond M: zero slopes, sorted like the others, never stored
    for (int idx = tid; idx < nslots; idx += 256) {
        const int k = idx >> tsh, ct = idx & (TC - 1), c = cbase + ct;
        double b = -__builtin_inf();
        if (k < n) {
            b = (c < Mc && c0 + c < M) ? slope[((size_t)h * n + k) * Mc + c] : 0.0;
            if (!(fabs(b) <= KGS_DBL_MAX)) s_bad[ct] = 1;
        }
        s_b[idx] = b;
        s_i[idx] = (unsigned short)k;
    }
    __syncthreads();
    // a candidate with a non-finite slope keeps the order of its lines (zero keys: the index decides) and is written as NaN
    for (int idx = tid; idx < n * TC; idx += 256)
        if (s_bad[idx & (TC - 1)]) s_b[idx] = 0.0;
    __syncthreads();
    const int npairs = nslots >> 1;
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < npairs; idx += 256) {
                const int t = idx >> tsh, ct = idx & (TC - 1);
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const int olo = (lo << tsh) + ct, ohi = (hi << tsh) + ct;
                const double blo = s_b[olo], bhi = s_b[ohi];
                const unsigned ilo = s_i[olo], ihi = s_i[ohi];
                const bool up = (lo & kk) == 0;                    // this run ends with `lo` in front
                if (kgs_before(bhi, ihi, blo, ilo) == up) {
                    s_b[olo] = bhi; s_b[ohi] = blo;
                    s_i[olo] = (unsigned short)ihi; s_i[ohi] = (unsigned short)ilo;
                }
            }
            __syncthreads();
        }
    }
    // (the pads are the last P - n of every set: ranks 0 .. n-1 are the lines)
    for (int idx = tid; idx < n * TC; idx += 256) {
        const int k = idx >> tsh, ct = idx & (TC - 1), c = cbase + ct;
        if (c >= Mc || c0 + c >= M) continue;
        // (the work item's own tables: orow = Mc, oc0 = oh0 = 0; resident [H][n][Mp] ones: orow = Mp, oc0 = c0, oh0 = h0)
        const size_t o = ((size_t)(oh0 + h) * n + k) * orow + oc0 + c;
        bsort[o] = s_bad[ct] ? __builtin_nan("") : s_b[idx];
        perm[o] = s_i[idx];
    }
}

__global__ __launch_bounds__(256) void k_kgs_value(const double* __restrict__ bsort /*[nh][n][Mc]*/,
                                                   const unsigned short* __restrict__ perm /*[nh][n][Mc]*/,
                                                   const double* __restrict__ muc /*[nh][Mc]*/, const double* __restrict__ mua /*[nh][n - 1]*/,
                                                   int Mc, int n, int64_t c0, int64_t M, int64_t Mp, int h0, double* __restrict__ ei_draw)
{
#pragma clang fp contract(off)
    extern __shared__ double kgs_lds[];
    const int A = n - 1, nw = (n + 31) >> 5;
    double* s_mua = kgs_lds;                                       // [A]
    unsigned* s_stk = (unsigned*)(s_mua + A);                      // [nw][256]
    int* s_bad = (int*)(s_stk + (size_t)nw * 256);                 // an intercept of the draw's points is not finite
    const int tid = threadIdx.x, h = blockIdx.y;
    const int c = blockIdx.x * 256 + tid;
    if (tid == 0) *s_bad = 0;
    __syncthreads();
    for (int a = tid; a < A; a += 256) {
        const double v = mua[(size_t)h * A + a];
        if (!(fabs(v) <= KGS_DBL_MAX)) *s_bad = 1;
        s_mua[a] = v;
    }
    __syncthreads();
    if (c >= Mc || c0 + c >= M) return;
    const size_t o = (size_t)h * n * Mc + c;
    const double m0 = muc[(size_t)h * Mc + c];
    double v = __builtin_nan("");
    // (k_kgs_order wrote NaN over every slope of a candidate that had a non-finite one)
    if (!*s_bad && fabs(m0) <= KGS_DBL_MAX && fabs(bsort[o]) <= KGS_DBL_MAX) {
        KgsLines L;
        L.mu0 = m0;
        L.mua = s_mua; L.ms = 1;
        L.perm = perm + o; L.ps = (size_t)Mc;
        L.bsort = bsort + o; L.bs = (size_t)Mc;
        v = kgf_value(L, n, s_stk + tid, 256);
    }
    ei_draw[(size_t)(h0 + h) * Mp + c0 + c] = v;
}

// the slope order of a work item's (d, c) into tables of row stride orow, the work item at column oc0 of draw oh0 + h (the plain
// pass: its own [nh][n][Mc]; KG over fantasies, kg_fant_scan_kernels.hip: the resident [H][n][Mp])
void launch_kgs_order(hipStream_t s, const double* slope, int Mc, int nh, int n, int64_t c0, int64_t M, size_t orow, int64_t oc0, int oh0,
                      double* bsort, unsigned short* perm)
{
    const int P = kgs_pow2(n), TC = kgs_tile_candidates(P);
    hipLaunchKernelGGL(k_kgs_order, dim3((Mc + TC - 1) / TC, nh), dim3(256), (size_t)10 * P * TC + 4 * TC, s, slope, Mc, n, P, TC, c0, M,
                       orow, oc0, oh0, bsort, perm);
}

// slope / muc as launch_kg_lines left them for the work item, mua the draws' [nh][n - 1]; bsort / perm: nh n Mc entries each
void launch_kgs_value(hipStream_t s, const double* slope, const double* muc, const double* mua, int Mc, int nh, int n, int64_t c0,
                      int64_t M, int64_t Mp, int h0, double* bsort, unsigned short* perm, double* ei_draw)
{
    launch_kgs_order(s, slope, Mc, nh, n, c0, M, (size_t)Mc, 0, 0, bsort, perm);
    hipLaunchKernelGGL(k_kgs_value, dim3((Mc + 255) / 256, nh), dim3(256), (size_t)8 * (n - 1) + 1024 * (size_t)((n + 31) / 32) + 4, s,
                       bsort, perm, muc, mua, Mc, n, c0, M, Mp, h0, ei_draw);
}
