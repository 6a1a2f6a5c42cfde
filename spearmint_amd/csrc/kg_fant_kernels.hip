// Knowledge gradient over the fantasies of pending jobs (spx.h: option "kg_fantasies") behind the pass's S > 0 GEMM branch with
// S + A right-hand sides per draw: columns 0 .. S-1 the held Gamma of the fantasies, columns S .. S+A-1 Gamma_a = L^-1 k(X, a) of
// the representer points.  Conditioned on the pending inputs the slopes of the n = A + 1 lines of (draw d, candidate c) are the
// same under every fantasy; only the intercepts move (kg_fant_device.h).  So:
//   k_kgf_mu      once per pass.  A wave owns one (d, a): it holds its share of Gamma_a in registers (rows lane, lane + 64, ...,
//                 KGF_MU_R of them: Np <= 1024) and walks the S columns of gamma against it, so Gamma_a is read once and not S
//                 times; a longer column is walked in k_kg_mu's order for four fantasies at a time (Gamma_a read S / 4 times).
//                 Per (a, s) the order of the sum is k_kg_mu's: lane i mod 64 takes row i, then the butterfly, then + mean.
//                 mu_a is kept as [H][A][S], s fastest: k_kgf_value stages a block of fantasies with coalesced reads.
//   k_kgf_lines   per work item, where k_kg_lines runs: one thread per (candidate, draw of the group, column) sums the partial
//                 sums over the row blocks in k_ei_fant_values' order.  Column s < S: mu_c[d][s][c], resident; column 0 also
//                 func_v[d][c] and the slope of line 0; column S + a: C(c, a) = Kac - bg, its slope, and C into cov when the
//                 moments are kept.  The arithmetic per element is k_kg_lines' / k_mes_fant_means'.
//   k_kgf_order   per work item, a launch of its own behind k_kgf_lines: the slope order of every (d, c) by rank counting in LDS
//                 (k_kg_value's tiling: TC = kg_tile_candidates(n) candidates, slopes as [line][candidate]); work item (line i,
//                 candidate ct) counts the lines that precede it -- n compare-selects, no division -- and writes its slope and
//                 its index to the resident [d][rank][c] tables (8 + 1 bytes per line).  It is not fused into the head of
//                 k_kgf_value because that kernel's workgroups may share a tile (the fantasies of a tile are split over
//                 several when the grid is small) and would each count again; per work item it reads the slopes where
//                 k_kgf_lines left them, and the scan needs no unsorted slopes at all.  A candidate with a non-finite slope keeps
//                 the order of the lines (its ranks would collide): k_kgf_value sees the slope and writes NaN.
//   k_kgf_value   the hot one, behind the last chunk: see below.
//   k_kgf_mean    one thread per (d, c): the mean of KG_ds(c) over s in numpy's pairwise order (np_sum.h), into ei_draw.
// k_kgf_value.  A workgroup of 256 threads owns TC candidates of one draw and a run of fantasies, which it walks in blocks of SB;
// a thread owns one (ct, s) of the block, fantasies fastest (sl = tid % SB, ct = tid / SB).  Staged once per workgroup: the
// sorted slopes and the permutation of its candidates as [rank][ct].  Staged once per block: mu_a[s] as [a][SB + 1].  The thread
// reads its mu_c[s] into a register and runs kgf_value of kg_fant_device.h: the scan, its stack a bit set in LDS as
// [word][thread] (lanes of a wave touch consecutive words), the top's intercept, slope and breakpoint in registers, then one walk
// over the stack for the terms.  With SB = 64 a wave is one candidate: its slope and permutation reads are broadcasts, its mu_a
// reads consecutive, and its lanes scan lines of one slope order.  With a smaller SB a wave spans 64 / SB candidates at
// consecutive ct: consecutive words again.
// KG_ds(c) is written where mu_c[d][s][c] was read (or, with the moments kept, into a table of its own, so that mu_c stays for
// spx_get_kg_fantasy_lines) and k_kgf_mean reads it back: 16 bytes of traffic per scan of several hundred fp64 instructions, and
// the mean then depends on S alone -- not on SB, TC or how the launcher split the fantasies -- by construction, without a
// cross-lane tree that has to mimic numpy's eight accumulators.
// LDS per workgroup (kgf_lds_bytes): 8 n TC (slopes) + 8 A (SB + 1) (mu_a) + 4 ceil(n / 32) 256 (stacks) + n TC (permutation)
// + 4 (TC + SB) (flags), held to 64 KB so that two workgroups fit a CU's 160 KB at any n.  kgf_tile picks, among SB = 64, 32, ..,
// 1 (no larger than S rounded up to a power of two) and the largest TC <= 256 / SB that fits, the pair with the most busy
// threads, the larger SB on a tie.  n = 65, S >= 64: SB = 64, TC = 4, 2.1 + 33.3 + 3.1 + 0.3 = 38.8 KB: four workgroups per CU by LDS, three by registers.
// n = 256: mu_a at SB = 64 alone is 132 KB, so SB = 16, TC = 8: 16.4 + 34.7 + 8.2 + 2.0 = 61.4 KB with 128 busy threads.
// When H ceil(M / TC) leaves CUs idle the launcher splits the fantasy blocks of a tile over several workgroups (2048 wanted);
// nothing is combined afterwards, a (d, s, c) is one thread's whatever the split.
// fp64-VALU bound, from the kernel as built (profiles/kg_pending_kernel_regs.txt: three division sites of the scan and the walk,
// three more inside kg_f).  Per scan of n lines, d of them dropped for an equal slope, E left on the envelope, P = n - d - E
// popped: one division per visited line against the top (n - 1 - d), one more per pop for the next top's test and one for the
// new top's own breakpoint (2 P), one per term (E - 1) -- n + 2 P + E - 2 - d <= 3 n - 4 divisions -- and E - 1 evaluations of f.
// With kg_kernels.hip's prices (a division 16 fp64 issue slots, f about 120, 4 cycles per wave instruction of 64 lanes) a scan
// costs (n + 2 P + E) + 7.5 E cycles of one SIMD per lane; at n = 65 and E = 8 (P = 57): 247 cycles, so
//     M H S x 247 / (1024 SIMDs x 2.4 GHz) = M H S / 9.9e9 s:  C2 (20 000 x 10) at S = 100: 2.0 ms, C3 (200 000 x 20): 40 ms
// -- the all-pairs rule per fantasy would be S x n^2 = 4225 cycles per (d, c, s), 17 times that.  What the count leaves out: the
// LDS reads of a step (permutation, intercept, slope; two more per pop for the line under the top), the bit-set updates, the
// divergence of the pop loop between the fantasies of a wave and around f, 135 VGPRs = 3 waves per SIMD to hide the LDS latency
// of a dependent chain, and the strided 8-byte reads and writes of mu_c / KG_ds.  k_kgf_order adds n^2 compare-selects per (d, c),
// not per fantasy.  Measured: README, "KG while jobs are pending".
// No atomics, no scratch.
#include "common.h"
#include "kg_fant_device.h"
#include "np_sum.h"

#define KGF_SLOTS 2048         // (line, candidate) pairs of a k_kgf_order tile: KG_SLOTS of kg_kernels.hip
#define KGF_MU_R 16            // rows of Gamma_a a lane of k_kgf_mu holds in registers
#define KGF_LDS_MAX 65536
#define KGF_DBL_MAX 1.79769313486231570815e308

__global__ __launch_bounds__(64) void k_kgf_mu(const double* __restrict__ gammaS /*[H][S + A][Np]*/, const double* __restrict__ htab,
                                               int Np, int S, int A, double* __restrict__ mua /*[H][A][S]*/)
{
#pragma clang fp contract(off)
    const int a = blockIdx.x, d = blockIdx.y, lane = threadIdx.x;
    const double* g0 = gammaS + (size_t)d * (S + A) * Np;
    const double* ga = g0 + (size_t)(S + a) * Np;
    const double mean = htab[d * SPX_HT + 0];
    double* out = mua + ((size_t)d * A + a) * S;
    if (Np <= 64 * KGF_MU_R) {
        double g[KGF_MU_R];
#pragma unroll
        for (int r = 0; r < KGF_MU_R; ++r) {
            const int i = lane + 64 * r;
            g[r] = i < Np ? ga[i] : 0.0;
        }
        for (int s = 0; s < S; ++s) {
            const double* gs = g0 + (size_t)s * Np;
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < KGF_MU_R; ++r) {
                const int i = lane + 64 * r;
                if (i < Np) acc = acc + g[r] * gs[i];
            }
            for (int m = 32; m > 0; m >>= 1) acc = acc + __shfl_xor(acc, m);
            if (lane == 0) out[s] = acc + mean;
        }
    } else {
        for (int s0 = 0; s0 < S; s0 += 4) {
            const int s1 = s0 + 1 < S ? s0 + 1 : s0, s2 = s0 + 2 < S ? s0 + 2 : s0, s3 = s0 + 3 < S ? s0 + 3 : s0;
            const double *q0 = g0 + (size_t)s0 * Np, *q1 = g0 + (size_t)s1 * Np, *q2 = g0 + (size_t)s2 * Np, *q3 = g0 + (size_t)s3 * Np;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int i = lane; i < Np; i += 64) {
                const double gi = ga[i];
                a0 = a0 + gi * q0[i];
                a1 = a1 + gi * q1[i];
                a2 = a2 + gi * q2[i];
                a3 = a3 + gi * q3[i];
            }
            for (int m = 32; m > 0; m >>= 1) {
                a0 = a0 + __shfl_xor(a0, m);
                a1 = a1 + __shfl_xor(a1, m);
                a2 = a2 + __shfl_xor(a2, m);
                a3 = a3 + __shfl_xor(a3, m);
            }
            if (lane == 0) {
                out[s0] = a0 + mean;
                if (s0 + 1 < S) out[s0 + 1] = a1 + mean;
                if (s0 + 2 < S) out[s0 + 2] = a2 + mean;
                if (s0 + 3 < S) out[s0 + 3] = a3 + mean;
            }
        }
    }
}

void launch_kgf_mu(hipStream_t s, const double* gammaS, const double* htab, int Np, int S, int A, int H, double* mua)
{
    hipLaunchKernelGGL(k_kgf_mu, dim3(A, H), dim3(64), 0, s, gammaS, htab, Np, S, A, mua);
}

// columns: St = S + A per draw; slope [nh][A + 1][Mc] of the work item; muc [H][S][Mp], fv [H][Mp], cov [H][A][Mp] or null
__global__ __launch_bounds__(256) void k_kgf_lines(const double* __restrict__ part_ss, const double* __restrict__ part_bgS,
                                                   const double* __restrict__ htab, const double* __restrict__ Kac /*[nh][Ap][Mc]*/,
                                                   int nrb, int Mc, int nh, int S, int A, int Ap, int64_t c0, int64_t M, int64_t Mp,
                                                   int h0, double* __restrict__ slope, double* __restrict__ muc, double* __restrict__ fv,
                                                   double* __restrict__ cov)
{
#pragma clang fp contract(off)
    const int St = S + A, n = A + 1;
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y / St, col = blockIdx.y - h * St;
    if (c >= Mc || c0 + c >= M) return;
    double bg = 0.0;
    for (int ib = 0; ib < nrb; ++ib) {
        const size_t o0 = ((((size_t)ib * 2 + 0) * nh + h) * St + col) * Mc + c;
        const size_t o1 = ((((size_t)ib * 2 + 1) * nh + h) * St + col) * Mc + c;
        bg += part_bgS[o0] + part_bgS[o1];
    }
    if (col < S) muc[((size_t)(h0 + h) * S + col) * Mp + c0 + c] = bg + htab[h * SPX_HT + 0];
    if (col > 0 && col < S) return;
    double ss = 0.0;
    for (int ib = 0; ib < nrb; ++ib) ss += part_ss[((size_t)ib * nh + h) * Mc + c];
    const double func_v = htab[h * SPX_HT + 3] - ss;
    const double vs = func_v + htab[h * SPX_HT + 1];      // the variance of a new observation at c
    const double sc = sqrt(vs);
    double sl;
    int line;
    if (col == 0) {
        fv[(size_t)(h0 + h) * Mp + c0 + c] = func_v;
        sl = func_v / sc;
        line = 0;
    } else {
        const int a = col - S;
        const double C = Kac[((size_t)h * Ap + a) * Mc + c] - bg;
        sl = C / sc;
        line = a + 1;
        if (cov) cov[((size_t)(h0 + h) * A + a) * Mp + c0 + c] = C;
    }
    slope[((size_t)h * n + line) * Mc + c] = (vs > 0.0) ? sl : __builtin_nan("");
}

__global__ __launch_bounds__(256) void k_kgf_order(const double* __restrict__ slope /*[nh][n][Mc]*/, int Mc, int n, int TC, int64_t c0,
                                                   int64_t M, int64_t Mp, int h0, double* __restrict__ bsort /*[H][n][Mp]*/,
                                                   unsigned char* __restrict__ perm /*[H][n][Mp]*/)
{
    __shared__ double s_b[KGF_SLOTS];
    __shared__ int s_bad[256];
    const int tid = threadIdx.x, h = blockIdx.y;
    const int cbase = blockIdx.x * TC;
    if (cbase >= Mc || c0 + cbase >= M) return;            // (the whole workgroup: before any barrier)
    const int nslots = n * TC;                             // <= KGF_SLOTS
    const int tsh = 31 - __builtin_clz(TC);                // (TC is a power of two)
    s_bad[tid] = 0;
    for (int idx = tid; idx < nslots; idx += 256) {
        const int i = idx >> tsh, ct = idx & (TC - 1), c = cbase + ct;
        s_b[idx] = (c < Mc && c0 + c < M) ? slope[((size_t)h * n + i) * Mc + c] : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < nslots; idx += 256)
        if (!(fabs(s_b[idx]) <= KGF_DBL_MAX)) s_bad[idx & (TC - 1)] = 1;
    __syncthreads();
    for (int idx = tid; idx < nslots; idx += 256) {
        const int i = idx >> tsh, ct = idx & (TC - 1), c = cbase + ct;
        if (c >= Mc || c0 + c >= M) continue;
        const int r = s_bad[ct] ? i : kgf_rank(s_b + ct, TC, n, i);
        const size_t o = ((size_t)(h0 + h) * n + r) * Mp + c0 + c;
        bsort[o] = s_b[idx];
        perm[o] = (unsigned char)i;
    }
}

// k_kgf_lines alone (kg_fant_scan_kernels.hip orders the slopes it leaves with a kernel of its own)
void launch_kgf_lines_only(hipStream_t s, const double* part_ss, const double* part_bgS, const double* htab, const double* Kac, int nrb,
                           int Mc, int nh, int S, int A, int Ap, int64_t c0, int64_t M, int64_t Mp, int h0, double* slope, double* muc,
                           double* fv, double* cov)
{
    hipLaunchKernelGGL(k_kgf_lines, dim3((Mc + 255) / 256, nh * (S + A)), dim3(256), 0, s, part_ss, part_bgS, htab, Kac, nrb, Mc, nh, S, A,
                       Ap, c0, M, Mp, h0, slope, muc, fv, cov);
}

void launch_kgf_lines(hipStream_t s, const double* part_ss, const double* part_bgS, const double* htab, const double* Kac, int nrb,
                      int Mc, int nh, int S, int A, int Ap, int64_t c0, int64_t M, int64_t Mp, int h0, double* slope, double* muc,
                      double* fv, double* cov, double* bsort, unsigned char* perm)
{
    const int n = A + 1, TC = kg_tile_candidates(n);
    launch_kgf_lines_only(s, part_ss, part_bgS, htab, Kac, nrb, Mc, nh, S, A, Ap, c0, M, Mp, h0, slope, muc, fv, cov);
    hipLaunchKernelGGL(k_kgf_order, dim3((Mc + TC - 1) / TC, nh), dim3(256), 0, s, slope, Mc, n, TC, c0, M, Mp, h0, bsort, perm);
}

// dynamic LDS of a k_kgf_value workgroup; the kernel lays it out in this order
size_t kgf_lds_bytes(int n, int TC, int SB)
{
    const size_t nw = (size_t)(n + 31) / 32;
    return (size_t)8 * n * TC + (size_t)8 * (n - 1) * (SB + 1) + 4 * nw * 256 + (size_t)4 * (TC + SB) + (size_t)n * TC;
}

void kgf_tile(int n, int S, int* TC, int* SB)
{
    int best = 0;
    *TC = 1; *SB = 1;
    for (int sb = 64; sb >= 1; sb >>= 1) {
        if (sb > 1 && sb / 2 >= S) continue;               // no larger than S rounded up to a power of two
        int tc = 256 / sb;
        while (tc >= 1 && kgf_lds_bytes(n, tc, sb) > KGF_LDS_MAX) tc >>= 1;
        if (tc >= 1 && tc * sb > best) { best = tc * sb; *TC = tc; *SB = sb; }
    }
}

// grid: (tiles of TC candidates, runs of `sper` fantasies, draws).  val may be muc itself: a (d, s, c) is read and written by one thread.
__global__ __launch_bounds__(256) void k_kgf_value(const double* __restrict__ bsort /*[H][n][Mp]*/,
                                                   const unsigned char* __restrict__ perm /*[H][n][Mp]*/,
                                                   const double* __restrict__ mua /*[H][A][S]*/, const double* muc /*[H][S][Mp]*/,
                                                   double* val /*[H][S][Mp]*/, int n, int S, int TC, int SB, int sper, int64_t M,
                                                   int64_t Mp)
{
#pragma clang fp contract(off)
    extern __shared__ double kgf_lds[];
    const int A = n - 1, nw = (n + 31) >> 5;
    double* s_bs = kgf_lds;                                // [n][TC]
    double* s_mua = s_bs + (size_t)n * TC;                 // [A][SB + 1]
    unsigned* s_stk = (unsigned*)(s_mua + (size_t)A * (SB + 1));   // [nw][256]
    int* s_bad = (int*)(s_stk + (size_t)nw * 256);         // [TC]: a slope of the candidate is not finite
    int* s_badcol = s_bad + TC;                            // [SB]: an intercept of the fantasy is not finite
    unsigned char* s_perm = (unsigned char*)(s_badcol + SB);       // [n][TC]
    const int tid = threadIdx.x, h = blockIdx.z;
    const int sl = tid & (SB - 1), ct = tid / SB;          // (SB is a power of two)
    const int64_t cbase = (int64_t)blockIdx.x * TC;
    const int64_t c = cbase + ct;
    const bool live = ct < TC && c < M;
    const int s_begin = blockIdx.y * sper, s_end = s_begin + sper < S ? s_begin + sper : S;
    const int tsh = 31 - __builtin_clz(TC);                // (TC is a power of two)
    if (tid < TC) s_bad[tid] = 0;
    __syncthreads();
    for (int idx = tid; idx < n * TC; idx += 256) {
        const int k = idx >> tsh, t = idx & (TC - 1);
        double b = 0.0;
        int p = k;
        if (cbase + t < M) {
            const size_t o = ((size_t)h * n + k) * Mp + cbase + t;
            b = bsort[o];
            p = perm[o];
            if (!(fabs(b) <= KGF_DBL_MAX)) s_bad[t] = 1;
            if (p >= n) p = k;                             // (cannot happen: k_kgf_order wrote an index below n)
        }
        s_bs[idx] = b;
        s_perm[idx] = (unsigned char)p;
    }
    for (int s0 = s_begin; s0 < s_end; s0 += SB) {
        const int sn = s_end - s0 < SB ? s_end - s0 : SB;
        __syncthreads();       // the block before this one has been read (first block: the staging above is complete)
        if (tid < SB) s_badcol[tid] = 0;
        __syncthreads();
        for (int idx = tid; idx < A * SB; idx += 256) {
            const int a = idx / SB, q = idx & (SB - 1);
            double v = 0.0;
            if (q < sn) {
                v = mua[((size_t)h * A + a) * S + s0 + q];
                if (!(fabs(v) <= KGF_DBL_MAX)) s_badcol[q] = 1;
            }
            s_mua[(size_t)a * (SB + 1) + q] = v;
        }
        __syncthreads();
        if (live && sl < sn) {
            const size_t o = ((size_t)h * S + s0 + sl) * Mp + c;
            const double m0 = muc[o];
            double v = __builtin_nan("");
            if (!s_bad[ct] && !s_badcol[sl] && fabs(m0) <= KGF_DBL_MAX) {
                KgfLines L;
                L.mu0 = m0;
                L.mua = s_mua + sl; L.ms = SB + 1;
                L.perm = s_perm + ct; L.ps = TC;
                L.bsort = s_bs + ct; L.bs = TC;
                v = kgf_value(L, n, s_stk + tid, 256);
            }
            val[o] = v;
        }
    }
}

// one thread per (candidate, draw); pad columns c >= M are not written
__global__ __launch_bounds__(256) void k_kgf_mean(const double* __restrict__ val /*[H][S][Mp]*/, int S, double* __restrict__ ei_draw,
                                                  int64_t M, int64_t Mp)
{
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y;
    if (c >= M) return;
    const double res = np_pairwise(val + (size_t)h * S * Mp + c, Mp, S);
    ei_draw[(size_t)h * Mp + c] = (0.0 + res) / (double)S;
}

void launch_kgf_mean(hipStream_t s, const double* val, int S, int H, int64_t M, int64_t Mp, double* ei_draw)
{
    hipLaunchKernelGGL(k_kgf_mean, dim3((unsigned)((M + 255) / 256), H), dim3(256), 0, s, val, S, ei_draw, M, Mp);
}

void launch_kgf_value(hipStream_t s, const double* bsort, const unsigned char* perm, const double* mua, const double* muc, double* val,
                      int n, int S, int H, int64_t M, int64_t Mp, double* ei_draw)
{
    int TC = 1, SB = 1;
    kgf_tile(n, S, &TC, &SB);
    const int64_t ntiles = (M + TC - 1) / TC;
    // fantasies per workgroup: whole blocks of SB, as few workgroups per (draw, tile) as fill the grid to 2048
    const int nsb = (S + SB - 1) / SB;
    int64_t want = (2048 + ntiles * H - 1) / (ntiles * H);
    int runs = (int)(want < 1 ? 1 : want > nsb ? nsb : want);
    const int sper = (nsb + runs - 1) / runs * SB;
    runs = (S + sper - 1) / sper;
    hipLaunchKernelGGL(k_kgf_value, dim3((unsigned)ntiles, runs, H), dim3(256), kgf_lds_bytes(n, TC, SB), s, bsort, perm, mua, muc, val,
                       n, S, TC, SB, sper, M, Mp);
    launch_kgf_mean(s, val, S, H, M, Mp, ei_draw);
}
