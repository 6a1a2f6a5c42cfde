// Knowledge gradient over the fantasies of pending jobs, the wide form (spx.h: option "kg_fantasies" = 2): kg_fant_kernels.hip's
// pass and kg_fant_device.h's rule, operation for operation, for n = A + 1 up to 1024 lines.  Upstream nothing changes -- k_kgf_mu,
// the S + A column GEMM branch, k_kgf_lines (grid.y = nh (S + A): the plan holds nh to 65535 / (S + A)) -- and k_kgf_mean closes
// the pass.  What differs:
//   order         k_kgs_order of kg_scan_kernels.hip (the bitonic network, 16-bit indices, -inf pads, NaN over the slopes of a
//                 candidate that has a non-finite one) writes the resident [H][n][Mp] tables through its output stride and
//                 offsets: 8 + 2 bytes per line.  Rank counting would be n^2 compare-selects and writes 8-bit indices.
//   k_kgw_cols    one thread per (d, s): is an intercept mu_a[.][s] not finite?  (k_kgf_value learns that while it stages mu_a.)
//   k_kgw_value   the hot one.  256 threads; a thread owns (candidate ct = tid / SB, fantasies sl = tid % SB, + SB, ...).
//     S > 32 (STAGED, SB = 64): a wave is ONE candidate, a lane a fantasy.  The candidate's sorted slopes and indices are staged
//       once per workgroup as [rank][4] (10 n bytes per candidate); their reads are LDS broadcasts.  All 64 lanes visit the same
//       rank in the same step outside a pop.
//     S <= 32 (SB = S rounded up to a power of two): a wave spans 64 / SB candidates at consecutive ct and reads slopes and
//       indices where the order kernel left them, [rank][c]: consecutive addresses, nothing staged.
//     mu_a is NOT staged: a block of 64 fantasies at A = 1023 would be 524 KB.  It lies as [H][A][S], s fastest, so the lanes of a
//       wave that visit rank k read 512 contiguous bytes of row perm[k]; per draw the table is 8 A S bytes (0.8 MB at A = 1023,
//       S = 100) and stays in L2.  The candidate's own intercept is read where k_kgf_lines left it (KgwLines, below).
//     The visit sequence does not depend on the data -- rank k is visited at step k -- so the lines of the NEXT KGW_PF ranks are
//       requested before the current KGW_PF are scanned (kgw_value) and a visit finds its intercept and slope in registers; only a
//       pop loads on demand, the new top and the line under it, rows that were read a few steps before.  kg_scan_kernels.hip
//       names the dependent load chain of a visit as what its scan waits for; this is the way round it.
//     Stacks: kgf_value's bit set in LDS as [word][thread].  KG_ds is written over mu_c (or into its own table with the moments
//       kept); a (d, s, c) is one thread's whatever the launcher's split, and nothing is combined afterwards but by k_kgf_mean.
//   Exact cases, the pending path's: all slopes equal: +0.0; no value negative; a non-finite slope or mu_c[s]: NaN for that (d, c)
//   alone; a non-finite mu_a[s]: NaN for the whole draw.
// LDS per workgroup (kgw_lds_bytes): 1024 ceil(n / 32) of stacks, + 40 n of lines when STAGED:
//     n = 65: 3.0 + 2.5 = 5.5 KB      n = 256: 8 + 10 = 18 KB      n = 1024: 32 + 40 = 72 KB     (not STAGED: 3, 8, 32 KB)
// Occupancy (profiles/kg_pending_scan_kernel_regs.txt): STAGED 161 VGPRs = 3 waves per SIMD = 3 workgroups per CU, which LDS allows
// up to n = 256; at n = 1024 two workgroups per CU (144 of 160 KB).  Not STAGED: 174 VGPRs, 2 waves per SIMD at every n.
// The launcher splits the fantasy blocks of a candidate group over several workgroups while the grid is below 2048 (k_kgf_value's
// rule).
// fp64-VALU bound, from the kernel as built (six division sites: the scan's test against the top, the new top's breakpoint after
// a pop, the term walk, three inside kg_f -- the rule's own count, kg_fant_kernels.hip derives it): per scan n + 2 P + E - 2 - d
// <= 3 n - 4 divisions and E - 1 evaluations of f; with a division at 16 fp64 issue slots, f at about 120 and 4 cycles per wave
// instruction a scan costs (n + 2 P + E) + 7.5 E cycles of one SIMD per lane.  E = 8:
//     n = 65 (P = 57): 247 cycles       n = 256: 820       n = 1024 (P = 1016): 3 124
//     M H S x 3 124 / (1024 SIMDs x 2.4 GHz):  C2 (20 000 x 10), S = 100, A = 1023: 25 ms;  S = 8: 2.0 ms
// The order adds P / 2 log2 P (log2 P + 1) / 2 compare-exchanges of two fp64 compares per (d, c), not per fantasy: 3 520 cycles at
// n = 1024, 1 % of the scans at S = 100.  What the count leaves out: the 12 32-bit selects that pick a visit's line out of the
// KGW_PF held ones, the address arithmetic and the two loads per visited line (the index, then the row), the bit-set updates, the
// divergence of the pop loop between the fantasies of a wave and around f, the pops' on-demand loads, and the strided 8-byte
// reads and writes of mu_c / KG_ds.  Measured (profiles/kg_pending_scan_time.jsonl, stage "kg"): 12 x the bound at C2, S = 100,
// A = 1023; 7 x at A = 255; 33 x at S = 8, A = 1023 (README, "KG over pending fantasies up to 1023 points").
// No atomics, no scratch.
#include "common.h"
#include "kg_fant_device.h"

#define KGW_DBL_MAX 1.79769313486231570815e308
#define KGW_PF 4               // ranks whose intercept and slope are in flight ahead of their visit
#define KGW_TC 4               // candidates of a staged workgroup: one per wave

// The lines by rank, KgfLinesOf's interface (kg_fant_device.h) for intercepts that lie in memory: mu_a as [A][S] and the
// candidate's own mu_c[s] where k_kgf_lines left it.  An intercept is ONE global load from one of two addresses, so that it can
// be issued ahead (a register copy of mu_c[s] under `p ? .. : ..` makes the compiler choose between a global address and one on
// the stack: a flat load and 16 bytes of scratch).  STAGED: slopes and indices in LDS as [rank][KGW_TC]; otherwise in memory as
// [rank][Mp].
template <bool STAGED>
struct KgwLines {
    const double* mu0;                                                 // &mu_c[d][s][c]
    const double* mua; int ms;
    const unsigned short* perm;
    const double* bsort;
    size_t rs;                                                         // (not STAGED: the row stride of perm and bsort)
    __device__ __forceinline__ size_t at(int k) const { return STAGED ? (size_t)k * KGW_TC : (size_t)k * rs; }
    __device__ __forceinline__ double m(int k) const
    {
        const int p = perm[at(k)];
        return *(p ? mua + (size_t)(p - 1) * ms : mu0);
    }
    __device__ __forceinline__ double b(int k) const { return bsort[at(k)]; }
};

// kgf_value of kg_fant_device.h, operation for operation, with the visit sequence's loads issued ahead: rank k is visited at step
// k whatever the data, so the lines of ranks k0 + KGW_PF .. k0 + 2 KGW_PF - 1 are requested before ranks k0 .. k0 + KGW_PF - 1
// are scanned and sit in registers when their turn comes.  Only a pop reads on demand (the new top and the line under it).
template <class Lines>
__device__ __forceinline__ double kgw_value(const Lines& L, int n, unsigned* stk, int ss)
{
#pragma clang fp contract(off)
    const int nw = (n + 31) >> 5;
    for (int w = 0; w < nw; ++w) stk[(size_t)w * ss] = 0u;
    int top = -1, under = -1;
    double mt = 0.0, bt = 0.0, zt = -SPX_KG_INF;
    double mq[KGW_PF], bq[KGW_PF];
#pragma unroll
    for (int j = 0; j < KGW_PF; ++j) {
        const int k = j < n ? j : n - 1;
        mq[j] = L.m(k); bq[j] = L.b(k);
    }
#pragma nounroll
    for (int k0 = 0; k0 < n; k0 += KGW_PF) {
        double mn[KGW_PF], bn[KGW_PF];
#pragma unroll
        for (int j = 0; j < KGW_PF; ++j) {                    // (beyond the last line: the last line again, never visited)
            const int k = k0 + KGW_PF + j < n ? k0 + KGW_PF + j : n - 1;
            mn[j] = L.m(k); bn[j] = L.b(k);
        }
#pragma nounroll
        for (int j = 0; j < KGW_PF; ++j) {                    // (one copy of the scan's body: the line is picked by selects)
            const int k = k0 + j;
            double mk = mq[0], bk = bq[0];
#pragma unroll
            for (int q = 1; q < KGW_PF; ++q) {
                mk = j == q ? mq[q] : mk;
                bk = j == q ? bq[q] : bk;
            }
            double z = -SPX_KG_INF;
            bool replace = top >= 0 && bk == bt;
            if (k < n && !(replace && !(mk < mt))) {
                while (top >= 0) {
                    if (!replace) {
                        z = (mk - mt) / (bt - bk);
                        if (under < 0 || z > zt) break;
                    }
                    replace = false;
                    stk[(size_t)(top >> 5) * ss] &= ~(1u << (top & 31));
                    top = under;
                    z = -SPX_KG_INF;
                    if (top >= 0) {
                        mt = L.m(top); bt = L.b(top);
                        under = kgf_below(stk, ss, top);
                        zt = under >= 0 ? (mt - L.m(under)) / (L.b(under) - bt) : -SPX_KG_INF;
                    }
                }
                under = top;
                zt = z;
                top = k; mt = mk; bt = bk;
                stk[(size_t)(k >> 5) * ss] |= 1u << (k & 31);
            }
        }
#pragma unroll
        for (int j = 0; j < KGW_PF; ++j) { mq[j] = mn[j]; bq[j] = bn[j]; }
    }
    return kgf_terms(L, n, stk, ss);
}

// one thread per (draw, fantasy): 1 where an intercept mu_a[.][s] of the draw's points is not finite (lanes read consecutive s)
__global__ __launch_bounds__(64) void k_kgw_cols(const double* __restrict__ mua /*[H][A][S]*/, int A, int S, int* __restrict__ badcol /*[H][S]*/)
{
    const int s = blockIdx.x * 64 + threadIdx.x, h = blockIdx.y;
    if (s >= S) return;
    int bad = 0;
    for (int a = 0; a < A; ++a)
        if (!(fabs(mua[((size_t)h * A + a) * S + s]) <= KGW_DBL_MAX)) bad = 1;
    badcol[(size_t)h * S + s] = bad;
}

// grid: (groups of 256 / SB candidates, runs of `sper` fantasies, draws).  A thread owns (ct = tid / SB, sl = tid % SB): one
// candidate of the group and the fantasies sl, sl + SB, ... of the run.  STAGED (SB = 64, a wave = one candidate): the
// group's sorted slopes and indices through LDS as [rank][KGW_TC]; otherwise they are read where k_kgs_order left them, [rank][c],
// consecutive ct at consecutive addresses.  val may be muc itself: a (d, s, c) is read and written by one thread.
template <bool STAGED>
__global__ __launch_bounds__(256) void k_kgw_value(const double* __restrict__ bsort /*[H][n][Mp]*/,
                                                   const unsigned short* __restrict__ perm /*[H][n][Mp]*/,
                                                   const double* __restrict__ mua /*[H][A][S]*/, const int* __restrict__ badcol /*[H][S]*/,
                                                   const double* muc /*[H][S][Mp]*/, double* val /*[H][S][Mp]*/, int n, int S, int SB,
                                                   int sper, int64_t M, int64_t Mp)
{
#pragma clang fp contract(off)
    extern __shared__ double kgw_lds[];
    const int A = n - 1, nw = (n + 31) >> 5;
    unsigned* s_stk = (unsigned*)kgw_lds;                              // [nw][256]
    double* s_bs = (double*)(s_stk + (size_t)nw * 256);               // STAGED: [n][KGW_TC]
    unsigned short* s_perm = (unsigned short*)(s_bs + (size_t)n * KGW_TC);   // STAGED: [n][KGW_TC]
    const int tid = threadIdx.x, h = blockIdx.z;
    const int TC = 256 / SB;                                           // (SB is a power of two; STAGED: SB = 64, TC = KGW_TC)
    const int sl = tid & (SB - 1), ct = tid / SB;
    const int s_begin = blockIdx.y * sper, s_end = s_begin + sper < S ? s_begin + sper : S;
    const int64_t cbase = (int64_t)blockIdx.x * TC, c = cbase + ct;
    const double* tab_b = bsort + (size_t)h * n * Mp;
    const unsigned short* tab_p = perm + (size_t)h * n * Mp;
    if (STAGED) {
        for (int idx = tid; idx < n * KGW_TC; idx += 256) {
            const int k = idx / KGW_TC, t = idx % KGW_TC;
            double b = 0.0;
            int p = k;
            if (cbase + t < M) {
                const size_t o = (size_t)k * Mp + cbase + t;
                b = tab_b[o];
                p = tab_p[o];
                if (p >= n) p = k;                                     // (cannot happen: k_kgs_order wrote an index below n)
            }
            s_bs[idx] = b;
            s_perm[idx] = (unsigned short)p;
        }
        __syncthreads();
    }
    if (c >= M) return;                                                // (behind the only barrier)
    // (k_kgs_order wrote NaN over every slope of a candidate that had a non-finite one)
    const bool slopes_ok = fabs(STAGED ? s_bs[ct] : tab_b[c]) <= KGW_DBL_MAX;
    for (int s = s_begin + sl; s < s_end; s += SB) {
        const size_t o = ((size_t)h * S + s) * Mp + c;
        const double m0 = muc[o];
        double v = __builtin_nan("");
        if (slopes_ok && !badcol[(size_t)h * S + s] && fabs(m0) <= KGW_DBL_MAX) {
            KgwLines<STAGED> L;
            L.mu0 = muc + o;                                           // (val[o], which may be muc[o], is written behind the scan)
            L.mua = mua + (size_t)h * A * S + s; L.ms = S;
            L.perm = STAGED ? s_perm + ct : tab_p + c;
            L.bsort = STAGED ? s_bs + ct : tab_b + c;
            L.rs = (size_t)Mp;
            v = kgw_value(L, n, s_stk + tid, 256);
        }
        val[o] = v;
    }
}

// the intercepts, the slopes and their order of a work item: k_kgf_lines as it is, then the bitonic network of kg_scan_kernels.hip
// into the resident tables
void launch_kgw_lines(hipStream_t s, const double* part_ss, const double* part_bgS, const double* htab, const double* Kac, int nrb,
                      int Mc, int nh, int S, int A, int Ap, int64_t c0, int64_t M, int64_t Mp, int h0, double* slope, double* muc,
                      double* fv, double* cov, double* bsort, unsigned short* perm)
{
    launch_kgf_lines_only(s, part_ss, part_bgS, htab, Kac, nrb, Mc, nh, S, A, Ap, c0, M, Mp, h0, slope, muc, fv, cov);
    launch_kgs_order(s, slope, Mc, nh, A + 1, c0, M, (size_t)Mp, c0, h0, bsort, perm);
}

size_t kgw_lds_bytes(int n, bool staged) { return (size_t)1024 * ((n + 31) / 32) + (staged ? (size_t)10 * n * KGW_TC : 0); }

void launch_kgw_value(hipStream_t s, const double* bsort, const unsigned short* perm, const double* mua, const double* muc, double* val,
                      int* badcol, int n, int S, int H, int64_t M, int64_t Mp, double* ei_draw)
{
    const bool staged = S > 32;
    int SB = 64;
    while (!staged && SB / 2 >= S) SB >>= 1;                           // S <= 32 rounded up to a power of two
    const int TC = 256 / SB;
    const int64_t ngroups = (M + TC - 1) / TC;
    // fantasies per workgroup: whole blocks of SB, as few workgroups per (draw, group) as fill the grid to 2048 (k_kgf_value's rule)
    const int nsb = (S + SB - 1) / SB;
    const int64_t want = (2048 + ngroups * H - 1) / (ngroups * H);
    int runs = (int)(want < 1 ? 1 : want > nsb ? nsb : want);
    const int sper = (nsb + runs - 1) / runs * SB;
    runs = (S + sper - 1) / sper;
    const unsigned gx = (unsigned)ngroups;
    const size_t lds = kgw_lds_bytes(n, staged);
    hipLaunchKernelGGL(k_kgw_cols, dim3((S + 63) / 64, H), dim3(64), 0, s, mua, n - 1, S, badcol);
    if (staged) {
        SPX_LDS_ATTR(k_kgw_value<true>, lds);
        hipLaunchKernelGGL(k_kgw_value<true>, dim3(gx, runs, H), dim3(256), lds, s, bsort, perm, mua, badcol, muc, val, n, S, SB, sper, M, Mp);
    } else {
        hipLaunchKernelGGL(k_kgw_value<false>, dim3(gx, runs, H), dim3(256), lds, s, bsort, perm, mua, badcol, muc, val, n, S, SB, sper, M, Mp);
    }
    launch_kgf_mean(s, val, S, H, M, Mp, ei_draw);
}
