// Knowledge gradient over the fantasies of pending jobs (spx.h: option "kg_fantasies"): the value of kg_device.h,
//     KG = sum_k (b_k - b_{k+1}) f(-|z_k|) over the lower envelope of the n lines mu_i + b_i Z in order of falling slope,
// for line sets that share their SLOPES and differ in their intercepts alone -- conditioned on the pending inputs every posterior
// covariance of (draw, candidate) is the same under every fantasy, only the means move.  So the slope order is found once per
// (draw, candidate) and each fantasy runs the linear stack scan over the lines in that order (Frazier, Powell & Dayanik 2009,
// algorithm 1): about 3 n divisions per line set where the all-pairs rule of kg_device.h spends n^2.
//
// The rule of this path, operation for operation:
//   order   kgf_rank(i) = the number of lines j that precede line i: b_j > b_i, or b_j == b_i and j < i (slope falling, ties by
//           rising index; n compare-selects, no division).  perm[rank] = i, bs[rank] = b_i.  The slopes must be finite.
//   scan    the lines are visited by rising rank k; (m_k, b_k) is the visited line, (m_t, b_t) the top of the stack, z_t the
//           breakpoint between the top and the line under it (-inf while the stack holds one line).
//             1. empty stack: push k.
//             2. b_k == b_t: the line is dropped unless m_k < m_t (strictly: lowest intercept, then lowest index -- today's tie
//                rule); then the top is popped and k goes on with 3 against the new top (or 1).
//             3. z = (m_k - m_t) / (b_t - b_k): ONE expression per breakpoint, the later line's intercept first.  While the stack
//                holds more than one line and z <= z_t, the top is popped -- z_t of the new top is recomputed by the same
//                expression from the line under it, no breakpoint is stored -- and 3 is repeated.  Then k is pushed, z_t = z.
//           The first line of the largest slope that survives 2 is never popped: it is the envelope at Z -> -inf.
//   terms   the stack from bottom to top is the envelope in order of falling slope.  For every line j but the last, with k the
//           next: db = b_j - b_k, z = (m_k - m_j) / db -- the scan's expression again, same bits -- term = db kg_f(z), kg_f of
//           kg_device.h unchanged; the terms are added in that order from +0.0.
// All slopes equal: one line stays, no term, +0.0 exactly.  Every term is >= 0, so no value is negative.  A line that touches the
// envelope in one point is off it here (z <= z_t pops) as it is in kg_device.h; where a rounding of a breakpoint decides, the two
// rules may keep different lines, and the values differ by that rounding, not by a term.
// The stack is a bit set over the ranks: pushes come in rising rank, so the stack's order is the ranks' order, its top the highest
// set bit, the line under a line the next lower set bit (kgf_below).  n / 8 bytes per scan instead of n: at n = 256 a workgroup
// of 256 scans needs 8 KB where a byte per depth would need 64 KB.  The words are strided (ss) so that the lanes of a wave touch
// consecutive words of LDS.
// Non-finite intercepts or slopes: the caller's business (k_kgf_value writes NaN); the functions here expect finite lines.
// SPX_KG_HOST: the same text compiled for the host (tests/c/kgf_client.cpp, built with -ffp-contract=off).
#pragma once
#include "kg_device.h"

// lines that precede line i; b[j * bs] the slope of line j
__device__ __forceinline__ int kgf_rank(const double* b, int bs, int n, int i)
{
    const double bi = b[(size_t)i * bs];
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const double bj = b[(size_t)j * bs];
        r += (bj > bi || (bj == bi && j < i)) ? 1 : 0;
    }
    return r;
}

// the highest rank below k on the stack, -1 when there is none
__device__ __forceinline__ int kgf_below(const unsigned* stk, int ss, int k)
{
    int w = k >> 5;
    unsigned m = stk[(size_t)w * ss] & ((1u << (k & 31)) - 1u);
    while (m == 0u && w > 0) {
        --w;
        m = stk[(size_t)w * ss];
    }
    return m ? (w << 5) + 31 - __builtin_clz(m) : -1;
}

// Lines by rank k: index p = perm[k * ps] (0: the candidate, a >= 1: representer point a - 1), intercept p ? mua[(p - 1) * ms] : mu0,
// slope bsort[k * bs].  stk: (n + 31) / 32 words at stride ss, the scan's own.  The index type is the caller's: a byte holds
// n <= 256 (KgfLines, the pending path), 16 bits n <= 65536 (KgsLines: option "kg_scan", kg_scan_kernels.hip); the strides are
// size_t there because its tables live in memory, a chunk of candidates apart.  kgf_value is the same text for every such type.
template <class Index, class Stride>
struct KgfLinesOf {
    double mu0;
    const double* mua; int ms;
    const Index* perm; Stride ps;
    const double* bsort; Stride bs;
    __device__ __forceinline__ double m(int k) const
    {
        const int p = perm[(size_t)k * ps];
        return p ? mua[(size_t)(p - 1) * ms] : mu0;
    }
    __device__ __forceinline__ double b(int k) const { return bsort[(size_t)k * bs]; }
};
typedef KgfLinesOf<unsigned char, int> KgfLines;
typedef KgfLinesOf<unsigned short, size_t> KgsLines;

// the terms of the envelope a scan left on the stack, from bottom to top (shared by kgf_value and kg_fant_scan_kernels.hip's scan)
template <class Lines>
__device__ __forceinline__ double kgf_terms(const Lines& L, int n, const unsigned* stk, int ss)
{
#pragma clang fp contract(off)
    const int nw = (n + 31) >> 5;
    double acc = 0.0, mj = 0.0, bj = 0.0;
    bool first = true;
    for (int w = 0; w < nw; ++w) {
        unsigned m = stk[(size_t)w * ss];
        while (m) {
            const int k = (w << 5) + __builtin_ctz(m);
            m &= m - 1u;
            const double mk = L.m(k), bk = L.b(k);
            if (!first) {
                const double db = bj - bk;
                acc = acc + db * kg_f((mk - mj) / db);
            }
            first = false;
            mj = mk; bj = bk;
        }
    }
    return acc;
}

template <class Lines>
__device__ __forceinline__ double kgf_value(const Lines& L, int n, unsigned* stk, int ss)
{
#pragma clang fp contract(off)
    const int nw = (n + 31) >> 5;
    for (int w = 0; w < nw; ++w) stk[(size_t)w * ss] = 0u;
    int top = -1, under = -1;
    double mt = 0.0, bt = 0.0, zt = -SPX_KG_INF;
    for (int k = 0; k < n; ++k) {
        const double mk = L.m(k), bk = L.b(k);
        double z = -SPX_KG_INF;
        bool replace = top >= 0 && bk == bt;
        if (replace && !(mk < mt)) continue;
        while (top >= 0) {
            if (!replace) {
                z = (mk - mt) / (bt - bk);
                if (under < 0 || z > zt) break;
            }
            replace = false;
            // pop: the top goes, the line under it is the top, its breakpoint against the line under IT is formed again
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
    return kgf_terms(L, n, stk, ss);
}
